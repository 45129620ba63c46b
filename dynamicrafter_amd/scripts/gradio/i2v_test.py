"""The class behind the reference's public demo (scripts/gradio/i2v_test.py): one image in memory and a prompt in, one clip
file out. The web UI around it (gradio_app.py) is not part of this package and nothing here imports `gradio`.

    Image2Video(result_dir, gpu_num, resolution).get_image(image, prompt, steps, cfg_scale, eta, fs, seed) -> path

Differences from the reference, all at the edges:
  * the constructor downloads nothing: pass `ckpt_path=` (and optionally `config=`, default this package's
    configs/inference_<width>_v1.0.yaml) or a ready `model=`; `download_model()` raises;
  * one model is held whatever `gpu_num` says (the reference builds `gpu_num` copies and uses the first), and it stays on its
    device between calls (no model.cuda() / model.cpu() shuffling);
  * the image is resized on the device by HIP launches (ops.resize_f32: torchvision's Resize / CenterCrop on a float tensor);
  * the clip is written by this package's encoders, so the extension follows `container` (.avi by default, not .mp4);
  * `get_image(..., **sample_kwargs)` hands extra keyword arguments to `batch_ddim_sampling` (`x_T`, `noises`, `use_graph`, ...).
"""
import os
import time

import numpy as np
import torch

from ..evaluation.funcs import batch_ddim_sampling, get_latent_z, load_model_checkpoint, save_videos
from ..evaluation.inference import resize_center_crop_f32, seed_everything

CONFIG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "configs")


def parse_resolution(resolution):
    """'320_512' -> (320, 512): height, width."""
    return int(resolution.split("_")[0]), int(resolution.split("_")[1])


def load_model(resolution, ckpt_path, config=None, device=None):
    """What the reference's constructors do after their download (i2v_test.py:21-33): the YAML of the resolution's width (or
    `config`, a path) -> LatentVisualDiffusion with use_checkpoint off -> load_model_checkpoint -> eval, on `device` (default:
    the current HIP device)."""
    import yaml
    from ...utils.utils import instantiate_from_config
    if config is None:
        config = os.path.join(CONFIG_DIR, f"inference_{resolution[1]}_v1.0.yaml")
    with open(config) as f:
        cfg = yaml.safe_load(f)
    model_config = cfg.pop("model", {})
    model_config["params"]["unet_config"]["params"]["use_checkpoint"] = False
    model = instantiate_from_config(model_config)
    assert os.path.exists(ckpt_path), "Error: checkpoint Not Found!"
    model = load_model_checkpoint(model, ckpt_path)
    model.eval()
    return model.to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)


def prompt_to_filename(prompt):
    """i2v_test.py:83-87: '/' -> '_slash_', ' ' -> '_', the first 40 characters, 'empty_prompt' for the empty prompt."""
    prompt_str = prompt.replace("/", "_slash_") if "/" in prompt else prompt
    prompt_str = prompt_str.replace(" ", "_") if " " in prompt else prompt_str
    prompt_str = prompt_str[:40]
    if len(prompt_str) == 0:
        prompt_str = "empty_prompt"
    return prompt_str


class Image2Video:
    def __init__(self, result_dir="./tmp/", gpu_num=1, resolution="256_256", *, ckpt_path=None, config=None, model=None,
                 container="avi"):
        self.resolution = parse_resolution(resolution)                       # hw
        self.result_dir = result_dir
        self.container = container
        if model is None:
            if ckpt_path is None:
                self.download_model()
            model = load_model(self.resolution, ckpt_path, config)
        if not os.path.exists(self.result_dir):
            os.mkdir(self.result_dir)
        self.model_list = [model]
        self.save_fps = 8

    def download_model(self):
        """The reference fetches model.ckpt from the hub here (i2v_test.py:94-102). This package never reaches out."""
        raise RuntimeError(f"{type(self).__name__} does not download weights: pass ckpt_path= (a DynamiCrafter model.ckpt for "
                           f"{self.resolution[0]}x{self.resolution[1]}) or a ready model=")

    def _image_tensor(self, image, device):
        """uint8 [H, W, 3] ndarray -> fp32 [3, H, W] in [-1, 1] on the device (i2v_test.py:62-63)."""
        img = torch.from_numpy(np.array(image)).to(device).permute(2, 0, 1).float().contiguous()
        return (img / 255. - 0.5) * 2

    def _concat_cond(self, z, z2, frames):
        """The c_concat latent [b, c, frames, h, w] from the image latent z [b, c, 1, h, w]: z on every frame (i2v_test.py:70)."""
        return z.repeat(1, 1, frames, 1, 1)

    def _generate(self, image, prompt, steps, cfg_scale, eta, fs, seed, image2=None, drop_last=False, **sample_kwargs):
        seed_everything(seed)
        print("start:", prompt, time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(time.time())))
        start = time.time()
        if steps > 60:
            steps = 60
        model = self.model_list[0]
        batch_size = 1
        channels = model.model.diffusion_model.out_channels
        frames = model.temporal_length
        h, w = self.resolution[0] // 8, self.resolution[1] // 8
        noise_shape = [batch_size, channels, frames, h, w]

        with torch.no_grad():
            text_emb = model.get_learned_conditioning([prompt])

            img_tensor = self._image_tensor(image, model.device)
            videos = resize_center_crop_f32(img_tensor, self.resolution).unsqueeze(0)          # b c h w
            z = get_latent_z(model, videos.unsqueeze(2))                                       # b c 1 h w
            z2 = None
            if image2 is not None:
                videos2 = resize_center_crop_f32(self._image_tensor(image2, model.device), self.resolution).unsqueeze(0)
                z2 = get_latent_z(model, videos2.unsqueeze(2))
            img_tensor_repeat = self._concat_cond(z, z2, frames)

            cond_images = model.embedder(img_tensor.unsqueeze(0))              # the UNRESIZED image, as the reference (:72)
            img_emb = model.image_proj_model(cond_images)
            imtext_cond = torch.cat([text_emb, img_emb], dim=1)

            fs = torch.tensor([fs], dtype=torch.long, device=model.device)
            cond = {"c_crossattn": [imtext_cond], "fs": fs, "c_concat": [img_tensor_repeat]}

            batch_samples = batch_ddim_sampling(model, cond, noise_shape, n_samples=1, ddim_steps=steps, ddim_eta=eta,
                                                cfg_scale=cfg_scale, **sample_kwargs)
            if drop_last:
                batch_samples = batch_samples[:, :, :, :-1, ...]
            prompt_str = prompt_to_filename(prompt)

        paths = save_videos(batch_samples, self.result_dir, filenames=[prompt_str], fps=self.save_fps, container=self.container)
        print(f"Saved in {prompt_str}. Time used: {(time.time() - start):.2f} seconds")
        return paths[0]

    def get_image(self, image, prompt, steps=50, cfg_scale=7.5, eta=1.0, fs=3, seed=123, **sample_kwargs):
        """i2v_test.py:37-92. image: uint8 [H, W, 3] ndarray. Returns the path of the written clip."""
        return self._generate(image, prompt, steps, cfg_scale, eta, fs, seed, **sample_kwargs)
