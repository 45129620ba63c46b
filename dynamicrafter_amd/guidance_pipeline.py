"""DynamiCrafterGuidancePipeline — the reference's score-distillation pipeline (guidance_pipeline.py:34-961) on the
fused HIP path.

`DynamiCrafterGuidancePipeline(model, resolution="256_256")(image, prompt, ...)` prepares the conditioning with
the reference's own steps (_preprocess_image :161-182, _encode_prompt :184-212, _encode_image :214-230,
_prepare_conditioning :232-265), optimises the video latent with SDS (lvdm/models/samplers/sds.py, which restates
_optimization_loop and _sds_loss) and decodes it. Differences by design:
  * it takes a loaded model: no checkpoint download, no device selection, no debug directory, images or videos;
  * resize and centre crop are F.interpolate (bilinear, antialias) with torchvision's size and crop arithmetic
    (torchvision is not a dependency): pixel parity with torchvision.transforms.Resize is not claimed;
  * `loss_type` and `weight_type` are accepted and change nothing, as in the reference, whose _optimization_loop
    never passes them on (_sds_loss always weights with "t"). SDSGuidance.optimize takes the other weightings.
"""
from typing import List, Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

from . import _hip
from .lvdm.models.samplers.sds import SDSGuidance, default_guidance_rescale, default_timestep_spacing
from .scripts.evaluation.inference import get_latent_z


def _resize(image, size):
    """[C, H, W] -> [C, h, w], bilinear with antialiasing (torchvision.transforms.Resize's filter on tensors)."""
    return F.interpolate(image[None], size=tuple(size), mode="bilinear", align_corners=False, antialias=True)[0]


class DynamiCrafterGuidancePipeline:
    def __init__(self, model, resolution: str = "256_256"):
        self.model = model
        self.resolution = tuple(map(int, resolution.split("_")))
        self.device = model.device

    # ------------------------------------------------------------------ the reference's preparation steps
    def _preprocess_image(self, image, height=None, width=None):
        """PIL / HWC array / CHW tensor -> [3, H, W] in [-1, 1]; Resize(min(resolution)) + CenterCrop(resolution),
        or Resize((height, width)) when both are given (:161-182)."""
        if not isinstance(image, (np.ndarray, torch.Tensor)):
            image = np.array(image)
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(image).permute(2, 0, 1).float()
        image = image.float()
        if image.max() > 1.0:
            image = image / 255.0
        image = (image - 0.5) * 2
        if height is not None and width is not None:
            return _resize(image, (height, width))
        h, w = image.shape[-2:]
        short = min(self.resolution)
        # torchvision Resize(int): the shorter edge becomes `short`, the longer int(short * long / shorter)
        size = (int(short * h / w), short) if w <= h else (short, int(short * w / h))
        image = _resize(image, size)
        th, tw = self.resolution
        top = int(round((size[0] - th) / 2.0))
        left = int(round((size[1] - tw) / 2.0))
        if top < 0 or left < 0:
            raise ValueError(f"image resized to {size} is smaller than the crop {self.resolution}")
        return image[:, top:top + th, left:left + tw]

    def _encode_prompt(self, prompt, negative_prompt):
        m = self.model
        text = m.get_learned_conditioning(prompt)
        if negative_prompt is not None:
            uncond = m.get_learned_conditioning(negative_prompt)
        elif m.uncond_type == "empty_seq":
            uncond = m.get_learned_conditioning([""] * len(prompt))
        else:                                             # "zero_embed"
            uncond = torch.zeros_like(text)
        return {"cond": text, "uncond": uncond}

    def _encode_image(self, image):
        if image.dim() == 3:
            image = image.unsqueeze(0)
        image = image.to(self.device)
        img_emb = self.model.image_proj_model(self.model.embedder(image))
        z = get_latent_z(self.model, image.unsqueeze(2))
        return img_emb, z

    def _prepare_conditioning(self, text_embeddings, image_embeddings, image_latents, frame_stride, guidance_scale,
                              batch_size, num_frames):
        m = self.model
        cond = {"c_crossattn": [torch.cat([text_embeddings["cond"], image_embeddings], dim=1)]}
        hybrid = m.model.conditioning_key == "hybrid"
        if hybrid:
            img_cat_cond = image_latents[:, :, :1, :, :].repeat(1, 1, num_frames, 1, 1)
            cond["c_concat"] = [img_cat_cond]
        uc = None
        if guidance_scale != 1.0:
            zero_image = torch.zeros((batch_size, 3, self.resolution[0], self.resolution[1]), device=self.device,
                                     dtype=getattr(m, "dtype", torch.float32))
            uc_img_emb = m.image_proj_model(m.embedder(zero_image))
            uc = {"c_crossattn": [torch.cat([text_embeddings["uncond"], uc_img_emb], dim=1)]}
            if hybrid:
                uc["c_concat"] = [img_cat_cond]
        fs = torch.tensor([frame_stride] * batch_size, dtype=torch.long, device=self.device)
        return {"cond": cond, "uc": uc, "fs": fs}

    def prepare(self, image, prompt="", negative_prompt=None, guidance_scale=7.5, frame_stride=24, num_frames=None,
                height=None, width=None):
        """The conditioning and latent shape of __call__: ({"cond", "uc", "fs"}, (B, C, T, h, w))."""
        prompt = [prompt] if isinstance(prompt, str) else list(prompt)
        batch_size = len(prompt)
        if negative_prompt is not None:
            if isinstance(negative_prompt, str):
                negative_prompt = [negative_prompt] * batch_size
            elif len(negative_prompt) != batch_size:
                raise ValueError(f"negative_prompt length ({len(negative_prompt)}) != batch_size ({batch_size})")
        processed = self._preprocess_image(image, height, width)
        num_frames = num_frames or self.model.temporal_length
        channels = self.model.model.diffusion_model.out_channels
        if height is None or width is None:
            height, width = self.resolution
        shape = (batch_size, channels, num_frames, height // 8, width // 8)
        with torch.no_grad():
            text = self._encode_prompt(prompt, negative_prompt)
            img_emb, z = self._encode_image(processed)
            cond = self._prepare_conditioning(text, img_emb, z, frame_stride, guidance_scale, batch_size, num_frames)
        return cond, shape

    @torch.no_grad()
    def __call__(self, image, prompt: Union[str, List[str]] = "", negative_prompt=None, guidance_scale: float = 7.5,
                 frame_stride: int = 24, num_frames: Optional[int] = None, height: Optional[int] = None,
                 width: Optional[int] = None, num_optimization_steps: int = 100, learning_rate: float = 0.05,
                 loss_type: str = "sds", weight_type: str = "t", cfg_scale: Optional[float] = None,
                 optimizer_type: str = "Adam", return_dict: bool = True, use_graph: bool = True, callback=None,
                 **kwargs):
        """The reference's __call__ (:810-961): conditioning, SDS optimisation of the latent, decode. Returns
        {"videos": [B, 3, T, H, W]} or the tensor when return_dict=False. `loss_type` and `weight_type` do not change
        the result (see the module docstring); the reference's sampling-only arguments (num_inference_steps, eta,
        generator, ...) are accepted in **kwargs and not used."""
        if cfg_scale is None:
            cfg_scale = guidance_scale
        cond, shape = self.prepare(image, prompt, negative_prompt, guidance_scale, frame_stride, num_frames, height,
                                   width)
        res_w = self.resolution[1]
        latents, _ = SDSGuidance(self.model).optimize(
            cond["cond"], cond["uc"], cond["fs"], shape, num_optimization_steps=num_optimization_steps,
            learning_rate=learning_rate, cfg_scale=cfg_scale, guidance_rescale=default_guidance_rescale(res_w),
            timestep_spacing=default_timestep_spacing(res_w), weight_type="t", optimizer_type=optimizer_type,
            use_graph=use_graph, callback=callback)
        videos = self.model.decode_first_stage(latents)
        _hip.check_error_word("DynamiCrafterGuidancePipeline decode")
        return {"videos": videos} if return_dict else videos
