"""The diffusers-style entry point of the reference (scripts/gradio/dynamicrafter_pipeline.py): one image (PIL, ndarray or
tensor) and a prompt in, a batch of decoded clips out, through `__call__` with the argument names of a diffusers pipeline.
Nothing here imports `gradio`, `diffusers` or `torchvision`.
"""
import os

import numpy as np
import torch

from ...lvdm.models.samplers import options
from ...lvdm.models.samplers.ddim import DDIMSampler
from ..evaluation.funcs import get_latent_z, save_videos
from ..evaluation.inference import resize_center_crop_f32
from .i2v_test import load_model, parse_resolution


class DynamiCrafterImg2VideoPipeline:
    """DynamiCrafter image-to-video with a diffusers-like interface (dynamicrafter_pipeline.py:68-571).

    `DynamiCrafterImg2VideoPipeline(resolution, model=..., | ckpt_path=..., config=...)`: nothing is downloaded; pass the
    checkpoint (and optionally a YAML; default this package's configs/inference_<width>_v1.0.yaml) or a ready model.
    `pipe(image, prompt, negative_prompt, num_inference_steps, guidance_scale, eta, frame_stride, ...)` follows the reference
    step by step: the image is normalised to [-1, 1] and resized (`_preprocess_image`), the RESIZED image goes to the image
    embedder and the AE (`_encode_image`), c_concat is its latent on every frame, the unconditional branch pairs the negative /
    empty / zero text embedding with the tokens of an all-zero image of the resolution's size, and `DDIMSampler.sample` runs with
    its defaults ("uniform" spacing, no guidance rescale), the reference's arguments and any extra **kwargs.

    Two deliberate departures from the reference:
      * `generator=` and `latents=` are honoured: `latents` ([b, c, t, h/8, w/8]) is the sampler's x_T; otherwise x_T is drawn
        from `generator` (on the generator's device) or, with neither, by the sampler from the global RNG. The reference accepts
        both arguments and then ignores them.
      * `output_type="pil"` returns, per batch entry, a list of `PIL.Image` frames (clamp, (v + 1) / 2, x 255 through
        `frames_to_uint8`). The reference prints that it is unimplemented and returns numpy.

    What neither argument reaches is the AE's posterior sample of the image latent (c_concat): it draws from torch's global CPU
    generator, as in the reference; seed that one too (torch.manual_seed) for bit-identical clips.

    Also: the fork's "fixed" DDIM sampler (get_fixed_ddim_sampler) is not ported - the step kernel clamps the radicand that it
    patches sigma for (see `use_fixed_scheduler` in inference.py); `callback(step, timestep, None)` is called from the sampler's
    `callback` hook every `callback_steps` steps (the latent stays in the sampler's buffers and is not handed out);
    `enable_attention_slicing`, `disable_attention_slicing` and `enable_xformers_memory_efficient_attention` are accepted and do
    nothing (attention is already a flash kernel); `num_videos_per_prompt` and `cross_attention_kwargs` are accepted and unused,
    as in the reference."""

    def __init__(self, resolution="256_256", *, model=None, ckpt_path=None, config=None, device=None):
        self.resolution = parse_resolution(resolution)                       # (height, width)
        if model is None:
            if ckpt_path is None:
                self._download_model()
            model = load_model(self.resolution, ckpt_path, config, device)
        elif device is not None:
            model = model.to(device)
        self.model = model
        self.device = model.device
        self.dtype = torch.float32

    def _download_model(self):
        raise RuntimeError(f"{type(self).__name__} does not download weights: pass ckpt_path= (a DynamiCrafter model.ckpt for "
                           f"{self.resolution[0]}x{self.resolution[1]}) or a ready model=")

    def enable_attention_slicing(self, slice_size="auto"):
        pass

    def disable_attention_slicing(self):
        pass

    def enable_xformers_memory_efficient_attention(self):
        pass

    def enable_freeu(self, s1, s2, b1, b2, version=1):
        """FreeU on the UNet's decoder for every later call of the pipeline, with diffusers' argument order
        (UNetModel.enable_freeu; `version=2` is the authors' mean-weighted backbone scaling). Not in the reference class."""
        self.model.model.diffusion_model.enable_freeu(s1, s2, b1, b2, version=version)

    def disable_freeu(self):
        self.model.model.diffusion_model.disable_freeu()

    def enable_token_downsampling(self, factor=2, levels=(0,), mode="nearest"):
        """K/V token downsampling in the UNet's spatial self-attentions for every later call of the pipeline
        (UNetModel.enable_token_downsampling). Not in the reference class."""
        self.model.model.diffusion_model.enable_token_downsampling(factor=factor, levels=levels, mode=mode)

    def disable_token_downsampling(self):
        self.model.model.diffusion_model.disable_token_downsampling()

    def to(self, device, dtype=None):
        """Moves the model. `dtype` other than float32 is refused: the kernels fix their own storage types."""
        if dtype is not None and dtype != torch.float32:
            raise ValueError(f"the HIP path fixes its storage types (bf16 activations, fp32 latents); dtype {dtype} is not an option")
        self.model = self.model.to(device)
        self.device = self.model.device
        return self

    def _preprocess_image(self, image, height=None, width=None):
        """dynamicrafter_pipeline.py:267-288: PIL / ndarray [H, W, 3] / tensor [3, H, W] -> fp32 [3, h, w] in [-1, 1] on the
        device. Values above 1 are taken as 0..255. With `height` and `width` it is an exact Resize((height, width)) (aspect not
        kept), otherwise the resolution's Resize + CenterCrop; both are ops.resize_f32(antialias=True)."""
        from ... import ops
        if not isinstance(image, (np.ndarray, torch.Tensor)):
            image = np.array(image)                                          # PIL.Image
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.array(image)).to(self.device).permute(2, 0, 1).float()
        image = image.to(self.device).float()
        if image.max() > 1.0:
            image = image / 255.0
        image = ((image - 0.5) * 2).contiguous()
        if height is not None and width is not None:
            return ops.resize_f32(image, (int(height), int(width)), antialias=True)
        return resize_center_crop_f32(image, self.resolution)

    def _encode_prompt(self, prompt, negative_prompt, device=None):
        """:290-318. -> {"cond", "uncond"}: the negative prompts' embedding replaces the empty-prompt / zero one."""
        text_embeddings = self.model.get_learned_conditioning(prompt)
        if negative_prompt is not None:
            uncond_embeddings = self.model.get_learned_conditioning(negative_prompt)
        elif self.model.uncond_type == "empty_seq":
            uncond_embeddings = self.model.get_learned_conditioning([""] * len(prompt))
        else:                                                                # "zero_embed"
            uncond_embeddings = torch.zeros_like(text_embeddings)
        return {"cond": text_embeddings, "uncond": uncond_embeddings}

    def _encode_image(self, image, num_frames=None):
        """:320-336. [3, h, w] or [b, 3, h, w] -> (image tokens [b, l, c], latent [b, c, 1, h/8, w/8])."""
        if image.dim() == 3:
            image = image.unsqueeze(0)
        image = image.to(self.device)
        img_emb = self.model.image_proj_model(self.model.embedder(image))
        z = get_latent_z(self.model, image.unsqueeze(2))
        return img_emb, z

    def _prepare_conditioning(self, text_embeddings, image_embeddings, image_latents, frame_stride, guidance_scale, batch_size,
                              num_frames=None):
        """:338-370. One image with several prompts: its tokens and latent are repeated over the batch."""
        if image_embeddings.shape[0] != batch_size:
            image_embeddings = image_embeddings.expand(batch_size, -1, -1)
            image_latents = image_latents.expand(batch_size, -1, -1, -1, -1)
        cond = {"c_crossattn": [torch.cat([text_embeddings["cond"], image_embeddings], dim=1)]}
        hybrid = self.model.model.conditioning_key == "hybrid"
        if hybrid:
            t = self.model.temporal_length if num_frames is None else num_frames
            img_cat_cond = image_latents[:, :, :1].repeat(1, 1, t, 1, 1)
            cond["c_concat"] = [img_cat_cond]
        uc = None
        if guidance_scale != 1.0:
            zero_image = torch.zeros((batch_size, 3, self.resolution[0], self.resolution[1]), device=self.model.device)
            uc_img_emb = self.model.image_proj_model(self.model.embedder(zero_image))
            uc = {"c_crossattn": [torch.cat([text_embeddings["uncond"], uc_img_emb], dim=1)]}
            if hybrid:
                uc["c_concat"] = [img_cat_cond]
        fs = torch.tensor([frame_stride] * batch_size, dtype=torch.long, device=self.model.device)
        return {"cond": cond, "uc": uc, "fs": fs}

    def _prepare_latents(self, noise_shape, device, generator, dtype=torch.float32):
        """:372-378. Drawn on the generator's device (a CPU generator gives the same x_T on every machine), then moved."""
        if isinstance(generator, (list, tuple)):
            if len(generator) != noise_shape[0]:
                raise ValueError(f"{len(generator)} generators for a batch of {noise_shape[0]}")
            return torch.cat([self._prepare_latents((1,) + tuple(noise_shape[1:]), device, g, dtype) for g in generator])
        if generator is not None:
            return torch.randn(tuple(noise_shape), generator=generator, device=generator.device, dtype=dtype).to(device)
        return torch.randn(tuple(noise_shape), device=device, dtype=dtype)

    def _decode_latents(self, latents):
        with torch.no_grad():
            return self.model.decode_first_stage(latents)

    def _postprocess_video(self, videos, output_type):
        """[b, 3, t, h, w] on the device -> "tensor": as is; "numpy": a float32 ndarray; "pil": b lists of t PIL images."""
        if output_type == "tensor":
            return videos
        if output_type == "numpy":
            return videos.cpu().float().numpy()
        if output_type == "pil":
            from PIL import Image
            from ...utils.save_video import frames_to_uint8
            out = []
            for v in videos:
                frames = frames_to_uint8(v[None]).cpu().numpy()              # [t, h, w, 3]
                out.append([Image.fromarray(f) for f in frames])
            return out
        raise ValueError(f"output_type must be 'tensor', 'numpy' or 'pil', got {output_type!r}")

    @torch.no_grad()
    @options.documented
    def __call__(self, image, prompt="", negative_prompt=None, num_inference_steps=50, guidance_scale=7.5, eta=0.0,
                 frame_stride=3, num_frames=None, height=None, width=None, num_videos_per_prompt=1, generator=None,
                 latents=None, output_type="tensor", return_dict=True, callback=None, callback_steps=1,
                 cross_attention_kwargs=None, freeu=None, apg=None, token_downsampling=None, tiles=None, **kwargs):
        """:398-530. Returns {"videos": v} (or v with return_dict=False); v is [b, 3, num_frames, height, width] as a device
        tensor ("tensor"), an ndarray ("numpy") or b lists of PIL frames ("pil"). Extra **kwargs reach DDIMSampler.sample.
        `freeu` and `token_downsampling` below hold for this call only; enable_freeu / enable_token_downsampling set them for
        every later call."""
        options.fold(kwargs, freeu=freeu, apg=apg, token_downsampling=token_downsampling, tiles=tiles)
        if isinstance(prompt, str):
            prompt = [prompt]
        batch_size = len(prompt)
        if negative_prompt is not None:
            if isinstance(negative_prompt, str):
                negative_prompt = [negative_prompt] * batch_size
            elif len(negative_prompt) != batch_size:
                raise ValueError(f"negative_prompt length ({len(negative_prompt)}) != batch_size ({batch_size})")
        if output_type not in ("tensor", "numpy", "pil"):
            raise ValueError(f"output_type must be 'tensor', 'numpy' or 'pil', got {output_type!r}")

        processed_image = self._preprocess_image(image, height, width)
        num_frames = num_frames or self.model.temporal_length
        channels = self.model.model.diffusion_model.out_channels
        if height is None or width is None:
            height, width = self.resolution
        noise_shape = (batch_size, channels, num_frames, height // 8, width // 8)

        text_embeddings = self._encode_prompt(prompt, negative_prompt, self.device)
        image_embeddings, image_latents = self._encode_image(processed_image, num_frames)
        conditioning = self._prepare_conditioning(text_embeddings, image_embeddings, image_latents, frame_stride, guidance_scale,
                                                  batch_size, num_frames)
        if latents is not None:
            if tuple(latents.shape) != noise_shape:
                raise ValueError(f"latents must be {noise_shape}, got {tuple(latents.shape)}")
            x_T = latents.to(self.device)
        elif generator is not None:
            x_T = self._prepare_latents(noise_shape, self.device, generator)
        else:
            x_T = None
        scheduler = DDIMSampler(self.model)
        if callback is not None:
            every = max(int(callback_steps), 1)
            kwargs["callback"] = lambda i: callback(i, int(scheduler._exec_timesteps[i]), None) if i % every == 0 else None
        samples, _ = scheduler.sample(S=num_inference_steps, conditioning=conditioning["cond"], batch_size=batch_size,
                                      shape=noise_shape[1:], verbose=False, unconditional_guidance_scale=guidance_scale,
                                      unconditional_conditioning=conditioning["uc"], eta=eta, fs=conditioning["fs"], x_T=x_T,
                                      **kwargs)
        videos = self._postprocess_video(self._decode_latents(samples), output_type)
        return {"videos": videos} if return_dict else videos

    def save_video(self, video, output_path, fps=8, container="avi", quality=90, **kwargs):
        """:532-571. video [c, t, h, w] or [b, c, t, h, w] on the device -> <output_path without extension>.<ext of
        `container`> (the first batch entry, as the reference names one file). Returns the path written."""
        output_dir = os.path.dirname(output_path)
        if output_dir:
            os.makedirs(output_dir, exist_ok=True)
        filename = os.path.basename(output_path).split(".")[0]
        if video.dim() == 4:
            video = video.unsqueeze(0).unsqueeze(0)
        elif video.dim() == 5:
            video = video.unsqueeze(1)
        return save_videos(video[:1].to(self.device), output_dir or ".", filenames=[filename], fps=fps, container=container,
                           quality=quality)[0]
