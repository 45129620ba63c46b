"""The helper module both of the reference's Gradio backends and most third-party wrappers import: the counterpart of the
reference's `scripts/evaluation/funcs.py`, same names and signatures.

    batch_ddim_sampling      funcs.py:14-80     conditioning dict -> unconditional branch -> DDIM loop -> decode
    get_filelist, get_dirlist   funcs.py:83-97  sorted glob by one extension / sorted sub-directories
    load_model_checkpoint, load_prompts, get_latent_z   funcs.py:100-140, 221-226   re-exported from inference.py (one copy)
    load_image_batch         funcs.py:182-203   image files -> [n, 3, h, w] in [-1, 1] on the device
    load_video_batch         funcs.py:143-179   raises: there is no video decoder in this package
    save_videos              funcs.py:206-218   [b, n_samples, c, t, h, w] -> one clip file per batch entry

`get_filelist(data_dir, ext="*")` here is the reference's funcs.py signature; inference.py keeps its own
`get_filelist(data_dir, postfixes)`, as the reference does.
"""
import glob
import os

import numpy as np
import torch

from ...lvdm.models.samplers.ddim import DDIMSampler
from ...lvdm.models.samplers.dpm_solver import SOLVERS as DPM_SOLVERS
from ...lvdm.models.samplers.dpm_solver import DPMSolverSampler
from .inference import get_latent_z, load_model_checkpoint, load_prompts  # noqa: F401  (re-exported)


@torch.no_grad()
def batch_ddim_sampling(model, cond, noise_shape, n_samples=1, ddim_steps=50, ddim_eta=1.0, cfg_scale=1.0,
                        temporal_cfg_scale=None, **kwargs):
    """funcs.py:14-80. `cond` is {"c_crossattn": [...], "c_concat": [...], "fs": tensor}; "fs" is taken out of it (the caller's
    dict comes back without it, as in the reference). A latent width of 32 (the 256 model) samples with "uniform" spacing and no
    guidance rescale, any other width with "uniform_trailing" and 0.7. With cfg_scale != 1 the unconditional branch is a copy of
    cond's keys (c_concat shared) whose c_crossattn is the empty prompt / zero embedding followed by the tokens of an all-zero
    [b, 3, 224, 224] image. `clean_cond=True` is passed, as the reference passes it. Returns [b, n_samples, c, t, h, w].

    The reference also hands `temporal_length=` and `conditional_guidance_scale_temporal=temporal_cfg_scale` to the sampler, where
    its UNet swallows them unused; they are not forwarded here and `temporal_cfg_scale` has no effect. Every other keyword
    argument reaches `DDIMSampler.sample` (`x_T`, `noises`, `use_graph`, `window_stride`, ...), except `sampler=`, which picks
    the sampler class as in `image_guided_synthesis` ("ddim", "dpmpp_2m", "dpmpp_2m_sde")."""
    name = kwargs.pop("sampler", "ddim")
    if name == "ddim":
        ddim_sampler = DDIMSampler(model)
    elif name in DPM_SOLVERS:
        ddim_sampler = DPMSolverSampler(model, solver=name)
    else:
        raise ValueError(f"sampler must be 'ddim' or one of {DPM_SOLVERS}, got {name!r}")
    kwargs.pop("temporal_length", None)
    kwargs.pop("conditional_guidance_scale_temporal", None)
    batch_size = noise_shape[0]
    fs = cond["fs"]
    del cond["fs"]
    if noise_shape[-1] == 32:
        timestep_spacing, guidance_rescale = "uniform", 0.0
    else:
        timestep_spacing, guidance_rescale = "uniform_trailing", 0.7

    if cfg_scale != 1.0:
        if model.uncond_type == "empty_seq":
            uc_emb = model.get_learned_conditioning(batch_size * [""])
        elif model.uncond_type == "zero_embed":
            c_emb = cond["c_crossattn"][0] if isinstance(cond, dict) else cond
            uc_emb = torch.zeros_like(c_emb)
        if hasattr(model, "embedder"):
            uc_img = torch.zeros(batch_size, 3, 224, 224, device=model.device)
            uc_img = model.image_proj_model(model.embedder(uc_img))          # b c h w -> b l c
            uc_emb = torch.cat([uc_emb, uc_img], dim=1)
        if isinstance(cond, dict):
            uc = {key: cond[key] for key in cond.keys()}
            uc.update({"c_crossattn": [uc_emb]})
        else:
            uc = uc_emb
    else:
        uc = None

    kwargs.update({"clean_cond": True})
    batch_variants = []
    for _ in range(n_samples):
        samples, _ = ddim_sampler.sample(S=ddim_steps, conditioning=cond, batch_size=batch_size, shape=noise_shape[1:],
                                         verbose=False, unconditional_guidance_scale=cfg_scale,
                                         unconditional_conditioning=uc, eta=ddim_eta, fs=fs,
                                         timestep_spacing=timestep_spacing, guidance_rescale=guidance_rescale, **kwargs)
        batch_variants.append(model.decode_first_stage(samples))
    return torch.stack(batch_variants, dim=1)                                  # batch, <samples>, c, t, h, w


def get_filelist(data_dir, ext="*"):
    """funcs.py:83-86: the files of `data_dir` with the extension `ext`, sorted."""
    file_list = glob.glob(os.path.join(data_dir, "*.%s" % ext))
    file_list.sort()
    return file_list


def get_dirlist(path):
    """funcs.py:88-97: the sub-directories of `path`, sorted; [] when it does not exist."""
    out = []
    if os.path.exists(path):
        out = [os.path.join(path, f) for f in os.listdir(path) if os.path.isdir(os.path.join(path, f))]
    out.sort()
    return out


_NO_VIDEO = ("{name}: reading a video needs a decoder (the reference uses decord), and this package ships none; decode the "
             "frames yourself and pass images (.png / .jpg), or tensors to get_latent_z")


def load_video_batch(filepath_list, frame_stride, video_size=(256, 256), video_frames=16):
    """funcs.py:143-179 reads clips through decord. Not available here: raises NotImplementedError."""
    raise NotImplementedError(_NO_VIDEO.format(name="load_video_batch"))


def load_image_batch(filepath_list, image_size=(256, 256), device=None):
    """funcs.py:182-203: every file -> fp32 [3, image_size[0], image_size[1]] in [-1, 1], stacked to [n, 3, h, w]. `.png` and
    `.jpg` are decoded with Pillow to float32 and resized to exactly `image_size` (aspect is not kept) on the device with
    ops.resize_f32(antialias=False), the equivalent of the reference's cv2.resize(INTER_LINEAR) on float32; then (x / 255 - 0.5)
    * 2. The result stays on `device` (default: the current HIP device), where the reference returns a CPU tensor. `.mp4`
    raises NotImplementedError (no video decoder); other extensions raise it as in the reference."""
    from PIL import Image
    from ... import ops
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("load_image_batch resamples on the HIP path only (there is no CPU fallback)")
    h, w = int(image_size[0]), int(image_size[1])
    batch_tensor = []
    for filepath in filepath_list:
        _, ext = os.path.splitext(os.path.split(filepath)[1])
        if ext == ".mp4":
            raise NotImplementedError(_NO_VIDEO.format(name=f"load_image_batch({filepath!r})"))
        if ext not in (".png", ".jpg"):
            raise NotImplementedError(f"ERROR: <{ext}> image loading only support format: [png], [jpg]")
        rgb = np.array(Image.open(filepath).convert("RGB"), np.float32)                       # [H, W, 3], 0..255
        planes = torch.from_numpy(rgb).to(device).permute(2, 0, 1).contiguous()
        img = ops.resize_f32(planes, (h, w), antialias=False)
        batch_tensor.append((img / 255. - 0.5) * 2)
    return torch.stack(batch_tensor, dim=0)


def save_videos(batch_tensors, savedir, filenames, fps=10, container="avi", quality=90):
    """funcs.py:206-218: batch_tensors [b, n_samples, c, t, h, w] on the device -> one clip per batch entry, its n_samples side
    by side (clamp, (v + 1) / 2, x 255, uint8: dc_frames_to_u8), written as <savedir>/<filenames[idx]>.<ext>. The reference writes
    h264 `.mp4`; here the extension follows `container`: "avi" (Motion-JPEG at JPEG `quality`, the default), "apng" (.png) or
    "gif". Returns the paths written (the reference returns nothing)."""
    from ...utils.save_video import _write_clip, frames_to_uint8
    paths = []
    for idx, vid_tensor in enumerate(batch_tensors):
        grid = frames_to_uint8(vid_tensor)                                     # [t, h, n * w, c]
        paths.append(_write_clip(os.path.join(savedir, f"{filenames[idx]}"), grid, fps, container, quality))
    return paths
