"""The helper module both of the reference's Gradio backends and most third-party wrappers import: the counterpart of the
reference's `scripts/evaluation/funcs.py`, same names and signatures.

    batch_ddim_sampling      funcs.py:14-80     conditioning dict -> unconditional branch -> DDIM loop -> decode
    get_filelist, get_dirlist   funcs.py:83-97  sorted glob by one extension / sorted sub-directories
    load_model_checkpoint, load_prompts, get_latent_z   funcs.py:100-140, 221-226   re-exported from inference.py (one copy)
    load_image_batch         funcs.py:182-203   image files (or the first frame of an .avi) -> [n, 3, h, w] in [-1, 1] on the device
    load_video_batch         funcs.py:143-179   Motion-JPEG .avi clips -> [b, 3, t, h, w] in [-1, 1] on the device (HIP JPEG decoder)
    save_videos              funcs.py:206-218   [b, n_samples, c, t, h, w] -> one clip file per batch entry
    video_guided_synthesis   (not in the reference) re-exported from edit.py: a load_video_batch clip + an edited first frame -> clip

`get_filelist(data_dir, ext="*")` here is the reference's funcs.py signature; inference.py keeps its own
`get_filelist(data_dir, postfixes)`, as the reference does.
"""
import glob
import os

import numpy as np
import torch

from ...lvdm.models.samplers import options
from ...lvdm.models.samplers.dpm_solver import make_sampler
from .edit import video_guided_synthesis  # noqa: F401  (re-exported)
from .inference import get_latent_z, load_model_checkpoint, load_prompts  # noqa: F401  (re-exported)


@torch.no_grad()
@options.documented
def batch_ddim_sampling(model, cond, noise_shape, n_samples=1, ddim_steps=50, ddim_eta=1.0, cfg_scale=1.0,
                        temporal_cfg_scale=None, freeu=None, apg=None, token_downsampling=None, tiles=None, **kwargs):
    """funcs.py:14-80. `cond` is {"c_crossattn": [...], "c_concat": [...], "fs": tensor}; "fs" is taken out of it (the caller's
    dict comes back without it, as in the reference). A latent width of 32 (the 256 model) samples with "uniform" spacing and no
    guidance rescale, any other width with "uniform_trailing" and 0.7. With cfg_scale != 1 the unconditional branch is a copy of
    cond's keys (c_concat shared) whose c_crossattn is the empty prompt / zero embedding followed by the tokens of an all-zero
    [b, 3, 224, 224] image. `clean_cond=True` is passed, as the reference passes it. Returns [b, n_samples, c, t, h, w].

    The reference also hands `temporal_length=` and `conditional_guidance_scale_temporal=temporal_cfg_scale` to the sampler, where
    its UNet swallows them unused; they are not forwarded here and `temporal_cfg_scale` has no effect. Every other keyword
    argument reaches `DDIMSampler.sample` (`x_T`, `noises`, `use_graph`, `window_stride`, ...), except `sampler=`, which picks
    the sampler class as in `image_guided_synthesis` ("ddim", "dpmpp_2m", "dpmpp_2m_sde").
    Here `apg` takes the place of the guidance rescale of 0.7, which is then not applied."""
    options.fold(kwargs, freeu=freeu, apg=apg, token_downsampling=token_downsampling, tiles=tiles)
    ddim_sampler = make_sampler(model, kwargs.pop("sampler", "ddim"))
    kwargs.pop("temporal_length", None)
    kwargs.pop("conditional_guidance_scale_temporal", None)
    batch_size = noise_shape[0]
    fs = cond["fs"]
    del cond["fs"]
    if noise_shape[-1] == 32:
        timestep_spacing, guidance_rescale = "uniform", 0.0
    else:
        timestep_spacing, guidance_rescale = "uniform_trailing", 0.7 if apg is None else 0.0

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


_NO_VIDEO = ("{name}: the only video format this package decodes is Motion-JPEG in an AVI container (.avi; utils/load_video.py, "
             "what save_videos(container='avi') writes); the reference reads other codecs through decord, which is not available "
             "here. Re-encode the clip as MJPEG AVI, or pass images (.png / .jpg), or tensors to get_latent_z")


def video_frame_indices(total_frames, frame_stride, video_frames):
    """The frame selection of funcs.py:156-173 for a clip of `total_frames`: (indices, padding, frame_stride). max_valid =
    (total - 1) // frame_stride + 1; video_frames < 0 asks for every frame and sets the stride to 1 (the count of frames read is
    still capped by max_valid of the stride that was passed, as in the reference); indices = frame_stride * i; `padding` = how
    often the last frame read is repeated to reach the required count. The returned stride is the one later files of the same
    call see (the reference overwrites its argument). Host arithmetic only."""
    if not frame_stride > 0:
        raise ValueError("valid frame stride should be a positive integer!")
    max_valid_frames = (total_frames - 1) // frame_stride + 1
    if video_frames < 0:
        required_frames, frame_stride = total_frames, 1
    else:
        required_frames = video_frames
    query_frames = min(required_frames, max_valid_frames)
    return [frame_stride * i for i in range(query_frames)], max(required_frames - max_valid_frames, 0), frame_stride


def _jpeg_frames_normalised(frames, indices, size, device):
    """Frames `indices` of a Motion-JPEG clip (its JPEG files) -> fp32 [t, 3, size[0], size[1]] in [-1, 1] on the device: decoded to fp32 planes by
    the HIP JPEG decoder, resized with ops.resize_f32(antialias=False) only when the file's size differs, (x / 255 - 0.5) * 2."""
    from ... import ops
    from ...utils.load_video import decode_jpeg_frames
    planes = decode_jpeg_frames([frames[i] for i in indices], device=device, planar=True)         # [t, 3, H, W], 0..255
    t, _, H, W = planes.shape
    h, w = int(size[0]), int(size[1])
    if (H, W) != (h, w):
        planes = ops.resize_f32(planes.view(3 * t, H, W), (h, w), antialias=False).view(t, 3, h, w)
    return (planes / 255. - 0.5) * 2


def _device(device, name):
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{name} decodes and resamples on the HIP path only (there is no CPU fallback)")
    return device


def load_video_batch(filepath_list, frame_stride, video_size=(256, 256), video_frames=16, device=None):
    """funcs.py:143-179: every clip -> fp32 [3, t, video_size[0], video_size[1]] in [-1, 1], stacked to [b, 3, t, h, w] on
    `device` (default: the current HIP device; the reference returns a CPU tensor). The reference reads through decord; here a
    clip is a Motion-JPEG `.avi` (utils/load_video.py), and only the frames `video_frame_indices` selects are decoded.
    `video_frames=-1` takes every frame with stride 1; a clip that is too short repeats its last frame, with the reference's
    message. decord scales to `video_size` inside its reader with its own (swscale) filter, which is not reproduced: a clip
    whose size differs is resized to exactly `video_size` with ops.resize_f32(antialias=False), bilinear on the decoded fp32
    values, and a clip of that size is not touched. Any other extension, `.mp4` included, raises NotImplementedError before the
    file is opened."""
    for filepath in filepath_list:
        if os.path.splitext(os.path.split(filepath)[1])[1] != ".avi":
            raise NotImplementedError(_NO_VIDEO.format(name=f"load_video_batch({filepath!r})"))
    from ...utils.load_video import read_avi_mjpeg
    device = _device(device, "load_video_batch")
    batch_tensor = []
    for filepath in filepath_list:
        frames = read_avi_mjpeg(filepath)[3]
        indices, padding_num, frame_stride = video_frame_indices(len(frames), frame_stride, video_frames)
        frame_tensor = _jpeg_frames_normalised(frames, indices, video_size, device).permute(1, 0, 2, 3)       # [c, t, h, w]
        if padding_num:
            frame_tensor = torch.cat([frame_tensor, *([frame_tensor[:, -1:, :, :]] * padding_num)], dim=1)
            print(f'{os.path.split(filepath)[1]} is not long enough: {padding_num} frames padded.')
        batch_tensor.append(frame_tensor.contiguous())
    return torch.stack(batch_tensor, dim=0)


def load_image_batch(filepath_list, image_size=(256, 256), device=None):
    """funcs.py:182-203: every file -> fp32 [3, image_size[0], image_size[1]] in [-1, 1], stacked to [n, 3, h, w]. `.png` and
    `.jpg` are decoded with Pillow to float32 and resized to exactly `image_size` (aspect is not kept) on the device with
    ops.resize_f32(antialias=False), the equivalent of the reference's cv2.resize(INTER_LINEAR) on float32; then (x / 255 - 0.5)
    * 2. The result stays on `device` (default: the current HIP device), where the reference returns a CPU tensor. `.avi`
    (Motion-JPEG) gives the clip's first frame through the HIP JPEG decoder, resized the same way, as the reference's `.mp4`
    branch does through decord. `.mp4` raises NotImplementedError (no decoder for its codecs); other extensions raise it as in
    the reference."""
    from PIL import Image
    from ... import ops
    from ...utils.load_video import read_avi_mjpeg
    device = _device(device, "load_image_batch")
    h, w = int(image_size[0]), int(image_size[1])
    batch_tensor = []
    for filepath in filepath_list:
        _, ext = os.path.splitext(os.path.split(filepath)[1])
        if ext == ".mp4":
            raise NotImplementedError(_NO_VIDEO.format(name=f"load_image_batch({filepath!r})"))
        if ext == ".avi":
            batch_tensor.append(_jpeg_frames_normalised(read_avi_mjpeg(filepath)[3], [0], (h, w), device)[0])
            continue
        if ext not in (".png", ".jpg"):
            raise NotImplementedError(f"ERROR: <{ext}> image loading only support format: [png], [jpg]")
        rgb = np.array(Image.open(filepath).convert("RGB"), np.float32)                       # [H, W, 3], 0..255
        planes = torch.from_numpy(rgb).to(device).permute(2, 0, 1).contiguous()
        img = ops.resize_f32(planes, (h, w), antialias=False)
        batch_tensor.append((img / 255. - 0.5) * 2)
    return torch.stack(batch_tensor, dim=0)


def save_videos(batch_tensors, savedir, filenames, fps=10, container="avi", quality=90, deflate=None):
    """funcs.py:206-218: batch_tensors [b, n_samples, c, t, h, w] on the device -> one clip per batch entry, its n_samples side
    by side (clamp, (v + 1) / 2, x 255, uint8: dc_frames_to_u8), written as <savedir>/<filenames[idx]>.<ext>. The reference writes
    h264 `.mp4`; here the extension follows `container`: "avi" (Motion-JPEG at JPEG `quality`, the default), "apng" (.png) or
    "gif". `deflate` ("zlib", "hip" or None = the environment's DC_PNG_DEFLATE) picks the compressor of "apng". Returns the paths
    written (the reference returns nothing)."""
    from ...utils.save_video import _write_clip, frames_to_uint8
    paths = []
    for idx, vid_tensor in enumerate(batch_tensors):
        grid = frames_to_uint8(vid_tensor)                                     # [t, h, n * w, c]
        paths.append(_write_clip(os.path.join(savedir, f"{filenames[idx]}"), grid, fps, container, quality, deflate=deflate))
    return paths
