"""Host harness of the hot path: the counterpart of the reference's `scripts/evaluation/inference.py` functions that
sit between the data loader and the sampler.

    image_guided_synthesis   inference.py:216-313   conditioning assembly -> DDIM (or DPM-Solver++) loop -> decode
    build_conditioning       inference.py:232-273   the conditioning assembly of image_guided_synthesis, shared with edit.py
    get_latent_z             inference.py:164-169   video -> per-frame AE latents
    load_model_checkpoint    inference.py:34-59     Lightning / DeepSpeed state dict -> model (key renames kept)
    get_filelist             funcs.py / inference.py:26-32   sorted glob by suffix
    load_prompts             inference.py:61-69     non-empty lines of a prompt file
    load_data_prompts        inference.py:71-113    prompt folder -> (file names, clips on the device, prompts)
    run_inference            inference.py:316-380   config + checkpoint + prompt folder -> clips under <savedir>/samples_separate
    get_parser, __main__     inference.py:383-427   the command line (python -m dynamicrafter_amd.scripts.evaluation.inference)

Same names, argument meaning and return layout as the reference, so `run_inference` style drivers can call them
unchanged. The loader's torchvision transform (Resize(min(video_size)) -> CenterCrop(video_size) -> ToTensor ->
Normalize(0.5, 0.5), inference.py:71-76) runs as HIP launches on the decoded uint8 pixels (csrc/preprocess.hip): files are
decoded with Pillow, but its resize is reproduced bit for bit on the device (`preprocess_image`), and torchvision's size and
crop arithmetic is restated in `resize_geometry` (torchvision is not a dependency). The model is this package's `LatentVisualDiffusion` on a HIP device; `model.embedder`,
`model.cond_stage_model` and `model.image_proj_model` are whatever the config instantiated (the OpenCLIP towers are
outside this package: see lvdm/modules/encoders/condition.py).
"""
import argparse
import datetime
import functools
import glob
import os
import random
import time
import warnings
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from ...lvdm.models.samplers import options
from ...lvdm.models.samplers.dpm_solver import SOLVERS as DPM_SOLVERS
from ...lvdm.models.samplers.dpm_solver import make_sampler


def load_model_checkpoint(model, ckpt):
    """inference.py:34-59. `ckpt` is a path (torch.load) or an already loaded mapping."""
    if isinstance(ckpt, (str, bytes)) or hasattr(ckpt, "__fspath__"):
        if str(ckpt).endswith(".safetensors"):
            # flat tensor file with the same keys (the pruned community releases, reference README.md:384-385)
            from safetensors.torch import load_file
            state_dict = {"state_dict": load_file(str(ckpt), device="cpu")}
        else:
            state_dict = torch.load(ckpt, map_location="cpu")
    else:
        state_dict = ckpt
    if "state_dict" in state_dict:
        state_dict = state_dict["state_dict"]
        try:
            model.load_state_dict(state_dict, strict=True)
        except RuntimeError:
            # the 256x256 release names the frame-stride embedding `framestride_embed` (inference.py:41-51)
            renamed = OrderedDict((k.replace("framestride_embed", "fps_embedding"), v) for k, v in state_dict.items())
            model.load_state_dict(renamed, strict=True)
    else:
        # DeepSpeed checkpoints: {"module": {"_forward_module.<key>": tensor}} (inference.py:52-57: key[16:])
        model.load_state_dict(OrderedDict((k[16:], v) for k, v in state_dict["module"].items()))
    return model


def get_latent_z(model, videos):
    """inference.py:164-169: [b,c,t,h,w] pixels in [-1,1] -> [b,4,t,h/8,w/8] scaled latents."""
    b, c, t, h, w = videos.shape
    x = videos.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)
    z = model.encode_first_stage(x)
    return z.reshape(b, t, *z.shape[1:]).permute(0, 2, 1, 3, 4).contiguous()


def build_conditioning(model, prompts, videos, unconditional_guidance_scale=1.0, cfg_img=None, multiple_cond_cfg=False,
                       ends_only=False, num_frames=None):
    """The conditioning assembly of inference.py:232-273, shared by image_guided_synthesis and video_guided_synthesis
    (scripts/evaluation/edit.py): `videos` [b, 3, t, h, w] whose first frame is the guiding image -> (cond, uc, uc_2).
    cond: text + image tokens in c_crossattn and, for a hybrid model, the image latent over all frames in c_concat
    (`ends_only`: first and last frame only, zeros between, for loop / interp; `num_frames`: repeat over that many frames).
    uc: the unconditional branch (None at guidance scale 1); uc_2: image yes, text "" (None unless multiple_cond_cfg and
    cfg_img != 1)."""
    batch_size = videos.shape[0]
    img = videos[:, :, 0]                                         # b c h w
    img_emb = model.image_proj_model(model.embedder(img))         # b (t l) c
    cond_emb = model.get_learned_conditioning(prompts)
    cond = {"c_crossattn": [torch.cat([cond_emb, img_emb], dim=1)]}
    hybrid = model.model.conditioning_key == "hybrid"
    if hybrid:
        z = get_latent_z(model, videos)                           # b c t h w
        if ends_only:
            img_cat_cond = torch.zeros_like(z)
            img_cat_cond[:, :, 0] = z[:, :, 0]
            img_cat_cond[:, :, -1] = z[:, :, -1]
        else:
            img_cat_cond = z[:, :, :1].repeat(1, 1, z.shape[2] if num_frames is None else num_frames, 1, 1)
        cond["c_concat"] = [img_cat_cond]

    if unconditional_guidance_scale != 1.0:
        if model.uncond_type == "empty_seq":
            uc_emb = model.get_learned_conditioning(batch_size * [""])
        elif model.uncond_type == "zero_embed":
            uc_emb = torch.zeros_like(cond_emb)
        uc_img_emb = model.image_proj_model(model.embedder(torch.zeros_like(img)))
        uc = {"c_crossattn": [torch.cat([uc_emb, uc_img_emb], dim=1)]}
        if hybrid:
            uc["c_concat"] = [img_cat_cond]
    else:
        uc = None

    # the third branch: image yes, text "" (inference.py:266-273)
    uc_2 = None
    if multiple_cond_cfg and cfg_img != 1.0:
        uc_2 = {"c_crossattn": [torch.cat([uc_emb, img_emb], dim=1)]}
        if hybrid:
            uc_2["c_concat"] = [img_cat_cond]
    return cond, uc, uc_2


def check_ae_extent(model, noise_shape):
    """The autoencoder runs on whole frames of a tiled call, whatever their size. Its scratch buffers are limited to 2^31
    elements (ops.Arena refuses a larger one with a ValueError of its own, but only in the middle of the encode or the
    decode): the two that grow fastest are checked here, ahead of the sampling, and the limit is named. They are the
    score matrix of the mid-block attention, (h w)^2 for a latent frame of h x w, and the full-resolution activations of
    one call, frames x pixels x channels."""
    dd = getattr(getattr(model, "first_stage_model", None), "ddconfig", None)
    if dd is None:
        return
    h, w = int(noise_shape[3]), int(noise_shape[4])
    if (h * w) ** 2 >= 2 ** 31:
        raise ValueError(f"tiles: a latent frame of {h} x {w} = {h * w} positions exceeds what the autoencoder's mid-block "
                         f"attention takes (its score matrix of (h w)^2 elements must stay under 2^31: h w <= 46340)")
    mult = list(dd["ch_mult"])
    f = 2 ** (len(mult) - 1)
    frames = max(1, getattr(model, "ae_frames_per_call", 1)) if getattr(model, "perframe_ae", False) \
        else int(noise_shape[0]) * int(noise_shape[2])
    width = dd["ch"] * max(mult[:2])                     # the widest buffer at full resolution (a level-0 ResBlock's input)
    if frames * h * f * w * f * width >= 2 ** 31:
        raise ValueError(f"tiles: {frames} frames of {h * f} x {w * f} pixels per autoencoder call exceed its 2^31-element "
                         f"buffer limit at {width} channels (decode frame by frame: perframe_ae)")


@torch.no_grad()
@options.documented
def image_guided_synthesis(model, prompts, videos, noise_shape, n_samples=1, ddim_steps=50, ddim_eta=1.,
                           unconditional_guidance_scale=1.0, cfg_img=None, fs=None, text_input=False,
                           multiple_cond_cfg=False, loop=False, interp=False, timestep_spacing="uniform",
                           guidance_rescale=0.0, use_fixed_scheduler=False, sampler="ddim", num_frames=None,
                           window_stride=None, window_weights="triangle", window_shift=0, freeu=None, apg=None,
                           token_downsampling=None, tiles=None, **kwargs):
    """inference.py:216-313. Returns [batch, n_samples, c, t, h, w] decoded frames.

    `use_fixed_scheduler` is accepted and ignored: the fork's "fixed" sampler only patches sigma so that
    1 - a_prev - sigma^2 cannot go negative (inference.py:172-214); the step kernel here clamps that radicand at zero
    (csrc/elementwise.hip), which is the same guard at the point of use.
    Extra keyword arguments (e.g. `x_T`, `noises`, `use_graph`) are passed to `DDIMSampler.sample` as the reference
    passes its **kwargs.
    `sampler` (not in the reference): "ddim" (default, the reference's sampler), or "dpmpp_2m" / "dpmpp_2m_sde" for
    DPM-Solver++ on the same timesteps (lvdm/models/samplers/dpm_solver.py; `ddim_steps` is then its step count and
    `ddim_eta` is not used).
    `num_frames` (not in the reference): the clip's length in latent frames. Above the model's `temporal_length` the
    sampler denoises overlapping windows of one long latent (lvdm/models/samplers/windows.py; `window_stride` defaults to
    temporal_length // 2): the image latent is repeated over `num_frames` for c_concat, `x_T` / `noises` passed through
    are `num_frames` long, and all frames are decoded. `window_stride` alone asks for windows at the clip's own length.
    Not with `loop` / `interp`: their c_concat is zero on interior frames, so interior windows would see a conditioning
    the model never met.
    With `tiles`, `noise_shape` and `videos` are at the large size: the large image is encoded for c_concat and the large
    latent decoded by the same autoencoder, frame by frame. `loop` / `interp` work with spatial tiles, since every tile
    holds the first and the last frame; they stay refused when the time axis is tiled too."""
    options.fold(kwargs, freeu=freeu, apg=apg, token_downsampling=token_downsampling, tiles=tiles)
    if tiles is not None:
        if window_stride is not None and (loop or interp):
            raise ValueError(f"tiles with window_stride = {window_stride} cannot be combined with loop = {loop} / interp = "
                             f"{interp}: boxes inside the clip would be conditioned on all-zero c_concat frames")
        check_ae_extent(model, noise_shape)
    T_model = getattr(model, "temporal_length", None)
    if num_frames is not None:
        if loop or interp:
            raise ValueError(f"num_frames = {num_frames} cannot be combined with loop = {loop} / interp = {interp}: "
                             f"windows inside the clip would be conditioned on all-zero c_concat frames")
        if T_model is None or num_frames < T_model:
            raise ValueError(f"num_frames = {num_frames} is below the model's temporal_length = {T_model}")
        if num_frames > T_model and window_stride is None:
            window_stride = T_model // 2
        noise_shape = list(noise_shape[:2]) + [num_frames] + list(noise_shape[3:])
    if window_stride is not None:
        kwargs.update(window_stride=window_stride, window_weights=window_weights, window_shift=window_shift)
    ddim_sampler = make_sampler(model, sampler, multiple_cond_cfg)
    ddim_sampler.make_schedule(ddim_num_steps=ddim_steps, ddim_discretize=timestep_spacing, ddim_eta=ddim_eta, verbose=False)

    batch_size = noise_shape[0]
    fs = torch.tensor([fs] * batch_size, dtype=torch.long, device=model.device)
    if not text_input:
        prompts = [""] * batch_size

    cond, uc, uc_2 = build_conditioning(model, prompts, videos, unconditional_guidance_scale, cfg_img, multiple_cond_cfg,
                                        loop or interp, num_frames)
    kwargs.update({"unconditional_conditioning_img_nonetext": uc_2})

    batch_variants = []
    for _ in range(n_samples):
        samples, _ = ddim_sampler.sample(S=ddim_steps, conditioning=cond, batch_size=batch_size, shape=noise_shape[1:],
                                         verbose=False, unconditional_guidance_scale=unconditional_guidance_scale,
                                         unconditional_conditioning=uc, eta=ddim_eta, cfg_img=cfg_img, mask=None,
                                         x0=None, fs=fs, timestep_spacing=timestep_spacing,
                                         guidance_rescale=guidance_rescale, **kwargs)
        batch_variants.append(model.decode_first_stage(samples))
    return torch.stack(batch_variants).permute(1, 0, 2, 3, 4, 5)


# ---------------------------------------------------------------------------------------------- prompt folder -> clips
def get_filelist(data_dir, postfixes):
    """scripts/evaluation/funcs.py (and inference.py:26-32): every file of `data_dir` with one of the suffixes, sorted."""
    file_list = []
    for postfix in postfixes:
        file_list.extend(glob.glob(os.path.join(data_dir, f"*.{postfix}")))
    file_list.sort()
    return file_list


def load_prompts(prompt_file):
    """inference.py:61-69: the stripped non-empty lines."""
    with open(prompt_file, "r") as f:
        return [l.strip() for l in f.readlines() if len(l.strip()) != 0]


ResizeGeometry = namedtuple("ResizeGeometry", "rh rw pad_top pad_bottom pad_left pad_right top left")


def resize_geometry(h, w, video_size):
    """Sizes and offsets of torchvision's Resize(min(video_size)) -> CenterCrop(video_size) on an h x w image, restated from
    their documented behaviour. Resize(s): the short side becomes s, the long side int(s * long / short); the width is the short
    side when w <= h. CenterCrop((ch, cw)): an image smaller than the crop on an axis is zero-padded by (c - i) // 2 before and
    (c - i + 1) // 2 after; then top = int(round((H' - ch) / 2.0)), left likewise (Python's round: halves go to even).
    Returns (rh, rw, pad_top, pad_bottom, pad_left, pad_right, top, left); top / left count in the padded image."""
    ch, cw = int(video_size[0]), int(video_size[1])
    s = min(ch, cw)
    if h < 1 or w < 1 or s < 1:
        raise ValueError(f"resize_geometry: image {h} x {w}, video_size {tuple(video_size)}")
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = s, int(s * long / short)
    rw, rh = (new_short, new_long) if w <= h else (new_long, new_short)
    if rh < 1 or rw < 1:
        raise ValueError(f"resize_geometry: {h} x {w} resized to {rh} x {rw}")
    pl, pr = ((cw - rw) // 2, (cw - rw + 1) // 2) if cw > rw else (0, 0)
    pt, pb = ((ch - rh) // 2, (ch - rh + 1) // 2) if ch > rh else (0, 0)
    top = int(round((rh + pt + pb - ch) / 2.0))
    left = int(round((rw + pl + pr - cw) / 2.0))
    return ResizeGeometry(rh, rw, pt, pb, pl, pr, top, left)


def resize_center_crop_f32(img, video_size, antialias=True):
    """torchvision's Resize(min(video_size)) -> CenterCrop(video_size) on a float tensor (scripts/gradio/i2v_test.py:39-42, 65;
    dynamicrafter_pipeline.py:175-178, 286): img fp32 [C, H, W] on the device -> fp32 [C, h, w]. The sizes and offsets are
    `resize_geometry`'s; the resize is interpolate(bilinear, antialias=True) as one or two HIP launches (ops.resize_f32), the
    crop and its padding with 0.0 fused into the last. Not the uint8 path: `preprocess_image` reproduces Pillow on decoded
    pixels, this reproduces what the reference's app classes do to an already normalised tensor."""
    from ... import ops
    g = resize_geometry(img.shape[-2], img.shape[-1], video_size)
    return ops.resize_f32(img, (g.rh, g.rw), crop_hw=(int(video_size[0]), int(video_size[1])),
                          offset=(g.top - g.pad_top, g.left - g.pad_left), antialias=antialias)


class PreprocessPlan:
    """Everything `preprocess_launch` needs for images of one size: the geometry, the tables of the axes that change size (on
    the device) and the extent of the uint8 intermediate between the two passes. Building it uploads; launching does not."""

    def __init__(self, h, w, video_size, device):
        from ... import ops
        self.h, self.w, self.ch, self.cw = int(h), int(w), int(video_size[0]), int(video_size[1])
        self.device = torch.device(device)
        g = self.geometry = resize_geometry(h, w, video_size)
        self.yoff, self.xoff = g.top - g.pad_top, g.left - g.pad_left       # crop pixel -> resized pixel
        self.tab_x = ops.ResizeTables(w, g.rw, self.device) if g.rw != w else None
        self.tab_y = ops.ResizeTables(h, g.rh, self.device) if g.rh != h else None
        # the resized pixels the crop keeps, and through the vertical tables the source rows they need (as Pillow computes only
        # the rows of the horizontal pass that its vertical pass reads)
        self.rx0, self.rx1 = max(self.xoff, 0), min(self.cw + self.xoff, g.rw)
        self.ry0, self.ry1 = max(self.yoff, 0), min(self.ch + self.yoff, g.rh)
        self.y0, self.rows = self.tab_y.span(self.ry0, self.ry1) if self.tab_y is not None else (0, self.h)
        self.two_pass = self.tab_x is not None and self.tab_y is not None
        self.workspace_bytes = self.rows * (self.rx1 - self.rx0) * 3 if self.two_pass else 0


_PLANS = OrderedDict()


def preprocess_plan(h, w, video_size, device):
    """The cached PreprocessPlan (a folder of photos has few distinct sizes; the last 16 are kept)."""
    key = (int(h), int(w), int(video_size[0]), int(video_size[1]), str(torch.device(device)))
    plan = _PLANS.pop(key, None)
    if plan is None:
        plan = PreprocessPlan(h, w, video_size, device)
    _PLANS[key] = plan
    while len(_PLANS) > 16:
        _PLANS.popitem(last=False)
    return plan


def preprocess_launch(plan, img_u8, out, workspace, t0, nt):
    """Enqueues the one or two launches of `plan` on the current stream: img_u8 uint8 [h, w, 3] -> frames t0 .. t0 + nt - 1 of
    out fp32 [3, T, ch, cw]. `workspace`: uint8, at least plan.workspace_bytes (None when that is 0). Allocates nothing and
    does not synchronise, so it can be captured into an ops.DeviceGraph."""
    from ... import ops
    g = plan.geometry
    if tuple(img_u8.shape) != (plan.h, plan.w, 3) or tuple(out.shape[2:]) != (plan.ch, plan.cw):
        raise ValueError(f"preprocess_launch: image {tuple(img_u8.shape)} / clip {tuple(out.shape)} do not match the plan "
                         f"({plan.h} x {plan.w} -> {plan.ch} x {plan.cw})")
    common = dict(resized=(g.rh, g.rw), offset=(plan.yoff, plan.xoff), t0=t0, nt=nt)
    if plan.two_pass:
        cols = plan.rx1 - plan.rx0
        if workspace is None or workspace.numel() < plan.workspace_bytes:
            raise ValueError(f"preprocess_launch: the intermediate needs {plan.workspace_bytes} bytes of workspace")
        ops.prep_resize_h(img_u8, workspace, plan.tab_x, y0=plan.y0, rows=plan.rows, x0=plan.rx0, cols=cols)
        ops.prep_finish(workspace, out, plan.tab_y, axis=2, src_hw=(plan.rows, cols), origin=(plan.y0, plan.rx0), **common)
    elif plan.tab_x is not None:
        ops.prep_finish(img_u8, out, plan.tab_x, axis=1, src_hw=(plan.h, plan.w), origin=(0, 0), **common)
    elif plan.tab_y is not None:
        ops.prep_finish(img_u8, out, plan.tab_y, axis=2, src_hw=(plan.h, plan.w), origin=(0, 0), **common)
    else:
        ops.prep_finish(img_u8, out, None, axis=0, src_hw=(plan.h, plan.w), origin=(0, 0), **common)
    return out


def preprocess_image(img_u8, video_size, video_frames, out=None, t0=0, nt=None):
    """The reference's transform (inference.py:71-76) and frame repetition (:95-108) on decoded pixels: img_u8 uint8 [H, W, 3]
    (a device tensor, or an ndarray that is uploaded to `out`'s device / the current one) -> fp32 [3, video_frames, h, w] in
    [-1, 1] on the device; with `out` given, frames t0 .. t0 + nt - 1 of it are written and the rest is left alone (interp mode
    fills the two halves from two images). HIP path only: a CPU tensor raises RuntimeError."""
    if out is not None and not out.is_cuda:
        raise RuntimeError("preprocess_image runs on the HIP path only (there is no CPU fallback)")
    if isinstance(img_u8, np.ndarray):
        dev = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
        with warnings.catch_warnings():                  # a decoded PIL image is a read-only array; it is only read here
            warnings.simplefilter("ignore", UserWarning)
            img_u8 = torch.from_numpy(np.ascontiguousarray(img_u8)).to(dev)
    if not isinstance(img_u8, torch.Tensor) or not img_u8.is_cuda:
        raise RuntimeError("preprocess_image runs on the HIP path only (there is no CPU fallback)")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3:
        raise ValueError(f"preprocess_image: uint8 [H, W, 3] expected, got {img_u8.dtype} {tuple(img_u8.shape)}")
    img_u8 = img_u8.contiguous()
    ch, cw = int(video_size[0]), int(video_size[1])
    if out is None:
        out = torch.empty((3, video_frames, ch, cw), dtype=torch.float32, device=img_u8.device)
    elif tuple(out.shape) != (3, video_frames, ch, cw) or out.dtype != torch.float32 or out.device != img_u8.device:
        raise ValueError(f"preprocess_image: out must be fp32 [3, {video_frames}, {ch}, {cw}] on {img_u8.device}, got "
                         f"{out.dtype} {tuple(out.shape)} on {out.device}")
    nt = video_frames - t0 if nt is None else nt
    plan = preprocess_plan(img_u8.shape[0], img_u8.shape[1], (ch, cw), img_u8.device)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=img_u8.device) if plan.workspace_bytes else None
    with torch.cuda.device(img_u8.device):
        return preprocess_launch(plan, img_u8, out, ws, t0, nt)


def load_data_prompts(data_dir, video_size=(256, 256), video_frames=16, interp=False, device="cuda"):
    """inference.py:71-113: the first prompt file (sorted by name) and the images of `data_dir` (jpg, png, jpeg, JPEG, PNG;
    sorted), one image per prompt, or images 2 idx and 2 idx + 1 per prompt with `interp` (first image into the first
    video_frames // 2 frames, second into the rest). Returns (filename_list, data_list, prompt_list); data_list[i] is fp32
    [3, video_frames, h, w], here already on `device`. Files are decoded with Pillow; the transform is preprocess_image."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("load_data_prompts resamples on the HIP path only (there is no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    from PIL import Image
    prompt_file = get_filelist(data_dir, ["txt"])
    assert len(prompt_file) > 0, "Error: found NO prompt file!"
    if len(prompt_file) > 1:
        print(f"Warning: multiple prompt files exist. The one {os.path.split(prompt_file[0])[1]} is used.")
    file_list = get_filelist(data_dir, ["jpg", "png", "jpeg", "JPEG", "PNG"])
    prompt_list = load_prompts(prompt_file[0])
    data_list, filename_list = [], []
    half = video_frames // 2

    def decode(path):
        return np.asarray(Image.open(path).convert("RGB"))

    for idx in range(len(prompt_list)):
        clip = torch.empty((3, video_frames, int(video_size[0]), int(video_size[1])), dtype=torch.float32, device=device)
        if interp:
            if 2 * half != video_frames:
                raise ValueError(f"interp needs an even video_frames, got {video_frames}")
            preprocess_image(decode(file_list[2 * idx]), video_size, video_frames, out=clip, t0=0, nt=half)
            preprocess_image(decode(file_list[2 * idx + 1]), video_size, video_frames, out=clip, t0=half, nt=half)
            _, filename = os.path.split(file_list[2 * idx])
        else:
            preprocess_image(decode(file_list[idx]), video_size, video_frames, out=clip)
            _, filename = os.path.split(file_list[idx])
        data_list.append(clip)
        filename_list.append(filename)
    return filename_list, data_list, prompt_list


# ---------------------------------------------------------------------------------------------- driver
def run_inference(args, gpu_num, gpu_no, device=None):
    """inference.py:316-380 for the rank slice `gpu_no` of `gpu_num` of the prompts, on device `gpu_no` as in the reference
    (`device`: another index, for a rank whose local device number differs). Clips go to <savedir>/samples_separate as
    <image stem>_sample<i>.png (APNG), .avi (`--container avi`) or .gif (`--container gif`, no dither); returns the paths
    written."""
    import yaml
    from ... import parallel
    from ...utils.save_video import save_results_seperate
    from ...utils.utils import instantiate_from_config
    with open(args.config) as f:
        config = yaml.safe_load(f)
    model_config = config.pop("model", {})
    model_config["params"]["unet_config"]["params"]["use_checkpoint"] = False
    device = torch.device("cuda", gpu_no if device is None else device)
    torch.cuda.set_device(device)
    model = instantiate_from_config(model_config)
    model = model.to(device)
    model.perframe_ae = args.perframe_ae
    assert os.path.exists(args.ckpt_path), "Error: checkpoint Not Found!"
    model = load_model_checkpoint(model, args.ckpt_path)
    model.eval()

    assert (args.height % 16 == 0) and (args.width % 16 == 0), "Error: image size [h,w] should be multiples of 16!"
    assert args.bs == 1, "Current implementation only support [batch size = 1]!"
    h, w = args.height // 8, args.width // 8
    channels = model.model.diffusion_model.out_channels
    n_frames = args.video_length
    print(f"Inference with {n_frames} frames")
    noise_shape = [args.bs, channels, n_frames, h, w]

    fakedir = os.path.join(args.savedir, "samples")
    os.makedirs(os.path.join(args.savedir, "samples_separate"), exist_ok=True)

    assert os.path.exists(args.prompt_dir), "Error: prompt file Not Found!"
    filename_list, data_list, prompt_list = load_data_prompts(args.prompt_dir, video_size=(args.height, args.width),
                                                              video_frames=n_frames, interp=args.interp, device=device)
    num_samples = len(prompt_list)
    indices = parallel.shard_indices(num_samples, gpu_num, gpu_no)
    print("Prompts testing [rank:%d] %d/%d samples loaded." % (gpu_no, len(indices), num_samples))
    prompt_list_rank = [prompt_list[i] for i in indices]
    data_list_rank = [data_list[i] for i in indices]
    filename_list_rank = [filename_list[i] for i in indices]

    extra = {k: getattr(args, k) for k in ("sampler", "num_frames", "window_stride") if getattr(args, k, None) is not None}
    extra.update(options.options_from_args(args))
    if "tiles" in extra:                                  # --tile gives pixels; the keyword takes latent units
        from ...lvdm.models.samplers.tiles import tiles_from_pixels
        extra["tiles"] = tiles_from_pixels(extra["tiles"], args.height // h)
    save_kw = dict(container=getattr(args, "container", "apng"), quality=getattr(args, "quality", 90))
    written = []
    start = time.time()
    with torch.no_grad():
        for indice in range(0, len(prompt_list_rank), args.bs):
            prompts = prompt_list_rank[indice:indice + args.bs]
            videos = torch.stack(data_list_rank[indice:indice + args.bs], dim=0).to(device)
            filenames = filename_list_rank[indice:indice + args.bs]
            batch_samples = image_guided_synthesis(model, prompts, videos, noise_shape, args.n_samples, args.ddim_steps,
                                                   args.ddim_eta, args.unconditional_guidance_scale, args.cfg_img,
                                                   args.frame_stride, args.text_input, args.multiple_cond_cfg, args.loop,
                                                   args.interp, args.timestep_spacing, args.guidance_rescale,
                                                   args.use_fixed_scheduler, **extra)
            for nn, samples in enumerate(batch_samples):                  # samples: [n_samples, c, t, h, w]
                written += save_results_seperate(prompts[nn], samples, filenames[nn], fakedir, fps=8, loop=args.loop, **save_kw)
    print(f"Saved in {args.savedir}. Time used: {(time.time() - start):.2f} seconds")
    return written


def get_parser():
    """inference.py:383-413, every flag with the reference's default, then this package's own (none changes a default)."""
    parser = argparse.ArgumentParser()
    parser.add_argument("--savedir", type=str, default=None, help="results saving path")
    parser.add_argument("--ckpt_path", type=str, default=None, help="checkpoint path")
    parser.add_argument("--config", type=str, help="config (yaml) path")
    parser.add_argument("--prompt_dir", type=str, default=None, help="a data dir containing videos and prompts")
    parser.add_argument("--n_samples", type=int, default=1, help="num of samples per prompt")
    parser.add_argument("--ddim_steps", type=int, default=50, help="steps of ddim if positive, otherwise use DDPM")
    parser.add_argument("--ddim_eta", type=float, default=1.0, help="eta for ddim sampling (0.0 yields deterministic sampling)")
    parser.add_argument("--bs", type=int, default=1, help="batch size for inference, should be one")
    parser.add_argument("--height", type=int, default=512, help="image height, in pixel space")
    parser.add_argument("--width", type=int, default=512, help="image width, in pixel space")
    parser.add_argument("--frame_stride", type=int, default=3, help="frame stride control for 256 model (larger->larger motion), "
                        "FPS control for 512 or 1024 model (smaller->larger motion)")
    parser.add_argument("--unconditional_guidance_scale", type=float, default=1.0, help="prompt classifier-free guidance")
    parser.add_argument("--seed", type=int, default=123, help="seed for random, numpy and torch; negative draws one")
    parser.add_argument("--video_length", type=int, default=16, help="inference video length")
    parser.add_argument("--negative_prompt", action="store_true", default=False, help="negative prompt")
    parser.add_argument("--text_input", action="store_true", default=False, help="input text to I2V model or not")
    parser.add_argument("--multiple_cond_cfg", action="store_true", default=False, help="use multi-condition cfg or not")
    parser.add_argument("--cfg_img", type=float, default=None, help="guidance scale for image conditioning")
    parser.add_argument("--timestep_spacing", type=str, default="uniform", help="how the timesteps are spaced (Table 2 of "
                        "'Common Diffusion Noise Schedules and Sample Steps are Flawed')")
    parser.add_argument("--guidance_rescale", type=float, default=0.0, help="guidance rescale of the same paper")
    parser.add_argument("--perframe_ae", action="store_true", default=False, help="per-frame AE decoding, saves GPU memory, "
                        "especially for the model of 576x1024")
    parser.add_argument("--use_fixed_scheduler", action="store_true", default=False, help="accepted; the step kernel already "
                        "guards the radicand the fork's fixed scheduler patches")
    parser.add_argument("--loop", action="store_true", default=False, help="generate looping videos or not")
    parser.add_argument("--interp", action="store_true", default=False, help="generate generative frame interpolation or not")
    # not in the reference
    parser.add_argument("--sampler", type=str, default="ddim", choices=("ddim",) + tuple(DPM_SOLVERS), help="sampler")
    parser.add_argument("--container", type=str, default="apng", choices=("apng", "avi", "gif"),
                        help="APNG (lossless), Motion-JPEG AVI or animated GIF (256 colours)")
    parser.add_argument("--quality", type=int, default=90, help="JPEG quality of --container avi")
    parser.add_argument("--num_frames", type=int, default=None, help="clip length in latent frames; above the model's "
                        "temporal_length the sampler denoises overlapping windows")
    parser.add_argument("--window_stride", type=int, default=None, help="stride of those windows (default temporal_length // 2)")
    options.add_option_arguments(parser)
    return parser


# one lookup per option of samplers/options.py: its flags in a parsed namespace as the keyword's dict, or None
freeu_from_args = functools.partial(options.from_args, "freeu")
apg_from_args = functools.partial(options.from_args, "apg")
token_downsampling_from_args = functools.partial(options.from_args, "token_downsampling")


def seed_everything(seed):
    """random, numpy and torch (all devices) from one seed, as pytorch_lightning.seed_everything does (inference.py:425)."""
    random.seed(seed)
    np.random.seed(seed % (1 << 32))
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    return seed


def main(argv=None):
    """inference.py:416-427. Under torch.distributed.run (WORLD_SIZE / RANK / LOCAL_RANK in the environment) this process is
    rank RANK of WORLD_SIZE on device LOCAL_RANK; no process group is formed, as the reference's ddp_wrapper.py issues no
    collective either. Otherwise rank 0 of 1."""
    print("@DynamiCrafter cond-Inference: %s" % datetime.datetime.now().strftime("%Y-%m-%d-%H-%M-%S"))
    args = get_parser().parse_args(argv)
    seed = args.seed
    if seed < 0:
        seed = random.randint(0, 2 ** 31)
    seed_everything(seed)
    gpu_num, rank = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0))
    return run_inference(args, gpu_num, rank, device=int(os.environ.get("LOCAL_RANK", rank)))


if __name__ == "__main__":
    main()
