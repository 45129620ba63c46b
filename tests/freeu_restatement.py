"""FreeU (Si et al., CVPR 2024; diffusers' apply_freeu / fourier_filter) restated in float64 torch, no GPU: what
csrc/freeu.hip, ops.freeu and UNetModel.enable_freeu are tested against (tests/test_freeu_cpu.py, tests/test_freeu_gpu.py).

    skip_filter_fft     the published form: fftshift(fftn(x)) * mask -> ifftn, threshold 1
    skip_filter_real    the same filter as seven sums per plane and a rank-7 update (what the kernels compute)
    backbone_scale      version 1 (constant b) / version 2 (b weighted by the min-max normalised channel mean)
    freeu_stage         which stage acts on an up block, from the width of its h
    unet_forward_freeu  oracle.unet.unet_forward's loop with FreeU ahead of every concat
"""
import math

import torch

from oracle import unet as ounet


def skip_filter_fft(x, s):
    """diffusers.utils.torch_utils.fourier_filter(x, threshold=1, scale=s) on the last two dims, in float64."""
    x = x.to(torch.float64)
    H, W = x.shape[-2:]
    xf = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(x.shape, dtype=torch.float64)
    crow, ccol = H // 2, W // 2
    mask[..., crow - 1:crow + 1, ccol - 1:ccol + 1] = s
    xf = xf * mask
    return torch.fft.ifftn(torch.fft.ifftshift(xf, dim=(-2, -1)), dim=(-2, -1)).real


def skip_basis(H, W):
    """The seven real modes [7, H, W]: 1, cos ty, sin ty, cos tx, sin tx, cos(ty+tx), sin(ty+tx)."""
    ty = (2 * math.pi * torch.arange(H, dtype=torch.float64) / H)[:, None].expand(H, W)
    tx = (2 * math.pi * torch.arange(W, dtype=torch.float64) / W)[None, :].expand(H, W)
    return torch.stack([torch.ones(H, W, dtype=torch.float64), torch.cos(ty), torch.sin(ty), torch.cos(tx), torch.sin(tx),
                        torch.cos(ty + tx), torch.sin(ty + tx)])


def skip_stats(x):
    """[..., H, W] -> [..., 7]: the seven sums over the plane (dc_freeu_skip_stats)."""
    x = x.to(torch.float64)
    return torch.einsum("...yx,kyx->...k", x, skip_basis(*x.shape[-2:]))


def skip_filter_real(x, s):
    """x + (s-1)/(HW) * sum_k stats_k * basis_k."""
    x = x.to(torch.float64)
    H, W = x.shape[-2:]
    return x + (s - 1.0) / (H * W) * torch.einsum("...k,kyx->...yx", skip_stats(x), skip_basis(H, W))


def backbone_factor(h, b, version):
    """h [F, ch, H, W] -> the factor on its first ch/2 channels, [F, 1, H, W]. Version 2: mhat = (m - min_f) / (max_f - min_f)
    with m the mean over all ch channels and min / max per frame; 0 where max_f == min_f (the published code divides by zero)."""
    h = h.to(torch.float64)
    if version == 1:
        return torch.full((h.shape[0], 1) + tuple(h.shape[2:]), float(b), dtype=torch.float64)
    m = h.mean(1, keepdim=True)
    lo = m.amin(dim=(2, 3), keepdim=True)
    hi = m.amax(dim=(2, 3), keepdim=True)
    rng = hi - lo
    mhat = torch.where(rng > 0, (m - lo) / torch.where(rng > 0, rng, torch.ones_like(rng)), torch.zeros_like(m))
    return (b - 1.0) * mhat + 1.0


def backbone_scale(h, b, version):
    h = h.to(torch.float64).clone()
    half = h.shape[1] // 2
    h[:, :half] = h[:, :half] * backbone_factor(h, b, version)
    return h


def freeu_stage(ch, model_channels):
    return 1 if ch == 4 * model_channels else 2 if ch == 2 * model_channels else None


def apply_freeu(h, skip, model_channels, s1, s2, b1, b2, version=1):
    """(h, skip) [F, C, H, W] as diffusers' apply_freeu returns them; float64."""
    stage = freeu_stage(h.shape[1], model_channels)
    if stage is None:
        return h, skip
    b, s = (b1, s1) if stage == 1 else (b2, s2)
    return backbone_scale(h, b, version), skip_filter_real(skip, s)


@torch.no_grad()
def unet_forward_freeu(sd, cfg, x, timesteps, context, fs=None, freeu=None):
    """oracle.unet.unet_forward with FreeU applied to h and hs.pop() ahead of the concat of every up block; freeu = dict(s1, s2,
    b1, b2, version) or None. The loop is unet_forward's, rebuilt from that module's own parts."""
    b, _, t, _, _ = x.shape
    mc = cfg.model_channels
    emb = ounet._mlp(sd, "time_embed", ounet.timestep_embedding(timesteps, mc))
    if context.shape[1] == 77 + t * 16:
        ctx_text, ctx_img = context[:, :77], context[:, 77:]
        ctx_text = ctx_text.repeat_interleave(t, dim=0)
        ctx_img = ctx_img.reshape(b, t, -1, ctx_img.shape[-1]).reshape(b * t, -1, ctx_img.shape[-1])
        context = torch.cat([ctx_text, ctx_img], dim=1)
    else:
        context = context.repeat_interleave(t, dim=0)
    emb = emb.repeat_interleave(t, dim=0)
    h = x.permute(0, 2, 1, 3, 4).reshape(b * t, x.shape[1], x.shape[3], x.shape[4])
    if cfg.fs_condition:
        if fs is None:
            fs = torch.tensor([cfg.default_fs] * b, dtype=torch.long)
        emb = emb + ounet._mlp(sd, "fps_embedding", ounet.timestep_embedding(fs, mc)).repeat_interleave(t, dim=0)
    inp, mid, out = ounet.build_plan(cfg)
    hs = []
    for i, layers in enumerate(inp):
        h = ounet._run_block(sd, f"input_blocks.{i}", layers, h, emb, context, b, cfg)
        if i == 0 and cfg.addition_attention:
            bt, c, hh, ww = h.shape
            h5 = h.reshape(b, t, c, hh, ww).permute(0, 2, 1, 3, 4)
            h5 = ounet.temporal_transformer(sd, "init_attn.0", h5, 8, cfg.num_head_channels, cfg)
            h = h5.permute(0, 2, 1, 3, 4).reshape(bt, c, hh, ww)
        hs.append(h)
    h = ounet._run_block(sd, "middle_block", mid, h, emb, context, b, cfg)
    for i, layers in enumerate(out):
        skip = hs.pop()
        if freeu is not None:
            dt = h.dtype
            h, skip = apply_freeu(h, skip, mc, **freeu)
            h, skip = h.to(dt), skip.to(dt)
        h = torch.cat([h, skip], dim=1)
        h = ounet._run_block(sd, f"output_blocks.{i}", layers, h, emb, context, b, cfg)
    h = torch.nn.functional.silu(ounet._gn(sd, "out.0", h, 1e-5))
    y = torch.nn.functional.conv2d(h, sd["out.2.weight"], sd["out.2.bias"], padding=1)
    return y.reshape(b, t, y.shape[1], y.shape[2], y.shape[3]).permute(0, 2, 1, 3, 4)
