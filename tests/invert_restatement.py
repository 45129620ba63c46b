"""Float64 restatement of the DDIM inversion step (include/dcrafter_hip.h: dc_ddim_invert_step) and of an inversion
loop, on oracle.ddim's schedules; shared by tests/test_invert_cpu.py and tests/test_invert_gpu.py. TEST INFRASTRUCTURE.

Inverse step k takes a latent at level ap[k] = ddim_alphas_prev[k] to level a[k] = ddim_alphas[k], the UNet having seen
the latent at t_src[k] (0 for k = 0, else ddim_timesteps[k - 1], so ap[k] = alphas_cumprod[t_src[k]]). The schedule
values are the fp32 ones the model holds, promoted to float64; all arithmetic is float64."""
import numpy as np
import torch

from oracle import ddim as oddim


def source_timesteps(sched):
    return np.concatenate([[0], sched.ddim_timesteps[:-1]]).astype(np.int64)


def inverse_tables(sched):
    """Per DDIM index k, float64: sqrt(ap), sqrt(1 - ap) (the model's buffers at t_src), sqrt(a), sqrt(1 - a), r."""
    ms = sched.ms
    src = torch.as_tensor(source_timesteps(sched))
    a = sched.tables["a_t"].double()
    t = dict(sa_src=ms.sqrt_alphas_cumprod[src].double(), s1_src=ms.sqrt_one_minus_alphas_cumprod[src].double(),
             sa_dst=a.sqrt(), s1_dst=(1.0 - a).sqrt(), r=torch.ones_like(a))
    if ms.use_dynamic_rescale:
        t["r"] = sched.tables["scale_prev"].double() / sched.tables["scale_t"].double()
    return t


def model_output(e_cond, e_uncond=None, e_img=None, *, cfg_scale=1.0, cfg_img=1.0, guidance_rescale=0.0):
    """CFG combine + guidance rescale as oracle.ddim.p_sample_ddim forms them (ddim.py:226-247, multiplecond :234)."""
    if e_uncond is None:
        return e_cond
    if e_img is not None:
        mo = e_uncond + cfg_img * (e_img - e_uncond) + cfg_scale * (e_cond - e_img)
    else:
        mo = e_uncond + cfg_scale * (e_cond - e_uncond)
    if guidance_rescale > 0.0:
        mo = oddim.rescale_noise_cfg(mo, e_cond, guidance_rescale)
    return mo


def invert_step(sched, x, k, e_cond, e_uncond=None, e_img=None, *, cfg_scale=1.0, cfg_img=1.0, guidance_rescale=0.0,
                tables=None):
    """-> (x_next, pred_x0), float64."""
    t = inverse_tables(sched) if tables is None else tables
    x = x.double()
    dbl = lambda e: None if e is None else e.double()
    mo = model_output(dbl(e_cond), dbl(e_uncond), dbl(e_img), cfg_scale=cfg_scale, cfg_img=cfg_img,
                      guidance_rescale=guidance_rescale)
    sa, s1 = t["sa_src"][k], t["s1_src"][k]
    if sched.ms.parameterization == "v":
        eps = sa * mo + s1 * x
        x0s = sa * x - s1 * mo
    else:
        eps = mo
        x0s = (x - s1 * eps) / sa
    return t["sa_dst"][k] * (x0s / t["r"][k]) + t["s1_dst"][k] * eps, x0s


@torch.no_grad()
def invert_loop(apply_model, sched, x0, cond, uncond=None, *, n, cfg_scale=1.0, guidance_rescale=0.0, uncond_img=None,
                cfg_img=None, trace=None, **model_kwargs):
    """Inverse steps k = 0 .. n - 1 from the clean latent x0; apply_model(x, t_long[b], cond, **model_kwargs)."""
    t = inverse_tables(sched)
    src = source_timesteps(sched)
    x = x0.double()
    for k in range(n):
        tl = torch.full((x.shape[0],), int(src[k]), dtype=torch.long)
        e_c = apply_model(x, tl, cond, **model_kwargs)
        e_u = e_i = None
        if uncond is not None and cfg_scale != 1.0:
            e_u = apply_model(x, tl, uncond, **model_kwargs)
            if uncond_img is not None:
                e_i = apply_model(x, tl, uncond_img, **model_kwargs)
        x, px0 = invert_step(sched, x, k, e_c, e_u, e_i, cfg_scale=cfg_scale,
                             cfg_img=cfg_scale if cfg_img is None else cfg_img, guidance_rescale=guidance_rescale, tables=t)
        if trace is not None:
            trace.append((x, px0))
    return x


def gaussian_denoiser(ms, s):
    """The exact denoiser of data N(0, s^2) under `ms`, as the model's parameterisation (eps or v), float64."""
    acp = ms.alphas_cumprod.double()

    def apply_model(x, t, c=None, **kw):
        a = acp[int(t[0])].item()
        al, sg = np.sqrt(a), np.sqrt(1.0 - a)
        x0 = al * s ** 2 / (a * s ** 2 + 1.0 - a) * x
        # sg = 0 only at t = 0 of no schedule here; with zero-terminal SNR al = 0 at t = 999, where eps = x / sg = x
        eps = (x - al * x0) / sg
        return al * eps - sg * x0 if ms.parameterization == "v" else eps
    return apply_model


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def max_rel(a, b):
    """max |a - b| / max |b|, the measure of dc_dpmpp_step's kernel test."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max())
