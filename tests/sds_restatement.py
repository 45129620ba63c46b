"""Float64 restatement of the reference's SDS step + torch.optim.Adam / AdamW (guidance_pipeline.py:273-424,
:759-808), shared by tests/test_sds_cpu.py and tests/test_sds_gpu.py. Test helper, not product code."""
import os

import numpy as np
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T, H, W = 4, 8, 8
OPT = {"Adam": ((0.9, 0.999), 1e-8, 0.0), "AdamW": ((0.9, 0.99), 1e-8, 1e-2)}
# tests/golden/make_golden_sds.py's cases: config, UNet extras, optimizer, batch, conditioning seed, rescale, spacing
CASES = {"a": ("inference_256_v1.0.yaml", dict(image_cross_attention_scale_learnable=True), "Adam", 1, 300, 0.0,
               "uniform"),
         "b": ("inference_512_v1.0.yaml", dict(), "AdamW", 2, 310, 0.7, "uniform_trailing"),
         "c": ("inference_512_v1.0.yaml", dict(), "Adam", 2, 320, 0.7, "uniform_trailing")}
DEFAULT_FS = {"inference_256_v1.0.yaml": 3, "inference_512_v1.0.yaml": 24}


def golden():
    return np.load(os.path.join(G, "sds_tiny.npz"), allow_pickle=False)


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def conditioning(tag):
    """The fixture's conditioning, regenerated from its seeds (CPU generator): ctx, uc_ctx, c_concat, fs."""
    cname, _, _, B, seed, _, _ = CASES[tag]
    ctx = rnd(B, 77 + 16 * T, 128, seed=seed)
    cc = rnd(B, 4, T, H, W, seed=seed + 1) * 0.18215
    uctx = rnd(B, 77 + 16 * T, 128, seed=seed + 2)
    return ctx, uctx, cc, torch.tensor([DEFAULT_FS[cname]] * B, dtype=torch.long)


def guidance(e_c, e_u, cfg, phi):
    """_apply_guidance_rescale :326-348 (CFG only with an unconditional branch and cfg > 1)."""
    if e_u is None or not cfg > 1.0:
        return e_c
    e = e_u + cfg * (e_c - e_u)
    if phi > 0:
        dims = tuple(range(1, e_c.ndim))
        st = e_c.std(axis=dims, ddof=1, keepdims=True)
        sc = e.std(axis=dims, ddof=1, keepdims=True)
        e = phi * e * (st / sc) + (1 - phi) * e
    return e


def sds_grad(L, x_t, e, a, weight="t", x0_formula="reference"):
    """grad (before the 1/(B N) of the loss) and d; a = alphas_cumprod[t] per clip, broadcast over the clip."""
    c1, c2 = np.sqrt(a), np.sqrt(1.0 - a)
    with np.errstate(all="ignore"):
        x0 = (x_t - c2 * e) / c1 if x0_formula == "reference" else c1 * x_t - c2 * e
        d = L - x0
        if weight == "t":
            grad = (1.0 - a) * d
        elif weight == "ada":
            wf = np.abs(d).mean(axis=tuple(range(1, d.ndim)), keepdims=True)
            wf = np.where(np.isnan(wf), wf, np.maximum(wf, 1e-4))
            grad = d / wf
        else:
            grad = d
    return np.nan_to_num(grad, nan=0.0, posinf=np.finfo(np.float32).max, neginf=-np.finfo(np.float32).max)


def adam_update(L, m, v, grad, k, lr, opt):
    """torch.optim.Adam / AdamW single-tensor step n = k + 1 on g = grad / (B N); returns L, m, v, loss."""
    (b1, b2), eps, wd = OPT[opt]
    B, N = L.shape[0], L.size
    loss = 0.5 * np.mean(grad * grad) / B
    g = grad / (B * N)
    if wd:
        L = L * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    n = k + 1
    L = L - lr / (1 - b1 ** n) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** n) + eps)
    return L, m, v, loss


def bcast(x, ndim):
    return np.asarray(x, np.float64).reshape((-1,) + (1,) * (ndim - 1))


def restated_trajectory(unet, acp, latent0, ts, noises, ctx, uctx, cc, fs, opt, phi, cfg=7.5, lr=0.05, weight="t",
                        x0_formula="reference"):
    """S steps of SDS + Adam(W) in float64 with `unet(x [B,8,T,H,W] fp32, t [B], ctx) -> [B,4,T,H,W]`; returns the
    latent after every step and the losses."""
    L = np.asarray(latent0, np.float64)
    m, v = np.zeros_like(L), np.zeros_like(L)
    acp = np.asarray(acp, np.float32).astype(np.float64)
    lats, losses = [], []
    for k in range(len(ts)):
        t = np.asarray(ts[k]).astype(np.int64)
        a = bcast(acp[t], L.ndim)
        x_t = np.sqrt(a) * L + np.sqrt(1.0 - a) * np.asarray(noises[k], np.float64)
        xin = torch.cat([torch.from_numpy(x_t).float(), cc], 1)
        tt = torch.from_numpy(t)
        e_c = unet(xin, tt, ctx).double().numpy()
        e_u = unet(xin, tt, uctx).double().numpy()
        grad = sds_grad(L, x_t, guidance(e_c, e_u, cfg, phi), a, weight, x0_formula)
        L, m, v, loss = adam_update(L, m, v, grad, k, lr, opt)
        lats.append(L.copy())
        losses.append(loss)
    return np.stack(lats), np.array(losses)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def maxrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
