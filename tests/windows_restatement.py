"""Float64 restatement of windowed sampling (temporal co-denoising: MultiDiffusion, arXiv:2302.08113, along time as in
Gen-L-Video, arXiv:2305.18264), shared by tests/test_windows_gpu.py. Written from the formulas, independent of the
package's kernels and of its torch blend:

    out[F] = sum over the windows w that contain F of wn[w, F - start_w] * e_w[F - start_w]

with wn the plan's fp32 weights taken as exact numbers, every product and sum in float64."""
import numpy as np
import torch


def rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def merge_rows(e, starts, wn, *, nb, B, T_long, HW, C):
    """e: rows [(k, b, w, f, p)][>= C] of the W windows in `starts` [W] with weights wn [W, T]. Returns (out, mag, n):
    the blend [nb, B, T_long, HW, C] in float64, sum_w |wn * e| and the number of windows containing each frame [T_long]
    (the kernel's error bound is (n + 1) 2^-24 mag)."""
    W, T = wn.shape
    e = torch.as_tensor(e).double().cpu()[:, :C].reshape(nb, B, W, T, HW, C).numpy()
    out = np.zeros((nb, B, T_long, HW, C))
    mag = np.zeros_like(out)
    n = np.zeros(T_long, dtype=np.int64)
    for w in range(W):
        s = int(starts[w])
        g = wn[w].astype(np.float64)[None, None, :, None, None]
        out[:, :, s:s + T] += g * e[:, :, w]
        mag[:, :, s:s + T] += np.abs(g * e[:, :, w])
        n[s:s + T] += 1
    return out, mag, n


def windowed_model(fn, starts, wn, T):
    """fn(x [B, C, T, h, w] fp32, window start) -> model output of one window; returns g(x_long, step) -> the float64
    blend over the windows of `step` that carry weight."""
    def g(x, step):
        out = torch.zeros(x.shape, dtype=torch.float64)
        for w, s in enumerate(int(v) for v in starts[step]):
            wt = torch.from_numpy(wn[step, w].astype(np.float64))
            if not bool(wt.any()):
                continue
            e = fn(x[:, :, s:s + T].float().contiguous(), s).double()
            out[:, :, s:s + T] += wt.view(1, 1, T, 1, 1) * e
        return out
    return g


def weight_sums(starts, wn, T_long):
    """[S, T_long] float64: what the fp32-rounded weights of the windows containing a frame add up to (1 + O(2^-24))."""
    S, W, T = wn.shape
    out = np.zeros((S, T_long))
    for i in range(S):
        for w in range(W):
            s = int(starts[i, w])
            out[i, s:s + T] += wn[i, w].astype(np.float64)
    return out
