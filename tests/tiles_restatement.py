"""Float64 restatement of spatially tiled sampling (MultiDiffusion, arXiv:2302.08113, over boxes in space and time),
shared by tests/test_tiles_cpu.py and tests/test_tiles_gpu.py. Written from the formulas, independent of the package's
plan code, of its kernels and of its torch blend:

    starts of an axis at step i   {0} + {d + k stride : 0 < d + k stride < L - n} + {L - n},  d = (i shift) mod stride
    share of window w at f        p(f) / sum over the windows v containing s_w + f of p(s_w + f - s_v), rounded to fp32
                                  p = 1 (uniform) or min(f + 1, n - f) (triangle)
    weight of box position        fl32(fl32(gt[f] gy[y]) gx[x])
    out[F, Y, X]                  sum over the boxes that contain it, in ascending box index, of weight * e_box

The blend takes the fp32 weights as exact numbers; `merge_rows` accumulates in float64 and rounds to fp32 after every
term (what a fused multiply-add chain gives, up to double rounding), `tiled_model` stays in float64 throughout."""
import numpy as np
import torch


def rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def axis_starts(L, n, stride, d):
    last = L - n
    inner = [s for s in range(d, last, stride) if 0 < s < last]
    return [0] + inner + ([last] if last > 0 else [])


def axis_plan(L, n, stride, weights, shift, S):
    """Per step: (starts, shares float32 [len(starts), n]) of one axis. An untiled axis (L == n): start 0, shares 1."""
    out = []
    for i in range(S):
        if L == n:
            out.append(([0], np.ones((1, n), dtype=np.float32)))
            continue
        starts = axis_starts(L, n, stride, (i * shift) % stride)
        f = np.arange(n, dtype=np.float64)
        p = np.ones(n) if weights == "uniform" else np.minimum(f + 1.0, n - f)
        total = np.zeros(L)
        for s in starts:
            total[s:s + n] += p
        out.append((starts, np.stack([p / total[s:s + n] for s in starts]).astype(np.float32)))
    return out


def plan(long_shape, box_shape, stride, weights, shift, S):
    """Per step the list of (start triple, gt, gy, gx) in product-grid order, time slowest."""
    axes = [axis_plan(L, n, st, weights, sh, S) for L, n, st, sh in zip(long_shape, box_shape, stride, shift)]
    steps = []
    for i in range(S):
        (st, gt), (sy, gy), (sx, gx) = (a[i] for a in axes)
        steps.append([((st[a], sy[b], sx[c]), gt[a], gy[b], gx[c])
                      for a in range(len(st)) for b in range(len(sy)) for c in range(len(sx))])
    return steps


def weights3(g_row, box_shape):
    """float32 [T, h, w] from a row (gt | gy | gx) with the two fp32 product roundings in the stated order."""
    T, h, w = box_shape
    g_row = np.asarray(g_row, dtype=np.float32)
    gt, gy, gx = g_row[:T], g_row[T:T + h], g_row[T + h:T + h + w]
    out = np.empty((T, h, w), dtype=np.float32)
    for f in range(T):
        ty = np.float32(gt[f]) * gy                           # float32 * float32 array: rounded to float32
        out[f] = ty[:, None] * gx[None, :]
    assert out.dtype == np.float32
    return out


def coverage(box, g, long_shape, box_shape):
    """float64 [T_long, H_long, W_long]: what the fp32 weights of one step's boxes add up to on every position."""
    T, h, w = box_shape
    cover = np.zeros(long_shape)
    for (t0, y0, x0), row in zip(np.asarray(box).tolist(), g):
        cover[t0:t0 + T, y0:y0 + h, x0:x0 + w] += weights3(row, box_shape).astype(np.float64)
    return cover


def merge_rows(e, box, g, *, nb, B, long_shape, box_shape, C, start=None):
    """e: rows [(k, b, w, f, y, x)][>= C] of the W boxes `box` [W, 3] with weight rows g [W, T + h + w]. Returns
    (out, exact): the blend [nb, B, T_long, H_long, W_long, C] accumulated in float64 and rounded to fp32 after every term
    (the first term a rounded product), in ascending box index with weight-0 boxes skipped, and the same sum without the
    intermediate roundings. `start`: what the output holds ahead of the first term (accumulate), else nothing."""
    T, h, w = box_shape
    W = len(box)
    e = torch.as_tensor(e).double().cpu()[:, :C].reshape(nb, B, W, T, h, w, C).numpy()
    shape = (nb, B) + tuple(long_shape) + (C,)
    out = np.zeros(shape) if start is None else np.asarray(start, dtype=np.float64).reshape(shape).copy()
    exact = out.copy()
    for k, (t0, y0, x0) in enumerate(np.asarray(box).tolist()):
        wt = weights3(g[k], box_shape).astype(np.float64)
        live = (wt != 0)[None, None, :, :, :, None]
        sl = (slice(None), slice(None), slice(t0, t0 + T), slice(y0, y0 + h), slice(x0, x0 + w))
        term = wt[None, None, :, :, :, None] * np.where(live, e[:, :, k], 0.0)      # a skipped term's e is never read
        out[sl] = np.where(live, (out[sl] + term).astype(np.float32).astype(np.float64), out[sl])
        exact[sl] += term
    return out, exact


def ulp_distance(a, b):
    """Per element, how many fp32 numbers lie between a and b (both fp32 arrays), 0 for equal values."""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def tiled_model(fn, steps, box_shape):
    """fn(x [B, C, T, h, w] fp32, (t0, y0, x0)) -> model output of one box; returns g(x_long, step) -> the float64 blend
    over the boxes of `steps[step]` (plan())."""
    T, h, w = box_shape

    def g(x, step):
        out = torch.zeros(x.shape, dtype=torch.float64)
        for (t0, y0, x0), gt, gy, gx in steps[step]:
            wt = torch.from_numpy(weights3(np.concatenate([gt, gy, gx]), box_shape).astype(np.float64))
            e = fn(x[:, :, t0:t0 + T, y0:y0 + h, x0:x0 + w].float().contiguous(), (t0, y0, x0)).double()
            out[:, :, t0:t0 + T, y0:y0 + h, x0:x0 + w] += wt.view(1, 1, T, h, w) * e
        return out
    return g
