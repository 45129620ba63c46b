"""Plain-numpy restatement of the input side of the harness (the reference of tests/test_preprocess_gpu.py; its own standing
against Pillow is tests/test_preprocess_cpu.py): Pillow's Image.resize(BILINEAR) on 8-bit channels and torchvision's
Resize(min(video_size)) -> CenterCrop(video_size) -> ToTensor -> Normalize(0.5, 0.5) geometry and arithmetic.

Pillow (Resample.c): per axis, with scale = in / out, fs = max(scale, 1), support = fs, ksize = 2 ceil(support) + 1; per output
xx: center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in), weights
w_i = triangle((i + xmin - center + 0.5) * (1 / fs)) divided by their running sum, k_i = int(0.5 + w_i 2^22); then
out = clamp(((1 << 21) + sum_i in[xmin + i] k_i) >> 22, 0, 255) in int32. Horizontal pass first (only the rows the vertical pass
reads), uint8 between the passes, a pass left out when its axis keeps its size. Written with scalar loops on purpose: the
package vectorises the same tables, and the two are compared."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def _triangle(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def coeffs(n_in, n_out):
    """-> k int32 [n_out, ksize], xmin int32 [n_out], n int32 [n_out]"""
    scale = float(n_in) / n_out
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    k = np.zeros((n_out, ksize), dtype=np.int32)
    xmin_a = np.zeros(n_out, dtype=np.int32)
    n_a = np.zeros(n_out, dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w, ww = [], 0.0
        for x in range(xmax):
            w.append(_triangle((x + xmin - center + 0.5) * ss))
            ww += w[-1]
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        xmin_a[xx], n_a[xx] = xmin, xmax
    return k, xmin_a, n_a


def _pass(a, tab):
    """Resamples axis 0 of a uint8 [L, M, 3] -> uint8 [n_out, M, 3]."""
    k, xmin, n = tab
    out = np.empty((k.shape[0],) + a.shape[1:], dtype=np.uint8)
    for xx in range(k.shape[0]):
        acc = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int32)
        for i in range(int(n[xx])):
            acc += a[xmin[xx] + i].astype(np.int32) * k[xx, i]
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize(a, oh, ow):
    """Image.fromarray(a).resize((ow, oh), Image.BILINEAR) for a uint8 [h, w, 3]."""
    h, w, _ = a.shape
    if ow != w:
        a = _pass(np.ascontiguousarray(a.transpose(1, 0, 2)), coeffs(w, ow)).transpose(1, 0, 2)
    if oh != h:
        a = _pass(np.ascontiguousarray(a), coeffs(h, oh))
    return np.ascontiguousarray(a)


def geometry(h, w, video_size):
    """-> dict(rh, rw, pad = (top, bottom, left, right), top, left): torchvision's Resize(min(video_size)) output size and
    CenterCrop(video_size) padding / offsets (offsets count in the padded image)."""
    ch, cw = video_size
    s = min(ch, cw)
    if w <= h:
        rw, rh = s, int(s * h / w)
    else:
        rh, rw = s, int(s * w / h)
    pl = (cw - rw) // 2 if cw > rw else 0
    pr = (cw - rw + 1) // 2 if cw > rw else 0
    pt = (ch - rh) // 2 if ch > rh else 0
    pb = (ch - rh + 1) // 2 if ch > rh else 0
    top = int(round((rh + pt + pb - ch) / 2.0))
    left = int(round((rw + pl + pr - cw) / 2.0))
    return dict(rh=rh, rw=rw, pad=(pt, pb, pl, pr), top=top, left=left)


def crop_pad(img, video_size, g):
    """CenterCrop(video_size) of the resized uint8 [rh, rw, 3]: zero padding, then the crop."""
    ch, cw = video_size
    pt, pb, pl, pr = g["pad"]
    padded = np.pad(img, ((pt, pb), (pl, pr), (0, 0)))
    return np.ascontiguousarray(padded[g["top"]:g["top"] + ch, g["left"]:g["left"] + cw])


def transform_u8(a, video_size, resize_fn=resize):
    """The uint8 [ch, cw, 3] picture behind the reference's transform of `a`; `resize_fn(a, oh, ow)` = this module's resize,
    or Pillow's."""
    g = geometry(a.shape[0], a.shape[1], video_size)
    return crop_pad(resize_fn(a, g["rh"], g["rw"]), video_size, g)


def make_image(kind, h, w, rng):
    """Test inputs uint8 [h, w, 3]: uniform noise; a smooth ramp plus a checkerboard; all 0; all 255."""
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        base = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), (x + y) * 255.0 / max(h + w - 2, 1)], axis=-1)
        check = (((x // 2) + (y // 3)) % 2 * 60 - 30)[..., None]
        return np.clip(base + check, 0, 255).astype(np.uint8)
    if kind in ("zeros", "ones"):
        return np.full((h, w, 3), 0 if kind == "zeros" else 255, dtype=np.uint8)
    raise ValueError(kind)
