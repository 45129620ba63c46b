"""Plain-numpy restatement of the float image resize of csrc/preprocess.hip (dc_resize_f32_h / dc_resize_f32_finish): the
coefficient rule, the two passes, the crop with its 0.0 padding. Scalar loops, no vector tricks: it is what the tests hold both
ops.resize_coeffs_f32 (equality) and the kernels (a rounding tolerance) to, and is itself held to
torch.nn.functional.interpolate on the CPU by tests/test_resize_f32_cpu.py.

The rule with antialias (ATen's window with the triangle filter tri(x) = max(0, 1 - |x|), all in float32):
    scale = n_in / n_out
    support = scale if scale >= 1 else 1;   invscale = 1 / scale in the first case, else 1
    ksize = 2 * ceil(support) + 1
    center = scale * (i + 0.5)
    xmin = max(int(center - support + 0.5), 0);   n = min(int(center + support + 0.5), n_in) - xmin
    w_j = tri((j + xmin - center + 0.5) * invscale) for j < n, normalised to sum 1 (summed tap by tap)
Without antialias the window rule at support 1 gives interpolate's two taps, but torch rounds the position elsewhere
(src = scale * (i + 0.5) - 0.5 is rounded once, as a fused multiply-add, at the magnitude of the coordinate, before its fraction
is taken); from a few hundred pixels on the difference is more than the tolerance (4e-5 at 700 -> 300; 1.9e-5 with the product
and the difference rounded separately), so that mode restates ATen's own order:
    src = max(fma(scale, i + 0.5, -0.5), 0);   i0 = min(floor(src), n_in - 1);   lam = clamp(src - i0, 0, 1)
    taps (i0: 1 - lam, i0 + 1: lam), or the single tap (i0: 1) when i0 is the last pixel;   ksize = 2
"""
import math

import numpy as np

F = np.float32

# (H, W) -> (rh, rw), crop (ch, cw) or None, offset (yoff, xoff): the shape pairs of the tests. The last offset is
# resize_geometry(50, 50, (20, 33)): 13 columns of padding split 6 / 7.
CASES = [
    ("down_37x53_to_16x24", (37, 53), (16, 24), None, (0, 0)),
    ("up_9x7_to_20x33", (9, 7), (20, 33), None, (0, 0)),
    ("vertical_only_128x16_to_16x16", (128, 16), (16, 16), None, (0, 0)),
    ("horizontal_only_16x130_to_16x17", (16, 130), (16, 17), None, (0, 0)),
    ("pad_only_24x24_crop_24x40", (24, 24), (24, 24), (24, 40), (0, -8)),
    ("odd_pad_50x50_to_20x20_crop_20x33", (50, 50), (20, 20), (20, 33), (0, -6)),
    ("two_tiles_12x700_to_5x300", (12, 700), (5, 300), None, (0, 0)),           # more than one tile of the horizontal pass
]
CHANNELS = (1, 3, 4)
TOL = 2e-5          # |x| <= 1, weights sum to 1, <= 17 taps per pass at scale <= 8: ~20 * 2^-23 per pass, two passes, both sides


def coeffs(n_in, n_out, antialias):
    scale = F(n_in) / F(n_out)
    if not antialias:
        k = np.zeros((n_out, 2), dtype=F)
        xmin = np.zeros(n_out, dtype=np.int32)
        n = np.zeros(n_out, dtype=np.int32)
        for i in range(n_out):
            src = max(F(float(scale) * (i + 0.5) - 0.5), F(0.0))       # one rounding (a fused multiply-add in ATen's builds)
            i0 = min(int(math.floor(float(src))), n_in - 1)
            lam = min(max(src - F(i0), F(0.0)), F(1.0))
            if i0 + 1 <= n_in - 1:
                k[i, 0], k[i, 1], n[i] = F(1.0) - lam, lam, 2
            else:
                k[i, 0], n[i] = F(1.0), 1
            xmin[i] = i0
        return k, xmin, n
    aa = scale >= F(1.0)
    support = scale if aa else F(1.0)
    invscale = F(1.0) / scale if aa else F(1.0)
    ksize = int(math.ceil(float(support))) * 2 + 1
    k = np.zeros((n_out, ksize), dtype=F)
    xmin = np.zeros(n_out, dtype=np.int32)
    n = np.zeros(n_out, dtype=np.int32)
    for i in range(n_out):
        center = scale * (F(i) + F(0.5))
        lo = max(int(center - support + F(0.5)), 0)                 # int() truncates, as C's (int) does
        hi = min(int(center + support + F(0.5)), n_in)
        total = F(0.0)
        for j in range(hi - lo):
            a = abs((F(j) + F(lo) - center + F(0.5)) * invscale)
            k[i, j] = max(F(0.0), F(1.0) - a)
            total = total + k[i, j]
        if total != 0:
            k[i] = k[i] / total
        xmin[i], n[i] = lo, hi - lo
    return k, xmin, n


def one_pass(a, k, xmin, n, axis):
    """a fp32 [C, H, W]; the pass along `axis` (1: rows = y, 2: columns = x), float32 multiply-adds in tap order."""
    a = np.moveaxis(a, axis, -1)
    out = np.zeros(a.shape[:-1] + (k.shape[0],), dtype=F)
    for i in range(k.shape[0]):
        acc = np.zeros(a.shape[:-1], dtype=F)
        for j in range(n[i]):
            acc = acc + a[..., xmin[i] + j] * k[i, j]
        out[..., i] = acc
    return np.moveaxis(out, -1, axis)


def resize(img, rh, rw, antialias):
    """fp32 [C, H, W] -> [C, rh, rw]: horizontal pass first; a pass is left out when its axis keeps its size."""
    a = np.asarray(img, dtype=F)
    if rw != a.shape[2]:
        a = one_pass(a, *coeffs(a.shape[2], rw, antialias), axis=2)
    if rh != a.shape[1]:
        a = one_pass(a, *coeffs(a.shape[1], rh, antialias), axis=1)
    return a


def crop_pad(a, ch, cw, yoff, xoff):
    """out[c, oy, ox] = a[c, oy + yoff, ox + xoff], 0.0 outside a."""
    out = np.zeros((a.shape[0], ch, cw), dtype=F)
    for oy in range(ch):
        for ox in range(cw):
            y, x = oy + yoff, ox + xoff
            if 0 <= y < a.shape[1] and 0 <= x < a.shape[2]:
                out[:, oy, ox] = a[:, y, x]
    return out


def resize_crop(img, resized, crop=None, offset=(0, 0), antialias=True):
    a = resize(img, resized[0], resized[1], antialias)
    return a if crop is None and tuple(offset) == (0, 0) else crop_pad(a, *(crop or resized), *offset)


def make_image(c, h, w, seed=0):
    """Uniform in [-1, 1], fixed seed."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(c, h, w)).astype(F)


def torch_reference(img, resized, crop=None, offset=(0, 0), antialias=True):
    """torch.nn.functional.interpolate on the CPU, then the same crop / pad."""
    import torch
    t = torch.from_numpy(np.asarray(img, dtype=F))[None]
    if tuple(resized) != tuple(t.shape[2:]):
        t = torch.nn.functional.interpolate(t, size=tuple(resized), mode="bilinear", align_corners=False, antialias=antialias)
    a = t[0].numpy()
    return a if crop is None and tuple(offset) == (0, 0) else crop_pad(a, *(crop or resized), *offset)
