"""Tile plans for spatially tiled sampling: frames larger than the size the model was trained at.

At every sampling step the UNet runs on W boxes of its own extent (T, h, w) inside one long latent
[B, C, T_long, H_long, W_long]; where boxes overlap, their outputs are blended with weights that sum to one on every
position, and the sampler's update then runs once on the long latent (MultiDiffusion, Bar-Tal et al., arXiv:2302.08113).
The UNet has no spatial position encoding and the conditioning is a global context plus a per-pixel c_concat, so the
blend applies in space exactly as samplers/windows.py applies it in time; with a tiled time axis the two compose.

`tile_plan` is the host side: pure NumPy, no device. The boxes of a step are the product grid of one 1-D `window_plan`
per axis, and the weight of a box position is the product of the three per-axis normalised weights, so it returns the
two per-step tables the kernels dc_pack_latent_tiles and dc_tile_merge index by the device step counter:

    box  int32 [S][W][3]          (t0, y0, x0) of every box
    g    fp32  [S][W][T + h + w]  (gt | gy | gx), the box's three per-axis normalised weight vectors

The blend weight of box position (f, y, x) is fl32(fl32(gt[f] * gy[y]) * gx[x]), in that order.
"""
import numpy as np

from .windows import WEIGHTS, window_plan

AXES = ("time", "height", "width")


def _triple(v, name, fill=None):
    """A per-axis (time, height, width) value: a triple as it is, a (height, width) pair with `fill` for time."""
    v = tuple(int(a) for a in (v if isinstance(v, (tuple, list, np.ndarray)) else (v,) * 3))
    if len(v) == 2 and fill is not None:
        v = (int(fill),) + v
    if len(v) != 3:
        raise ValueError(f"tile {name} must give one value per axis {AXES}, got {v}")
    return v


def _axis_plan(axis, L, n, stride, weights, shift, S):
    """window_plan along one axis; an axis that is not tiled (L == n) has one start, 0, and weights exactly 1.0."""
    if n < 1 or L < n:
        raise ValueError(f"tile plan: the box extent {n} along {axis} exceeds the latent's {L}")
    if shift < 0:
        raise ValueError(f"tile plan: shift along {axis} must be >= 0, got {shift}")
    if L == n:
        return np.zeros((S, 1), dtype=np.int32), np.ones((S, 1, n), dtype=np.float32)
    if stride < 1 or stride > n:
        raise ValueError(f"tile plan: stride {stride} along {axis} must be in 1 .. {n} (the box extent): positions between "
                         f"boxes would never be denoised")
    return window_plan(L, n, stride, weights, shift, S)


def tile_plan(long_shape, box_shape, stride, weights="triangle", shift=(0, 0, 0), S=1, multiple_of=1):
    """(box int32 [S, W, 3], g float32 [S, W, T + h + w]) for S executed steps of boxes `box_shape` = (T, h, w) inside
    `long_shape` = (T_long, H_long, W_long).

    Each axis has its own stride and its own shift (step i displaces the interior starts of an axis by (i * shift) mod
    stride, window_plan's rule) and the same `weights` name. The boxes of a step are the product grid of the per-axis
    windows that carry weight at that step, flat index (wt * Wy + wy) * Wx + wx with that step's own counts. W is the
    same at every step: the largest count any step needs, rounded up to a multiple of `multiple_of` (the boxes one UNet
    call takes); a step that needs fewer repeats its last box with all-zero weights. Each axis is normalised on its own
    (window_plan), which makes the product weights of the boxes containing a position sum to 1 (check_tiles' bound)."""
    long_shape, box_shape = _triple(long_shape, "long_shape"), _triple(box_shape, "box_shape")
    stride, shift = _triple(stride, "stride"), _triple(shift, "shift")
    S, multiple_of = int(S), int(multiple_of)
    if weights not in WEIGHTS:
        raise ValueError(f"tile weights must be one of {WEIGHTS}, got {weights!r}")
    if S < 1 or multiple_of < 1:
        raise ValueError(f"S = {S} and multiple_of = {multiple_of} must be >= 1")
    axes = [_axis_plan(a, L, n, st, weights, sh, S) for a, L, n, st, sh in zip(AXES, long_shape, box_shape, stride, shift)]
    steps = []
    for i in range(S):
        # the windows of each axis that carry weight at this step (window_plan pads an axis with weight-0 duplicates)
        live = [[w for w in range(st.shape[1]) if wn[i, w].any()] for st, wn in axes]
        steps.append([(wt, wy, wx) for wt in live[0] for wy in live[1] for wx in live[2]])
    W = max(len(s) for s in steps)
    box = np.zeros((S, W, 3), dtype=np.int32)
    g = np.zeros((S, W, sum(box_shape)), dtype=np.float32)
    for i, grid in enumerate(steps):
        for k, ws in enumerate(grid):
            box[i, k] = [axes[a][0][i, ws[a]] for a in range(3)]
            g[i, k] = np.concatenate([axes[a][1][i, ws[a]] for a in range(3)])
        box[i, len(grid):] = box[i, len(grid) - 1]        # padding: a duplicate of the last box, weight 0
    return pad_tiles(box, g, multiple_of)


def pad_tiles(box, g, multiple_of):
    """The plan with W rounded up to a multiple of `multiple_of`: every step repeats its last box, with weight 0."""
    S, W, _ = box.shape
    extra = -(-W // multiple_of) * multiple_of - W
    if extra == 0:
        return box, g
    box = np.concatenate([box, np.repeat(box[:, -1:], extra, axis=1)], axis=1)
    g = np.concatenate([g, np.zeros((S, extra, g.shape[2]), dtype=g.dtype)], axis=1)
    return np.ascontiguousarray(box), np.ascontiguousarray(g)


def box_weights(g_row, box_shape):
    """fp32 [T, h, w]: the blend weights of one box from its row of `g`, with the kernel's two fp32 product roundings."""
    T, h, w = box_shape
    gt, gy, gx = (np.asarray(v, dtype=np.float32) for v in (g_row[:T], g_row[T:T + h], g_row[T + h:T + h + w]))
    ty = (gt[:, None] * gy[None, :]).astype(np.float32)
    return (ty[:, :, None] * gx[None, None, :]).astype(np.float32)


def coverage_bound(n_axis):
    """How far from 1 the fp32 product weights of a step may sum on a position, for `n_axis` = (Wt, Wy, Wx) boxes along
    the axes. The weights of axis a sum to 1 + d_a with |d_a| <= W_a 2^-24 (window_plan: each fp32 weight is within half
    an ulp, 2^-24 relative, of a float64 share that sums to 1). Over a product grid the exact products gt gy gx sum to
    (1 + d_t)(1 + d_y)(1 + d_x), and each of the two fp32 product roundings of a weight multiplies its term by
    (1 + e), |e| <= 2^-24 (the weights are far from the subnormal range). Hence
        |sum - 1| <= (1 + Wt u)(1 + Wy u)(1 + Wx u)(1 + u)^2 - 1,   u = 2^-24,
    about (Wt + Wy + Wx + 2) 2^-24; 1e-12 covers the float64 summation of the check itself."""
    u = 2.0 ** -24
    return float(np.prod([1.0 + int(n) * u for n in n_axis]) * (1.0 + u) ** 2 - 1.0 + 1e-12)


def check_tiles(box, g, long_shape, box_shape):
    """Refuse tables a kernel must not index with: called on the host copy before upload, since the C entries cannot look
    into device memory. In float64: the shapes, every start in [0, long - extent] of its axis, weights finite and >= 0,
    and on every position of every step the fp32 product weights (box_weights) of the boxes that contain it sum to 1
    within coverage_bound(the number of distinct starts the step has along each axis). Returns (S, W)."""
    box, g = np.asarray(box), np.asarray(g)
    long_shape, box_shape = _triple(long_shape, "long_shape"), _triple(box_shape, "box_shape")
    if box.ndim != 3 or box.shape[2] != 3 or g.shape != box.shape[:2] + (sum(box_shape),):
        raise ValueError(f"tile plan: box {box.shape} and weights {g.shape} are not [S, W, 3] and [S, W, {sum(box_shape)}]")
    if box.size == 0:
        raise ValueError("tile plan: empty")
    for a, (L, n) in enumerate(zip(long_shape, box_shape)):
        lo, hi = int(box[:, :, a].min()), int(box[:, :, a].max())
        if n < 1 or L < n or lo < 0 or hi > L - n:
            raise ValueError(f"tile plan: starts along {AXES[a]} span [{lo}, {hi}], a box of {n} must start in [0, {L - n}]")
    if not np.isfinite(g).all() or g.min() < 0:
        raise ValueError("tile plan: weights must be finite and >= 0")
    T, h, w = box_shape
    for i in range(box.shape[0]):
        cover = np.zeros(long_shape, dtype=np.float64)
        live = []
        for k, (t0, y0, x0) in enumerate(box[i].tolist()):
            wt = box_weights(g[i, k], box_shape)
            if wt.any():
                live.append((t0, y0, x0))
                cover[t0:t0 + T, y0:y0 + h, x0:x0 + w] += wt.astype(np.float64)
        bound = coverage_bound([len({b[a] for b in live}) for a in range(3)])
        if not live or np.abs(cover - 1.0).max() > bound:
            raise ValueError(f"tile plan: the weights of step {i} do not sum to 1 on every position "
                             f"(range [{cover.min()}, {cover.max()}], bound {bound:.3e})")
    return int(box.shape[0]), int(box.shape[1])


def check_box(box_hw, multiple):
    """Refuse a box the UNet cannot take: its height and width must divide by `multiple`, the UNet's own rule
    (UNetModel.spatial_multiple: one halving per downsampling level, and the skips must meet the decoder's sizes)."""
    h, w = (int(v) for v in box_hw)
    if h < 1 or w < 1 or h % multiple or w % multiple:
        raise ValueError(f"tiles: a box of {h} x {w} latent positions is not one the UNet takes (height and width must be "
                         f"multiples of {multiple})")
    return h, w


def tiles_config(tiles, keys):
    """The `tiles=` keyword (samplers/options.py) with its defaults filled in: size (h, w) in latent units, stride
    (default size // 2 per axis), weights, shift, per_call."""
    cfg = dict(keys, **tiles)
    if cfg.get("size") is None or isinstance(cfg["size"], str) or len(tuple(cfg["size"])) != 2:
        raise ValueError(f"tiles=: size must be (height, width) in latent units, got {cfg.get('size')!r}")
    size = tuple(int(v) for v in cfg["size"])
    stride = cfg["stride"]
    stride = tuple(max(1, v // 2) for v in size) if stride is None else tuple(int(v) for v in stride)
    shift = tuple(int(v) for v in cfg["shift"])
    if len(stride) != 2 or len(shift) != 2:
        raise ValueError(f"tiles=: stride {stride} and shift {shift} must each be a (height, width) pair")
    return dict(size=size, stride=stride, weights=cfg["weights"], shift=shift, per_call=cfg["per_call"])


def tiles_from_pixels(tiles, factor):
    """A `tiles=` dict whose size / stride / shift are in pixels (the command line's units) in latent units: every value
    must be a multiple of the autoencoder's downsampling `factor`."""
    out = dict(tiles)
    for k in ("size", "stride", "shift"):
        if out.get(k) is None:
            continue
        vals = tuple(int(v) for v in out[k])
        if any(v % factor for v in vals):
            raise ValueError(f"--tile{'' if k == 'size' else '_' + k} {vals} must be multiples of {factor} pixels (one latent "
                             f"position)")
        out[k] = tuple(v // factor for v in vals)
    return out
