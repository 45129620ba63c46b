"""Window plans for temporal co-denoising: clips longer than the UNet's `temporal_length` frames.

At every sampling step the UNet runs on W overlapping T-frame windows of one long latent [B, C, T_long, h, w]; where
windows overlap, their outputs are blended with per-frame weights that sum to one, and the sampler's update then runs
once on the long latent (MultiDiffusion, Bar-Tal et al., arXiv:2302.08113, along time as in Gen-L-Video, Wang et al.,
arXiv:2305.18264). The blend is linear in the model output, so it commutes with CFG and the v / eps / x0 conversions
of a step that has one timestep.

`window_plan` is the host side: pure NumPy, no device. It returns the two per-step tables the kernels
dc_pack_latent_windows and dc_window_merge index by the device step counter.
"""
import numpy as np

WEIGHTS = ("uniform", "triangle")


def window_profile(T, weights="triangle"):
    """The un-normalised float64 weight of frame f of a T-frame window. "triangle" is min(f + 1, T - f): it peaks at
    the window centre and is >= 1 at both ends."""
    if weights not in WEIGHTS:
        raise ValueError(f"window weights must be one of {WEIGHTS}, got {weights!r}")
    f = np.arange(T, dtype=np.float64)
    return np.ones(T) if weights == "uniform" else np.minimum(f + 1.0, T - f)


def _step_starts(T_long, T, stride, d):
    """Window starts of one step whose interior windows are displaced by d (0 <= d < stride): the grid d + k * stride
    below the last start T_long - T, with the first window clamped to frame 0 and the last to the clip's end.
    Consecutive starts differ by at most `stride` <= T, so every frame is covered."""
    last = T_long - T
    starts = [0] + [s for s in range(d, last, stride) if s > 0]
    if last > 0:
        starts.append(last)
    return starts


def window_plan(T_long, T, stride, weights="triangle", shift=0, S=1, multiple_of=1):
    """(starts int32 [S, W], wn float32 [S, W, T]) for S executed steps.

    Step i displaces the interior window starts by (i * shift) mod stride; the first and last windows stay clamped to
    the clip's ends, so with shift > 0 the seams do not sit on the same frames at every step. W is the same at every
    step (one captured step graph has one batch size): the largest count any step needs, rounded up to a multiple of
    `multiple_of` (the windows one UNet call takes). A step that needs fewer windows repeats its last start with
    weight 0. wn is normalised per long frame in float64 and then rounded to fp32: for every step and frame F,
    sum_w wn[s, w, F - starts[s, w]] over the windows that contain F is 1 to within W * 2^-24."""
    T_long, T, stride, shift, S, multiple_of = (int(v) for v in (T_long, T, stride, shift, S, multiple_of))
    if T < 1 or T_long < T:
        raise ValueError(f"the clip has T_long = {T_long} frames, fewer than one window of T = {T}")
    if stride < 1:
        raise ValueError(f"window stride must be >= 1, got {stride}")
    if stride > T:
        raise ValueError(f"window stride {stride} exceeds the window length T = {T}: frames between windows would "
                         f"never be denoised")
    if shift < 0:
        raise ValueError(f"window shift must be >= 0, got {shift}")
    if S < 1 or multiple_of < 1:
        raise ValueError(f"S = {S} and multiple_of = {multiple_of} must be >= 1")
    prof = window_profile(T, weights)
    per_step = [_step_starts(T_long, T, stride, (i * shift) % stride) for i in range(S)]
    W = max(len(s) for s in per_step)
    starts = np.zeros((S, W), dtype=np.int32)
    wn = np.zeros((S, W, T), dtype=np.float32)
    for i, st in enumerate(per_step):
        total = np.zeros(T_long, dtype=np.float64)
        for s in st:
            total[s:s + T] += prof
        starts[i, :len(st)] = st
        starts[i, len(st):] = st[-1]                  # padding: a duplicate of the last window, weight 0
        for w, s in enumerate(st):
            wn[i, w] = (prof / total[s:s + T]).astype(np.float32)
    return pad_plan(starts, wn, multiple_of)


def pad_plan(starts, wn, multiple_of):
    """The plan with W rounded up to a multiple of `multiple_of`: every step repeats its last start, with weight 0."""
    S, W = starts.shape
    extra = -(-W // multiple_of) * multiple_of - W
    if extra == 0:
        return starts, wn
    starts = np.concatenate([starts, np.repeat(starts[:, -1:], extra, axis=1)], axis=1)
    wn = np.concatenate([wn, np.zeros((S, extra, wn.shape[2]), dtype=wn.dtype)], axis=1)
    return np.ascontiguousarray(starts), np.ascontiguousarray(wn)


def windows_per_call(W, cap, per_call=None):
    """How many of W windows one UNet call takes: at most `cap` (the scratch limit) and at most `per_call` (the
    caller's cap, None = none), in equal chunks - the fewest calls, then the fewest windows per call that still make W
    in that many calls (the plan is padded to calls * n_w windows)."""
    W, cap = int(W), int(cap)
    if cap < 1:
        raise ValueError(f"the scratch limit admits {cap} windows per call")
    if per_call is not None and int(per_call) < 1:
        raise ValueError(f"windows_per_call must be >= 1, got {per_call}")
    n_w = min(W, cap if per_call is None else min(int(per_call), cap))
    calls = -(-W // n_w)
    return -(-W // calls)


def check_plan(starts, wn, T_long, T):
    """Refuse tables a kernel must not index with: called on the host copy before upload, since the C entries cannot
    look into device memory. Returns (S, W)."""
    starts, wn = np.asarray(starts), np.asarray(wn)
    if starts.ndim != 2 or wn.shape != starts.shape + (T,):
        raise ValueError(f"window plan: starts {starts.shape} and weights {wn.shape} are not [S, W] and [S, W, {T}]")
    if starts.size == 0:
        raise ValueError("window plan: empty")
    if starts.min() < 0 or starts.max() > T_long - T:
        raise ValueError(f"window plan: starts span [{starts.min()}, {starts.max()}], a window of {T} frames must start "
                         f"in [0, {T_long - T}]")
    if not np.isfinite(wn).all() or wn.min() < 0:
        raise ValueError("window plan: weights must be finite and >= 0")
    for i in range(starts.shape[0]):
        cover = np.zeros(T_long, dtype=np.float64)
        for w, s in enumerate(starts[i]):
            cover[s:s + T] += wn[i, w].astype(np.float64)
        if np.abs(cover - 1.0).max() > starts.shape[1] * 2.0 ** -24 + 1e-12:
            raise ValueError(f"window plan: the weights of step {i} do not sum to 1 on every frame "
                             f"(range [{cover.min()}, {cover.max()}])")
    return int(starts.shape[0]), int(starts.shape[1])
