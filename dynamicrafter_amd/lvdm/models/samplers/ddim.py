"""DDIMSampler — the reference's sampler API (lvdm/models/samplers/ddim.py:10-317) over the fused HIP step.

`DDIMSampler(model).sample(S, batch_size, shape, conditioning, ..., x_T, unconditional_guidance_scale,
unconditional_conditioning, eta, fs, timestep_spacing, guidance_rescale, **kwargs) -> (samples, intermediates)`
behaves as the reference's, including the 3-branch guidance of ddim_multiplecond.py (pass `cfg_img` and
`unconditional_conditioning_img_nonetext`). Differences by design:
  * per step, the cond / uncond (/ image-only) UNet evaluations run as ONE batched forward
    (`model.apply_model_rows`) and CFG combine + guidance-rescale + v->eps/x0 + dynamic rescale + the DDIM update
    are one fused kernel (dc_ddim_step) instead of ~25 elementwise launches and 6 host->device scalars;
  * per-step scalars live in device tables indexed by a device-side step counter, so one captured hipGraph of
    a step is replayed S times (`use_graph=True`);
  * `noises=` (tensor [S, *x.shape]) injects the per-step Gaussian noise (parity tests); otherwise it is drawn
    with torch.randn on the device as the reference does (common.py:31-34).
  * sqrt(1 - a_prev - sigma^2) is clamped at 0 (the reference can produce NaN there: SURVEY §8 a2).
  * `mask` / `x0` blending (reference :174-180) is one more kernel ahead of the step (dc_mask_blend: q_sample + blend),
    inside the captured graph; `q_noises=` (tensor [S, *x.shape]) injects the q_sample draws (parity tests).
  * `window_stride=` (not in the reference) samples clips longer than the UNet's `temporal_length` by temporal
    co-denoising: `shape`'s frame count is then T_long, the UNet runs on overlapping windows of the long latent and their
    outputs are blended ahead of the unchanged update (samplers/windows.py, WindowedRun below).
  * `encode` (not in the reference, which leaves it as a TODO at :179) is DDIM inversion: InvertRun below, one
    dc_ddim_invert_step per step. `decode` and `ddim_sampling(timesteps=k)` run the last n steps of the schedule on the
    same fused path as `sample` (a FusedRun over the tail of the execution-order tables), DESIGN 4.11.
  * the optional dict keywords of samplers/options.py (not in the reference; None, the default, adds nothing): the model
    settings `freeu=` and `token_downsampling=` on `sample`, `ddim_sampling`, `decode` and `encode` are in force on the UNet
    for that call and the model's previous setting is back afterwards, also when the call raises; the run
    setting `apg=` on `sample`, `ddim_sampling` and `decode` replaces the CFG combine by adaptive projected guidance (Sadat
    et al., ICLR 2025): two launches (ops.apg_guide) between the UNet and the unchanged update, which then takes the guided
    output as its only branch; the running update lives in the run and is zeroed by rewind(). Two branches only, not with
    guidance_rescale (check_apg).
"""
import numpy as np
import torch

from .... import _hip, ops
from ..utils_diffusion import make_ddim_sampling_parameters, make_ddim_timesteps
from . import options
from .options import OPTIONS, takes_model_settings
from .tiles import box_weights, check_box, pad_tiles, tile_plan, tiles_config
from .windows import pad_plan, window_plan, windows_per_call


def _step_inputs(img, S, noises, mask, x0, q_noises, clean_cond, long_branches=None, long_space=False):
    """The per-step draws and the mask operands as the kernels read them, checked in this one place for the fused and
    the generic path: fp32 on the latent's device, `noises` / `q_noises` long enough for S steps, x0 / mask expanded to
    the latent's shape. With windows (`long_branches`: the conditioning branches) everything is T_long frames long, the
    c_concat entries included; with tiles (`long_space`) they have the latent's height and width too. Returns
    (noises, blend); blend is None without a mask."""
    f32 = lambda t: t.to(device=img.device, dtype=torch.float32)
    for k, c in enumerate(long_branches or ()):
        for cc in (c.get("c_concat") or ()) if isinstance(c, dict) else ():
            if long_space and (cc.dim() != img.dim() or tuple(cc.shape[2:]) != tuple(img.shape[2:])):
                raise ValueError(f"tiled sampling: c_concat of branch {k} has shape {tuple(cc.shape)}, the latent is "
                                 f"{tuple(img.shape[2:])} (frames, height, width)")
            if cc.dim() != img.dim() or cc.shape[2] != img.shape[2]:
                raise ValueError(f"windowed sampling: c_concat of branch {k} has shape {tuple(cc.shape)}, the latent has "
                                 f"{img.shape[2]} frames")
    # mask / x0 blending ahead of every step (ddim.py:174-180): the original latent, re-noised to the step's timestep
    # with pre-drawn q_sample noise [S, ...] unless clean_cond
    blend = None
    if mask is not None:
        assert x0 is not None
        if not clean_cond and q_noises is None:
            q_noises = torch.randn((S,) + tuple(img.shape), device=img.device)
        blend = dict(x0=f32(x0).expand_as(img).contiguous(), mask=f32(mask).expand_as(img).contiguous(),
                     clean=bool(clean_cond), q=None if clean_cond else f32(q_noises).contiguous())
    if noises is not None:
        noises = f32(noises).contiguous()
    for name, t in (("noises", noises), ("q_noises", blend and blend["q"])):
        if t is not None and t.numel() < S * img.numel():
            raise ValueError(f"{name}: the step kernels read step index * {img.numel()} + i for {S} steps; "
                             f"got {t.numel()} elements")
    return noises, blend


APG_DEFAULTS = OPTIONS["apg"].keys


def apg_config(apg):
    """The validated, completed copy of an `apg=` dict (keys of APG_DEFAULTS), or None for None."""
    if apg is None:
        return None
    options.check_keys(OPTIONS["apg"], apg)
    cfg = dict(APG_DEFAULTS, **apg)
    for k in ("eta", "momentum", "norm_threshold"):
        v = cfg[k]
        if k == "norm_threshold" and v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v):
            raise ValueError(f"apg=: {k} must be a finite number{' or None' if k == 'norm_threshold' else ''}, got {v!r}")
        cfg[k] = float(v)
    if cfg["space"] not in ops.APG_SPACES:
        raise ValueError(f"apg=: space must be one of {ops.APG_SPACES}, got {cfg['space']!r}")
    return cfg


def check_apg(apg, sampler, n_branches, guidance_rescale, three_branch, last=None):
    """What adaptive projected guidance cannot be combined with, refused before any GPU work; returns apg_config(apg).
    `last`: the run covers the last `last` steps of the sampler's schedule only (all of them: None)."""
    apg = apg_config(apg)
    if apg is None:
        return None
    if three_branch or n_branches > 2:
        raise ValueError("apg= is defined for two guidance branches: not with unconditional_conditioning_img_nonetext / cfg_img")
    if n_branches < 2:
        raise ValueError("apg= needs classifier-free guidance: an unconditional_conditioning and a guidance scale other than 1")
    if guidance_rescale > 0:
        raise ValueError("apg= replaces guidance_rescale (both counter the saturation of high guidance scales): pass "
                         "guidance_rescale=0 with it")
    if apg["space"] == "x0" and sampler.model.parameterization != "v":
        a = np.asarray(sampler.ddim_alphas, dtype=np.float64)       # ascending DDIM index; a run's steps are the first `last`
        a = a if last is None else a[:int(last)]
        if not (a > 0).all():
            raise ValueError("apg= with space='x0' on an eps model needs a_t > 0 at every step (x0 = (x - sqrt(1-a_t) eps) / "
                             "sqrt(a_t)); this schedule reaches a_t = 0: use space='model'")
    return apg


def apg_generic(tables, apg, state, e_c, e_u, x, w, *, v_param, index):
    """Adaptive projected guidance on the generic path: the kernels of the fused path (ops.apg_guide) on the [B, C, ...]
    outputs of separate apply_model calls, at executed step `index` of `tables`. `state`: a dict that carries the running
    update and the scratch from call to call (the sampling loop holds one per call; None: a single first step). Returns the
    guided output, which the update then takes as its only branch."""
    st = {} if state is None else state
    geo = dict(B=x.shape[0], Cc=x.shape[1], THW=int(np.prod(x.shape[2:])))
    if "m" not in st:
        st.update(m=torch.zeros_like(x), out=torch.empty_like(x),
                  ws=torch.empty(ops.apg_workspace_floats(**geo), dtype=torch.float32, device=x.device))
    return ops.apg_guide(tables, e_c, e_u, x, st["m"], st["out"], st["ws"], cfg_scale=float(w), v_param=v_param, index=index,
                         e_nchw=True, **geo, **apg)


def _update_kw(m, x, cfg_scale, cfg_img, guidance_rescale, temperature, **extra):
    """The keyword arguments ops.ddim_step and ops.dpmpp_step share, for a latent x [B, C, ...]."""
    return dict(B=x.shape[0], Cc=x.shape[1], THW=int(np.prod(x.shape[2:])), v_param=m.parameterization == "v",
                cfg_scale=cfg_scale, cfg_img=cfg_scale if cfg_img is None else cfg_img,
                guidance_rescale=guidance_rescale, temperature=temperature, **extra)


class StepRun:
    """What every fused run owns: the latent `img` (updated in place), the batched guidance branches, the step
    workspace, the device step counter with the [S, nb*B] timestep table it indexes, and optionally the captured
    hipGraph of a step. A subclass supplies `_enqueue()`, the launches of one step (no allocation, no host sync,
    ending in ops.advance_counter), and `_reset_state()`, which puts back whatever else a step changes besides the
    latent and the counter. `step()` advances the device counter by one; after `S` steps `rewind()` starts over."""

    def __init__(self, model, img, branches, t_table, fs=None, windows=None, tiles=None):
        self.model, self.img = model, img
        self.S = int(t_table.shape[0])
        self.nb = len(branches)
        t_table = t_table.to(torch.int64)
        if windows is None and tiles is None:
            self.prep = model.prepare_branches(tuple(img.shape), branches, fs=fs)
        elif tiles is None:                             # the UNet batch is (branch, clip, window): WindowedRun
            self.prep = model.prepare_branches(tuple(img.shape), branches, fs=fs, windows=windows)
            t_table = t_table.repeat_interleave(int(windows["n_w"]), dim=1)
        else:                                           # the UNet batch is (branch, clip, box): TiledRun
            self.prep = model.prepare_branches(tuple(img.shape), branches, fs=fs, tiles=tiles)
            t_table = t_table.repeat_interleave(int(tiles["n_w"]), dim=1)
        self.ws = ops.step_workspace(img.shape[0], img.device)
        self.counter = torch.zeros(1, dtype=torch.int32, device=img.device)
        self.t_table = t_table.repeat(1, self.nb).contiguous().to(img.device)   # [S, B] -> [S, nb*B]
        self.graph = None
        self.steps_done = 0

    def _reset_state(self):
        pass

    def _restart(self, img):
        self.counter.zero_()
        self.steps_done = 0
        self._reset_state()
        if img is not None:
            self.img.copy_(img)
        torch.cuda.synchronize()

    def capture(self):
        """Warm up once eagerly (allocates all scratch), restore the state, capture one step into a hipGraph."""
        keep = self.img.clone()
        self._enqueue()
        torch.cuda.synchronize()
        self._restart(keep)
        self.graph = ops.DeviceGraph().capture(self._enqueue)
        return self

    def step(self):
        # the kernels index the per-step tables, the timestep table and the pre-drawn noise by the device counter
        if self.steps_done >= self.S:
            raise RuntimeError(f"{type(self).__name__}: all {self.S} steps have run; rewind() first")
        if self.graph is not None:
            self.graph.launch()
        else:
            self._enqueue()
        self.steps_done += 1

    def _split(self, e):
        """The branch-major rows `e` [nb * M, C] of a model evaluation as (e_c, e_u, e_i); None for a branch the run lacks."""
        M = self.kw["B"] * self.kw["THW"]
        return e[:M], e[M:2 * M] if self.nb > 1 else None, e[2 * M:3 * M] if self.nb > 2 else None

    def rewind(self, x_T=None):
        """Start over: the counter and the subclass's state to their initial values; optionally a new initial latent."""
        self.sync()
        self._restart(x_T)

    def sync(self):
        """Wait for the issued steps, then read the library's error word: a kernel whose bounded LDS-counter wait timed out
        (csrc/gemm_pipe.h) has produced garbage, and that must not leave the sampler silently."""
        if self.graph is not None:
            self.graph.sync()
        else:
            torch.cuda.current_stream().synchronize()
        _hip.check_error_word(f"{type(self).__name__}.sync")


class FusedRun(StepRun):
    """One fused sampling run: per step [mask blend +] batched UNet + the sampler's update kernel (`_update`: the fused
    DDIM step here, dc_dpmpp_step in samplers/dpm_solver.py), which leaves x_prev in `img` and the step's `pred_x0`."""

    def __init__(self, sampler, img, branches, *, fs=None, noises=None, cfg_scale=1.0, cfg_img=None,
                 guidance_rescale=0.0, temperature=1.0, mask=None, x0=None, q_noises=None, clean_cond=False,
                 windows=None, tiles=None, last=None, apg=None):
        # `last`: a partial run over the last n steps of the schedule (decode, timesteps=): the execution-order tables and
        # the timestep table are sliced, so the counter still starts at 0 and noises / q_noises are [n, ...]
        S_all = int(sampler._exec_timesteps.shape[0])
        n = S_all if last is None else int(last)
        if not 1 <= n <= S_all:
            raise ValueError(f"a partial run covers 1 .. {S_all} steps, got {n}")
        if n < S_all and windows is not None:
            raise ValueError("partial runs are not implemented with windows")
        if n < S_all and tiles is not None:
            raise ValueError("partial runs are not implemented with tiles")
        # `apg`: adaptive projected guidance (apg_config's dict) in place of the CFG combine: two launches between the UNet
        # and the unchanged update, which then sees the guided rows as a single branch
        apg = check_apg(apg, sampler, len(branches), guidance_rescale, cfg_img is not None, last=n)
        t_host = torch.as_tensor(sampler._exec_timesteps[S_all - n:].copy(), dtype=torch.int64)
        super().__init__(sampler.model, img, branches, t_host[:, None].expand(-1, img.shape[0]), fs=fs, windows=windows,
                         **({} if tiles is None else {"tiles": tiles}))
        self.sampler = sampler
        self.tables = sampler._tables if n == S_all else \
            {k: v[S_all - n:] for k, v in sampler._tables.items() if not k.startswith("inv_")}
        self.noises, self.blend = _step_inputs(img, self.S, noises, mask, x0, q_noises, clean_cond,
                                               long_branches=None if windows is None and tiles is None else branches,
                                               long_space=tiles is not None)
        self.pred_x0 = torch.empty_like(img)
        self.apg = apg
        if apg is None:
            self.kw = _update_kw(self.model, img, cfg_scale, cfg_img, guidance_rescale, temperature,
                                 noise_step_stride=img.numel())
        else:
            # the update takes the guided rows as its only branch
            self.kw = _update_kw(self.model, img, 1.0, None, 0.0, temperature, noise_step_stride=img.numel())
            geo = {k: self.kw[k] for k in ("B", "Cc", "THW")}
            self.apg_kw = dict(geo, v_param=self.kw["v_param"], cfg_scale=float(cfg_scale), **apg)
            self.apg_m = torch.zeros_like(img)          # the running update m, zero ahead of the first step
            self.apg_out = torch.empty((geo["B"] * geo["THW"], geo["Cc"]), dtype=torch.float32, device=img.device)
            self.apg_ws = torch.empty(ops.apg_workspace_floats(**geo), dtype=torch.float32, device=img.device)

    def _reset_state(self):
        if self.apg is not None:
            self.apg_m.zero_()                          # capture()'s eager warm-up step wrote it

    def _enqueue(self):
        if self.blend is not None:
            b = self.blend
            ops.mask_blend(self.img, b["x0"], b["mask"], b["q"], self.tables, step_index=self.counter,
                           clean=b["clean"], noise_step_stride=self.img.numel())
        e_c, e_u, e_i = self._split(self._evaluate())
        if self.apg is None:
            self._update(e_c, e_u, e_i)
        else:
            self._update(ops.apg_guide(self.tables, e_c, e_u, self.img, self.apg_m, self.apg_out, self.apg_ws,
                                       step_index=self.counter, **self.apg_kw), None, None)
        ops.advance_counter(self.counter)

    def _evaluate(self):
        """The raw model output of every branch on the latent: fp32 rows [nb * B * THW, C], branch-major."""
        return self.model.apply_model_rows(self.img, self.prep, self.t_table, t_index=self.counter)

    def _update(self, e_c, e_u, e_i):
        ops.ddim_step(self.tables, e_c, e_u, e_i, self.img, self.noises, self.img, self.pred_x0, self.ws,
                      step_index=self.counter, **self.kw)


_INVERT_TABLES = ("inv_sqrt_a_src", "inv_sqrt_1ma_src", "inv_sqrt_a_dst", "inv_sqrt_1ma_dst", "inv_scale_ratio")


def _invert_kw(m, x, cfg_scale, cfg_img, guidance_rescale, **extra):
    kw = _update_kw(m, x, cfg_scale, cfg_img, guidance_rescale, 1.0, **extra)
    del kw["temperature"]                               # an inversion draws no noise
    return kw


class InvertRun(StepRun):
    """One fused DDIM inversion run over the DDIM indices k = 0 .. n - 1, in that order: per step the batched UNet on the
    latent at the source level's own timestep (`sampler._inv_timesteps`) + dc_ddim_invert_step, which leaves the latent
    of the next level in `img` and the step's `pred_x0`. The tables are in ascending k already, so the counter indexes
    them as they are."""

    def __init__(self, sampler, img, branches, n, *, fs=None, cfg_scale=1.0, cfg_img=None, guidance_rescale=0.0):
        S_all = int(sampler._inv_timesteps.shape[0])
        if not 1 <= int(n) <= S_all:
            raise ValueError(f"an inversion covers 1 .. {S_all} steps, got {n}")
        t_host = torch.as_tensor(sampler._inv_timesteps[:int(n)].copy(), dtype=torch.int64)
        super().__init__(sampler.model, img, branches, t_host[:, None].expand(-1, img.shape[0]), fs=fs)
        self.sampler = sampler
        self.tables = {k: sampler._tables[k][:int(n)] for k in _INVERT_TABLES if k in sampler._tables}
        self.pred_x0 = torch.empty_like(img)
        self.kw = _invert_kw(self.model, img, cfg_scale, cfg_img, guidance_rescale)

    def _enqueue(self):
        e = self.model.apply_model_rows(self.img, self.prep, self.t_table, t_index=self.counter)
        ops.ddim_invert_step(self.tables, *self._split(e), self.img, self.img, self.pred_x0, self.ws,
                             step_index=self.counter, **self.kw)
        ops.advance_counter(self.counter)


class WindowedRun:
    """Mixin ahead of FusedRun or a subclass of it (`windowed(cls)`): the latent is a clip of T_long > T frames and the
    model evaluation of a step is, per chunk of `n_w` windows, window pack per branch + one batched UNet forward with
    B_eff = nb * B * n_w + blend into the long output rows. Mask blend, the sampler's update (`_update`, unchanged, on
    T_long * HW positions), the counter, capture / step / rewind / sync are the base run's. The window starts and blend
    weights are two more device tables indexed by the step counter, so one captured step graph serves windows that
    move from step to step.

    window = dict(T=, stride=, weights=, shift=, per_call=): per_call caps the windows of one UNet call (None: the most
    that keeps every scratch buffer under 2^31 elements); the plan is padded to whole calls with weight-0 windows."""

    def __init__(self, sampler, img, branches, *, window, **kw):
        model = sampler.model
        T, nb, S = int(window["T"]), len(branches), int(sampler._exec_timesteps.shape[0])
        plan = window.get("plan")                       # ddim_sampling has built it already (argument checks)
        if plan is None:
            plan = window_plan(img.shape[2], T, window["stride"], window.get("weights", "triangle"),
                               window.get("shift", 0), S)
        W = plan[0].shape[1]
        n_w = windows_per_call(W, model.max_windows_per_call(tuple(img.shape), nb, T), window.get("per_call"))
        starts, wn = pad_plan(*plan, n_w)
        super().__init__(sampler, img, branches, windows=dict(T=T, n_w=n_w), **kw)
        self.plan = ops.window_tables(starts, wn, T_long=img.shape[2], T=T, device=img.device)
        rows = nb * img.shape[0] * int(np.prod(img.shape[2:]))
        self.e_long = torch.empty((rows, model.model.diffusion_model.out_channels), dtype=torch.float32, device=img.device)

    def _evaluate(self):
        return self.model.apply_model_windows(self.img, self.prep, self.t_table, self.plan, self.e_long,
                                              t_index=self.counter)


_windowed_classes = {}


def windowed(run_class):
    """The windowed form of a FusedRun class (FusedRun itself, DpmRun): WindowedRun mixed in ahead of it."""
    if run_class not in _windowed_classes:
        _windowed_classes[run_class] = type("Windowed" + run_class.__name__, (WindowedRun, run_class), {})
    return _windowed_classes[run_class]


class _WindowedModel:
    """The generic path's windows: a stand-in for the model whose apply_model evaluates the wrapped model on every
    window of the current step (`step`, set by the sampling loop) and blends the outputs with the same plan tables,
    in plain torch indexing on the device. Every other attribute is the wrapped model's."""

    def __init__(self, model, starts, wn, T, device):
        self._m, self._starts, self._T = model, starts, T
        self._wn = torch.from_numpy(wn).to(device)
        self.step = 0

    def __getattr__(self, name):
        return getattr(self._m, name)

    def apply_model(self, x, t, c, **kw):
        T, out = self._T, None
        for w, s in enumerate(int(v) for v in self._starts[self.step]):
            g = self._wn[self.step, w]
            if not bool((g != 0).any()):
                continue                                # padding / duplicate window
            cw = c
            if isinstance(c, dict) and c.get("c_concat") is not None:
                cw = dict(c, c_concat=[cc[:, :, s:s + T].contiguous() for cc in c["c_concat"]])
            e = self._m.apply_model(x[:, :, s:s + T].contiguous(), t, cw, **kw).to(torch.float32)
            if out is None:
                out = torch.zeros(x.shape[:1] + e.shape[1:2] + x.shape[2:], dtype=torch.float32, device=x.device)
            # dc_window_merge's order and roundings, in ascending w: the product of two fp32 numbers is exact in float64;
            # the sum is then rounded to float64 and to fp32. That is a fused multiply-add except where the float64 sum
            # lands within 2^-29 ulp of a midpoint between two fp32 numbers (double rounding, about one term in 10^8), so the
            # two paths agree bitwise on almost every element, not by construction on all: with other inputs or another
            # toolchain a last-bit difference can appear
            seg = out[:, :, s:s + T]
            seg.copy_((seg.double() + g.double().view(1, 1, T, 1, 1) * e.double()).float())
        return out


class TiledRun:
    """Mixin ahead of FusedRun or a subclass of it (`tiled(cls)`), WindowedRun's sibling in space: the latent is larger
    than the box (T, h, w) one UNet call is made for, and the model evaluation of a step is, per chunk of `n_w` boxes, box
    pack per branch + one batched UNet forward with B_eff = nb * B * n_w at the box's size + blend into the long output
    rows (LatentDiffusion.apply_model_tiles). Mask blend, APG, the sampler's update (`_update`, unchanged, on
    T_long * H_long * W_long positions, guidance-rescale statistics per clip over the whole latent), the counter and
    capture / step / rewind / sync are the base run's. The box starts and the per-axis blend weights are two more device
    tables indexed by the step counter (samplers/tiles.py), so one captured step graph serves boxes that move from step to
    step. With a tiled time axis (`window_stride` beside `tiles`) the boxes are the product plan.

    tile = dict(T=, h=, w=, stride=(st, sy, sx), weights=, shift=(dt, dy, dx), per_call=[, plan=]): per_call caps the boxes
    of one UNet call (None: the most that keeps every scratch buffer under 2^31 elements); the plan is padded to whole
    calls with weight-0 boxes."""

    def __init__(self, sampler, img, branches, *, tile, **kw):
        model = sampler.model
        box_shape = (int(tile["T"]), int(tile["h"]), int(tile["w"]))
        nb, S = len(branches), int(sampler._exec_timesteps.shape[0])
        plan = tile.get("plan")                         # _denoise has built it already (argument checks)
        if plan is None:
            plan = tile_plan(tuple(img.shape[2:]), box_shape, tile["stride"], tile.get("weights", "triangle"),
                             tile.get("shift", (0, 0, 0)), S)
        W = plan[0].shape[1]
        cap = model.max_windows_per_call(tuple(img.shape), nb, box_shape[0], hw=box_shape[1:])
        n_w = windows_per_call(W, cap, tile.get("per_call"))
        box, g = pad_tiles(*plan, n_w)
        super().__init__(sampler, img, branches, tiles=dict(T=box_shape[0], h=box_shape[1], w=box_shape[2], n_w=n_w), **kw)
        self.plan = ops.tile_tables(box, g, long_shape=tuple(img.shape[2:]), box_shape=box_shape, device=img.device)
        rows = nb * img.shape[0] * int(np.prod(img.shape[2:]))
        self.e_long = torch.empty((rows, model.model.diffusion_model.out_channels), dtype=torch.float32, device=img.device)

    def _evaluate(self):
        return self.model.apply_model_tiles(self.img, self.prep, self.t_table, self.plan, self.e_long,
                                            t_index=self.counter)


_tiled_classes = {}


def tiled(run_class):
    """The tiled form of a FusedRun class (FusedRun itself, DpmRun): TiledRun mixed in ahead of it."""
    if run_class not in _tiled_classes:
        _tiled_classes[run_class] = type("Tiled" + run_class.__name__, (TiledRun, run_class), {})
    return _tiled_classes[run_class]


class _TiledModel:
    """The generic path's tiles, in the manner of _WindowedModel: a stand-in for the model whose apply_model evaluates
    the wrapped model on every box of the current step (`step`, set by the sampling loop) that carries weight and blends
    the outputs with the same plan tables, in plain torch indexing on the device. Every other attribute is the wrapped
    model's."""

    def __init__(self, model, box, g, box_shape, device):
        self._m, self._box, self._g, self._shape, self._dev = model, box, g, tuple(box_shape), device
        self.step = 0

    def __getattr__(self, name):
        return getattr(self._m, name)

    def apply_model(self, x, t, c, **kw):
        (T, h, w), out = self._shape, None
        for k, (t0, y0, x0) in enumerate(self._box[self.step].tolist()):
            wt = box_weights(self._g[self.step, k], self._shape)     # dc_tile_merge's two fp32 product roundings
            if not wt.any():
                continue                                # padding box
            crop = lambda v: v[:, :, t0:t0 + T, y0:y0 + h, x0:x0 + w].contiguous()
            cw = c
            if isinstance(c, dict) and c.get("c_concat") is not None:
                cw = dict(c, c_concat=[crop(cc) for cc in c["c_concat"]])
            e = self._m.apply_model(crop(x), t, cw, **kw).to(torch.float32)
            if out is None:
                out = torch.zeros(x.shape[:1] + e.shape[1:2] + x.shape[2:], dtype=torch.float32, device=x.device)
            # dc_tile_merge's order and roundings, in ascending box index, through float64 as _WindowedModel does (a fused
            # multiply-add except for rare double roundings)
            seg = out[:, :, t0:t0 + T, y0:y0 + h, x0:x0 + w]
            seg.copy_((seg.double() + torch.from_numpy(wt).to(self._dev).double().view(1, 1, T, h, w) * e.double()).float())
        return out


class DDIMSampler(object):
    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.counter = 0
        self._graph = None
        self._graph_key = None

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    # ------------------------------------------------------------------ schedule (host, once per call)
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        m = self.model
        self.ddim_timesteps = make_ddim_timesteps(ddim_discr_method=ddim_discretize, num_ddim_timesteps=ddim_num_steps,
                                                  num_ddpm_timesteps=self.ddpm_num_timesteps, verbose=verbose)
        acp = m.alphas_cumprod.detach().float().cpu()
        assert acp.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        dev = m.device
        if getattr(m, "use_dynamic_rescale", False):
            sa = m.scale_arr.detach().cpu()[self.ddim_timesteps]
            self.ddim_scale_arr = sa
            self.ddim_scale_arr_prev = torch.cat([sa[0:1], sa[:-1]])
        sig, a, a_prev = make_ddim_sampling_parameters(alphacums=acp, ddim_timesteps=self.ddim_timesteps, eta=ddim_eta,
                                                       verbose=verbose)
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev = sig, a, a_prev
        self.ddim_sqrt_one_minus_alphas = np.sqrt(1. - a.numpy())
        for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
                  "sqrt_one_minus_alphas_cumprod"):
            setattr(self, k, getattr(m, k).detach().float().to(dev))
        # fp32 tables in EXECUTION order (step i uses DDIM index S-1-i): what torch.full(size, v) would hold
        S = self.ddim_timesteps.shape[0]
        order = np.arange(S)[::-1].copy()
        f32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float64)).float()[order].contiguous().to(dev)
        ts = torch.as_tensor(self.ddim_timesteps.copy(), dtype=torch.long)
        t = {"a_t": a.float()[order].contiguous().to(dev), "a_prev": f32(a_prev), "sigma_t": f32(sig.numpy()),
             "sqrt_one_minus_at": torch.as_tensor(self.ddim_sqrt_one_minus_alphas)[order].contiguous().to(dev),
             "sqrt_acp_t": m.sqrt_alphas_cumprod.detach().float().cpu()[ts][order].contiguous().to(dev),
             "sqrt_1macp_t": m.sqrt_one_minus_alphas_cumprod.detach().float().cpu()[ts][order].contiguous().to(dev)}
        if getattr(m, "use_dynamic_rescale", False):
            t["scale_ratio"] = (self.ddim_scale_arr_prev / self.ddim_scale_arr)[order].contiguous().to(dev)
        # inversion (encode): step k takes the latent from level a_prev[k] up to a[k] after a UNet call at the source level's
        # own timestep t_src[k] (0 for k = 0, else ddim_timesteps[k - 1], so a_prev[k] = alphas_cumprod[t_src[k]]). Tables in
        # ASCENDING k, which is an inversion's execution order; float64 on the host, cast once
        self._inv_timesteps = np.concatenate([[0], self.ddim_timesteps[:-1]]).astype(np.int64)
        src = torch.as_tensor(self._inv_timesteps)
        up = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float64)).float().contiguous().to(dev)
        a64 = a.double().numpy()
        t.update(inv_sqrt_a_src=m.sqrt_alphas_cumprod.detach().float().cpu()[src].contiguous().to(dev),
                 inv_sqrt_1ma_src=m.sqrt_one_minus_alphas_cumprod.detach().float().cpu()[src].contiguous().to(dev),
                 inv_sqrt_a_dst=up(np.sqrt(a64)), inv_sqrt_1ma_dst=up(np.sqrt(1.0 - a64)))
        if getattr(m, "use_dynamic_rescale", False):
            t["inv_scale_ratio"] = up((self.ddim_scale_arr_prev.double() / self.ddim_scale_arr.double()).numpy())
        self._tables = t
        self._exec_timesteps = np.flip(self.ddim_timesteps).copy()

    # ------------------------------------------------------------------ public API
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, schedule_verbose=False, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, precision=None, fs=None,
               timestep_spacing="uniform", guidance_rescale=0.0, **kwargs):
        if conditioning is not None and isinstance(conditioning, dict):
            first = conditioning[list(conditioning.keys())[0]]
            cbs = (first[0] if isinstance(first, (list, tuple)) else first).shape[0]
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")
        self.make_schedule(ddim_num_steps=S, ddim_discretize=timestep_spacing, ddim_eta=eta, verbose=schedule_verbose)
        size = (batch_size,) + tuple(shape)
        return self.ddim_sampling(conditioning, size, callback=callback, img_callback=img_callback, mask=mask, x0=x0,
                                  noise_dropout=noise_dropout, temperature=temperature,
                                  score_corrector=score_corrector, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, verbose=verbose,
                                  precision=precision, fs=fs, guidance_rescale=guidance_rescale,
                                  quantize_denoised=quantize_x0, **kwargs)

    def _branches(self, cond, uc, scale, kwargs):
        br = [cond]
        if uc is not None and scale != 1.:
            br.append(uc)
            uc2 = kwargs.get("unconditional_conditioning_img_nonetext")
            if uc2 is not None:
                br.append(uc2)
        return br

    def _fused(self, branches):
        """Fused path (a StepRun on the model's batched entry) or generic path (separate apply_model calls)?"""
        return hasattr(self.model, "apply_model_rows") and all(isinstance(c, dict) for c in branches)

    # ------------------------------------------------------------------ what a subclass's update changes (dpm_solver.py)
    _run_class = FusedRun

    def _step_noise_plan(self, noises):
        """(the injected step noises to use, draw one per step?, keep the draws?). The reference calls noise_like on EVERY
        step, also when sigma_t = 0 (eta = 0): the draw is then made and discarded here too, so the generator - and with
        a mask the q_sample noises of the later steps - stays in step with the reference for the same seed."""
        return noises, noises is None, bool((self._tables["sigma_t"] != 0).any().item())

    def _generic_update(self, img, branches, g, kwargs, model=None):
        """The generic path's update, (img, i, noise) -> (x_prev, pred_x0), for any model exposing
        apply_model(x, t, c, **kw) -> [B, C, ...]: p_sample_ddim on separate apply_model calls. `model`: what to
        evaluate instead of self.model (the windowed stand-in)."""
        S = self._exec_timesteps.shape[0]

        def update(img, i, noise):
            ts = torch.full((img.shape[0],), int(self._exec_timesteps[i]), device=img.device, dtype=torch.long)
            return self.p_sample_ddim(img, branches[0], ts, index=S - i - 1, noise=noise, model=model, **g, **kwargs)
        return update

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.,
                      noise_dropout=0., score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, verbose=True, precision=None, fs=None, guidance_rescale=0.0,
                      noises=None, use_graph=False, window_stride=None, window_weights="triangle", window_shift=0,
                      windows_per_call=None, apg=None, tiles=None, **kwargs):
        if ddim_use_original_steps or quantize_denoised or score_corrector is not None or noise_dropout > 0.:
            raise NotImplementedError("only the options DynamiCrafter inference uses are implemented "
                                      "(no original-steps / quantised / corrected sampling)")
        n = self._exec_timesteps.shape[0] if timesteps is None else self.subset_steps(timesteps)
        return self._denoise(n, cond, shape, x_T=x_T, callback=callback, mask=mask, x0=x0, img_callback=img_callback,
                             log_every_t=log_every_t, temperature=temperature,
                             unconditional_guidance_scale=unconditional_guidance_scale,
                             unconditional_conditioning=unconditional_conditioning, fs=fs,
                             guidance_rescale=guidance_rescale, noises=noises, use_graph=use_graph,
                             window_stride=window_stride, window_weights=window_weights, window_shift=window_shift,
                             windows_per_call=windows_per_call, apg=apg, **({} if tiles is None else {"tiles": tiles}),
                             **kwargs)

    def subset_steps(self, timesteps):
        """How many steps `ddim_sampling(timesteps=k)` runs: the DDIM indices range(S)[:subset_end], descending, with the
        reference's expression for subset_end taken literally (ddim.py:155-156) - its off-by-one, float rounding and
        Python's slicing of a negative subset_end (k = 0 selects all but the last index) included."""
        S = self.ddim_timesteps.shape[0]
        subset_end = int(min(timesteps / S, 1) * S) - 1
        return len(range(S)[:subset_end])

    @takes_model_settings
    def _denoise(self, n, cond, shape, x_T=None, callback=None, mask=None, x0=None, img_callback=None, log_every_t=100,
                 temperature=1., unconditional_guidance_scale=1., unconditional_conditioning=None, fs=None,
                 guidance_rescale=0.0, noises=None, use_graph=False, window_stride=None, window_weights="triangle",
                 window_shift=0, windows_per_call=None, apg=None, tiles=None, **kwargs):
        """The last `n` steps of the schedule from x_T (all S of them: ddim_sampling; fewer: timesteps= and decode).
        Executed step i of the n is step S - n + i of the full run and indexes `noises` / `q_noises` ([n, ...]) by i."""
        m = self.model
        dev = m.device
        if apg is not None:                              # refused combinations: before anything touches the GPU
            apg = check_apg(apg, self, len(self._branches(cond, unconditional_conditioning, unconditional_guidance_scale,
                                                          kwargs)), guidance_rescale,
                            kwargs.get("cfg_img") is not None, last=n or None)
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the HIP path only: put the model on the GPU")
        img = (torch.randn(shape, device=dev) if x_T is None else x_T.to(dev)).to(torch.float32).contiguous().clone()
        S_all = self._exec_timesteps.shape[0]
        if n == 0:                                       # an empty selection: the reference's loop body never runs
            return img, {"x_inter": [img.clone()], "pred_x0": [img.clone()]}
        if n < S_all and window_stride is not None:
            raise ValueError("window_stride cannot be combined with a partial run (timesteps= / decode)")
        if n < S_all and tiles is not None:
            raise ValueError("tiles cannot be combined with a partial run (timesteps= / decode)")
        S, off = n, S_all - n
        window = tile = None
        if tiles is not None:
            # spatial tiles; `window_stride` beside them tiles the time axis of the same product plan
            options.check_keys(options.EXTENT_OPTIONS["tiles"], tiles)
            cfg = tiles_config(tiles, options.EXTENT_OPTIONS["tiles"].keys)
            net = getattr(getattr(m, "model", None), "diffusion_model", None)
            if hasattr(net, "spatial_multiple"):
                check_box(cfg["size"], net.spatial_multiple())
            T = getattr(m, "temporal_length", None) if window_stride is not None else img.shape[2]
            if T is None:
                raise ValueError("windowed sampling needs the model's temporal_length (the frames one UNet call takes)")
            box_shape = (int(T),) + cfg["size"]
            stride = (1 if window_stride is None else window_stride,) + cfg["stride"]
            shift = (0 if window_stride is None else window_shift,) + cfg["shift"]
            weights = cfg["weights"]                    # one name for every axis
            plan_host = tile_plan(tuple(img.shape[2:]), box_shape, stride, weights, shift, S)
            per_call = cfg["per_call"] if cfg["per_call"] is not None else windows_per_call
            tile = dict(T=box_shape[0], h=box_shape[1], w=box_shape[2], stride=stride, weights=weights, shift=shift,
                        per_call=per_call, plan=plan_host)
        elif window_stride is not None:
            T = getattr(m, "temporal_length", None)
            if T is None:
                raise ValueError("windowed sampling needs the model's temporal_length (the frames one UNet call takes)")
            # the one host plan of the call: refuses bad values here, then serves the fused run or the generic stand-in
            plan_host = window_plan(img.shape[2], T, window_stride, window_weights, window_shift, S)
            window = dict(T=int(T), stride=window_stride, weights=window_weights, shift=window_shift,
                          per_call=windows_per_call, plan=plan_host)
        clean_cond = kwargs.pop("clean_cond", False)
        branches = self._branches(cond, unconditional_conditioning, unconditional_guidance_scale, kwargs)
        q_noises = kwargs.pop("q_noises", None)
        draw_q = mask is not None and not clean_cond and q_noises is None
        noises, draw_n, keep_n = self._step_noise_plan(noises)
        if draw_n or draw_q:
            # drawn up front so a captured graph can index them by the device step counter - in the order of the reference's
            # per-step draws: with a mask, q_sample's randn_like of step i comes before that step's noise_like
            # (ddim.py:174-180, then p_sample_ddim :270)
            qs, ns = [], []
            for _ in range(S):
                if draw_q:
                    qs.append(torch.randn(shape, device=dev))
                if draw_n:
                    n_i = torch.randn(shape, device=dev)
                    if keep_n:
                        ns.append(n_i)
            if qs:
                q_noises = torch.stack(qs)
            if ns:
                noises = torch.stack(ns)
        g = dict(temperature=temperature, unconditional_guidance_scale=unconditional_guidance_scale, fs=fs,
                 guidance_rescale=guidance_rescale)
        if apg is not None:                              # the generic path's running update lives as long as this call
            g.update(apg=apg, apg_state={})
        intermediates = {"x_inter": [img.clone()], "pred_x0": [img.clone()]}
        run = None
        if self._fused(branches):
            cls, wkw = (self._run_class, {}) if window is None else (windowed(self._run_class), dict(window=window))
            if tile is not None:
                cls, wkw = tiled(self._run_class), dict(tile=tile)
            run = cls(self, img, branches, fs=fs, noises=noises, cfg_scale=unconditional_guidance_scale,
                      cfg_img=kwargs.get("cfg_img"), guidance_rescale=guidance_rescale, temperature=temperature,
                      mask=mask, x0=x0, q_noises=q_noises, clean_cond=clean_cond, **wkw,
                      **({} if off == 0 else {"last": n}), **({} if apg is None else {"apg": apg}))
            if use_graph:
                run.capture()
        else:
            noises, blend = _step_inputs(img, S, noises, mask, x0, q_noises, clean_cond,
                                         long_branches=None if window is None and tile is None else branches,
                                         long_space=tile is not None)
        proxy = None
        if run is None:
            if window is not None:
                # the update's apply_model calls go to a stand-in that evaluates the model per window and blends
                proxy = _WindowedModel(m, *plan_host, window["T"], dev)
            if tile is not None:
                proxy = _TiledModel(m, *plan_host, (tile["T"], tile["h"], tile["w"]), dev)
            update = self._generic_update(img, branches, dict(g, unconditional_conditioning=unconditional_conditioning),
                                          kwargs, **({} if proxy is None else {"model": proxy}))
        for i in range(S):
            if run is not None:
                run.step()
                pred_x0 = run.pred_x0
            else:
                if blend is not None:
                    img = ops.mask_blend(img.contiguous().clone(), blend["x0"], blend["mask"],
                                         None if blend["clean"] else blend["q"][i], self._tables, index=off + i,
                                         clean=blend["clean"])
                if proxy is not None:
                    proxy.step = i
                img, pred_x0 = update(img, off + i, None if noises is None else noises[i])
            index = S - i - 1                  # total_steps - i - 1 with the reference's total_steps = n (ddim.py:160-170)
            log_now = index % log_every_t == 0 or index == S - 1
            if run is not None and use_graph and (callback or img_callback or log_now):
                run.sync()                     # the graph runs on its own stream: the step must have finished before the
            if callback: callback(i)           # callbacks / snapshots read its results (ddim.py:196-201)
            if img_callback: img_callback(pred_x0, i)
            if log_now:
                intermediates["x_inter"].append(img.clone())
                intermediates["pred_x0"].append(pred_x0.clone())
        if run is not None:
            run.sync()
            self._last_run = run
        return img, intermediates

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, uc_type=None,
                      conditional_guidance_scale_temporal=None, mask=None, x0=None, guidance_rescale=0.0, noise=None,
                      cfg_img=None, model=None, apg=None, apg_state=None, **kwargs):
        """One DDIM update from separate apply_model calls (reference :205-279 / multiplecond :211-285). `apg`: adaptive
        projected guidance (apg_generic) ahead of the same kernel; `apg_state`: a dict that carries the running update from
        call to call (None: this call is a first step)."""
        if use_original_steps or quantize_denoised or score_corrector is not None or noise_dropout > 0.:
            raise NotImplementedError
        m = self.model if model is None else model
        dev = x.device
        x = x.to(torch.float32).contiguous()
        uc2 = kwargs.pop("unconditional_conditioning_img_nonetext", None)
        kwargs.pop("clean_cond", None)
        mk = {k: v for k, v in kwargs.items() if k == "fs"}
        e_c = m.apply_model(x, t, c, **mk).to(torch.float32).contiguous()
        e_u = e_i = None
        if unconditional_conditioning is not None and unconditional_guidance_scale != 1.:
            e_u = m.apply_model(x, t, unconditional_conditioning, **mk).to(torch.float32).contiguous()
            if uc2 is not None:
                e_i = m.apply_model(x, t, uc2, **mk).to(torch.float32).contiguous()
        S = self._exec_timesteps.shape[0]
        if noise is None:
            noise = torch.randn(x.shape, device=dev)        # drawn even when sigma == 0, as the reference does
            if repeat_noise:
                noise = noise[:1].expand_as(x)
        noise = noise.to(torch.float32).contiguous()
        x_prev, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        if apg is not None:
            apg = check_apg(apg, self, 1 + (e_u is not None) + (e_i is not None), guidance_rescale,
                            cfg_img is not None or uc2 is not None)
            e_c = apg_generic(self._tables, apg, apg_state, e_c, e_u, x, unconditional_guidance_scale,
                              v_param=m.parameterization == "v", index=S - 1 - index)
            e_u, unconditional_guidance_scale = None, 1.0
        return ops.ddim_step(self._tables, e_c, e_u, e_i, x, noise, x_prev, pred_x0, ops.step_workspace(x.shape[0], dev),
                             index=S - 1 - index, e_nchw=True,
                             **_update_kw(m, x, unconditional_guidance_scale, cfg_img, guidance_rescale, temperature))

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """ddim.py:303-317 (tiny elementwise helper, torch)."""
        if use_original_steps:
            sa, s1 = self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod
        else:
            sa = torch.sqrt(self.ddim_alphas).to(x0.device)
            s1 = torch.as_tensor(self.ddim_sqrt_one_minus_alphas).to(x0.device)
        noise = torch.randn_like(x0) if noise is None else noise
        shp = (t.shape[0],) + (1,) * (x0.dim() - 1)
        return sa.to(x0.device)[t].reshape(shp) * x0 + s1[t].reshape(shp) * noise

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, callback=None, *, fs=None, guidance_rescale=0.0, cfg_img=None,
               unconditional_conditioning_img_nonetext=None, noises=None, temperature=1., mask=None, x0=None,
               q_noises=None, use_graph=False, img_callback=None, log_every_t=100, **sampling_options):
        """ddim.py:281-301: run the last t_start DDIM steps from x_latent (at level ddim_alphas[t_start - 1]) and return
        the result. The steps are those of `sample`, on the same path (a partial FusedRun when the model has the batched
        entry), so the keyword-only options mean what they mean there; `noises` / `q_noises` are [t_start, ...], indexed
        by the executed step. Without `fs` none is passed to the model, as in the reference. `sampling_options`: the
        keywords of samplers/options.py (`freeu=`, `apg=`, `token_downsampling=`) and no other."""
        if use_original_steps:
            raise NotImplementedError
        unexpected = sorted(set(sampling_options) - set(OPTIONS) - set(options.EXTENT_OPTIONS))
        if unexpected:
            raise TypeError(f"decode() got an unexpected keyword argument {unexpected[0]!r}")
        n = len(self.ddim_timesteps[:t_start])
        kw = sampling_options
        if cfg_img is not None:
            kw["cfg_img"] = cfg_img
        if unconditional_conditioning_img_nonetext is not None:
            kw["unconditional_conditioning_img_nonetext"] = unconditional_conditioning_img_nonetext
        if q_noises is not None:
            kw["q_noises"] = q_noises
        x_dec, _ = self._denoise(n, cond, tuple(x_latent.shape), x_T=x_latent, callback=callback, mask=mask, x0=x0,
                                 img_callback=img_callback, log_every_t=log_every_t, temperature=temperature,
                                 unconditional_guidance_scale=unconditional_guidance_scale,
                                 unconditional_conditioning=unconditional_conditioning, fs=fs,
                                 guidance_rescale=guidance_rescale, noises=noises, use_graph=use_graph, **kw)
        return x_dec

    @torch.no_grad()
    @takes_model_settings
    def encode(self, x0, c, t_enc, use_original_steps=False, return_intermediates=None,
               unconditional_guidance_scale=1.0, unconditional_conditioning=None, callback=None, *, fs=None,
               guidance_rescale=0.0, use_graph=False, **kwargs):
        """DDIM inversion: the deterministic pass from the clean latent x0 up to level ddim_alphas[t_enc - 1], where
        `decode(x, c, t_enc)` starts - the reference's TODO at ddim.py:179, with the signature of the latent-diffusion
        sampler's `encode`. Runs the inverse steps k = 0 .. t_enc - 1 (include/dcrafter_hip.h: dc_ddim_invert_step; the
        UNet sees the latent at the source level's timestep): InvertRun when the model has the batched entry and the
        conditionings are dicts, else separate apply_model calls and the same kernel. Three-branch guidance through
        `cfg_img` / `unconditional_conditioning_img_nonetext`. Returns (x_encoded, {"x_inter": [...], "pred_x0": [...]}):
        with return_intermediates = r the latent and pred_x0 after every max(t_enc // r, 1)-th step and after the last."""
        if use_original_steps:
            raise NotImplementedError("encode runs on the DDIM timesteps only")
        for opt in options.of_kind(options.RUN_SETTING):    # a run setting with a running state has no inversion
            if opt.name in kwargs:
                raise ValueError(f"encode: {opt.name}= is a sampling-time guidance with a running state; an inversion under it "
                                 f"is not defined")
        if kwargs.get("window_stride") is not None:
            raise ValueError("encode: windowed (long-clip) inversion is not defined")
        if kwargs.get("tiles") is not None:
            raise ValueError("encode: tiled (large-frame) inversion is not defined")
        S = self.ddim_timesteps.shape[0]
        if not isinstance(t_enc, (int, np.integer)) or not 1 <= t_enc <= S:
            raise ValueError(f"encode: t_enc must be an integer in 1 .. {S}, got {t_enc!r}")
        n = int(t_enc)
        m = self.model
        dev = m.device
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the HIP path only: put the model on the GPU")
        img = x0.to(dev).to(torch.float32).contiguous().clone()
        branches = self._branches(c, unconditional_conditioning, unconditional_guidance_scale, kwargs)
        cfg_img = kwargs.get("cfg_img")
        inter = {"x_inter": [], "pred_x0": []}
        every = max(n // int(return_intermediates), 1) if return_intermediates else 0
        run = None
        if self._fused(branches):
            run = InvertRun(self, img, branches, n, fs=fs, cfg_scale=unconditional_guidance_scale, cfg_img=cfg_img,
                            guidance_rescale=guidance_rescale)
            if use_graph:
                run.capture()
        else:
            ws = ops.step_workspace(img.shape[0], dev)
            kw = _invert_kw(m, img, unconditional_guidance_scale, cfg_img, guidance_rescale, e_nchw=True)
            mk = {} if fs is None else {"fs": fs}
        for k in range(n):
            if run is not None:
                run.step()
                pred_x0 = run.pred_x0
            else:
                ts = torch.full((img.shape[0],), int(self._inv_timesteps[k]), device=dev, dtype=torch.long)
                e = [m.apply_model(img, ts, b, **mk).to(torch.float32).contiguous() for b in branches]
                e += [None] * (3 - len(e))
                img, pred_x0 = ops.ddim_invert_step(self._tables, e[0], e[1], e[2], img, torch.empty_like(img),
                                                    torch.empty_like(img), ws, index=k, **kw)
            log_now = every and (k % every == 0 or k == n - 1)
            if run is not None and use_graph and (callback or log_now):
                run.sync()
            if callback: callback(k)
            if log_now:
                inter["x_inter"].append(img.clone())
                inter["pred_x0"].append(pred_x0.clone())
        if run is not None:
            run.sync()
            self._last_run = run
        return img, inter
