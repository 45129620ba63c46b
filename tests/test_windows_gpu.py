"""Windowed sampling (clips longer than the UNet's temporal_length) on the GPU: the two kernels against dc_pack_latent /
a float64 restatement, the one-window identity, a tiny-UNet trajectory against the CPU oracle driven per window, fused
against generic, graph == eager with rewind, the analytic pointwise-denoiser check, the harness's num_frames, and one
step at real width under arena guards.

Stated tolerances (every test prints what it measures):
  dc_pack_latent_windows        torch.equal with dc_pack_latent on the gathered frames
  dc_window_merge (fp32)        per element |err| <= (n + 1) 2^-24 sum_w |wn e|, n = windows containing the frame
                                (one rounding per product, one per sum); chunked == unchunked and a single window of
                                weight 1 == its input, torch.equal
  one-window run                torch.equal with the plain run (final sample and every intermediate)
  8-step windowed trajectory    rel-L2 <= 8.5e-2, the project's multi-step bound for this tiny model
                                (tests/test_dpm_solver_gpu.py); measured values in the test's docstring
  fused vs generic, windowed    <= 2x the rel-L2 of the unwindowed fused / generic pair on a T = 4 slice
  pointwise denoiser            windowed vs plain rel-L2 <= 10x what the float64 restatement shows for fp32-rounded weights
  real width, one step          rel-L2 <= 3e-2 and cosine >= 0.9997 per branch: tests/test_fullsize_gpu.py's UNet bound
"""
import gc
import os

import numpy as np
import pytest
import torch
import yaml

from tests import windows_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAJ_TOL = 8.5e-2
UNET_TOL, UNET_COS = 3e-2, 0.9997


def _plan(T_long, T, stride, weights="triangle", shift=0, S=1, multiple_of=1):
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers.windows import window_plan
    starts, wn = window_plan(T_long, T, stride, weights, shift, S, multiple_of)
    return ops.window_tables(starts, wn, T_long=T_long, T=T, device=DEV)


# ------------------------------------------------------------------ 5. dc_pack_latent_windows
@pytest.mark.parametrize("Cx,Cc,c_pad", [(4, 4, 64), (4, 5, 16), (4, 4, 8), (4, 0, 8)])
def test_pack_latent_windows_equals_pack_latent_on_gathered_frames(Cx, Cc, c_pad):
    from dynamicrafter_amd import ops
    B, T_long, T, HW, S = 2, 9, 4, 24, 5
    plan = _plan(T_long, T, 2, shift=1, S=S)                     # a shifting plan: odd steps start at 0, 1, 3, 5
    W = plan["W"]
    assert (plan["host_starts"][0] != plan["host_starts"][1]).any()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, Cx, T_long, HW, generator=g).to(DEV)
    cc = torch.randn(B, Cc, T_long, HW, generator=g).to(DEV) if Cc else None
    counter = torch.tensor([3], dtype=torch.int32, device=DEV)
    for step, sel in ((3, dict(step_index=counter, index=1)), (2, dict(index=2)), (0, dict(index=0))):
        for w0, n_w, nrep in ((0, W, 1), (1, W - 1, 1), (2, 1, 2), (0, 2, 1)):
            st = plan["host_starts"][step, w0:w0 + n_w]
            gather = lambda t: torch.stack([t[b, :, s:s + T] for b in range(B) for s in st]).contiguous()
            M = B * n_w * T * HW
            ref = torch.full((nrep * M, c_pad), 7.0, dtype=torch.bfloat16, device=DEV)
            ops.pack_latent(gather(x), None if cc is None else gather(cc), ref, B=B * n_w, Cx=Cx, Cc=Cc, T=T, HW=HW, nrep=nrep)
            out = torch.full((nrep * M + 3, c_pad), 7.0, dtype=torch.bfloat16, device=DEV)
            ops.pack_latent_windows(x, cc, out, plan, B=B, Cx=Cx, Cc=Cc, HW=HW, w0=w0, n_w=n_w, nrep=nrep, **sel)
            torch.cuda.synchronize()
            assert torch.equal(out[:nrep * M], ref), (step, w0, n_w)
            assert bool((out[nrep * M:] == 7.0).all())            # nothing past the last row
            if Cx + Cc < c_pad:
                assert not out[:nrep * M, Cx + Cc:].any()         # pad channels are zero
    with pytest.raises(ValueError):
        ops.pack_latent_windows(x, cc, out, plan, B=B, Cx=Cx, Cc=Cc, HW=HW, w0=W - 1, n_w=2)
    with pytest.raises(ValueError):
        ops.pack_latent_windows(x, cc, out[:5], plan, B=B, Cx=Cx, Cc=Cc, HW=HW)
    with pytest.raises(ValueError):
        ops.pack_latent_windows(x, cc, out, plan, B=B, Cx=Cx, Cc=Cc, HW=HW, index=S)


# ------------------------------------------------------------------ 6. dc_window_merge
@pytest.mark.parametrize("weights", ["uniform", "triangle"])
@pytest.mark.parametrize("C,ld_e,ld_out", [(4, 4, 4), (4, 8, 4), (4, 8, 8), (3, 5, 3)])
@pytest.mark.parametrize("nb", [1, 2, 3])
def test_window_merge_vs_restatement(nb, C, ld_e, ld_out, weights):
    from dynamicrafter_amd import ops
    B, T_long, T, HW, S = 2, 8, 4, 20, 3
    plan = _plan(T_long, T, 2, weights, shift=1, S=S)             # W = 4: all four carry weight at step 1, three at step 0
    W = plan["W"]
    assert W == 4
    g = torch.Generator().manual_seed(5 + nb)
    e = torch.randn(nb * B * W * T * HW, ld_e, generator=g).to(DEV)
    e[:, C:] = float("nan")                                       # columns past C are not the kernel's to read
    counter = torch.tensor([1], dtype=torch.int32, device=DEV)
    worst = 0.0
    for step, sel in ((1, dict(step_index=counter)), (0, dict(index=0)), (2, dict(index=2))):
        out = torch.full((nb * B * T_long * HW + 2, ld_out), 7.0, device=DEV)
        ops.window_merge(e, out, plan, nb=nb, B=B, C=C, HW=HW, **sel)
        # chunked: two calls of two windows; e rows of a chunk are [(k, b, w in chunk, f, p)]
        e6 = e.reshape(nb, B, W, T * HW, ld_e)
        chunked = torch.full_like(out, 7.0)
        for w0 in (0, 2):
            ops.window_merge(e6[:, :, w0:w0 + 2].reshape(-1, ld_e).contiguous(), chunked, plan, nb=nb, B=B, C=C, HW=HW,
                             w0=w0, n_w=2, accumulate=w0 > 0, **sel)
        torch.cuda.synchronize()
        n_rows = nb * B * T_long * HW
        assert bool((out[n_rows:] == 7.0).all()) and bool((out[:n_rows, C:] == 7.0).all())
        assert torch.equal(out, chunked), step                    # ascending windows either way: the same roundings
        ref, mag, n = R.merge_rows(e, plan["host_starts"][step], plan["host_wn"][step], nb=nb, B=B, T_long=T_long, HW=HW,
                                   C=C)
        got = out[:n_rows, :C].double().cpu().numpy().reshape(ref.shape)
        bound = (n[None, None, :, None, None] + 1) * 2.0 ** -24 * mag
        err = np.abs(got - ref)
        assert np.isfinite(got).all()
        assert (err <= bound).all(), (step, float((err - bound).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"\n[window merge nb={nb} C={C} ld_e={ld_e} {weights}] worst |err| / bound {worst:.3f}")


def test_window_merge_never_reads_a_padding_window():
    """A window of weight 0 (padding, or a duplicate) is skipped: whatever the UNet wrote for it, infinities and NaN
    included, does not reach the blend, chunked or not."""
    from dynamicrafter_amd import ops
    nb, B, T_long, T, HW = 2, 1, 8, 4, 12
    plan = _plan(T_long, T, 2, "triangle", shift=1, S=2)
    assert plan["W"] == 4 and not plan["host_wn"][0, 3].any()     # step 0: window 3 is padding
    e = torch.randn(nb, B, 4, T * HW, 4, generator=torch.Generator().manual_seed(9)).to(DEV)
    clean = e.clone()
    e[:, :, 3] = float("nan")
    e[0, 0, 3, 0, 0] = float("inf")
    outs = []
    for src in (e, clean):
        out = torch.empty(nb * B * T_long * HW, 4, device=DEV)
        ops.window_merge(src.reshape(-1, 4), out, plan, nb=nb, B=B, C=4, HW=HW, index=0)
        outs.append(out)
    chunked = torch.empty_like(outs[0])
    for w0 in (0, 2):
        ops.window_merge(e[:, :, w0:w0 + 2].reshape(-1, 4).contiguous(), chunked, plan, nb=nb, B=B, C=4, HW=HW, w0=w0, n_w=2,
                         accumulate=w0 > 0, index=0)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(chunked, outs[0])


def test_window_merge_single_window_of_weight_one_is_the_identity():
    from dynamicrafter_amd import ops
    nb, B, T, HW = 2, 2, 4, 20
    plan = _plan(T, T, 2, "triangle", shift=1, S=2)
    assert plan["W"] == 1 and bool((plan["wn"] == 1.0).all())
    e = torch.randn(nb * B * T * HW, 4, generator=torch.Generator().manual_seed(8)).to(DEV)
    e[3, 1] = -0.0
    out = torch.empty_like(e)
    ops.window_merge(e, out, plan, nb=nb, B=B, C=4, HW=HW, index=1)
    torch.cuda.synchronize()
    assert torch.equal(out, e)
    assert torch.equal(out.view(torch.int32), e.view(torch.int32))          # the sign of zero too


# ------------------------------------------------------------------ the tiny model of the existing GPU tests
def _tiny_model(toy_conditioners=False):
    from dynamicrafter_amd.utils.utils import instantiate_from_config
    from oracle import unet as ounet
    from oracle.weights import fill_state_dict
    from tests.golden_cfg import TINY_AE, TINY_RESAMPLER, TINY_UNET
    root = os.path.join(os.path.dirname(__file__), "..", "dynamicrafter_amd", "configs")
    cfg = yaml.safe_load(open(os.path.join(root, "inference_512_v1.0.yaml")))
    p = cfg["model"]["params"]
    params = dict(TINY_UNET, default_fs=24)
    p["unet_config"]["params"] = params
    p["first_stage_config"]["params"]["ddconfig"] = dict(TINY_AE)
    if toy_conditioners:
        p["cond_stage_config"] = {"target": "tests.golden_cfg.ToyTextEmbedder"}
        p["img_cond_stage_config"] = {"target": "tests.golden_cfg.ToyImageEmbedder"}
        p["image_proj_stage_config"] = {"target": "lvdm.modules.encoders.resampler.Resampler",
                                        "params": dict(TINY_RESAMPLER)}
    else:
        for k in ("cond_stage_config", "img_cond_stage_config", "image_proj_stage_config"):
            p[k] = {"target": "torch.nn.Identity"}
    model = instantiate_from_config(cfg["model"])
    ocfg = ounet.UNetCfg.from_params(params)
    sd = fill_state_dict(ounet.unet_param_shapes(ocfg), seed=11)
    model.model.diffusion_model.load_state_dict(sd, strict=True)
    if toy_conditioners:
        for mod, seed in ((model.first_stage_model, 13), (model.image_proj_model, 14)):
            sdict = mod.state_dict()
            mod.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in sdict.items()}, seed), strict=True)
    return model.to(DEV).eval(), sd, ocfg


@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


def _inputs(S, seed=9, b=1, t=8, h=16, w=16, T=4):
    g = torch.Generator().manual_seed(seed)
    return dict(x_T=torch.randn(b, 4, t, h, w, generator=g),
                ctx=[torch.randn(b, 77 + 16 * T, 128, generator=g) for _ in range(3)],
                cc=torch.randn(b, 4, t, h, w, generator=g) * 0.2,
                noises=torch.randn(S, b, 4, t, h, w, generator=g),
                q_noises=torch.randn(S, b, 4, t, h, w, generator=g),
                x0=torch.randn(b, 4, t, h, w, generator=g),
                fs=torch.tensor([24] * b))


def _frames(inp, lo, hi):
    """The same inputs restricted to frames lo .. hi - 1."""
    out = dict(inp)
    for k in ("x_T", "cc", "x0"):
        out[k] = inp[k][:, :, lo:hi].contiguous()
    for k in ("noises", "q_noises"):
        out[k] = inp[k][:, :, :, lo:hi].contiguous()
    return out


class _Generic:
    """The model without its fused entry: the sampler takes the generic path (separate apply_model calls)."""

    def __init__(self, model):
        self._m = model

    def __getattr__(self, name):
        if name in ("apply_model_rows", "_m"):
            raise AttributeError(name)
        return getattr(self._m, name)


def _sample(model, inp, S, solver="ddim", nb=2, use_graph=False, mask=None, log_every_t=100, **win):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    mk = lambda c: {"c_crossattn": [c.to(DEV)], "c_concat": [inp["cc"].to(DEV)]}
    kw = dict(win)
    if nb == 3:
        kw.update(cfg_img=2.0, unconditional_conditioning_img_nonetext=mk(inp["ctx"][2]))
    if mask is not None:
        kw.update(mask=mask.to(DEV), x0=inp["x0"].to(DEV), q_noises=inp["q_noises"].to(DEV))
    s = DDIMSampler(model) if solver == "ddim" else DPMSolverSampler(model, solver=solver)
    x_T = inp["x_T"]
    out, inter = s.sample(S, x_T.shape[0], tuple(x_T.shape[1:]), conditioning=mk(inp["ctx"][0]), verbose=False,
                          unconditional_guidance_scale=7.5, unconditional_conditioning=mk(inp["ctx"][1]), eta=1.0,
                          x_T=x_T.to(DEV), fs=inp["fs"].to(DEV), timestep_spacing="uniform_trailing",
                          guidance_rescale=0.7, noises=inp["noises"].to(DEV), use_graph=use_graph,
                          log_every_t=log_every_t, **kw)
    return out, inter, s


# ------------------------------------------------------------------ 7. one window == the plain call
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nb", [2, 3])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m", "dpmpp_2m_sde"])
def test_one_window_equals_the_plain_call(tiny, solver, nb, masked, use_graph):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import WindowedRun
    model = tiny[0]
    S = 4
    inp = _inputs(S, seed=17, t=4)
    mask = None
    if masked:
        mask = torch.zeros(1, 1, 4, 16, 16)
        mask[:, :, 0] = 1.0
    plain, pi, sp = _sample(model, inp, S, solver, nb, use_graph, mask, log_every_t=1)
    win, wi, sw = _sample(model, inp, S, solver, nb, use_graph, mask, log_every_t=1, window_stride=2, window_shift=1)
    assert isinstance(sw._last_run, WindowedRun) and not isinstance(sp._last_run, WindowedRun)
    assert sw._last_run.plan["W"] == 1 and (sw._last_run.graph is not None) == use_graph
    assert torch.isfinite(plain).all()
    assert torch.equal(win, plain)
    for k in ("x_inter", "pred_x0"):
        assert len(wi[k]) == len(pi[k]) == S + 1
        for a, b in zip(wi[k], pi[k]):
            assert torch.equal(a, b), k


# ------------------------------------------------------------------ 8. trajectory against the oracle
def test_windowed_trajectory_vs_oracle(tiny):
    """8 DDIM eta = 1 steps of an 8-frame latent through 4-frame windows (stride 2, triangle weights, shift 1; v-param,
    ZTSNR, dynamic rescale, CFG 7.5, guidance rescale 0.7, injected noises): the fused path against the restatement
    driving oracle.unet.unet_forward per window on the CPU and blending in float64.
    Measured on MI355X: rel-L2 3.57e-2 (1.5x = 5.4e-2; eager and graph agree bitwise); bound 8.5e-2."""
    from oracle import ddim as oddim
    from oracle import unet as ounet
    from dynamicrafter_amd.lvdm.models.samplers.windows import window_plan
    model, sd, ocfg = tiny
    S, T = 8, 4
    inp = _inputs(S)
    win = dict(window_stride=2, window_weights="triangle", window_shift=1)
    out, _, s = _sample(model, inp, S, **win)
    graph, _, _ = _sample(model, inp, S, use_graph=True, **win)
    assert s._last_run.plan["W"] == 4 and s._last_run.prep["win"]["n_w"] == 4
    starts, wn = window_plan(8, T, 2, "triangle", 1, S)
    state = {"i": 0}

    def apply_model(x, tl, c, fs=None):
        g = R.windowed_model(lambda xw, st: ounet.unet_forward(sd, ocfg, torch.cat([xw, inp["cc"][:, :, st:st + T]], 1), tl,
                                                               c, fs), starts, wn, T)
        return g(x, state["i"])

    ms = oddim.ModelSchedule(rescale_betas_zero_snr=True, parameterization="v", use_dynamic_rescale=True, base_scale=0.7)
    sc = oddim.DDIMSchedule(ms, S, "uniform_trailing", 1.0)
    ref = oddim.ddim_sample(apply_model, sc, inp["x_T"].double(), inp["ctx"][0], inp["ctx"][1], cfg_scale=7.5,
                            guidance_rescale=0.7, noises=list(inp["noises"].double()), fs=inp["fs"],
                            trace=lambda i, x, p: state.update(i=i + 1))
    r = R.rel_l2(out, ref)
    print(f"\n[windowed trajectory] 8 DDIM steps, T_long 8 / T 4 / stride 2 / shift 1, vs oracle rel-L2 {r:.3e} "
          f"(1.5x = {1.5 * r:.3e}, bound {TRAJ_TOL})")
    assert torch.isfinite(out).all()
    assert torch.equal(out, graph)
    assert r < TRAJ_TOL


# ------------------------------------------------------------------ 9. fused against generic
@pytest.mark.parametrize("nb", [2, 3])
def test_windowed_fused_vs_generic(tiny, nb):
    """The windowed fused path (batched windows, dc_window_merge) against the windowed generic path (one apply_model per
    window and branch, torch blend) on the inputs of the trajectory test. The tolerance is twice what the parent
    commit's own fused / generic pair differs by, without windows, on the first four frames of the same inputs.
    With three branches the UNet batch is 3 x 4 = 12 clips: the embedding MLPs (dc_gemv_small, at most 8 rows a launch)
    run in two launches.
    Measured on MI355X with the kernel as it is here (weight-0 terms skipped), for 2 and for 3 branches alike:
    unwindowed 0 (bitwise equal at this size), windowed 0: the generic blend follows dc_window_merge's order and
    roundings (an earlier generic blend, a plain fp32 multiply-then-add, differed from the fused path by 5.6e-8). The generic blend reproduces a fused multiply-add through float64, which is exact except for rare double
    roundings, so the equality of the windowed pair holds for these inputs and is not guaranteed for all."""
    model = tiny[0]
    S = 8
    inp = _inputs(S)
    win = dict(window_stride=2, window_weights="triangle", window_shift=1)
    short = _frames(inp, 0, 4)
    base = R.rel_l2(_sample(model, short, S, nb=nb)[0], _sample(_Generic(model), short, S, nb=nb)[0])
    fused, _, sf = _sample(model, inp, S, nb=nb, **win)
    generic, _, sg = _sample(_Generic(model), inp, S, nb=nb, **win)
    assert hasattr(sf, "_last_run") and not hasattr(sg, "_last_run")
    assert sf._last_run.t_table.shape[1] == nb * 4         # clips in the one UNet call of a step
    r = R.rel_l2(fused, generic)
    print(f"\n[windowed fused vs generic, {nb} branches] unwindowed pair rel-L2 {base:.3e}, windowed pair {r:.3e} (allowed {2 * base:.3e})")
    assert torch.isfinite(fused).all() and torch.isfinite(generic).all()
    assert r <= 2 * base


# ------------------------------------------------------------------ 10. graph == eager, chunked, with rewind
def test_graph_equals_eager_and_rewind_with_chunks_and_mask(tiny):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler, FusedRun, windowed
    model = tiny[0]
    S = 5
    a, b = _inputs(S, seed=41), _inputs(S, seed=42)
    mask = torch.zeros(1, 1, 8, 16, 16)
    mask[:, :, 0] = 1.0
    window = dict(T=4, stride=2, weights="triangle", shift=1, per_call=2)
    s = DDIMSampler(model)
    s.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    mk = lambda c: {"c_crossattn": [c.to(DEV)], "c_concat": [a["cc"].to(DEV)]}
    br = [mk(a["ctx"][0]), mk(a["ctx"][1])]

    def fresh(x_T, graph):
        run = windowed(FusedRun)(s, x_T.to(DEV).clone(), br, window=window, fs=a["fs"].to(DEV), noises=a["noises"].to(DEV),
                                 cfg_scale=7.5, guidance_rescale=0.7, mask=mask.to(DEV), x0=a["x0"].to(DEV),
                                 q_noises=a["q_noises"].to(DEV))
        if graph:
            run.capture()
        for _ in range(S):
            run.step()
        run.sync()
        return run, run.img.clone()

    run, first = fresh(a["x_T"], True)
    assert run.plan["W"] == 4 and run.prep["win"]["n_w"] == 2 and run.graph is not None
    run.rewind(b["x_T"].to(DEV))
    for _ in range(S):
        run.step()
    run.sync()
    second = run.img.clone()
    with pytest.raises(RuntimeError, match="rewind"):
        run.step()
    _, eager_a = fresh(a["x_T"], False)
    _, eager_b = fresh(b["x_T"], False)
    _, graph_b = fresh(b["x_T"], True)
    assert torch.isfinite(first).all() and not torch.equal(first, second)
    assert torch.equal(first, eager_a)
    assert torch.equal(second, eager_b) and torch.equal(second, graph_b)


def test_scratch_bound_covers_the_arena_after_a_windowed_run(tiny):
    """max_row_width / max_context_row_width (what the default windows_per_call is computed from) against the buffers
    the arena really holds after windowed runs of the tiny model: none is larger than the bound says."""
    model = tiny[0]
    net = model.model.diffusion_model
    inp = _inputs(2)
    _sample(model, inp, 2, nb=3, window_stride=2, window_shift=1)
    clips, T, HW = 3 * 4, 4, 16 * 16
    bound = max(clips * T * HW * net.max_row_width(), clips * T * 93 * net.max_context_row_width())
    sizes = {key[0]: key[1] * key[2] for key in net._arena._bufs}
    tag = max(sizes, key=sizes.get)
    print(f"\n[scratch bound] largest arena buffer {tag}: {sizes[tag]} elements, bound {bound:.0f}")
    assert sizes[tag] <= bound
    with pytest.raises(ValueError, match="windows_per_call"):
        _sample(model, inp, 2, window_stride=2, windows_per_call=0)


# ------------------------------------------------------------------ 11. analytic: a pointwise denoiser makes the blend an identity
class ScheduleModel:
    """The model's schedule buffers on the GPU (oracle.ddim.ModelSchedule); `apply_model` is the exact denoiser of data
    N(0, s^2), returned as v (restated from tests/test_dpm_solver_gpu.py). Pointwise: no frame sees another."""
    temporal_length = 4

    def __init__(self, s=6.0):
        from oracle import ddim as oddim
        ms = oddim.ModelSchedule(rescale_betas_zero_snr=True, parameterization="v", use_dynamic_rescale=False)
        self.ms = ms
        for k in ("num_timesteps", "parameterization", "use_dynamic_rescale"):
            setattr(self, k, getattr(ms, k))
        for k in ("alphas_cumprod", "betas", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
            setattr(self, k, getattr(ms, k).to(DEV))
        self.device = torch.device(DEV)
        self.s = s
        self._acp = ms.alphas_cumprod.double()

    def denoise(self, xd, t):
        a = self._acp[int(t)].item()
        al, sg = np.sqrt(a), np.sqrt(1 - a)
        x0 = al * self.s ** 2 / (a * self.s ** 2 + 1 - a) * xd
        return (al * xd - x0) / sg

    def apply_model(self, x, t, c, **kw):
        return self.denoise(x.double(), t[0]).float()


def test_pointwise_denoiser_windowed_equals_plain():
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.windows import window_plan
    from oracle import ddim as oddim
    m = ScheduleModel()
    S, T_long = 8, 8
    g = torch.Generator().manual_seed(23)
    x_T = torch.randn(1, 4, T_long, 8, 8, generator=g)
    noises = torch.randn(S, 1, 4, T_long, 8, 8, generator=g)
    kw = dict(S=S, batch_size=1, shape=(4, T_long, 8, 8), conditioning=None, verbose=False, eta=1.0, x_T=x_T.to(DEV),
              timestep_spacing="uniform_trailing", noises=noises.to(DEV))
    plain, _ = DDIMSampler(m).sample(**kw)
    win, _ = DDIMSampler(m).sample(window_stride=2, window_weights="triangle", window_shift=1, **kw)
    # what rounding the weights to fp32 does, everything else in float64
    starts, wn = window_plan(T_long, 4, 2, "triangle", 1, S)
    sums = torch.from_numpy(R.weight_sums(starts, wn, T_long))
    assert float((sums - 1).abs().max()) > 0                      # triangle weights of 1/3, 2/3: inexact in fp32
    sc = oddim.DDIMSchedule(m.ms, S, "uniform_trailing", 1.0)
    state = {"i": 0}

    def restated(scale):
        state["i"] = 0
        fn = lambda x, tl, c: m.denoise(x, tl[0]) * (sums[state["i"]].view(1, 1, -1, 1, 1) if scale else 1.0)
        return oddim.ddim_sample(fn, sc, x_T.double(), None, noises=list(noises.double()),
                                 trace=lambda i, x, p: state.update(i=i + 1))
    d64 = R.rel_l2(restated(True), restated(False))
    r = R.rel_l2(win, plain)
    print(f"\n[pointwise denoiser] windowed vs plain rel-L2 {r:.3e}; float64 restatement with fp32-rounded weights "
          f"{d64:.3e} (bound {10 * d64:.3e}); plain vs float64 {R.rel_l2(plain, restated(False)):.3e}")
    assert torch.isfinite(win).all()
    assert r <= 10 * d64


# ------------------------------------------------------------------ 12. the harness
def test_image_guided_synthesis_num_frames():
    from dynamicrafter_amd.scripts.evaluation.inference import image_guided_synthesis
    model = _tiny_model(toy_conditioners=True)[0]
    g = torch.Generator().manual_seed(5)
    b, t, H, W, S = 1, 4, 128, 128, 4
    videos = (torch.rand(b, 3, 1, H, W, generator=g) * 2 - 1).repeat(1, 1, t, 1, 1).to(DEV)
    x_T = torch.randn(b, 4, 8, H // 8, W // 8, generator=g).to(DEV)
    noises = torch.randn(S, b, 4, 8, H // 8, W // 8, generator=g).to(DEV)
    kw = dict(n_samples=1, ddim_steps=S, ddim_eta=1.0, unconditional_guidance_scale=7.5, cfg_img=None, fs=24,
              timestep_spacing="uniform_trailing", guidance_rescale=0.7)
    shape = [b, 4, t, H // 8, W // 8]
    torch.manual_seed(0)                                  # the posterior draw of the first-stage encode
    long = image_guided_synthesis(model, ["a corgi"], videos, shape, num_frames=8, x_T=x_T, noises=noises, **kw)
    assert tuple(long.shape) == (b, 1, 3, 8, H, W)
    assert torch.isfinite(long).all() and float(long.std()) > 1e-3
    short = dict(x_T=x_T[:, :, :t].contiguous(), noises=noises[:, :, :, :t].contiguous())
    torch.manual_seed(0)
    plain = image_guided_synthesis(model, ["a corgi"], videos, shape, **short, **kw)
    torch.manual_seed(0)
    one = image_guided_synthesis(model, ["a corgi"], videos, shape, num_frames=t, window_stride=2, window_shift=1, **short,
                                 **kw)
    assert tuple(plain.shape) == (b, 1, 3, t, H, W)
    assert torch.equal(one, plain)
    with pytest.raises(ValueError, match="num_frames"):
        image_guided_synthesis(model, ["a corgi"], videos, shape, num_frames=3, **short, **kw)


# ------------------------------------------------------------------ 13. real width, one step, under arena guards
def test_real_width_one_windowed_step_under_arena_guard():
    """The released 1.44 B-parameter UNet (recipe weights) at the 512 config's latent 16 x 40 x 64: a 24-frame latent,
    stride 8, two windows, cond + uncond as ONE forward of four clips, merged by dc_window_merge - against the existing
    path's apply_model_rows per window (batch 2) blended in torch float64. Batched and separate launches may choose
    different tile plans, so the bound is the UNet-forward bound of tests/test_fullsize_gpu.py at this size.
    Measured on MI355X: rel-L2 1.33e-2 / 1.31e-2, cosine 0.99991 / 0.99991 (cond / uncond), 156 guarded buffers intact."""
    from dynamicrafter_amd.utils.utils import instantiate_from_config
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers.windows import window_plan
    from oracle import unet as ounet
    from oracle.weights import fill_state_dict
    old = os.environ.get("DC_ARENA_GUARD")
    os.environ["DC_ARENA_GUARD"] = "1"
    try:
        root = os.path.join(os.path.dirname(__file__), "..", "dynamicrafter_amd", "configs")
        cfg = yaml.safe_load(open(os.path.join(root, "inference_512_v1.0.yaml")))
        p = cfg["model"]["params"]
        for k in ("cond_stage_config", "img_cond_stage_config", "image_proj_stage_config"):
            p[k] = {"target": "torch.nn.Identity"}
        model = instantiate_from_config(cfg["model"])
        ocfg = ounet.UNetCfg.from_params(p["unet_config"]["params"])
        model.model.diffusion_model.load_state_dict(fill_state_dict(ounet.unet_param_shapes(ocfg), seed=12), strict=True)
        model = model.to(DEV).eval()
        net = model.model.diffusion_model
        assert net._arena.guard
        rnd = lambda *shape, seed: torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
        B, TL, T, H, W, nb = 1, 24, 16, 40, 64, 2
        x = rnd(B, 4, TL, H, W, seed=401).to(DEV)
        cc = (rnd(B, 4, 1, H, W, seed=402) * 0.18215 * 4).repeat(1, 1, TL, 1, 1).contiguous().to(DEV)
        ctx = [rnd(B, 77 + 16 * T, 1024, seed=403 + k).to(DEV) for k in range(nb)]
        fs = torch.tensor([24], device=DEV)
        br = [{"c_crossattn": [c], "c_concat": [cc]} for c in ctx]
        starts, wn = window_plan(TL, T, 8)
        assert starts.tolist() == [[0, 8]]
        assert model.max_windows_per_call((B, 4, TL, H, W), nb, T) >= 2
        plan = ops.window_tables(starts, wn, T_long=TL, T=T, device=DEV)
        t_step = 601
        prep = model.prepare_branches((B, 4, TL, H, W), br, fs=fs, windows=dict(T=T, n_w=2))
        assert prep["share"] == 2
        t_table = torch.full((1, nb * B * 2), t_step, dtype=torch.int64, device=DEV)
        merged = torch.empty(nb * B * TL * H * W, 4, device=DEV)
        model.apply_model_windows(x, prep, t_table, plan, merged)
        torch.cuda.synchronize()
        n_guarded = net._arena.check()
        merged = merged.double().cpu().reshape(nb, B, TL, H * W, 4)
        # the existing path, one window at a time
        ref = torch.zeros_like(merged)
        for w, s in enumerate(int(v) for v in starts[0]):
            brw = [{"c_crossattn": [c], "c_concat": [cc[:, :, s:s + T].contiguous()]} for c in ctx]
            prep_w = model.prepare_branches((B, 4, T, H, W), brw, fs=fs)
            e = model.apply_model_rows(x[:, :, s:s + T].contiguous(), prep_w, torch.full((1, nb * B), t_step,
                                                                                          dtype=torch.int64, device=DEV))
            torch.cuda.synchronize()
            e = e.double().cpu().reshape(nb, B, T, H * W, 4)
            ref[:, :, s:s + T] += torch.from_numpy(wn[0, w].astype(np.float64)).view(1, 1, T, 1, 1) * e
        net._arena.check()
        r = [R.rel_l2(merged[k], ref[k]) for k in range(nb)]
        cos = [float((merged[k].flatten() @ ref[k].flatten()) / (merged[k].norm() * ref[k].norm())) for k in range(nb)]
        print(f"\n[real width, windowed step] 24 frames / 2 windows of 16 at 40x64, 4 clips in one forward vs per-window "
              f"batch-2 forwards: rel-L2 " + " / ".join(f"{v:.3e}" for v in r) + " cosine "
              + " / ".join(f"{v:.6f}" for v in cos) + f"; {n_guarded} guarded scratch buffers intact")
        assert torch.isfinite(merged).all() and n_guarded > 10
        assert max(r) < UNET_TOL and min(cos) > UNET_COS
    finally:
        if old is None:
            os.environ.pop("DC_ARENA_GUARD", None)
        else:
            os.environ["DC_ARENA_GUARD"] = old
        model = net = None
        gc.collect()
        torch.cuda.empty_cache()
