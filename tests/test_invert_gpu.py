"""DDIM inversion and partial denoising on the GPU: dc_ddim_invert_step against the float64 restatement
(tests/invert_restatement.py), the algebraic inverse of dc_ddim_step, a tiny-UNet inversion trajectory against the CPU
oracle, fused against generic, graph == eager with rewind, partial runs as the bitwise tail of a full run, decode on the
reference fixture, the harness function and the command line.

Stated tolerances (every test prints what it measures):
  dc_ddim_invert_step (fp32)     max-rel <= 1e-5 on x_next and pred_x0: dc_dpmpp_step's stated tolerance (measured 3.2e-7)
  inverse of dc_ddim_step        max-rel <= 1e-5 (the same arithmetic in fp32 numpy: 1.8e-7; measured 4.1e-7)
  6-step inversion trajectory    rel-L2 <= 8.5e-2, the project's multi-step bound for this tiny model (TRAJ_TOL)
  fused vs generic encode        <= 2x the rel-L2 of the forward fused / generic `sample` pair on the same inputs
  partial runs                   torch.equal with the tail of the full run, eager and graph
  decode on the fixture          rel-L2 <= 1e-1, the existing test's bound (tests/test_model_gpu.py)
"""
import os

import numpy as np
import pytest
import torch
import yaml

from oracle import ddim as oddim
from tests import invert_restatement as R
from tests.test_windows_gpu import TRAJ_TOL, _Generic, _tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")
V_KW = dict(rescale_betas_zero_snr=True, parameterization="v", use_dynamic_rescale=True, base_scale=0.7)


@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


# ------------------------------------------------------------------ 1. the kernel against the restatement
def _device_tables(sc, with_ratio):
    t = R.inverse_tables(sc)
    d = {ours: t[theirs].float().contiguous().to(DEV) for ours, theirs in
         (("inv_sqrt_a_src", "sa_src"), ("inv_sqrt_1ma_src", "s1_src"), ("inv_sqrt_a_dst", "sa_dst"),
          ("inv_sqrt_1ma_dst", "s1_dst"))}
    if with_ratio:
        d["inv_scale_ratio"] = t["r"].float().contiguous().to(DEV)
    return d


@pytest.mark.parametrize("nb", [1, 2, 3])
@pytest.mark.parametrize("v_param", [False, True], ids=["eps", "v"])
@pytest.mark.parametrize("B,C,THW", [(1, 4, 1024), (2, 4, 105), (1, 4, 16400)])
def test_invert_step_kernel_vs_restatement(B, C, THW, v_param, nb):
    """Both layouts (rows with ld_e = 16, NCHW), with and without scale_ratio, guidance rescale 0 and 0.7, host index and
    device counter, x_next aliasing x, over the steps of an S = 6 schedule (v: zero-terminal SNR, so the last step's
    destination level is 0)."""
    from dynamicrafter_amd import ops
    S = 6
    kw = dict(V_KW) if v_param else dict(parameterization="eps", use_dynamic_rescale=True, base_scale=0.7)
    sc_r = oddim.DDIMSchedule(oddim.ModelSchedule(**kw), S, "uniform_trailing", 0.0)
    sc_1 = oddim.DDIMSchedule(oddim.ModelSchedule(**dict(kw, use_dynamic_rescale=False)), S, "uniform_trailing", 0.0)
    g = torch.Generator().manual_seed(100 * B + THW + nb)
    n = B * C * THW
    ws = ops.step_workspace(B, DEV)
    worst, case = 0.0, 0
    for nchw in (False, True):
        for with_ratio in (False, True):
            sc = sc_r if with_ratio else sc_1
            tables = _device_tables(sc, with_ratio)
            for phi in (0.0, 0.7):
                k = case % S if case % 4 else S - 1                # every step shows up, the last one (a = 0 for v) often
                case += 1
                x = torch.randn(B, C, THW, generator=g)
                e = [torch.randn(B, C, THW, generator=g) for _ in range(nb)] + [None] * (3 - nb)
                ref_x, ref_p = R.invert_step(sc, x, k, e[0], e[1], e[2], cfg_scale=2.0, cfg_img=1.5, guidance_rescale=phi)
                if nchw:
                    dev_e = [None if t is None else t.contiguous().to(DEV) for t in e]
                else:
                    dev_e = []
                    for t in e:
                        rows = None
                        if t is not None:
                            rows = torch.full((B * THW, 16), float("nan"))       # columns past C are not the kernel's to read
                            rows[:, :C] = t.permute(0, 2, 1).reshape(B * THW, C)
                            rows = rows.to(DEV)
                        dev_e.append(rows)
                common = dict(B=B, Cc=C, THW=THW, v_param=v_param, cfg_scale=2.0, cfg_img=1.5, guidance_rescale=phi,
                              e_nchw=nchw)
                counter = torch.tensor([k], dtype=torch.int32, device=DEV)
                for sel, alias in ((dict(index=k), False), (dict(step_index=counter, index=(k + 1) % S), True)):
                    xd = torch.full((n + 5,), 7.0, device=DEV)
                    xd[:n] = x.flatten().to(DEV)
                    xn = xd if alias else torch.full((n + 5,), 7.0, device=DEV)
                    pd = torch.full((n + 5,), 7.0, device=DEV)
                    ops.ddim_invert_step(tables, dev_e[0], dev_e[1], dev_e[2], xd, xn, pd, ws, **common, **sel)
                    torch.cuda.synchronize()
                    assert bool((xn[n:] == 7.0).all()) and bool((pd[n:] == 7.0).all())       # nothing past the latent
                    assert torch.isfinite(xn[:n]).all() and torch.isfinite(pd[:n]).all()
                    rx, rp = R.max_rel(xn[:n].reshape(B, C, THW), ref_x), R.max_rel(pd[:n].reshape(B, C, THW), ref_p)
                    worst = max(worst, rx, rp)
                    assert rx <= 1e-5 and rp <= 1e-5, (nchw, with_ratio, phi, k, sel.keys(), rx, rp)
    print(f"\n[invert step B={B} C={C} THW={THW} {'v' if v_param else 'eps'} {nb} branches] worst max-rel {worst:.3e}")


# ------------------------------------------------------------------ 2. the algebraic inverse of dc_ddim_step
class _SchedModel:
    """The schedule buffers of a model on the GPU (oracle.ddim.ModelSchedule): enough for make_schedule."""

    def __init__(self, **kw):
        ms = oddim.ModelSchedule(**kw)
        self.ms = ms
        for k in ("num_timesteps", "parameterization", "use_dynamic_rescale"):
            setattr(self, k, getattr(ms, k))
        for k in ("alphas_cumprod", "betas", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
            setattr(self, k, getattr(ms, k).to(DEV))
        if ms.use_dynamic_rescale:
            self.scale_arr = ms.scale_arr.to(DEV)
        self.device = torch.device(DEV)


def test_ddim_step_undoes_the_invert_step():
    """eps-parameterisation with dynamic rescale, e_nchw, every k of S = 6: dc_ddim_step (eta = 0) on the inverse step's
    output with the same e returns x. Max-rel <= 1e-5; the same arithmetic in fp32 numpy gives 1.8e-7. Measured on MI355X:
    4.1e-7."""
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    S = 6
    s = DDIMSampler(_SchedModel(parameterization="eps", use_dynamic_rescale=True, base_scale=0.7))
    s.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=0.0, verbose=False)
    assert s.ddim_timesteps.shape[0] == S
    B, C, THW = 2, 4, 300
    g = torch.Generator().manual_seed(77)
    ws = ops.step_workspace(B, DEV)
    kw = dict(B=B, Cc=C, THW=THW, e_nchw=True)
    worst = 0.0
    for k in range(S):
        x = torch.randn(B, C, THW, generator=g).to(DEV)
        e = torch.randn(B, C, THW, generator=g).to(DEV)
        up, _ = ops.ddim_invert_step(s._tables, e, None, None, x, torch.empty_like(x), torch.empty_like(x), ws, index=k, **kw)
        down, _ = ops.ddim_step(s._tables, e, None, None, up, None, torch.empty_like(x), torch.empty_like(x), ws,
                                index=S - 1 - k, **kw)
        torch.cuda.synchronize()
        worst = max(worst, R.max_rel(down, x))
        assert R.max_rel(down, x) <= 1e-5, (k, R.max_rel(down, x))
    print(f"\n[invert then ddim step] worst max-rel over k = 0 .. {S - 1}: {worst:.3e}")


# ------------------------------------------------------------------ 3. inversion trajectory against the oracle
S6 = 6


def _inputs(seed=9, b=1, t=4, h=16, w=16, S=S6):
    g = torch.Generator().manual_seed(seed)
    return dict(x0=torch.randn(b, 4, t, h, w, generator=g),
                ctx=[torch.randn(b, 77 + 16 * t, 128, generator=g) for _ in range(3)],
                cc=torch.randn(b, 4, t, h, w, generator=g) * 0.2,
                noises=torch.randn(S, b, 4, t, h, w, generator=g),
                fs=torch.tensor([24] * b))


def _mk(inp, k):
    return {"c_crossattn": [inp["ctx"][k].to(DEV)], "c_concat": [inp["cc"].to(DEV)]}


def _sampler(model, eta=0.0, S=S6):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    s = DDIMSampler(model)
    s.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=eta, verbose=False)
    return s


def _guidance(nb):
    return {1: dict(), 2: dict(unconditional_guidance_scale=2.0, guidance_rescale=0.7),
            3: dict(unconditional_guidance_scale=2.0, guidance_rescale=0.7, cfg_img=1.5)}[nb]


def _encode(model, inp, nb, use_graph=False, n=S6, **kw):
    s = _sampler(model)
    g = _guidance(nb)
    if nb > 1:
        g["unconditional_conditioning"] = _mk(inp, 1)
    if nb > 2:
        g["unconditional_conditioning_img_nonetext"] = _mk(inp, 2)
    out, inter = s.encode(inp["x0"].to(DEV), _mk(inp, 0), n, fs=inp["fs"].to(DEV), use_graph=use_graph, **g, **kw)
    return out, inter, s


@pytest.mark.parametrize("nb", [1, 2])
def test_inversion_trajectory_vs_oracle(tiny, nb):
    """Fused `encode` with t_enc = S = 6 (v-param, zero-terminal SNR, dynamic rescale, uniform_trailing; the last step ends
    at level 0, where x = eps) against the restatement driving oracle.unet.unet_forward on the CPU: one branch, and two
    branches at guidance scale 2 with guidance rescale 0.7. Graph == eager bitwise; rewind() and a second run == the first.
    Measured on MI355X: rel-L2 9.48e-3 with one branch, 1.56e-2 with two (1.5x = 1.42e-2 / 2.34e-2, both under the
    bound 8.5e-2); eager and graph agree bitwise."""
    from oracle import unet as ounet
    from dynamicrafter_amd.lvdm.models.samplers.ddim import InvertRun
    model, sd, ocfg = tiny
    inp = _inputs()
    out, inter, s = _encode(model, inp, nb, return_intermediates=S6)
    assert isinstance(s._last_run, InvertRun) and s._last_run.graph is None and s._last_run.nb == nb
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == S6 and torch.equal(inter["x_inter"][-1], out)
    graph, _, sg = _encode(model, inp, nb, use_graph=True)
    assert sg._last_run.graph is not None
    # the oracle UNet is fp32; the inversion arithmetic around it is float64
    am = lambda x, tl, c, fs=None: ounet.unet_forward(sd, ocfg, torch.cat([x.float(), inp["cc"]], 1), tl, c, fs).double()
    sc = oddim.DDIMSchedule(oddim.ModelSchedule(**V_KW), S6, "uniform_trailing", 0.0)
    g = _guidance(nb)
    ref = R.invert_loop(am, sc, inp["x0"], inp["ctx"][0], inp["ctx"][1] if nb > 1 else None, n=S6,
                        cfg_scale=g.get("unconditional_guidance_scale", 1.0),
                        guidance_rescale=g.get("guidance_rescale", 0.0), fs=inp["fs"])
    r = R.rel_l2(out, ref)
    print(f"\n[inversion trajectory, {nb} branch(es)] 6 inverse steps vs oracle rel-L2 {r:.3e} (1.5x = {1.5 * r:.3e}, "
          f"bound {TRAJ_TOL})")
    assert torch.isfinite(out).all()
    assert torch.equal(out, graph)
    run = sg._last_run
    with pytest.raises(RuntimeError, match="rewind"):
        run.step()
    run.rewind(inp["x0"].to(DEV))
    for _ in range(S6):
        run.step()
    run.sync()
    assert torch.equal(run.img, out)
    assert r < TRAJ_TOL


# ------------------------------------------------------------------ 4. fused against generic encode
def _sample(model, inp, nb, use_graph=False, **kw):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    g = _guidance(nb)
    if nb > 1:
        g["unconditional_conditioning"] = _mk(inp, 1)
    if nb > 2:
        g["unconditional_conditioning_img_nonetext"] = _mk(inp, 2)
    s = DDIMSampler(model)
    x_T = inp["x0"]
    noises = kw.pop("noises", inp["noises"].to(DEV))
    out, inter = s.sample(S6, x_T.shape[0], tuple(x_T.shape[1:]), conditioning=_mk(inp, 0), verbose=False, eta=1.0,
                          x_T=x_T.to(DEV), fs=inp["fs"].to(DEV), timestep_spacing="uniform_trailing",
                          noises=noises, use_graph=use_graph, **g, **kw)
    return out, inter, s


@pytest.mark.parametrize("nb", [1, 2, 3])
def test_fused_vs_generic_encode(tiny, nb):
    """The fused inversion (InvertRun: one batched UNet forward per step, rows into the kernel) against the generic path
    (one apply_model per branch, NCHW into the same kernel) on the same inputs. The tolerance is twice what the forward
    fused / generic `sample` pair differs by on those inputs, measured here. Measured on MI355X for 1, 2 and 3 branches:
    forward pair 0 (bitwise equal at this size), encode pair 0."""
    model = tiny[0]
    inp = _inputs(seed=21)
    base = R.rel_l2(_sample(model, inp, nb)[0], _sample(_Generic(model), inp, nb)[0])
    fused, _, sf = _encode(model, inp, nb)
    generic, _, sg = _encode(_Generic(model), inp, nb)
    assert hasattr(sf, "_last_run") and not hasattr(sg, "_last_run")
    r = R.rel_l2(fused, generic)
    print(f"\n[fused vs generic encode, {nb} branch(es)] forward sample pair rel-L2 {base:.3e}, encode pair {r:.3e} "
          f"(allowed {2 * base:.3e})")
    assert torch.isfinite(fused).all() and torch.isfinite(generic).all()
    assert r <= 2 * base


# ------------------------------------------------------------------ 5. partial runs are the tail of a full run
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("nb", [2, 3])
def test_partial_runs_are_the_tail_of_the_full_run(tiny, nb, use_graph):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import FusedRun
    model = tiny[0]
    inp = _inputs(seed=33)
    full, inter, _ = _sample(model, inp, nb, log_every_t=1)
    assert len(inter["x_inter"]) == S6 + 1
    s = _sampler(model, eta=1.0)
    g = _guidance(nb)
    kw = dict(unconditional_guidance_scale=g["unconditional_guidance_scale"], unconditional_conditioning=_mk(inp, 1),
              fs=inp["fs"].to(DEV), guidance_rescale=g["guidance_rescale"], use_graph=use_graph)
    if nb > 2:
        kw.update(cfg_img=g["cfg_img"], unconditional_conditioning_img_nonetext=_mk(inp, 2))
    seen = []
    dec = s.decode(inter["x_inter"][2], _mk(inp, 0), 4, noises=inp["noises"][2:].to(DEV), callback=seen.append, **kw)
    assert isinstance(s._last_run, FusedRun) and s._last_run.S == 4 and (s._last_run.graph is not None) == use_graph
    assert seen == [0, 1, 2, 3]
    assert torch.isfinite(full).all() and torch.equal(dec, full)
    # timesteps=5 of S = 6: subset_end = 4, the same four steps from x_T
    assert s.subset_steps(5) == 4
    part, pi, _ = _sample(model, inp, nb, use_graph=use_graph, timesteps=5, noises=inp["noises"][:4].to(DEV), log_every_t=1)
    dec2 = s.decode(inp["x0"].to(DEV), _mk(inp, 0), 4, noises=inp["noises"][:4].to(DEV), **kw)
    assert len(pi["x_inter"]) == 5 and torch.equal(part, dec2) and not torch.equal(part, full)
    # an empty selection returns x_T unchanged
    same, si, _ = _sample(model, inp, nb, timesteps=1)
    assert torch.equal(same, inp["x0"].to(DEV)) and len(si["x_inter"]) == 1


def test_partial_run_with_a_mask_is_the_tail_too(tiny):
    model = tiny[0]
    inp = _inputs(seed=35)
    g = torch.Generator().manual_seed(5)
    q = torch.randn(S6, 1, 4, 4, 16, 16, generator=g).to(DEV)
    x0 = torch.randn(1, 4, 4, 16, 16, generator=g).to(DEV)
    mask = torch.zeros(1, 1, 4, 16, 16, device=DEV)
    mask[:, :, 0] = 1.0
    full, inter, _ = _sample(model, inp, 2, log_every_t=1, mask=mask, x0=x0, q_noises=q)
    s = _sampler(model, eta=1.0)
    gd = _guidance(2)
    for use_graph in (False, True):
        dec = s.decode(inter["x_inter"][3], _mk(inp, 0), 3, unconditional_conditioning=_mk(inp, 1), fs=inp["fs"].to(DEV),
                       noises=inp["noises"][3:].to(DEV), mask=mask, x0=x0, q_noises=q[3:], use_graph=use_graph, **gd)
        assert torch.equal(dec, full)
    # the generic path (separate apply_model calls, host index into the same tables) from its own intermediate
    gfull, ginter, _ = _sample(_Generic(model), inp, 2, log_every_t=1, mask=mask, x0=x0, q_noises=q)
    generic = _sampler(_Generic(model), eta=1.0)
    dec = generic.decode(ginter["x_inter"][3], _mk(inp, 0), 3, unconditional_conditioning=_mk(inp, 1), fs=inp["fs"].to(DEV),
                         noises=inp["noises"][3:].to(DEV), mask=mask, x0=x0, q_noises=q[3:], **gd)
    assert not hasattr(generic, "_last_run") and torch.equal(dec, gfull)


# ------------------------------------------------------------------ 6. decode on the committed reference fixture
def test_decode_on_the_reference_fixture_runs_fused():
    """tests/test_model_gpu.py's decode check (reference output decode/x_dec of sampler_extras, rel-L2 < 1e-1), now on the
    fused path: a partial FusedRun, eager and graph. Measured on MI355X: 4.7e-2."""
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler, FusedRun
    from tests.test_model_gpu import T, _tiny_lvd, load
    g = load("sampler_extras")
    model = _tiny_lvd("inference_512_v1.0.yaml")
    cond = {"c_crossattn": [T(g["ctx"])], "c_concat": [T(g["c_concat"])]}
    uc = {"c_crossattn": [T(g["uc_ctx"])], "c_concat": [T(g["c_concat"])]}
    outs = []
    for use_graph in (False, True):
        s = DDIMSampler(model)
        s.make_schedule(6, ddim_discretize="uniform", ddim_eta=0.0, verbose=False)
        dec = s.decode(T(g["decode/x_latent"]), cond, int(g["decode/t_start"]), unconditional_guidance_scale=7.5,
                       unconditional_conditioning=uc, use_graph=use_graph)
        assert isinstance(s._last_run, FusedRun) and s._last_run.S == int(g["decode/t_start"])
        outs.append(dec)
    r = R.rel_l2(outs[0], g["decode/x_dec"])
    print(f"\n[decode fixture, fused] rel-L2 {r:.3e} (bound 1e-1)")
    assert r < 1e-1 and torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------ 7. the harness
@pytest.fixture(scope="module")
def toy():
    return _tiny_model(toy_conditioners=True)[0]


@pytest.mark.parametrize("invert", [True, False])
def test_video_guided_synthesis_equals_the_composition(toy, invert):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.scripts.evaluation.edit import strength_steps, video_guided_synthesis
    from dynamicrafter_amd.scripts.evaluation.inference import build_conditioning, get_latent_z
    model = toy
    g = torch.Generator().manual_seed(6)
    b, t, H, W, S = 1, 4, 128, 128, 6
    videos = (torch.rand(b, 3, 1, H, W, generator=g) * 2 - 1).repeat(1, 1, t, 1, 1).to(DEV)
    source = (torch.rand(b, 3, t, H // 8, W // 8, generator=g) * 2 - 1).repeat_interleave(8, 3).repeat_interleave(8, 4).to(DEV)
    noise = torch.randn(b, 4, t, H // 8, W // 8, generator=g).to(DEV)
    shape = [b, 4, t, H // 8, W // 8]
    kw = dict(ddim_steps=S, ddim_eta=0.0, unconditional_guidance_scale=2.0, fs=24, text_input=True,
              timestep_spacing="uniform_trailing", guidance_rescale=0.7, strength=0.6, invert=invert)
    n = strength_steps(0.6, S)
    assert n == 4
    torch.manual_seed(0)
    out = video_guided_synthesis(model, ["a corgi"], videos, source, shape, noise=None if invert else noise, **kw)
    assert tuple(out.shape) == (b, 1, 3, t, H, W) and torch.isfinite(out).all() and float(out.std()) > 1e-3
    # the composition by hand, in the function's documented order
    torch.manual_seed(0)
    fs = torch.tensor([24] * b, dtype=torch.long, device=DEV)
    s = DDIMSampler(model)
    s.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=0.0, verbose=False)
    cond, uc, uc_2 = build_conditioning(model, ["a corgi"], videos, 2.0)
    assert uc is not None and uc_2 is None
    z = get_latent_z(model, source)
    if invert:
        cond_src, uc_src, _ = build_conditioning(model, [""], source[:, :, :1], 1.0, num_frames=t)
        assert uc_src is None
        x, _ = s.encode(z, cond_src, n, fs=fs)
    else:
        x = s.stochastic_encode(z, torch.full((b,), n - 1, dtype=torch.long, device=DEV), noise=noise)
    lat = s.decode(x, cond, n, unconditional_guidance_scale=2.0, unconditional_conditioning=uc, fs=fs, guidance_rescale=0.7)
    assert s._last_run.S == n
    want = model.decode_first_stage(lat)
    assert torch.equal(out[:, 0], want)


def test_video_guided_synthesis_full_strength_runs_every_step(toy):
    from dynamicrafter_amd.lvdm.models.samplers import ddim as D
    from dynamicrafter_amd.scripts.evaluation.edit import video_guided_synthesis
    g = torch.Generator().manual_seed(8)
    b, t, H, W, S = 1, 4, 128, 128, 6
    videos = (torch.rand(b, 3, 1, H, W, generator=g) * 2 - 1).repeat(1, 1, t, 1, 1).to(DEV)
    source = (torch.rand(b, 3, t, H, W, generator=g) * 2 - 1).to(DEV)
    made = []
    inv_init, fused_init = D.InvertRun.__init__, D.FusedRun.__init__

    def spy(init, tag):
        def wrapped(self, *a, **k):
            init(self, *a, **k)
            made.append((tag, self.S))
        return wrapped
    D.InvertRun.__init__, D.FusedRun.__init__ = spy(inv_init, "invert"), spy(fused_init, "denoise")
    try:
        out = video_guided_synthesis(toy, [""], videos, source, [b, 4, t, H // 8, W // 8], ddim_steps=S, fs=24,
                                     timestep_spacing="uniform_trailing", strength=1.0)
    finally:
        D.InvertRun.__init__, D.FusedRun.__init__ = inv_init, fused_init
    assert made == [("invert", S), ("denoise", S)]
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------ 8. end to end through the command line
def test_edit_command_line_end_to_end(tmp_path):
    from PIL import Image
    from dynamicrafter_amd.scripts.evaluation import edit
    from dynamicrafter_amd.scripts.evaluation.funcs import load_video_batch, save_videos
    from dynamicrafter_amd.utils.utils import instantiate_from_config
    from oracle.weights import fill_state_dict
    from tests.golden_cfg import TINY_AE, TINY_RESAMPLER, TINY_UNET
    root = os.path.join(os.path.dirname(__file__), "..", "dynamicrafter_amd", "configs")
    cfg = yaml.safe_load(open(os.path.join(root, "inference_512_v1.0.yaml")))
    p = cfg["model"]["params"]
    p["unet_config"]["params"] = dict(TINY_UNET, default_fs=24)
    p["first_stage_config"]["params"]["ddconfig"] = dict(TINY_AE)
    p["cond_stage_config"] = {"target": "tests.golden_cfg.ToyTextEmbedder"}
    p["img_cond_stage_config"] = {"target": "tests.golden_cfg.ToyImageEmbedder"}
    p["image_proj_stage_config"] = {"target": "lvdm.modules.encoders.resampler.Resampler", "params": dict(TINY_RESAMPLER)}
    with open(str(tmp_path / "tiny.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
    model = instantiate_from_config(cfg["model"])
    for mod, seed in ((model.model.diffusion_model, 11), (model.first_stage_model, 13), (model.image_proj_model, 14)):
        sdict = mod.state_dict()
        mod.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in sdict.items()}, seed), strict=True)
    torch.save({"state_dict": model.state_dict()}, str(tmp_path / "tiny.ckpt"))
    del model
    size, t = 128, 4
    stems = ["a_dog", "b_sea"]
    prompts, sources, out = tmp_path / "prompts", tmp_path / "sources", tmp_path / "out"
    prompts.mkdir(); sources.mkdir()
    rng = np.random.default_rng(4)
    for stem in stems:
        Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(str(prompts / f"{stem}.png"))
    (prompts / "prompts.txt").write_text("a corgi runs\nwaves on a beach\n")
    (tmp_path / "source_prompts.txt").write_text("a dog runs\nthe sea\n")
    g = torch.Generator().manual_seed(12)
    clips = (torch.rand(2, 1, 3, t, size // 8, size // 8, generator=g) * 2 - 1).repeat_interleave(8, 4).repeat_interleave(8, 5)
    written = save_videos(clips.to(DEV), str(sources), stems, container="avi")
    assert [os.path.basename(w) for w in written] == [s + ".avi" for s in stems]
    assert tuple(load_video_batch(written, 1, (size, size), t, device=DEV).shape) == (2, 3, t, size, size)
    common = ["--config", str(tmp_path / "tiny.yaml"), "--ckpt_path", str(tmp_path / "tiny.ckpt"), "--prompt_dir", str(prompts),
              "--source_dir", str(sources), "--height", str(size), "--width", str(size), "--ddim_steps", "4",
              "--video_length", str(t), "--frame_stride", "24", "--text_input", "--unconditional_guidance_scale", "2.0",
              "--timestep_spacing", "uniform_trailing", "--guidance_rescale", "0.7", "--strength", "0.5", "--seed", "123"]
    for extra, sub in ((["--source_prompt_file", str(tmp_path / "source_prompts.txt")], "inv"),
                       (["--no_invert", "--container", "avi"], "sde")):
        files = edit.main(common + ["--savedir", str(out / sub)] + extra)
        ext = "avi" if "avi" in extra else "png"
        assert [os.path.relpath(f, str(out / sub)) for f in files] == \
            [os.path.join("samples_separate", f"{stem}_sample0.{ext}") for stem in stems]
        for f in files:
            assert os.path.getsize(f) > 0
            if ext == "avi":
                clip = load_video_batch([f], 1, (size, size), t, device=DEV)
                assert tuple(clip.shape) == (1, 3, t, size, size) and torch.isfinite(clip).all()
            else:
                im = Image.open(f)
                assert im.size == (size, size) and getattr(im, "n_frames", 1) == t
    with pytest.raises(FileNotFoundError):
        os.remove(written[1])
        edit.main(common + ["--savedir", str(out / "missing")])
