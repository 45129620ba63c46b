"""Adaptive projected guidance on the GPU: ops.apg_guide (csrc/guidance.hip) against the float64 restatement
(tests/apg_restatement.py), exact cases on small-integer data, the running update under the device step counter, and the samplers
with `apg=` on the tiny model.

Stated tolerances (every test prints what it measures):
  op vs float64       max |got - ref64| / rms(ref64) per clip <= 4 x the same figure of the restatement run in fp32 torch on the
                      CPU on the same inputs: another summation order, the same precision class (measured on MI355X: kernel
                      at most 8.1e-7, fp32 torch at most 2.1e-6, worst ratio 1.07)
  equal predictions   the output is e_c, bit for bit
  eta = 1, plain      within 1 ulp of the fp32 expression e_c + (w - 1) (e_c - e_u)
  orthogonal update   eta has no effect, bit for bit
  parallel update     |got - p_c| <= ((w - 1) |alpha| 2^-23 + 2^-24) |p_c| for D = alpha p_c: g = (1 - eta) s (m . p_c) / ||p_c||^2
                      is rounded to fp32 once, as is s, and the output once more
  +-1 difference      at norm_threshold = sqrt(N) / 2 the applied update is exactly half the unclipped one
  momentum buffer     |m - ref64| <= 2^-21 max(|d|, |m|): per step two roundings in d = ps (e_c - e_u) and one in the
                      multiply-add, (2 |d| + |m|) 2^-24 <= 3 * 2^-24 max, and |momentum| = 0.5 carries at most as much again
  graph vs eager, rewind, apg=None   torch.equal
  fused vs generic    rel-L2 <= 2 x the rel-L2 of the plain fused / generic pair on the same inputs (tests/test_invert_gpu.py's rule)
  on vs off           rel-L2 > 1e-3
"""
import math

import pytest
import torch

from tests import apg_restatement as R
from tests.test_windows_gpu import _Generic, _tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = 7.5
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 4, 8, 8), (1, 16, 32, 32)]           # [B, 4, T, H, W] latents
LAYOUTS = ["rows", "rows8", "nchw"]
MODES = [("model", True), ("x0", True), ("x0", False)]                         # (space, v_param)
AMPS = (1.0, 10.0, 0.1)                                                         # per clip: a reduction leaking across clips shows
SENTINEL = 12345.0
GUARD = 64


def rel_l2(a, b):
    a = torch.as_tensor(a).float().cpu(); b = torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _tables(S=3):
    """fp32 per-step tables with a_t > 0, different at every step."""
    a = torch.linspace(0.15, 0.9, S, dtype=torch.float64)
    t = {"a_t": a, "sqrt_one_minus_at": (1 - a).sqrt(), "sqrt_acp_t": a.sqrt(), "sqrt_1macp_t": (1 - a).sqrt()}
    return {k: v.float().contiguous().to(DEV) for k, v in t.items()}


def _coefs(tables, i, v_param):
    """sqrt(a_t), sqrt(1 - a_t) of step i as the restatement takes them: the fp32 table entries (eps: the root of the entry)."""
    if v_param:
        return float(tables["sqrt_acp_t"][i]), float(tables["sqrt_1macp_t"][i])
    return math.sqrt(float(tables["a_t"][i])), float(tables["sqrt_one_minus_at"][i])


def _to_layout(e, layout):
    """[B, C, T, H, W] fp32 on the CPU -> (the device operand, ld_e or None)"""
    B, Cc = e.shape[:2]
    if layout == "nchw":
        return e.contiguous().to(DEV), None
    rows = e.permute(0, 2, 3, 4, 1).reshape(-1, Cc)
    if layout == "rows":
        return rows.contiguous().to(DEV), None
    wide = torch.full((rows.shape[0], 8), SENTINEL)
    wide[:, :Cc] = rows
    return wide.to(DEV), 8


def _guide(e_c, e_u, x, m_prev, layout, *, tables=None, index=0, step_index=None, **kw):
    """ops.apg_guide on CPU inputs [B, C, T, H, W] -> (guided [B, C, T, H, W], m) on the CPU. out and the momentum buffer sit in
    front of sentinel elements, and the pad columns of padded rows hold sentinels: all of them must come back untouched."""
    from dynamicrafter_amd import ops
    B, Cc = e_c.shape[:2]
    THW = e_c[0, 0].numel()
    n = B * Cc * THW
    ec, ld = _to_layout(e_c, layout)
    eu, _ = _to_layout(e_u, layout)
    m_full = torch.full((n + GUARD,), SENTINEL, device=DEV)
    m_full[:n] = (torch.zeros(n) if m_prev is None else m_prev.reshape(-1)).to(DEV)
    if layout == "rows8":
        out_full = torch.full((B * THW, 8), SENTINEL, device=DEV)
        out = out_full[:, :Cc]
    else:
        out_full = torch.full((n + GUARD,), SENTINEL, device=DEV)
        out = out_full[:n].view(B, Cc, THW) if layout == "nchw" else out_full[:n].view(B * THW, Cc)
    ws = torch.full((ops.apg_workspace_floats(B=B, Cc=Cc, THW=THW),), float("nan"), device=DEV)      # needs no clearing
    ops.apg_guide(tables or {}, ec, eu, None if x is None else x.contiguous().to(DEV), m_full[:n], out, ws, B=B, Cc=Cc, THW=THW,
                  cfg_scale=W, index=index, step_index=step_index, e_nchw=layout == "nchw", ld_e=ld, **kw)
    torch.cuda.synchronize()
    if layout == "rows8":
        assert (out_full[:, Cc:] == SENTINEL).all()
        got = out_full[:, :Cc].cpu()
    else:
        assert (out_full[n:] == SENTINEL).all()
        got = out_full[:n].cpu()
    assert (m_full[n:] == SENTINEL).all()
    if layout != "nchw":
        got = got.reshape(B, *e_c.shape[2:], Cc).permute(0, 4, 1, 2, 3)
    return got.reshape(e_c.shape).contiguous(), m_full[:n].cpu().reshape(e_c.shape)


def _random(shape, seed):
    B = shape[0]
    g = torch.Generator().manual_seed(seed)
    full = (B, 4) + tuple(shape[1:])
    amp = torch.tensor([AMPS[b % 3] for b in range(B)]).view(B, 1, 1, 1, 1)
    e_c, e_u, x, m_prev = (torch.randn(full, generator=g) for _ in range(4))
    return e_c * amp, (e_c + 0.4 * e_u) * amp, x * amp, 0.7 * m_prev * amp


def _ints(shape, seed, lo=-3, hi=4):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).float()


# ------------------------------------------------------------------ 1. the op against the float64 restatement
@pytest.mark.parametrize("space,v_param", MODES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_op_vs_restatement(shape, layout, space, v_param):
    e_c, e_u, x, m_prev = _random(shape, seed=sum(shape))
    tables = _tables()
    sa, s1 = _coefs(tables, 1, v_param)
    # half the norm of clip 0's running update: clips 0 and 1 (x 10) are clipped, clip 2 (x 0.1) is not
    _, m64 = R.apg(e_c, e_u, x, m_prev, w=W, momentum=-0.5, space=space, v_param=v_param, sqrt_a=sa, sqrt_1ma=s1)
    norms = m64.flatten(1).norm(dim=1)
    kw = dict(eta=0.25, norm_threshold=0.5 * norms[0].item(), momentum=-0.5, space=space, v_param=v_param)
    if shape[0] == 3:
        assert norms[1] > kw["norm_threshold"] > norms[2]
    ref, m_ref = R.apg(e_c, e_u, x, m_prev, w=W, sqrt_a=sa, sqrt_1ma=s1, **kw)
    f32, _ = R.apg(e_c, e_u, x, m_prev, w=W, sqrt_a=sa, sqrt_1ma=s1, dtype=torch.float32, **kw)
    got, m = _guide(e_c, e_u, x if space == "x0" else None, m_prev, layout, tables=tables, index=1, **kw)
    again, _ = _guide(e_c, e_u, x if space == "x0" else None, m_prev, layout, tables=tables, index=1, **kw)
    rms = ref.flatten(1).pow(2).mean(1).sqrt()
    err = (got.double() - ref).flatten(1).abs().amax(1) / rms
    yard = (f32.double() - ref).flatten(1).abs().amax(1) / rms
    print(f"\n[apg op {shape} {layout} {space} {'v' if v_param else 'eps'}] max-abs / rms per clip: kernel "
          f"{[f'{v:.2e}' for v in err.tolist()]}, fp32 torch {[f'{v:.2e}' for v in yard.tolist()]}")
    assert torch.isfinite(got).all()
    assert (err <= 4.0 * yard).all()
    m_scale = m_ref.flatten(1).abs().amax(1) + 0.5 * m_prev.double().flatten(1).abs().amax(1)        # >= max(|d|, |m|) per clip
    assert ((m.double() - m_ref).flatten(1).abs().amax(1) <= 2.0 ** -21 * m_scale).all()
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))           # two runs, the same bits


# ------------------------------------------------------------------ 2. exact cases on small-integer data
EXACT_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 16, 32, 32)]


@pytest.mark.parametrize("space,v_param", MODES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_equal_predictions_return_the_conditional_one_bitwise(shape, layout, space, v_param):
    full = (shape[0], 4) + tuple(shape[1:])
    e_c, x = _ints(full, 1), _ints(full, 2)
    got, m = _guide(e_c, e_c.clone(), x if space == "x0" else None, None, layout, tables=_tables(), index=2, eta=0.0,
                    norm_threshold=1.5, momentum=-0.5, space=space, v_param=v_param)
    assert torch.equal(got.view(torch.int32), e_c.view(torch.int32))
    assert not m.any()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_eta_one_is_plain_cfg_within_one_ulp(shape, layout):
    full = (shape[0], 4) + tuple(shape[1:])
    e_c, e_u = _ints(full, 3), _ints(full, 4)
    got, m = _guide(e_c, e_u, None, None, layout, eta=1.0, norm_threshold=None, momentum=0.0, space="model", v_param=True)
    expr = e_c + (W - 1.0) * (e_c - e_u)                               # fp32 torch on the CPU
    ulp = (torch.nextafter(expr.abs(), torch.full_like(expr, math.inf)) - expr.abs())
    print(f"\n[apg eta=1 {shape} {layout}] max |got - expr| / ulp = {((got - expr).abs() / ulp).max().item():.2f}")
    assert ((got - expr).abs() <= ulp).all()
    assert torch.equal(m, e_c - e_u)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_orthogonal_update_ignores_eta_bitwise(shape, layout):
    """Pairs of elements (a, b) of p_c meet (b, -a) of d: D . p_c = 0 exactly, so par = 0 whatever eta is."""
    full = (shape[0], 4) + tuple(shape[1:])
    e_c = _ints(full, 5)
    pairs = e_c.reshape(-1, 2)
    d = torch.stack([pairs[:, 1], -pairs[:, 0]], 1).reshape(full)
    assert not (d * e_c).flatten(1).sum(1).any()
    outs = [_guide(e_c, e_c - d, None, None, layout, eta=eta, norm_threshold=0.75, momentum=0.0, space="model", v_param=True)[0]
            for eta in (0.0, 0.5, 1.0)]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert torch.equal(outs[0].view(torch.int32), outs[2].view(torch.int32))
    if e_c.any():
        assert not torch.equal(outs[0], e_c)                           # the update itself is applied


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_parallel_update_with_eta_zero_returns_the_conditional_one(shape, layout):
    full = (shape[0], 4) + tuple(shape[1:])
    e_c, alpha = _ints(full, 6), 0.5
    got, _ = _guide(e_c, e_c - alpha * e_c, None, None, layout, eta=0.0, norm_threshold=None, momentum=0.0, space="model",
                    v_param=True)
    bound = ((W - 1.0) * alpha * 2.0 ** -23 + 2.0 ** -24) * e_c.abs()
    print(f"\n[apg parallel {shape} {layout}] max |got - p_c| = {(got - e_c).abs().max().item():.3e}")
    assert ((got - e_c).abs() <= bound).all()
    plain, _ = _guide(e_c, e_c - alpha * e_c, None, None, layout, eta=1.0, norm_threshold=None, momentum=0.0, space="model",
                      v_param=True)
    assert torch.equal(plain, e_c + (W - 1.0) * alpha * e_c)           # with eta = 1 the same update is kept


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(4, 4, 4), (16, 32, 32)])           # N = 256 (one workgroup) and 65536 (64 of them)
def test_norm_threshold_halves_a_unit_difference(shape, layout):
    full = (1, 4) + shape
    N = 4 * shape[0] * shape[1] * shape[2]
    root = math.isqrt(N)
    assert root * root == N
    e_c = _ints(full, 7)
    d = _ints(full, 8, 0, 2) * 2 - 1                                   # all +-1: ||d|| = sqrt(N)
    kw = dict(eta=1.0, momentum=0.0, space="model", v_param=True)
    free, _ = _guide(e_c, e_c - d, None, None, layout, norm_threshold=None, **kw)
    clipped, _ = _guide(e_c, e_c - d, None, None, layout, norm_threshold=root / 2, **kw)
    loose, _ = _guide(e_c, e_c - d, None, None, layout, norm_threshold=float(root), **kw)
    assert torch.equal(free - e_c, (W - 1.0) * d)
    assert torch.equal(clipped - e_c, 0.5 * (free - e_c))
    assert torch.equal(loose, free)                                    # at the threshold: s = 1


# ------------------------------------------------------------------ 3. momentum under the device step counter
@pytest.mark.parametrize("space,v_param", MODES)
def test_momentum_recurrence_with_the_device_counter(space, v_param):
    from dynamicrafter_amd import ops
    S, shape = 3, (2, 3, 5, 7)
    B, THW = shape[0], shape[1] * shape[2] * shape[3]
    tables = _tables(S)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    m_dev = torch.zeros((B, 4) + shape[1:], device=DEV)
    out = torch.empty(B * THW, 4, device=DEV)
    ws = torch.empty(ops.apg_workspace_floats(B=B, Cc=4, THW=THW), device=DEV)
    kw = dict(eta=0.0, norm_threshold=3.0, momentum=-0.5, space=space, v_param=v_param)
    m_ref = None
    for k in range(S):
        e_c, e_u, x, _ = _random(shape, seed=100 + k)
        ops.apg_guide(tables, _to_layout(e_c, "rows")[0], _to_layout(e_u, "rows")[0], x.to(DEV), m_dev, out, ws, B=B, Cc=4,
                      THW=THW, cfg_scale=W, step_index=counter, **kw)
        ops.advance_counter(counter)
        torch.cuda.synchronize()
        sa, s1 = _coefs(tables, k, v_param)                            # the step's own table row: the counter was read
        m_before = m_ref
        ref, m_ref = R.apg(e_c, e_u, x, m_before, w=W, sqrt_a=sa, sqrt_1ma=s1, **kw)
        f32, _ = R.apg(e_c, e_u, x, m_before, w=W, sqrt_a=sa, sqrt_1ma=s1, dtype=torch.float32, **kw)
        got = out.cpu().reshape(B, *shape[1:], 4).permute(0, 4, 1, 2, 3)
        ps = 1.0 if space == "model" else s1 if v_param else s1 / sa   # |factor of e in p|: d = ps (e_c - e_u)
        scale = max((e_c - e_u).abs().max().item() * ps, m_ref.abs().max().item())
        m_err = (m_dev.cpu().double() - m_ref).abs().max().item()
        rms = ref.flatten(1).pow(2).mean(1).sqrt()
        err = (got.double() - ref).flatten(1).abs().amax(1) / rms
        yard = (f32.double() - ref).flatten(1).abs().amax(1) / rms
        print(f"\n[apg momentum {space} {'v' if v_param else 'eps'} step {k}] |m - ref| = {m_err:.3e} (bound {2.0 ** -21 * scale:.3e}); "
              f"output max-abs / rms per clip: kernel {[f'{v:.2e}' for v in err.tolist()]}, fp32 torch {[f'{v:.2e}' for v in yard.tolist()]}")
        assert m_err <= 2.0 ** -21 * scale
        assert (err <= 4.0 * yard).all()                               # the step's own row of the tables, test 1's rule
    assert int(counter.item()) == S


# ------------------------------------------------------------------ 4. the samplers on the tiny model
@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


def _inputs(S, seed=9, b=1, t=4, h=16, w=16, T=4):
    g = torch.Generator().manual_seed(seed)
    return dict(x=torch.randn(b, 4, t, h, w, generator=g), ctx=[torch.randn(b, 77 + 16 * T, 128, generator=g) for _ in range(2)],
                cc=torch.randn(b, 4, t, h, w, generator=g) * 0.2, noises=torch.randn(S, b, 4, t, h, w, generator=g),
                fs=torch.tensor([24] * b))


def _mk(inp, k):
    return {"c_crossattn": [inp["ctx"][k].to(DEV)], "c_concat": [inp["cc"].to(DEV)]}


def _sample(sampler, inp, S, **kw):
    out, _ = sampler.sample(S=S, batch_size=inp["x"].shape[0], shape=tuple(inp["x"].shape[1:]), conditioning=_mk(inp, 0),
                            verbose=False, unconditional_guidance_scale=W, unconditional_conditioning=_mk(inp, 1), eta=1.0,
                            x_T=inp["x"].to(DEV), fs=inp["fs"].to(DEV), timestep_spacing="uniform_trailing",
                            noises=inp["noises"].to(DEV), **kw)
    return out.clone()


def _run(model, inp, S, apg, graph=False):
    """A FusedRun of S steps built by hand (what the sampler builds), and the norm of its running update after every step."""
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler, FusedRun
    s = DDIMSampler(model)
    s.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    with torch.no_grad():
        run = FusedRun(s, inp["x"].to(DEV).clone(), [_mk(inp, 0), _mk(inp, 1)], fs=inp["fs"].to(DEV), noises=inp["noises"].to(DEV),
                       cfg_scale=W, apg=apg)
        if graph:
            run.capture()
    return run


def _steps(run):
    norms = []
    with torch.no_grad():
        for _ in range(run.S):
            run.step()
            run.sync()
            norms.append(run.apg_m.double().norm().item())
    return norms


@pytest.fixture(scope="module")
def apg3(tiny):
    """apg= for the 3-step runs: the threshold is half the ||d|| of the first step of these inputs, which every run from the
    same x_T meets (m = d there), so the clip is active at least in that step."""
    model, _, _ = tiny
    norms = _steps(_run(model, _inputs(3), 3, dict(eta=0.0, norm_threshold=None, momentum=0.0)))
    print(f"\n[apg tiny model] ||d|| per step (x0 space): {[f'{v:.3f}' for v in norms]}")
    assert all(math.isfinite(v) and v > 0 for v in norms)
    return dict(eta=0.0, norm_threshold=0.5 * norms[0], momentum=-0.5)


def test_fused_run_clips_and_rewinds_bitwise(tiny, apg3):
    model, _, _ = tiny
    inp = _inputs(3)
    run = _run(model, inp, 3, apg3, graph=True)
    first = _steps(run)
    img, m = run.img.clone(), run.apg_m.clone()
    print(f"\n[apg rewind] ||m|| per step {[f'{v:.3f}' for v in first]}, threshold {apg3['norm_threshold']:.3f}")
    assert first[0] > apg3["norm_threshold"]                          # the clip is active in at least one step
    run.rewind(inp["x"].to(DEV))
    assert not run.apg_m.any()                                        # the running update starts from zero again
    second = _steps(run)
    assert second == first and torch.equal(run.img, img) and torch.equal(run.apg_m, m)
    eager = _run(model, inp, 3, apg3)
    assert _steps(eager) == first and torch.equal(eager.img, img)     # and the captured step is the eager step


def test_ddim_with_apg_graph_equals_eager_and_differs_from_off(tiny, apg3):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    model, _, _ = tiny
    inp = _inputs(3)
    eager = _sample(DDIMSampler(model), inp, 3, apg=apg3, use_graph=False)
    graph = _sample(DDIMSampler(model), inp, 3, apg=apg3, use_graph=True)
    plain = _sample(DDIMSampler(model), inp, 3, use_graph=True)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graph)
    print(f"\n[3-step DDIM, APG] on vs off rel-L2 {rel_l2(eager, plain):.3e}")
    assert rel_l2(eager, plain) > 1e-3
    for space in ("model",):                                          # the other space runs too and is another result
        other = _sample(DDIMSampler(model), inp, 3, apg=dict(apg3, space=space), use_graph=True)
        assert torch.isfinite(other).all() and rel_l2(other, eager) > 1e-3


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_fused_vs_generic(tiny, apg3, solver):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    """The fused run (one batched UNet forward per step, rows into the APG kernels) against the generic path (one apply_model
    per branch, NCHW into the same kernels, whose threads own a position in either layout and so add in the same order). The
    tolerance is twice what the plain fused / generic `sample` pair differs by on the same inputs, measured here: on MI355X
    that pair is bitwise equal at this size (0), and so is the APG pair."""
    model, _, _ = tiny
    inp = _inputs(3)
    mk = (lambda m: DDIMSampler(m)) if solver == "ddim" else (lambda m: DPMSolverSampler(m, solver=solver))
    fused, generic = _sample(mk(model), inp, 3, apg=apg3), _sample(mk(_Generic(model)), inp, 3, apg=apg3)
    fused0, generic0 = _sample(mk(model), inp, 3), _sample(mk(_Generic(model)), inp, 3)
    r, r0 = rel_l2(fused, generic), rel_l2(fused0, generic0)
    print(f"\n[{solver}, APG] fused vs generic rel-L2 {r:.3e}; the plain pair {r0:.3e}; on vs off {rel_l2(fused, fused0):.3e}")
    assert torch.isfinite(fused).all() and torch.isfinite(generic).all()
    assert r <= 2.0 * r0
    assert rel_l2(fused, fused0) > 1e-3


def test_dpm_solver_windows_and_decode_with_apg(tiny, apg3):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    model, _, _ = tiny
    inp = _inputs(3)
    for solver in ("dpmpp_2m", "dpmpp_2m_sde"):
        on = _sample(DPMSolverSampler(model, solver=solver), inp, 3, apg=apg3, use_graph=True)
        off = _sample(DPMSolverSampler(model, solver=solver), inp, 3, use_graph=True)
        assert torch.isfinite(on).all() and rel_l2(on, off) > 1e-3
        assert torch.equal(on, _sample(DPMSolverSampler(model, solver=solver), inp, 3, apg=apg3, use_graph=False))
    long = _inputs(3, seed=10, t=8)                                   # T = 8 over windows of 4
    # the norms run over the whole long clip: twice the elements, so the threshold grows by sqrt(2)
    apg_long = dict(apg3, norm_threshold=apg3["norm_threshold"] * math.sqrt(2.0))
    on = _sample(DDIMSampler(model), long, 3, apg=apg_long, window_stride=2, use_graph=True)
    off = _sample(DDIMSampler(model), long, 3, window_stride=2, use_graph=True)
    assert torch.isfinite(on).all() and rel_l2(on, off) > 1e-3
    assert torch.equal(on, _sample(DDIMSampler(model), long, 3, apg=apg_long, window_stride=2, use_graph=False))
    s = DDIMSampler(model)
    s.make_schedule(4, ddim_discretize="uniform_trailing", ddim_eta=0.0, verbose=False)
    x_mid = s.stochastic_encode(inp["x"].to(DEV) * 0.5, torch.tensor([1], device=DEV), noise=inp["noises"][0].to(DEV))
    dec = lambda **kw: s.decode(x_mid, _mk(inp, 0), 2, unconditional_guidance_scale=W, unconditional_conditioning=_mk(inp, 1),
                                fs=inp["fs"].to(DEV), **kw).clone()
    d_on, d_off = dec(apg=apg3), dec()
    assert torch.isfinite(d_on).all() and rel_l2(d_on, d_off) > 1e-3
    assert torch.equal(dec(apg=apg3, use_graph=True), d_on)
    assert s._last_run.S == 2 and s._last_run.apg is not None


# ------------------------------------------------------------------ 5. apg=None is never having passed it
def test_apg_none_is_bitwise_the_plain_run(tiny):
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    model, _, _ = tiny
    inp = _inputs(3)
    launches = []
    real = ops.apg_guide
    try:
        ops.apg_guide = lambda *a, **k: (launches.append(1), real(*a, **k))[1]
        s0, s1 = DDIMSampler(model), DDIMSampler(model)
        never = _sample(s0, inp, 3, guidance_rescale=0.7, use_graph=True)
        none = _sample(s1, inp, 3, guidance_rescale=0.7, use_graph=True, apg=None)
        assert launches == []
        _sample(DDIMSampler(model), inp, 3, apg=dict(eta=0.5))
        assert len(launches) == 3                                     # one call (two launches) per step
    finally:
        ops.apg_guide = real
    assert torch.equal(never, none)
    for run in (s0._last_run, s1._last_run):
        assert run.apg is None and not any(hasattr(run, a) for a in ("apg_m", "apg_out", "apg_ws", "apg_kw"))
    assert run.kw["cfg_scale"] == W and run.kw["guidance_rescale"] == 0.7
