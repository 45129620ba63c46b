"""Spatially tiled sampling (frames larger than the trained size) on the GPU: the two kernels against dc_pack_latent / the
float64 restatement, the one-tile identity, fused against generic, a tiny-UNet trajectory against the CPU oracle driven
per box, graph == eager with rewind and chunks, the composition with temporal windows, the harness, the scratch bound.

Stated tolerances (every test prints what it measures):
  dc_pack_latent_tiles          torch.equal (bit pattern) with dc_pack_latent on the cropped tensors
  dc_tile_merge (fp32)          <= 1 ulp from the restatement that accumulates in float64 and rounds per term (the one
                                admitted cause: double rounding); chunked == unchunked and a single box of
                                weight 1 == its input bit for bit; a weight-0 box is never read
  one-tile run                  torch.equal with the plain run (final sample and every intermediate)
  fused vs generic, tiled       <= 2x the rel-L2 of the untiled fused / generic pair of the same size
  4-step tiled trajectory       rel-L2 <= 8.5e-2, the project's multi-step bound for this tiny model
  tiles + degenerate space      torch.equal with the windowed path
"""
import numpy as np
import pytest
import torch

from tests import tiles_restatement as R
from tests.test_windows_gpu import TRAJ_TOL, _Generic, _tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _plan(long_shape, box_shape, stride, weights="triangle", shift=(0, 0, 0), S=1, multiple_of=1):
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers.tiles import tile_plan
    box, g = tile_plan(long_shape, box_shape, stride, weights, shift, S, multiple_of)
    return ops.tile_tables(box, g, long_shape=long_shape, box_shape=box_shape, device=DEV)


def _raw_plan(box, g, long_shape, box_shape):
    """Device tables as given, without the host check: what the kernels' own clamping and skipping are tested with."""
    box = np.ascontiguousarray(box, dtype=np.int32)
    g = np.ascontiguousarray(g, dtype=np.float32)
    return dict(box=torch.from_numpy(box).to(DEV), g=torch.from_numpy(g).to(DEV), S=box.shape[0], W=box.shape[1],
                long_shape=tuple(long_shape), box_shape=tuple(box_shape), host_box=box, host_g=g)


# ------------------------------------------------------------------ 1. dc_pack_latent_tiles
@pytest.mark.parametrize("Cx,Cc,c_pad", [(4, 4, 64), (4, 5, 16), (4, 4, 8), (4, 0, 8)])
def test_pack_latent_tiles_equals_pack_latent_on_the_crops(Cx, Cc, c_pad):
    from dynamicrafter_amd import ops
    B, long_shape, box_shape, S = 2, (4, 24, 32), (4, 16, 16), 3
    TL, HL, WL = long_shape
    T, h, w = box_shape
    plan = _plan(long_shape, box_shape, (1, 8, 8), shift=(0, 3, 5), S=S)      # step 1: y starts 0, 3, 8; x starts 0, 5, 13, 16
    W = plan["W"]
    assert [0, 3, 5] in plan["host_box"][1].tolist() and [0, 8, 16] in plan["host_box"][1].tolist()
    # starts outside their range, which the host check refuses: the kernel clamps them to both ends
    wild = np.array([[[-2, -1, -7], [5, 30, 40], [0, 3, 5], [0, 9, 17]]], dtype=np.int32)
    clamped = np.array([[0, 0, 0], [0, 8, 16], [0, 3, 5], [0, 8, 16]])
    raw = _raw_plan(wild, np.ones((1, 4, T + h + w), dtype=np.float32), long_shape, box_shape)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B, Cx, TL, HL, WL, generator=gen).to(DEV)
    cc = torch.randn(B, Cc, TL, HL, WL, generator=gen).to(DEV) if Cc else None
    counter = torch.tensor([1], dtype=torch.int32, device=DEV)
    cases = [(plan, plan["host_box"][1], dict(step_index=counter, index=2), w0, n_w, nrep)
             for w0, n_w, nrep in ((0, W, 1), (1, W - 1, 1), (2, 1, 2), (0, 2, 1))]
    cases += [(plan, plan["host_box"][0], dict(index=0), 0, W, 1), (raw, clamped, dict(index=0), 0, 4, 1),
              (raw, clamped, dict(index=0), 1, 2, 2)]
    for pl, starts, sel, w0, n_w, nrep in cases:
        st = [tuple(int(v) for v in s) for s in starts[w0:w0 + n_w]]
        crop = lambda t: torch.stack([t[b, :, t0:t0 + T, y0:y0 + h, x0:x0 + w] for b in range(B)
                                      for t0, y0, x0 in st]).contiguous()
        M = B * n_w * T * h * w
        ref = torch.full((nrep * M, c_pad), 7.0, dtype=torch.bfloat16, device=DEV)
        ops.pack_latent(crop(x), None if cc is None else crop(cc), ref, B=B * n_w, Cx=Cx, Cc=Cc, T=T, HW=h * w, nrep=nrep)
        out = torch.full((nrep * M + 3, c_pad), 7.0, dtype=torch.bfloat16, device=DEV)
        ops.pack_latent_tiles(x, cc, out, pl, B=B, Cx=Cx, Cc=Cc, w0=w0, n_w=n_w, nrep=nrep, **sel)
        torch.cuda.synchronize()
        assert torch.equal(out[:nrep * M].view(torch.int16), ref.view(torch.int16)), (w0, n_w, nrep)
        assert bool((out[nrep * M:] == 7.0).all())                # nothing past the last row
        if Cx + Cc < c_pad:
            assert not out[:nrep * M, Cx + Cc:].any()             # pad channels are zero
    # a counter outside the tables launches nothing
    out = torch.full((B * W * T * h * w, c_pad), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.pack_latent_tiles(x, cc, out, plan, B=B, Cx=Cx, Cc=Cc, step_index=torch.tensor([S], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError):
        ops.pack_latent_tiles(x, cc, out, plan, B=B, Cx=Cx, Cc=Cc, w0=W - 1, n_w=2)
    with pytest.raises(ValueError):
        ops.pack_latent_tiles(x, cc, out[:5], plan, B=B, Cx=Cx, Cc=Cc)
    with pytest.raises(ValueError):
        ops.pack_latent_tiles(x, cc, out, plan, B=B, Cx=Cx, Cc=Cc, index=S)


# ------------------------------------------------------------------ 2. dc_tile_merge
@pytest.mark.parametrize("C,ld_e,ld_out", [(4, 4, 4), (4, 8, 4), (4, 8, 8), (3, 5, 3)])
@pytest.mark.parametrize("nb", [1, 2, 3])
def test_tile_merge_vs_restatement(nb, C, ld_e, ld_out):
    from dynamicrafter_amd import ops
    B, long_shape, box_shape, S = 2, (3, 12, 20), (2, 8, 8), 3
    plan = _plan(long_shape, box_shape, (1, 4, 4), "triangle", shift=(0, 1, 3), S=S, multiple_of=2)
    W = plan["W"]
    T, h, w = box_shape
    n_long = int(np.prod(long_shape))
    assert W % 2 == 0 and W >= 12
    gen = torch.Generator().manual_seed(5 + nb)
    e = torch.randn(nb * B * W * T * h * w, ld_e, generator=gen).to(DEV)
    e[:, C:] = float("nan")                                       # columns past C are not the kernel's to read
    counter = torch.tensor([1], dtype=torch.int32, device=DEV)
    worst, differ = 0, 0
    for step, sel in ((1, dict(step_index=counter)), (0, dict(index=0)), (2, dict(index=2))):
        n_rows = nb * B * n_long
        out = torch.full((n_rows + 2, ld_out), 7.0, device=DEV)
        ops.tile_merge(e, out, plan, nb=nb, B=B, C=C, **sel)
        e5 = e.reshape(nb, B, W, T * h * w, ld_e)
        for n_w in (1, 2):                                        # chunked: e rows of a chunk are [(k, b, w in chunk, ...)]
            chunked = torch.full_like(out, 7.0)
            for w0 in range(0, W, n_w):
                ops.tile_merge(e5[:, :, w0:w0 + n_w].reshape(-1, ld_e).contiguous(), chunked, plan, nb=nb, B=B, C=C, w0=w0,
                               n_w=n_w, accumulate=w0 > 0, **sel)
            torch.cuda.synchronize()
            assert torch.equal(out, chunked), (step, n_w)         # ascending boxes either way: the same roundings
        assert bool((out[n_rows:] == 7.0).all()) and bool((out[:n_rows, C:] == 7.0).all())
        ref, exact = R.merge_rows(e, plan["host_box"][step], plan["host_g"][step], nb=nb, B=B, long_shape=long_shape,
                                  box_shape=box_shape, C=C)
        got = out[:n_rows, :C].cpu().numpy().reshape(ref.shape)
        assert np.isfinite(got).all()
        d = R.ulp_distance(got, ref.astype(np.float32))
        worst, differ = max(worst, int(d.max())), differ + int((d != 0).sum())
        assert d.max() <= 1, (step, int(d.max()))
        assert np.abs(got - exact).max() <= np.abs(ref - exact).max() + 2.0 ** -23 * np.abs(exact).max()
    print(f"\n[tile merge nb={nb} C={C} ld_e={ld_e}] W {W}: worst distance to the per-term-rounded restatement {worst} ulp, "
          f"{differ} elements differ")


def test_tile_merge_never_reads_a_padding_box():
    """A box of weight 0 (padding) is skipped: whatever the UNet wrote for it, infinities and NaN included, does not
    reach the blend, chunked or not."""
    from dynamicrafter_amd import ops
    nb, B, long_shape, box_shape = 2, 1, (2, 8, 20), (2, 8, 8)
    plan = _plan(long_shape, box_shape, (1, 4, 4), "triangle", shift=(0, 0, 3), S=2, multiple_of=2)
    W = plan["W"]
    pad = [k for k in range(W) if not plan["host_g"][0, k].any()]
    assert pad and pad[-1] == W - 1
    M = 2 * 8 * 8
    e = torch.randn(nb, B, W, M, 4, generator=torch.Generator().manual_seed(9)).to(DEV)
    clean = e.clone()
    e[:, :, pad] = float("nan")
    e[0, 0, pad[0], 0, 0] = float("inf")
    outs = []
    for src in (e, clean):
        out = torch.empty(nb * B * int(np.prod(long_shape)), 4, device=DEV)
        ops.tile_merge(src.reshape(-1, 4), out, plan, nb=nb, B=B, C=4, index=0)
        outs.append(out)
    chunked = torch.empty_like(outs[0])
    for w0 in range(0, W, 2):
        ops.tile_merge(e[:, :, w0:w0 + 2].reshape(-1, 4).contiguous(), chunked, plan, nb=nb, B=B, C=4, w0=w0, n_w=2,
                       accumulate=w0 > 0, index=0)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(chunked, outs[0])


def test_tile_merge_single_box_of_weight_one_is_the_identity():
    from dynamicrafter_amd import ops
    nb, B, shape = 2, 2, (2, 8, 12)
    plan = _plan(shape, shape, (1, 4, 4), "triangle", shift=(1, 1, 1), S=2)
    assert plan["W"] == 1 and bool((plan["g"] == 1.0).all())
    for C in (4, 3):
        e = torch.randn(nb * B * int(np.prod(shape)), C, generator=torch.Generator().manual_seed(8)).to(DEV)
        e[3, 1] = -0.0
        out = torch.empty_like(e)
        ops.tile_merge(e, out, plan, nb=nb, B=B, C=C, index=1)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), e.view(torch.int32))      # the sign of zero too


# ------------------------------------------------------------------ the tiny model of the existing GPU tests
@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


def _inputs(S, seed=9, b=1, t=4, h=16, w=16, T=4):
    g = torch.Generator().manual_seed(seed)
    return dict(x_T=torch.randn(b, 4, t, h, w, generator=g),
                ctx=[torch.randn(b, 77 + 16 * T, 128, generator=g) for _ in range(3)],
                cc=torch.randn(b, 4, t, h, w, generator=g) * 0.2,
                noises=torch.randn(S, b, 4, t, h, w, generator=g),
                q_noises=torch.randn(S, b, 4, t, h, w, generator=g),
                x0=torch.randn(b, 4, t, h, w, generator=g),
                fs=torch.tensor([24] * b))


def _sample(model, inp, S, solver="ddim", nb=2, use_graph=False, mask=None, log_every_t=100, **kw):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    mk = lambda c: {"c_crossattn": [c.to(DEV)], "c_concat": [inp["cc"].to(DEV)]}
    kw = dict(kw)
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


TILES = dict(size=(16, 16), stride=(8, 8), shift=(0, 1))


# ------------------------------------------------------------------ 3. one tile == the plain call
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nb", [2, 3])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m", "dpmpp_2m_sde"])
def test_one_tile_equals_the_plain_call(tiny, solver, nb, masked, use_graph):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import TiledRun, WindowedRun
    model = tiny[0]
    S = 4
    inp = _inputs(S, seed=17)
    mask = None
    if masked:
        mask = torch.zeros(1, 1, 4, 16, 16)
        mask[:, :, 0] = 1.0
    plain, pi, sp = _sample(model, inp, S, solver, nb, use_graph, mask, log_every_t=1)
    one, ti, st = _sample(model, inp, S, solver, nb, use_graph, mask, log_every_t=1, tiles=dict(size=(16, 16)))
    assert isinstance(st._last_run, TiledRun) and not isinstance(sp._last_run, (TiledRun, WindowedRun))
    assert st._last_run.plan["W"] == 1 and (st._last_run.graph is not None) == use_graph
    assert torch.isfinite(plain).all()
    assert torch.equal(one, plain)
    for k in ("x_inter", "pred_x0"):
        assert len(ti[k]) == len(pi[k]) == S + 1
        for a, b in zip(ti[k], pi[k]):
            assert torch.equal(a, b), k


# ------------------------------------------------------------------ 4. fused against generic
@pytest.mark.parametrize("nb", [2, 3])
def test_tiled_fused_vs_generic(tiny, nb):
    """The tiled fused path (batched boxes, dc_tile_merge) against the tiled generic path (one apply_model per box and
    branch, torch blend through float64 in the kernel's order) on a 24 x 32 latent, boxes of 16 x 16 at stride 8 with the x
    seams moving by 1 per step. The tolerance is twice what the untiled fused / generic pair of the same size differs by.
    Measured on MI355X, for 2 and for 3 branches alike: untiled pair 0 (bitwise equal at this size), tiled pair 0
    (DESIGN 4.16)."""
    model = tiny[0]
    S = 4
    inp = _inputs(S, h=24, w=32)
    base = R.rel_l2(_sample(model, inp, S, nb=nb)[0], _sample(_Generic(model), inp, S, nb=nb)[0])
    fused, _, sf = _sample(model, inp, S, nb=nb, tiles=TILES)
    generic, _, sg = _sample(_Generic(model), inp, S, nb=nb, tiles=TILES)
    assert hasattr(sf, "_last_run") and not hasattr(sg, "_last_run")
    W = sf._last_run.plan["W"]
    assert W == 8 and sf._last_run.t_table.shape[1] == nb * W     # 2 x 4 boxes once the x seams have moved, one UNet call
    r = R.rel_l2(fused, generic)
    print(f"\n[tiled fused vs generic, {nb} branches] untiled pair rel-L2 {base:.3e}, tiled pair {r:.3e} "
          f"(allowed {2 * base:.3e})")
    assert torch.isfinite(fused).all() and torch.isfinite(generic).all()
    assert r <= 2 * base


# ------------------------------------------------------------------ 5. trajectory against the oracle
def test_tiled_trajectory_vs_oracle(tiny):
    """4 DDIM eta = 1 steps of a 4 x 24 x 32 latent through boxes of 16 x 16 (stride 8, triangle weights, x shift 1; v-param,
    ZTSNR, dynamic rescale, CFG 7.5, guidance rescale 0.7, injected noises): the fused path against the restatement
    driving oracle.unet.unet_forward per box on the CPU and blending in float64. Bound: TRAJ_TOL = 8.5e-2, the project's
    multi-step bound for this model. Measured on MI355X: rel-L2 4.785e-2."""
    from oracle import ddim as oddim
    from oracle import unet as ounet
    model, sd, ocfg = tiny
    S, box_shape, long_shape = 4, (4, 16, 16), (4, 24, 32)
    inp = _inputs(S, h=24, w=32)
    out, _, s = _sample(model, inp, S, tiles=TILES)
    steps = R.plan(long_shape, box_shape, (1, 8, 8), "triangle", (0, 0, 1), S)
    assert s._last_run.plan["W"] == max(len(b) for b in steps) == 8
    state = {"i": 0}

    def apply_model(x, tl, c, fs=None):
        def one(xb, start):
            t0, y0, x0 = start
            ccb = inp["cc"][:, :, t0:t0 + 4, y0:y0 + 16, x0:x0 + 16]
            return ounet.unet_forward(sd, ocfg, torch.cat([xb, ccb], 1), tl, c, fs)
        return R.tiled_model(one, steps, box_shape)(x, state["i"])

    ms = oddim.ModelSchedule(rescale_betas_zero_snr=True, parameterization="v", use_dynamic_rescale=True, base_scale=0.7)
    sc = oddim.DDIMSchedule(ms, S, "uniform_trailing", 1.0)
    ref = oddim.ddim_sample(apply_model, sc, inp["x_T"].double(), inp["ctx"][0], inp["ctx"][1], cfg_scale=7.5,
                            guidance_rescale=0.7, noises=list(inp["noises"].double()), fs=inp["fs"],
                            trace=lambda i, x, p: state.update(i=i + 1))
    r = R.rel_l2(out, ref)
    print(f"\n[tiled trajectory] 4 DDIM steps, 24x32 / box 16x16 / stride 8 / x shift 1, vs oracle rel-L2 {r:.3e} "
          f"(bound {TRAJ_TOL})")
    assert torch.isfinite(out).all()
    assert r < TRAJ_TOL


# ------------------------------------------------------------------ 6. graph == eager, chunked, with rewind
@pytest.mark.parametrize("per_call", [1, 2])
def test_graph_equals_eager_and_rewind_with_chunks_and_mask(tiny, per_call):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler, FusedRun, tiled
    model = tiny[0]
    S = 4
    a, b = _inputs(S, seed=41, h=24, w=32), _inputs(S, seed=42, h=24, w=32)
    mask = torch.zeros(1, 1, 4, 24, 32)
    mask[:, :, 0] = 1.0
    tile = dict(T=4, h=16, w=16, stride=(1, 8, 8), weights="triangle", shift=(0, 0, 1), per_call=per_call)
    s = DDIMSampler(model)
    s.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    mk = lambda c: {"c_crossattn": [c.to(DEV)], "c_concat": [a["cc"].to(DEV)]}
    br = [mk(a["ctx"][0]), mk(a["ctx"][1])]

    def fresh(x_T, graph):
        run = tiled(FusedRun)(s, x_T.to(DEV).clone(), br, tile=tile, fs=a["fs"].to(DEV), noises=a["noises"].to(DEV),
                              cfg_scale=7.5, guidance_rescale=0.7, mask=mask.to(DEV), x0=a["x0"].to(DEV),
                              q_noises=a["q_noises"].to(DEV))
        if graph:
            run.capture()
        for _ in range(S):
            run.step()
        run.sync()
        return run, run.img.clone()

    run, first = fresh(a["x_T"], True)
    assert run.plan["W"] == 8 and run.prep["tile"]["n_w"] == per_call and run.graph is not None
    run.rewind(b["x_T"].to(DEV))
    for _ in range(S):
        run.step()
    run.sync()
    second = run.img.clone()
    with pytest.raises(RuntimeError, match="rewind"):
        run.step()
    run.rewind(a["x_T"].to(DEV))
    for _ in range(S):
        run.step()
    run.sync()
    assert torch.equal(run.img, first)                            # rewind reproduces the run
    _, eager_a = fresh(a["x_T"], False)
    _, eager_b = fresh(b["x_T"], False)
    assert torch.isfinite(first).all() and not torch.equal(first, second)
    assert torch.equal(first, eager_a) and torch.equal(second, eager_b)


# ------------------------------------------------------------------ 7. composition with temporal windows
@pytest.mark.parametrize("nb", [2, 3])
def test_tiles_with_window_stride_fused_vs_generic(tiny, nb):
    """Latent 8 x 16 x 24, boxes 4 x 16 x 16: `window_stride=2` beside `tiles` builds the product plan with a tiled time
    axis. Fused against generic as for the spatial tiles."""
    from dynamicrafter_amd.lvdm.models.samplers.ddim import TiledRun
    model = tiny[0]
    S = 4
    inp = _inputs(S, t=8, h=16, w=24)
    kw = dict(window_stride=2, window_shift=1, tiles=dict(size=(16, 16), stride=(8, 8)))
    short = {k: (v[:, :, :4].contiguous() if k in ("x_T", "cc", "x0") else v[:, :, :, :4].contiguous()
                 if k in ("noises", "q_noises") else v) for k, v in inp.items()}
    base = R.rel_l2(_sample(model, short, S, nb=nb)[0], _sample(_Generic(model), short, S, nb=nb)[0])
    fused, _, sf = _sample(model, inp, S, nb=nb, **kw)
    generic, _, _ = _sample(_Generic(model), inp, S, nb=nb, **kw)
    assert isinstance(sf._last_run, TiledRun) and sf._last_run.plan["box_shape"] == (4, 16, 16)
    assert sf._last_run.plan["W"] == 8                            # 4 windows in time x 2 boxes along x
    r = R.rel_l2(fused, generic)
    print(f"\n[tiles + windows fused vs generic, {nb} branches] untiled 4-frame pair rel-L2 {base:.3e}, tiled pair {r:.3e} "
          f"(allowed {2 * base:.3e})")
    assert torch.isfinite(fused).all()
    assert r <= 2 * base


def test_tiles_with_degenerate_space_equal_the_windowed_path(tiny):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import TiledRun, WindowedRun
    model = tiny[0]
    S = 4
    inp = _inputs(S, t=8)
    mask = torch.zeros(1, 1, 8, 16, 16)
    mask[:, :, 0] = 1.0
    win = dict(window_stride=2, window_weights="triangle", window_shift=1)
    a, _, sa = _sample(model, inp, S, mask=mask, **win)
    b, _, sb = _sample(model, inp, S, mask=mask, tiles=dict(size=(16, 16)), **win)
    assert isinstance(sa._last_run, WindowedRun) and isinstance(sb._last_run, TiledRun)
    assert sb._last_run.plan["W"] == sa._last_run.plan["W"] == 4
    assert torch.isfinite(a).all() and torch.equal(a, b)


# ------------------------------------------------------------------ 8. the harness
@pytest.mark.parametrize("interp", [False, True])
def test_image_guided_synthesis_tiles(interp):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler, TiledRun
    from dynamicrafter_amd.scripts.evaluation.inference import build_conditioning, image_guided_synthesis
    model = _tiny_model(toy_conditioners=True)[0]
    g = torch.Generator().manual_seed(5)
    b, t, H, W, S = 1, 4, 192, 256, 4
    if interp:                                                    # a first and a last frame
        ends = torch.rand(b, 3, 2, H, W, generator=g) * 2 - 1
        videos = torch.cat([ends[:, :, :1].repeat(1, 1, t // 2, 1, 1), ends[:, :, 1:].repeat(1, 1, t // 2, 1, 1)], 2).to(DEV)
    else:
        videos = (torch.rand(b, 3, 1, H, W, generator=g) * 2 - 1).repeat(1, 1, t, 1, 1).to(DEV)
    shape = [b, 4, t, H // 8, W // 8]
    x_T = torch.randn(*shape, generator=g).to(DEV)
    noises = torch.randn(S, *shape, generator=g).to(DEV)
    kw = dict(ddim_steps=S, ddim_eta=1.0, unconditional_guidance_scale=7.5, cfg_img=None, fs=24,
              timestep_spacing="uniform_trailing", guidance_rescale=0.7)
    seen = []
    decode = model.decode_first_stage
    model.decode_first_stage = lambda z, **k: (seen.append(z.clone()), decode(z, **k))[1]
    try:
        torch.manual_seed(0)                              # the posterior draw of the first-stage encode
        clip = image_guided_synthesis(model, ["a corgi"], videos, shape, n_samples=1, interp=interp, x_T=x_T, noises=noises,
                                      tiles=dict(TILES), **kw)
    finally:
        del model.decode_first_stage
    assert tuple(clip.shape) == (b, 1, 3, t, H, W)
    assert torch.isfinite(clip).all() and float(clip.std()) > 1e-3
    # the sampler by hand on the same inputs
    torch.manual_seed(0)
    cond, uc, _ = build_conditioning(model, [""], videos, 7.5, None, False, interp, None)     # text_input=False: no prompt
    assert tuple(cond["c_concat"][0].shape) == tuple(shape)
    if interp:
        assert not cond["c_concat"][0][:, :, 1:-1].any() and cond["c_concat"][0][:, :, -1].any()
    s = DDIMSampler(model)
    by_hand, _ = s.sample(S=S, conditioning=cond, batch_size=b, shape=shape[1:], verbose=False,
                          unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=1.0, cfg_img=None,
                          fs=torch.tensor([24], device=DEV), timestep_spacing="uniform_trailing", guidance_rescale=0.7,
                          x_T=x_T, noises=noises, tiles=dict(TILES))
    assert isinstance(s._last_run, TiledRun) and s._last_run.plan["W"] == 8
    assert len(seen) == 1 and torch.equal(seen[0], by_hand)
    if not interp:
        with pytest.raises(ValueError, match="window_stride = 2 cannot be combined with loop"):
            image_guided_synthesis(model, ["a corgi"], videos, shape, loop=True, window_stride=2, tiles=dict(TILES), **kw)
        with pytest.raises(ValueError, match="not one the UNet takes"):
            image_guided_synthesis(model, ["a corgi"], videos, shape, x_T=x_T, noises=noises, tiles=dict(size=(12, 16)), **kw)
        with pytest.raises(ValueError, match="partial run"):
            s.decode(x_T, cond, 2, tiles=dict(TILES))


# ------------------------------------------------------------------ 9. the scratch bound
def test_scratch_bound_covers_the_arena_after_a_tiled_run(tiny):
    """max_row_width / max_context_row_width (what the default boxes per call is computed from) against the buffers the
    arena really holds after tiled runs of the tiny model: none is larger than the bound says for the box's size."""
    model = tiny[0]
    net = model.model.diffusion_model
    inp = _inputs(2, h=24, w=32)
    _, _, s = _sample(model, inp, 2, nb=3, tiles=TILES)
    W = s._last_run.plan["W"]
    clips, T, HW = 3 * W, 4, 16 * 16
    assert s._last_run.prep["tile"]["n_w"] == W <= model.max_windows_per_call(tuple(inp["x_T"].shape), 3, 4, hw=(16, 16))
    bound = max(clips * T * HW * net.max_row_width(), clips * T * 93 * net.max_context_row_width())
    sizes = {key[0]: key[1] * key[2] for key in net._arena._bufs}
    tag = max(sizes, key=sizes.get)
    print(f"\n[scratch bound] largest arena buffer {tag}: {sizes[tag]} elements, bound {bound:.0f}")
    assert sizes[tag] <= bound
    with pytest.raises(ValueError, match="windows_per_call"):
        _sample(model, inp, 2, tiles=dict(TILES, per_call=0))
