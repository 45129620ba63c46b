"""The exact-fit GEMM (csrc/gemm_fit.hip, ops.gemm_fit): 288 x 320 tiles, one workgroup per CU, whole rounds only.

  * bit for bit against a float64 reference on integer data (the method of tests/exact_cases.py): operands and outputs are
    windows of NaN-filled buffers (lda > K, ldc > N, ldr > N); M is one round of tiles over the device's CUs (two for one
    case); N in {320, 640}; K = 64 (shorter than the ring of 4 K tiles of 32), 128 (the ring), 192 (the ring wraps and is
    left partly filled), 1280 (long); epilogues none / bias / residual / bias + residual / in place (out is the residual) /
    "round" (a wide integer bias puts the fp32 value between bf16 values: truncation or a second rounding changes bits).
    The kernel adds bias and residual in fp32 and rounds once; on the bf16-exact flavours every order gives the same bits.
  * against ops.gemm on randn data at a level-2 shape, bounded by what two existing kernels of dc_gemm_conv measure against
    each other at that shape (measured here, printed).
  * without a GPU: the argument checks of dc_gemm_fit, ops.gemm_fits, the exported symbols.
  * model level: a one-level UNet of width 1280 whose rows are one round; the exact-fit route on against off, and hipGraph
    replay against eager with the new kernel in the graph."""
import ctypes as C

import pytest
import torch

from tests import exact_cases as X

DEV = "cuda:0"
gpu = pytest.mark.gpu


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def ops():
    from dynamicrafter_amd import ops as _ops
    return _ops


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- exact ---------------------------------------------------------------------------------------------------------------
EPIS = {      # bias, wide bias, residual, in place
    "none": (False, False, False, False),
    "bias": (True, False, False, False),
    "res": (False, False, True, False),
    "bias_res": (True, False, True, False),
    "inplace": (True, False, True, True),
    "round": (True, True, False, False),
}
EXACT = [(N, K, 1) for N in (320, 640) for K in (64, 128, 192, 1280)] + [(640, 192, 2)]


@gpu
@pytest.mark.parametrize("N,K,rounds", EXACT, ids=[f"N{n}-K{k}-r{r}" for n, k, r in EXACT])
def test_fit_exact(ops, N, K, rounds):
    cus = _cus()
    tiles_n = N // 320
    assert cus % tiles_n == 0
    M = 288 * (cus // tiles_n) * rounds
    gen = torch.Generator(device=DEV).manual_seed(4000 + N * 7 + K + rounds)
    p = X.density(K)
    x, w = X.ternary((M, K), p, gen), X.ternary((N, K), p, gen)
    acc = x.double() @ w.double().t()
    _, a = X.poisoned(M, K, X.BF16, DEV, fill=x)
    assert a.stride(0) > K
    for epi, (has_bias, wide, has_res, inplace) in EPIS.items():
        what = f"gemm_fit [{M} x {N} x {K}] {epi}"
        assert ops.gemm_fits(M, ops.PackedWeight.linear(w, None, DEV)), what
        bias = X.integers((N,), *((-2000, 2000) if wide else (-8, 8)), gen) if has_bias else None
        res = X.integers((M, N), -8, 8, gen) if has_res else None
        v = acc if bias is None else acc + bias.double()
        if wide:          # an exact fp32 integer, rounded to nearest even once
            assert v.abs().max().item() < 2 ** 24 and torch.equal(v.round(), v)
            ref = v.float().to(X.BF16).double()
            assert not torch.equal(ref, v), what + ": the wide bias left nothing to round"
        else:
            ref = v if res is None else v + res.double()
            X.assert_bf16_exact_points([v, ref], what)
        pw = ops.PackedWeight.linear(w, bias, DEV)
        outs = []
        for _ in range(2):
            if inplace:
                buf, out = X.poisoned(M, N, X.BF16, DEV, fill=res)
                ops.gemm_fit(a, pw, out, residual=out)
            else:
                buf, out = X.poisoned(M, N, X.BF16, DEV)
                r = None if res is None else X.poisoned(M, N, X.BF16, DEV, fill=res)[1]
                ops.gemm_fit(a, pw, out, residual=r)
                assert out.stride(0) > N and (r is None or r.stride(0) > N)
            outs.append((buf, out))
        torch.cuda.synchronize()
        ops._hip.check_error_word(what)
        X.assert_exact(outs[0][1], ref, 288, 320, what)
        X.assert_margins_nan(outs[0][0], M, N, what)
        assert torch.equal(outs[0][1], outs[1][1]), f"{what}: two launches differ"
        X.assert_margins_nan(outs[1][0], M, N, what + " (second launch)")


# ---- against ops.gemm ------------------------------------------------------------------------------------------------------
PLAN_NO_PIPE_PLAIN = 17     # the default plan 19 without bit 1: plain launches leave the one-wave kernel


@pytest.fixture(scope="module")
def level2(ops):
    """[72 CUs x 1280 x 2560] on randn data (the level-2 ResBlock skip of the up path; 18432 rows on 256 CUs): ops.gemm under
    the default plan (the one-wave kernel), under plan 17 (the 128-row persistent kernel), and the exact-fit kernel.
    The bound of this file is the rel-L2 of the first two against each other."""
    lib = ops._hip.lib()
    M, N, K = 72 * _cus(), 1280, 2560
    gen = torch.Generator(device=DEV).manual_seed(77)
    a = torch.randn((M, K), generator=gen, device=DEV).to(X.BF16)
    w = torch.randn((N, K), generator=gen, device=DEV) * K ** -0.5
    bias = torch.randn((N,), generator=gen, device=DEV)
    pw = ops.PackedWeight.linear(w, bias, DEV)
    got, names = {}, {}
    for tag, plan in (("default", X.PLAN_DEFAULT), ("plan17", PLAN_NO_PIPE_PLAIN)):
        prev = lib.dc_gemm_set_plan(plan)
        assert prev >= 0
        try:
            got[tag] = ops.gemm(a, pw, torch.empty((M, N), dtype=X.BF16, device=DEV))
            names[tag] = lib.dc_gemm_last_variant().decode()
        finally:
            lib.dc_gemm_set_plan(prev)
    got["fit"] = ops.gemm_fit(a, pw, torch.empty((M, N), dtype=X.BF16, device=DEV))
    torch.cuda.synchronize()
    ops._hip.check_error_word("level2")
    return dict(M=M, got=got, names=names, bound=rel_l2(got["plan17"], got["default"]))


@gpu
def test_fit_vs_gemm_randn(ops, level2):
    g, names = level2["got"], level2["names"]
    assert names["default"] != names["plan17"], names
    r_fit, r_fit17 = rel_l2(g["fit"], g["default"]), rel_l2(g["fit"], g["plan17"])
    print(f"\n[{level2['M']} x 1280 x 2560 randn] {names['plan17']} vs {names['default']}: rel-L2 {level2['bound']:.3e} (the bound); "
          f"gemm_fit vs ops.gemm ({names['default']}): {r_fit:.3e}; gemm_fit vs {names['plan17']}: {r_fit17:.3e}")
    assert level2["bound"] > 0
    assert r_fit <= level2["bound"]


ROUTED = [(1280, 1280, False), (1280, 1280, True), (3840, 1280, False)]


@gpu
@pytest.mark.parametrize("N,K,has_res", ROUTED, ids=[f"N{n}-K{k}{'-res' if r else ''}" for n, k, r in ROUTED])
def test_fit_returns_the_bits_of_the_kernel_it_replaces(ops, N, K, has_res):
    """The route list of the UNet (openaimodel3d._FIT_ROUTES) rests on this: at the routed shapes, [72 CUs x 1280 x 1280] with
    and without a residual (also in place) and [72 CUs x 3840 x 1280], the exact-fit kernel equals ops.gemm bit for bit on randn
    data, where sums fall between bf16 values and a second rounding or another order of the adds changes bits."""
    from dynamicrafter_amd.lvdm.modules.networks import openaimodel3d as U
    assert (N, K) in U._FIT_ROUTES
    M = 72 * _cus()
    gen = torch.Generator(device=DEV).manual_seed(100 + N + K + has_res)
    a = torch.randn((M, K), generator=gen, device=DEV).to(X.BF16)
    pw = ops.PackedWeight.linear(torch.randn((N, K), generator=gen, device=DEV) * K ** -0.5, torch.randn((N,), generator=gen, device=DEV), DEV)
    res = torch.randn((M, N), generator=gen, device=DEV).to(X.BF16) if has_res else None
    assert ops.gemm_fits(M, pw)
    old = ops.gemm(a, pw, torch.empty((M, N), dtype=X.BF16, device=DEV), residual=res)
    name = ops._hip.lib().dc_gemm_last_variant().decode()
    fit = ops.gemm_fit(a, pw, torch.empty((M, N), dtype=X.BF16, device=DEV), residual=res)
    differ = (fit != old).sum().item()
    print(f"\n[{M} x {N} x {K}{' + residual' if has_res else ''}] gemm_fit vs {name}: {differ} of {M * N} elements differ")
    assert differ == 0 and torch.equal(fit, old)
    if has_res:
        inplace = res.clone()
        ops.gemm_fit(a, pw, inplace, residual=inplace)
        assert torch.equal(inplace, old), "in place"
    torch.cuda.synchronize()
    ops._hip.check_error_word("routed shapes")


# ---- without a GPU ---------------------------------------------------------------------------------------------------------
def _params(lib_mod, **kw):
    p = lib_mod.DcGemmParams()
    p.A = p.W = p.C = 4096                      # never dereferenced: every case below is refused before a launch
    p.M, p.N, p.K, p.n_pad = 288 * 64, 1280, 1280, 1280
    p.lda, p.ldc = 1280, 1280
    p.mode, p.flags, p.alpha = 0, 0, 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_fit_refuses_without_launch():
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    bad = dict(m_not_288=dict(M=288 * 64 + 16), n_not_320=dict(N=1024, n_pad=1024), tiles_not_cus=dict(M=288 * 3, N=320, n_pad=384),
               geglu=dict(flags=_hip.DC_GEMM_GEGLU), f32=dict(flags=_hip.DC_GEMM_OUT_F32), mode=dict(mode=1),
               gelu=dict(flags=_hip.DC_GEMM_GELU), k_not_64=dict(K=1248), alpha=dict(alpha=0.5))
    for name, kw in bad.items():
        p = _params(_hip, **kw)
        code = lib.dc_gemm_fit(C.byref(p), None)
        assert code in (-1, -2), f"{name}: dc_gemm_fit returned {code}"
    assert lib.dc_gemm_fit(None, None) == -2
    # the shape query agrees: the refused shapes do not fit (a tile count of 3 is no multiple of any device's CU count;
    # without a device nothing fits)
    for M, N, K in ((288 * 64 + 16, 1280, 1280), (288 * 64, 1024, 1280), (288 * 3, 320, 1280), (288 * 64, 1280, 1248)):
        assert lib.dc_gemm_fit_shape(M, N, K) == 0


def test_gemm_fits_agrees_with_the_entry(ops):
    from dynamicrafter_amd import _hip
    lib = _hip.lib()

    class PW:                                   # the two fields gemm_fits reads
        def __init__(self, N, K):
            self.N, self.K = N, K

    cus = _cus() if torch.cuda.is_available() else 0
    shapes = [(288 * 64, 1280, 1280), (288 * 64 + 16, 1280, 1280), (288 * 64, 1024, 1280), (288 * 3, 320, 1280), (288 * 64, 1280, 1248)]
    if cus:
        shapes += [(72 * cus, 1280, 1280), (72 * cus, 3840, 1280), (288 * cus, 640, 2560), (288 * cus + 288, 320, 64)]
    for M, N, K in shapes:
        fits = ops.gemm_fits(M, PW(N, K))
        assert fits == bool(lib.dc_gemm_fit_shape(M, N, K))
        p = _params(_hip, M=M, N=N, K=K, n_pad=N, lda=K, ldc=N, A=0)      # A = NULL: a shape that fits stops at DC_ERR_ARG
        code = lib.dc_gemm_fit(C.byref(p), None)
        multiples = M % 288 == 0 and N % 320 == 0 and K % 64 == 0
        # DC_ERR_SHAPE for a shape that does not fit; DC_ERR_ARG for the null operand behind a shape that fits, or for "no device"
        assert code == (-2 if multiples and (fits or not cus) else -1), (M, N, K, fits, code)
        if cus:
            want = M % 288 == 0 and N % 320 == 0 and K % 64 == 0 and ((M // 288) * (N // 320)) % cus == 0
            assert fits == want, (M, N, K)
        else:
            assert not fits


def test_fit_symbols_exported():
    import re
    import subprocess
    from dynamicrafter_amd import _hip
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (dc_[a-z0-9_]+)", nm))
    assert {"dc_gemm_fit", "dc_gemm_fit_shape"} <= exported
    assert {"dc_gemm_fit", "dc_gemm_fit_shape"} <= set(_hip.SIGNATURES)


# ---- model level -----------------------------------------------------------------------------------------------------------
ONE_LEVEL_1280 = dict(in_channels=8, out_channels=4, model_channels=1280, attention_resolutions=[1], num_res_blocks=1,
                      channel_mult=[1], dropout=0.0, num_head_channels=64, transformer_depth=1, context_dim=128,
                      use_linear=True, use_checkpoint=False, temporal_conv=True, temporal_attention=True,
                      temporal_selfatt_only=True, use_relative_position=False, use_causal_attention=False,
                      temporal_length=16, addition_attention=False, image_cross_attention=False, default_fs=10,
                      fs_condition=True)


@gpu
def test_model_fit_on_vs_off_and_graph_replay(ops, level2, monkeypatch):
    """One level of width 1280 on 16 frames of 18 x (CUs / 4) positions: 72 CUs rows, one round of tiles for its proj_in,
    to_q, to_out, proj_out [1280 x 1280] and qkv [3840 x 1280], the routed shapes (measured on MI355X: 48 launches, on vs off
    rel-L2 0.0 - the routed launches return the bits of the kernels they replace. With the ff2 [1280 x 5120] routed as well the
    forward moved by 9.1e-3 against a bound of 9.1e-6, which is why that shape is measured and not routed)."""
    from dynamicrafter_amd.lvdm.modules.networks import openaimodel3d as U
    from oracle.weights import fill_state_dict
    cus = _cus()
    assert cus % 4 == 0
    B, T, H, W = 1, 16, 18, cus // 4
    M = B * T * H * W
    net = U.UNetModel(**ONE_LEVEL_1280)
    sd = net.state_dict()
    net.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in sd.items()}, 21), strict=True)
    net.to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((B, 8, T, H, W), generator=gen, device=DEV)
    ctx = torch.randn((B, 16, 128), generator=gen, device=DEV)
    xr = torch.zeros((M, U.C_IN_PAD), dtype=X.BF16, device=DEV)
    ops.pack_latent(x, None, xr, B=B, Cx=8, Cc=0, T=T, HW=H * W)
    ctx_rows, Lc = net.build_context_rows(ctx, B, T)
    t_table = torch.full((1, B), 500, dtype=torch.int64, device=DEV)
    fs_table = torch.full((B,), 10, dtype=torch.int64, device=DEV)

    def run():
        return net.forward_rows(xr, t_table, ctx_rows, B=B, T=T, H=H, W=W, Lc=Lc, n_text=min(77, Lc), fs_table=fs_table)

    with ops.Tracer() as tr:
        run()
        fams = tr.summary()
    assert fams.get("gemm_fit_kernel", {}).get("launches", 0) >= 6, sorted(fams)
    on = run().clone()
    monkeypatch.setattr(U, "_GEMM_FIT", False)
    with ops.Tracer() as tr:
        run()
        assert "gemm_fit_kernel" not in tr.summary()
    off = run().clone()
    monkeypatch.setattr(U, "_GEMM_FIT", True)
    eager = run().clone()
    assert torch.equal(eager, on)
    held = {}
    graph = ops.DeviceGraph().capture(lambda: held.update(y=run()))
    held["y"].zero_()                                 # the replay itself must write the output
    torch.cuda.synchronize()
    graph.launch()
    graph.sync()
    replay = held["y"].clone()
    torch.cuda.synchronize()
    ops._hip.check_error_word("one-level 1280 model")
    r = rel_l2(on, off)
    print(f"\n[one level of 1280, {M} rows] exact-fit route on vs off: rel-L2 {r:.3e}; bound (level2 fixture) {level2['bound']:.3e}")
    assert torch.isfinite(on).all()
    assert torch.equal(replay, eager), "hipGraph replay differs from eager"
    assert r <= level2["bound"]
