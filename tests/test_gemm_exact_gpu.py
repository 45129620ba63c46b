"""Every kernel variant of dc_gemm_conv, pinned by name and checked bit for bit against a float64 reference on integer data
(tests/exact_cases.py has the method, the table and the derivation of each shape), and the X-stationary kernels of
ff_fused.hip that can be exact: linear_residual, ln_linear without the LayerNorm, gn_linear on hand-made statistics.

For every (table entry, epilogue flavour): the plan is set through dc_gemm_set_plan and restored; dc_gemm_last_variant()
must be the entry's name; the output - a window of a NaN-filled buffer, computed from NaN-padded operands - equals the
reference element for element; the NaN margins are untouched; a second launch into a fresh buffer gives the same bits;
and the library's error word is clear. GEGLU / GELU outputs are bounded per element instead (exact_cases.activation_bound)."""
import os

import pytest
import torch

from tests import exact_cases as X

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

_SWITCHES = sorted(k for k in os.environ if k.startswith("DC_GEMM_") or k == "DC_PIPE_MIN_K")


@pytest.fixture(scope="module")
def ops():
    # the dispatch switches are read once per process: with one of them set, the variant names below mean something else
    assert not _SWITCHES, f"unset {', '.join(_SWITCHES)}: these tests pin the default dispatch of dc_gemm_conv"
    from dynamicrafter_amd import ops as _ops
    return _ops


def _variant(ops):
    return ops._hip.lib().dc_gemm_last_variant().decode()


# operands, packed activation buffer and float64 accumulator of the entry under test: shared by its flavours, one entry at a time
_cache = {}


def _entry(case, dense):
    key = (case["id"], dense)
    if _cache.get("key") != key:
        _cache.clear()
        geo, x, w = X.make_operands(case, dense, DEV)
        acc = X.ref_accumulate(case, geo, x, w)
        a_buf, a = X.poisoned(geo["a_rows"], geo["a_cols"], X.BF16, DEV, fill=x)
        _cache.update(key=key, geo=geo, x=x, w=w, acc=acc, a_buf=a_buf, a=a)
    return _cache


def _pack(ops, case, w, bias):
    pw_cls = ops.PackedWeight
    if case["kind"] == "gemm":
        return pw_cls.linear(w, bias, DEV)
    if case["kind"] == "conv":
        return pw_cls.conv3x3(w, bias, DEV, n_align=4)
    return pw_cls.tconv3(w, bias, DEV)


def _mode_args(case, geo):
    s = geo["shape"]
    if case["kind"] == "conv":
        return dict(conv=dict(IH=s["H"], IW=s["W"], OH=geo["OH"], OW=geo["OW"], stride=s["stride"], pad=s["pad"], ups=s["ups"]))
    if case["kind"] == "tconv":
        return dict(tconv=dict(T=s["T"], HW=s["HW"]))
    return {}


@pytest.mark.parametrize("case,epi", X.case_params(), ids=X.case_ids())
def test_variant_exact(ops, case, epi):
    lib = ops._hip.lib()
    what = f"{case['id']}-{epi} [{case['variant']}]"
    dense = bool(X.EPIS[epi].get("f32"))
    ent = _entry(case, dense)
    geo = ent["geo"]
    M, n_out = geo["M"], (geo["N"] // 2 if case["geglu"] else geo["N"])
    ep = X.make_epilogue(case, epi, geo, DEV)
    ref, points, extra = X.ref_epilogue(case, geo, ent["acc"], ep)
    # preconditions, on the reference alone
    if dense:
        X.assert_fp32_exact_operands(case, geo, ent["x"], ent["w"], what)
    elif extra:
        assert ep["rowvec"] is None and ep["residual"] is None and ep["alpha"] == 1.0
        X.assert_bf16_exact_points([extra["val"] if case["geglu"] else extra["gate"]], what)
    else:
        X.assert_bf16_exact_points(points, what)

    pw = _pack(ops, case, ent["w"], ep["bias"])
    assert pw.N == geo["N"] and pw.K == geo["K"]
    kw = _mode_args(case, geo)
    if ep["rowvec"] is not None:
        G = ep["rowvec"].shape[0]
        rv_buf = torch.full((G + 1, n_out + X.COL_OFF + X.COL_PAD), X.NAN, dtype=torch.float32, device=DEV)
        rv_buf[:G, X.COL_OFF:X.COL_OFF + n_out] = ep["rowvec"]
        kw.update(rowvec=rv_buf[:G, X.COL_OFF:X.COL_OFF + n_out], rows_per_vec=ep["rows_per_vec"])
    if ep["residual"] is not None:
        kw.update(residual=X.poisoned(M, n_out, X.BF16, DEV, fill=ep["residual"])[1])
    odt = torch.float32 if ep["f32"] else X.BF16
    outs = []
    prev = lib.dc_gemm_set_plan(case["plan"])
    assert prev >= 0
    try:
        for _ in range(2):
            buf, out = X.poisoned(M, n_out, odt, DEV)
            ops.gemm(ent["a"], pw, out, geglu=case["geglu"], gelu=ep["gelu"], alpha=ep["alpha"], **kw)
            outs.append((buf, out))
            assert _variant(ops) == case["variant"], f"{what}: dispatched to {_variant(ops)}"
    finally:
        lib.dc_gemm_set_plan(prev)
    torch.cuda.synchronize()
    ops._hip.check_error_word(what)
    tr, tc = X.tile_of(case["variant"])
    if extra:
        want, bound = X.activation_bound(ref, extra)
        X.assert_within(outs[0][1], want, bound, tr, tc, what)
    else:
        X.assert_exact(outs[0][1], ref, tr, tc, what)
    X.assert_margins_nan(outs[0][0], M, n_out, what)
    assert torch.equal(outs[0][1], outs[1][1]), f"{what}: two launches differ"
    X.assert_margins_nan(outs[1][0], M, n_out, what + " (second launch)")


# ---- the X-stationary kernels (ff_fused.hip) -------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", X.XS_SHAPES)
def test_linear_residual_exact(ops, K, N):
    """out = bf16(residual + x @ w.T + bias): one fp32 add, one rounding; ragged last tile; in place; into a column slice."""
    what = f"linear_residual K={K} N={N}"
    x, w, bias, res = X.xs_operands(K, N, DEV)
    ref = x.double() @ w.double().t() + bias.double() + res.double()
    X.assert_bf16_exact_points([ref], what)
    pw = ops.PackedWeight.linear(w, bias, DEV)
    _, a = X.poisoned(X.XS_M, K, X.BF16, DEV, fill=x)
    _, r = X.poisoned(X.XS_M, N, X.BF16, DEV, fill=res)
    buf, out = X.poisoned(X.XS_M, N, X.BF16, DEV)                   # a column slice of a wider buffer
    ops.linear_residual(a, pw, r, out)
    X.assert_exact(out, ref, 128, 32, what)
    X.assert_margins_nan(buf, X.XS_M, N, what)
    buf2, inplace = X.poisoned(X.XS_M, N, X.BF16, DEV, fill=res)    # residual is the output buffer
    ops.linear_residual(a, pw, inplace, inplace)
    X.assert_exact(inplace, ref, 128, 32, what + " in place")
    X.assert_margins_nan(buf2, X.XS_M, N, what + " in place")


@pytest.mark.parametrize("K,N", X.XS_SHAPES)
def test_ln_linear_without_ln_exact(ops, K, N):
    what = f"ln_linear(ln=None) K={K} N={N}"
    x, w, bias, _ = X.xs_operands(K, N, DEV, seed=1)
    for b in (bias, None):
        ref = x.double() @ w.double().t() + (0 if b is None else b.double())
        X.assert_bf16_exact_points([ref], what)
        pw = ops.PackedWeight.linear(w, b, DEV)
        _, a = X.poisoned(X.XS_M, K, X.BF16, DEV, fill=x)
        buf, out = X.poisoned(X.XS_M, N, X.BF16, DEV)
        ops.ln_linear(a, pw, out)
        X.assert_exact(out, ref, 128, 32, what)
        X.assert_margins_nan(buf, X.XS_M, N, what)


@pytest.mark.parametrize("K,N", X.XS_SHAPES)
def test_gn_linear_hand_made_stats_exact(ops, K, N):
    """GroupNorm with statistics made by hand (integer mean, rstd in {1, 2}, gamma in {1, 2}, integer beta): the normalised
    activation is a small integer, so the fused Linear is exact, and a wrong instance or group index changes the bits."""
    what = f"gn_linear K={K} N={N}"
    d = X.gn_operands(K, N, DEV)
    X.assert_bf16_exact_points([d["normed"], d["ref"]], what)
    pw = ops.PackedWeight.linear(d["w"], d["bias"], DEV)
    M = X.GN_INST * X.GN_RPI
    _, a = X.poisoned(M, K, X.BF16, DEV, fill=d["x"])
    buf, out = X.poisoned(M, N, X.BF16, DEV)
    ops.gn_linear(a, d["gamma"], d["beta"], d["stats"], pw, out, groups=X.GN_GROUPS, rows_per_inst=X.GN_RPI)
    X.assert_exact(out, d["ref"], 128, 32, what)
    X.assert_margins_nan(buf, M, N, what)
