"""The census behind tests/test_gemm_exact_gpu.py, without a GPU: every name dc_note_variant can report has an exact case
(or a stated reason why ops.gemm cannot reach it), no table entry names a kernel that is gone, and the integer generators
keep the preconditions that make the comparison bit for bit."""
import os
import re

import pytest
import torch

from tests import exact_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamicrafter_amd", "csrc")
SOURCES = ("gemm_conv.hip", "gemm_conv_glds.hip", "gemm_pp.h")
CAP_ROWS = 1024                 # rows of the large entries that the CPU builds (whole frames / clips: at least one)


def noted_variants():
    """Every string literal inside a dc_note_variant(...) statement of the three sources."""
    names = set()
    for f in SOURCES:
        text = open(os.path.join(CSRC, f)).read()
        text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
        for m in re.finditer(r"\bdc_note_variant\s*\(", text):
            if re.match(r"\s*const\s+char", text[m.end():]):          # the declaration / definition, not a call
                continue
            stmt = text[m.end():text.index(";", m.end())]
            names.update(re.findall(r'"([^"]*)"', stmt))
    return names


def test_every_variant_name_has_an_exact_case():
    noted = noted_variants()
    assert len(noted) >= 30 and "gemm_conv_kernel<128>" in noted and "gemm_pp_kernel<geglu>" in noted, sorted(noted)
    table = {c["variant"] for c in X.VARIANT_CASES}
    assert not (table & set(X.UNREACHABLE)), sorted(table & set(X.UNREACHABLE))
    missing = noted - table - set(X.UNREACHABLE)
    assert not missing, f"dc_note_variant names without a VARIANT_CASES entry or an UNREACHABLE reason: {sorted(missing)}"
    stale = (table | set(X.UNREACHABLE)) - noted
    assert not stale, f"table entries whose name no source reports any more: {sorted(stale)}"
    assert all(isinstance(r, str) and len(r) > 20 for r in X.UNREACHABLE.values())


def test_table_is_well_formed():
    ids = [c["id"] for c in X.VARIANT_CASES]
    assert len(ids) == len(set(ids))
    for c in X.VARIANT_CASES:
        assert c["epis"] and set(c["epis"]) <= set(X.EPIS), c["id"]
        assert 0 <= c["plan"] <= 511 and not c["plan"] & 4, c["id"]
        geo = X.geometry(c)
        tr, tc = X.tile_of(c["variant"])
        assert geo["K"] % 64 == 0 and geo["a_cols"] % 64 == 0, c["id"]
        if not c["variant"].startswith("conv3x3_"):
            assert geo["M"] % tr != 0, f"{c['id']}: M = {geo['M']} leaves no ragged last row tile of {tr}"
        if c["kind"] == "conv" and geo["M"] > 4096:
            # the image width is no multiple of 8 and a row-tile boundary falls inside an image row
            assert geo["OW"] % 8 != 0 and 256 % geo["OW"] != 0, c["id"]
        if c["geglu"]:
            assert set(c["epis"]) <= {"bias", "nobias"}, c["id"]


def test_integers_up_to_256_are_bf16_values():
    v = torch.arange(-256, 257, dtype=torch.float64)
    assert torch.equal(v.float().to(torch.bfloat16).double(), v)
    half = torch.arange(-255, 256, dtype=torch.float64) * 0.5          # alpha = 0.5: half-integers below 128
    assert torch.equal(half.float().to(torch.bfloat16).double(), half)


@pytest.mark.parametrize("case", X.VARIANT_CASES, ids=[c["id"] for c in X.VARIANT_CASES])
def test_generator_preconditions(case):
    """Operands and float64 reference of every entry (rows capped), every flavour: the <= 256 / bf16-exact and < 2^24
    conditions hold, and fp32 arithmetic on these operands reproduces float64 - the premise of the exact comparison."""
    accs = {}
    for epi in case["epis"]:
        dense = bool(X.EPIS[epi].get("f32"))
        if dense not in accs:
            geo, x, w = X.make_operands(case, dense, "cpu", cap_rows=CAP_ROWS)
            accs[dense] = (geo, x, w, X.ref_accumulate(case, geo, x, w))
            if case["kind"] == "gemm":
                assert torch.equal((x @ w.t()).double(), accs[dense][3])      # fp32 matmul == float64 on this data
        geo, x, w, acc = accs[dense]
        what = f"{case['id']}-{epi}"
        ep = X.make_epilogue(case, epi, geo, "cpu")
        ref, points, extra = X.ref_epilogue(case, geo, acc, ep)
        assert ref.shape == (geo["M"], geo["N"] // 2 if case["geglu"] else geo["N"])
        if dense:
            X.assert_fp32_exact_operands(case, geo, x, w, what)
            assert torch.equal(ref.float().double(), ref), what
        elif extra:
            X.assert_bf16_exact_points([extra["val"] if case["geglu"] else extra["gate"]], what)
            want, bound = X.activation_bound(ref, extra)
            near = extra["gate"].abs() <= 4
            assert near.any() and (~near).any(), f"{what}: the gates do not cover both sides of |gate| = 4"
            assert (bound[~near] == 0).all() and (bound[near] >= 0).all()
        else:
            X.assert_bf16_exact_points(points, what)
            assert torch.equal(ref.float().to(torch.bfloat16).double(), ref), what


def test_conv_reference_against_direct_sum():
    """The shifted-matmul conv reference, against the definition written as loops, on the geometries it covers: stride 1
    and 2 with pad 1, the asymmetric pad (0, 1, 0, 1), nearest x2; and the temporal conv."""
    for shape in (X._c(2, 64, 8, 5, 6), X._c(1, 64, 8, 7, 5, stride=2), X._c(1, 64, 8, 6, 8, stride=2, pad=0), X._c(1, 64, 8, 3, 4, ups=1)):
        case = X._case("probe", "gemm_conv_kernel<64>", "conv", shape, ("bias",))
        geo, x, w = X.make_operands(case, True, "cpu")
        acc = X.ref_accumulate(case, geo, x, w)
        s, OH, OW = geo["shape"], geo["OH"], geo["OW"]
        img = x.double().reshape(s["n"], s["H"], s["W"], s["C"])
        H, W = (2 * s["H"], 2 * s["W"]) if s["ups"] else (s["H"], s["W"])
        want = torch.zeros(s["n"], OH, OW, s["Co"], dtype=torch.float64)
        for oy in range(OH):
            for ox in range(OW):
                for dy in range(3):
                    for dx in range(3):
                        iy, ix = oy * s["stride"] - s["pad"] + dy, ox * s["stride"] - s["pad"] + dx
                        if 0 <= iy < H and 0 <= ix < W:
                            src = img[:, iy // 2, ix // 2] if s["ups"] else img[:, iy, ix]
                            want[:, oy, ox] += src @ w[:, :, dy, dx].double().t()
        assert torch.equal(acc, want.reshape(-1, s["Co"])), shape
    case = X._case("probe", "gemm_conv_kernel<64>", "tconv", X._t(2, 4, 3, 64, 8), ("bias",))
    geo, x, w = X.make_operands(case, True, "cpu")
    acc = X.ref_accumulate(case, geo, x, w).reshape(2, 4, 3, 8)
    clip = x.double().reshape(2, 4, 3, 64)
    want = torch.zeros(2, 4, 3, 8, dtype=torch.float64)
    for t in range(4):
        for k in range(3):
            if 0 <= t + k - 1 < 4:
                want[:, t] += clip[:, t + k - 1] @ w[:, :, k, 0, 0].double().t()
    assert torch.equal(acc, want)


def test_mismatch_report_names_the_place():
    ref = torch.zeros(300, 200, dtype=torch.float64)
    out = torch.zeros(300, 200, dtype=torch.bfloat16)
    X.assert_exact(out, ref, 128, 64)
    out[257:260, 130:140] = 1.0
    out[299, 199] = float("nan")
    with pytest.raises(AssertionError) as e:
        X.assert_exact(out, ref, 128, 64, "probe")
    msg = str(e.value)
    assert "31 of 60000" in msg and "first (row, col) = (257, 130)" in msg and "rows 257..299" in msg and "cols 130..199" in msg
    assert "(2,2), (2,3)" in msg and "all in the last row tile (2, ragged): True" in msg and "got 1.0, want 0.0" in msg
    buf, win = X.poisoned(5, 8, torch.bfloat16, "cpu")
    win.zero_()
    X.assert_margins_nan(buf, 5, 8)
    buf[5, 3] = 0
    with pytest.raises(AssertionError, match="OUTSIDE"):
        X.assert_margins_nan(buf, 5, 8)
    buf[5, 3] = float("nan"); win[2, 2] = float("nan")
    with pytest.raises(AssertionError, match="never written"):
        X.assert_margins_nan(buf, 5, 8)


def test_x_stationary_preconditions():
    for K, N in X.XS_SHAPES:
        for seed in (0, 1):
            x, w, bias, res = X.xs_operands(K, N, "cpu", seed=seed)
            acc = x.double() @ w.double().t()
            X.assert_bf16_exact_points([acc, acc + bias.double(), acc + bias.double() + res.double()], f"xs {K} {N}")
        d = X.gn_operands(K, N, "cpu")
        X.assert_bf16_exact_points([d["normed"], d["ref"]], f"gn {K} {N}")
        assert d["normed"].abs().max() <= 14
