"""Exact-integer checks of dc_gemm_conv: data, float64 reference, mismatch report and the table of kernel variants.

The method needs no tolerance. With small-integer operands every product and every partial sum is an integer far below
2^24, so fp32 accumulation gives the same bits in ANY summation order (tile shape, split-K plan, MFMA shape), and every
integer up to |256| is a bf16 value: each variant, split-K plan and fused epilogue must reproduce a float64 reference bit
for bit, and a mismatch is a list of coordinates, not a norm.

  * bf16 cases: ternary operands {-1, 0, 1} of density p = min(0.75, sqrt(1000 / K)) (accumulator sigma <= 32), integer
    bias / row vector / residual in [-8, 8]. Precondition, asserted on the reference alone: every value at a rounding
    point (before the residual, and the final one) is <= 256 in magnitude and survives a bf16 round trip.
  * the "round" flavour adds a wide integer bias: the fp32 value is still an exact integer, now between bf16 values, and the
    reference is its one round-to-nearest-even bf16 - the only flavour that can tell rounding from truncation.
  * fp32 cases: dense integers in [-31, 31] with alpha in {1, 0.5}; exact only if accumulation really is fp32.
    Precondition: max_row(|x|) @ max_col(|w|) < 2^24.
  * the reference is float64: a plain matmul for mode 0, nine (three) shifted matmuls over the channels-last rows for the
    3x3 (temporal) convs - never a library convolution, whose Winograd / FFT algorithms are not exact on integers.
  * every operand the kernel reads or writes is a window of a larger buffer the test owns, the rest of which is NaN:
    an element the kernel never writes, a store outside [M, N], or a clamped / over-read operand element multiplied into
    a real output all show up in the exact comparison. Only memory inside these tensors is poisoned.

VARIANT_CASES holds, for every name dc_note_variant can report, the smallest shape the dispatch thresholds allow; the
derivation of each shape stands next to it. tests/test_gemm_variants_cpu.py checks the names against the sources, so a
new dc_note_variant name needs an entry here (or a reason in UNREACHABLE)."""
import math

import torch

BF16 = torch.bfloat16
NAN = float("nan")
PLAN_DEFAULT = 19           # gemm_conv_glds.hip: PLAN_DEFAULT = 3 | 16

# margins of the poisoned buffers, in elements: multiples of 8, so that the 16-byte epilogues / LDS-DMA paths still qualify
COL_OFF, COL_PAD, ROW_PAD = 8, 16, 16

# ---- epilogue flavours. The variant name does not tell them apart, so each entry lists the ones its kernel accepts.
EPIS = {
    "bias": dict(bias=True),
    "nobias": dict(bias=False),
    # the rounding itself: an integer bias in [-2000, 2000] puts most outputs between bf16 values (spacing 2 .. 8). The fp32 value
    # before the rounding is still an exact integer in any summation order, so its round-to-nearest-even bf16 is one definite
    # number: truncation, or a second rounding, changes bits. No residual: the ring residual (EPI 3) legitimately rounds once
    # where the epilogue-load residual rounds twice (csrc/gemm_parts.h), which only coincide on bf16-exact values.
    "round": dict(bias=True, wide=True),
    "rv_res": dict(bias=True, rowvec=True, residual=True),      # ResBlock: + embedding row vector, + skip
    "res": dict(bias=True, residual=True),                       # persistent kernels: the residual rides the LDS ring (EPI 3)
    "res_half": dict(bias=True, residual=True, alpha=0.5),       # alpha != 1 keeps the residual on epilogue loads (EPI 1)
    "f32": dict(bias=True, f32=True, alpha=0.5),                 # dense integer data
    "f32_one": dict(bias=False, f32=True, alpha=1.0),
    "gelu": dict(bias=True, gelu=True),                          # bounded, not exact (see activation_bound)
}
ALL_EPIS = ("bias", "nobias", "round", "rv_res", "res", "res_half", "f32")
BF16_EPIS = ("bias", "nobias", "round", "rv_res", "res", "res_half")


def _case(id, variant, kind, shape, epis, plan=PLAN_DEFAULT, geglu=False):
    return dict(id=id, variant=variant, kind=kind, shape=shape, epis=tuple(epis), plan=plan, geglu=geglu)


def _g(M, N, K):
    return dict(M=M, N=N, K=K)


def _c(n, C, Co, H, W, stride=1, pad=1, ups=0):
    return dict(n=n, C=C, Co=Co, H=H, W=W, stride=stride, pad=pad, ups=ups)


def _t(B, T, HW, C, Co):
    return dict(B=B, T=T, HW=HW, C=C, Co=Co)


# Dispatch, as read from dc_gemm_conv (gemm_conv.hip) and dc_gemm_conv_glds_try (gemm_conv_glds.hip); t = row tiles of 256,
# w320 / w256 / w128 = t x column tiles of that width, eff(w) = w / (256 ceil(w / 256)):
#   narrow conv -> window128 conv -> [persistent block, mode 0, K <= 2560, not pipe: GEGLU: ping-pong (plan bit 4, K <= 640,
#   >= 1024 64-wide tiles), <256,geglu> (n_out % 128 == 0, >= 512 tiles), <128,geglu> (>= 512 64-wide tiles); plain:
#   <320> (N % 320 == 0, w320 >= 512), <128> (waste <= 1.15, w128 >= 512), <64> (waste > 1.15, >= 512 64-wide tiles)]
#   -> persistent conv320 (not pipe; N % 320 == 0, >= 1024 tiles conv / >= 512 temporal, K <= 2880)
#   -> GEGLU LDS-DMA tiles (w128 >= 384) -> 320-wide split-K (w320 in [8, 200): every tile cut, nk / splits >= 12; w320 in (256, 1280]
#   with 0 < w320 % 256 <= 128: whole waves + remainder cut, nk / splits >= 8; on the one-wave kernel where pipe_ok) -> 256-wide
#   split-K (N % 256 == 0, not N % 320, bf16) -> 256-wide tile (w256 >= 200, 1.2 eff(w256) >= s128) -> 320-wide tile (w320 >= 200,
#   128 for pipe convs; s320 = 1.25 (1.4) eff(w320) >= s128 = eff(w128) / waste128) -> 128-wide tile (w128 >= 384) -> 128-row kernel.
# pipe_ok (the one-wave kernel): plan bit 0 for 3x3 convs, bit 1 for plain / temporal launches with K >= 1920; N % 320 == 0, bf16.
# Conv images are 31 x 33 (1023 rows: OW is no multiple of 8 and every 256-row tile boundary falls inside an image row), so
# M = frames x 1023 leaves the last row tile ragged; temporal clips are 5 frames of an odd HW for the same reason.
VARIANT_CASES = [
    # ---- the 128-row kernel (gemm_conv.hip): everything the large-tile dispatch declines (-100)
    _case("tile128", "gemm_conv_kernel<128>", "gemm", _g(130, 640, 128), ALL_EPIS + ("f32_one", "gelu")),
    _case("tile64", "gemm_conv_kernel<64>", "gemm", _g(130, 320, 128), ALL_EPIS),               # 384 / 320 = 1.2 > 1.15: 64-wide
    _case("tile_geglu", "gemm_conv_kernel<geglu>", "gemm", _g(130, 256, 128), ("bias", "nobias"), geglu=True),
    _case("tile128_conv_s2", "gemm_conv_kernel<128>", "conv", _c(3, 64, 128, 13, 11, stride=2), ALL_EPIS),
    _case("tile64_conv_aepad", "gemm_conv_kernel<64>", "conv", _c(2, 64, 64, 12, 10, stride=2, pad=0), ("bias", "rv_res", "f32")),
    _case("tile64_conv_ups", "gemm_conv_kernel<64>", "conv", _c(2, 128, 192, 6, 7, ups=1), ("bias", "rv_res", "f32")),
    _case("tile128_tconv", "gemm_conv_kernel<128>", "tconv", _t(2, 5, 37, 128, 128), ("bias", "rv_res", "f32")),
    # ---- LDS-DMA tiles, mode 0
    # N = 384: not 320 k, not 256 k; t = 128 -> w128 = 384 (>= 384, < 512 so not persistent)
    _case("glds128", "gemm_conv_glds_kernel<128>", "gemm", _g(128 * 256 - 37, 384, 128), ALL_EPIS),
    # N = 256, t = 200: persistent <128> needs 2 t >= 512; w256 = 200, 1.2 eff(200) = 0.94 >= s128 = eff(400) = 0.78
    _case("glds256", "gemm_conv_glds_kernel<256>", "gemm", _g(200 * 256 - 50, 256, 128), ALL_EPIS),
    # N = 640, t = 100: w320 = 200, w128 = 500 (< 512). s320 = 1.25 * 200 / 256 and s128 = 500 / 512 are both exactly 0.9765625
    # (for any N = 320 k the two scores tie while both stay inside one wave): the dispatch takes the 320-wide tile on >=
    _case("glds320", "gemm_conv_glds_kernel<320>", "gemm", _g(100 * 256 - 9, 640, 128), ALL_EPIS + ("gelu",)),
    # ---- persistent kernels, mode 0 (>= 512 tiles)
    _case("persist320", "gemm_persist_kernel<320>", "gemm", _g(128 * 256 - 19, 1280, 128), ("bias", "nobias", "round", "f32")),
    _case("persist320_res", "gemm_persist_kernel<320,residual>", "gemm", _g(128 * 256 - 19, 1280, 128), ("rv_res", "res", "res_half")),
    _case("persist128", "gemm_persist_kernel<128>", "gemm", _g(128 * 256 - 19, 512, 128), ALL_EPIS + ("gelu",)),
    # N = 448: 512 / 448 = 1.14 waste, the last 128-wide column tile is half empty (residual: N % 128 != 0 -> epilogue loads)
    _case("persist128_ragged_n", "gemm_persist_kernel<128>", "gemm", _g(128 * 256 - 19, 448, 128), ("bias", "res", "f32")),
    _case("persist64", "gemm_persist_kernel<64>", "gemm", _g(171 * 256 - 5, 192, 128), ALL_EPIS),   # 256 / 192 = 1.33 waste; 171 x 3 = 513
    # ---- GEGLU
    _case("pp_geglu", "gemm_pp_kernel<geglu>", "gemm", _g(128 * 256 - 19, 1024, 128), ("bias", "nobias"), geglu=True),  # 128 x 8 = 1024 tiles
    # K = 704 steps past the ping-pong kernel's K <= 640; n_out = 512: 128 x 4 = 512 tiles of 128 columns
    _case("persist256_geglu", "gemm_persist_kernel<256,geglu>", "gemm", _g(128 * 256 - 19, 1024, 704), ("bias", "nobias"), geglu=True),
    # n_out = 192 (no multiple of 128): 171 x 3 = 513 tiles of 64 columns, below the ping-pong kernel's 1024
    _case("persist128_geglu", "gemm_persist_kernel<128,geglu>", "gemm", _g(171 * 256 - 5, 384, 128), ("bias", "nobias"), geglu=True),
    # K = 2624 steps past the persistent kernels' K <= 2560. n_out = 512, t = 48: w128 = 384, w256 = 192 -> the 128-wide tile;
    # n_out = 1024, t = 64: w256 = 512, eff = 1 -> the 256-wide tile, under the same name
    _case("glds_geglu128", "gemm_conv_glds_kernel<geglu>", "gemm", _g(48 * 256 - 5, 1024, 2624), ("bias", "nobias"), geglu=True),
    _case("glds_geglu256", "gemm_conv_glds_kernel<geglu>", "gemm", _g(64 * 256 - 5, 2048, 2624), ("bias",), geglu=True),
    # ---- the one-wave kernel (gemm_pipe16.h), default plan. 3x3 convs: any K; w320 >= 128 as whole tiles
    # Cin = 64 (nk = 9: no split-K plan has 12 K tiles per range), N = 320, 32 frames: t = 128, s320 = 1.4 * 0.5 >= s128 = 0.75 / 1.2
    _case("pipe_conv", "gemm_pipe320x16_kernel<conv>", "conv", _c(32, 64, 320, 31, 33), BF16_EPIS),
    # 72 tiles: N = 640, 20 frames of 17 x 27 (t = 36); Cin = 256: nk = 36 -> 3 splits of 12 K tiles
    _case("pipe_conv_splitk3", "gemm_pipe320x16_kernel<conv>+splitk", "conv", _c(20, 256, 640, 17, 27), BF16_EPIS),
    # 288 tiles: N = 640, 36 frames (t = 144); Cin = 128: nk = 18 -> 256 whole + 32 x 2 splits of 9, one launch / two (plan bit 6)
    _case("pipe_conv_whole_rem", "gemm_pipe320x16_kernel<conv>+splitk", "conv", _c(36, 128, 640, 31, 33), ("bias", "rv_res", "res_half")),
    _case("pipe_conv_whole_rem_2launch", "gemm_pipe320x16_kernel<conv>+splitk", "conv", _c(36, 128, 640, 31, 33),
          ("bias", "rv_res"), plan=PLAN_DEFAULT | 64),
    # nearest x2 fused: 15 x 17 -> 30 x 34 (1020 rows), 32 frames: t = 128; and 9 frames x 640 wide with Cin = 256: 72 tiles, 3 splits
    _case("pipe_conv_ups", "gemm_pipe320x16_kernel<conv,ups>", "conv", _c(32, 64, 320, 15, 17, ups=1), BF16_EPIS),
    _case("pipe_conv_ups_splitk", "gemm_pipe320x16_kernel<conv,ups>+splitk", "conv", _c(9, 256, 640, 15, 17, ups=1), ("bias", "rv_res")),
    # plain / temporal launches need K >= 1920 (30 K tiles). N = 320, t = 200: s320 = 1.25 * 0.78 >= s128 = eff(600) / 1.2 = 0.65
    _case("pipe_plain", "gemm_pipe320x16_kernel", "gemm", _g(200 * 256 - 7, 320, 1920), BF16_EPIS),
    _case("pipe_plain_splitk", "gemm_pipe320x16_kernel+splitk", "gemm", _g(36 * 256 - 5, 640, 1920), ("bias", "rv_res")),   # 72 tiles, 2 x 15
    _case("pipe_tconv", "gemm_pipe320x16_kernel<tconv>", "tconv", _t(10, 5, 1023, 640, 320), BF16_EPIS),                          # t = 200
    _case("pipe_tconv_splitk", "gemm_pipe320x16_kernel<tconv>+splitk", "tconv", _t(6, 5, 307, 640, 640), ("bias", "rv_res")),  # t = 36
    # ---- 256 x 320 tiles without the one-wave kernel: plan 0 for the 3x3 convs (the documented A/B fallback), or K < 1920
    # N = 1280, 64 frames: t = 256 -> 1024 tiles
    _case("persist320_conv", "gemm_persist_kernel<320,conv>", "conv", _c(64, 64, 1280, 31, 33), BF16_EPIS, plan=0),
    _case("persist320_conv_s2", "gemm_persist_kernel<320,conv>", "conv", _c(64, 64, 1280, 61, 67, stride=2), ("bias",), plan=0),  # 31 x 34 out
    # temporal: K = 192 < 1920 keeps the default plan off the one-wave kernel; N = 1280, t = 128 -> 512 tiles
    _case("persist320_tconv", "gemm_persist_kernel<320,tconv>", "tconv", _t(4, 5, 1637, 64, 1280), BF16_EPIS),
    # N = 320, t = 200: below the persistent kernels' tile counts, s320 = 0.98 > s128 = 0.65
    _case("glds320_conv", "gemm_conv_glds_kernel<320,conv>", "conv", _c(50, 64, 320, 31, 33), ALL_EPIS, plan=0),
    _case("glds320_conv_ups", "gemm_conv_glds_kernel<320,conv>", "conv", _c(50, 64, 320, 15, 17, ups=1), ("bias", "rv_res"), plan=0),
    _case("glds320_tconv", "gemm_conv_glds_kernel<320,tconv>", "tconv", _t(10, 5, 1023, 64, 320), ALL_EPIS),
    # 72 tiles: conv Cin = 256 (nk = 36, 3 splits); temporal Cin = 512 (nk = 24, 2 splits); plain K = 1536 (nk = 24, 2 splits)
    _case("glds320_conv_splitk", "gemm_conv_glds_kernel<320,conv>+splitk", "conv", _c(20, 256, 640, 17, 27), BF16_EPIS, plan=0),
    _case("glds320_tconv_splitk", "gemm_conv_glds_kernel<320,tconv>+splitk", "tconv", _t(6, 5, 307, 512, 640), BF16_EPIS),
    _case("glds320_splitk", "gemm_conv_glds_kernel<320>+splitk", "gemm", _g(36 * 256 - 5, 640, 1536), BF16_EPIS),
    # ---- 128- and 256-wide LDS-DMA tiles in conv / temporal mode (the AutoencoderKL's widths)
    _case("glds128_conv", "gemm_conv_glds_kernel<128,conv>", "conv", _c(32, 64, 384, 31, 33), ALL_EPIS),               # t = 128, w128 = 384
    _case("glds128_tconv", "gemm_conv_glds_kernel<128,tconv>", "tconv", _t(4, 5, 1637, 64, 384), ALL_EPIS),
    # N = 256: 50 frames x 8 window tiles = 400 < 1024 keeps the window kernel off; t = 200 as for glds256
    _case("glds256_conv", "gemm_conv_glds_kernel<256,conv>", "conv", _c(50, 64, 256, 31, 33), ALL_EPIS),
    _case("glds256_conv_aepad", "gemm_conv_glds_kernel<256,conv>", "conv", _c(50, 64, 256, 62, 66, stride=2, pad=0), ("bias",)),   # 31 x 33 out
    _case("glds256_tconv", "gemm_conv_glds_kernel<256,tconv>", "tconv", _t(10, 5, 1023, 64, 256), ALL_EPIS),
    # 256-wide split-K: N = 512, w256s in (256, 1280] with 0 < w256s % 256 <= 128. Mode 0 needs K > 2560 to pass the persistent
    # <128> kernel (4 t >= 512): K = 2624 (nk = 41), t = 130 -> 260 = 256 + 4 x 5 splits of 8
    _case("glds256_splitk", "gemm_conv_glds_kernel<256>+splitk", "gemm", _g(130 * 256 - 7, 512, 2624), BF16_EPIS),
    # conv: 33 frames -> t = 132, 264 = 256 + 8; Cin = 128 (nk = 18): 2 splits of 9. temporal: Cin = 384 (nk = 18)
    _case("glds256_conv_splitk", "gemm_conv_glds_kernel<256,conv>+splitk", "conv", _c(33, 128, 512, 31, 33), BF16_EPIS),
    _case("glds256_tconv_splitk", "gemm_conv_glds_kernel<256,tconv>+splitk", "tconv", _t(11, 3, 1023, 384, 512), BF16_EPIS),
    # ---- the halo-window kernels (gemm_conv.hip) and the tile kernels that take their launches when the plan turns them off
    _case("narrow", "conv3x3_narrow_kernel", "conv", _c(3, 128, 4, 17, 70), ("bias", "nobias", "round", "f32", "f32_one")),
    _case("narrow_off", "gemm_conv_kernel<64>", "conv", _c(3, 128, 4, 17, 70), ("bias", "f32"), plan=PLAN_DEFAULT | 128),
    # 257 frames of 6 x 66: 2 x 2 window tiles each = 1028 tiles (>= 1024), ragged in both directions
    _case("window128", "conv3x3_window128_kernel", "conv", _c(257, 64, 128, 6, 66), ("bias", "nobias", "round", "res")),
    _case("window128_x2", "conv3x3_window128_kernel x2", "conv", _c(257, 64, 256, 6, 66), ("bias", "res")),
    _case("window128_off", "gemm_conv_glds_kernel<128,conv>", "conv", _c(257, 64, 128, 6, 66), ("bias", "res"), plan=PLAN_DEFAULT | 256),  # t = 398
    _case("window128_x2_off", "gemm_conv_glds_kernel<256,conv>", "conv", _c(257, 64, 256, 6, 66), ("bias", "res"), plan=PLAN_DEFAULT | 256),
]

# names that ops.gemm cannot reach without a DC_GEMM_* environment switch (read once per process: tests must not set them),
# each with the dispatch condition that blocks it
UNREACHABLE = {}


def case_params():
    """(case, flavour) pairs in table order, with ids."""
    return [(c, e) for c in VARIANT_CASES for e in c["epis"]]


def case_ids():
    return [f"{c['id']}-{e}" for c, e in case_params()]


def tile_of(variant):
    """(rows, columns) of the variant's output tile, for the mismatch report."""
    if variant.startswith("conv3x3_"):
        return 256, 128                                   # 4 x 64 pixels of one frame: not rows of the GEMM; reported as is
    rows = 128 if variant.startswith("gemm_conv_kernel") else 256
    if "pipe320" in variant:
        return rows, 320
    if "gemm_pp" in variant:
        return rows, 64
    inside = variant[variant.index("<") + 1:variant.index(">")].split(",")
    if inside[0] == "geglu":
        return rows, 64
    cols = int(inside[0])
    return rows, cols // 2 if "geglu" in inside else cols


# ---- geometry ------------------------------------------------------------------------------------------------------
def conv_out_hw(s):
    H, W = (2 * s["H"], 2 * s["W"]) if s["ups"] else (s["H"], s["W"])
    if s["stride"] == 2 and s["pad"] == 0:                # the AutoencoderKL's Downsample: pad (0, 1, 0, 1)
        return (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1
    return (H + 2 * s["pad"] - 3) // s["stride"] + 1, (W + 2 * s["pad"] - 3) // s["stride"] + 1


def geometry(case, cap_rows=None):
    """Shape of the case, optionally with the row count capped (CPU precondition checks of the large entries):
    dict(M, N, K, a_rows, a_cols, shape)."""
    s = dict(case["shape"])
    if case["kind"] == "gemm":
        if cap_rows:
            s["M"] = min(s["M"], cap_rows)
        return dict(M=s["M"], N=s["N"], K=s["K"], a_rows=s["M"], a_cols=s["K"], shape=s)
    if case["kind"] == "conv":
        OH, OW = conv_out_hw(s)
        if cap_rows:
            s["n"] = max(1, min(s["n"], cap_rows // (OH * OW)))
        return dict(M=s["n"] * OH * OW, N=s["Co"], K=9 * s["C"], a_rows=s["n"] * s["H"] * s["W"], a_cols=s["C"], shape=s, OH=OH, OW=OW)
    if cap_rows:
        s["B"] = max(1, min(s["B"], cap_rows // (s["T"] * s["HW"])))
    M = s["B"] * s["T"] * s["HW"]
    return dict(M=M, N=s["Co"], K=3 * s["C"], a_rows=M, a_cols=s["C"], shape=s)


# ---- generators ----------------------------------------------------------------------------------------------------
def density(K):
    return min(0.75, math.sqrt(1000.0 / K))


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def ternary(shape, p, gen):
    """float32 tensor of {-1, 0, 1}, non-zero with probability p."""
    dev = gen.device
    sign = torch.randint(0, 2, shape, generator=gen, device=dev, dtype=torch.int8).float() * 2 - 1
    return sign * (torch.rand(shape, generator=gen, device=dev) < p).float()


def integers(shape, lo, hi, gen):
    """float32 tensor of integers in [lo, hi]."""
    return torch.randint(lo, hi + 1, shape, generator=gen, device=gen.device, dtype=torch.int32).float()


def _seed(case, salt):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(case["id"])) * 7 + salt) % (2 ** 31)


def make_operands(case, dense, device, cap_rows=None):
    """x: float32 integers [a_rows, a_cols] (channels-last rows), w: float32 integers in the torch layout of the op
    ([N, K], [Co, C, 3, 3] or [Co, C, 3, 1, 1]). Ternary, or dense integers in [-31, 31] for the fp32-output flavours."""
    geo = geometry(case, cap_rows)
    gen = _gen(_seed(case, 1 if dense else 0), device)
    s = geo["shape"]
    wshape = {"gemm": (geo["N"], geo["K"]), "conv": (geo["N"], s.get("C"), 3, 3), "tconv": (geo["N"], s.get("C"), 3, 1, 1)}[case["kind"]]
    if dense:
        x = integers((geo["a_rows"], geo["a_cols"]), -31, 31, gen)
        w = integers(wshape, -31, 31, gen)
    else:
        p = density(geo["K"])
        x = ternary((geo["a_rows"], geo["a_cols"]), p, gen)
        w = ternary(wshape, p, gen)
    return geo, x, w


def make_epilogue(case, epi, geo, device):
    """Integer bias [N], row vector [groups, n_out] with rows_per_vec, residual [M, n_out] in [-8, 8] (None where the flavour
    has none). rows_per_vec is no multiple of 128: a group boundary falls inside a row tile."""
    e = EPIS[epi]
    gen = _gen(_seed(case, 100 + sorted(EPIS).index(epi)), device)
    n_out = geo["N"] // 2 if case["geglu"] else geo["N"]
    M = geo["M"]
    wide = bool(e.get("wide"))
    bias = integers((geo["N"],), *((-2000, 2000) if wide else (-8, 8)), gen) if e.get("bias") else None
    rowvec, rpv = None, 1
    if e.get("rowvec"):
        rpv = {"gemm": 1000 if M > 1000 else 37, "conv": geo.get("OH", 0) * geo.get("OW", 0), "tconv": 1000 if M > 1000 else 37}[case["kind"]]
        assert rpv % 128 != 0
        rowvec = integers(((M + rpv - 1) // rpv, n_out), -8, 8, gen)
    residual = integers((M, n_out), -8, 8, gen) if e.get("residual") else None
    return dict(bias=bias, rowvec=rowvec, rows_per_vec=rpv, residual=residual, alpha=e.get("alpha", 1.0), f32=bool(e.get("f32")),
                gelu=bool(e.get("gelu")), wide=wide)


# ---- float64 reference ---------------------------------------------------------------------------------------------
def ref_accumulate(case, geo, x, w):
    """The un-fused result in float64: x @ w.T for mode 0; the convs as shifted matmuls over the channels-last rows."""
    xd = x.double()
    s = geo["shape"]
    if case["kind"] == "gemm":
        return xd @ w.double().t()
    if case["kind"] == "conv":
        n, C, H, W = s["n"], s["C"], s["H"], s["W"]
        img = xd.reshape(n, H, W, C)
        if s["ups"]:                                       # nearest x2
            img = img.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
            H, W = 2 * H, 2 * W
        OH, OW, st = geo["OH"], geo["OW"], s["stride"]
        lo = s["pad"]                                      # zeros before the image; after it, as many as the last tap needs
        need_h, need_w = (OH - 1) * st + 3, (OW - 1) * st + 3
        pad = torch.zeros(n, max(need_h, lo + H), max(need_w, lo + W), C, dtype=torch.float64, device=x.device)
        pad[:, lo:lo + H, lo:lo + W] = img
        acc = torch.zeros(n * OH * OW, geo["N"], dtype=torch.float64, device=x.device)
        wd = w.double()
        for dy in range(3):
            for dx in range(3):
                tap = pad[:, dy:dy + (OH - 1) * st + 1:st, dx:dx + (OW - 1) * st + 1:st].reshape(-1, C)
                acc += tap @ wd[:, :, dy, dx].t()
        return acc
    B, T, HW, C = s["B"], s["T"], s["HW"], s["C"]
    clip = xd.reshape(B, T, HW, C)
    pad = torch.zeros(B, T + 2, HW, C, dtype=torch.float64, device=x.device)
    pad[:, 1:T + 1] = clip
    acc = torch.zeros(B * T * HW, geo["N"], dtype=torch.float64, device=x.device)
    wd = w.double()
    for k in range(3):
        acc += pad[:, k:k + T].reshape(-1, C) @ wd[:, :, k, 0, 0].t()
    return acc


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * (2.0 ** -0.5)))


def ref_epilogue(case, geo, acc, ep):
    """The kernel contract (csrc/gemm_parts.h), in float64: + bias, (GEGLU / GELU), + row vector, * alpha, round to bf16,
    + residual, round again. Returns (ref, rounding_points, extra): rounding_points are the values that must be bf16-exact
    for the comparison to be bit for bit (none for fp32 output); extra holds val / gate for the activation bound."""
    v = acc if ep["bias"] is None else acc + ep["bias"].double()
    extra = {}
    if case["geglu"]:
        n_out = geo["N"] // 2
        val, gate = v[:, :n_out], v[:, n_out:]
        extra = dict(val=val, gate=gate)
        v = val * gelu_erf(gate)
    elif ep["gelu"]:
        extra = dict(val=torch.ones_like(v), gate=v)                    # gelu(x) = 1 * gelu(x): the bound's |val| is 1
        v = gelu_erf(v)
    if ep["rowvec"] is not None:
        v = v + ep["rowvec"].double().repeat_interleave(ep["rows_per_vec"], 0)[:geo["M"]]
    if ep["alpha"] != 1.0:
        v = v * ep["alpha"]
    if ep["f32"]:
        return v, [], extra
    if ep["wide"]:                                         # an exact fp32 integer, rounded to nearest even once
        assert ep["residual"] is None and not extra
        assert v.abs().max().item() < 2 ** 24 and torch.equal(v.float().double(), v) and torch.equal(v.round(), v)
        return v.float().to(BF16).double(), [], extra
    points = [v]
    if ep["residual"] is not None:
        v = v + ep["residual"].double()
        points.append(v)
    return v, points, extra


def assert_bf16_exact_points(points, what=""):
    """Precondition of a bf16 case, on the reference alone: every rounding point holds values <= 256 that are bf16 numbers."""
    for i, v in enumerate(points):
        big = v.abs().max().item()
        assert big <= 256, f"{what}: reference reaches {big} at rounding point {i} - the generator's bound does not hold"
        assert torch.equal(v.float().to(BF16).double(), v), f"{what}: reference is not bf16-exact at rounding point {i}"


def assert_fp32_exact_operands(case, geo, x, w, what=""):
    """Precondition of an fp32 case: the sum of |products| of any output stays below 2^24, so every partial sum is exact."""
    if case["kind"] == "gemm":
        bound = x.abs().amax(0).double() @ w.abs().amax(0).double()
    elif case["kind"] == "conv":
        bound = (x.abs().amax(0).double() * w.abs().amax(0).double().sum((1, 2))).sum()
    else:
        bound = (x.abs().amax(0).double() * w.abs().amax(0).double().sum((1, 2, 3))).sum()
    assert float(bound) + 8 < 2 ** 24, f"{what}: sum of |products| can reach {float(bound)} >= 2^24"


def activation_bound(ref, extra):
    """GEGLU / GELU outputs are not exact: the epilogues' GELU is x Phi(x) with a polynomial Phi, pinned by
    test_gelu_phi_error at |gelu_phi - gelu_erf| < 2.5e-4, and the product is rounded to bf16 once (half an ulp <= 2^-8
    relative). With integer val and gate: |out - val gelu_erf(gate)| <= 2.5e-4 |val| + 2^-8 |ref|. Beyond |gate| = 4 the
    kernel's GELU is exactly x or exactly 0 (same test), so those entries get bound 0 against val * gate (an integer, exact
    in fp32) rounded to bf16 once, or against 0.
    Returns (want, bound)."""
    val, gate = extra["val"], extra["gate"]
    bound = 2.5e-4 * val.abs() + 2.0 ** -8 * ref.abs()
    far = gate.abs() > 4
    exact = torch.where(gate > 4, val * gate, torch.zeros_like(val))
    want = torch.where(far, exact.float().to(BF16).double(), ref)
    return want, torch.where(far, torch.zeros_like(bound), bound)


# ---- poisoned buffers ----------------------------------------------------------------------------------------------
def poisoned(rows, cols, dtype, device, fill=None):
    """A [rows, cols] window (column offset COL_OFF, ROW_PAD rows after it) of a larger NaN-filled buffer.
    Returns (buffer, window)."""
    buf = torch.full((rows + ROW_PAD, cols + COL_OFF + COL_PAD), NAN, dtype=dtype, device=device)
    win = buf[:rows, COL_OFF:COL_OFF + cols]
    if fill is not None:
        win.copy_(fill)
    return buf, win


def assert_margins_nan(buf, rows, cols, what=""):
    """Nothing outside the window was written (all of it is still NaN) and nothing inside it is NaN."""
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[:rows, COL_OFF:COL_OFF + cols] = False
    nan = torch.isnan(buf)
    touched = (mask & ~nan).nonzero()
    assert touched.shape[0] == 0, (f"{what}: {touched.shape[0]} elements OUTSIDE the [{rows}, {cols}] output were written; first at "
                                   f"buffer (row, col) = {tuple(touched[0].tolist())} (window starts at column {COL_OFF})")
    inside = (~mask & nan).nonzero()
    assert inside.shape[0] == 0, (f"{what}: {inside.shape[0]} output elements are NaN (never written, or fed by poisoned padding); first at "
                                  f"(row, col) = ({inside[0][0].item()}, {inside[0][1].item() - COL_OFF})")


# ---- report --------------------------------------------------------------------------------------------------------
def mismatch_report(bad, got, want, tile_rows, tile_cols, what=""):
    """Where the mismatches are: count, first (row, col), bounding box, the (row tile, column tile) pairs hit, whether they
    all lie in the last (ragged) row tile, three (got, want) samples."""
    idx = bad.nonzero()
    n = idx.shape[0]
    r, c = idx[:, 0], idx[:, 1]
    M, N = bad.shape
    tiles = torch.unique(torch.stack([r // tile_rows, c // tile_cols], 1), dim=0).tolist()
    last_tile = (M - 1) // tile_rows
    ragged = M % tile_rows != 0
    only_last = all(t[0] == last_tile for t in tiles)
    pick = sorted({0, n // 2, n - 1})
    samples = [f"({r[i].item()}, {c[i].item()}): got {got[r[i], c[i]].item()!r}, want {want[r[i], c[i]].item()!r}" for i in pick]
    shown = ", ".join(f"({a},{b})" for a, b in tiles[:16]) + (f", ... {len(tiles)} in all" if len(tiles) > 16 else "")
    return (f"{what}: {n} of {M * N} elements differ from the float64 reference\n"
            f"  first (row, col) = ({r[0].item()}, {c[0].item()}); bounding box rows {r.min().item()}..{r.max().item()}, "
            f"cols {c.min().item()}..{c.max().item()}\n"
            f"  {tile_rows} x {tile_cols} tiles hit (row tile, column tile): {shown}\n"
            f"  all in the last row tile ({last_tile}, {'ragged' if ragged else 'whole'}): {only_last}\n"
            f"  samples: " + "; ".join(samples))


def assert_exact(out, ref, tile_rows, tile_cols, what=""):
    """out (bf16 or fp32) equals the float64 reference element for element (a NaN in out is a mismatch)."""
    assert out.shape == ref.shape, (out.shape, ref.shape)
    got = out.double()
    bad = ~(got == ref)
    if bad.any().item():
        raise AssertionError(mismatch_report(bad, got, ref, tile_rows, tile_cols, what))


def assert_within(out, want, bound, tile_rows, tile_cols, what=""):
    """|out - want| <= bound element for element (bound 0: equality); same report."""
    got = out.double()
    bad = ~((got - want).abs() <= bound)
    if bad.any().item():
        raise AssertionError(mismatch_report(bad, got, want, tile_rows, tile_cols, what))


# ---- the X-stationary kernels of ff_fused.hip that can be exact ------------------------------------------------------
XS_SHAPES = [(K, N) for K in (320, 640) for N in (64, 96, 320, 1280)]
XS_M = 128 * 3 - 5                       # ragged last 128-row tile
GN_INST, GN_RPI, GN_GROUPS = 3, 128, 32


def xs_operands(K, N, device, w_density=None, seed=0):
    gen = _gen(9000 + K * 7 + N + seed, device)
    p = density(K)
    x = ternary((XS_M, K), p, gen)
    w = ternary((N, K), p if w_density is None else w_density, gen)
    bias = integers((N,), -8, 8, gen)
    res = integers((XS_M, N), -8, 8, gen)
    return x, w, bias, res


def gn_operands(K, N, device):
    """x ternary [3 x 128, K]; hand-made statistics per (instance, group): integer mean in [-2, 2], rstd in {1, 2}; gamma in
    {1, 2}, beta integer in [-2, 2]: (x - mean) rstd gamma + beta is a small integer (|.| <= 14) in any evaluation order,
    and a wrong instance or group index changes it. The weight is sparse enough for the <= 256 precondition:
    E[normalised^2] is about 20, so density 1000 / (20 K) keeps the accumulator's sigma near 32."""
    gen = _gen(9500 + K * 7 + N, device)
    M = GN_INST * GN_RPI
    x = ternary((M, K), 0.75, gen)
    mean = integers((GN_INST, GN_GROUPS), -2, 2, gen)
    rstd = integers((GN_INST, GN_GROUPS), 1, 2, gen)
    gamma = integers((K,), 1, 2, gen)
    beta = integers((K,), -2, 2, gen)
    w = ternary((N, K), min(0.75, 1000.0 / (20.0 * K)), gen)
    bias = integers((N,), -8, 8, gen)
    cpg = K // GN_GROUPS
    mean_rc = mean.repeat_interleave(GN_RPI, 0).repeat_interleave(cpg, 1)
    rstd_rc = rstd.repeat_interleave(GN_RPI, 0).repeat_interleave(cpg, 1)
    normed = (x.double() - mean_rc.double()) * rstd_rc.double() * gamma.double() + beta.double()
    ref = normed @ w.double().t() + bias.double()
    stats = torch.stack([mean, rstd], -1).reshape(-1).contiguous()
    return dict(x=x, w=w, bias=bias, gamma=gamma, beta=beta, stats=stats, normed=normed, ref=ref)
