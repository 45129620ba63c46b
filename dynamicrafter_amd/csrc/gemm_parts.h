// The two decisions of dc_gemm_conv that every kernel implementing it shares (gemm_conv.hip, gemm_conv_glds.hip with gemm_pipe16.h /
// gemm_pp.h): what the epilogue computes, in which order, and how the conv modes address their input. A kernel keeps its own
// accumulator layout, guards and address form (pointer, 32-bit offset + buffer descriptor, zero chunk) and calls these pieces.
// Everything here is forced inline: a kernel that uses them compiles to the arithmetic it would spell out itself.
//
// THE EPILOGUE, on 4 consecutive output channels n .. n + 3 of output row m, all in fp32 until the rounding:
//   1. + bias[n]                                   (GEGLU: the gate columns get bias[N/2 + n])
//   2. GEGLU: value *= DC_GELU(gate)
//   3. DC_GEMM_GELU: DC_GELU(value)
//   4. + rowvec[m / rows_per_vec][n]               (the per-row-group vector: ResBlock embedding add)
//   5. * alpha                                     (skipped when alpha == 1)
//   6. fp32 output: stored as is. bf16 output: rounded to bf16,
//   7. + residual[m][n] on the ROUNDED value - the reference adds two already-rounded tensors -, and
//   8. rounded to bf16 again.
// Sites that differ, and keep their behaviour:
//   * gemm_pp.h (GEGLU only) preloads the bias registers (zeros without a bias) and adds them while it forms the value and the
//     gate, the gate's inside the DC_GELU argument: the same sums in the same order as steps 1-2.
//   * the ring residual of gemm_persist_kernel (EPI 3) adds the residual on the MFMA pipe in fp32, BEFORE step 1, and rounds once;
//     dispatch takes it only where steps 3 and 5 are off (ring_residual_ok).
//   * conv3x3_narrow_kernel and conv3x3_window128_kernel (gemm_conv.hip) are dispatched without rowvec / GELU: the narrow one
//     has steps 1, 5 (always multiplies: x * 1 is x) and 6 on bias registers loaded once, the window one steps 1 and 6-8.
//
// THE K ORDER OF THE CONV MODES. K = taps * Cin is ordered (64-channel slice, tap, channel), the order ops.PackedWeight packs
// for: a 3x3 weight is stored [Cout][Cin/64][kh*kw][64], a temporal one [Cout][Cin/64][3][64]. K tile kt (64 wide) is therefore
// tap kt % 9 (kt % 3) of slice kt / 9 (kt / 3), tap = 3 dy + dx: the taps of one slice are consecutive K tiles, so taps 2..9
// re-read (shifted) rows that the first tap just pulled into L2. Output row m is pixel (oy, ox) of frame n in row-major order;
// its tap (dy, dx) reads input pixel (oy * stride - pad + dy, ox * stride - pad + dx), zero outside the image. A row carries one
// validity bit per tap (bit t = tap t may be dereferenced); rows beyond M have none.
// Two sites compute their own masks, because any other spelling changed instructions inside their K loops
// (profiles/gemm_parts_isa.txt): gemm_persist_kernel's set_issue_tile, which runs between the MFMAs of its tile loop, keeps the
// 9-tap loop, and gemm_pipe320x16_kernel keeps the 3-bit temporal mask, of which it is the only user.
#pragma once
#include "dc_common.h"
#include "dcrafter_hip.h"

namespace {

// ---- epilogue values
__device__ __forceinline__ void ep_add4(float4& v, const float* src) {
    const float4 a = *reinterpret_cast<const float4*>(src);
    v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
}
__device__ __forceinline__ void ep_geglu4(float4& v, const float4& g) {
    v.x *= DC_GELU(g.x); v.y *= DC_GELU(g.y); v.z *= DC_GELU(g.z); v.w *= DC_GELU(g.w);
}
__device__ __forceinline__ void ep_gelu4(float4& v, const DcGemmParams& p) {
    if (p.flags & DC_GEMM_GELU) { v.x = DC_GELU(v.x); v.y = DC_GELU(v.y); v.z = DC_GELU(v.z); v.w = DC_GELU(v.w); }
}
__device__ __forceinline__ void ep_alpha4(float4& v, const DcGemmParams& p) {
    if (p.alpha != 1.0f) { v.x *= p.alpha; v.y *= p.alpha; v.z *= p.alpha; v.w *= p.alpha; }
}
// row m's vector (only where p.rowvec is set: rows_per_vec is 0 without one)
__device__ __forceinline__ const float* ep_rowvec_row(const DcGemmParams& p, int m) {
    return p.rowvec + (size_t)(m / p.rows_per_vec) * p.rowvec_ld;
}
// steps 3-5 for (m, n) (two forms, and ep_pack4's by-value argument: profiles/gemm_parts_isa.txt has the reasons)
__device__ __forceinline__ void ep_tail4(float4& v, const DcGemmParams& p, int m, int n) {
    ep_gelu4(v, p);
    if (p.rowvec) ep_add4(v, ep_rowvec_row(p, m) + n);
    ep_alpha4(v, p);
}
// steps 3-5 where the caller fetched the row's vector once per row and has guards of its own: rv_on = there is a row vector and
// this lane may read it, rv_row = ep_rowvec_row
__device__ __forceinline__ void ep_tail4(float4& v, const DcGemmParams& p, bool rv_on, const float* rv_row, int n) {
    ep_gelu4(v, p);
    if (rv_on) ep_add4(v, rv_row + n);
    ep_alpha4(v, p);
}
__device__ __forceinline__ uint2 ep_pack4(float4 v) {
    uint2 pk;
    pk.x = pack_bf2(v.x, v.y);
    pk.y = pack_bf2(v.z, v.w);
    return pk;
}
// steps 6-8 for channels n .. n + 3 of row m
__device__ __forceinline__ void ep_store4(const DcGemmParams& p, bool out_f32, int m, int n, const float4& v) {
    if (out_f32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n) = v;
    } else {
        uint2 pk = ep_pack4(v);
        if (p.residual) {
            const uint2 rr = *reinterpret_cast<const uint2*>(p.residual + (size_t)m * p.ldr + n);
            pk.x = add_bf2(pk.x, rr.x);
            pk.y = add_bf2(pk.y, rr.y);
        }
        *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(p.C) + (size_t)m * p.ldc + n) = pk;
    }
}

// ---- conv addressing
// output row m -> frame n, output pixel (oy, ox)
__device__ __forceinline__ void conv_row(const DcGemmParams& p, int m, int& n, int& oy, int& ox) {
    const int ohw = p.OH * p.OW;
    n = m / ohw;
    const int rem = m - n * ohw;
    oy = rem / p.OW;
    ox = rem - oy * p.OW;
}
// 9-bit tap mask of a row whose tap (0, 0) is pixel (y0, x0) of an h x w image: the input image, or - nearest x2 upsampling fused
// into a stride-1 pad-1 conv - the OUTPUT image with (y0, x0) = (oy - 1, ox - 1)
__device__ __forceinline__ int conv_tap_mask(bool ok, int y0, int x0, int h, int w) {
    int mask = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int y = y0 + t / 3, x = x0 + t % 3;
        if (ok && y >= 0 && y < h && x >= 0 && x < w) mask |= 1 << t;
    }
    return mask;
}
// frame index of row m of the temporal conv (tap t reads frame + t - 1)
__device__ __forceinline__ int tconv_frame(const DcGemmParams& p, int m) { return (m / p.HW) % p.T; }
// K tile kt -> 64-channel slice cs and tap (= 3 dy + dx for the 3x3 modes)
__device__ __forceinline__ void conv_ktile(int kt, int& cs, int& tap, int& dy, int& dx) {
    cs = kt / 9;
    tap = kt - cs * 9;
    dy = tap / 3;
    dx = tap - dy * 3;
}
__device__ __forceinline__ void tconv_ktile(int kt, int& cs, int& tap) {
    cs = kt / 3;
    tap = kt - cs * 3;
}
// weight row of row r of a BN-row B tile at output column n0: GEGLU tiles hold BN/2 value rows, then their BN/2 gate rows
template <int BN, bool GEGLU>
__device__ __forceinline__ int gemm_wrow(const DcGemmParams& p, int n0, int r) {
    if (GEGLU) return (r < BN / 2) ? (n0 + r) : ((p.N >> 1) + n0 + (r - BN / 2));
    return n0 + r;
}

}  // namespace
