// Adaptive projected guidance (APG: Sadat, Hilliges, Weber, ICLR 2025, Algorithm 1; diffusers AdaptiveProjectedGuidance) ahead
// of the sampler's update kernel, for gfx950.
//
// Per clip, over all n = C*THW elements, with p_c / p_u the two predictions in the chosen space and w the guidance scale:
//   d = p_c - p_u,  m = d + momentum m_prev,  s = min(1, norm_threshold / ||m||),  D = s m,
//   par = (D . p_c / ||p_c||^2) p_c,  guided = p_c + (w - 1) ((D - par) + eta par)
// Both spaces are affine in the model output e for a fixed latent x: p = pa x + ps e (model: pa = 0, ps = 1; x0 of a v model:
// pa = sqrt(a_t), ps = -sqrt(1 - a_t); x0 of an eps model: pa = 1 / sqrt(a_t), ps = -sqrt(1 - a_t) / sqrt(a_t)). So
//   d = ps (e_c - e_u)                      formed from the difference of the outputs: no cancellation of the common pa x
//   (D - par) + eta par = D - (1 - eta) par  =: U = s m - g p_c,  g = (1 - eta) s (m . p_c) / ||p_c||^2
//   guided, mapped back to the model's space = e_c + (w - 1) / ps * U
// which at eta = 1 without threshold and momentum is plain CFG to the last bit of one fused multiply-add.
//
// Two launches. apg_reduce_kernel updates m in place and writes three partial sums (||m||^2, m . p_c, ||p_c||^2; s commutes
// with the dot product, so one pass is enough) per workgroup; apg_apply_kernel adds them in a fixed order in float64, forms s
// and g, and writes the guided rows. A thread owns a position and walks its C channels, so channels-last rows and NCTHW are
// both read in whole cache lines. No atomics, no scratch that needs clearing, nothing but plain vector loads and stores:
// capturable, and two runs on the same input give the same bits.
#include "dc_common.h"
#include "dcrafter_hip.h"
#include <math.h>

#define APG_THREADS 256
#define APG_BLOCKS_MAX 256        // workgroups (= partial sums) per clip at most; positions beyond are taken grid-stride
#define APG_APPLY_BLOCKS_MAX 1024

static int apg_blocks(int THW, int cap) {
    const int64_t g = ((int64_t)THW + APG_THREADS - 1) / APG_THREADS;
    return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

// p = pa x + ps e for the step the launch works on
struct ApgAffine { float pa, ps; };
__device__ __forceinline__ ApgAffine apg_affine(const DcApgParams& p) {
    if (!p.x0_space) return {0.f, 1.f};
    const int idx = p.step_index ? p.step_index[0] : p.index;
    if (p.v_param) return {p.sqrt_acp_t[idx], -p.sqrt_1macp_t[idx]};         // predict_start_from_z_and_v ddpm3d.py:239-245
    const float sa = sqrtf(p.a_t[idx]);                                       // ddim.py:258
    return {1.0f / sa, -p.sqrt_one_minus_at[idx] / sa};
}

__device__ __forceinline__ size_t apg_eoff(int nchw, int b, int c, int64_t pos, int C, int THW, int ld) {
    return nchw ? ((size_t)b * C + c) * THW + pos : ((size_t)b * THW + pos) * ld + c;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid (G, B): workgroup (g, b) takes positions g*256 + t, + G*256, ... of clip b -> ws[b][g][3]
__global__ __launch_bounds__(APG_THREADS) void apg_reduce_kernel(const DcApgParams p, const float* __restrict__ ec,
                                                                 const float* __restrict__ eu, int ld_e,
                                                                 const float* __restrict__ x, float* __restrict__ mbuf, int C,
                                                                 int THW, float* __restrict__ ws) {
    __shared__ float red[3][APG_THREADS / 64];
    const int b = blockIdx.y, t = threadIdx.x;
    const ApgAffine k = apg_affine(p);
    const bool keep = p.momentum != 0.f;            // momentum 0: m_prev is not read (the buffer may hold anything)
    float s_mm = 0.f, s_mp = 0.f, s_pp = 0.f;
    for (int64_t pos = (int64_t)blockIdx.x * APG_THREADS + t; pos < THW; pos += (int64_t)gridDim.x * APG_THREADS) {
        for (int c = 0; c < C; ++c) {
            const size_t eoff = apg_eoff(p.e_nchw, b, c, pos, C, THW, ld_e);
            const size_t xoff = ((size_t)b * C + c) * THW + pos;
            const float e = ec[eoff];
            const float pc = fmaf(k.pa, x ? x[xoff] : 0.f, k.ps * e);
            const float d = k.ps * (e - eu[eoff]);
            const float m = keep ? fmaf(p.momentum, mbuf[xoff], d) : d;
            mbuf[xoff] = m;
            s_mm = fmaf(m, m, s_mm);
            s_mp = fmaf(m, pc, s_mp);
            s_pp = fmaf(pc, pc, s_pp);
        }
    }
    s_mm = wave_sum(s_mm); s_mp = wave_sum(s_mp); s_pp = wave_sum(s_pp);
    const int lane = t & 63, wave = t >> 6;
    if (lane == 0) { red[0][wave] = s_mm; red[1][wave] = s_mp; red[2][wave] = s_pp; }
    __syncthreads();
    if (t < 3) ws[((size_t)b * gridDim.x + blockIdx.x) * 3 + t] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
}

// grid (G2, B). Every workgroup adds the G partial sums of its clip (wave j < 3 the j-th sum: a lane takes partials lane,
// lane + 64, ... in order, then the butterfly), then writes out = e_c + (w - 1) / ps * (s m - g p_c) for its positions.
__global__ __launch_bounds__(APG_THREADS) void apg_apply_kernel(const DcApgParams p, const float* __restrict__ ec, int ld_e,
                                                                const float* __restrict__ x, const float* __restrict__ mbuf,
                                                                float* __restrict__ out, int ld_out, int C, int THW,
                                                                const float* __restrict__ ws, int G) {
    __shared__ double tot[3];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (wave < 3) {
        double a = 0.0;
        for (int g = lane; g < G; g += 64) a += (double)ws[((size_t)b * G + g) * 3 + wave];
        a = wave_sum_d(a);
        if (lane == 0) tot[wave] = a;
    }
    __syncthreads();
    const double mm = tot[0], mp = tot[1], pp = tot[2];
    double s = 1.0;
    if (p.norm_threshold > 0.f && mm > 0.0) s = fmin(1.0, (double)p.norm_threshold / sqrt(mm));
    const double coef = pp > 0.0 ? s * mp / pp : 0.0;
    const float sf = (float)s, gf = (float)((1.0 - (double)p.eta) * coef);
    const ApgAffine k = apg_affine(p);
    const float kw = (p.cfg_scale - 1.0f) / k.ps;
    for (int64_t pos = (int64_t)blockIdx.x * APG_THREADS + t; pos < THW; pos += (int64_t)gridDim.x * APG_THREADS) {
        for (int c = 0; c < C; ++c) {
            const size_t xoff = ((size_t)b * C + c) * THW + pos;
            const float e = ec[apg_eoff(p.e_nchw, b, c, pos, C, THW, ld_e)];
            const float pc = fmaf(k.pa, x ? x[xoff] : 0.f, k.ps * e);
            const float u = fmaf(-gf, pc, sf * mbuf[xoff]);
            out[apg_eoff(p.e_nchw, b, c, pos, C, THW, ld_out)] = fmaf(kw, u, e);
        }
    }
}

static int apg_check(const DcApgParams* pp, const float* e_cond, const float* x, const float* mbuf, const float* ws, int ld_e,
                     int B, int C, int THW) {
    if (!pp || !e_cond || !mbuf || !ws) return DC_ERR_ARG;
    const DcApgParams& p = *pp;
    if (p.x0_space) {
        if (!x) return DC_ERR_ARG;
        if (p.v_param ? (!p.sqrt_acp_t || !p.sqrt_1macp_t) : (!p.a_t || !p.sqrt_one_minus_at)) return DC_ERR_ARG;
        if (!p.step_index && p.index < 0) return DC_ERR_ARG;
    }
    if (!isfinite(p.cfg_scale) || !isfinite(p.eta) || !isfinite(p.momentum) || isnan(p.norm_threshold)) return DC_ERR_ARG;
    if (B < 1 || B > 65535 || C < 1 || THW < 1) return DC_ERR_SHAPE;
    if (!p.e_nchw && ld_e < C) return DC_ERR_SHAPE;
    return 0;
}

extern "C" int64_t dc_apg_workspace_floats(int B, int C, int THW) {
    if (B < 1 || C < 1 || THW < 1) return DC_ERR_ARG;
    return (int64_t)B * apg_blocks(THW, APG_BLOCKS_MAX) * 3;
}

extern "C" int dc_apg_reduce(const DcApgParams* pp, const float* e_cond, const float* e_uncond, int ld_e, const float* x,
                             float* momentum_buf, int B, int C, int THW, float* workspace, void* stream_) {
    if (!e_uncond) return DC_ERR_ARG;
    if (int e = apg_check(pp, e_cond, x, momentum_buf, workspace, ld_e, B, C, THW)) return e;
    hipLaunchKernelGGL(apg_reduce_kernel, dim3(apg_blocks(THW, APG_BLOCKS_MAX), B), dim3(APG_THREADS), 0, (hipStream_t)stream_,
                       *pp, e_cond, e_uncond, ld_e, pp->x0_space ? x : nullptr, momentum_buf, C, THW, workspace);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_apg_apply(const DcApgParams* pp, const float* e_cond, int ld_e, const float* x, const float* momentum_buf,
                            float* out, int ld_out, int B, int C, int THW, const float* workspace, void* stream_) {
    if (!out) return DC_ERR_ARG;
    if (int e = apg_check(pp, e_cond, x, momentum_buf, workspace, ld_e, B, C, THW)) return e;
    if (!pp->e_nchw && ld_out < C) return DC_ERR_SHAPE;
    hipLaunchKernelGGL(apg_apply_kernel, dim3(apg_blocks(THW, APG_APPLY_BLOCKS_MAX), B), dim3(APG_THREADS), 0,
                       (hipStream_t)stream_, *pp, e_cond, ld_e, pp->x0_space ? x : nullptr, momentum_buf, out, ld_out, C, THW,
                       workspace, apg_blocks(THW, APG_BLOCKS_MAX));
    DC_CHECK_LAUNCH();
    return 0;
}
