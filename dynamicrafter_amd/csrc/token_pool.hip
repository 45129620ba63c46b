// LayerNorm + spatial token pooling for K/V token downsampling ("ToDo", Smith et al., IJCAI 2024) of the spatial self-attention:
// from the bf16 rows [F*H*W, C] of a transformer's hidden state it writes the LayerNorm'd tokens of the pooled grid
// [F*Hp*Wp, C], Hp = ceil(H/f), Wp = ceil(W/f), which the K/V projection then reads instead of all H*W tokens.
//   mode 0 (nearest): p[yp][xp] = LN(x[yp f][xp f]): only the kept rows are read. The row arithmetic is layernorm_kernel's
//                     (norms.hip), operation for operation - vectors lane + 64 j, wave_sum, rsqrtf(var + eps) - so the output equals
//                     the corresponding rows of dc_layernorm bit for bit.
//   mode 1 (mean):    p[yp][xp] = mean of LN(x[y][x']) over the cell y in [yp f, min(H, yp f + f)), x' likewise: every token of the
//                     cell is normalised in fp32, the cell is summed in (y, x') order, multiplied by 1 / (tokens in the cell) and
//                     rounded to bf16 once.
// One wave per output token, 16-byte loads and stores, no atomics, no scratch: capturable and bit-reproducible. HBM-bound: mode 0
// moves 4 C bytes per output token, mode 1 up to (2 f^2 + 2) C.
//   reference: nn.LayerNorm norm1 lvdm/modules/attention.py:225-227,243 ahead of attn1's to_k / to_v (:75-76); the pooling itself
//   is not in the reference.
#include "dc_common.h"
#include "dcrafter_hip.h"

namespace {

// LayerNorm of one row into o (this lane's vectors lane + 64 j): the arithmetic of layernorm_kernel, in its order
template <int MAXV>
__device__ __forceinline__ void ln_row(const bf16_t* __restrict__ xr, int lane, int vecs, float invC, float eps,
                                       const float* __restrict__ gamma, const float* __restrict__ beta, float (&o)[MAXV][8]) {
    float f[MAXV][8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int v = lane + 64 * j;
        if (v < vecs) {
            const uint4 raw = *reinterpret_cast<const uint4*>(xr + v * 8);
            unpack_bf8(raw, f[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += f[j][e];
        }
    }
    const float mean = wave_sum(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int v = lane + 64 * j;
        if (v < vecs) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = f[j][e] - mean; q += d * d; }
        }
    }
    const float rstd = rsqrtf(wave_sum(q) * invC + eps);
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int v = lane + 64 * j;
        if (v < vecs) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = v * 8 + e;
                o[j][e] = (f[j][e] - mean) * rstd * gamma[c] + beta[c];
            }
        }
    }
}

// one wave per output token, four per workgroup; grid-stride over the F * Hp * Wp tokens
template <int MAXV, bool MEAN>
__global__ __launch_bounds__(256) void ln_pool_kernel(const bf16_t* __restrict__ x, int ldx, bf16_t* __restrict__ y, int ldy,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      int n_out, int H, int W, int Hp, int Wp, int C, int fac, float eps) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int vecs = C >> 3;
    const float invC = 1.0f / (float)C;
    for (long long tl = blockIdx.x * 4 + wave; tl < n_out; tl += gridDim.x * 4) {       // 64-bit: n_out may be close to 2^31
        const int t = (int)tl;
        const int fr = t / (Hp * Wp);
        const int rem = t - fr * (Hp * Wp);
        const int yp = rem / Wp, xp = rem - yp * Wp;
        const int y0 = yp * fac, x0 = xp * fac;                    // < H, < W: Hp = ceil(H / fac), Wp = ceil(W / fac)
        const bf16_t* cell = x + ((size_t)fr * H * W + (size_t)y0 * W + x0) * ldx;
        float o[MAXV][8];
        if (!MEAN) {
            ln_row<MAXV>(cell, lane, vecs, invC, eps, gamma, beta, o);
        } else {
            const int ny = H - y0 < fac ? H - y0 : fac;            // the cell, clipped at the border
            const int nx = W - x0 < fac ? W - x0 : fac;
            float acc[MAXV][8];
#pragma unroll
            for (int j = 0; j < MAXV; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
            for (int dy = 0; dy < ny; ++dy)
                for (int dx = 0; dx < nx; ++dx) {
                    ln_row<MAXV>(cell + ((size_t)dy * W + dx) * ldx, lane, vecs, invC, eps, gamma, beta, o);
#pragma unroll
                    for (int j = 0; j < MAXV; ++j)
                        if (lane + 64 * j < vecs) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) acc[j][e] += o[j][e];
                        }
                }
            const float inv_n = 1.0f / (float)(ny * nx);
#pragma unroll
            for (int j = 0; j < MAXV; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) o[j][e] = acc[j][e] * inv_n;
        }
#pragma unroll
        for (int j = 0; j < MAXV; ++j) {
            const int v = lane + 64 * j;
            if (v < vecs) *reinterpret_cast<uint4*>(y + (size_t)t * ldy + v * 8) = pack_bf8(o[j]);
        }
    }
}

template <int MAXV>
void launch_pool(int mode, int grid, hipStream_t stream, const bf16_t* x, int ldx, bf16_t* y, int ldy, const float* gamma,
                 const float* beta, int n_out, int H, int W, int Hp, int Wp, int C, int fac, float eps) {
    if (mode == 0)
        hipLaunchKernelGGL((ln_pool_kernel<MAXV, false>), dim3(grid), dim3(256), 0, stream, x, ldx, y, ldy, gamma, beta, n_out, H, W,
                           Hp, Wp, C, fac, eps);
    else
        hipLaunchKernelGGL((ln_pool_kernel<MAXV, true>), dim3(grid), dim3(256), 0, stream, x, ldx, y, ldy, gamma, beta, n_out, H, W,
                           Hp, Wp, C, fac, eps);
}

}  // namespace

extern "C" int dc_ln_pool_tokens(const uint16_t* x, int ldx, uint16_t* y, int ldy, const float* gamma, const float* beta, int F,
                                 int H, int W, int C, int factor, int mode, float eps, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!x || !y || !gamma || !beta) return DC_ERR_ARG;
    if (C <= 0 || C % 8 != 0 || C > 2048 || ldx % 8 != 0 || ldy % 8 != 0 || ldx < C || ldy < C) return DC_ERR_SHAPE;
    if (F < 1 || H < 1 || W < 1 || factor < 2 || factor > 8 || (mode != 0 && mode != 1)) return DC_ERR_SHAPE;
    if (((uintptr_t)x | (uintptr_t)y) & 15) return DC_ERR_SHAPE;              // 16-byte loads and stores
    if ((int64_t)F * H * W > 0x7fffffffLL) return DC_ERR_SHAPE;
    const int Hp = (H + factor - 1) / factor, Wp = (W + factor - 1) / factor;
    const int n_out = F * Hp * Wp;
    int grid = (n_out + 3) / 4;
    if (grid > 16384) grid = 16384;
    const int vecs = C / 8;
    if (vecs <= 64)
        launch_pool<1>(mode, grid, stream, x, ldx, y, ldy, gamma, beta, n_out, H, W, Hp, Wp, C, factor, eps);
    else if (vecs <= 128)
        launch_pool<2>(mode, grid, stream, x, ldx, y, ldy, gamma, beta, n_out, H, W, Hp, Wp, C, factor, eps);
    else
        launch_pool<4>(mode, grid, stream, x, ldx, y, ldy, gamma, beta, n_out, H, W, Hp, Wp, C, factor, eps);
    DC_CHECK_LAUNCH();
    return 0;
}
