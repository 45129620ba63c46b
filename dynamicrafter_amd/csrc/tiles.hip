// Spatially tiled sampling (frames larger than the trained size): the UNet runs on boxes of its own extent (T, H, Wd)
// inside one long latent [B, C, T_long, H_long, W_long] and the outputs are blended where boxes overlap (MultiDiffusion,
// arXiv:2302.08113, in space - and in time too when the time axis is tiled). Two kernels: the box form of
// pack_latent_kernel and the box form of window_merge_kernel (elementwise.hip). Both index two per-step device tables by
// the device step counter: box int32 [S][W][3] = (t0, y0, x0), g fp32 [S][W][T + H + Wd] = the three per-axis weight
// vectors of the box, concatenated.
#include "dc_common.h"
#include "dcrafter_hip.h"

namespace {

// x [B][Cx][T_long][H_long][W_long], cc [B][Cc][...] fp32 -> rows [nrep][B][n_w][T][H][Wd][c_pad] bf16. One thread per
// (b, w, f, y, x) with x fastest: the lanes of a wave read runs of Wd consecutive floats of a latent row. The per-element
// conversion is pack_latent_kernel's (pack_bf8). A start outside its range is clamped into it (the host wrapper refuses
// such a table; this keeps a wrong one from reading outside x).
__global__ void pack_latent_tiles_kernel(const float* __restrict__ x, const float* __restrict__ cc, bf16_t* __restrict__ out,
                                         const int32_t* __restrict__ box, const int32_t* __restrict__ step_index, int index,
                                         int S, int W, int w0, int n_w, int B, int Cx, int Cc, int T_long, int H_long,
                                         int W_long, int T, int H, int Wd, int c_pad, int nrep) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int THW = T * H * Wd;
    const int64_t total = (int64_t)B * n_w * THW;
    if (idx >= total) return;
    const int step = step_index ? step_index[0] : index;
    if (step < 0 || step >= S) return;
    const int pos = (int)(idx % THW);
    const int bw = (int)(idx / THW);
    const int b = bw / n_w, w = bw - b * n_w;
    const int px = pos % Wd, py = (pos / Wd) % H, pf = pos / (Wd * H);
    const int32_t* bx = box + ((size_t)step * W + w0 + w) * 3;
    const int t0 = min(max(bx[0], 0), T_long - T);
    const int y0 = min(max(bx[1], 0), H_long - H);
    const int x0 = min(max(bx[2], 0), W_long - Wd);
    const size_t lpos = ((size_t)(t0 + pf) * H_long + (y0 + py)) * W_long + (x0 + px);
    const size_t LTHW = (size_t)T_long * H_long * W_long;
    for (int c0 = 0; c0 < c_pad; c0 += 8) {
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = c0 + e;
            float v = 0.f;
            if (c < Cx) v = x[((size_t)b * Cx + c) * LTHW + lpos];
            else if (c < Cx + Cc) v = cc[((size_t)b * Cc + (c - Cx)) * LTHW + lpos];
            f[e] = v;
        }
        const uint4 pk = pack_bf8(f);
        for (int r = 0; r < nrep; ++r)
            *reinterpret_cast<uint4*>(out + ((size_t)r * total + idx) * c_pad + c0) = pk;
    }
}

// e rows [(k, b, w, f, y, x)][ld_e] fp32 (first C channels) -> out rows [(k, b, F, Y, X)][ld_out]:
//   out = sum_w fl(fl(gt_w[F - t0_w] * gy_w[Y - y0_w]) * gx_w[X - x0_w]) * e[k, b, w, F - t0_w, Y - y0_w, X - x0_w]
// over the n_w boxes of this call that contain (F, Y, X) with a non-zero weight, in ascending w: the first term is a
// product, every later one a fused multiply-add, so a chunked evaluation (accumulate: start from what out holds) rounds as
// the unchunked one and a single box of weight 1 returns its input. One thread per output row; the box loop reads the
// tables at addresses that do not depend on the thread. VEC: C == 4 with 16-byte aligned rows.
template <bool VEC>
__global__ __launch_bounds__(256) void tile_merge_kernel(const float* __restrict__ e, int ld_e, float* __restrict__ out,
                                                         int ld_out, const int32_t* __restrict__ box,
                                                         const float* __restrict__ g,
                                                         const int32_t* __restrict__ step_index, int index, int S, int W,
                                                         int w0, int n_w, int KB, int C, int T_long, int H_long, int W_long,
                                                         int T, int H, int Wd, int accumulate) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // (kb, F, Y, X)
    const int64_t total = (int64_t)KB * T_long * H_long * W_long;
    if (idx >= total) return;
    const int step = step_index ? step_index[0] : index;
    if (step < 0 || step >= S) return;
    const int X = (int)(idx % W_long);
    int64_t r = idx / W_long;
    const int Y = (int)(r % H_long);
    r /= H_long;
    const int F = (int)(r % T_long);
    const int kb = (int)(r / T_long);
    const int G = T + H + Wd;
    const int32_t* bx = box + ((size_t)step * W + w0) * 3;
    const float* gw = g + ((size_t)step * W + w0) * G;
    float* o = out + (size_t)idx * ld_out;
    constexpr int MAXC = 4;
    for (int c0 = 0; c0 < C; c0 += MAXC) {
        const int nc = min(MAXC, C - c0);
        float acc[MAXC] = {0.f, 0.f, 0.f, 0.f};
        bool have = false;
        if (accumulate) {
            have = true;
            if (VEC) { const float4 v = *reinterpret_cast<const float4*>(o); acc[0] = v.x; acc[1] = v.y; acc[2] = v.z; acc[3] = v.w; }
            else for (int c = 0; c < nc; ++c) acc[c] = o[c0 + c];
        }
        for (int w = 0; w < n_w; ++w) {
            const int f = F - bx[w * 3 + 0], y = Y - bx[w * 3 + 1], x = X - bx[w * 3 + 2];
            if (f < 0 || f >= T || y < 0 || y >= H || x < 0 || x >= Wd) continue;
            const float* gv = gw + (size_t)w * G;
            const float wt = __fmul_rn(__fmul_rn(gv[f], gv[T + y]), gv[T + H + x]);
            if (wt == 0.f) continue;                           // padding box: its output is never read
            const float* src = e + (((((size_t)kb * n_w + w) * T + f) * H + y) * Wd + x) * ld_e + c0;
            float v[MAXC] = {0.f, 0.f, 0.f, 0.f};
            if (VEC) { const float4 q = *reinterpret_cast<const float4*>(src); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
            else for (int c = 0; c < nc; ++c) v[c] = src[c];
#pragma unroll
            for (int c = 0; c < MAXC; ++c) acc[c] = have ? __fmaf_rn(wt, v[c], acc[c]) : __fmul_rn(wt, v[c]);
            have = true;
        }
        if (VEC) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else for (int c = 0; c < nc; ++c) o[c0 + c] = acc[c];
    }
}

// the geometry both entries share: a box of (T, H, Wd) inside (T_long, H_long, W_long), the boxes w0 .. w0 + n_w - 1 of W
bool tile_geometry_ok(const int32_t* step_index, int index, int S, int W, int w0, int n_w, int T_long, int H_long,
                      int W_long, int T, int H, int Wd) {
    return T >= 1 && H >= 1 && Wd >= 1 && T_long >= T && H_long >= H && W_long >= Wd && S >= 1 && W >= 1 && w0 >= 0 &&
           n_w >= 1 && n_w <= W && w0 <= W - n_w && (step_index || (index >= 0 && index < S));
}

}  // namespace

extern "C" int dc_pack_latent_tiles(const float* x, const float* cc, uint16_t* out, const int32_t* box,
                                    const int32_t* step_index, int index, int S, int W, int w0, int n_w, int B, int Cx,
                                    int Cc, int T_long, int H_long, int W_long, int T, int H, int Wd, int c_pad, int nrep,
                                    void* stream_) {
    if (!x || !out || !box || (Cc > 0 && !cc)) return DC_ERR_ARG;
    if (c_pad % 8 != 0 || Cx < 1 || Cc < 0 || c_pad < Cx + Cc || nrep < 1 || B < 1 ||
        !tile_geometry_ok(step_index, index, S, W, w0, n_w, T_long, H_long, W_long, T, H, Wd))
        return DC_ERR_SHAPE;
    const int64_t total = (int64_t)B * n_w * T * H * Wd;
    if ((int64_t)T * H * Wd > INT32_MAX || total > INT32_MAX || (int64_t)T_long * H_long * W_long > INT32_MAX)
        return DC_ERR_SHAPE;
    hipLaunchKernelGGL(pack_latent_tiles_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_,
                       x, cc, out, box, step_index, index, S, W, w0, n_w, B, Cx, Cc, T_long, H_long, W_long, T, H, Wd, c_pad,
                       nrep);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_tile_merge(const float* e, int ld_e, float* out, int ld_out, const int32_t* box, const float* g,
                             const int32_t* step_index, int index, int S, int W, int w0, int n_w, int nb, int B, int C,
                             int T_long, int H_long, int W_long, int T, int H, int Wd, int accumulate, void* stream_) {
    if (!e || !out || !box || !g) return DC_ERR_ARG;
    if (nb < 1 || B < 1 || C < 1 || ld_e < C || ld_out < C ||
        !tile_geometry_ok(step_index, index, S, W, w0, n_w, T_long, H_long, W_long, T, H, Wd))
        return DC_ERR_SHAPE;
    const int64_t total = (int64_t)nb * B * T_long * H_long * W_long;
    if ((int64_t)T_long * H_long * W_long > INT32_MAX || total > INT32_MAX ||
        (int64_t)T * H * Wd > INT32_MAX || (int64_t)nb * B * n_w * T * H * Wd > INT32_MAX)
        return DC_ERR_SHAPE;
    const bool vec = C == 4 && ld_e % 4 == 0 && ld_out % 4 == 0 && ((uintptr_t)e % 16) == 0 && ((uintptr_t)out % 16) == 0;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(tile_merge_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream_, e, ld_e, out, ld_out, box, g,
                           step_index, index, S, W, w0, n_w, nb * B, C, T_long, H_long, W_long, T, H, Wd, accumulate);
    else
        hipLaunchKernelGGL(tile_merge_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream_, e, ld_e, out, ld_out, box, g,
                           step_index, index, S, W, w0, n_w, nb * B, C, T_long, H_long, W_long, T, H, Wd, accumulate);
    DC_CHECK_LAUNCH();
    return 0;
}
