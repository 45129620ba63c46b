// FreeU (Si et al., CVPR 2024; diffusers enable_freeu) on the skip-concat buffer of an up block, in place, for gfx950.
//
// cat rows [F*H*W][ld] bf16, channels last: columns 0..ch-1 are the decoder's h, columns ch..ch+cs-1 the skip (openaimodel3d.py
// forward_rows, cat{u}). The published skip filter is fftshift(fftn(x)) * mask -> ifftn with a 2x2 block of the mask set to s:
// at threshold 1 those are the four frequencies (ky, kx) in {-1, 0}^2, so the filter is x + (s-1) * P x with P the projection
// onto four Fourier modes. Its real part needs seven sums per (frame, channel) plane (dc_freeu_skip_stats) and a rank-7 update
// per element (dc_freeu_apply): no FFT, any H x W.
//
// Layout of every kernel: a lane owns 4 or 8 adjacent channels (one 8- or 16-byte load), 16 or 8 lanes cover a 64-channel
// group, the remaining lane bits and the waves of the workgroup take different pixels. The trig factors are tabulated once per
// workgroup in LDS per row index and per column index. No atomics: partial sums meet in LDS and in the scratch and are added in
// a fixed order, so two runs on the same input give the same bits, and no scratch needs clearing between steps.
#include "dc_common.h"
#include "dcrafter_hip.h"

#define FU_TRIG_MAX 1024          // H + W the LDS trig table holds (8 KB of float2)
#define FU_STATS_THREADS 256      // 4 waves = 16 pixel slots x 16 channel quads
#define FU_STATS_SLOTS (FU_STATS_THREADS / 16)
#define FU_SPLIT_ROWS 256         // pixels of one plane a stats workgroup takes at least: planes above it are split over
#define FU_SPLIT_MAX 8            //   up to FU_SPLIT_MAX workgroups, whose partial sums dc_freeu_apply adds in order
#define FU_APPLY_THREADS 256      // 4 waves = 32 pixel slots x 8 channel octets
#define FU_APPLY_ROWS 512         // pixels of one plane an apply workgroup takes at least (gridDim.z splits the plane)

static int fu_splits(int HW) { return HW / FU_SPLIT_ROWS < 1 ? 1 : HW / FU_SPLIT_ROWS > FU_SPLIT_MAX ? FU_SPLIT_MAX : HW / FU_SPLIT_ROWS; }

// tab[i] = (cos, sin)(2 pi i / H) for i < H, then (cos, sin)(2 pi j / W) for j < W. sincospif: exact at the multiples of 1/2
// (the Nyquist row of an even H is +-1, 0).
__device__ __forceinline__ void fu_trig_fill(float2* tab, int H, int W, int tid, int nt) {
    for (int i = tid; i < H + W; i += nt) {
        const int n = i < H ? H : W, j = i < H ? i : i - H;
        float s, c;
        sincospif(2.0f * (float)j / (float)n, &s, &c);
        tab[i] = make_float2(c, s);
    }
}

// the six trig factors of pixel p = y*W + x: cos/sin of theta_y, theta_x and theta_y + theta_x
struct FuTrig { float cy, sy, cx, sx, cxy, sxy; };
__device__ __forceinline__ FuTrig fu_trig_at(const float2* tab, int p, int H, int W) {
    const int y = p / W, x = p - y * W;
    const float2 ty = tab[y], tx = tab[H + x];
    FuTrig r;
    r.cy = ty.x; r.sy = ty.y; r.cx = tx.x; r.sx = tx.y;
    r.cxy = ty.x * tx.x - ty.y * tx.y;
    r.sxy = ty.y * tx.x + ty.x * tx.y;
    return r;
}

// grid (cs/64 [+1], F, nz). Workgroup (g, f, z), g < cs/64: the seven sums of skip channels g*64..g*64+63 of frame f over the
// z-th of nz slices of the plane -> stats[z][f][c][7] = (S0, Cy, Sy, Cx, Sx, Cxy, Sxy). A lane owns 4 channels (8-byte loads),
// 16 lanes a pixel, the 16 pixel slots of the workgroup meet in LDS and are added in slot order: a shuffle butterfly over 28
// sums per lane kept the CU's LDS crossbar busier than the loads kept HBM.
// Workgroup g == cs/64, z == 0 (launched only with hmean != NULL, FreeU version 2): min and max over the frame's H*W row
// means -> mm[f][2].
__global__ __launch_bounds__(FU_STATS_THREADS) void freeu_stats_kernel(const bf16_t* __restrict__ cat, int ld, int ch, int cs,
                                                                       int H, int W, float* __restrict__ stats,
                                                                       const float* __restrict__ hmean, float* __restrict__ mm) {
    __shared__ float2 tab[FU_TRIG_MAX];
    __shared__ float red[FU_STATS_SLOTS * 64 * 7];
    const int f = blockIdx.y, g = blockIdx.x, z = blockIdx.z, t = threadIdx.x, HW = H * W, F = gridDim.y;
    if (g == cs / 64) {
        if (z) return;
        const int wave = t >> 6, lane = t & 63;
        float lo = INFINITY, hi = -INFINITY;
        for (int p = t; p < HW; p += FU_STATS_THREADS) {
            const float v = hmean[(size_t)f * HW + p];
            lo = fminf(lo, v); hi = fmaxf(hi, v);
        }
        lo = -wave_max(-lo); hi = wave_max(hi);
        if (lane == 0) { red[wave] = lo; red[8 + wave] = hi; }
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < FU_STATS_THREADS / 64; ++w) { lo = fminf(lo, red[w]); hi = fmaxf(hi, red[8 + w]); }
            mm[2 * f] = lo; mm[2 * f + 1] = hi;
        }
        return;
    }
    fu_trig_fill(tab, H, W, t, FU_STATS_THREADS);
    __syncthreads();
    const int quad = t & 15, slot = t >> 4;
    const int chunk = (HW + (int)gridDim.z - 1) / (int)gridDim.z;
    const int p0 = z * chunk, p1 = min(HW, p0 + chunk);
    const bf16_t* base = cat + (size_t)f * HW * ld + ch + g * 64 + quad * 4;
    float a[4][7];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 7; ++k) a[j][k] = 0.f;
#pragma unroll 4
    for (int p = p0 + slot; p < p1; p += FU_STATS_SLOTS) {
        const uint2 v = *reinterpret_cast<const uint2*>(base + (size_t)p * ld);
        const FuTrig q = fu_trig_at(tab, p, H, W);
        const float e[4] = {__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                            __uint_as_float(v.y & 0xffff0000u)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j][0] += e[j];
            a[j][1] = fmaf(e[j], q.cy, a[j][1]);
            a[j][2] = fmaf(e[j], q.sy, a[j][2]);
            a[j][3] = fmaf(e[j], q.cx, a[j][3]);
            a[j][4] = fmaf(e[j], q.sx, a[j][4]);
            a[j][5] = fmaf(e[j], q.cxy, a[j][5]);
            a[j][6] = fmaf(e[j], q.sxy, a[j][6]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 7; ++k) red[(slot * 64 + quad * 4 + j) * 7 + k] = a[j][k];
    __syncthreads();
    for (int i = t; i < 64 * 7; i += FU_STATS_THREADS) {
        float v = red[i];
        for (int sl = 1; sl < FU_STATS_SLOTS; ++sl) v += red[sl * 64 * 7 + i];
        stats[(((size_t)z * F + f) * cs + g * 64) * 7 + i] = v;
    }
}

// one wave per row: hmean[row] = mean over the ch columns of h (FreeU version 2)
__global__ __launch_bounds__(256) void freeu_hmean_kernel(const bf16_t* __restrict__ cat, int ld, int ch, int64_t rows,
                                                          float* __restrict__ hmean) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const bf16_t* src = cat + (size_t)row * ld;
    float acc = 0.f;
    for (int c = lane * 8; c < ch; c += 512) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + c);
        float e[8];
        unpack_bf8(v, e);
        acc += ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
    }
    acc = wave_sum(acc);
    if (lane == 0) hmean[row] = acc / (float)ch;
}

// grid (cs/64 + ch/128, F, nz): workgroup (g, f, z) takes pixels [z*chunk, (z+1)*chunk) of frame f and
//   g < cs/64: skip channels g*64..+63:  x += (s-1)/HW * (S0 + Cy cos ty + Sy sin ty + Cx cos tx + Sx sin tx + Cxy cos(ty+tx) + Sxy sin(ty+tx))
//   else     : h channels (g - cs/64)*64..+63 of the first ch/2:  x *= b (version 1) or x *= (b-1) * mhat + 1 (version 2, hmean != NULL)
// columns ch/2..ch-1 are neither read nor written.
__global__ __launch_bounds__(FU_APPLY_THREADS) void freeu_apply_kernel(bf16_t* __restrict__ cat, int ld, int ch, int cs, int H, int W,
                                                                       const float* __restrict__ stats, int nsplit, float b,
                                                                       float s, const float* __restrict__ hmean,
                                                                       const float* __restrict__ mm) {
    __shared__ float2 tab[FU_TRIG_MAX];
    __shared__ float sst[64 * 7];
    const int f = blockIdx.y, g = blockIdx.x, t = threadIdx.x, HW = H * W;
    const int oct = t & 7, slot = t >> 3;
    const int chunk = (HW + (int)gridDim.z - 1) / (int)gridDim.z;
    const int p0 = (int)blockIdx.z * chunk, p1 = min(HW, p0 + chunk);
    bf16_t* frame = cat + (size_t)f * HW * ld;
    if (g < cs / 64) {
        fu_trig_fill(tab, H, W, t, FU_APPLY_THREADS);
        const float kf = (s - 1.0f) / (float)HW;
        // the group's 64 x 7 sums: read once per workgroup (coalesced; the partial sums of the stats launch's slices added in
        // order), scaled, and handed to the lanes through LDS
        const float* sp = stats + ((size_t)f * cs + g * 64) * 7;
        const size_t zstride = (size_t)gridDim.y * cs * 7;
        for (int i = t; i < 64 * 7; i += FU_APPLY_THREADS) {
            float v = sp[i];
            for (int zz = 1; zz < nsplit; ++zz) v += sp[zz * zstride + i];
            sst[i] = kf * v;
        }
        __syncthreads();
        float st[8][7];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int k = 0; k < 7; ++k) st[j][k] = sst[(oct * 8 + j) * 7 + k];
        bf16_t* base = frame + ch + g * 64 + oct * 8;
#pragma unroll 2
        for (int p = p0 + slot; p < p1; p += FU_APPLY_THREADS / 8) {
            uint4* ptr = reinterpret_cast<uint4*>(base + (size_t)p * ld);
            const uint4 v = *ptr;
            const FuTrig q = fu_trig_at(tab, p, H, W);
            float e[8];
            unpack_bf8(v, e);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float u = st[j][0];
                u = fmaf(st[j][1], q.cy, u);
                u = fmaf(st[j][2], q.sy, u);
                u = fmaf(st[j][3], q.cx, u);
                u = fmaf(st[j][4], q.sx, u);
                u = fmaf(st[j][5], q.cxy, u);
                u = fmaf(st[j][6], q.sxy, u);
                e[j] += u;
            }
            *ptr = pack_bf8(e);
        }
        return;
    }
    bf16_t* base = frame + (g - cs / 64) * 64 + oct * 8;
    float lo = 0.f, range = 0.f;
    if (hmean) { lo = mm[2 * f]; range = mm[2 * f + 1] - lo; }
    for (int p = p0 + slot; p < p1; p += FU_APPLY_THREADS / 8) {
        uint4* ptr = reinterpret_cast<uint4*>(base + (size_t)p * ld);
        const uint4 v = *ptr;
        float fac = b;
        if (hmean) {
            const float mhat = range > 0.f ? (hmean[(size_t)f * HW + p] - lo) / range : 0.f;     // a flat frame: mhat = 0
            fac = (b - 1.0f) * mhat + 1.0f;
        }
        float e[8];
        unpack_bf8(v, e);
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] *= fac;
        *ptr = pack_bf8(e);
    }
}

static int fu_check(const void* cat, int ld, int ch, int cs, int F, int H, int W) {
    if (!cat) return DC_ERR_ARG;
    if (ch < 128 || ch % 128 || cs < 64 || cs % 64 || ld < ch + cs || ld % 8 || ((uintptr_t)cat & 15)) return DC_ERR_SHAPE;
    if (F < 1 || F > 65535 || H < 1 || W < 1 || H + W > FU_TRIG_MAX) return DC_ERR_SHAPE;
    if ((int64_t)F * H * W * ld >= (1ll << 31)) return DC_ERR_SHAPE;
    return 0;
}

extern "C" int64_t dc_freeu_scratch_floats(int cs, int F, int H, int W, int version) {
    if (cs < 1 || F < 1 || H < 1 || W < 1 || version < 1 || version > 2) return DC_ERR_ARG;
    const int64_t HW = (int64_t)H * W;
    return (int64_t)fu_splits((int)(HW > (1 << 30) ? (1 << 30) : HW)) * F * cs * 7 + (version == 2 ? (int64_t)F * HW + 2 * F : 0);
}

extern "C" int dc_freeu_hmean(const uint16_t* cat, int ld, int ch, int cs, int F, int H, int W, float* hmean, void* stream_) {
    if (!hmean) return DC_ERR_ARG;
    if (int e = fu_check(cat, ld, ch, cs, F, H, W)) return e;
    const int64_t rows = (int64_t)F * H * W;
    hipLaunchKernelGGL(freeu_hmean_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, cat, ld, ch,
                       rows, hmean);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_freeu_skip_stats(const uint16_t* cat, int ld, int ch, int cs, int F, int H, int W, float* stats,
                                   const float* hmean, float* mm, void* stream_) {
    if (!stats || (hmean == nullptr) != (mm == nullptr)) return DC_ERR_ARG;
    if (int e = fu_check(cat, ld, ch, cs, F, H, W)) return e;
    hipLaunchKernelGGL(freeu_stats_kernel, dim3(cs / 64 + (hmean ? 1 : 0), F, fu_splits(H * W)), dim3(FU_STATS_THREADS), 0,
                       (hipStream_t)stream_, cat, ld, ch, cs, H, W, stats, hmean, mm);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_freeu_apply(uint16_t* cat, int ld, int ch, int cs, int F, int H, int W, const float* stats, float b, float s,
                              const float* hmean, const float* mm, void* stream_) {
    if (!stats || (hmean == nullptr) != (mm == nullptr)) return DC_ERR_ARG;
    if (int e = fu_check(cat, ld, ch, cs, F, H, W)) return e;
    const int nz = min(64, max(1, H * W / FU_APPLY_ROWS));
    hipLaunchKernelGGL(freeu_apply_kernel, dim3(cs / 64 + ch / 128, F, nz), dim3(FU_APPLY_THREADS), 0, (hipStream_t)stream_, cat,
                       ld, ch, cs, H, W, stats, fu_splits(H * W), b, s, hmean, mm);
    DC_CHECK_LAUNCH();
    return 0;
}
