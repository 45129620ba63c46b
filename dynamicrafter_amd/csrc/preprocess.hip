// Input side of the harness: a decoded image uint8 [H][W][3] on the device -> the fp32 clip [3][T][Hc][Wc] in [-1, 1] that
// image_guided_synthesis takes, i.e. what the reference's loader does on the host with torchvision on a PIL image
// (scripts/evaluation/inference.py:71-76, 95-108): Resize(min(video_size)) -> CenterCrop(video_size) -> ToTensor ->
// Normalize(0.5, 0.5) -> repeat over frames. Resize on a PIL image is Pillow's Image.resize(BILINEAR): a separable triangle
// filter whose support grows with the reduction factor, in 22-bit fixed point, horizontal pass first, with a uint8 rounding
// between the passes. Integer arithmetic, so the kernels reproduce it bit for bit:
//     acc = (1 << 21) + sum_{i < n[xx]} in[xmin[xx] + i] * k[xx][i];   out = clamp(acc >> 22, 0, 255)
// The tables k / xmin / n come from the host (ops.resize_coeffs: float64, Pillow's operation order); computing them here would
// let the compiler contract a * b + c into an fma, and the last bit of a coefficient would no longer be Pillow's.
// Two entries (the float resize of the application classes, dc_resize_f32_*, follows them at the end of the file):
//   dc_prep_resize_h   horizontal pass into a uint8 intermediate, only the rows / columns the rest will read (used when a
//                      vertical pass follows)
//   dc_prep_finish     the LAST pass (horizontal, vertical, or none when the image already has the resized size) fused with the
//                      centre crop, the zero padding, v / 255, (v - 0.5) / 0.5 and the store into frames t0 .. t0 + nt - 1
// Direct version: one thread per output pixel (3 channels), lanes along x. In the vertical pass a wave reads 192 contiguous
// bytes per tap and k / ymin / n are wave-uniform; in the horizontal pass neighbouring lanes read windows 3 * scale bytes apart
// that overlap (a window is 2 * scale wide), so a row segment is fetched once and re-read from the vector L1.
#include "dc_common.h"
#include "dcrafter_hip.h"

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;         // Pillow's PRECISION_BITS for 8-bit channels

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> kPrecisionBits, 0), 255); }

// The tables are trusted (the wrapper guarantees start + n <= extent); all the same a window is cut to [0, extent) and to ksize
// taps here, once per output pixel, so that a bad table gives wrong pixels and never a read outside the operand.
__device__ __forceinline__ int taps_within(int start, int n, int ksize, int extent) {
    if (start < 0 || start >= extent) return 0;
    return min(min(n, ksize), extent - start);
}

// acc[c] = (1 << 21) + sum_i p[i * stride + c] * kk[i]
__device__ __forceinline__ void tap_sum(const uint8_t* __restrict__ p, int64_t stride, const int32_t* __restrict__ kk, int m,
                                        int& a0, int& a1, int& a2) {
    a0 = a1 = a2 = 1 << (kPrecisionBits - 1);
    for (int i = 0; i < m; ++i) {
        const int c = kk[i];
        a0 += (int)p[0] * c;
        a1 += (int)p[1] * c;
        a2 += (int)p[2] * c;
        p += stride;
    }
}

// dst[r][j][c] = the horizontal pass at source row y0 + r, resized column x0 + j
__global__ __launch_bounds__(256) void prep_resize_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            const int32_t* __restrict__ k, const int32_t* __restrict__ xmin,
                                                            const int32_t* __restrict__ n, int ksize, int W, int y0, int x0,
                                                            int rows, int cols) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)rows * cols) return;
    const int r = (int)(idx / cols), j = (int)(idx % cols);
    const int xx = x0 + j;
    const int s = xmin[xx];
    const int m = taps_within(s, n[xx], ksize, W);
    int a0, a1, a2;
    tap_sum(src + ((int64_t)(y0 + r) * W + s) * 3, 3, k + (int64_t)xx * ksize, m, a0, a1, a2);
    uint8_t* d = dst + idx * 3;
    d[0] = (uint8_t)clip8(a0);
    d[1] = (uint8_t)clip8(a1);
    d[2] = (uint8_t)clip8(a2);
}

struct FinishArgs {
    const uint8_t* src;            // [sh][sw][3]; its element (0, 0) is the pixel (sy0, sx0) of the image it is a part of
    float* clip;                   // [3][T][ch][cw]
    const int32_t *k, *kmin, *kn;  // tables of the pass (AXIS 1: per resized column, AXIS 2: per resized row)
    int ksize;
    int sh, sw, sy0, sx0;
    int rh, rw;                    // the resized image
    int yoff, xoff;                // crop pixel (oy, ox) = resized pixel (oy + yoff, ox + xoff); outside of it: padding
    int ch, cw, T, t0, nt;
};

// AXIS 0: src is (a part of) the resized image. AXIS 1: src has the resized height, the pass runs along x. AXIS 2: src has the
// resized width, the pass runs along y.
template <int AXIS>
__global__ __launch_bounds__(256) void prep_finish_kernel(const FinishArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)a.ch * a.cw) return;
    const int oy = (int)(idx / a.cw), ox = (int)(idx % a.cw);
    const int ry = oy + a.yoff, rx = ox + a.xoff;
    int u0 = 0, u1 = 0, u2 = 0;                                 // the padding is uint8 0
    if (ry >= 0 && ry < a.rh && rx >= 0 && rx < a.rw) {
        if (AXIS == 0) {
            const uint8_t* p = a.src + ((int64_t)(ry - a.sy0) * a.sw + (rx - a.sx0)) * 3;
            u0 = p[0]; u1 = p[1]; u2 = p[2];
        } else {
            const int o = AXIS == 1 ? rx : ry;
            const int s = a.kmin[o] - (AXIS == 1 ? a.sx0 : a.sy0);
            const int m = taps_within(s, a.kn[o], a.ksize, AXIS == 1 ? a.sw : a.sh);
            const uint8_t* p = AXIS == 1 ? a.src + ((int64_t)(ry - a.sy0) * a.sw + s) * 3
                                         : a.src + ((int64_t)s * a.sw + (rx - a.sx0)) * 3;
            int a0, a1, a2;
            tap_sum(p, AXIS == 1 ? 3 : (int64_t)a.sw * 3, a.k + (int64_t)o * a.ksize, m, a0, a1, a2);
            u0 = clip8(a0); u1 = clip8(a1); u2 = clip8(a2);
        }
    }
    // ToTensor: u8 / 255; Normalize: (v - 0.5) / 0.5, each rounded to fp32 as torch does it
    const float f0 = (__fdiv_rn((float)u0, 255.0f) - 0.5f) * 2.0f;
    const float f1 = (__fdiv_rn((float)u1, 255.0f) - 0.5f) * 2.0f;
    const float f2 = (__fdiv_rn((float)u2, 255.0f) - 0.5f) * 2.0f;
    const int64_t plane = (int64_t)a.ch * a.cw;
    float* o0 = a.clip + (int64_t)a.t0 * plane + idx;
    float* o1 = o0 + (int64_t)a.T * plane;
    float* o2 = o1 + (int64_t)a.T * plane;
    for (int t = 0; t < a.nt; ++t) {
        o0[t * plane] = f0;
        o1[t * plane] = f1;
        o2[t * plane] = f2;
    }
}

inline bool blocks_for(int64_t n, unsigned& blocks) {
    const int64_t b = (n + 255) / 256;
    if (b < 1 || b > 0x7fffffffLL) return false;
    blocks = (unsigned)b;
    return true;
}

}  // namespace

extern "C" int dc_prep_resize_h(const uint8_t* src, uint8_t* dst, const int32_t* k, const int32_t* xmin, const int32_t* n,
                                int ksize, int H, int W, int out_w, int y0, int rows, int x0, int cols, void* stream_) {
    if (!src || !dst || !k || !xmin || !n) return DC_ERR_ARG;
    if (H < 1 || W < 1 || out_w < 1 || ksize < 1 || rows < 1 || cols < 1) return DC_ERR_SHAPE;
    if (y0 < 0 || (int64_t)y0 + rows > H || x0 < 0 || (int64_t)x0 + cols > out_w) return DC_ERR_SHAPE;
    unsigned blocks;
    if (!blocks_for((int64_t)rows * cols, blocks)) return DC_ERR_SHAPE;
    hipLaunchKernelGGL(prep_resize_h_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, src, dst, k, xmin, n, ksize, W, y0,
                       x0, rows, cols);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_prep_finish(const uint8_t* src, float* clip, const int32_t* k, const int32_t* kmin, const int32_t* kn,
                              int ksize, int axis, int sh, int sw, int sy0, int sx0, int rh, int rw, int yoff, int xoff, int ch,
                              int cw, int T, int t0, int nt, void* stream_) {
    if (!src || !clip) return DC_ERR_ARG;
    if (axis < 0 || axis > 2) return DC_ERR_SHAPE;
    if (axis != 0 && (!k || !kmin || !kn)) return DC_ERR_ARG;
    if (sh < 1 || sw < 1 || rh < 1 || rw < 1 || ch < 1 || cw < 1 || T < 1 || (axis != 0 && ksize < 1)) return DC_ERR_SHAPE;
    if (t0 < 0 || nt < 1 || (int64_t)t0 + nt > T || sy0 < 0 || sx0 < 0) return DC_ERR_SHAPE;
    // the resized pixels the crop keeps: rows ry0 .. ry1 - 1, columns rx0 .. rx1 - 1. Along the axis of the pass src is addressed
    // through the tables, along the other one directly: there it has to hold all of them.
    const int64_t ry0 = yoff > 0 ? yoff : 0, ry1 = (int64_t)ch + yoff < rh ? (int64_t)ch + yoff : rh;
    const int64_t rx0 = xoff > 0 ? xoff : 0, rx1 = (int64_t)cw + xoff < rw ? (int64_t)cw + xoff : rw;
    if (ry0 < ry1 && rx0 < rx1) {
        if (axis != 2 && (ry0 < sy0 || ry1 > (int64_t)sy0 + sh)) return DC_ERR_SHAPE;
        if (axis != 1 && (rx0 < sx0 || rx1 > (int64_t)sx0 + sw)) return DC_ERR_SHAPE;
    }
    unsigned blocks;
    if (!blocks_for((int64_t)ch * cw, blocks)) return DC_ERR_SHAPE;
    const FinishArgs a{src, clip, k, kmin, kn, ksize, sh, sw, sy0, sx0, rh, rw, yoff, xoff, ch, cw, T, t0, nt};
    hipStream_t stream = (hipStream_t)stream_;
    if (axis == 0) hipLaunchKernelGGL(prep_finish_kernel<0>, dim3(blocks), dim3(256), 0, stream, a);
    else if (axis == 1) hipLaunchKernelGGL(prep_finish_kernel<1>, dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(prep_finish_kernel<2>, dim3(blocks), dim3(256), 0, stream, a);
    DC_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------- float resize (the app classes)
// The programmatic entry points resize a float tensor that is already normalised to [-1, 1], not uint8 pixels: torchvision's
// Resize / CenterCrop on a tensor (scripts/gradio/i2v_test.py:39-42, 65; i2v_test_application.py:39-42, 65, 75;
// dynamicrafter_pipeline.py:281-288) is interpolate(bilinear, antialias = True) plus a crop that pads with 0.0f, and
// cv2.resize(INTER_LINEAR) on float32 (scripts/evaluation/funcs.py:196) is the same interpolation without the antialias
// support. Same structure as above - host tables (ops.resize_coeffs_f32: float weights, ATen's window rule), horizontal pass
// first into an fp32 intermediate that holds only the rows and columns the rest reads, the last pass fused with crop and
// padding - on planar fp32 [C][H][W] with any C.
// One thread per output element, lanes along x: a wave stores 256 contiguous bytes, and in the vertical pass it also reads 256
// contiguous bytes per tap with wave-uniform weights. In the horizontal pass neighbouring lanes read windows `scale` floats apart
// that overlap: the two-pass form stages the row segment and the weights of a tile of outputs in the LDS (coalesced loads; the
// direct form, which leaves the re-reads to the vector L1, measured 2.2 - 3.2x the pass's byte floor at 3000x4000 -> 576x1024). No
// vector accesses: rows start at arbitrary element offsets (W, sw, cols, xmin, xoff are free), so there are no alignment cases and
// no tails; a wave still moves whole 256-byte runs.
namespace {

// sum_i p[i * stride] * kk[i], taps in order
__device__ __forceinline__ float tap_sum_f32(const float* __restrict__ p, int64_t stride, const float* __restrict__ kk, int m) {
    float acc = 0.0f;
    for (int i = 0; i < m; ++i) {
        acc = fmaf(p[0], kk[i], acc);
        p += stride;
    }
    return acc;
}

// dst[c][r][j] = the horizontal pass at source row y0 + r, resized column x0 + j of plane c. Direct form: every lane reads
// its window and its weights from global memory (the form of a pass whose tile does not fit the LDS: seg = 0).
__global__ __launch_bounds__(256) void resize_f32_h_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           const float* __restrict__ k, const int32_t* __restrict__ xmin,
                                                           const int32_t* __restrict__ n, int ksize, int C, int H, int W, int y0,
                                                           int x0, int rows, int cols) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)C * rows * cols) return;
    const int j = (int)(idx % cols);
    const int64_t cr = idx / cols;
    const int r = (int)(cr % rows), c = (int)(cr / rows);
    const int xx = x0 + j;
    const int s = xmin[xx];
    const int m = taps_within(s, n[xx], ksize, W);
    dst[idx] = tap_sum_f32(src + ((int64_t)c * H + (y0 + r)) * W + s, 1, k + (int64_t)xx * ksize, m);
}

// The same pass staged through the LDS: a workgroup computes DC_RESIZE_F32_TILE consecutive outputs of one row. Their windows
// tile one contiguous segment of the source row (xmin and xmin + n do not decrease), which the workgroup loads once, lanes on
// consecutive floats, and their weights are one contiguous block of k: both land in the LDS (dynamic: seg floats of the row,
// then TILE * ksize weights), and the taps are read from there - the row at a lane stride of about `scale` floats, the weights
// at a lane stride of ksize floats, which is odd with antialias: no bank conflict. A window that leaves the staged segment (a bad table, or a
// seg smaller than promised) is cut to it: wrong pixels, no read outside the row or the LDS.
__global__ __launch_bounds__(DC_RESIZE_F32_TILE) void resize_f32_h_lds_kernel(
        const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ k, const int32_t* __restrict__ xmin,
        const int32_t* __restrict__ n, int ksize, int H, int W, int y0, int x0, int rows, int cols, int seg) {
    extern __shared__ float lds[];
    constexpr int TILE = DC_RESIZE_F32_TILE;
    float* row = lds;
    float* kw = lds + seg;
    const int tiles = (cols + TILE - 1) / TILE;
    const int tile = (int)(blockIdx.x % tiles);
    const int64_t cr = blockIdx.x / tiles;                       // c * rows + r
    const int r = (int)(cr % rows), c = (int)(cr / rows);
    const int j0 = tile * TILE, nj = min(TILE, cols - j0);
    const int xf = x0 + j0, xl = xf + nj - 1;                     // the first and the last output of the tile
    const int lo = min(max(xmin[xf], 0), W);
    const int hi = min(max(xmin[xl] + n[xl], lo), W);
    const int len = min(hi - lo, seg);
    const float* p = src + ((int64_t)c * H + (y0 + r)) * W + lo;
    for (int i = threadIdx.x; i < len; i += TILE) row[i] = p[i];
    const float* kt = k + (int64_t)xf * ksize;
    for (int i = threadIdx.x; i < nj * ksize; i += TILE) kw[i] = kt[i];
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= nj) return;
    const int s = xmin[xf + t] - lo;
    const int m = taps_within(s, n[xf + t], ksize, len);
    dst[cr * cols + j0 + t] = tap_sum_f32(row + s, 1, kw + t * ksize, m);
}

struct FinishF32Args {
    const float* src;              // [C][sh][sw]; its element (0, 0) of a plane is the pixel (sy0, sx0) of the image it is a part of
    float* out;                    // [C][ch][cw]
    const float* k;                // tables of the pass (AXIS 1: per resized column, AXIS 2: per resized row)
    const int32_t *kmin, *kn;
    int ksize;
    int C, sh, sw, sy0, sx0;
    int rh, rw;                    // the resized image
    int yoff, xoff;                // crop pixel (oy, ox) = resized pixel (oy + yoff, ox + xoff); outside of it: 0.0f
    int ch, cw;
};

// AXIS as in prep_finish_kernel
template <int AXIS>
__global__ __launch_bounds__(256) void resize_f32_finish_kernel(const FinishF32Args a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t plane = (int64_t)a.ch * a.cw;
    if (idx >= (int64_t)a.C * plane) return;
    const int c = (int)(idx / plane);
    const int64_t pix = idx % plane;
    const int oy = (int)(pix / a.cw), ox = (int)(pix % a.cw);
    const int ry = oy + a.yoff, rx = ox + a.xoff;
    float v = 0.0f;                                             // the padding is 0.0f: mid-grey of a [-1, 1] image
    if (ry >= 0 && ry < a.rh && rx >= 0 && rx < a.rw) {
        const float* sp = a.src + (int64_t)c * a.sh * a.sw;
        if (AXIS == 0) {
            v = sp[(int64_t)(ry - a.sy0) * a.sw + (rx - a.sx0)];
        } else {
            const int o = AXIS == 1 ? rx : ry;
            const int s = a.kmin[o] - (AXIS == 1 ? a.sx0 : a.sy0);
            const int m = taps_within(s, a.kn[o], a.ksize, AXIS == 1 ? a.sw : a.sh);
            const float* p = AXIS == 1 ? sp + (int64_t)(ry - a.sy0) * a.sw + s : sp + (int64_t)s * a.sw + (rx - a.sx0);
            v = tap_sum_f32(p, AXIS == 1 ? 1 : (int64_t)a.sw, a.k + (int64_t)o * a.ksize, m);
        }
    }
    a.out[idx] = v;
}

}  // namespace

extern "C" int dc_resize_f32_h(const float* src, float* dst, const float* k, const int32_t* xmin, const int32_t* n, int ksize,
                               int C, int H, int W, int out_w, int y0, int rows, int x0, int cols, int seg, void* stream_) {
    if (!src || !dst || !k || !xmin || !n) return DC_ERR_ARG;
    if (C < 1 || H < 1 || W < 1 || out_w < 1 || ksize < 1 || rows < 1 || cols < 1 || seg < 0) return DC_ERR_SHAPE;
    if (y0 < 0 || (int64_t)y0 + rows > H || x0 < 0 || (int64_t)x0 + cols > out_w) return DC_ERR_SHAPE;
    hipStream_t stream = (hipStream_t)stream_;
    if (seg == 0) {
        unsigned blocks;
        if (!blocks_for((int64_t)C * rows * cols, blocks)) return DC_ERR_SHAPE;
        hipLaunchKernelGGL(resize_f32_h_kernel, dim3(blocks), dim3(256), 0, stream, src, dst, k, xmin, n, ksize, C, H, W, y0, x0,
                           rows, cols);
    } else {
        const int64_t lds_bytes = DC_RESIZE_F32_LDS_BYTES(seg, ksize);
        const int64_t blocks = (int64_t)C * rows * ((cols + DC_RESIZE_F32_TILE - 1) / DC_RESIZE_F32_TILE);
        if (lds_bytes > DC_RESIZE_F32_LDS_MAX || blocks > 0x7fffffffLL) return DC_ERR_SHAPE;
        hipLaunchKernelGGL(resize_f32_h_lds_kernel, dim3((unsigned)blocks), dim3(DC_RESIZE_F32_TILE), (size_t)lds_bytes, stream,
                           src, dst, k, xmin, n, ksize, H, W, y0, x0, rows, cols, seg);
    }
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_resize_f32_finish(const float* src, float* out, const float* k, const int32_t* kmin, const int32_t* kn,
                                    int ksize, int axis, int C, int sh, int sw, int sy0, int sx0, int rh, int rw, int yoff,
                                    int xoff, int ch, int cw, void* stream_) {
    if (!src || !out) return DC_ERR_ARG;
    if (axis < 0 || axis > 2) return DC_ERR_SHAPE;
    if (axis != 0 && (!k || !kmin || !kn)) return DC_ERR_ARG;
    if (C < 1 || sh < 1 || sw < 1 || rh < 1 || rw < 1 || ch < 1 || cw < 1 || (axis != 0 && ksize < 1)) return DC_ERR_SHAPE;
    if (sy0 < 0 || sx0 < 0) return DC_ERR_SHAPE;
    // as in dc_prep_finish: along the axis of the pass src is addressed through the tables, along the other one directly
    const int64_t ry0 = yoff > 0 ? yoff : 0, ry1 = (int64_t)ch + yoff < rh ? (int64_t)ch + yoff : rh;
    const int64_t rx0 = xoff > 0 ? xoff : 0, rx1 = (int64_t)cw + xoff < rw ? (int64_t)cw + xoff : rw;
    if (ry0 < ry1 && rx0 < rx1) {
        if (axis != 2 && (ry0 < sy0 || ry1 > (int64_t)sy0 + sh)) return DC_ERR_SHAPE;
        if (axis != 1 && (rx0 < sx0 || rx1 > (int64_t)sx0 + sw)) return DC_ERR_SHAPE;
    }
    unsigned blocks;
    if (!blocks_for((int64_t)C * ch * cw, blocks)) return DC_ERR_SHAPE;
    const FinishF32Args a{src, out, k, kmin, kn, ksize, C, sh, sw, sy0, sx0, rh, rw, yoff, xoff, ch, cw};
    hipStream_t stream = (hipStream_t)stream_;
    if (axis == 0) hipLaunchKernelGGL(resize_f32_finish_kernel<0>, dim3(blocks), dim3(256), 0, stream, a);
    else if (axis == 1) hipLaunchKernelGGL(resize_f32_finish_kernel<1>, dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(resize_f32_finish_kernel<2>, dim3(blocks), dim3(256), 0, stream, a);
    DC_CHECK_LAUNCH();
    return 0;
}
