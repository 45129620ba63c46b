// Baseline JPEG (ITU-T T.81 sequential DCT, SOF0, 8-bit) decoder for the input side of the harness: the entropy-coded scans of a
// batch of frames of one geometry (utils/load_video.py cuts them out of the JFIF files of a Motion-JPEG AVI) -> display frames
// uint8 [T][h][w][3] or fp32 planes [T][3][h][w]. The inverse of jpeg.hip. One component (grey) or three (YCbCr) with luma
// sampling 1x1, 2x1 or 2x2 and chroma 1x1; quantisation and Huffman tables come from the file, per frame. Three stages:
//   dc_jpeg_decode_entropy   Huffman decoding, one lane per restart segment (or per whole scan without DRI) -> coefficients
//   dc_jpeg_decode_idct      dequantisation + inverse DCT -> 8-bit sample planes padded to whole MCUs (one wave per block)
//   dc_jpeg_decode_output    "fancy" chroma upsampling + YCbCr -> RGB -> the output tensor (one thread per pixel)
// gfx950 only (wave64: one 8x8 block is one wave, a lane per sample).
#include "dc_common.h"
#include "dcrafter_hip.h"
#include "jpeg_tables.h"

namespace {

using dc_jpeg::kDct;
using dc_jpeg::kZigzag;

// the per-frame table block (DC_JPEG_FRAME_TAB_BYTES): 4 Huffman tables (DC0 DC1 AC0 AC1, each BITS[16] HUFFVAL[256]), 4
// quantisation tables of 64 bytes in zigzag order, per component its Huffman selectors (Td | Ta << 4) and its Tq
constexpr int kHuffBytes = 272, kQuantAt = 4 * kHuffBytes, kSelAt = kQuantAt + 4 * 64, kTqAt = kSelAt + 3;
static_assert(kTqAt + 3 <= DC_JPEG_FRAME_TAB_BYTES, "frame table block");

// ---------------------------------------------------------------------------------------------- stage 1: entropy decoding
constexpr int kLutBits = 9;

// The bits of one segment, MSB first. Only bytes [0, len) of the segment are ever read; FF 00 is one FF; past the end (and from
// an FF that is not followed by 00 on: a marker has no business inside a segment) the bits read as 1s, as T.81 pads. `pad` counts
// the 1s fed that way, so the end of the decode can tell whether it consumed bits that were never there.
struct SegBits {
    const uint8_t* p;
    int len, pos, n, pad;                  // n: valid bits, the low ones of acc
    unsigned long long acc;
    bool stop;
    __device__ __forceinline__ void fill() {                     // afterwards n >= 57
        while (n <= 56) {
            uint32_t b = 0xFF;
            bool real = false;
            if (!stop) {
                if (pos < len) {
                    b = p[pos];
                    if (b != 0xFF) { ++pos; real = true; }
                    else if (pos + 1 < len && p[pos + 1] == 0) { pos += 2; real = true; }
                    else stop = true;
                } else {
                    stop = true;
                }
            }
            if (!real) { b = 0xFF; pad += 8; }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    __device__ __forceinline__ uint32_t peek16() const { return (uint32_t)(acc >> (n - 16)) & 0xFFFFu; }
    __device__ __forceinline__ uint32_t get(int s) {             // s in 0..16
        n -= s;
        return (uint32_t)(acc >> n) & ((1u << s) - 1u);
    }
};

struct HuffLds {
    uint16_t lut[4][1 << kLutBits];        // next kLutBits bits -> length << 8 | symbol; 0: a longer code, or none
    int32_t maxcode[4][17];                // [length 1..16]: the largest code of that length, -1 if there is none (T.81 F.2.2.3)
    int32_t valoff[4][17];                 // VALPTR - MINCODE: HUFFVAL index = valoff + code
    uint8_t vals[4][256];
    uint8_t sel[8];                        // Td | Ta << 4 per component
};

// the symbol of the next code of table `t`, or -1 when the next 16 bits start no code of it; consumes the code
__device__ __forceinline__ int huff_decode(const HuffLds& h, int t, SegBits& br) {
    const uint32_t v = br.peek16();
    const uint32_t e = h.lut[t][v >> (16 - kLutBits)];
    if (e) {
        br.n -= (int)(e >> 8);
        return (int)(e & 0xFF);
    }
    for (int l = kLutBits + 1; l <= 16; ++l) {
        const int code = (int)(v >> (16 - l));
        if (code <= h.maxcode[t][l]) {
            const int idx = h.valoff[t][l] + code;
            if (idx < 0 || idx > 255) return -1;                 // a table that is no prefix code
            br.n -= l;
            return h.vals[t][idx];
        }
    }
    return -1;
}

// T.81 F.2.2.1 EXTEND: the s-bit amplitude -> the signed value
__device__ __forceinline__ int extend(uint32_t v, int s) { return s && v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// One lane per segment; the workgroup (one wave) takes 64 consecutive segments of ONE frame, whose four Huffman tables it
// expands into LDS first. The coefficient buffer was zeroed by the entry; only non-zero values are stored. Every loop is
// bounded by the segment's MCU count x blocks x 64 coefficients whatever the bytes are; a lane that meets an error records it
// in status[seg] and stops.
__global__ __launch_bounds__(64) void jpeg_decode_entropy_kernel(const uint8_t* __restrict__ scan, int64_t scan_bytes,
                                                                 const int32_t* __restrict__ seg, const int32_t* __restrict__ frame_seg,
                                                                 const uint8_t* __restrict__ ftab, int16_t* __restrict__ coef,
                                                                 int32_t* __restrict__ status, int nseg, int nmcu, int ny,
                                                                 int bpm) {
    __shared__ HuffLds h;
    const int lane = threadIdx.x, f = blockIdx.y;
    const int s0 = max(frame_seg[f], 0), s1 = min(frame_seg[f + 1], nseg);
    if (s0 + (int)blockIdx.x * 64 >= s1) return;                 // the whole workgroup: this frame has fewer segments
    const uint8_t* ft = ftab + (int64_t)f * DC_JPEG_FRAME_TAB_BYTES;
    for (int i = lane; i < 4 * 256; i += 64) h.vals[i >> 8][i & 255] = ft[(i >> 8) * kHuffBytes + 16 + (i & 255)];
    if (lane < 3) h.sel[lane] = ft[kSelAt + lane];
    if (lane < 4) {
        int code = 0, k = 0;
        h.maxcode[lane][0] = -1;
        h.valoff[lane][0] = 0;
        for (int l = 1; l <= 16; ++l) {
            const int n = ft[lane * kHuffBytes + l - 1];
            h.valoff[lane][l] = k - code;
            h.maxcode[lane][l] = n ? code + n - 1 : -1;
            code = (code + n) << 1;
            k += n;
        }
    }
    __syncthreads();
    for (int i = lane; i < 4 << kLutBits; i += 64) {
        const int t = i >> kLutBits, v = i & ((1 << kLutBits) - 1);
        uint32_t e = 0;
        for (int l = 1; l <= kLutBits; ++l) {
            const int code = v >> (kLutBits - l);
            if (code <= h.maxcode[t][l]) {
                const int idx = h.valoff[t][l] + code;
                if (idx >= 0 && idx <= 255) e = ((uint32_t)l << 8) | h.vals[t][idx];
                break;
            }
        }
        h.lut[t][v] = (uint16_t)e;
    }
    __syncthreads();
    const int s = s0 + (int)blockIdx.x * 64 + lane;
    if (s >= s1) return;
    const int32_t* d = seg + (int64_t)s * 5;
    const int64_t off = d[0];
    const int len = d[1], mcu0 = d[2], cnt = d[3];
    if (off < 0 || len < 0 || off + len > scan_bytes || mcu0 < 0 || cnt < 0 || (int64_t)mcu0 + cnt > nmcu || d[4] != f) {
        status[s] = DC_JPEG_ST_DESCRIPTOR;
        return;
    }
    SegBits br;
    br.p = scan + off; br.len = len; br.pos = 0; br.n = 0; br.pad = 0; br.acc = 0; br.stop = false;
    int pred0 = 0, pred1 = 0, pred2 = 0, st = 0;
    for (int m = 0; m < cnt && !st; ++m) {
        int16_t* cm = coef + ((int64_t)f * nmcu + mcu0 + m) * bpm * 64;
        for (int b = 0; b < bpm && !st; ++b) {
            const int comp = b < ny ? 0 : b - ny + 1;
            const int sel = h.sel[comp], td = sel & 1, ta = 2 + ((sel >> 4) & 1);
            int16_t* cb = cm + b * 64;
            br.fill();
            int sym = huff_decode(h, td, br);
            if (sym < 0) { st = DC_JPEG_ST_CODE; break; }
            if (sym > 11) { st = DC_JPEG_ST_CATEGORY; break; }
            const int diff = extend(br.get(sym), sym);
            int pred = comp == 0 ? pred0 : comp == 1 ? pred1 : pred2;
            pred += diff;
            if (comp == 0) pred0 = pred; else if (comp == 1) pred1 = pred; else pred2 = pred;
            if (pred) cb[0] = (int16_t)pred;
            int k = 1;
            while (k < 64) {
                br.fill();
                sym = huff_decode(h, ta, br);
                if (sym < 0) { st = DC_JPEG_ST_CODE; break; }
                const int r = sym >> 4, sz = sym & 15;
                if (sz == 0) {
                    if (r == 0) break;                           // EOB
                    if (r != 15) { st = DC_JPEG_ST_CODE; break; }            // EOBn belongs to progressive scans
                    k += 16;                                     // ZRL
                    if (k > 64) { st = DC_JPEG_ST_RUN; break; }
                    continue;
                }
                if (sz > 10) { st = DC_JPEG_ST_CATEGORY; break; }
                k += r;
                if (k > 63) { st = DC_JPEG_ST_RUN; break; }
                cb[k] = (int16_t)extend(br.get(sz), sz);         // never 0: sz >= 1
                ++k;
            }
        }
    }
    if (!st) {
        if (br.n < br.pad) st = DC_JPEG_ST_MISSING;              // bits were consumed that the segment does not hold
        else if (br.pos < br.len || br.n - br.pad >= 8) st = DC_JPEG_ST_LEFTOVER;
    }
    status[s] = st;
}

// ---------------------------------------------------------------------------------------------- stage 2: dequantise + IDCT
// One wave per 8x8 block, a lane per coefficient / sample, four blocks per workgroup. fp32: F = coef x q at its natural place,
// rows then columns through LDS with the orthonormal matrix (s[y][x] = sum_v sum_u D[v][y] F[v][u] D[u][x]), + 128,
// floor(v + 0.5), clamp to 0..255. Planes of a frame: Y [my 8 vs][mx 8 hs], then Cb and Cr [my 8][mx 8] each.
__global__ __launch_bounds__(256) void jpeg_decode_idct_kernel(const int16_t* __restrict__ coef, const uint8_t* __restrict__ ftab,
                                                               uint8_t* __restrict__ planes, int64_t nblocks, int my, int mx,
                                                               int hs, int vs, int bpm) {
    __shared__ float F[4][8][9];
    __shared__ float tmp[4][8][9];
    __shared__ float dct[64];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    if (tid < 64) dct[tid] = kDct[tid];
    const int64_t blk = (int64_t)blockIdx.x * 4 + wv;
    const bool live = blk < nblocks;
    const int ny = hs * vs, nmcu = my * mx;
    const int b = (int)(blk % bpm);
    const int64_t mcu = blk / bpm;
    const int mi = (int)(mcu % nmcu), f = (int)(mcu / nmcu);
    const int comp = b < ny ? 0 : b - ny + 1;
    if (live) {
        const uint8_t* ft = ftab + (int64_t)f * DC_JPEG_FRAME_TAB_BYTES;
        const int tq = ft[kTqAt + comp] & 3;
        const int nat = kZigzag[lane];
        F[wv][nat >> 3][nat & 7] = (float)coef[blk * 64 + lane] * (float)ft[kQuantAt + tq * 64 + lane];
    }
    __syncthreads();
    const int r = lane >> 3, c = lane & 7;
    if (live) {                                                  // rows: tmp[v][x] = sum_u F[v][u] D[u][x]
        float acc = 0.0f;
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += F[wv][r][u] * dct[u * 8 + c];
        tmp[wv][r][c] = acc;
    }
    __syncthreads();
    if (live) {                                                  // columns: s[y][x] = sum_v D[v][y] tmp[v][x]
        float acc = 0.0f;
#pragma unroll
        for (int v = 0; v < 8; ++v) acc += dct[v * 8 + r] * tmp[wv][v][c];
        const float px = fminf(fmaxf(floorf(acc + 128.0f + 0.5f), 0.0f), 255.0f);
        const int myi = mi / mx, mxi = mi % mx;
        const int64_t ysz = (int64_t)my * 8 * vs * mx * 8 * hs, csz = (int64_t)my * 8 * mx * 8;
        uint8_t* fp = planes + (int64_t)f * (ysz + (bpm > ny ? 2 * csz : 0));
        if (comp == 0) {
            const int by = b / hs, bx = b % hs;
            fp[((int64_t)(myi * vs + by) * 8 + r) * (mx * 8 * hs) + (mxi * hs + bx) * 8 + c] = (uint8_t)px;
        } else {
            fp[ysz + (comp - 1) * csz + ((int64_t)myi * 8 + r) * (mx * 8) + mxi * 8 + c] = (uint8_t)px;
        }
    }
}

// ---------------------------------------------------------------------------------------------- stage 3: upsample + colour
// One thread per output pixel. Per doubled axis the chroma sample the pixel lies in gets 3/4 and its neighbour on the pixel's
// side 1/4 (libjpeg's "fancy" triangle filter, in fp32 without its intermediate integer roundings); neighbours beyond the
// ceil(h / vs) x ceil(w / hs) real chroma samples replicate the edge, so MCU padding is never read.
template <bool PLANAR>
__global__ __launch_bounds__(256) void jpeg_decode_output_kernel(const uint8_t* __restrict__ planes, void* __restrict__ out_, int T,
                                                                 int h, int w, int my, int mx, int hs, int vs, int ncomp) {
    const int64_t hw = (int64_t)h * w;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)T * hw) return;
    const int f = (int)(i / hw);
    const int64_t p = i % hw;
    const int y = (int)(p / w), x = (int)(p % w);
    const int yw = mx * 8 * hs, cwp = mx * 8;
    const int64_t ysz = (int64_t)my * 8 * vs * yw, csz = (int64_t)my * 8 * cwp;
    const uint8_t* fp = planes + (int64_t)f * (ysz + (ncomp == 3 ? 2 * csz : 0));
    const float Y = (float)fp[(int64_t)y * yw + x];
    float R = Y, G = Y, B = Y;
    if (ncomp == 3) {
        const int ch = (h + vs - 1) / vs, cw = (w + hs - 1) / hs;
        int x0 = x, x1 = x, y0 = y, y1 = y;                      // nearer and farther sample per axis
        float wx = 0.0f, wy = 0.0f;                              // the farther one's weight
        if (hs == 2) { x0 = x >> 1; x1 = min(max(x0 + ((x & 1) ? 1 : -1), 0), cw - 1); wx = 0.25f; }
        if (vs == 2) { y0 = y >> 1; y1 = min(max(y0 + ((y & 1) ? 1 : -1), 0), ch - 1); wy = 0.25f; }
        float cc[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint8_t* cp = fp + ysz + k * csz;
            const float near_row = (1.0f - wx) * (float)cp[(int64_t)y0 * cwp + x0] + wx * (float)cp[(int64_t)y0 * cwp + x1];
            const float far_row = (1.0f - wx) * (float)cp[(int64_t)y1 * cwp + x0] + wx * (float)cp[(int64_t)y1 * cwp + x1];
            cc[k] = (1.0f - wy) * near_row + wy * far_row - 128.0f;
        }
        R = Y + 1.402f * cc[1];
        G = Y - 0.344136286f * cc[0] - 0.714136286f * cc[1];
        B = Y + 1.772f * cc[0];
        R = fminf(fmaxf(floorf(R + 0.5f), 0.0f), 255.0f);
        G = fminf(fmaxf(floorf(G + 0.5f), 0.0f), 255.0f);
        B = fminf(fmaxf(floorf(B + 0.5f), 0.0f), 255.0f);
    }
    if (PLANAR) {
        float* o = (float*)out_ + (int64_t)f * 3 * hw + p;
        o[0] = R; o[hw] = G; o[2 * hw] = B;
    } else {
        uint8_t* o = (uint8_t*)out_ + i * 3;
        o[0] = (uint8_t)R; o[1] = (uint8_t)G; o[2] = (uint8_t)B;
    }
}

// the sampling layouts the decoder takes: grey, or YCbCr with luma 1x1, 2x1 or 2x2 over chroma 1x1
bool geometry_ok(int ncomp, int hs, int vs) {
    if (ncomp == 1) return hs == 1 && vs == 1;
    return ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
}

}  // namespace

extern "C" int dc_jpeg_decode_entropy(const uint8_t* scan, int64_t scan_bytes, const int32_t* seg, const int32_t* frame_seg,
                                      const uint8_t* ftab, int16_t* coef, int32_t* status, int n_seg, int T, int my, int mx,
                                      int ncomp, int hs, int vs, int max_segs_per_frame, void* stream_) {
    if (!scan || !seg || !frame_seg || !ftab || !coef || !status) return DC_ERR_ARG;
    if (T < 1 || T > 65535 || my < 1 || mx < 1 || scan_bytes < 1 || n_seg < 1 || max_segs_per_frame < 1 || !geometry_ok(ncomp, hs, vs))
        return DC_ERR_SHAPE;
    const int64_t nmcu = (int64_t)my * mx;
    const int ny = hs * vs, bpm = ny + (ncomp == 3 ? 2 : 0);
    if (nmcu > 0x7fffffffLL / (bpm * 64)) return DC_ERR_SHAPE;
    hipStream_t stream = (hipStream_t)stream_;
    const hipError_t e = hipMemsetAsync(coef, 0, (size_t)T * nmcu * bpm * 64 * sizeof(int16_t), stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(jpeg_decode_entropy_kernel, dim3((unsigned)((max_segs_per_frame + 63) / 64), T), dim3(64), 0, stream, scan,
                       scan_bytes, seg, frame_seg, ftab, coef, status, n_seg, (int)nmcu, ny, bpm);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_jpeg_decode_idct(const int16_t* coef, const uint8_t* ftab, uint8_t* planes, int T, int my, int mx, int ncomp,
                                   int hs, int vs, void* stream_) {
    if (!coef || !ftab || !planes) return DC_ERR_ARG;
    if (T < 1 || my < 1 || mx < 1 || !geometry_ok(ncomp, hs, vs)) return DC_ERR_SHAPE;
    const int bpm = hs * vs + (ncomp == 3 ? 2 : 0);
    const int64_t nmcu = (int64_t)my * mx;
    if (nmcu > 0x7fffffffLL / (bpm * 64)) return DC_ERR_SHAPE;
    const int64_t nblocks = (int64_t)T * nmcu * bpm;
    if ((nblocks + 3) / 4 > 0x7fffffffLL) return DC_ERR_SHAPE;
    hipLaunchKernelGGL(jpeg_decode_idct_kernel, dim3((unsigned)((nblocks + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, coef, ftab,
                       planes, nblocks, my, mx, hs, vs, bpm);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_jpeg_decode_output(const uint8_t* planes, void* out, int T, int H, int W, int ncomp, int hs, int vs, int planar,
                                     void* stream_) {
    if (!planes || !out) return DC_ERR_ARG;
    if (T < 1 || H < 1 || W < 1 || H > 65535 || W > 65535 || !geometry_ok(ncomp, hs, vs) || (planar != 0 && planar != 1))
        return DC_ERR_SHAPE;
    const int my = (H + 8 * vs - 1) / (8 * vs), mx = (W + 8 * hs - 1) / (8 * hs);
    const int64_t n = (int64_t)T * H * W, nwg = (n + 255) / 256;
    if (nwg > 0x7fffffffLL) return DC_ERR_SHAPE;
    hipStream_t stream = (hipStream_t)stream_;
    if (planar)
        hipLaunchKernelGGL(jpeg_decode_output_kernel<true>, dim3((unsigned)nwg), dim3(256), 0, stream, planes, out, T, H, W, my, mx,
                           hs, vs, ncomp);
    else
        hipLaunchKernelGGL(jpeg_decode_output_kernel<false>, dim3((unsigned)nwg), dim3(256), 0, stream, planes, out, T, H, W, my, mx,
                           hs, vs, ncomp);
    DC_CHECK_LAUNCH();
    return 0;
}
