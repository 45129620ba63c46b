// Baseline JPEG (ITU-T T.81 sequential DCT, SOF0) encoder for the output side of the harness: display frames uint8
// [T][H][W][3] (what dc_frames_to_u8 writes) -> the entropy-coded scan of every frame, ready to be wrapped in JFIF headers
// and an AVI container on the host (utils/save_video.py). 8-bit YCbCr 4:2:0: an MCU is 16x16 pixels and holds the blocks
// Y00 Y01 Y10 Y11 Cb Cr; Annex K Huffman tables; a restart interval of `ri` MCUs makes every segment of the bitstream
// independent, so entropy coding runs one wave per segment. Three stages, three entries:
//   dc_jpeg_dct_quant  colour transform, chroma mean, DCT, quantisation   (one workgroup per MCU)
//   dc_jpeg_entropy    Huffman coding of one restart segment per wave into a worst-case-sized scratch row
//   dc_jpeg_pack       exclusive scan of the segment lengths + gather into one contiguous scan per frame, RSTm between
// gfx950 only (wave64: one 8x8 block is one wave, a lane per coefficient).
#include "dc_common.h"
#include "dcrafter_hip.h"
#include "jpeg_tables.h"
#include "stream_pack.h"

namespace {

using dc_jpeg::kDct;          // jpeg_tables.h: shared with the decoder (jpeg_decode.hip)
using dc_jpeg::kZigzag;

// ---------------------------------------------------------------------------------------------- stage 1: coefficients
// One workgroup per MCU, one thread per pixel. All arithmetic fp32: Y/Cb/Cr per pixel, chroma = mean of its 2x2 pixels, level
// shift, separable DCT through LDS (rows, then columns), true division by the table entry, round half away from zero, AC clamped
// to +-1023. Pixels beyond the frame replicate its last row / column. Each pixel is read once; the 384 coefficients of the MCU
// leave as one contiguous 768-byte run.
__global__ __launch_bounds__(256) void jpeg_dct_quant_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ qtab,
                                                             int16_t* __restrict__ coef, int H, int W, int my, int mx) {
    __shared__ float s[6][8][9];           // level-shifted samples [block][y][x]
    __shared__ float tmp[6][8][9];         // after the row pass [block][y][u]
    __shared__ float chroma[2][16][17];    // per-pixel Cb, Cr
    __shared__ float dct[64];
    __shared__ float qf[2][64];
    __shared__ uint8_t zz[64];
    const int tid = threadIdx.x;
    const int64_t mcu = blockIdx.x;
    const int mxi = (int)(mcu % mx);
    const int64_t r = mcu / mx;
    const int myi = (int)(r % my), t = (int)(r / my);
    if (tid < 64) { dct[tid] = kDct[tid]; zz[tid] = kZigzag[tid]; }
    if (tid < 128) qf[tid >> 6][tid & 63] = (float)qtab[tid];
    const int py = tid >> 4, px = tid & 15;
    const int y = min(myi * 16 + py, H - 1), x = min(mxi * 16 + px, W - 1);
    const uint8_t* p = frames + (((int64_t)t * H + y) * W + x) * 3;
    const float R = (float)p[0], G = (float)p[1], B = (float)p[2];
    s[(py >> 3) * 2 + (px >> 3)][py & 7][px & 7] = (0.299f * R + 0.587f * G + 0.114f * B) - 128.0f;
    chroma[0][py][px] = -0.168735892f * R - 0.331264108f * G + 0.5f * B + 128.0f;
    chroma[1][py][px] = 0.5f * R - 0.418687589f * G - 0.081312411f * B + 128.0f;
    __syncthreads();
    if (tid < 128) {
        const int c = tid >> 6, cy = (tid >> 3) & 7, cx = tid & 7;
        const float m = (chroma[c][2 * cy][2 * cx] + chroma[c][2 * cy][2 * cx + 1] + chroma[c][2 * cy + 1][2 * cx]
                         + chroma[c][2 * cy + 1][2 * cx + 1]) * 0.25f;
        s[4 + c][cy][cx] = m - 128.0f;
    }
    __syncthreads();
    for (int i = tid; i < 384; i += 256) {                       // rows: tmp[b][y][u] = sum_x s[b][y][x] D[u][x]
        const int b = i >> 6, yy = (i >> 3) & 7, u = i & 7;
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += s[b][yy][k] * dct[u * 8 + k];
        tmp[b][yy][u] = acc;
    }
    __syncthreads();
    for (int i = tid; i < 384; i += 256) {                       // columns, quantisation, zigzag order
        const int b = i >> 6, k = i & 63;
        const int nat = zz[k], v = nat >> 3, u = nat & 7;
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += dct[v * 8 + j] * tmp[b][j][u];
        const float xq = __fdiv_rn(acc, qf[b >= 4 ? 1 : 0][k]);
        float q = copysignf(floorf(fabsf(xq) + 0.5f), xq);
        if (k) q = fminf(fmaxf(q, -1023.0f), 1023.0f);
        coef[(mcu * 6 + b) * 64 + k] = (int16_t)q;
    }
}

// ---------------------------------------------------------------------------------------------- stage 2: entropy coding
// Annex K.3 - K.6 Huffman tables (BITS = codes per length 1..16, HUFFVAL = symbols in code order)
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// symbol -> (code length << 16 | code), canonical codes of T.81 Annex C; [0]: luminance, [1]: chrominance
struct HuffTables {
    uint32_t ac[2][256];
    uint32_t dc[2][12];
};
constexpr int kHuffWords = 2 * 256 + 2 * 12;

constexpr HuffTables make_huff_tables() {
    HuffTables h{};
    for (int t = 0; t < 2; ++t) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kDcBits[t][len - 1]; ++i) h.dc[t][k++] = ((uint32_t)len << 16) | code++;    // HUFFVAL = 0..11
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kAcBits[t][len - 1]; ++i) h.ac[t][kAcVals[t][k++]] = ((uint32_t)len << 16) | code++;
            code <<= 1;
        }
    }
    return h;
}
__device__ const HuffTables kHuff = make_huff_tables();

// One wave per restart segment, a lane per coefficient. Per 8x8 block: a ballot of the non-zero AC coefficients gives each
// lane its zero run (the distance to the previous non-zero lane); a lane with a non-zero coefficient builds up to three ZRL
// codes, its run/size code and the amplitude bits in one 64-bit word (at most 3 x 11 + 16 + 10 = 59 bits), lane 0 does the same
// for the DC difference (at most 22 bits), lane 63 emits EOB when the block ends in zeros. A wave prefix sum of the bit counts
// places every lane's bits, which are ORed MSB-first into a 64-word LDS window (a block is at most 1660 bits behind at most 7
// carried ones). Each lane then owns one word of the window: it counts its complete bytes and the 0x00 each 0xFF drags along, a
// second prefix sum gives the byte offsets, and the bytes leave with ordinary byte stores. The incomplete last byte is carried
// into the next block's window; at the end of the segment it is padded with 1-bits. DC prediction starts from 0 per segment.
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, uint8_t* __restrict__ scratch,
                                                          int32_t* __restrict__ seg_len, int nmcu, int ri, int spf,
                                                          int64_t stride) {
    __shared__ uint32_t huff[kHuffWords];
    __shared__ uint32_t win[64];
    const int lane = threadIdx.x;
    const int64_t seg = blockIdx.x;
    const int f = (int)(seg / spf), sg = (int)(seg % spf);
    {
        const uint32_t* src = (const uint32_t*)&kHuff;
        for (int i = lane; i < kHuffWords; i += 64) huff[i] = src[i];
    }
    win[lane] = 0;
    __syncthreads();
    const int m0 = sg * ri, m1 = min(nmcu, m0 + ri);
    const int nblk = (m1 - m0) * 6;
    const int16_t* cp = coef + ((int64_t)f * nmcu + m0) * 384;
    uint8_t* out = scratch + seg * stride;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    int outpos = 0, carry = 0;                                   // bytes written; bits (< 8) carried in win[0]
    int nxt = cp[lane];
    for (int blk = 0; blk < nblk; ++blk) {
        // the ranges stage 1 guarantees (DC -1024..1016, AC +-1023), enforced: the window and the stride bound rest on them
        const int cur = lane == 0 ? min(max(nxt, -1024), 1023) : min(max(nxt, -1023), 1023);
        if (blk + 1 < nblk) nxt = cp[(int64_t)(blk + 1) * 64 + lane];
        const int b6 = blk % 6;
        const int comp = b6 < 4 ? 0 : b6 - 3, tc = comp ? 1 : 0;
        const int dcv = __shfl(cur, 0, 64);
        const int pred = comp == 0 ? pred0 : comp == 1 ? pred1 : pred2;
        if (comp == 0) pred0 = dcv; else if (comp == 1) pred1 = dcv; else pred2 = dcv;
        const int v = lane == 0 ? dcv - pred : cur;
        const int size = 32 - __clz(abs(v));                     // 0 for v = 0
        const uint32_t amp = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
        const unsigned long long nz = __ballot(lane > 0 && cur != 0);
        unsigned long long bits = 0;
        int n = 0;
        if (lane == 0) {
            const uint32_t e = huff[512 + tc * 12 + size];
            n = (int)(e >> 16) + size;
            bits = ((unsigned long long)(e & 0xffffu) << size) | amp;
        } else if (cur != 0) {
            const unsigned long long below = nz & ((1ull << lane) - 1ull);
            const int prev = below ? 63 - __clzll((long long)below) : 0;
            const int run = lane - prev - 1;
            const uint32_t zrl = huff[tc * 256 + 0xF0];
            for (int i = 0; i < (run >> 4); ++i) {
                bits = (bits << (zrl >> 16)) | (zrl & 0xffffu);
                n += (int)(zrl >> 16);
            }
            const uint32_t e = huff[tc * 256 + (((run & 15) << 4) | size)];
            bits = (((bits << (e >> 16)) | (e & 0xffffu)) << size) | amp;
            n += (int)(e >> 16) + size;
        } else if (lane == 63) {                                 // the block ends in zeros: EOB
            const uint32_t e = huff[tc * 256];
            bits = e & 0xffffu;
            n = (int)(e >> 16);
        }
        int blockbits;
        const int p = carry + wave_excl_scan(n, lane, blockbits);
        if (n) {
            const int end = p + n;
            for (int w = p >> 5; w * 32 < end; ++w) {            // at most 3 words
                const int sh = end - (w + 1) * 32;               // value bits to the right of this word
                const uint32_t part = sh >= 0 ? (uint32_t)(bits >> sh) : (uint32_t)(bits << -sh);
                atomicOr(&win[w], part);
            }
        }
        __syncthreads();
        const int total = carry + blockbits;                     // <= 7 + 1660: at most word 52 of the window
        const int nB = total >> 3;
        const uint32_t word = win[lane];
        uint8_t by[4];
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            by[i] = (uint8_t)(word >> (24 - 8 * i));
            if (4 * lane + i < nB) cnt += by[i] == 0xFF ? 2 : 1;
        }
        int nbytes;
        int64_t o = outpos + wave_excl_scan(cnt, lane, nbytes);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (4 * lane + i < nB) {
                if (o < stride) out[o] = by[i];
                ++o;
                if (by[i] == 0xFF) {
                    if (o < stride) out[o] = 0;
                    ++o;
                }
            }
        }
        const uint32_t cbyte = (win[nB >> 2] >> (24 - 8 * (nB & 3))) & 0xFFu;       // the incomplete byte (same word for all lanes)
        __syncthreads();
        win[lane] = lane == 0 ? cbyte << 24 : 0u;
        __syncthreads();
        outpos += nbytes;
        carry = total & 7;
    }
    if (lane == 0) {
        if (carry) {                                             // pad the last byte with 1-bits
            const uint32_t b = (win[0] >> 24) | (0xFFu >> carry);
            if (outpos < stride) out[outpos] = (uint8_t)b;
            ++outpos;
            if (b == 0xFFu) {
                if (outpos < stride) out[outpos] = 0;
                ++outpos;
            }
        }
        seg_len[seg] = outpos;
    }
}

// ---------------------------------------------------------------------------------------------- stage 3: pack
// Exclusive scan of one frame's segment lengths (each but the last followed by a 2-byte RSTm): seg_off[s] = where segment s
// starts in the frame's scan, frame_len = the scan's length. One workgroup per frame (stream_pack.h).
__global__ __launch_bounds__(256) void jpeg_scan_kernel(const int32_t* __restrict__ seg_len, int32_t* __restrict__ seg_off,
                                                        int32_t* __restrict__ frame_len, int spf) {
    const int64_t f0 = (int64_t)blockIdx.x * spf;
    const int total = frame_excl_scan(spf, 0, seg_off + f0, [&](int s) { return seg_len[f0 + s] + (s + 1 < spf ? 2 : 0); });
    if (threadIdx.x == 0) frame_len[blockIdx.x] = total;
}

// Gather: segment s of frame f -> out[f][seg_off ..], then FF D0+(s mod 8) unless it is the frame's last. Bytes that would
// fall beyond frame_stride are dropped (frame_len still reports the full length, so the host can tell and size the row anew).
__global__ __launch_bounds__(256) void jpeg_gather_kernel(const uint8_t* __restrict__ scratch, const int32_t* __restrict__ seg_len,
                                                          const int32_t* __restrict__ seg_off, uint8_t* __restrict__ out, int spf,
                                                          int64_t stride, int64_t frame_stride) {
    const int s = blockIdx.x, f = blockIdx.y;
    const int64_t seg = (int64_t)f * spf + s;
    const int len = seg_len[seg];
    const int64_t off = seg_off[seg];
    uint8_t* dst = out + (int64_t)f * frame_stride;
    pack_copy_chunk(scratch + seg * stride, len, dst, off, frame_stride);
    if (threadIdx.x < 2 && s + 1 < spf && off + len + threadIdx.x < frame_stride)
        dst[off + len + threadIdx.x] = threadIdx.x == 0 ? (uint8_t)0xFF : (uint8_t)(0xD0 + (s & 7));
}

}  // namespace

extern "C" int dc_jpeg_dct_quant(const uint8_t* frames, const uint8_t* qtab, int16_t* coef, int T, int H, int W, void* stream_) {
    if (!frames || !qtab || !coef) return DC_ERR_ARG;
    if (T < 1 || H < 1 || W < 1) return DC_ERR_SHAPE;
    const int my = (H + 15) / 16, mx = (W + 15) / 16;
    const int64_t nblocks = (int64_t)T * my * mx;
    if (nblocks > 0x7fffffffLL) return DC_ERR_SHAPE;
    hipLaunchKernelGGL(jpeg_dct_quant_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream_, frames, qtab, coef, H, W,
                       my, mx);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_jpeg_entropy(const int16_t* coef, uint8_t* scratch, int32_t* seg_len, int T, int my, int mx, int ri,
                               int64_t stride, void* stream_) {
    if (!coef || !scratch || !seg_len) return DC_ERR_ARG;
    if (T < 1 || my < 1 || mx < 1 || ri < 1) return DC_ERR_SHAPE;
    const int64_t nmcu = (int64_t)my * mx;
    if (nmcu > 0x7fffffffLL / 6) return DC_ERR_SHAPE;
    const int64_t per_seg = ri < nmcu ? ri : nmcu;               // MCUs the longest segment holds
    if (stride < per_seg * DC_JPEG_MCU_MAX_BYTES + 1) return DC_ERR_SHAPE;
    const int64_t spf = (nmcu + ri - 1) / ri;
    if (T * spf > 0x7fffffffLL) return DC_ERR_SHAPE;
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)(T * spf)), dim3(64), 0, (hipStream_t)stream_, coef, scratch, seg_len,
                       (int)nmcu, ri, (int)spf, stride);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_jpeg_pack(const uint8_t* scratch, const int32_t* seg_len, int32_t* seg_off, uint8_t* out, int32_t* frame_len,
                            int T, int segs_per_frame, int64_t stride, int64_t frame_stride, void* stream_) {
    if (!scratch || !seg_len || !seg_off || !out || !frame_len) return DC_ERR_ARG;
    if (T < 1 || T > 65535 || segs_per_frame < 1 || stride < 1 || frame_stride < 1) return DC_ERR_SHAPE;
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream_, seg_len, seg_off, frame_len, segs_per_frame);
    DC_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_gather_kernel, dim3(segs_per_frame, T), dim3(256), 0, (hipStream_t)stream_, scratch, seg_len, seg_off,
                       out, segs_per_frame, stride, frame_stride);
    DC_CHECK_LAUNCH();
    return 0;
}
