// GIF89a image data for the output side of the harness: display frames uint8 [T][H][W][3] (what dc_frames_to_u8 writes) -> the
// sub-blocked LZW image data of every frame, ready to be wrapped in the GIF container on the host (utils/save_video.py). One
// global colour table per clip; no transparency, no frame differencing. LZW is serial within a stream, so a frame's raster is cut
// into chunks of `chunk` pixels that each start from the reset state (a Clear code between them): every chunk is coded on its
// own, as a restart interval is in jpeg.hip. Four stages, four entries:
//   dc_gif_histogram  15-bit colour histogram of the whole clip (the host builds the palette from it)
//   dc_gif_map        ordered dither + exact nearest palette entry, one pixel per thread, the palette in LDS
//   dc_gif_lzw        LZW coding of one chunk per wave into a worst-case-sized scratch row, lengths in bits
//   dc_gif_pack       exclusive scan of the bit lengths + shift-merge gather into sub-blocks, one run per frame
// gfx950 only (wave64).
#include "dc_common.h"
#include "dcrafter_hip.h"
#include "stream_pack.h"

namespace {

// ---------------------------------------------------------------------------------------------- stage 1: histogram
constexpr int kHistRun = 16;     // consecutive pixels per thread

__global__ __launch_bounds__(256) void gif_hist_clear_kernel(uint32_t* __restrict__ hist) {
    hist[blockIdx.x * 256 + threadIdx.x] = 0u;
}

// Each thread walks kHistRun consecutive pixels and adds a run of equal bins with one atomic: flat areas, where every pixel
// would hit the same counter, cost one atomic per run instead of one per pixel. Integer adds: the result has no order in it.
__global__ __launch_bounds__(256) void gif_hist_kernel(const uint8_t* __restrict__ frames, uint32_t* __restrict__ hist, int64_t npix) {
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * kHistRun;
    if (p0 >= npix) return;
    const int n = (int)min((int64_t)kHistRun, npix - p0);
    const uint8_t* p = frames + p0 * 3;
    int bin = -1;
    uint32_t run = 0;
    for (int i = 0; i < n; ++i) {
        const int b = ((p[3 * i] >> 3) << 10) | ((p[3 * i + 1] >> 3) << 5) | (p[3 * i + 2] >> 3);
        if (b != bin) {
            if (run) atomicAdd(&hist[bin], run);
            bin = b;
            run = 0;
        }
        ++run;
    }
    atomicAdd(&hist[bin], run);
}

// ---------------------------------------------------------------------------------------------- stage 2: palette mapping
// 8x8 Bayer matrix, values 0..63: the bits of x ^ y and y interleaved, most significant first from the lowest bit of each
__device__ __forceinline__ int bayer8(int x, int y) {
    const int q = x ^ y;
    return ((q & 1) << 5) | ((y & 1) << 4) | ((q & 2) << 2) | ((y & 2) << 1) | ((q & 4) >> 1) | ((y & 4) >> 2);
}

constexpr int kMapPix = 4;       // pixels per thread: one LDS read of a palette entry serves four distance evaluations

// All integer: c' = clamp(c + d, 0, 255) per channel with the position-only offset d, then the exact minimum of
// dr^2 + dg^2 + db^2 over the first n entries, scanned upwards with a strict comparison (ties go to the lowest index). The entry
// is the same for all lanes, so every palette read is an LDS broadcast.
__global__ __launch_bounds__(256) void gif_map_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ palette,
                                                      uint8_t* __restrict__ idx, int64_t npix, int hw, int W, int n, int dither) {
    __shared__ int4 pal[256];
    const int tid = threadIdx.x;
    if (tid < n) pal[tid] = make_int4(palette[3 * tid], palette[3 * tid + 1], palette[3 * tid + 2], 0);
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * (256 * kMapPix) + tid;
    int r[kMapPix], g[kMapPix], b[kMapPix], best[kMapPix], bi[kMapPix];
#pragma unroll
    for (int k = 0; k < kMapPix; ++k) {
        const int64_t p = min(base + k * 256, npix - 1);         // lanes beyond the clip repeat its last pixel (not stored)
        const int q = (int)(p % hw);
        const int y = q / W, x = q - y * W;
        const int d = ((2 * bayer8(x & 7, y & 7) - 63) * dither) >> 7;          // arithmetic shift: floor for negatives too
        const uint8_t* s = frames + p * 3;
        r[k] = min(max((int)s[0] + d, 0), 255);
        g[k] = min(max((int)s[1] + d, 0), 255);
        b[k] = min(max((int)s[2] + d, 0), 255);
        best[k] = 0x7fffffff;
        bi[k] = 0;
    }
    for (int e = 0; e < n; ++e) {
        const int4 c = pal[e];
#pragma unroll
        for (int k = 0; k < kMapPix; ++k) {
            const int dr = r[k] - c.x, dg = g[k] - c.y, db = b[k] - c.z;
            const int dist = dr * dr + dg * dg + db * db;
            if (dist < best[k]) { best[k] = dist; bi[k] = e; }
        }
    }
#pragma unroll
    for (int k = 0; k < kMapPix; ++k) {
        const int64_t p = base + k * 256;
        if (p < npix) idx[p] = (uint8_t)bi[k];
    }
}

// ---------------------------------------------------------------------------------------------- stage 3: LZW
constexpr int kClear = 256, kEoi = 257, kFirstCode = 258, kMaxCodes = 4096;
constexpr int kSlots = 8192;                     // open-addressed dictionary: at most 3838 of 8192 slots in use
constexpr uint32_t kEmpty = 0xFFFFFFFFu;         // no entry looks like this: code 4095 cannot have the prefix 4095
constexpr int kStage = 256;                      // pixels staged in LDS per round

// One wave per chunk. The wave stages 256 indices in LDS and clears the dictionary; lane 0 runs the (serial) greedy match:
// dictionary entry = (prefix << 8 | pixel) << 12 | code in one LDS word, multiplicative hash, linear probing. Codes are appended
// LSB first to a 64-bit accumulator that leaves in aligned 32-bit words; the tail leaves byte by byte, so nothing is written
// behind ceil(bits / 8). Every store is checked against `stride`.
// Widths: the code that follows j codes since the last reset is written at the smallest w in 9..12 with 258 + j - 1 < 2^w: what
// a decoder, which adds its entries one code later than the encoder, has arrived at by then. The encoder's `next` runs one
// ahead (258 + j after j codes), so it widens when next > 2^w; in front of the terminator no entry is added, and the same
// comparison is made with next + 1.
__global__ __launch_bounds__(64) void gif_lzw_kernel(const uint8_t* __restrict__ idx, uint8_t* __restrict__ scratch,
                                                     int32_t* __restrict__ chunk_bits, int hw, int chunk, int cpf, int64_t stride) {
    __shared__ uint32_t table[kSlots];
    __shared__ uint32_t pix[kStage / 4];
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int f = (int)(c / cpf), ci = (int)(c % cpf);
    const int p0 = ci * chunk;                                   // ci * chunk < hw <= INT_MAX
    const int n = min(chunk, hw - p0);
    const uint8_t* src = idx + (int64_t)f * hw + p0;
    uint8_t* out = scratch + c * stride;
    for (int i = lane; i < kSlots; i += 64) table[i] = kEmpty;
    // lane 0's coder state
    int prefix = src[0], next = kFirstCode, width = 9;
    unsigned long long acc = 0;
    int nacc = 0;
    int64_t wpos = 0;                                            // bytes already stored
    auto emit = [&](int code, int w) {
        acc |= (unsigned long long)code << nacc;
        nacc += w;
        if (nacc >= 32) {
            if (wpos + 4 <= stride) *(uint32_t*)(out + wpos) = (uint32_t)acc;
            wpos += 4;
            acc >>= 32;
            nacc -= 32;
        }
    };
    int pos = 1;                                                 // pixels consumed
    while (pos < n) {                                            // wave-uniform
        const int m = min(kStage, n - pos);
        __syncthreads();                                         // the previous round's reads of pix, the clear of the table
        {
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * lane + j < m) w |= (uint32_t)src[pos + 4 * lane + j] << (8 * j);
            pix[lane] = w;
        }
        __syncthreads();
        int used = m, reset = 0;
        if (lane == 0) {
            uint32_t w = 0;
            for (int i = 0; i < m; ++i) {
                if ((i & 3) == 0) w = pix[i >> 2];
                const int k = (int)(w & 0xffu);
                w >>= 8;
                const uint32_t key = ((uint32_t)prefix << 8) | (uint32_t)k;
                uint32_t h = (key * 2654435761u) >> 19;          // 13 bits
                int hit = -1;
                for (;;) {
                    const uint32_t e = table[h];
                    if (e == kEmpty) break;
                    if ((e >> 12) == key) { hit = (int)(e & 0xfffu); break; }
                    h = (h + 1) & (kSlots - 1);
                }
                if (hit >= 0) {
                    prefix = hit;
                    continue;
                }
                emit(prefix, width);
                table[h] = (key << 12) | (uint32_t)next;
                ++next;
                prefix = k;
                if (next == kMaxCodes) {                         // 4095 has been assigned: Clear at 12 bits, start over
                    emit(kClear, 12);
                    next = kFirstCode;
                    width = 9;
                    used = i + 1;
                    reset = 1;
                    break;
                }
                if (next > (1 << width)) ++width;                // next < 4096 here, so width stays <= 12
            }
        }
        used = __shfl(used, 0, 64);
        reset = __shfl(reset, 0, 64);
        pos += used;
        if (reset) {
            __syncthreads();
            for (int i = lane; i < kSlots; i += 64) table[i] = kEmpty;
        }
    }
    if (lane == 0) {
        emit(prefix, width);                                     // the last data code
        if (next + 1 > (1 << width) && width < 12) ++width;      // the entry a decoder adds behind it
        emit(ci + 1 < cpf ? kClear : kEoi, width);
        const int64_t bits = wpos * 8 + nacc;
        for (int i = 0; i * 8 < nacc; ++i) {                     // at most 4 bytes, the last one padded with zero bits
            if (wpos < stride) out[wpos] = (uint8_t)(acc >> (8 * i));
            ++wpos;
        }
        chunk_bits[c] = (int32_t)bits;
    }
}

// ---------------------------------------------------------------------------------------------- stage 4: pack
// Exclusive scan of one frame's chunk bit lengths behind the 9-bit leading Clear: chunk_off[c] = the bit at which chunk c starts
// in the frame's code stream; frame_len = data bytes + one length byte per started sub-block of 255 + the closing 00. One
// workgroup per frame (stream_pack.h). The entry has checked that a frame's worst case stays below 2^31 bits.
__global__ __launch_bounds__(256) void gif_scan_kernel(const int32_t* __restrict__ chunk_bits, int32_t* __restrict__ chunk_off,
                                                       int32_t* __restrict__ frame_len, int cpf) {
    const int64_t f0 = (int64_t)blockIdx.x * cpf;
    const int bits = frame_excl_scan(cpf, 9, chunk_off + f0, [&](int s) { return chunk_bits[f0 + s]; });
    if (threadIdx.x == 0) {
        const int nbytes = (bits + 7) >> 3;
        frame_len[blockIdx.x] = nbytes + (nbytes + 254) / 255 + 1;
    }
}

// 8 bits of a chunk's string from bit `rel` on (0 <= rel < len), zeros behind its end
__device__ __forceinline__ uint32_t chunk_byte(const uint8_t* __restrict__ row, int len, int rel) {
    const int b = rel >> 3, s = rel & 7, nb = (len + 7) >> 3;
    const uint32_t v = (uint32_t)row[b] | (b + 1 < nb ? (uint32_t)row[b + 1] << 8 : 0u);
    const int valid = min(8, len - rel);
    return (v >> s) & ((1u << valid) - 1u);
}

// Gather: one workgroup per chunk. Byte i of the frame's code stream belongs to the chunk that holds its first bit (chunk 0 also
// owns the leading Clear, code 256 at 9 bits: byte 0 = 0, bit 0 of byte 1 = 1). A chunk is at least 18 bits long, so a byte takes
// its bits from its owner and at most the one chunk behind it; behind the frame's last chunk the byte is padded with zeros.
// Byte i lands at i + i / 255 + 1; the owner of the first byte of a sub-block writes its length byte, the owner of the stream's
// last byte the closing 00. Bytes that would fall beyond frame_stride are dropped (frame_len still reports the full length).
__global__ __launch_bounds__(256) void gif_gather_kernel(const uint8_t* __restrict__ scratch, const int32_t* __restrict__ chunk_bits,
                                                         const int32_t* __restrict__ chunk_off, uint8_t* __restrict__ out, int cpf,
                                                         int64_t stride, int64_t frame_stride) {
    const int s = blockIdx.x, f = blockIdx.y;
    const int64_t c = (int64_t)f * cpf + s;
    const int len = chunk_bits[c], off = chunk_off[c];
    const int end = off + len;
    const int64_t last = c - s + cpf - 1;
    const int total = chunk_off[last] + chunk_bits[last];
    const int nbytes = (total + 7) >> 3;
    const bool tail = s + 1 == cpf;
    const int i0 = s == 0 ? 0 : (off + 7) >> 3, i1 = (end + 7) >> 3;           // for the last chunk i1 = nbytes
    const uint8_t* row = scratch + c * stride;
    const uint8_t* nrow = row + stride;
    const int nlen = tail ? 0 : chunk_bits[c + 1];
    uint8_t* dst = out + (int64_t)f * frame_stride;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const int rel = 8 * i - off;                             // >= 0 except for bytes 0 and 1 of the frame
        uint32_t v;
        int have;
        if (rel >= 0) {
            v = chunk_byte(row, len, rel);
            have = min(8, len - rel);
        } else if (i == 0) {
            v = 0;
            have = 8;
        } else {                                                 // i == 1: the Clear's top bit, then 7 bits of chunk 0
            v = 1u | ((chunk_byte(row, len, 0) & 0x7fu) << 1);
            have = 8;
        }
        if (have < 8 && !tail) v |= (chunk_byte(nrow, nlen, 0) << have) & 0xffu;
        const int64_t o = (int64_t)i + i / 255 + 1;
        if (o < frame_stride) dst[o] = (uint8_t)v;
        if (i % 255 == 0 && o - 1 < frame_stride) dst[o - 1] = (uint8_t)min(255, nbytes - i);
        if (i == nbytes - 1 && o + 1 < frame_stride) dst[o + 1] = 0;
    }
}

}  // namespace

extern "C" int dc_gif_histogram(const uint8_t* frames, uint32_t* hist, int T, int H, int W, void* stream_) {
    if (!frames || !hist) return DC_ERR_ARG;
    if (T < 1 || H < 1 || W < 1) return DC_ERR_SHAPE;
    const int64_t npix = (int64_t)T * H * W;
    if (npix > 0xffffffffLL) return DC_ERR_SHAPE;                // a counter is 32 bits
    const int64_t nblocks = (npix + 256 * kHistRun - 1) / (256 * kHistRun);
    hipLaunchKernelGGL(gif_hist_clear_kernel, dim3(DC_GIF_HIST_BINS / 256), dim3(256), 0, (hipStream_t)stream_, hist);
    DC_CHECK_LAUNCH();
    hipLaunchKernelGGL(gif_hist_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream_, frames, hist, npix);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_gif_map(const uint8_t* frames, const uint8_t* palette, uint8_t* idx, int T, int H, int W, int n, int dither,
                          void* stream_) {
    if (!frames || !palette || !idx) return DC_ERR_ARG;
    if (T < 1 || H < 1 || W < 1 || n < 1 || n > 256 || dither < 0 || dither > 64) return DC_ERR_SHAPE;
    if ((int64_t)H * W > 0x7fffffffLL) return DC_ERR_SHAPE;
    const int64_t npix = (int64_t)T * H * W;
    const int64_t nblocks = (npix + 256 * kMapPix - 1) / (256 * kMapPix);
    if (nblocks > 0x7fffffffLL) return DC_ERR_SHAPE;
    hipLaunchKernelGGL(gif_map_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream_, frames, palette, idx, npix,
                       H * W, W, n, dither);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_gif_lzw(const uint8_t* idx, uint8_t* scratch, int32_t* chunk_bits, int T, int hw, int chunk, int64_t stride,
                          void* stream_) {
    if (!idx || !scratch || !chunk_bits) return DC_ERR_ARG;
    if ((uintptr_t)scratch & 3) return DC_ERR_ARG;               // the coder stores aligned 32-bit words
    if (T < 1 || hw < 1 || chunk < 1) return DC_ERR_SHAPE;
    const int64_t per = chunk < hw ? chunk : hw;                 // pixels the longest chunk holds
    if ((stride & 3) || stride < DC_GIF_CHUNK_MAX_BYTES(per)) return DC_ERR_SHAPE;
    const int64_t cpf = ((int64_t)hw + chunk - 1) / chunk;
    if (T * cpf > 0x7fffffffLL) return DC_ERR_SHAPE;
    hipLaunchKernelGGL(gif_lzw_kernel, dim3((unsigned)(T * cpf)), dim3(64), 0, (hipStream_t)stream_, idx, scratch, chunk_bits, hw,
                       chunk, (int)cpf, stride);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_gif_pack(const uint8_t* scratch, const int32_t* chunk_bits, int32_t* chunk_off, uint8_t* out, int32_t* frame_len,
                           int T, int chunks_per_frame, int64_t stride, int64_t frame_stride, void* stream_) {
    if (!scratch || !chunk_bits || !chunk_off || !out || !frame_len) return DC_ERR_ARG;
    if (T < 1 || T > 65535 || chunks_per_frame < 1 || stride < 1 || frame_stride < 1) return DC_ERR_SHAPE;
    if (9 + chunks_per_frame * (stride * 8) > 0x7fffffffLL) return DC_ERR_SHAPE;          // bit offsets are 32 bits
    hipLaunchKernelGGL(gif_scan_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream_, chunk_bits, chunk_off, frame_len,
                       chunks_per_frame);
    DC_CHECK_LAUNCH();
    hipLaunchKernelGGL(gif_gather_kernel, dim3(chunks_per_frame, T), dim3(256), 0, (hipStream_t)stream_, scratch, chunk_bits,
                       chunk_off, out, chunks_per_frame, stride, frame_stride);
    DC_CHECK_LAUNCH();
    return 0;
}
