// PNG / APNG image data for the output side of the harness: display frames uint8 [T][H][W][C] (what dc_frames_to_u8 writes) -> one
// zlib stream per frame, ready to be wrapped in IDAT / fdAT chunks on the host (utils/save_video.py, deflate="hip"). Lossless.
// Deflate is serial within a stream, so a frame's filtered scanlines are cut into chunks of `chunk` bytes that are each coded on
// their own into a whole number of bytes (as pigz does it), the way a restart interval is in jpeg.hip and a chunk in gif.hip.
// Matches are run-length only (distance 1): on filtered residuals a general match search buys nothing (zlib's Z_RLE), and runs
// come from a scan. Three stages, three entries:
//   dc_png_filter   per row the PNG filter 0..4 with the least sum of min(r, 256 - r), one wave per row
//   dc_png_deflate  one chunk per wave: runs -> counts -> two Huffman tables -> one dynamic block, or the stored form if that is
//                   not longer; the chunk's Adler-32 while the bytes are in LDS
//   dc_png_pack     exclusive scan of the chunk lengths, byte copy, the frame's Adler-32 from the chunks' values
// All integer arithmetic. gfx950 only (wave64).
#include "dc_common.h"
#include "dcrafter_hip.h"
#include "stream_pack.h"

namespace {

constexpr int kAdlerBase = 65521;

// ---------------------------------------------------------------------------------------------- stage 1: row filters
constexpr int kFilterMaxBlocks = 2048;          // 8 workgroups of 4 waves per CU: rows beyond that are walked by a grid stride

__device__ __forceinline__ int cost8(int r) {
    r &= 255;
    return min(r, 256 - r);
}
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// the predictor of filter `ft` from the left (a), upper (b) and upper-left (c) raw bytes
__device__ __forceinline__ int predict(int ft, int a, int b, int c) {
    return ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
}

// One wave per row. Filters read raw bytes of this row and the one above (a zero row above row 0 of every frame), so rows are
// independent. First walk: the five costs, reduced over the wave; the least wins, the lowest type on a tie. Second walk: the
// winner's residuals (the row is in L2 by then).
__global__ __launch_bounds__(256) void png_filter_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ planes,
                                                         int64_t rows, int H, int rb, int bpp) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += nw) {
        const bool top = r % H == 0;
        const uint8_t* cur = frames + r * rb;
        const uint8_t* up = top ? cur : cur - rb;                // never read through when top
        int cost[5] = {0, 0, 0, 0, 0};
        for (int x = lane; x < rb; x += 64) {
            const int v = cur[x], a = x >= bpp ? cur[x - bpp] : 0, b = top ? 0 : up[x], c = (top || x < bpp) ? 0 : up[x - bpp];
#pragma unroll
            for (int ft = 0; ft < 5; ++ft) cost[ft] += cost8(v - predict(ft, a, b, c));
        }
        int best = 0, bc = wave_sum_i(cost[0]);
#pragma unroll
        for (int ft = 1; ft < 5; ++ft) {
            const int s = wave_sum_i(cost[ft]);
            if (s < bc) { bc = s; best = ft; }
        }
        uint8_t* dst = planes + r * ((int64_t)rb + 1);
        if (lane == 0) dst[0] = (uint8_t)best;
        for (int x = lane; x < rb; x += 64) {
            const int v = cur[x], a = x >= bpp ? cur[x - bpp] : 0, b = top ? 0 : up[x], c = (top || x < bpp) ? 0 : up[x - bpp];
            dst[1 + x] = (uint8_t)(v - predict(best, a, b, c));
        }
    }
}

// ---------------------------------------------------------------------------------------------- stage 2: deflate of one chunk
constexpr int kLit = 286, kCl = 19, kSym = 288;  // literal/length alphabet, code-length alphabet, table size
constexpr int kMaxRounds = 17;                   // halvings of a count below 2^16 until it is 1, plus the first build
__constant__ uint8_t kClOrder[kCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// match length 3..258 -> its symbol 257..285 (RFC 1951 3.2.5); the extra value is (m - 3) & ((1 << extra) - 1)
__device__ __forceinline__ int len_symbol(int m) {
    if (m == 258) return 285;
    const int l = m - 3;
    if (l < 8) return 257 + l;
    const int e = 29 - __clz(l);                                 // floor(log2 l) - 2
    return 261 + 4 * e + ((l >> e) & 3);
}
__device__ __forceinline__ int sym_extra_bits(int s) { return (s < 265 || s == 285) ? 0 : (s - 261) >> 2; }

struct Tables {                                                  // LDS, one per wave
    int cnt[kSym];                                               // counts as counted
    int work[kSym];                                              // counts as the builder halves them
    int lens[kSym], code[kSym];                                  // literal/length code: lengths, bit-reversed codes
    int leaf_w[kSym], leaf_s[kSym], lpar[kSym];                  // leaves sorted by (count, symbol); the node each went into
    int iw[kSym], ipar[kSym], depth[kSym];                       // merged nodes in the order made
    int ct[kSym];                                                // code-length tokens: symbol | extra value << 8
    int ccnt[kCl], cwork[kCl], clens[kCl], ccode[kCl];
    int blc[16], nxt[16];
    int nct, hclen, hdr_bits;
};

// Deterministic Huffman lengths under `limit`, by the whole wave: see tests/png_restatement.py huff_lengths, which restates this.
// work[] holds the counts and is consumed. The serial part (two queues, depths of the merged nodes) runs on lane 0.
__device__ void build_lengths(Tables& t, int* work, int nsym, int limit, int* lens, int lane) {
    __syncthreads();
    {
        int used = 0, only = -1;
        for (int s = lane; s < nsym; s += 64)
            if (work[s]) { ++used; only = s; }
        used = wave_sum_i(used);
        only = wave_max_i(only);
        if (used == 1 && lane == 0) work[only == 0 ? 1 : 0] = 1;
    }
    for (int round = 0; round < kMaxRounds; ++round) {
        __syncthreads();
        int mine = 0;
        for (int s = lane; s < nsym; s += 64) {
            const int c = work[s];
            lens[s] = 0;
            if (c) {
                int rank = 0;
                for (int j = 0; j < nsym; ++j) {                 // the same j in every lane: an LDS broadcast
                    const int cj = work[j];
                    rank += (cj != 0) & ((cj < c) | ((cj == c) & (j < s)));
                }
                t.leaf_w[rank] = c;
                t.leaf_s[rank] = s;
                ++mine;
            }
        }
        const int m = wave_sum_i(mine);                          // >= 2
        __syncthreads();
        if (lane == 0 && m >= 2) {
            int li = 0, ii = 0;
            for (int k = 0; k < m - 1; ++k) {
                int w = 0;
#pragma unroll
                for (int pick = 0; pick < 2; ++pick) {
                    if (li < m && (ii >= k || t.leaf_w[li] <= t.iw[ii])) {
                        w += t.leaf_w[li];
                        t.lpar[li++] = k;
                    } else {
                        w += t.iw[ii];
                        t.ipar[ii++] = k;
                    }
                }
                t.iw[k] = w;
            }
            t.depth[m - 2] = 0;
            for (int k = m - 3; k >= 0; --k) t.depth[k] = t.depth[t.ipar[k]] + 1;
        }
        __syncthreads();
        int deepest = 0;
        for (int i = lane; i < m; i += 64) {
            const int d = t.depth[t.lpar[i]] + 1;
            lens[t.leaf_s[i]] = d;
            deepest = max(deepest, d);
        }
        if (wave_max_i(deepest) <= limit) break;                 // wave-uniform
        __syncthreads();
        for (int s = lane; s < nsym; s += 64) work[s] = (work[s] + 1) >> 1;
    }
    __syncthreads();
}

// canonical codes (RFC 1951 3.2.2), stored bit-reversed: Huffman codes go out most significant bit first. Lane 0.
__device__ void canonical_codes(Tables& t, const int* lens, int* code, int nsym) {
    for (int b = 0; b < 16; ++b) t.blc[b] = 0;
    for (int s = 0; s < nsym; ++s) t.blc[lens[s] & 15]++;
    t.blc[0] = 0;
    int c = 0;
    t.nxt[0] = 0;
    for (int b = 1; b < 16; ++b) {
        c = (c + t.blc[b - 1]) << 1;
        t.nxt[b] = c;
    }
    for (int s = 0; s < nsym; ++s) {
        const int l = lens[s] & 15;                              // lengths are at most 15: the index stays inside the tables
        code[s] = l ? (int)(__brev((unsigned)t.nxt[l]++) >> (32 - l)) : 0;
    }
}

// ORs `nb` <= 32 bits into the zeroed bit string; nothing lands behind `nwords`
__device__ __forceinline__ void put_bits(uint32_t* outw, int nwords, int pos, uint32_t v, int nb) {
    const int w = pos >> 5, s = pos & 31;
    if (w < nwords) atomicOr(&outw[w], v << s);
    if (s + nb > 32 && w + 1 < nwords) atomicOr(&outw[w + 1], v >> (32 - s));
}

// The runs that END inside this lane's four bytes of tile `tile` (256 bytes per tile, lane l holds bytes 4 l .. 4 l + 3): len[k] =
// the length of the run that ends at byte k, 0 if none does. A run's start is the last boundary (byte 0, or a byte that differs
// from the one before) at or in front of its end: the lane's own, else the latest of the lanes and tiles in front - an inclusive
// max-scan over the wave and `carry` from tile to tile (wave-uniform).
__device__ __forceinline__ uint32_t tile_runs(const uint32_t* dataw, int dwords, int n, int tile, int lane, int& carry, int len[4]) {
    const int wi = tile * 64 + lane, base = wi * 4;
    const uint32_t w = wi < dwords ? dataw[wi] : 0u;
    const int prev = (wi > 0 && wi - 1 < dwords) ? (int)(dataw[wi - 1] >> 24) : -1;
    const int next = wi + 1 < dwords ? (int)(dataw[wi + 1] & 0xffu) : -1;
    int last = -1;
    bool bd[4], en[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = base + k;
        const int cur = (int)(w >> (8 * k)) & 0xff;
        const int before = k ? (int)(w >> (8 * k - 8)) & 0xff : prev;
        const int after = k < 3 ? (int)(w >> (8 * k + 8)) & 0xff : next;
        bd[k] = p < n && (p == 0 || cur != before);
        en[k] = p < n && (p == n - 1 || cur != after);
        if (bd[k]) last = p;
    }
    int inc = last;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc = max(inc, up);
    }
    int start = __shfl_up(inc, 1, 64);
    if (lane == 0) start = -1;
    start = max(start, carry);
    carry = max(carry, __shfl(inc, 63, 64));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (bd[k]) start = base + k;
        len[k] = en[k] ? base + k + 1 - start : 0;
    }
    return w;
}

// One wave per chunk; the chunk, the bit string and the tables in LDS. See the file header and DESIGN 4.10 for the format.
__global__ __launch_bounds__(64) void png_deflate_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ scratch,
                                                         int32_t* __restrict__ chunk_len, uint32_t* __restrict__ chunk_adler, int N,
                                                         int chunk, int cpf, int64_t stride, int dwords_max, int owords) {
    extern __shared__ uint32_t lds[];
    __shared__ Tables t;
    uint32_t* dataw = lds;
    uint32_t* outw = lds + dwords_max;
    uint8_t* datab = (uint8_t*)dataw;
    uint8_t* outb = (uint8_t*)outw;
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int f = (int)(c / cpf), ci = (int)(c % cpf);
    const int p0 = ci * chunk;                                   // ci * chunk < N <= INT_MAX
    const int n = min(chunk, N - p0);
    const int dwords = (n + 3) >> 2;
    const bool final = ci + 1 == cpf;
    const uint8_t* src = planes + (int64_t)f * N + p0;
    uint8_t* out = scratch + c * stride;

    if (lane == 0) dataw[dwords - 1] = 0u;                       // the bytes behind n in the last word
    for (int i = lane; i < owords; i += 64) outw[i] = 0u;
    for (int i = lane; i < kSym; i += 64) t.cnt[i] = 0;
    __syncthreads();
    for (int i = lane; i < n; i += 64) datab[i] = src[i];
    __syncthreads();

    // pass 1: counts per run (integer atomics: no order in the result), Adler sums of the chunk alone
    const int tiles = (n + 255) >> 8;
    unsigned long long sa = 0, sb = 0;
    int carry = -1;
    for (int tile = 0; tile < tiles; ++tile) {
        int len[4];
        const uint32_t w = tile_runs(dataw, dwords, n, tile, lane, carry, len);
        const int base = (tile * 64 + lane) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = (int)(w >> (8 * k)) & 0xff;
            if (base + k < n) {
                sa += (unsigned)d;
                sb += (unsigned long long)(unsigned)(n - base - k) * (unsigned)d;
            }
            if (len[k]) {
                const int rem = len[k] - 1, full = rem / 258, r = rem % 258;
                atomicAdd(&t.cnt[d], 1 + (r < 3 ? r : 0));
                if (full) atomicAdd(&t.cnt[285], full);
                if (r >= 3) atomicAdd(&t.cnt[len_symbol(r)], 1);
            }
        }
    }
    sa = wave_sum_u64(sa);
    sb = wave_sum_u64(sb);
    if (lane == 0) {
        t.cnt[256] = 1;
        chunk_adler[c] = (uint32_t)((1 + sa) % kAdlerBase) | ((uint32_t)((n + sb) % kAdlerBase) << 16);
    }
    __syncthreads();

    // the literal/length code
    int nmatch = 0;
    for (int s = lane; s < kSym; s += 64) {
        const int v = s < kLit ? t.cnt[s] : 0;
        t.work[s] = v;
        if (s >= 257) nmatch += v;
    }
    nmatch = wave_sum_i(nmatch);
    build_lengths(t, t.work, kLit, 15, t.lens, lane);
    int hl = 0;
    for (int s = lane; s < kLit; s += 64)
        if (t.lens[s]) hl = s + 1;
    const int hlit = max(257, wave_max_i(hl));
    const int dlen = nmatch ? 1 : 0;

    // the lengths as runs in the code-length alphabet, its counts
    if (lane == 0) {
        canonical_codes(t, t.lens, t.code, kLit);
        for (int s = 0; s < kCl; ++s) t.ccnt[s] = 0;
        int nct = 0, i = 0;
        const int nseq = hlit + 1;
        while (i < nseq) {                                       // every round consumes at least one of nseq <= 287 entries
            const int v = i < hlit ? t.lens[i] : dlen;
            int j = i + 1;
            while (j < nseq && (j < hlit ? t.lens[j] : dlen) == v) ++j;
            int L = j - i;
            if (v == 0) {
                while (L >= 11) {
                    const int m = min(L, 138);
                    t.ct[nct++] = 18 | ((m - 11) << 8);
                    t.ccnt[18]++;
                    L -= m;
                }
                if (L >= 3) {
                    t.ct[nct++] = 17 | ((L - 3) << 8);
                    t.ccnt[17]++;
                    L = 0;
                }
            } else {
                t.ct[nct++] = v;
                t.ccnt[v]++;
                --L;
                while (L >= 3) {
                    const int m = min(L, 6);
                    t.ct[nct++] = 16 | ((m - 3) << 8);
                    t.ccnt[16]++;
                    L -= m;
                }
            }
            for (; L > 0; --L) {
                t.ct[nct++] = v;
                t.ccnt[v]++;
            }
            i = j;
        }
        t.nct = nct;
        for (int s = 0; s < kCl; ++s) t.cwork[s] = t.ccnt[s];
    }
    build_lengths(t, t.cwork, kCl, 7, t.clens, lane);
    if (lane == 0) {
        canonical_codes(t, t.clens, t.ccode, kCl);
        int hclen = 4;
        for (int i = 4; i < kCl; ++i)
            if (t.clens[kClOrder[i]]) hclen = i + 1;
        int bits = 17 + 3 * hclen;
        for (int s = 0; s < kCl; ++s) bits += t.ccnt[s] * (t.clens[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0));
        t.hclen = hclen;
        t.hdr_bits = bits;
    }
    __syncthreads();

    // (a) dynamic block + empty stored block against (b) one stored block
    int tok_bits = 0;
    for (int s = lane; s < kLit; s += 64) tok_bits += t.cnt[s] * (t.lens[s] + sym_extra_bits(s));
    const int dyn_bits = t.hdr_bits + wave_sum_i(tok_bits) + nmatch;            // header, tokens with their extra and distance bits, EOB
    const int body = (dyn_bits + 3 + 7) >> 3;
    int nbytes;
    if (body + 4 < n + 5) {
        nbytes = body + 4;
        if (lane == 0) {
            int pos = 0;
            auto put = [&](uint32_t v, int nb) { put_bits(outw, owords, pos, v, nb); pos += nb; };
            put(0u, 1);
            put(2u, 2);
            put((uint32_t)(hlit - 257), 5);
            put(0u, 5);
            put((uint32_t)(t.hclen - 4), 4);
            for (int i = 0; i < t.hclen; ++i) put((uint32_t)t.clens[kClOrder[i]], 3);
            for (int i = 0; i < t.nct; ++i) {
                const int s = t.ct[i] & 0xff;
                put((uint32_t)t.ccode[s], t.clens[s]);
                if (s >= 16) put((uint32_t)(t.ct[i] >> 8), s == 16 ? 2 : s == 17 ? 3 : 7);
            }
            put_bits(outw, owords, dyn_bits - t.lens[256], (uint32_t)t.code[256], t.lens[256]);
            put_bits(outw, owords, dyn_bits, final ? 1u : 0u, 3);
            put_bits(outw, owords, 8 * (body + 2), 0xffffu, 16);
        }
        // pass 2: every run's bit offset from a scan of the runs' sizes, then its tokens
        const int l285 = t.lens[285], c285 = t.code[285];
        int at = t.hdr_bits;
        carry = -1;
        for (int tile = 0; tile < tiles; ++tile) {
            int len[4], size[4], mine = 0;
            const uint32_t w = tile_runs(dataw, dwords, n, tile, lane, carry, len);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                size[k] = 0;
                if (len[k]) {
                    const int d = (int)(w >> (8 * k)) & 0xff;
                    const int rem = len[k] - 1, full = rem / 258, r = rem % 258;
                    size[k] = t.lens[d] * (1 + (r < 3 ? r : 0)) + full * (l285 + 1);
                    if (r >= 3) {
                        const int s = len_symbol(r);
                        size[k] += t.lens[s] + sym_extra_bits(s) + 1;
                    }
                }
                mine += size[k];
            }
            int total;
            int pos = at + wave_excl_scan(mine, lane, total);
            at += total;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!len[k]) continue;
                const int d = (int)(w >> (8 * k)) & 0xff;
                const int rem = len[k] - 1, full = rem / 258, r = rem % 258;
                const int ld = t.lens[d];
                const uint32_t cd = (uint32_t)t.code[d];
                put_bits(outw, owords, pos, cd, ld);
                pos += ld;
                for (int i = 0; i < full; ++i) {                 // at most n / 258 rounds
                    put_bits(outw, owords, pos, (uint32_t)c285, l285 + 1);     // the distance code is one 0 bit behind it
                    pos += l285 + 1;
                }
                if (r >= 3) {
                    const int s = len_symbol(r), e = sym_extra_bits(s), ls = t.lens[s];
                    put_bits(outw, owords, pos, (uint32_t)t.code[s] | ((uint32_t)((r - 3) & ((1 << e) - 1)) << ls), ls + e + 1);
                    pos += ls + e + 1;
                } else {
                    for (int i = 0; i < r; ++i) {
                        put_bits(outw, owords, pos, cd, ld);
                        pos += ld;
                    }
                }
            }
        }
    } else {
        nbytes = n + 5;
        if (lane == 0) {
            outb[0] = final ? 1 : 0;
            outb[1] = (uint8_t)n;
            outb[2] = (uint8_t)(n >> 8);
            outb[3] = (uint8_t)~n;
            outb[4] = (uint8_t)(~n >> 8);
        }
        for (int i = lane; i < n; i += 64) outb[5 + i] = datab[i];
    }
    __syncthreads();
    const int whole = nbytes >> 2;                               // nbytes <= n + 5 <= 4 owords
    for (int i = lane; i < whole; i += 64)
        if (4 * (int64_t)i + 4 <= stride) *(uint32_t*)(out + 4 * (int64_t)i) = outw[i];
    for (int i = 4 * whole + lane; i < nbytes; i += 64)
        if (i < stride) out[i] = outb[i];
    if (lane == 0) chunk_len[c] = nbytes;
}

// ---------------------------------------------------------------------------------------------- stage 3: pack
// One workgroup per frame: chunk_off[c] = the byte at which chunk c starts in the frame's stream, behind the two header bytes;
// the frame's Adler-32 from the chunks' own values. With s_c = A_c - 1 the byte sum of chunk c and R_c the number of bytes of
// the plane behind it, A = 1 + sum s_c and B = sum (B_c + R_c s_c), modulo 65521: what folding zlib's adler32_combine over the
// chunks in order gives, as a plain sum. The thread that ends the scan writes 78 01, the trailer and frame_len.
__global__ __launch_bounds__(256) void png_scan_kernel(const int32_t* __restrict__ chunk_len, const uint32_t* __restrict__ chunk_adler,
                                                       int32_t* __restrict__ chunk_off, uint8_t* __restrict__ out,
                                                       int32_t* __restrict__ frame_len, int N, int chunk, int cpf, int64_t stride,
                                                       int64_t frame_stride) {
    __shared__ unsigned long long pa[4], pb[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t f0 = (int64_t)blockIdx.x * cpf;
    unsigned long long sa = 0, sb = 0;
    for (int s = tid; s < cpf; s += 256) {
        const uint32_t ad = chunk_adler[f0 + s];
        const unsigned long long sc = ((ad & 0xffffu) + kAdlerBase - 1) % kAdlerBase;
        const unsigned long long behind = (unsigned long long)(N - min((int64_t)(s + 1) * chunk, (int64_t)N));
        sa += sc;
        sb += ((ad >> 16) + behind * sc) % kAdlerBase;
    }
    sa = wave_sum_u64(sa);
    sb = wave_sum_u64(sb);
    if (lane == 0) { pa[wv] = sa; pb[wv] = sb; }
    // a chunk's length clamped to [0, stride]: what png_copy_kernel moves; the scan's barriers also publish pa / pb
    const int end = frame_excl_scan(cpf, 2, chunk_off + f0,
                                    [&](int s) { return (int)min((int64_t)max(chunk_len[f0 + s], 0), stride); });
    if (tid == 0) {
        const uint32_t A = (uint32_t)((1 + pa[0] + pa[1] + pa[2] + pa[3]) % kAdlerBase);
        const uint32_t B = (uint32_t)((pb[0] + pb[1] + pb[2] + pb[3]) % kAdlerBase);
        uint8_t* dst = out + (int64_t)blockIdx.x * frame_stride;
        const uint8_t head[2] = {0x78, 0x01}, tail[4] = {(uint8_t)(B >> 8), (uint8_t)B, (uint8_t)(A >> 8), (uint8_t)A};
        for (int i = 0; i < 2; ++i)
            if (i < frame_stride) dst[i] = head[i];
        for (int i = 0; i < 4; ++i)
            if ((int64_t)end + i < frame_stride) dst[end + i] = tail[i];
        frame_len[blockIdx.x] = end + 4;
    }
}

// Byte copy, one workgroup per chunk: every byte of the stream has one writer. Bytes that would fall beyond frame_stride are
// dropped (frame_len still reports the full length).
__global__ __launch_bounds__(256) void png_copy_kernel(const uint8_t* __restrict__ scratch, const int32_t* __restrict__ chunk_len,
                                                       const int32_t* __restrict__ chunk_off, uint8_t* __restrict__ out, int cpf,
                                                       int64_t stride, int64_t frame_stride) {
    const int64_t c = (int64_t)blockIdx.y * cpf + blockIdx.x;
    const int len = (int)min((int64_t)max(chunk_len[c], 0), stride);
    pack_copy_chunk(scratch + c * stride, len, out + (int64_t)blockIdx.y * frame_stride, chunk_off[c], frame_stride);
}

}  // namespace

extern "C" int dc_png_filter(const uint8_t* frames, uint8_t* planes, int T, int H, int W, int C, void* stream_) {
    if (!frames || !planes) return DC_ERR_ARG;
    if (T < 1 || H < 1 || W < 1 || (C != 1 && C != 3 && C != 4)) return DC_ERR_SHAPE;
    if ((1 + (int64_t)W * C) * H > 0x7fffffffLL) return DC_ERR_SHAPE;           // a plane is addressed with 31 bits
    const int64_t rows = (int64_t)T * H;
    const int64_t nblocks = (rows + 3) / 4;
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)(nblocks < kFilterMaxBlocks ? nblocks : kFilterMaxBlocks)), dim3(256), 0,
                       (hipStream_t)stream_, frames, planes, rows, H, W * C, C);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_png_deflate(const uint8_t* planes, uint8_t* scratch, int32_t* chunk_len, uint32_t* chunk_adler, int T, int N,
                              int chunk, int64_t stride, void* stream_) {
    if (!planes || !scratch || !chunk_len || !chunk_adler) return DC_ERR_ARG;
    if ((uintptr_t)scratch & 3) return DC_ERR_ARG;               // whole words of a string are stored as aligned 32-bit words
    if (T < 1 || N < 1 || chunk < 1 || chunk > DC_PNG_CHUNK_LIMIT) return DC_ERR_SHAPE;
    const int per = chunk < N ? chunk : N;                       // bytes the longest chunk holds
    if ((stride & 3) || stride < DC_PNG_CHUNK_MAX_BYTES(per)) return DC_ERR_SHAPE;
    const int64_t cpf = ((int64_t)N + chunk - 1) / chunk;
    if (T * cpf > 0x7fffffffLL) return DC_ERR_SHAPE;
    const int dwords = (per + 3) / 4, owords = (per + 5 + 3) / 4;
    static DcLdsOnce lds_once;
    if (const int e = lds_once.ensure(reinterpret_cast<const void*>(&png_deflate_kernel),
                                      4 * ((DC_PNG_CHUNK_LIMIT + 3) / 4 + (DC_PNG_CHUNK_LIMIT + 8) / 4)))
        return e;
    hipLaunchKernelGGL(png_deflate_kernel, dim3((unsigned)(T * cpf)), dim3(64), 4 * (size_t)(dwords + owords), (hipStream_t)stream_,
                       planes, scratch, chunk_len, chunk_adler, N, chunk, (int)cpf, stride, dwords, owords);
    DC_CHECK_LAUNCH();
    return 0;
}

extern "C" int dc_png_pack(const uint8_t* scratch, const int32_t* chunk_len, const uint32_t* chunk_adler, int32_t* chunk_off,
                           uint8_t* out, int32_t* frame_len, int T, int N, int chunk, int64_t stride, int64_t frame_stride,
                           void* stream_) {
    if (!scratch || !chunk_len || !chunk_adler || !chunk_off || !out || !frame_len) return DC_ERR_ARG;
    if (T < 1 || T > 65535 || N < 1 || chunk < 1 || chunk > DC_PNG_CHUNK_LIMIT || stride < 1 || frame_stride < 1) return DC_ERR_SHAPE;
    const int64_t cpf = ((int64_t)N + chunk - 1) / chunk;
    if (6 + cpf * stride > 0x7fffffffLL) return DC_ERR_SHAPE;   // byte offsets inside a frame are 32 bits
    hipLaunchKernelGGL(png_scan_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream_, chunk_len, chunk_adler, chunk_off, out,
                       frame_len, N, chunk, (int)cpf, stride, frame_stride);
    DC_CHECK_LAUNCH();
    hipLaunchKernelGGL(png_copy_kernel, dim3((unsigned)cpf, T), dim3(256), 0, (hipStream_t)stream_, scratch, chunk_len, chunk_off, out,
                       (int)cpf, stride, frame_stride);
    DC_CHECK_LAUNCH();
    return 0;
}
