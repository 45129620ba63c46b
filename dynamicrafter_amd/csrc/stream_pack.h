// The pack stage of the output encoders (jpeg.hip, gif.hip, png.hip), stated once. Each coder writes one variable-length string
// per chunk (a restart segment, an LZW chunk, a deflate chunk) into a worst-case-sized scratch row and records its length; the
// pack turns the rows of a frame into one contiguous run:
//   scan    one 256-thread workgroup per frame: off[s] = base0 + the lengths in front of chunk s; the grand total is the frame's
//           length (frame_excl_scan). What a chunk contributes, the base and what is done with the total stay with the format.
//   gather  one workgroup per chunk moves its string to its offset in the frame's output row (pack_copy_chunk for whole bytes;
//           gif.hip shifts bits and keeps its own). Bytes at or past frame_stride are dropped: frame_len still reports the full
//           length, so the host can tell and size the row anew.
// Everything here is forced inline. gfx950 only (wave64).
#pragma once
#include "dc_common.h"

// exclusive prefix sum over the wave; `total` = the sum over all 64 lanes
__device__ __forceinline__ int wave_excl_scan(int v, int lane, int& total) {
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    total = __shfl(inc, 63, 64);
    return inc - v;
}

// Exclusive scan over the n items of one frame, by a whole 256-thread workgroup: off[s] = base0 + the sum of len_of(s') over
// s' < s, for s < n. Returns base0 + the sum over all items, to every thread. 256 items per round: a wave scan, the four waves'
// totals through LDS, and a running base carried from round to round.
template <class LenOf>
__device__ __forceinline__ int frame_excl_scan(int n, int base0, int32_t* __restrict__ off, LenOf len_of) {
    __shared__ int part[4];
    __shared__ int base_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) base_s = base0;
    __syncthreads();
    for (int s0 = 0; s0 < n; s0 += 256) {
        const int s = s0 + tid;
        const int v = s < n ? len_of(s) : 0;
        int wtot;
        int ex = wave_excl_scan(v, lane, wtot);
        if (lane == 0) part[wv] = wtot;
        __syncthreads();
        const int base = base_s;
        for (int w = 0; w < wv; ++w) ex += part[w];
        if (s < n) off[s] = base + ex;
        __syncthreads();
        if (tid == 0) base_s = base + part[0] + part[1] + part[2] + part[3];
        __syncthreads();
    }
    return base_s;
}

// Byte copy of one chunk by a 256-thread workgroup: src[0 .. len) -> dst[off ..], dst = the frame's output row. Every byte has
// one writer; bytes that would fall at or beyond frame_stride are dropped.
__device__ __forceinline__ void pack_copy_chunk(const uint8_t* __restrict__ src, int len, uint8_t* __restrict__ dst, int64_t off,
                                                int64_t frame_stride) {
    for (int i = threadIdx.x; i < len; i += 256)
        if (off + i < frame_stride) dst[off + i] = src[i];
}
