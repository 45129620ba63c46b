// The fragment scheme of the head_dim-64 attention kernels built on v_mfma_f32_32x32x16_bf16 (attention.hip: flash_attn_d64_kernel,
// cross_attn_resident_kernel; flash_pipe.hip: flash_attn_d64_pipe_kernel; ff_fused.hip: ln_qkv_tattn_kernel), stated once. A kernel
// keeps its own tile loop, softmax and synchronisation and calls these pieces. Everything here is forced inline: a kernel that
// uses them compiles to the arithmetic it would spell out itself (profiles/attn_parts_isa.txt).
// temporal_attn_d64_kernel uses the 16x16 forms and a layout of its own; nothing here applies to it.
//
// A wave owns 32 query rows. lane = 32 fh + fr: fr = the lane's query row, fh = which half of every 8-wide k group it holds.
//   S^T = K (cQ)^T   A = K fragment kk (kk = 0..3): lane (fr, fh) holds K[key 32 jb + fr][d = 16 kk + 8 fh .. + 7], one 16-byte
//                        read of the key's 128-byte LDS row (chunk 2 kk + fh, XOR-swizzled: lds_off128).
//                    B = Q fragment kk: Q[query fr][the same d], times c = scale * log2(e) and rounded to bf16 again - one more
//                        rounding of Q, the size of the one it already has. The scores then leave the MFMA in exp2 units (and,
//                        where the accumulator starts at -m, as s - m directly).
//                    D: the lane owns ITS query row: register r of key block jb is key attn_key_of(32 jb, r, fh) =
//                        32 jb + (r & 3) + 8 (r >> 2) + 4 fh. The row's other 16 keys are in lane ^ 32: max and sum are per-lane scalars
//                        and one __shfl_xor(.., 32).
//   O^T += V^T P^T   B = P fragment ks (ks = 0, 1) of key block jb: registers 8 ks .. 8 ks + 7 of exp2(S^T), packed to bf16 in
//                        pairs (attn_pack_p). The accumulator IS the operand: its key order is the k order of this MFMA, keys
//                        32 jb + 16 ks + 4 fh + {0..3, 8..11}.
//                    A = V^T fragment (ks, db) (db = 32-wide slice of d): V[those 8 keys][d = 32 db + fr] from two
//                        ds_read_b64_tr_b16, 8 V rows apart (attn_vt_frag). In a transposed read lane i of a 16-lane group
//                        supplies the address of row (i >> 2), columns 4 (i & 3).. of the 16-column block ((lane >> 4) & 1):
//                        attn_vt_lane_off; the caller adds row 32 jb + 16 ks + 4 fh and column byte 64 db.
//                    D: register 4 qd + i of slice db is O[query fr][d = 32 db + 8 qd + 4 fh + i].
// V rows are ATTN_VLD = 192 bytes apart in LDS (128 of data): the four consecutive rows that a transposed read touches then land
// on four distinct 64-byte quarters of the 256-byte bank row (at a pitch of 128 they would share two of them).
// THE STORE. A row's channels 8 qd .. 8 qd + 7 are split over its two lanes, 4 each. One v_permlane32_swap per dword between the
// groups qd and qd + 1 gives the lower lane the 16 contiguous bytes of group qd and the upper lane those of group qd + 1: four
// 16-byte stores per row block instead of eight 8-byte ones (the store tail is issue-bound; with 93 keys it is a large part of a
// cross-attention workgroup). Rows past Lq compute on a clamped row and skip the store.
#pragma once
#include "dc_common.h"
#include "lds_stage.h"

namespace {

constexpr int ATTN_VLD = 192;   // bytes per V row in LDS

// key of S^T accumulator register r of the 32-key block that starts at key j0. Keys past a set's length are masked with it:
// their score becomes -1e30f, so P = 0 exactly (the staged rows there repeat the last key: finite data)
__device__ __forceinline__ int attn_key_of(int j0, int r, int fh) { return j0 + (r & 3) + 8 * (r >> 2) + 4 * fh; }
// 8 bf16 times c, rounded to bf16: the Q fragment from its 16-byte load (and a packed P fragment times 2^-step)
__device__ __forceinline__ bf16x8_t attn_q_scaled(const u32x4_t& raw, float c) {
    u32x4_t sc;
#pragma unroll
    for (int e = 0; e < 4; ++e) sc[e] = pack_bf2(__uint_as_float(raw[e] << 16) * c, __uint_as_float(raw[e] & 0xffff0000u) * c);
    return __builtin_bit_cast(bf16x8_t, sc);
}
// P fragment ks of a key block
__device__ __forceinline__ bf16x8_t attn_pack_p(const f32x16_t& s, int ks) {
    u32x4_t pw;
#pragma unroll
    for (int e = 0; e < 4; ++e) pw[e] = pack_bf2(s[8 * ks + 2 * e], s[8 * ks + 2 * e + 1]);
    return __builtin_bit_cast(bf16x8_t, pw);
}
__device__ __forceinline__ int attn_vt_lane_off(int lane) {
    const int li = lane & 15;
    return (li >> 2) * ATTN_VLD + (((lane >> 4) & 1) * 16 + (li & 3) * 4) * 2;
}
__device__ __forceinline__ bf16x8_t attn_vt_join(const bf16x4_t lo, const bf16x4_t hi) {
    bf16x8_t vf;
    vf[0] = lo[0]; vf[1] = lo[1]; vf[2] = lo[2]; vf[3] = lo[3];
    vf[4] = hi[0]; vf[5] = hi[1]; vf[6] = hi[2]; vf[7] = hi[3];
    return vf;
}
// vp = V tile + (32 jb + 16 ks + 4 fh) * ATTN_VLD + 64 db + attn_vt_lane_off(lane)
__device__ __forceinline__ bf16x8_t attn_vt_frag(const lds_char_t* vp) {
    const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4_t*)(vp));
    const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4_t*)(vp + 8 * ATTN_VLD));
    return attn_vt_join(lo, hi);
}
// staging: 16-byte chunk `chunk` of row r of a K tile (128-byte rows, swizzled: lds_off128) and of a V tile
__device__ __forceinline__ void attn_stage_row(char* sk, char* sv, int r, int chunk, const u32x4_t& kreg, const u32x4_t& vreg) {
    *reinterpret_cast<u32x4_t*>(sk + lds_off128(r, chunk)) = kreg;
    *reinterpret_cast<u32x4_t*>(sv + r * ATTN_VLD + chunk * 16) = vreg;
}
// THE STORE of one query row's 64 channels: f[db] = the finished (normalised) accumulator of slice db, orow = the (clamped)
// output row, live = the row exists
__device__ __forceinline__ void attn_store_row(bf16_t* orow, bool live, int fh, const f32x16_t (&f)[2]) {
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int qd = 0; qd < 4; qd += 2) {
            const unsigned a0 = pack_bf2(f[db][4 * qd + 0], f[db][4 * qd + 1]);
            const unsigned a1 = pack_bf2(f[db][4 * qd + 2], f[db][4 * qd + 3]);
            const unsigned b0 = pack_bf2(f[db][4 * qd + 4], f[db][4 * qd + 5]);
            const unsigned b1 = pack_bf2(f[db][4 * qd + 6], f[db][4 * qd + 7]);
            const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
            const auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
            const u32x4_t pk = {r0[0], r1[0], r0[1], r1[1]};
            if (live) *reinterpret_cast<u32x4_t*>(orow + db * 32 + 8 * (qd + fh)) = pk;
        }
}

}  // namespace
