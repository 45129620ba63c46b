// LDS staging vocabulary shared by the kernels that stream operands into LDS (gemm_conv.hip, gemm_conv_glds.hip with gemm_pipe.h /
// gemm_pipe16.h / gemm_pp.h, ff_fused.hip, flash_pipe.hip, attention.hip): the LDS address-space typedefs, the XOR swizzles of the
// 128- and 64-byte-row images, the zero chunk, the LDS-DMA issue functions with the one statement of the m0 rule, the counted
// vector-memory wait, the bounded wait on an LDS counter and the compile-time loop helpers. Everything here is forced inline
// or a type: a kernel that uses these compiles to the same instructions as one that spells them out.
#pragma once
#include "dc_common.h"
#include <stdint.h>
#include <type_traits>
#include <utility>

namespace {

typedef __attribute__((address_space(3))) char lds_char_t;
typedef __attribute__((address_space(3))) int lds_int_t;
typedef __attribute__((address_space(3))) bf16x4_t lds_bf16x4_t;
// pinned LDS fragment load: volatile, so it is issued where it is written and a hand-set read-ahead distance holds (the PD / PD2
// comment in ff_geglu_fused320_kernel, ff_fused.hip, tells why; the gemm_pipe16.h / gemm_pp.h / flash_pipe.hip streams rely on it too)
typedef const volatile __attribute__((address_space(3))) bf16x8_t lds_vfrag_t;

__device__ __forceinline__ int lds_off128(int row, int chunk) {
    // 128-byte rows, 16-byte chunks; XOR the chunk with bits of the row so that 16 rows (distinct mod 16)
    // reading the same logical chunk hit 16 distinct 16-byte slots of the 256-byte bank row.
    return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}
// the same for 64-byte rows of 4 chunks
__device__ __forceinline__ int lds_off64(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

// 32 zero bytes in device memory: padded taps / tail rows load from here, so every global load of the main loop is
// unconditional (a branch around a load makes hipcc wait for it at the join: four serialised round trips per tile).
// One copy per translation unit; a file that never names it emits none.
__device__ __attribute__((aligned(16))) uint32_t g_zero_chunk[8];

// ---- LDS-DMA: one wave instruction moves 64 lanes x 16 B from global memory to LDS [lds_dst, lds_dst + 1024), lane-linear
// (base + lane * 16: a swizzle is applied to the per-lane SOURCE address). lds_dst is wave-uniform and travels in m0.
// Issued from inline asm on purpose: hipcc tracks the builtin as a pending LDS write and drains vmcnt before the next
// ds_read; the asm form is invisible to that pass, so its completion is counted by hand (wait_vmcnt below).
//
// The m0 rule. m0 is reserved by the compiler and cannot be named as a clobber (hipcc only warns "inline asm clobber list
// contains reserved registers"), so every statement writes m0 and reads it in the same asm string. lds_dma16 and
// lds_dma16_sbase leave their value in m0: two scalar moves per piece are 8-10 issue clocks of a one-wave-per-SIMD stream
// (-0.5 % on the fused FeedForward). That is sound only while nothing else in a kernel that uses them reads or writes m0,
// i.e. while hipcc keeps no value of its own there (as it would for s_movrel, s_sendmsg or ds_gws_*, which these kernels
// do not use). Nothing promises that, so it is checked in the ISA the product flags give:
// tests/test_host_cpu.py::test_isa_keeps_m0_for_the_lds_dma_only compiles gemm_conv.hip, gemm_conv_glds.hip and ff_fused.hip
// and requires every m0 reference to be one of the moves below. lds_dma16_keep_m0 saves and restores m0 and needs no such
// promise; the 8-wave kernels of gemm_conv_glds.hip use it.

// per-lane 64-bit source address
__device__ __forceinline__ void lds_dma16(const void* gsrc, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(lds_dst) : "memory");
}
// 64-bit scalar base + per-lane 32-bit byte offset
__device__ __forceinline__ void lds_dma16_sbase(unsigned lds_dst, unsigned voff, uint64_t sbase) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_dst), "v"(voff), "s"(sbase) : "memory");
}
// per-lane 64-bit source address, m0 saved and restored
__device__ __forceinline__ void lds_dma16_keep_m0(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_dst)
        : "memory");
}

// at most N vector-memory operations of this wave still in flight (LDS-DMA pieces and asm loads are counted by hand;
// gfx950 counts stores in vmcnt too)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// A wait on an LDS counter; the caller has `int gave_up` in scope (0 at kernel start). Every wave posts every counter the
// same number of times, so a wait always ends; the bound (about 10 ms, once per wave) only keeps a future bookkeeping
// mistake from hanging the GPU. A wave that gave up carries on with whatever the ring holds - its tile is garbage - and
// ORs its kernel's bit (DC_ERRW_GEMM_PIPE, DC_ERRW_FLASH_RING) into the library's error word before it leaves:
// dc_error_word_read / ops.check_error_word make that loud on the host.
constexpr int LDS_SPIN_LIMIT = 200000;
#define LDS_SPIN(cond, reread)                                                     \
    do {                                                                           \
        int spins__ = 0;                                                           \
        while (!gave_up && (cond)) { reread; if (++spins__ > LDS_SPIN_LIMIT) gave_up = 1; } \
    } while (0)

// compile-time loop index / parameter, and f(ic<G>{}) for every G of an integer sequence in order
template <int V> using ic = std::integral_constant<int, V>;
template <int... G, class F>
__device__ __forceinline__ void for_ic(std::integer_sequence<int, G...>, F&& f) { (f(ic<G>{}), ...); }

}  // namespace
