// The exact-fit GEMM: C[M,N] = A[M,K] W[N,K]^T (+ bias) (+ bf16 residual), bf16 out, fp32 accumulation, for launches whose
// output is a whole number of rounds of 288 x 320 tiles over the CUs of the device.
//
// Why another kernel. The UNet's native resolution has row counts that are multiples of 256 x 72 (level 2: 18432 rows), and a
// 288 x 320 tile covers [18432 x 1280] in exactly 64 x 4 = 256 tiles: one per CU, one round, no ragged last round, no split-K,
// no fp32 partials and no reduce launch. The 128 x 256 tiles of gemm_persist_kernel<128> need 2.8 rounds for the same output, and
// prologue, epilogue and the partial third round are a third of each of those launches.
//   * a workgroup is 4 waves, one per SIMD, arranged 2 x 2: a wave owns 144 rows x 160 columns = 9 x 10 accumulator blocks of
//     v_mfma_f32_16x16x32_bf16 (360 accumulator registers of the 512 a lone wave may use). 2 x 2 needs 9 + 10 fragment reads
//     per K step for 90 MFMAs; 4 x 1 would need 18 + 5.
//   * both operands come by LDS-DMA (lds_stage.h) in lane-linear pieces of 16 rows x 64 B with the 64-byte-row swizzle of
//     gemm_pp.h: K tiles of 32, a stage = 18 activation pieces + 20 weight pieces = 38 KB, ring of 4 = 152 KB. The four waves
//     share the 38 pieces of a stage round-robin (waves 0 and 1 issue 10, waves 2 and 3 issue 9).
//   * ring synchronisation is ONE workgroup barrier per K tile: behind "my pieces of tile t have landed" it says both that all
//     of tile t is in LDS and that every wave is past its reads of tile t - 1, whose stage then receives tile t + 3.
//     Workgroups never talk to each other.
//   * the K loop is compiler-scheduled code around MFMAs in source order: ordinary LDS loads, no hand-placed gaps; the MFMAs,
//     the LDS-DMA pieces and their counted waits are asm statements.
//   * the residual is added to the accumulators on the matrix pipe behind the K loop, the way gemm_persist_kernel's ring residual
//     is (gemm_parts.h): (acc + residual) + bias in fp32, rounded ONCE. A wave reads its own 144 x 160 patch of the residual,
//     and all of it before its first store: out may be the residual.
//   * epilogue: 16 rows x 160 columns of a wave at a time go as fp32 through a patch of the freed ring and come back row-major,
//     8 columns (16 bytes of bf16) per lane; the bias is added there.
// Tiles loop per workgroup: tile = xcd_remap(workgroup) + round * grid; consecutive tiles share an activation panel.
#include "lds_stage.h"
#include "dcrafter_hip.h"

namespace {

constexpr int FIT_BM = 288, FIT_BN = 320, FIT_K = 32, FIT_NST = 4;
constexpr int FIT_APIECES = FIT_BM / 16;                   // 18
constexpr int FIT_PIECES = FIT_APIECES + FIT_BN / 16;      // 38
constexpr int FIT_STAGE = FIT_PIECES * 1024;               // 38 KB
constexpr int FIT_LDS = FIT_NST * FIT_STAGE;               // 152 KB
constexpr int FIT_PROW = 164;                              // fp32 per patch row: 160 + 4 (16 rows start in 16 distinct bank quads)
constexpr int FIT_PATCH = 16 * FIT_PROW * 4;               // 10.25 KB per wave
static_assert(4 * FIT_PATCH <= FIT_LDS, "epilogue patches live in the freed ring");

// The MFMAs are asm statements, because the 90 accumulator blocks must be split by hand: hipcc keeps the accumulator of a builtin
// MFMA in the accumulator file only (256 registers = 64 blocks) and moved the other 26 blocks in and out of it around every use
// (212 v_accvgpr moves per K tile). Row blocks 0 .. 5 (240 registers) live in the accumulator file, 6 .. 8 (120) in VGPRs.
constexpr int FIT_RB_A = 6;
#define FIT_MFMA_A(d, w, x) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(d) : "v"(w), "v"(x))
#define FIT_MFMA_V(d, w, x) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(d) : "v"(w), "v"(x))

// padding between compiler-generated accesses of the accumulators and the asm MFMAs (hipcc does not see the MFMA inside an asm
// statement and pads no hazard for it): every block passes through a statement that holds 16 wait states
__device__ __forceinline__ void fit_settle(f32x4_t (&acc)[9][10]) {
#pragma unroll
    for (int rb = 0; rb < 9; ++rb) {
        if (rb < FIT_RB_A)
            asm volatile("s_nop 7\n\ts_nop 7"
                         : "+a"(acc[rb][0]), "+a"(acc[rb][1]), "+a"(acc[rb][2]), "+a"(acc[rb][3]), "+a"(acc[rb][4]), "+a"(acc[rb][5]),
                           "+a"(acc[rb][6]), "+a"(acc[rb][7]), "+a"(acc[rb][8]), "+a"(acc[rb][9]));
        else
            asm volatile("s_nop 7\n\ts_nop 7"
                         : "+v"(acc[rb][0]), "+v"(acc[rb][1]), "+v"(acc[rb][2]), "+v"(acc[rb][3]), "+v"(acc[rb][4]), "+v"(acc[rb][5]),
                           "+v"(acc[rb][6]), "+v"(acc[rb][7]), "+v"(acc[rb][8]), "+v"(acc[rb][9]));
    }
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
}

// at most `n` of this wave's LDS-DMA pieces still in flight; n is wave-uniform and one of {0, 9, 10, 18, 20}
__device__ __forceinline__ void fit_wait(int n) {
    if (n >= 20) wait_vmcnt<20>();
    else if (n >= 18) wait_vmcnt<18>();
    else if (n >= 10) wait_vmcnt<10>();
    else if (n >= 9) wait_vmcnt<9>();
    else wait_vmcnt<0>();
}

// Requirements (fit_check): mode 0, bf16 output, no GEGLU / GELU / rowvec / alpha, M % 288 == 0, N % 320 == 0, K % 64 == 0,
// tiles % gridDim.x == 0, 16-byte aligned rows. Tile bases are 64-bit; the 32-bit per-lane offsets span the 320 rows of a tile.
__global__ __launch_bounds__(256, 1) __attribute__((amdgpu_waves_per_eu(1, 1)))
void gemm_fit_kernel(const DcGemmParams p, const int rounds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 15, lq = lane >> 4;
    const int tiles_n = p.N / FIT_BN;
    const int nk = p.K / FIT_K;
    const int grid = gridDim.x;
    const unsigned lds_base = (unsigned)(uintptr_t)((const lds_char_t*)smem);

    // ---- LDS-DMA pieces (1 KB, lane-linear in LDS = 16 rows x 64 B): lane l carries row l >> 2 of the piece, chunk slot l & 3,
    // which holds source chunk (l & 3) ^ ((row >> 1) & 3). Piece q of a stage: q < 18 activation rows 16 q .. + 15 of the tile,
    // else weight rows 16 (q - 18) .. + 15; this wave issues pieces wave + 4 j.
    const int np = wave < 2 ? 10 : 9;
    const unsigned src_chunk = (unsigned)(((lane & 3) ^ ((lane >> 3) & 3)) << 4);
    unsigned voff[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const int q = wave + 4 * j;
        const bool is_a = q < FIT_APIECES;
        const int row = (is_a ? q : q - FIT_APIECES) * 16 + (lane >> 2);
        voff[j] = (unsigned)row * (unsigned)(is_a ? p.lda : p.K) * 2u + src_chunk;
    }
    // ---- fragment reads: row 16 b + lr of a 64-byte-row image, chunk lq
    const int frag = lr * 64 + ((lq ^ ((lr >> 1) & 3)) << 4);
    const char* const fa = smem + wm * 9 * 1024 + frag;
    const char* const fw = smem + (FIT_APIECES + wn * 10) * 1024 + frag;

    for (int round = 0; round < rounds; ++round) {
        const int tile = xcd_remap(blockIdx.x, grid) + round * grid;
        const int tile_m = tile / tiles_n, tile_n = tile - tile_m * tiles_n;
        const int m0 = tile_m * FIT_BM, n0 = tile_n * FIT_BN;
        const char* const a_tile = reinterpret_cast<const char*>(p.A) + (size_t)m0 * p.lda * 2;
        const char* const w_tile = reinterpret_cast<const char*>(p.W) + (size_t)n0 * p.K * 2;

        // pieces wave + 4 j: j < 4 activations, j > 4 weights, j = 4 activations for waves 0 / 1; j = 9 exists for waves 0 / 1 only
        const char* const mid_tile = wave < 2 ? a_tile : w_tile;
        auto issue1 = [&](int kt, int j) __attribute__((always_inline)) {        // j: a constant once the caller's loop is unrolled
            const unsigned dst = lds_base + (unsigned)((kt & (FIT_NST - 1)) * FIT_STAGE + wave * 1024);
            if (j < 9 || wave < 2)
                lds_dma16_keep_m0((j < 4 ? a_tile : j > 4 ? w_tile : mid_tile) + (size_t)kt * 64 + voff[j], dst + j * 4096);
        };
        auto issue = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < 10; ++j) issue1(kt, j);
        };

        f32x4_t acc[9][10];
#pragma unroll
        for (int rb = 0; rb < 9; ++rb)
#pragma unroll
            for (int cb = 0; cb < 10; ++cb) acc[rb][cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        fit_settle(acc);

        for (int t = 0; t < 3 && t < nk; ++t) issue(t);
        for (int t = 0; t < nk; ++t) {
            const int ahead = nk - 1 - t < 2 ? nk - 1 - t : 2;      // tiles issued behind tile t
            fit_wait(np * ahead);                                    // this wave's pieces of tile t are in LDS
            __syncthreads();                                         // everybody's are, and everybody is past tile t - 1
            const bool more = t + 3 < nk;                            // tile t + 3 goes into the stage of tile t - 1, a piece per
            const int st = (t & (FIT_NST - 1)) * FIT_STAGE;          // row block: in the shadow of the MFMAs, not ahead of them
            bf16x8_t wf[10], af[2];
            af[0] = *reinterpret_cast<const bf16x8_t*>(fa + st);
#pragma unroll
            for (int cb = 0; cb < 10; ++cb) wf[cb] = *reinterpret_cast<const bf16x8_t*>(fw + st + cb * 1024);
#pragma unroll
            for (int rb = 0; rb < 9; ++rb) {
                if (rb < 8) af[(rb + 1) & 1] = *reinterpret_cast<const bf16x8_t*>(fa + st + (rb + 1) * 1024);
#pragma unroll
                for (int cb = 0; cb < 10; ++cb) {
                    if (cb == 5 && more) {
                        issue1(t + 3, rb);
                        if (rb == 8) issue1(t + 3, 9);
                    }
                    if (rb < FIT_RB_A) FIT_MFMA_A(acc[rb][cb], wf[cb], af[rb & 1]);
                    else FIT_MFMA_V(acc[rb][cb], wf[cb], af[rb & 1]);
                }
            }
        }
        // ---- residual: added on the matrix pipe, acc += I x R, as gemm_persist_kernel's ring residual adds it (gemm_parts.h), so
        // that the sum (acc + residual) + bias is formed by the same units in the same order and the launches this kernel takes
        // over from that one keep their bits (a VALU add differed in 3 of 10^6 elements). A 16 rows x 32 columns fragment of
        // the residual is the activation-side operand of two MFMAs whose weight-side operand holds a 16 x 16 identity at
        // k = 0 .. 15 / 16 .. 31. A wave reads only its own 144 x 160 patch of the residual, all of it ahead of its first store.
        if (p.residual) {
            bf16x8_t idf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 8; ++e) idf[i][e] = (8 * lq + e == lr + 16 * i) ? (short)0x3F80 : (short)0;
            const bf16_t* const rsrc = p.residual + (size_t)(m0 + wm * 144 + lr) * p.ldr + n0 + wn * 160 + 8 * lq;
#pragma unroll
            for (int rb = 0; rb < 9; ++rb)
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    const bf16x8_t rf = *reinterpret_cast<const bf16x8_t*>(rsrc + (size_t)(rb * 16) * p.ldr + 32 * c);
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        if (rb < FIT_RB_A) FIT_MFMA_A(acc[rb][2 * c + i], idf[i], rf);
                        else FIT_MFMA_V(acc[rb][2 * c + i], idf[i], rf);
                    }
                }
        }
        fit_settle(acc);
        __syncthreads();                                             // the ring is free: every wave is past its last fragment

        // ---- epilogue. A lane holds, of output row 16 rb + lr of its wave, columns 16 cb + 4 lq .. + 3 of every column block.
        float* const patch = reinterpret_cast<float*>(smem + wave * FIT_PATCH);
        const int mw = m0 + wm * 144, nw = n0 + wn * 160;
        float4 b8[5][2];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int c8 = (i * 64 + lane) % 20;
            b8[i][0] = b8[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p.bias) {
                b8[i][0] = *reinterpret_cast<const float4*>(p.bias + nw + c8 * 8);
                b8[i][1] = *reinterpret_cast<const float4*>(p.bias + nw + c8 * 8 + 4);
            }
        }
#pragma unroll
        for (int rb = 0; rb < 9; ++rb) {
#pragma unroll
            for (int cb = 0; cb < 10; ++cb)
                *reinterpret_cast<f32x4_t*>(patch + lr * FIT_PROW + cb * 16 + lq * 4) = acc[rb][cb];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int slot = i * 64 + lane, row = slot / 20, c8 = slot - row * 20;
                const float4 x0 = *reinterpret_cast<const float4*>(patch + row * FIT_PROW + c8 * 8);
                const float4 x1 = *reinterpret_cast<const float4*>(patch + row * FIT_PROW + c8 * 8 + 4);
                float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                const size_t m = (size_t)(mw + rb * 16 + row);
                v[0] += b8[i][0].x; v[1] += b8[i][0].y; v[2] += b8[i][0].z; v[3] += b8[i][0].w;
                v[4] += b8[i][1].x; v[5] += b8[i][1].y; v[6] += b8[i][1].z; v[7] += b8[i][1].w;
                *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(p.C) + m * p.ldc + nw + c8 * 8) = pack_bf8(v);
            }
        }
        wait_vmcnt<0>();                 // the next round counts its LDS-DMA pieces by hand: no store may still be in flight
        __syncthreads();                 // and its first pieces land where the patches are
    }
}

int fit_cu_count() {
    static std::atomic<int> cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int n = cus[dev].load(std::memory_order_acquire);
    if (n <= 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 0;
        cus[dev].store(n, std::memory_order_release);
    }
    return n;
}

// 0, or why the shape is refused: what can be told without a device first, then (once per device) the CU count
int fit_shape(int M, int N, int K, int* cus_out) {
    if (M <= 0 || N <= 0 || K < 64 || M % FIT_BM != 0 || N % FIT_BN != 0 || K % 64 != 0) return DC_ERR_SHAPE;
    const int cus = fit_cu_count();
    if (cus <= 0) return DC_ERR_ARG;
    const long long tiles = (long long)(M / FIT_BM) * (N / FIT_BN);
    if (tiles % cus != 0) return DC_ERR_SHAPE;
    if (cus_out) *cus_out = cus;
    return 0;
}

int fit_check(const DcGemmParams* p, int* cus_out) {
    if (!p) return DC_ERR_ARG;
    if (p->mode != 0 || (p->flags & (DC_GEMM_OUT_F32 | DC_GEMM_GEGLU | DC_GEMM_GELU)) || p->rowvec || p->alpha != 1.0f) return DC_ERR_ARG;
    if (const int e = fit_shape(p->M, p->N, p->K, cus_out)) return e;
    if (!p->A || !p->W || !p->C) return DC_ERR_ARG;
    if (p->n_pad < p->N || p->lda < p->K || p->ldc < p->N || (p->residual && p->ldr < p->N)) return DC_ERR_SHAPE;
    if (p->lda % 8 != 0 || p->ldc % 8 != 0 || (p->residual && p->ldr % 8 != 0)) return DC_ERR_SHAPE;
    if ((uintptr_t)p->A % 16 != 0 || (uintptr_t)p->W % 16 != 0 || (uintptr_t)p->C % 16 != 0 || (uintptr_t)p->residual % 16 != 0 ||
        (uintptr_t)p->bias % 16 != 0)
        return DC_ERR_SHAPE;
    return 0;
}

}  // namespace

extern "C" int dc_gemm_fit_shape(int M, int N, int K) { return fit_shape(M, N, K, nullptr) == 0 ? 1 : 0; }

extern "C" int dc_gemm_fit(const DcGemmParams* p, void* stream) {
    int cus = 0;
    if (const int e = fit_check(p, &cus)) return e;
    static DcLdsOnce lds_once;
    if (const int e = lds_once.ensure(reinterpret_cast<const void*>(&gemm_fit_kernel), FIT_LDS)) return e;
    const int tiles = (p->M / FIT_BM) * (p->N / FIT_BN);
    hipLaunchKernelGGL(gemm_fit_kernel, dim3(cus), dim3(256), FIT_LDS, (hipStream_t)stream, *p, tiles / cus);
    DC_CHECK_LAUNCH();
    return 0;
}
