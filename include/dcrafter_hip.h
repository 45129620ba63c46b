/* dcrafter_hip.h — C ABI of libdcrafter_hip.so: the MI355X (gfx950) device path of the DynamiCrafter denoising
 * loop (DDIM sampler -> 3D UNet forward -> AutoencoderKL encode/decode).
 *
 * The reference (87003697/DynamiCrafter) contains no native code; its "FFI" for this path is PyTorch's ATen
 * dispatch underneath the lvdm Python classes. Each entry point below therefore names the reference call site
 * (path:line under the reference root) whose ATen ops it replaces. The Python classes in
 * the dynamicrafter_amd/lvdm package keep the reference's constructor/forward signatures and call these through ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every function returns 0 on success, a hipError_t (>0) from the launch, or a DC_ERR_* (<0) for bad arguments;
 *     nothing throws, nothing allocates, nothing synchronises: all work is enqueued on `stream` (a hipStream_t
 *     passed as void*), so every call is hipGraph-capturable.
 *   - device pointers only. bf16 = raw uint16 bits. Activations are channels-last rows: [rows, C] with
 *     row = ((b*T + t)*H + y)*W + x and `ld*` the row stride in elements.
 *   - weights are repacked once by the host: Linear [N][K] as in torch; conv3x3 [Cout][Cin/64][kh*kw][64];
 *     temporal conv [Cout][Cin/64][kt][64] (K = 64-channel slice, tap, channel); N zero-padded to a multiple of
 *     128 rows; biases/affine params fp32.
 */
#ifndef DCRAFTER_HIP_H
#define DCRAFTER_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DC_ERR_SHAPE (-1)   /* unsupported / inconsistent shape or stride */
#define DC_ERR_ARG   (-2)   /* null pointer or bad enum */

#define DC_GEMM_OUT_F32 1   /* C is float32 (no residual) */
#define DC_GEMM_GEGLU   2   /* W = [value half ; gate half] (N = 2*Nout): C = (xW_v+b_v) * gelu_erf(xW_g+b_g) */
#define DC_GEMM_GELU    4   /* C = gelu_erf(xW + b)  (Resampler FeedForward, lvdm/modules/encoders/resampler.py:27-34) */

typedef struct DcGemmParams {
    const uint16_t* A;        /* activation rows (bf16) */
    const uint16_t* W;        /* weights [n_pad][K] (bf16), rows >= N are zero */
    void* C;                  /* output rows, bf16 or f32 (flags) */
    const float* bias;        /* [N] or NULL */
    const float* rowvec;      /* optional broadcast add: rowvec[(m / rows_per_vec) * rowvec_ld + n] (timestep-embedding add) */
    const uint16_t* residual; /* optional bf16 residual rows, added after everything else */
    int lda, ldc, ldr, rowvec_ld;
    int rows_per_vec;
    int M, N, K, n_pad;
    int mode;                 /* 0 plain, 1 conv2d 3x3, 2 temporal conv 3x1x1 */
    int Cin;                  /* channels per tap (mode 1/2): K = taps*Cin */
    int IH, IW, OH, OW;       /* mode 1: source frame size (before the fused upsample) and output frame size */
    int stride, pad, ups;     /* mode 1: stride 1|2, top/left pad (bottom/right implied by OH/OW), ups=1 -> nearest x2 of the source */
    int T, HW;                /* mode 2: frames per clip, rows per frame */
    int flags;
    float alpha;              /* output scale applied last (before the residual add) */
    void* workspace;          /* optional device scratch for split-K partial sums (dc_gemm_workspace_bytes()); NULL = never split */
    long long workspace_bytes;
} DcGemmParams;

/* Name of the kernel family the last dc_gemm_conv call of this host thread dispatched to. A thread-local DIAGNOSTIC label
 * for profilers (bench.py's per-kernel table): it carries no state any compute entry reads - the compute ABI stays
 * stateless. */
const char* dc_gemm_last_variant(void);

/* Which kernels take the launches with 320-wide tiles. bit 0: the one-wave-per-SIMD kernel on v_mfma_f32_16x16x32_bf16
 * (gemm_pipe16.h: activations straight into registers, no barrier in the K loop) for the 3x3 convs, bit 1: also for plain /
 * temporal launches with K >= 1920; bit 4 (16): the ping-pong kernel (gemm_pp.h: 4-wave workgroups, two per CU, whose epilogues
 * overlap each other's K loops) for GEGLU projections with K <= 640, bit 5 (32): for any K. Default 19 (bits 0, 1, 4): the matrix
 * pipe is power-managed on MI355X and holds a higher clock on the 16x16x32 shape. 0 = the 8-wave LDS-DMA kernels everywhere. Bit 3 is accepted and ignored (it once chose between
 * the two MFMA shapes of that kernel: plans 9 / 11 = 1 / 3); bit 2 is rejected (the 32x32x16 form and the LDS-window conv kernel
 * lost every measured shape and live in tools/experimental); bit 6 (64): the split-K plans "whole waves of tiles + the remainder
 * cut along K" as two launches instead of one (bit-identical results: tests, A/B); bit 7 (128): the narrow-output 3x3 conv kernel
 * (N <= 16: conv_out of the UNet and of the AE decoder) off, the tile kernels take those launches; bit 8 (256): likewise without the window kernel for N = 128 (the AE's
 * full-resolution ResnetBlock convs). All plans give the same results to bf16 rounding and each is
 * bit-reproducible. Process-wide (env DC_GEMM_PLAN sets the initial value, validated the same way). Returns the previous plan,
 * or DC_ERR_ARG. */
int dc_gemm_set_plan(int plan);

/* Recommended size of DcGemmParams.workspace (one buffer per stream; contents are scratch, no initialisation). */
int64_t dc_gemm_workspace_bytes(void);

/* Linear / 1x1 conv / conv2d 3x3 / Conv3d(3,1,1) on MFMA.
 * replaces: nn.Linear  lvdm/modules/attention.py:53-57,75-76,269,290,336,362,418,438
 *           nn.Conv2d  lvdm/modules/networks/openaimodel3d.py:68,96,154,179,187,386,545 (+F.interpolate :103 when ups=1)
 *           nn.Conv3d  lvdm/modules/networks/openaimodel3d.py:255-266
 *           nn.Conv2d  lvdm/modules/networks/ae_modules.py:31-50,96-106,117-126,161-186 ; lvdm/models/autoencoder.py:34-35
 *           GEGLU      lvdm/modules/attention.py:415-422 (DC_GEMM_GEGLU) */
int dc_gemm_conv(const DcGemmParams* p, void* stream);

/* The exact-fit GEMM (gemm_fit.hip): C[M,N] = A[M,K] W[N,K]^T (+ bias) (+ bf16 residual), bf16 output, fp32 accumulation, in
 * 288 x 320 output tiles, one workgroup per CU, for launches whose (M / 288) (N / 320) tiles are a whole number of rounds over
 * the device's CUs (queried at run time): no ragged last round, no split-K. Operands as dc_gemm_conv takes them in mode 0 (lda /
 * ldc / ldr row strides, W bf16 [n_pad][K]); bias and residual are added in fp32 and the sum is rounded once; C may be the
 * residual. Refuses, before any launch, with DC_ERR_ARG: mode != 0, fp32 output, GEGLU, GELU, a row vector, alpha != 1, a null
 * operand, no usable device; with DC_ERR_SHAPE: M % 288, N % 320 or K % 64 != 0, a tile count that is no multiple of the CU count,
 * row strides that are no multiple of 8 elements, or operands that are not 16-byte aligned.
 * dc_gemm_fit_shape answers 1 when [M x N x K] passes the shape rules on the current device, else 0, and launches nothing.
 * replaces: nn.Linear lvdm/modules/attention.py:53-57,75-76,269,290,336,362,438 and the 1x1 nn.Conv2d skip_connection
 *           lvdm/modules/networks/openaimodel3d.py:187 at the UNet's native resolution */
int dc_gemm_fit(const DcGemmParams* p, void* stream);
int dc_gemm_fit_shape(int M, int N, int K);

/* GroupNorm (+ optional SiLU) over channels-last rows; statistics in fp32.
 * One "instance" = rows_per_inst consecutive rows sharing statistics: H*W for the 4-D norms, T*H*W for the 5-D
 * norms of TemporalConvBlock / TemporalTransformer.
 * replaces: GroupNormSpecific lvdm/basics.py:76-87; nn.GroupNorm openaimodel3d.py:256-265, attention.py:265,331;
 *           Normalize + nonlinearity lvdm/modules/networks/ae_modules.py:10-16
 * workspace: dc_groupnorm_workspace_bytes() bytes of device scratch. */
int dc_groupnorm(const uint16_t* x, int ldx, uint16_t* y, int ldy, const float* gamma, const float* beta,
                 int C, int groups, int n_inst, int rows_per_inst, float eps, int silu,
                 float* workspace, void* stream);
int64_t dc_groupnorm_workspace_bytes(int n_inst, int groups, int rows_per_inst);

/* LayerNorm over the last dim of [rows, C]. replaces nn.LayerNorm lvdm/modules/attention.py:225-227 */
int dc_layernorm(const uint16_t* x, int ldx, uint16_t* y, int ldy, const float* gamma, const float* beta,
                 int rows, int C, float eps, void* stream);

/* LayerNorm + spatial token pooling: the K/V tokens of a spatial self-attention with token downsampling ("ToDo", Smith et
 * al., IJCAI 2024; not in the reference). x: bf16 rows [F*H*W][ldx], rows ordered (frame, y, x'); y: bf16 rows [F*Hp*Wp][ldy]
 * with Hp = ceil(H / factor), Wp = ceil(W / factor), ordered (frame, yp, xp); gamma / beta fp32 [C].
 *   mode 0 (nearest): y[yp][xp] = LN(x[yp factor][xp factor]), the strided slice n[::f, ::f]; only the kept rows are read and the
 *                     output equals the corresponding rows of dc_layernorm bit for bit.
 *   mode 1 (mean):    y[yp][xp] = mean of LN(x[.][.]) over the cell [yp factor, min(H, yp factor + factor)) x [xp factor, min(W,
 *                     xp factor + factor)): each token normalised in fp32, summed in (y, x') order, times 1 / (tokens in the
 *                     cell), one rounding to bf16 (avg_pool2d with ceil_mode=True, count_include_pad=False).
 * One wave per output token, 16-byte loads and stores, no atomics, no scratch: capturable, bit-reproducible.
 * DC_ERR_ARG: a null pointer. DC_ERR_SHAPE: C % 8 != 0 or C > 2048 (dc_layernorm's limits), a row stride that is no multiple
 * of 8 or below C, x or y not 16-byte aligned, F, H or W < 1, F*H*W >= 2^31, factor outside 2..8, mode outside {0, 1}.
 * replaces, for to_k / to_v of attn1 only, nn.LayerNorm norm1 lvdm/modules/attention.py:225-227,243 followed by the slice or
 * F.avg_pool2d of the token grid that the published ToDo patch applies ahead of CrossAttention.to_k / to_v (:75-76) */
int dc_ln_pool_tokens(const uint16_t* x, int ldx, uint16_t* y, int ldy, const float* gamma, const float* beta, int F, int H,
                      int W, int C, int factor, int mode, float eps, void* stream);

/* softmax(q k^T * scale) v, head_dim 64, flash-style (no score matrix in HBM).
 * q rows: [batch][Lq] at q + (b*q_bstride + i)*ldq + h*64 ; k/v rows: [batch][Lk] likewise with kv_bstride.
 * accumulate != 0: o += acc_scale * result (image cross-attention branch), else o = result.
 * All row strides % 8 == 0 and q/k/v/o 16-byte aligned (16-byte loads and stores).
 * replaces: CrossAttention.forward core lvdm/modules/attention.py:101-142 (einsum/softmax/einsum, and the
 *           xformers path :166-207) for spatial self-attention and text / image cross-attention. */
int dc_flash_attn_d64(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* o,
                      int ldq, int ldk, int ldv, int ldo, int batch, int heads, int Lq, int Lk,
                      int64_t q_bstride, int64_t kv_bstride, float scale, int accumulate, float acc_scale,
                      void* stream);

/* Test / measurement hook for the long self-attention path of dc_flash_attn_d64 (Lq >= 512, Lk >= 256, Lk % 64 == 0, no
 * accumulate: the one-wave-per-SIMD pipelined kernel, which runs softmax without a running maximum and repeats a workgroup's
 * block with a running-max pass when a row sum leaves [2^-100, 2^100)). mode bit 0: run the running-max pass directly; bit 1:
 * two 32-row query blocks per wave for every shape (default: three when Lq % 384 == 0); thr (0..64, exp2 units): how far a
 * score must exceed the running max before that pass rescales its state. Process-wide (atomics: a launch reads each once);
 * default mode 0, thr 8. Returns 0 or DC_ERR_ARG (mode outside 0..3). */
int dc_flash_attn_set_mode(int mode, float thr);

/* Temporal self-attention over T <= 16 frames, head_dim 64: for every (clip b, position p, head h) the T rows
 * (b, t, p) attend to each other. qkv rows are [q | k | v] (3*heads*64 wide, row stride ld).
 * replaces: CrossAttention.forward lvdm/modules/attention.py:81-144 as used by TemporalTransformer :365-412. */
int dc_temporal_attn_d64(const uint16_t* qkv, int ld, uint16_t* o, int ldo, int B, int T, int HW, int heads,
                         float scale, void* stream);

/* out[m][n] = act_out( bias[n] + sum_k act_in(in[m][k]) * W[n][k] ), m < 8; in/out fp32, W bf16.
 * act: 0 none, 1 SiLU. accumulate: out += result.
 * replaces: time_embed / fps_embedding MLPs openaimodel3d.py:370-382,551,575 and ResBlock emb_layers :168-174,219 */
int dc_gemv_small(const float* in, int ld_in, const uint16_t* W, const float* bias, float* out, int ld_out,
                  int M, int N, int K, int act_in, int act_out, int accumulate, void* stream);

/* Sinusoidal embedding: out[b][0:half]=cos(t_b*f_i), out[b][half:]=sin(t_b*f_i), f_i=exp(-ln(max_period)*i/half).
 * t is read from device memory: t_table[t_index[0]*t_stride + b] if t_index != NULL else t_table[b].
 * replaces: timestep_embedding lvdm/models/utils_diffusion.py:8-28 */
int dc_timestep_embedding(const int64_t* t_table, const int32_t* t_index, int t_stride, float* out, int B, int dim,
                          float max_period, void* stream);

/* UNet input assembly: cat([x, c_concat], dim=1) of [B,Cx,T,H,W] + [B,Cc,T,H,W] fp32 tensors -> channels-last
 * bf16 rows [nrep*B*T*H*W, c_pad] (channels >= Cx+Cc zeroed); the batch is written nrep times (nrep=2 serves
 * the cond/uncond pair of classifier-free guidance from one latent).
 * replaces: torch.cat ddpm3d.py:1256 + rearrange openaimodel3d.py:566 */
int dc_pack_latent(const float* x, const float* cc, uint16_t* out, int B, int Cx, int Cc, int T, int HW,
                   int c_pad, int nrep, void* stream);

/* dc_pack_latent for a set of overlapping T-frame windows of a clip of T_long > T frames (temporal co-denoising: the UNet
 * denoises windows of one long latent, their outputs are blended where they overlap - dc_window_merge - and the sampler's
 * update runs once on the long latent). x [B,Cx,T_long,H,W], cc [B,Cc,T_long,H,W] fp32 -> channels-last bf16 rows
 * [(rep, b, w, f, p)][c_pad] for the windows w = w0 .. w0+n_w-1 of one step: frame f of window w is long frame
 * starts[step*W + w] + f, channels >= Cx+Cc zeroed; (b, w) is the clip index of the UNet batch (B*n_w clips). starts: int32
 * [S][W] device table, every entry in [0, T_long-T]; step = step_index[0] (device counter) or `index`, < S. The per-element
 * conversion is dc_pack_latent's: for the gathered frames the rows are bit-identical to dc_pack_latent on a gathered tensor.
 * no reference call site (the reference samples T frames only): MultiDiffusion, Bar-Tal et al., arXiv:2302.08113, applied
 * along time as in Gen-L-Video, Wang et al., arXiv:2305.18264 */
int dc_pack_latent_windows(const float* x, const float* cc, uint16_t* out, const int32_t* starts,
                           const int32_t* step_index, int index, int S, int W, int w0, int n_w, int B, int Cx, int Cc,
                           int T_long, int T, int HW, int c_pad, int nrep, void* stream);

/* Blend of the UNet's window outputs onto the long clip. e: fp32 rows [(k, b, w, f, p)][ld_e] (nb branches k, n_w windows,
 * first C channels valid) -> out: fp32 rows [(k, b, F, p)][ld_out], which dc_ddim_step / dc_dpmpp_step read as branch k at
 * row offset k*B*T_long*HW with THW = T_long*HW:
 *   out[k,b,F,p,c] = sum_w wn[(step*W + w)*T + F - starts[step*W + w]] * e[k,b,w,F - starts[step*W + w],p,c]
 * over the windows w0 <= w < w0+n_w that contain F, summed in ascending w (first term a product, then fused multiply-adds);
 * a term of weight 0 (padding window) is skipped and its e never read. Any two runs agree bitwise and a single window of
 * weight 1 returns its input. accumulate == 0 writes (0 where no window of the call covers F), != 0 adds to what out holds:
 * windows evaluated in chunks of n_w give the unchunked values (equal as numbers; a frame whose first term comes in a later
 * chunk receives it through a multiply-add onto +0, so a -0 product becomes +0). wn: fp32 [S][W][T] device table, normalised so that the weights of the windows containing a frame sum to 1.
 * no reference call site: arXiv:2302.08113 (eq. 5, the closed-form blend), arXiv:2305.18264 */
int dc_window_merge(const float* e, int ld_e, float* out, int ld_out, const int32_t* starts, const float* wn,
                    const int32_t* step_index, int index, int S, int W, int w0, int n_w, int nb, int B, int C, int T_long,
                    int T, int HW, int accumulate, void* stream);

/* dc_pack_latent for boxes of the UNet's own extent (T, H, Wd) inside a latent of (T_long, H_long, W_long) (spatially tiled
 * sampling: frames larger than the trained size; the time axis may be tiled as well). x [B,Cx,T_long,H_long,W_long],
 * cc [B,Cc,T_long,H_long,W_long] fp32 -> channels-last bf16 rows [(rep, b, w, f, y, x)][c_pad] for the boxes
 * w = w0 .. w0+n_w-1 of one step: position (f, y, x) of box w is long position (t0 + f, y0 + y, x0 + x) with
 * (t0, y0, x0) = box[(step*W + w)*3 ..], channels >= Cx+Cc zeroed; (b, w) is the clip index of the UNet batch. box: int32
 * [S][W][3] device table, every start in [0, long - extent] of its axis (one outside is clamped into it);
 * step = step_index[0] (device counter) or `index`; a counter outside [0, S) launches nothing. The per-element conversion is
 * dc_pack_latent's: every row is bit-identical to dc_pack_latent on the cropped tensors.
 * no reference call site (the reference samples one latent size per config): MultiDiffusion, Bar-Tal et al.,
 * arXiv:2302.08113 */
int dc_pack_latent_tiles(const float* x, const float* cc, uint16_t* out, const int32_t* box, const int32_t* step_index,
                         int index, int S, int W, int w0, int n_w, int B, int Cx, int Cc, int T_long, int H_long,
                         int W_long, int T, int H, int Wd, int c_pad, int nrep, void* stream);

/* Blend of the UNet's box outputs onto the long latent. e: fp32 rows [(k, b, w, f, y, x)][ld_e] (nb branches k, n_w boxes,
 * first C channels valid) -> out: fp32 rows [(k, b, F, Y, X)][ld_out], which dc_ddim_step / dc_dpmpp_step read as branch k at
 * row offset k*B*T_long*H_long*W_long:
 *   out[k,b,F,Y,X,c] = sum_w fl(fl(gt_w[F - t0_w] * gy_w[Y - y0_w]) * gx_w[X - x0_w]) * e[k,b,w,F - t0_w,Y - y0_w,X - x0_w,c]
 * over the boxes w0 <= w < w0+n_w that contain (F, Y, X), in ascending w (first term a product, then fused multiply-adds);
 * fl is rounding to fp32 and (gt_w | gy_w | gx_w) = g[(step*W + w)*(T+H+Wd) ..], the box's three per-axis weight vectors.
 * A term of weight 0 (padding box) is skipped and its e never read. Any two runs agree bitwise and a single box of weight 1
 * returns its input, the sign of zero included. accumulate == 0 writes (0 where no box of the call covers the position),
 * != 0 adds to what out holds: boxes evaluated in chunks of n_w give the unchunked values (equal as numbers; a position whose
 * first term comes in a later chunk receives it through a multiply-add onto +0, so a -0 product becomes +0). g: fp32
 * [S][W][T+H+Wd] device table, each axis normalised so that the product weights of the boxes containing a position sum to 1.
 * no reference call site: arXiv:2302.08113 (eq. 5, the closed-form blend) */
int dc_tile_merge(const float* e, int ld_e, float* out, int ld_out, const int32_t* box, const float* g,
                  const int32_t* step_index, int index, int S, int W, int w0, int n_w, int nb, int B, int C, int T_long,
                  int H_long, int W_long, int T, int H, int Wd, int accumulate, void* stream);

/* Generic layout helpers (channels-last bf16 <-> NCHW fp32), used at the AutoencoderKL boundary.
 * nchw_to_rows: x[N][C][HW] fp32 -> rows[N*HW][c_pad] bf16 (scaled by `scale`, pad channels zero)
 * rows_to_nchw: rows[N*HW][ld] (bf16 or f32) -> y[N][C][HW] fp32 */
int dc_nchw_to_rows(const float* x, uint16_t* out, int N, int C, int HW, int c_pad, float scale, void* stream);
int dc_rows_to_nchw(const void* rows, int ld, int rows_f32, float* y, int N, int C, int HW, float scale, void* stream);

/* im2col for a 3x3 / stride 1 / pad 1 conv with <= 8 input channels (the UNet's conv_in: 4 latent + 4 concat channels,
 * openaimodel3d.py:379-381 `conv_nd(dims, in_channels, model_channels, 3, padding=1)`): x rows [n_img*H*W][ldx] bf16 whose first
 * 8 channels are read -> out rows [n_img*H*W][ldo >= 128]: elements 8 t .. 8 t + 7 = the 8 channels of tap t = kh*3 + kw (zeros
 * outside the image), elements 72 .. 127 zero. The conv is then dc_gemm_conv (mode 0) on these rows with the weight reordered to
 * [Cout][128] (k = 8 (kh*3 + kw) + c): two K tiles instead of nine, each eight times denser. */
int dc_im2col3x3_c8(const uint16_t* x, int ldx, uint16_t* out, int ldo, int n_img, int H, int W, void* stream);

/* 2-D strided copy of bf16 rows (skip-connection concat: torch.cat openaimodel3d.py:596). cols % 8 == 0. */
int dc_copy2d(const uint16_t* src, int lds, uint16_t* dst, int ldd, int rows, int cols, void* stream);

/* Per-frame context assembly: context [B, 77 + T*L, D] fp32 -> [B*T, 77+L, D] bf16 where frame (b,t) gets the
 * 77 text tokens of b followed by image tokens t*L..t*L+L-1. replaces openaimodel3d.py:555-562 */
int dc_build_context(const float* ctx, uint16_t* out, int B, int T, int n_text, int L, int D, void* stream);

/* Row softmax fp32 -> bf16 (AutoencoderKL mid attention, ae_modules.py:68). */
int dc_softmax_rows(const float* x, int ldx, uint16_t* y, int ldy, int rows, int cols, void* stream);

/* dst[c][r] = src[r][c] on bf16 rows (V^T operand of the AutoencoderKL mid attention, ae_modules.py:71-74). */
int dc_transpose(const uint16_t* src, int lds, uint16_t* dst, int ldd, int rows, int cols, void* stream);

/* y = a + b elementwise on bf16 rows (AE residual adds where no GEMM epilogue is available). */
int dc_add_rows(const uint16_t* a, int lda, const uint16_t* b, int ldb, uint16_t* y, int ldy, int rows, int cols,
                void* stream);

/* DiagonalGaussianDistribution.sample x scale_factor: moments rows [N*HW][ld] (mean | logvar, zc channels each)
 * -> z[N][zc][HW] fp32 = scale * (mean + exp(0.5*clamp(logvar,-30,20)) * noise[N][zc][HW]); noise NULL -> mode().
 * replaces lvdm/distributions.py:25-40 + ddpm3d.py:611-618 */
int dc_vae_sample(const uint16_t* moments, int ld, const float* noise, float* z, int N, int zc, int HW,
                  float scale, void* stream);

typedef struct DcDdimParams {
    /* per-step scalar tables, indexed by step_index[0] (device) when step_index != NULL, else by `index` */
    const float* a_t;            /* ddim_alphas[index]            (fp32 as torch.full casts them, ddim.py:251) */
    const float* a_prev;         /* ddim_alphas_prev[index] */
    const float* sigma_t;        /* ddim_sigmas[index] */
    const float* sqrt_one_minus_at;
    const float* sqrt_acp_t;     /* model.sqrt_alphas_cumprod[t]           (v-param, ddpm3d.py:239-251) */
    const float* sqrt_1macp_t;   /* model.sqrt_one_minus_alphas_cumprod[t] */
    const float* scale_ratio;    /* ddim_scale_arr_prev[index]/ddim_scale_arr[index] or NULL (ddim.py:262-266) */
    const int32_t* step_index;   /* device counter or NULL */
    int index;
    int v_param;                 /* parameterization == "v" */
    float cfg_scale;             /* unconditional_guidance_scale; e_uncond may be NULL when 1.0 */
    float cfg_img;               /* 3-branch CFG (ddim_multiplecond.py:234); used when e_img != NULL */
    float guidance_rescale;      /* 0 -> off */
    float temperature;
    int e_nchw;                  /* 0: e_* are channels-last rows [B*T*HW, ld_e]; 1: e_* are [B, C, T*HW] like x */
    int64_t noise_step_stride;   /* with step_index: noise for this step starts at noise + step_index[0]*stride */
} DcDdimParams;

/* One DDIM update for B clips. e_* are the UNet outputs as channels-last fp32 rows [B*T*HW, ld_e] (first C
 * channels valid); x, noise, x_prev, pred_x0 are [B, C, T*HW] fp32 (the reference's NCTHW layout).
 * workspace: >= 16 * B * 256 floats.
 * replaces: p_sample_ddim lvdm/models/samplers/ddim.py:226-277 + rescale_noise_cfg utils_diffusion.py:147-157 */
int dc_ddim_step(const DcDdimParams* p, const float* e_cond, const float* e_uncond, const float* e_img, int ld_e,
                 const float* x, const float* noise, float* x_prev, float* pred_x0, int B, int C, int THW,
                 float* workspace, void* stream);

typedef struct DcInvertParams {
    /* per-step fp32 tables in execution order, which for an inversion is ASCENDING DDIM index k; indexed by
     * step_index[0] (device) when step_index != NULL, else by `index`. Host float64 -> fp32 (samplers/ddim.py). */
    const float* sqrt_a_src;     /* sqrt(ap[k]): model.sqrt_alphas_cumprod[t_src[k]], t_src[0] = 0, else ddim_timesteps[k-1] */
    const float* sqrt_1ma_src;   /* sqrt(1 - ap[k]): model.sqrt_one_minus_alphas_cumprod[t_src[k]] */
    const float* sqrt_a_dst;     /* sqrt(ddim_alphas[k]) */
    const float* sqrt_1ma_dst;   /* sqrt(1 - ddim_alphas[k]) */
    const float* scale_ratio;    /* r[k] = ddim_scale_arr_prev[k]/ddim_scale_arr[k], or NULL (r = 1) */
    const int32_t* step_index;   /* device counter or NULL */
    int index;
    int v_param;
    float cfg_scale;
    float cfg_img;
    float guidance_rescale;
    int e_nchw;                  /* as DcDdimParams */
} DcInvertParams;

/* One DDIM inversion step for B clips: the latent x at level ap[k] = ddim_alphas_prev[k] goes to level
 * a[k] = ddim_alphas[k], the deterministic forward pass the reference leaves as a TODO
 * ("# TODO: deterministic forward pass? <ddim inversion>", lvdm/models/samplers/ddim.py:179). The reference has no
 * call site for it. With mo = CFG combine of e_cond [, e_uncond, e_img] followed by guidance rescale, formed exactly
 * as dc_ddim_step forms it, the UNet having been evaluated on x at t_src[k]:
 *   v:    eps = sqrt(ap) mo + sqrt(1 - ap) x,    x0s = sqrt(ap) x - sqrt(1 - ap) mo
 *   eps:  eps = mo,                              x0s = (x - sqrt(1 - ap) eps) / sqrt(ap)
 *   x_next = sqrt(a[k]) (x0s / r[k]) + sqrt(1 - a[k]) eps,    pred_x0 = x0s
 * For equal eps this is the algebraic inverse of dc_ddim_step at eta = 0, the dynamic rescale included. ap[k] > 0 for
 * every k; with zero-terminal SNR the last a[k] is 0 and x_next = eps. Operands as in dc_ddim_step without the noise
 * (x and x_next may alias). workspace: >= 16 * B * 256 floats. */
int dc_ddim_invert_step(const DcInvertParams* p, const float* e_cond, const float* e_uncond, const float* e_img,
                        int ld_e, const float* x, float* x_next, float* pred_x0, int B, int C, int THW,
                        float* workspace, void* stream);

typedef struct DcDpmParams {
    /* per-step fp32 tables in execution order, indexed by step_index[0] (device) when step_index != NULL, else by
     * `index`. The solver's own tables (host float64 -> fp32, samplers/dpm_solver.py): */
    const float* A;              /* sigma_p/sigma_t (2M) or (sigma_p/sigma_t) e^-h (2M SDE) */
    const float* alpha_t;        /* sqrt(ddim_alphas[index]) */
    const float* alpha_p_r;      /* sqrt(ddim_alphas_prev[index]) * r, r = scale_arr_prev/scale_arr or 1 */
    const float* k;              /* second-order weight 1/(2 rho); 0 -> first order (the previous x0 is not read) */
    const float* N;              /* noise coefficient sigma_p sqrt(1 - e^-2h) (2M SDE) or NULL (2M) */
    /* the DDIM sampler's tables, for the model-output conversion (same fp32 values dc_ddim_step reads): */
    const float* sqrt_one_minus_at;  /* sigma_t (eps-param) */
    const float* sqrt_acp_t;         /* model.sqrt_alphas_cumprod[t]           (v-param) */
    const float* sqrt_1macp_t;       /* model.sqrt_one_minus_alphas_cumprod[t] (v-param) */
    const float* scale_ratio;        /* r for pred_x0 = r x0_i, or NULL (r = 1) */
    const int32_t* step_index;   /* device counter or NULL */
    int index;
    int v_param;
    float cfg_scale;
    float cfg_img;
    float guidance_rescale;
    float temperature;
    int e_nchw;                  /* as DcDdimParams */
    int64_t noise_step_stride;   /* with step_index: noise for this step starts at noise + step_index[0]*stride */
    float* x0_hist;              /* ring [2][B*C*THW] fp32 of raw data predictions: step i reads slot (i-1)&1, writes slot i&1 */
} DcDpmParams;

/* One DPM-Solver++ (2M / 2M SDE) multistep update for B clips, in the data-prediction form
 *   x0_i  = raw data prediction (after CFG and guidance rescale, before dynamic rescale)
 *   D     = (1 + k) x0_i - k x0_{i-1}
 *   x_prev = A (x - alpha_t D) + alpha_p_r D + N temperature noise
 * which is dc_ddim_step's eta = 0 update when k = 0 and A = sigma_p/sigma_t. Operands as in dc_ddim_step (x and x_prev
 * may alias); pred_x0 receives r x0_i (dc_ddim_step's pred_x0); noise may be NULL when p->N is NULL.
 * workspace: >= 16 * B * 256 floats.
 * replaces (generalises): p_sample_ddim lvdm/models/samplers/ddim.py:226-277 + rescale_noise_cfg
 * utils_diffusion.py:147-157 (multistep solver: Lu et al., DPM-Solver++, arXiv:2211.01095, Alg. 2) */
int dc_dpmpp_step(const DcDpmParams* p, const float* e_cond, const float* e_uncond, const float* e_img, int ld_e,
                  const float* x, const float* noise, float* x_prev, float* pred_x0, int B, int C, int THW,
                  float* workspace, void* stream);

typedef struct DcSdsParams {
    /* per-step fp32 tables, indexed by k = step_index[0] (device) when step_index != NULL, else by `index`; host-side
     * values as torch computes them (samplers/sds.py). Per clip b: entry [k * B + b]. */
    const float* c1;             /* [S][B] sqrt(alphas_cumprod[t]) */
    const float* c2;             /* [S][B] sqrt(1 - alphas_cumprod[t]) */
    const float* w;              /* [S][B] 1 - alphas_cumprod[t] ("t" weighting; may be NULL otherwise) */
    const float* step_size;      /* [S] lr / (1 - beta1^n), n = k + 1 */
    const float* bc2_sqrt;       /* [S] sqrt(1 - beta2^n) */
    const int32_t* step_index;   /* device counter or NULL */
    int index;
    int weight_type;             /* 0 "t": w d, 1 "ada": d / max(mean|d|, 1e-4) per clip, 2 "uniform": d */
    int x0_param;                /* 0: x0 = (x_t - c2 e) / c1 (the reference's formula), 1: x0 = c1 x_t - c2 e (v) */
    int e_nchw;                  /* as DcDdimParams */
    float cfg_scale;             /* CFG applied when e_uncond != NULL and cfg_scale > 1 */
    float guidance_rescale;      /* 0 -> off */
    float beta2, eps;            /* Adam's beta2 and eps */
    float one_minus_beta1;       /* 1 - beta1 and 1 - beta2, rounded from double as torch.optim rounds them */
    float one_minus_beta2;
    float decay;                 /* 1 - lr * weight_decay (AdamW), 1 (Adam) */
    float grad_scale;            /* 1 / (B * N), N = numel(latent): the gradient of 0.5 mse / B */
    int64_t noise_step_stride;   /* dc_sds_noise with step_index: noise for step k starts at noise + k * stride */
    float* loss;                 /* [S] fp32: loss[k] = 0.5 mean(grad^2) / B; NULL -> not written */
} DcSdsParams;

/* SDS noising pass: x_t[b] = c1[k,b] latent[b] + c2[k,b] noise[k] for B clips of n_per_clip fp32 elements each.
 * latent is not written. replaces: DynamiCrafterGuidancePipeline._add_noise guidance_pipeline.py:304-324 */
int dc_sds_noise(const DcSdsParams* p, const float* latent, const float* noise, float* x_t, int B, int64_t n_per_clip,
                 void* stream);

/* SDS gradient + Adam / AdamW step on the latent [B, C, T*HW] fp32 in place, with its moments m, v (same shape).
 * e_cond / e_uncond are the UNet outputs as in dc_ddim_step (channels-last rows unless p->e_nchw; e_uncond may be
 * NULL); x_t is the noised latent of dc_sds_noise. Per element: e = CFG [+ guidance rescale], x0, d = latent - x0,
 * grad = nan_to_num(weight(d)), g = grad_scale grad, then torch.optim.Adam(W)'s update with n = k + 1; loss[k] gets
 * 0.5 sum(grad^2) grad_scale. workspace: >= 16 * B * 256 floats.
 * replaces: DynamiCrafterGuidancePipeline._sds_loss + _apply_guidance_rescale guidance_pipeline.py:326-424 and the
 * loss.backward() / optimizer.step() of _optimization_loop :759-808 */
int dc_sds_step(const DcSdsParams* p, const float* e_cond, const float* e_uncond, int ld_e, const float* x_t,
                float* latent, float* m, float* v, int B, int C, int THW, float* workspace, void* stream);

/* DynamiCrafter's dual cross-attention in one launch: o = softmax(s q k^T) v + scale2 * softmax(s q k2^T) v2 with two
 * independent softmaxes (text keys Lk, image keys Lk2) over the same queries; head_dim 64. q/o rows as in
 * dc_flash_attn_d64; k, v, k2, v2 rows share the stride ldkv and the batch stride kv_bstride (views into one fused
 * projection buffer). replaces CrossAttention.forward lvdm/modules/attention.py:128-142 (image_cross_attention) */
int dc_cross_attn_dual_d64(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* k2, const uint16_t* v2,
                           uint16_t* o, int ldq, int ldkv, int ldo, int batch, int heads, int Lq, int Lk, int Lk2,
                           int64_t q_bstride, int64_t kv_bstride, float scale, float scale2, void* stream);

/* Fused GEGLU FeedForward for dim = 320: out[M,320] = ((n W1v^T + b1v) * gelu(n W1g^T + b1g)) W2^T + b2 (+ residual),
 * n = x, or LayerNorm(x; ln_gamma, ln_beta, ln_eps) when ln_gamma != NULL (rounded to bf16 like dc_layernorm's output);
 * the [M,1280] intermediate never leaves the CU. x/out/residual: bf16 rows (ld % 8 == 0; residual may alias out and x).
 * w1: ff.net.0.proj.weight as dc_gemm_conv takes it, bf16 [>= 2560][320] (rows 0..1279 value, 1280..2559 gate), b1 fp32
 * [2560]; w2p: ff.net.2.weight bf16 [>= 320][1280] with the K order permuted inside every 32-channel chunk: position
 * 16 s + 8 h + e of a chunk holds channel 8 (2 s + e / 4) + 4 h + e % 4 (s, h in {0,1}, e in 0..7); b2 fp32 [320].
 * replaces FeedForward(GEGLU) lvdm/modules/attention.py:415-442 with norm3 and the residual add of
 * BasicTransformerBlock._forward :246 (x = ff(norm3(x)) + x) */
int dc_ff_geglu_fused320(const uint16_t* x, int ldx, const float* ln_gamma, const float* ln_beta, float ln_eps,
                         const uint16_t* w1, const float* b1, const uint16_t* w2p, const float* b2, const uint16_t* residual,
                         int ldr, uint16_t* out, int ldo, int M, void* stream);

/* dc_ff_geglu_fused320 with the transformer's proj_out behind it: out = residual2 + h2 wp^T + bp, h2 = x + FeedForward(norm3(x))
 * (h2 itself is not stored). wp: proj_out.weight bf16 [>= 320][320] with the k order of w2p inside every 32-chunk; bp fp32
 * [320]; residual2 (the transformer's input) / out: bf16 rows; out may alias residual2 but not x.
 * replaces BasicTransformerBlock._forward :246 + SpatialTransformer.forward :307-310 / TemporalTransformer.forward :404-412
 * (proj_out and the `+ x_in`) of lvdm/modules/attention.py at the UNet's level 0 */
int dc_ff_geglu_proj_fused320(const uint16_t* x, int ldx, const float* ln_gamma, const float* ln_beta, float ln_eps,
                              const uint16_t* w1, const float* b1, const uint16_t* w2p, const float* b2, const uint16_t* wp,
                              const float* bp, const uint16_t* residual2, int ldr2, uint16_t* out, int ldo, int M, void* stream);

/* Norm + Linear for dim K = 320 or 640: out[M,N] = n W^T (+ bias), N % 32 == 0; x/out: bf16 rows (ld % 8 == 0, 16-byte
 * aligned); w: bf16 [>= N][K] as dc_gemm_conv takes a Linear weight; bias fp32 [N] or NULL. The normalised rows live in
 * registers only (rounded to bf16 where dc_layernorm / dc_groupnorm round their outputs).
 * dc_ln_linear: n = x, or LayerNorm(x; ln_gamma, ln_beta, ln_eps) when ln_gamma != NULL.
 *   replaces norm1 -> attn1.to_q/k/v (one [3K, K] weight) and norm2 -> attn2.to_q of BasicTransformerBlock._forward
 *   lvdm/modules/attention.py:242-245 (CrossAttention.forward :101-105) at the UNet's levels 0 and 1
 * dc_gn_linear: n = GroupNorm(x) (no activation) with the statistics computed by dc_groupnorm_stats (fp32
 *   [n_inst][groups][2] = mean, rstd); rows_per_inst % 128 == 0 and M % rows_per_inst == 0 (a 128-row tile never straddles
 *   two instances).
 *   replaces SpatialTransformer.forward norm -> proj_in lvdm/modules/attention.py:296-301 and TemporalTransformer.forward
 *   norm -> proj_in :367-377 */
int dc_ln_linear(const uint16_t* x, int ldx, int K, const float* ln_gamma, const float* ln_beta, float ln_eps, const uint16_t* w,
                 const float* bias, uint16_t* out, int ldo, int M, int N, void* stream);
int dc_groupnorm_stats(const uint16_t* x, int ldx, int C, int groups, int n_inst, int rows_per_inst, float eps,
                       float* workspace, float* stats_out, void* stream);
int dc_gn_linear(const uint16_t* x, int ldx, int K, const float* gamma, const float* beta, const float* stats, int groups,
                 int rows_per_inst, const uint16_t* w, const float* bias, uint16_t* out, int ldo, int M, int N, void* stream);

/* out[M,N] = residual + x W^T + bias for K = 320 or 640 (N % 32 == 0; rows bf16, ld % 8 == 0, 16-byte aligned; residual may
 * alias out): the activation rows of a workgroup stay in registers (the kernel of dc_ln_linear without a norm), the residual
 * rows are fetched a chunk ahead in the stores' coalesced pattern and added in fp32 (one rounding).
 *   replaces attn1 / attn2 .to_out[0] + the residual add of BasicTransformerBlock._forward lvdm/modules/attention.py:242-245
 *   (CrossAttention.forward :143-144) and proj_out + x_in of SpatialTransformer / TemporalTransformer.forward :309-310, :404-412
 *   at the UNet's levels 0 and 1 */
int dc_linear_residual(const uint16_t* x, int ldx, int K, const uint16_t* w, const float* bias, const uint16_t* residual, int ldr,
                       uint16_t* out, int ldo, int M, int N, void* stream);

/* LayerNorm + to_q/k/v + attention over the T = 16 frames of every spatial position for dim 320 (5 heads x 64) in one launch:
 * out[M, 320] = softmax_T(q k^T scale) v, [q | k | v] = LayerNorm(x) wqkv^T, rows ordered (clip, frame, position), M = B*16*HW,
 * HW % 8 == 0. wqkv: bf16 [>= 960][320] (to_q, to_k, to_v rows). The qkv tensor never reaches HBM; bf16 roundings as in
 * dc_layernorm -> dc_gemm_conv -> dc_temporal_attn_d64. out must not alias x.
 * replaces TemporalTransformer's norm1 -> attn1 / norm2 -> attn2 up to (not including) to_out: lvdm/modules/attention.py:242-244
 * (BasicTransformerBlock._forward) with CrossAttention.forward :101-125, at the UNet's level 0 */
int dc_ln_qkv_temporal_attn320(const uint16_t* x, int ldx, const float* ln_gamma, const float* ln_beta, float ln_eps,
                               const uint16_t* wqkv, uint16_t* out, int ldo, int B, int T, int HW, float scale, void* stream);
/* The same for dim 640 (10 heads x 64: level 1): wqkv bf16 [>= 1920][640]; out[M, 640]. */
int dc_ln_qkv_temporal_attn640(const uint16_t* x, int ldx, const float* ln_gamma, const float* ln_beta, float ln_eps,
                               const uint16_t* wqkv, uint16_t* out, int ldo, int B, int T, int HW, float scale, void* stream);

/* GroupNorm (statistics from dc_groupnorm_stats, instances = clips) + SiLU + temporal convolution (3,1,1), zero padding in
 * time, (+ residual) for C = 320 or 640 input channels in one launch; rows ordered (clip, frame, position), T = 16,
 * HW % 8 == 0, N % 32 == 0. w: the temporal-conv weight as dc_gemm_conv takes it (bf16 [>= N][3 C], k = (64-channel slice,
 * tap, channel)); bias fp32 [N]. The activated copy never reaches HBM; roundings as dc_groupnorm (silu) -> dc_gemm_conv.
 * replaces TemporalConvBlock conv1..conv4 lvdm/modules/networks/openaimodel3d.py:239-279 at the UNet's levels 0 and 1 */
int dc_gn_silu_tconv3(const uint16_t* x, int ldx, int C, const float* gamma, const float* beta, const float* stats, int groups,
                      const uint16_t* w, const float* bias, const uint16_t* residual, int ldr, uint16_t* out, int ldo, int B, int T,
                      int HW, int N, void* stream);

/* ---- conditioning encoders (once per clip) ---------------------------------------------------- */

/* Multi-head attention for any (even) head width d <= 256 and Lk <= 1024, optional causal mask (key j visible to query
 * i iff j <= i): o[b, i, h*d..] = softmax_j(scale * q[b,i,h] . k[b,j,h]) v[b,j,h]. q/o rows [B*Lq, >= heads*d], k/v rows
 * [B*Lk, >= heads*d] (bf16, row strides ld*). Needs dc_attn_small_lds_bytes(Lk, d) <= 160 KiB.
 * replaces open_clip's ResidualAttentionBlock attention (nn.MultiheadAttention, 16 heads x 80 in the ViT-H/14 vision
 * tower, 16 x 64 causal in the text tower) as driven by lvdm/modules/encoders/condition.py:216-234, 364-368 */
int dc_attn_small(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* o, int ldq, int ldk, int ldv, int ldo,
                  int B, int heads, int Lq, int Lk, int d, float scale, int causal, void* stream);
int64_t dc_attn_small_lds_bytes(int Lk, int d);

/* CLIP image preprocessing: img[N][3][H][W] fp32 in [-1,1] -> out[N][3][OH][OW] fp32 = normalize((resize(img)+1)/2).
 * resize = kornia.geometry.resize(bicubic, align_corners=True, antialias): when downscaling and antialias != 0, a
 * separable Gaussian blur (sigma = max((factor-1)/2, 0.001), ks = int(max(4 sigma, 3)) made odd, reflect borders) first;
 * tmp0/tmp1: N*3*H*W floats each (only used with the blur). mean3/std3: HOST pointers to 3 floats.
 * replaces FrozenOpenCLIPImageEmbedderV2.preprocess lvdm/modules/encoders/condition.py:322-330 */
int dc_clip_preprocess(const float* img, float* tmp0, float* tmp1, float* out, int N, int C, int H, int W, int OH, int OW,
                       int antialias, const float* mean3, const float* std3, void* stream);

/* Non-overlapping p x p patches of img[N][C][H][W] fp32 -> bf16 rows [N*(H/p)*(W/p)][kpad], column c*p*p + py*p + px
 * (the ViT patch embedding conv1 as a plain GEMM; zero columns up to kpad, kpad % 8 == 0).
 * replaces model.visual.conv1 lvdm/modules/encoders/condition.py:349-351 */
int dc_patchify(const float* img, uint16_t* rows, int N, int C, int H, int W, int p, int kpad, void* stream);

/* out[b*L + i][:] = table[tokens[b][i]][:] + pos[i][:] (bf16 rows of width D; token ids clamped to the vocabulary).
 * replaces token_embedding + positional_embedding lvdm/modules/encoders/condition.py:216-217 */
int dc_embed_tokens(const int64_t* tokens, const uint16_t* table, const uint16_t* pos, uint16_t* out, int B, int L, int D,
                    int vocab, void* stream);

/* Decoded clips video[N][C][T][H][W] fp32 in [-1,1] -> display frames out[T][H][N*W][C] uint8: clamp, (v+1)/2, *255,
 * truncation; the N clips of a batch side by side (torchvision make_grid(nrow=N, padding=0)).
 * replaces scripts/evaluation/inference.py:127-137 (save_results) / :151-160 (save_results_seperate, N = 1),
 * utils/save_video.py:35-42 */
int dc_frames_to_u8(const float* video, uint8_t* out, int N, int C, int T, int H, int W, void* stream);

/* ---- baseline JPEG (T.81 SOF0, 8-bit, YCbCr 4:2:0, Annex K Huffman tables, restart intervals) for Motion-JPEG output ----
 * Together the three entries stand where the reference hands its uint8 frames to a video encoder
 * (torchvision.io.write_video: utils/save_video.py:27-43, scripts/evaluation/inference.py:115-162); the host adds the JFIF
 * headers and the AVI container (dynamicrafter_amd/utils/save_video.py). An MCU is 16x16 pixels and holds the blocks
 * Y00 Y01 Y10 Y11 Cb Cr; my = ceil(H/16), mx = ceil(W/16). */

/* Upper bound of one entropy-coded MCU: 6 blocks x (22 + 63 x 26) bits = 1245 bytes, every one of them a stuffed 0xFF, plus
 * the padded (and possibly stuffed) last byte of a segment. */
#define DC_JPEG_MCU_MAX_BYTES 2496

/* frames[T][H][W][3] uint8 (the layout dc_frames_to_u8 writes) -> quantised DCT coefficients coef[T][my][mx][6][64] int16 in
 * zigzag order. fp32 throughout: Y = 0.299R + 0.587G + 0.114B, Cb = -0.168735892R - 0.331264108G + 0.5B + 128,
 * Cr = 0.5R - 0.418687589G - 0.081312411B + 128, chroma = mean of its 2x2 pixels, level shift -128, orthonormal 2-D DCT-II,
 * x = F / q (true division), coef = sign(x) floor(|x| + 0.5), AC clamped to +-1023. Pixels beyond the frame replicate its
 * last row / column (any H, W >= 1). qtab[2][64] uint8 (device): luminance and chrominance tables in zigzag order, entries >= 1.
 * replaces utils/save_video.py:27-43, scripts/evaluation/inference.py:115-162 (the encoder's transform stage) */
int dc_jpeg_dct_quant(const uint8_t* frames, const uint8_t* qtab, int16_t* coef, int T, int H, int W, void* stream);

/* coef[T][my][mx][6][64] -> one Huffman-coded byte string per restart segment of `ri` MCUs (the last of a frame may be
 * shorter): scratch[n_seg][stride], seg_len[n_seg], n_seg = T * ceil(my*mx / ri), frames in order. Per segment the DC
 * prediction starts from 0, 0xFF is followed by a stuffed 0x00 and the last byte is padded with 1-bits; no markers.
 * stride >= min(ri, my*mx) * DC_JPEG_MCU_MAX_BYTES + 1, else DC_ERR_SHAPE. Coefficients outside DC -1024..1023 / AC +-1023
 * are clamped to it.
 * replaces utils/save_video.py:27-43, scripts/evaluation/inference.py:115-162 (the encoder's entropy stage) */
int dc_jpeg_entropy(const int16_t* coef, uint8_t* scratch, int32_t* seg_len, int T, int my, int mx, int ri, int64_t stride,
                    void* stream);

/* Exclusive scan of each frame's segment lengths into seg_off[n_seg] (workspace), then a gather of the segments into one
 * contiguous scan per frame, out[T][frame_stride], with RSTm (FF D0+m, m = the segment's index within its frame mod 8)
 * between the segments of a frame and none after the last; frame_len[T] = the scan's length. Bytes beyond frame_stride are
 * not written: a frame_len above frame_stride tells the caller to pack again into wider rows. T <= 65535.
 * replaces utils/save_video.py:27-43, scripts/evaluation/inference.py:115-162 (the encoder's output stage) */
int dc_jpeg_pack(const uint8_t* scratch, const int32_t* seg_len, int32_t* seg_off, uint8_t* out, int32_t* frame_len, int T,
                 int segs_per_frame, int64_t stride, int64_t frame_stride, void* stream);

/* ---- baseline JPEG decoding (T.81 SOF0, 8-bit, one interleaved scan) for Motion-JPEG input ----
 * Together the three entries stand where the reference reads a clip through decord (VideoReader.get_batch:
 * scripts/evaluation/funcs.py:154-169, and the first frame of a clip at :188-190); the host walks the AVI container and the JFIF
 * headers and cuts the scans into segments (dynamicrafter_amd/utils/load_video.py). A batch is T frames of one geometry:
 * ncomp = 1 (grey; hs = vs = 1) or 3 (YCbCr, luma sampling hs x vs = 1x1, 2x1 or 2x2, chroma 1x1). An MCU is 8 hs x 8 vs
 * pixels and holds hs vs luma blocks (row-major) followed by Cb and Cr: bpm = hs vs + 2 blocks (1 for grey);
 * my = ceil(H / (8 vs)), mx = ceil(W / (8 hs)). Tables may differ from frame to frame. */

/* Per frame one table block of DC_JPEG_FRAME_TAB_BYTES bytes: the Huffman tables DC0, DC1, AC0, AC1 (each BITS[16] then
 * HUFFVAL[256], unused tail zero; a table the frame lacks is all zero), 4 quantisation tables of 64 bytes in zigzag order,
 * 3 bytes Td | Ta << 4 (one per component), 3 bytes Tq (one per component), 2 bytes padding. */
#define DC_JPEG_FRAME_TAB_BYTES 1352

/* status word of a segment after dc_jpeg_decode_entropy: 0 = decoded, else why its lane stopped */
#define DC_JPEG_ST_CODE 1         /* the next bits start no code of the table (or a symbol baseline scans do not have) */
#define DC_JPEG_ST_RUN 2          /* a zero run passes coefficient 63 */
#define DC_JPEG_ST_CATEGORY 3     /* a DC category above 11 or an AC category above 10 */
#define DC_JPEG_ST_LEFTOVER 4     /* all MCUs decoded, a whole byte or more of the segment is left (or it holds a marker) */
#define DC_JPEG_ST_MISSING 5      /* the MCUs need more bits than the segment holds */
#define DC_JPEG_ST_DESCRIPTOR 6   /* the segment's descriptor points outside the scan buffer, the frame's MCUs or its frame */

/* Entropy decoding. scan[scan_bytes]: the entropy-coded bytes of the batch, concatenated (what lies between two segments,
 * such as an RSTn, is not read). seg[n_seg][5] int32: byte offset, byte length, first MCU, MCU count, frame index of every segment (a restart interval, or
 * the whole scan of a frame without DRI), the segments of a frame contiguous and the frames in order; frame_seg[T + 1]: the
 * first segment of every frame (frame_seg[T] = n_seg); max_segs_per_frame: the largest difference. ftab[T]: table blocks.
 * -> coef[T][my][mx][bpm][64] int16 in zigzag order (zeroed by a memset on the stream first; only non-zero values are stored)
 * and status[n_seg]. One lane decodes one segment: FF 00 -> FF, DC prediction from 0, ZRL, EOB. It reads no byte outside its
 * segment (beyond the end bits read as 1s), writes only its own MCUs, and stops with a status at the first error.
 * replaces scripts/evaluation/funcs.py:154-169, :188-190 (decord's get_batch: the entropy stage) */
int dc_jpeg_decode_entropy(const uint8_t* scan, int64_t scan_bytes, const int32_t* seg, const int32_t* frame_seg,
                           const uint8_t* ftab, int16_t* coef, int32_t* status, int n_seg, int T, int my, int mx, int ncomp, int hs,
                           int vs, int max_segs_per_frame, void* stream);

/* coef -> sample planes uint8 padded to whole MCUs, per frame Y [my 8 vs][mx 8 hs] followed (ncomp = 3) by Cb and Cr
 * [my 8][mx 8]. fp32: coefficient x table entry, separable 8x8 inverse DCT with the orthonormal matrix the encoder uses, + 128,
 * floor(v + 0.5), clamp to 0..255.
 * replaces scripts/evaluation/funcs.py:154-169, :188-190 (decord's get_batch: the transform stage) */
int dc_jpeg_decode_idct(const int16_t* coef, const uint8_t* ftab, uint8_t* planes, int T, int my, int mx, int ncomp, int hs, int vs,
                        void* stream);

/* planes -> out: uint8 [T][H][W][3] (planar = 0) or fp32 [T][3][H][W] holding the same integers (planar = 1). Chroma is
 * upsampled by the triangle filter (per doubled axis 3/4 of the nearer and 1/4 of the farther sample, edges replicate, only the
 * ceil(H / vs) x ceil(W / hs) real samples are read); R = Y + 1.402 (Cr - 128), G = Y - 0.344136286 (Cb - 128) - 0.714136286
 * (Cr - 128), B = Y + 1.772 (Cb - 128); floor(v + 0.5), clamp. Grey writes Y to all three channels.
 * replaces scripts/evaluation/funcs.py:154-169, :188-190 (decord's get_batch: the output stage) */
int dc_jpeg_decode_output(const uint8_t* planes, void* out, int T, int H, int W, int ncomp, int hs, int vs, int planar,
                          void* stream);

/* ---- animated GIF (GIF89a, one global colour table of up to 256 entries, LZW minimum code size 8) ----
 * Together the four entries stand where the reference hands its uint8 frames to a video encoder
 * (torchvision.io.write_video: utils/save_video.py:27-43, scripts/evaluation/inference.py:115-162) and where its guidance
 * pipeline saves a GIF preview through Pillow (guidance_pipeline.py:647-660: duration 125 ms, loop 0); the host builds the
 * palette from the histogram and writes the container
 * (dynamicrafter_amd/utils/save_video.py). None of them allocates or synchronises; all check their arguments before any launch.
 * A frame's raster of hw = H*W indices is cut into chunks of `chunk` pixels (the last may be shorter, chunks may cross rows):
 * chunks_per_frame = ceil(hw / chunk). Every chunk is LZW-coded from the reset state, so chunks are independent. */

#define DC_GIF_HIST_BINS 32768
/* Upper bound of one chunk's code string: every one of its n pixels emits at most one data code of at most 12 bits; a Clear
 * inside the chunk needs 3838 data codes (258..4095 assigned) in front of it, so there are at most n / 3838 of them, 12 bits each;
 * one terminator of at most 12 bits. In bytes it is rounded up to whole 32-bit words (the coder stores aligned words). */
#define DC_GIF_CLEAR_INTERVAL 3838
#define DC_GIF_CHUNK_MAX_BITS(n) (12LL * ((n) + (n) / DC_GIF_CLEAR_INTERVAL + 1))
#define DC_GIF_CHUNK_MAX_BYTES(n) ((DC_GIF_CHUNK_MAX_BITS(n) + 31) / 32 * 4)

/* frames[T][H][W][3] uint8 -> hist[32768] uint32: the number of pixels of the whole clip in each bin
 * (r>>3)<<10 | (g>>3)<<5 | (b>>3). The entry clears hist itself; integer atomics, so the result does not depend on order.
 * T*H*W < 2^32.
 * replaces guidance_pipeline.py:647-660 (the colour statistics of Pillow's quantiser) */
int dc_gif_histogram(const uint8_t* frames, uint32_t* hist, int T, int H, int W, void* stream);

/* frames[T][H][W][3] uint8 + palette[n][3] uint8 (device, 1 <= n <= 256) -> idx[T][H][W] uint8. All integer:
 *   d = floor((2 B[y&7][x&7] - 63) * dither / 128), B the 8x8 Bayer matrix with values 0..63 (B[0][0..7] = 0 32 8 40 2 34 10 42,
 *   B[1][0] = 48), dither in 0..64; c' = clamp(c + d, 0, 255) per channel; idx = the entry among the first n with the least
 *   dr^2 + dg^2 + db^2 to c', ties to the lowest index. d depends on the position only, not on the frame: a static pixel maps
 *   to the same index in every frame. Exact search, the palette in LDS.
 * replaces guidance_pipeline.py:647-660 (Pillow's RGB -> P conversion on save) */
int dc_gif_map(const uint8_t* frames, const uint8_t* palette, uint8_t* idx, int T, int H, int W, int n, int dither, void* stream);

/* idx[T][hw] -> one LZW code string per chunk, codes packed LSB first: scratch[n_chunks][stride] (bytes; the last byte of a
 * string padded with zero bits, nothing written behind it), chunk_bits[n_chunks] = its length in BITS,
 * n_chunks = T * ceil(hw / chunk), frames in order. A string starts in the reset state (width 9, next code 258) and holds the
 * chunk's data codes; after code 4095 has been assigned it holds a Clear at 12 bits and starts over; it ends with a Clear if
 * another chunk of the frame follows, with EOI if not, written at the width a decoder has after adding the entry that follows
 * the last data code. The leading Clear of a frame is not part of any string (dc_gif_pack writes it).
 * scratch 4-byte aligned (else DC_ERR_ARG); stride a multiple of 4 and >= DC_GIF_CHUNK_MAX_BYTES(min(chunk, hw)), else
 * DC_ERR_SHAPE.
 * replaces guidance_pipeline.py:647-660 (Pillow's GIF encoder: the LZW stage) */
int dc_gif_lzw(const uint8_t* idx, uint8_t* scratch, int32_t* chunk_bits, int T, int hw, int chunk, int64_t stride, void* stream);

/* Exclusive scan of each frame's chunk bit lengths behind a 9-bit leading Clear into chunk_off[n_chunks] (workspace, bit
 * offsets), then a shift-merge gather of the strings at their bit offsets, the last byte padded with zero bits, wrapped into
 * sub-blocks (a length byte, at most 255 data bytes) and closed by a 00 block: out[T][frame_stride] is what follows the LZW
 * minimum code size byte of an image; frame_len[T] = its length. Bytes beyond frame_stride are not written: a frame_len above
 * frame_stride tells the caller to pack again into wider rows. T <= 65535; chunks_per_frame * stride * 8 + 9 < 2^31.
 * replaces guidance_pipeline.py:647-660 (Pillow's GIF encoder: the output stage) */
int dc_gif_pack(const uint8_t* scratch, const int32_t* chunk_bits, int32_t* chunk_off, uint8_t* out, int32_t* frame_len, int T,
                int chunks_per_frame, int64_t stride, int64_t frame_stride, void* stream);

/* ---- PNG / APNG image data (8-bit grey, RGB or RGBA; one zlib stream per frame) ----
 * Together the three entries stand where the reference hands its uint8 frames to a video encoder
 * (torchvision.io.write_video: utils/save_video.py:27-43, scripts/evaluation/inference.py:115-162); the host adds the PNG chunk
 * framing and the chunk CRCs (dynamicrafter_amd/utils/save_video.py, deflate="hip"). None of them allocates or synchronises; all
 * check their arguments before any launch.
 * A frame's plane of N = H * (1 + W * C) scanline bytes is cut into chunks of `chunk` bytes (the last may be shorter),
 * chunks_per_frame = ceil(N / chunk). Every chunk is coded alone into a whole number of bytes: no token refers to a byte in
 * front of its chunk. Tokens: a maximal run of L equal bytes is one literal, then matches of min(rem, 258) at distance 1 while
 * rem >= 3, then the 0..2 bytes left as literals. */

#define DC_PNG_CHUNK 16384         /* the default chunk of utils/save_video.py */
#define DC_PNG_CHUNK_LIMIT 65535   /* LEN of a stored block is 16 bits */
/* Upper bound of one chunk's string: the stored form, 5 bytes of block header and the n bytes themselves; a dynamic block is
 * taken only where it is shorter. Rounded up to whole 32-bit words (whole words of a string are stored as words). */
#define DC_PNG_CHUNK_MAX_BYTES(n) (((n) + 5LL + 3) / 4 * 4)
/* Upper bound of a frame's stream: 78 01, every chunk in the stored form, Adler-32. */
#define DC_PNG_FRAME_MAX_BYTES(N, chunk) (6LL + (N) + 5LL * (((N) + (chunk) - 1LL) / (chunk)))

/* frames[T][H][W][C] uint8 (C = 1, 3, 4) -> planes[T][H][1 + W*C]: per row a filter type byte 0..4 (None, Sub, Up, Average, Paeth
 * of the PNG specification, bpp = C) and the row's residuals. Filters read the raw bytes of the row and the row above (zeros above
 * row 0 of every frame). The type with the least sum over the row of min(r, 256 - r) of its residual bytes r wins, the lowest
 * type on a tie. H * (1 + W*C) < 2^31.
 * replaces utils/save_video.py:27-43, scripts/evaluation/inference.py:115-162 (the encoder's prediction stage) */
int dc_png_filter(const uint8_t* frames, uint8_t* planes, int T, int H, int W, int C, void* stream);

/* planes[T][N] (any bytes) -> per chunk its string scratch[n_chunks][stride], its length in bytes chunk_len[n_chunks] and the
 * Adler-32 of its bytes alone chunk_adler[n_chunks] (A | B << 16), n_chunks = T * ceil(N / chunk), frames in order. A string is
 * (a) one dynamic-Huffman block with BFINAL 0 (canonical codes of at most 15 bits over the chunk's literal/length counts with
 * end-of-block counted once; one distance code of length 1, or a single zero length if the chunk has no match; code lengths sent
 * as runs with 16 / 17 / 18 under a code of at most 7 bits) followed by an empty stored block, which carries BFINAL in the
 * frame's last chunk, or (b) one stored block; (b) exactly when (a) is not shorter. Bytes behind a string's length are not
 * written. scratch 4-byte aligned (else DC_ERR_ARG); 1 <= chunk <= DC_PNG_CHUNK_LIMIT; stride a multiple of 4 and >=
 * DC_PNG_CHUNK_MAX_BYTES(min(chunk, N)), else DC_ERR_SHAPE.
 * replaces utils/save_video.py:27-43, scripts/evaluation/inference.py:115-162 (the encoder's entropy stage) */
int dc_png_deflate(const uint8_t* planes, uint8_t* scratch, int32_t* chunk_len, uint32_t* chunk_adler, int T, int N, int chunk,
                   int64_t stride, void* stream);

/* Exclusive scan of each frame's chunk lengths behind the two bytes 78 01 into chunk_off[n_chunks] (workspace), a byte copy of
 * the strings to their offsets, the Adler-32 of the whole plane from the chunks' values (big-endian) behind them:
 * out[T][frame_stride] holds one zlib stream per frame, frame_len[T] = its length, at most DC_PNG_FRAME_MAX_BYTES(N, chunk). Every
 * byte has one writer; bytes beyond frame_stride are not written: a frame_len above frame_stride tells the caller to pack again
 * into wider rows. T <= 65535; 6 + ceil(N / chunk) * stride < 2^31.
 * replaces utils/save_video.py:27-43, scripts/evaluation/inference.py:115-162 (the encoder's output stage) */
int dc_png_pack(const uint8_t* scratch, const int32_t* chunk_len, const uint32_t* chunk_adler, int32_t* chunk_off, uint8_t* out,
                int32_t* frame_len, int T, int N, int chunk, int64_t stride, int64_t frame_stride, void* stream);

/* ---- image -> conditioning clip: Pillow's antialiased bilinear resize, centre crop / zero padding, ToTensor, Normalize ----
 * Together the two entries stand where the reference's loader runs torchvision's Resize(min(video_size)) ->
 * CenterCrop(video_size) -> ToTensor -> Normalize(0.5, 0.5) on a PIL image and repeats the result over the frames
 * (scripts/evaluation/inference.py:71-76, 95-108). Resize on a PIL image is Image.resize(BILINEAR): per axis
 *   out[xx] = clamp(((1 << 21) + sum_{i < n[xx]} in[xmin[xx] + i] * k[xx][i]) >> 22, 0, 255)      (int32, per channel)
 * horizontal pass first, uint8 between the passes, a pass left out when its axis keeps its size.
 * TABLES: k int32 [out][ksize], xmin int32 [out], n int32 [out] are device memory built on the host in float64 with Pillow's
 * operation order (dynamicrafter_amd/ops.py resize_coeffs). They are TRUSTED: the entries cannot read them without a
 * synchronisation, so it is the ops.py wrapper that guarantees xmin + n <= in and n <= ksize for every output, and that the
 * rows of an intermediate cover every window of the vertical pass. (A window that breaks this is cut to the operand inside the
 * kernel: wrong pixels, no read outside it.)
 * Neither entry allocates or synchronises; both check their arguments before any launch. */

/* Horizontal pass of src uint8 [H][W][3] into the intermediate dst uint8 [rows][cols][3]: source rows y0 .. y0 + rows - 1
 * (the ones the vertical pass reads), resized columns x0 .. x0 + cols - 1 of out_w (the ones the crop keeps).
 * replaces scripts/evaluation/inference.py:73 (transforms.Resize, horizontal pass), applied at :97, :99, :106 */
int dc_prep_resize_h(const uint8_t* src, uint8_t* dst, const int32_t* k, const int32_t* xmin, const int32_t* n, int ksize, int H,
                     int W, int out_w, int y0, int rows, int x0, int cols, void* stream);

/* The last pass, fused with crop, padding, normalisation and the repetition over frames. src uint8 [sh][sw][3] is a part of an
 * image whose pixel (sy0, sx0) is src's (0, 0); the resized image is rh x rw; crop pixel (oy, ox) of ch x cw is the resized
 * pixel (oy + yoff, ox + xoff), or padding (uint8 0) where that lies outside the resized image.
 *   axis 0: no pass (src is the resized image);  k, kmin, kn may be NULL
 *   axis 1: horizontal pass (src has the resized height; tables per resized column)
 *   axis 2: vertical pass (src has the resized width: the source, or dc_prep_resize_h's intermediate; tables per resized row)
 * Then v = u8 / 255, (v - 0.5) / 0.5 in fp32, stored into frames t0 .. t0 + nt - 1 of clip fp32 [3][T][ch][cw]; other frames
 * are not touched (the reference's interp mode: the first image into frames 0 .. T/2 - 1, the second into the rest).
 * DC_ERR_SHAPE unless src holds, along the axis it is addressed directly, every resized pixel the crop keeps.
 * replaces scripts/evaluation/inference.py:73-76 (Resize's last pass, CenterCrop, ToTensor, Normalize) and :95-108
 * (unsqueeze / repeat over video_frames / cat of the two halves) */
int dc_prep_finish(const uint8_t* src, float* clip, const int32_t* k, const int32_t* kmin, const int32_t* kn, int ksize, int axis,
                   int sh, int sw, int sy0, int sx0, int rh, int rw, int yoff, int xoff, int ch, int cw, int T, int t0, int nt,
                   void* stream);

/* ---- float image -> conditioning frame: bilinear resize of fp32 planes with optional antialias, crop / 0.0f padding ----
 * The reference's programmatic entry points resize a float tensor already normalised to [-1, 1]: torchvision's Resize /
 * CenterCrop on a tensor = torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=True) and a crop
 * that pads with 0.0; cv2.resize(INTER_LINEAR) on float32 = the same with antialias=False. Per axis
 *   out[xx] = sum_{i < n[xx]} in[xmin[xx] + i] * k[xx][i]                  (fp32, fma in tap order, per plane)
 * horizontal pass first, an fp32 intermediate between the passes, a pass left out when its axis keeps its size.
 * TABLES: k fp32 [out][ksize], xmin int32 [out], n int32 [out] are device memory built on the host
 * (dynamicrafter_amd/ops.py resize_coeffs_f32, ATen's antialias window rule) and TRUSTED exactly as the uint8 tables above: the
 * ops.py wrapper guarantees xmin + n <= in and n <= ksize, and a window that breaks this is cut to the operand inside the kernel.
 * Images are planar fp32 [C][H][W], any C >= 1. Neither entry allocates or synchronises; both check their arguments before any
 * launch. Not bit-compatible with the uint8 path (Pillow's fixed point) nor bit-for-bit with ATen (summation order): see
 * DESIGN 4.8. */

/* Horizontal pass of src fp32 [C][H][W] into the intermediate dst fp32 [C][rows][cols]: source rows y0 .. y0 + rows - 1 (the
 * ones the vertical pass reads), resized columns x0 .. x0 + cols - 1 of out_w (the ones the crop keeps).
 * seg = 0: every lane reads its window from global memory. seg > 0: a workgroup stages the source segment and the weights of
 * DC_RESIZE_F32_TILE consecutive outputs (tiles count from x0) in the LDS; seg = the most source columns such a tile spans,
 * max over tiles of xmin[last] + n[last] - xmin[first] (the caller knows the tables; xmin and xmin + n must not decrease; a
 * window outside the staged segment is cut to it). DC_ERR_SHAPE if DC_RESIZE_F32_LDS_BYTES(seg, ksize) exceeds
 * DC_RESIZE_F32_LDS_MAX: use seg = 0 then. Both forms sum in tap order and give the same bits.
 * replaces scripts/gradio/i2v_test.py:39-42, 65; scripts/gradio/i2v_test_application.py:39-42, 65, 75;
 * scripts/gradio/dynamicrafter_pipeline.py:281-288 (transforms.Resize on a tensor, horizontal pass) and
 * scripts/evaluation/funcs.py:196 (cv2.resize INTER_LINEAR, horizontal pass) */
#define DC_RESIZE_F32_TILE 256
#define DC_RESIZE_F32_LDS_BYTES(seg, ksize) (4LL * ((long long)(seg) + (long long)DC_RESIZE_F32_TILE * (ksize)))
#define DC_RESIZE_F32_LDS_MAX 65536
int dc_resize_f32_h(const float* src, float* dst, const float* k, const int32_t* xmin, const int32_t* n, int ksize, int C, int H,
                    int W, int out_w, int y0, int rows, int x0, int cols, int seg, void* stream);

/* The last pass fused with crop and padding. src fp32 [C][sh][sw] is a part of an image whose pixel (sy0, sx0) is src's (0, 0)
 * in every plane; the resized image is rh x rw; pixel (oy, ox) of out fp32 [C][ch][cw] is the resized pixel
 * (oy + yoff, ox + xoff), or 0.0f where that lies outside the resized image.
 *   axis 0: no pass (src is the resized image: a crop / pad copy);  k, kmin, kn may be NULL
 *   axis 1: horizontal pass (src has the resized height; tables per resized column)
 *   axis 2: vertical pass (src has the resized width: the source, or dc_resize_f32_h's intermediate; tables per resized row)
 * DC_ERR_SHAPE unless src holds, along the axis it is addressed directly, every resized pixel the crop keeps.
 * replaces scripts/gradio/i2v_test.py:39-42, 65; scripts/gradio/i2v_test_application.py:39-42, 65, 75;
 * scripts/gradio/dynamicrafter_pipeline.py:281-288 (Resize's last pass and CenterCrop with its zero padding) and
 * scripts/evaluation/funcs.py:196 (cv2.resize's last pass) */
int dc_resize_f32_finish(const float* src, float* out, const float* k, const int32_t* kmin, const int32_t* kn, int ksize, int axis,
                         int C, int sh, int sw, int sy0, int sx0, int rh, int rw, int yoff, int xoff, int ch, int cw,
                         void* stream);

/* Mask / x0 blend ahead of a DDIM step, in place on img [n] fp32: img = orig*mask + (1-mask)*img with
 * orig = x0 (clean != 0) or sqrt_acp_t[i]*x0 + sqrt_1macp_t[i]*qnoise (q_sample of x0 at the step's timestep);
 * i = step_index[0] (device counter; qnoise then starts at qnoise + i*noise_step_stride) or `index`.
 * replaces lvdm/models/samplers/ddim.py:174-180 + DDPM.q_sample lvdm/models/ddpm3d.py:305-308 */
int dc_mask_blend(float* img, const float* x0, const float* mask, const float* qnoise, const float* sqrt_acp_t,
                  const float* sqrt_1macp_t, const int32_t* step_index, int index, int64_t n,
                  int64_t noise_step_stride, int clean, void* stream);

/* ---- FreeU (Si et al., CVPR 2024; diffusers enable_freeu) in place on the [h | skip] buffer of an up block ----
 * cat: bf16 rows [F*H*W][ld], 16-byte aligned, ld % 8 == 0, ld >= ch + cs; columns 0..ch-1 are h, ch..ch+cs-1 the skip;
 * ch % 128 == 0, cs % 64 == 0, H + W <= 1024, F <= 65535, F*H*W*ld < 2^31 (else DC_ERR_SHAPE). Rows are (frame, y, x).
 * No atomics and no scratch that needs clearing: every call is capturable and two runs on the same input give the same bits.
 * replaces diffusers' apply_freeu + fourier_filter (utils/torch_utils.py), which the reference UNet would call ahead of
 * torch.cat([h, hs.pop()]) (openaimodel3d.py:596).
 *
 * dc_freeu_scratch_floats: the fp32 elements of the scratch the three entries share for one buffer: `stats`, then (version 2)
 * `hmean` [F*H*W] and `mm` [F][2], in this order (DC_ERR_ARG for a bad argument). No initialisation needed.
 *
 * dc_freeu_skip_stats: per (frame f, skip channel c) the seven fp32 sums over the plane x[y][x'] with ty = 2 pi y / H,
 * tx = 2 pi x' / W: sum x * (1, cos ty, sin ty, cos tx, sin tx, cos(ty+tx), sin(ty+tx)) -> stats[z][f][c][0..6]. A plane of
 * 512 pixels or more is summed in nz = min(8, H*W / 256) slices z by as many workgroups, whose partial sums dc_freeu_apply
 * adds in the order of z; smaller planes have nz = 1 and stats is [F][cs][7]. With hmean / mm (both or neither; FreeU
 * version 2) it also writes mm[f][0..1] = min / max of hmean[f*H*W ..] over the frame. */
int64_t dc_freeu_scratch_floats(int cs, int F, int H, int W, int version);
int dc_freeu_skip_stats(const uint16_t* cat, int ld, int ch, int cs, int F, int H, int W, float* stats, const float* hmean,
                        float* mm, void* stream);

/* hmean[row] = mean over the ch columns of h, fp32 [F*H*W] (FreeU version 2: hidden_states.mean(1)). */
int dc_freeu_hmean(const uint16_t* cat, int ld, int ch, int cs, int F, int H, int W, float* hmean, void* stream);

/* One in-place pass. Skip columns: x + (s-1)/(H*W) * (S0 + Cy cos ty + Sy sin ty + Cx cos tx + Sx sin tx + Cxy cos(ty+tx)
 * + Sxy sin(ty+tx)) with the sums of dc_freeu_skip_stats: fourier_filter(x, threshold=1, scale=s). Columns 0..ch/2-1:
 * x * b (hmean == mm == NULL, version 1) or x * ((b-1) * mhat + 1), mhat = (hmean - min_f) / (max_f - min_f) and 0 where
 * max_f == min_f (version 2). fp32 arithmetic, one rounding to bf16. Columns ch/2..ch-1 are neither read nor written. */
int dc_freeu_apply(uint16_t* cat, int ld, int ch, int cs, int F, int H, int W, const float* stats, float b, float s,
                   const float* hmean, const float* mm, void* stream);

/* ---- Adaptive projected guidance (APG: Sadat, Hilliges, Weber, ICLR 2025, Algorithm 1) ahead of a step's update kernel ---- */
typedef struct DcApgParams {
    /* per-step fp32 tables in execution order (DcDdimParams'), read only with x0_space and indexed by step_index[0] (device)
     * when step_index != NULL, else by `index` */
    const float* a_t;                /* eps models: x0 = (x - sqrt_one_minus_at eps) / sqrt(a_t); a_t > 0 is the caller's duty */
    const float* sqrt_one_minus_at;
    const float* sqrt_acp_t;         /* v models: x0 = sqrt_acp_t x - sqrt_1macp_t v (ddpm3d.py:239-245) */
    const float* sqrt_1macp_t;
    const int32_t* step_index;       /* device counter or NULL */
    int index;
    int v_param;                     /* parameterization == "v" */
    int x0_space;                    /* 1: p_c, p_u are the denoised predictions (the paper); 0: the raw outputs (diffusers) */
    int e_nchw;                      /* as DcDdimParams; `out` has the layout of e_cond */
    float cfg_scale;                 /* w = unconditional_guidance_scale */
    float eta;                       /* weight of the component of the update parallel to p_c; 1 keeps plain CFG's */
    float norm_threshold;            /* <= 0: the norm of the update is not clipped */
    float momentum;                  /* 0: no running average (momentum_buf is then written, not read) */
} DcApgParams;

/* Per clip b, over all C*THW elements, with p_c / p_u the predictions from e_cond / e_uncond in the chosen space:
 *   d = p_c - p_u,  m = d + momentum m_prev,  s = min(1, norm_threshold / ||m||) (1 without threshold or for m = 0),  D = s m,
 *   par = (D . p_c / ||p_c||^2) p_c (0 for p_c = 0),  guided = p_c + (cfg_scale - 1) ((D - par) + eta par)
 * and `out` = guided, mapped back to the model's output space when x0_space. The update kernels then take `out` as e_cond with
 * e_uncond = NULL and cfg_scale = 1. e_cond, e_uncond: fp32 rows [B*THW, ld_e] (first C valid) or [B, C, THW] under e_nchw;
 * out: the same layout with row stride ld_out; x, momentum_buf: fp32 [B, C, THW]; x may be NULL without x0_space.
 * B <= 65535, ld_e >= C and ld_out >= C for rows (else DC_ERR_SHAPE); non-finite cfg_scale / eta / momentum, NaN threshold or
 * a missing operand or table: DC_ERR_ARG. No atomics, nothing to clear between calls, capturable, bit-reproducible.
 * replaces the plain CFG combine inside dc_ddim_step / dc_dpmpp_step (p_sample_ddim lvdm/models/samplers/ddim.py:226-245) with
 * diffusers' AdaptiveProjectedGuidance / normalized_guidance (guiders/adaptive_projected_guidance.py), which the reference
 * does not have.
 *
 * dc_apg_workspace_floats: fp32 elements of `workspace`: three partial sums per workgroup of dc_apg_reduce,
 * 3 * B * min(256, ceil(THW / 256)); no initialisation needed (DC_ERR_ARG for a bad argument).
 *
 * dc_apg_reduce: momentum_buf = m in place (the caller zeroes it ahead of a run's first step), workspace[b][g][0..2] = workgroup
 * g's sums of m*m, m*p_c, p_c*p_c. d is formed as ps (e_cond - e_uncond), ps the factor of e in p (1, -sqrt_1macp_t or
 * -sqrt_one_minus_at / sqrt(a_t)): equal outputs give d = 0 exactly. */
int64_t dc_apg_workspace_floats(int B, int C, int THW);
int dc_apg_reduce(const DcApgParams* p, const float* e_cond, const float* e_uncond, int ld_e, const float* x,
                  float* momentum_buf, int B, int C, int THW, float* workspace, void* stream);

/* dc_apg_apply: adds the partial sums of dc_apg_reduce in a fixed order in float64, forms s and g = (1 - eta) s (m . p_c) /
 * ||p_c||^2, and writes out = e_cond + (cfg_scale - 1) / ps * (s m - g p_c): one fused multiply-add on e_cond, so eta = 1
 * without threshold and momentum is plain CFG. Same p, e_cond, x and momentum_buf as the dc_apg_reduce call before it. */
int dc_apg_apply(const DcApgParams* p, const float* e_cond, int ld_e, const float* x, const float* momentum_buf, float* out,
                 int ld_out, int B, int C, int THW, const float* workspace, void* stream);

/* step_index[0] += 1 (device-side loop counter for the graph-captured sampler). */
int dc_advance_counter(int32_t* counter, void* stream);

/* ---- stream / hipGraph plumbing (one capture per sampler configuration; replayed once per DDIM step) ---- */
int dc_stream_create(void** stream_out);
int dc_stream_destroy(void* stream);
int dc_stream_sync(void* stream);
int dc_graph_begin_capture(void* stream);
int dc_graph_end_capture(void* stream, void** graph_exec_out);
int dc_graph_launch(void* graph_exec, void* stream);
int dc_graph_destroy(void* graph_exec);
/* HIP-event timing on an arbitrary stream (bench.py roofline leg) */
int dc_event_create(void** ev_out);
int dc_event_record(void* ev, void* stream);
int dc_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out); /* synchronises on ev_stop */
int dc_event_destroy(void* ev);

/* The library's error word. Kernels that synchronise through LDS arrival counters (the one-wave-per-SIMD GEMM / conv kernel,
 * the ping-pong GEMM, the long self-attention) bound every wait so that a bookkeeping mistake cannot hang the GPU; a wave whose
 * wait ran out ORs a bit into one device word (1: gemm_pipe320x16, 2: flash attention K/V ring, 4: gemm_pp) and its results
 * are then NOT valid. This entry synchronises the device, copies the word to *out and, if `reset`, clears it. It is the one
 * entry that synchronises and is not capturable: call it at the host's own sync points (the sampler does after a run, bench.py
 * before it prints). Returns 0 or a hipError_t / DC_ERR_ARG. */
int dc_error_word_read(int* out, int reset);

const char* dc_version(void);

#ifdef __cplusplus
}
#endif
#endif
