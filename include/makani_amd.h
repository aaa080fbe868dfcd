/*
 * makani_amd.h — C ABI of libmakani_amd.so (gfx950 / MI355X).
 *
 * The reference (NVIDIA/makani) has no FFI of its own: its hot path is Python
 * calling torch ops.  This header is therefore the boundary a
 * maintainer would bind *behind* the reference's nn.Module interface; every
 * entry point names the reference call it replaces (paths relative to
 * /root/reference).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - all pointers are DEVICE pointers (hipMalloc'ed / torch-allocated), 16-byte aligned;
 *  - `stream` is a hipStream_t passed as void* (0 = default stream); every call
 *    only enqueues work, nothing synchronises;
 *  - return value: 0 on success, negative MK_E* code on invalid arguments,
 *    positive hipError_t if the launch failed. mk_last_error() gives a message;
 *  - dtype codes: MK_F32 = 0, MK_BF16 = 1.
 *
 * Internal spectral layouts (all fp32, planar re/im, padded to multiples of 4):
 *  F-layout  F[m][k][ri][row]   m < M, k < nlat, ri in {re,im}, row < R (R = B*Cp)  (k-major: rows contiguous)
 *  S-layout  S[l][m][ri][row]   l < L, m < M, row < R                                (coefficients)
 *  W-layout  W[l][ri][i][o]     dhconv weights, i < Cip, o < Cop (zero padded)
 */
#ifndef MAKANI_AMD_H
#define MAKANI_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define MK_F32 0
#define MK_BF16 1

#define MK_EINVAL -1   /* bad argument (shape / alignment / dtype)            */
#define MK_EUNSUP -2   /* unsupported size (e.g. odd nlon, prime factor > 31)  */

/* triangular structure of the spherical-harmonic index space (P_l^m = 0 for l < m) */
#define MK_TRI_NONE 0
#define MK_TRI_ROW_GE 1 /* only output rows i >= t are computed                (Legendre analysis, t = m)   */
#define MK_TRI_K_GE 2   /* contraction runs over k >= t only                   (Legendre synthesis, t = m)  */
#define MK_TRI_ROW_LE 3 /* only output rows i <= t are computed                (dhconv fwd/dgrad, t = l)    */
#define MK_TRI_K_LE 4   /* contraction runs over k <= t only                   (dhconv wgrad, t = l)        */
/* with t = batch_index / inner + tri_off  (the OUTER batch index, shifted by the shard offset when the
 * triangular index space is sharded across ranks; t may be negative or exceed the extent) */

/* Strided batched GEMM descriptor:  C[b][i][j] (+)= sum_k A[b][i][k] * B[b][j][k]
 * Element strides.  One of {a_row, a_k} must be 1 (same for B); c_col must be 1.
 * Two-level batch: b = outer * inner + in;  offset = outer * x_batch + in * x_inner.
 * Complex variant: *_im = element offset from the real plane to the imaginary plane. */
typedef struct MkGemm {
    const float* A;
    const float* B;
    float* C;
    long long a_batch, a_row, a_k;
    long long b_batch, b_col, b_k;
    long long c_batch, c_row, c_col;
    long long a_inner, b_inner, c_inner;
    long long a_im, b_im, c_im;
    int M, N, K, batch; /* batch = outer count * inner */
    int inner;          /* >= 1 */
    int tri_mode;
    int tri_off;
    int conj_a, conj_b;
    int beta; /* 0: C = A*B^T ; 1: C += A*B^T */
} MkGemm;

const char* mk_last_error(void);
int mk_version(void);

/* ---- fp32 MFMA batched GEMMs ------------------------------------------------
 * mk_sgemm_batched : real.  Replaces the two einsums of th.RealSHT.forward /
 *   th.InverseRealSHT.forward [torch-harmonics, un-vendored; call sites
 *   makani/models/common/spectral_convolution.py:239,241,253] and their autograd.
 * mk_cgemm_batched : complex (planar).  Replaces _contract_lwise
 *   (makani/models/common/contractions.py:23-24) and its autograd. */
int mk_sgemm_batched(const MkGemm* g, void* stream);
int mk_cgemm_batched(const MkGemm* g, void* stream);
/* Same contracts on the bf16 matrix cores: every fp32 operand is split on the fly into `limbs` bf16 limbs
 * (3: x = hi+mid+lo, 6 MFMAs per product, fp32 round-off class, measured rel-L2 1.8e-7 vs fp64;
 *  2: x = hi+mid, 3 MFMAs, ~4e-6), fp32 accumulation.  6/16 resp. 3/16 of the exact-fp32 MFMA time. */
int mk_sgemm_split_batched(const MkGemm* g, int limbs, void* stream);
int mk_cgemm_split_batched(const MkGemm* g, int limbs, void* stream);
/* Second-generation kernels of the same arithmetic for the hot shapes (csrc/xgemm2.hip: 512-thread workgroups whose two
 * wave groups alternate between the matrix pipe and the limb split, double-buffered LDS images).
 * mk_cgemm_split2_batched: the complex split engine (mk_cgemm_split_batched is an alias of it since round 5, when the
 *   first-generation complex kernel was retired): any complex descriptor (the dhconv forward / data-gradient /
 *   weight-gradient GEMMs of _contract_lwise, makani/models/common/contractions.py:23-24).
 * mk_sgemm_presplit_batched: real GEMM whose A operand is a CONSTANT matrix handed over already split into `limbs`
 *   bf16 limb planes — the Legendre matrices of th.RealSHT / th.InverseRealSHT [un-vendored; precomputed in
 *   makani_amd/legendre.py].  g->A is ignored; plane q of batch b holds A[b][k][row] at
 *   a_planes + q*pl_stride + b*pl_batch + k*pl_k + row (bf16 elements; row contiguous, pl_k % 8 == 0, rows beyond M
 *   inside pl_k are zero).  B must be [k][col] with the column index contiguous (b_col == 1).  With inner > 1 the constant
 *   matrix, its band and the triangle belong to the OUTER index bo = b / inner (planes at + bo*pl_batch, band_lo[bo]); the
 *   inner index only moves B and C (b_inner / c_inner): several column blocks that live in separate buffers (the plane blocks
 *   of the h x w distributed transform, makani_amd/dist_pipeline.py) then share ONE launch and one pass over the matrix.
 *   band_lo / band_hi (device int[batch / inner], optional): outside [lo[b], hi[b]) every entry of A[b] is numerically zero by the
 *   caller's threshold (the Legendre functions of order m vanish towards the poles like sin^m theta).  band_mode 1: a range
 *   of k (analysis: the latitude sum is clipped); 2: a range of rows (synthesis: output latitudes outside the band are
 *   written as exact zeros); 0: no band.  Neither A nor B is read outside the band. */
int mk_cgemm_split2_batched(const MkGemm* g, int limbs, void* stream);
/* mk_cgemm_split2_batched that also hands back the sum of re^2 + im^2 over everything it writes, as one fp32 partial per workgroup
 * (ssq_part[0 .. mk_cgemm_split2_ssq_count(g)), fixed summation order; workgroups without work write 0): the weight gradient of
 * _contract_lwise (makani/models/common/contractions.py:23-24) is 283 MB per layer, and the global-norm clipping of
 * makani/utils/training/training_helpers.py:123-165 would otherwise read it once more just to square it (mk_grad_clip_coef_pre
 * takes the partials instead).  With beta = 1 the sums are those of the accumulated values. */
long long mk_cgemm_split2_ssq_count(const MkGemm* g);
int mk_cgemm_split2_batched_ssq(const MkGemm* g, int limbs, float* ssq_part, void* stream);
int mk_sgemm_presplit_batched(const MkGemm* g, const void* a_planes, long long pl_stride, long long pl_batch,
                              long long pl_k, int limbs, const int* band_lo, const int* band_hi, int band_mode,
                              void* stream);

/* ---- vector Legendre stage (csrc/vlegendre.hip) --------------------------------
 * mk_vlegendre: the Legendre stage of th.RealVectorSHT / th.InverseRealVectorSHT [torch-harmonics, un-vendored; call sites
 *   makani/utils/losses/base_loss.py:461-469,547-554] and its autograd, one launch per direction.
 *   A vector field of P pairs is a scalar F / S tensor whose rows are (component, pair), Rp = P rounded up to 32 rows per
 *   component: F (orders, nlat, 2, 2 Rp), S (L, orders, 2, 2 Rp).  planes0 / planes1: limb planes (as for
 *   mk_sgemm_presplit_batched: [plane][order][k][row], row contiguous) of dP/dtheta and m P/sin(theta), both over
 *   sqrt(l (l + 1)).  mode 0 analysis (rows = L, K = nlat; planes = weighted matrices, [lat][l]):
 *       s = A0 U - i A1 V,  t = i A1 U + A0 V;
 *   mode 1 synthesis (rows = nlat, K = L; planes [l][lat]):  U = A0 s - i A1 t,  V = i A1 s + A0 t;
 *   mode 2 analysis that forms s only: out is S (L, orders, 2, Rp);
 *   mode 3 synthesis with t = 0: in is S (L, orders, 2, Rp) (the gradient of a scalar field).
 *   Modes 1 / 0 with the transposed matrices are the transposed maps of modes 0 / 1, modes 3 / 2 those of 2 / 3.
 *   band_lo / band_hi (device int[orders], optional): the latitude band outside of which BOTH matrices vanish; analysis
 *   clips the latitude sum, synthesis writes exact zeros outside.  Rows l < m + tri_off are skipped in 32-row steps.
 *   The m-shard form (an azimuth rank of the h x w distributed pair): `orders` consecutive orders starting at tri_off, i.e.
 *   batch b is the GLOBAL order b + tri_off; planes, in / out and the band arrays are indexed by the LOCAL order b (the
 *   caller hands over the slices [tri_off, tri_off + orders) of all of them).  Orders are independent batches, so the shard
 *   launch writes the same bits, and leaves the same rows l < m unwritten, as the same orders of the full launch. */
int mk_vlegendre(const void* planes0, const void* planes1, long long pl_stride, long long pl_batch, long long pl_k,
                 int limbs, const float* in, float* out, int mode, int rows, int K, int orders, int Rp, int tri_off,
                 const int* band_lo, const int* band_hi, void* stream);
/* mk_vcols_repack (csrc/vcols.hip): pack / unpack side of the exchanges that split or join the PAIRS of a vector F / S tensor,
 *   whose last axis is `blocks` (4, or 2 for the s-only / t = 0 forms) column blocks of rp columns.  For outer x inner rows:
 *       dst[o][i][blk][dst_c0 + c] = src[o][i][blk][src_c0 + c],  c in [0, ncols);
 *   a row is blocks * src_rp (blocks * dst_rp) floats, inner rows are adjacent, src_outer / dst_outer are the strides (in
 *   floats) of the outer index.  zero_tail != 0: columns [dst_c0 + ncols, dst_rp) of every block are written as zeros.
 *   Any extents and offsets (16-byte accesses when all are multiples of 4 and the bases aligned); ncols == 0 or no rows: no
 *   launch.  One pass, no host reads, no allocation. */
int mk_vcols_repack(const float* src, float* dst, long long outer, long long inner, int blocks, int ncols,
                    long long src_outer, int src_rp, int src_c0, long long dst_outer, int dst_rp, int dst_c0,
                    int zero_tail, void* stream);

/* ---- longitude FFTs ----------------------------------------------------------
 * mk_rfft_rows: x[row][lat][lon] (f32|bf16)  ->  F-layout, modes m < mmax:
 *     X_m = w_m * sum_n x_n exp(-2 pi i m n / nlon),  w = (w_dc, w_pos, w_nyq)
 *   Replaces `2*pi*torch.fft.rfft(x, norm="forward")[..., :mmax]` (th.RealSHT.forward;
 *   in-tree twin makani/mpu/fft.py:157-160) and, with other weights, the adjoint of irfft.
 * mk_irfft_rows: F-layout -> x[row][lat][lon] (f32|bf16):
 *     x_n = sum_m w_m * ( Re X_m cos(2 pi m n/nlon) - Im X_m sin(2 pi m n/nlon) )
 *   Replaces `torch.fft.irfft(X, n=nlon, norm="forward")` incl. the Im(m=0)/Im(Nyquist)
 *   drop (th.InverseRealSHT.forward; twin makani/mpu/fft.py:242) and the adjoint of rfft.
 * x holds B*C planes; plane (b, c) maps to F row b*Cp + c (R = B*Cp rows, pad rows untouched).
 * A workgroup transforms one latitude of 8-16 consecutive planes, so the F side is touched in runs of
 * 8-16 consecutive rows and the Legendre GEMMs see both operands row-contiguous.
 * `twiddle` = device table of nlon float2: exp(-2 pi i q / nlon) (host fp64 -> fp32).
 * `radix`   = host array of `nradix` radices whose product is nlon/2.               */
int mk_rfft_rows(const void* x, int x_dtype, float* F, const float* twiddle, const int* radix, int nradix,
                 int B, int C, int Cp, int nlat, int nlon, int mmax, float w_dc, float w_pos, float w_nyq,
                 void* stream);
int mk_irfft_rows(const float* F, void* x, int x_dtype, const float* twiddle, const int* radix, int nradix,
                  int B, int C, int Cp, int nlat, int nlon, int mmax, float w_dc, float w_pos, float w_nyq,
                  void* stream);

/* Segmented addressing for the distributed transforms (makani_amd/distributed.py; the reference schedule: torch-harmonics'
 * DistributedRealSHT / DistributedInverseRealSHT [un-vendored], in-tree twin makani/mpu/fft.py:148-182,214-249 with the
 * split / all_to_all / cat of makani/mpu/mappings.py:38-67).  Instead of packing send chunks and concatenating received ones
 * in separate passes, the FFT kernels address both of their sides through this descriptor:
 *   F side = per-peer slabs: slab (jw, ih) = orders m in [m_off[jw], m_off[jw+1]) x rows in [r_off[ih], r_off[ih+1]) of every
 *     latitude of the call, latitude outermost: [lat][m][re/im][row] at F + base[jw][ih] (floats).  nw / nh = number of
 *     m ranges / row ranges (<= MK_FFT_SEG_MAX); r_off and base entries are multiples of 4.
 *   x side = every row (plane, latitude) of nlon points cut into `xseg` equal pieces; piece j of all rows at
 *     x + j * x_stride elements, rows of a piece [plane][x_nlat][nlon / xseg] (xseg <= 1: whole rows, as mk_rfft_rows).
 *   A call may transform a latitude sub-range (chunked overlap of transform and exchange): nlat = its length, x and the slab
 *   offsets point at its first latitude, x_nlat = latitudes per plane of the x buffers.
 * One batch entry; C planes; implemented by the specialised row lengths only (mk_fft_seg_supported). */
#define MK_FFT_SEG_MAX 8
typedef struct MkFftSeg {
    int nw, nh;
    int m_off[MK_FFT_SEG_MAX + 1];
    int r_off[MK_FFT_SEG_MAX + 1];
    long long base[MK_FFT_SEG_MAX][MK_FFT_SEG_MAX];
    int xseg;
    long long x_stride;
    int x_nlat; /* latitudes per plane in the x buffers (the call may cover a sub-range: x then points at its first latitude);
                   0 = nlat of the call */
} MkFftSeg;
int mk_fft_seg_supported(int nlon);
int mk_rfft_rows_seg(const void* x, int x_dtype, float* F, const float* twiddle, int C, int nlat, int nlon, int mmax,
                     float w_dc, float w_pos, float w_nyq, const MkFftSeg* seg, void* stream);
int mk_irfft_rows_seg(const float* F, void* x, int x_dtype, const float* twiddle, int C, int nlat, int nlon, int mmax,
                      float w_dc, float w_pos, float w_nyq, const MkFftSeg* seg, void* stream);

/* ---- layout changes ------------------------------------------------------------
 * complex64 dhconv parameter (Cin, Cout, L) [makani/models/common/spectral_convolution.py:164-193]
 * <-> W-layout, and S-layout <-> complex64 (rows, L, M) tensors at the RealSHT API boundary. */
int mk_weight_to_wlayout(const float* w_c64, float* W, int cin, int cout, int cip, int cop, int L, void* stream);
int mk_wlayout_to_weight_grad(const float* gW, float* gw_c64, int cin, int cout, int cip, int cop, int L, void* stream);
int mk_slayout_to_complex(const float* S, float* out_c64, int B, int C, int Cp, int L, int M, int l_off, int m_off,
                          void* stream);
int mk_complex_to_slayout(const float* in_c64, float* S, int B, int C, int Cp, int L, int M, void* stream);

/* ---- pointwise blocks -----------------------------------------------------------
 * All operate on NCHW planes: x[(b*channels + c)][hw], dtype f32 | bf16, fp32 arithmetic.
 * `ws` is a caller-provided scratch of >= planes * mk_pointwise_chunks(hw, dtype, planes) * 2 floats (a plane is cut
 * into as many chunks as keep every workgroup of the launch resident at once).
 *
 * Instance norm = nn.InstanceNorm2d(C, eps, affine=True) at makani/models/networks/sfnonet.py:618-620
 * (statistics in fp32 as in makani/mpu/layer_norm.py:147-168); optional fused GELU
 * (nn.GELU, sfnonet.py:392-393; exact erff on fp32 tensors, the A&S 7.1.26 erf — |err| < 1.5e-7 — on bf16 tensors).  stats: (planes, 2) f32 = {mean, rstd}.
 * Backward: sums (2, planes) f32, planar: row 0 = sum ga (dbeta per plane), row 1 = sum ga * xhat (dgamma per plane),
 * gx = rstd*gamma*(ga - mean(ga) - xhat*mean(ga*xhat)), ga = gy * (gelu'(a) if fused).
 * phase 0 = reduce + apply (serial); 1 = reduce only (writes the local `sums`); 2 = apply only with the
 * caller-provided (all-reduced) `sums` and `hw_total` = pixels of the whole plane over all spatial ranks —
 * the split DistributedInstanceNorm2d (makani/mpu/layer_norm.py:108-170) needs.                      */
int mk_pointwise_chunks(long long hw, int dtype, long long planes);
/* sums[p] = sum of plane p (fp32; `sums` holds 2 * planes floats, the second row is zero): the bias gradient of a 1x1
 * convolution, `grad_output.sum((0, 2, 3))` in the autograd of nn.Conv2d (makani/models/common/layers.py:603-643). */
int mk_plane_sums(const void* x, int dtype, float* sums, float* ws, long long planes, long long hw, void* stream);
/* `quad` (hw fp32 weights of this shard, may be NULL) with `quad_sum` = their sum: quadrature-weighted local moments
 * with count = quad_sum — what DistributedGeometricInstanceNormS2 merges (makani/mpu/layer_norm.py:207-222). */
int mk_instnorm_stats(const void* x, int dtype, float* stats, float* ws, long long planes, long long hw, float eps,
                      const float* quad, float quad_sum, void* stream);
/* merged statistics of planes sharded over `nranks` ranks: all_stats (nranks, planes, 2) = every rank's local {mean, rstd}
 * (the all-gathered outputs of mk_instnorm_stats), counts (nranks) = every rank's pixel count (or sum of quadrature weights);
 * stats (planes, 2) = {mean, rstd} of the whole plane — the pairwise moment merge of DistributedInstanceNorm2d
 * (makani/mpu/layer_norm.py:31-81,140-152), fp64 inside, no host round trip. */
int mk_instnorm_merge(const float* all_stats, const float* counts, float* stats, long long planes, int nranks, float eps,
                      void* stream);
int mk_instnorm_apply(const void* x, void* y, int dtype, const float* stats, const float* gamma, const float* beta,
                      long long planes, int channels, long long hw, int fuse_gelu, void* stream);
/* stats + apply in two launches (the apply kernel finishes the statistics reduction itself and writes `stats` for the
 * backward): what the serial InstanceNorm2d forward uses.  `pre_bias` (channels, may be NULL) folds the bias of the
 * convolution in front of the norm (the MLP's fc2, makani/models/common/layers.py:768-823) into both passes: the norm
 * sees (x + pre_bias[c]) rounded to the tensor dtype, exactly the tensor the reference materialises; same in backward.
 * `quad` (hw floats, may be NULL; `quad_sum` = their sum Q, 1 on a full grid, < 1 on a crop) switches to
 * quadrature-weighted statistics mean = sum q x, var = sum q (x - mean)^2: GeometricInstanceNormS2
 * (makani/models/common/layer_norm.py:30-160); the backward then is
 * gx_i = rstd gamma (ga_i - q_i (S1 + (n_i - mean rstd (1 - Q)) S2)) with the unweighted sums S1 = sum ga, S2 = sum ga n. */
int mk_instnorm_fwd(const void* x, void* y, int dtype, float* stats, float* ws, const float* gamma, const float* beta,
                    const float* pre_bias, const float* quad, float quad_sum, long long planes, int channels, long long hw,
                    float eps, int fuse_gelu, void* stream);
int mk_instnorm_bwd(const void* x, const void* gy, void* gx, int dtype, const float* stats, const float* gamma,
                    const float* beta, const float* pre_bias, const float* quad, float quad_sum, float* sums, float* ws, long long planes, int channels, long long hw,
                    long long hw_total, int phase, int fuse_gelu, void* stream);
/* The same norm in ONE pass over the plane (round 6): a block keeps its chunk of the plane in registers between the
 * statistics and the apply phase — 2 plane-sized transfers forward instead of 3, 3 backward instead of 5 — and the blocks of a
 * plane hand their partial sums over through 64-bit agent-scope atomics (csrc/pointwise.hip: in_fwd_fused).  Serves unweighted
 * statistics on planes whose size is a multiple of the 16-byte vector; mk_instnorm_fused_chunks returns 0 otherwise (use the
 * two-kernel entry points above).  `slots`: planes * mk_instnorm_fused_chunks(..., kind) 64-bit words, ALL ONES before the first
 * launch; `depart`: planes 32-bit words, ZERO before the first launch; the kernels leave both as they found them, so one pair
 * serves every later launch on the same stream (never two launches that may run concurrently).  Same arithmetic and outputs
 * as mk_instnorm_fwd / mk_instnorm_bwd (phase 0) — nn.InstanceNorm2d, makani/models/networks/sfnonet.py:618-620. */
int mk_instnorm_fused_chunks(long long hw, int dtype, long long planes, int kind);   /* kind: 0 forward, 1 backward, 2 backward + GELU */
int mk_instnorm_fwd_fused(const void* x, void* y, int dtype, float* stats, const float* gamma, const float* beta,
                          const float* pre_bias, void* slots, void* depart, long long planes, int channels, long long hw,
                          float eps, int fuse_gelu, void* stream);
int mk_instnorm_bwd_fused(const void* x, const void* gy, void* gx, int dtype, const float* stats, const float* gamma,
                          const float* beta, const float* pre_bias, float* sums, void* slots, void* depart, long long planes,
                          int channels, long long hw, int fuse_gelu, void* stream);
/* The statistics of mk_instnorm_fwd_fused WITHOUT its apply phase, for a consumer that normalises the plane where it reads it
 * (mk_conv1x1_nn_rnorm): stats (planes, 2) = (mean, rstd), bit for bit what mk_instnorm_fwd_fused writes for the same input, and
 * coef (planes rounded up to a multiple of 8, 2) = (sc, sh) = (rstd gamma, beta - mean rstd gamma), the two numbers of the apply
 * y = bf16(pre(x) sc + sh); rows past `planes` are not written.  ws: planes * mk_instnorm_fused_chunks(hw, dtype, planes, 0) * 2
 * floats, no initial state.  Two launches ordered by the stream: partial sums per chunk (plain stores), then one block per
 * plane; no hand-over between workgroups. */
int mk_instnorm_stats_fused(const void* x, int dtype, float* stats, float* coef, float* ws, const float* gamma, const float* beta,
                            const float* pre_bias, long long planes, int channels, long long hw, float eps, void* stream);
/* y = gelu(x + bias[c])  — the bias+activation of the 1x1 convolutions in MLP / EncoderDecoder
 * (makani/models/common/layers.py:603-643,768-823).  bias may be NULL (plain GELU).
 * Backward: gx = gy * gelu'(x + bias[c]); optional sums (2, planes): sums[0][p] = sum gx (bias grad). */
int mk_bias_gelu_fwd(const void* x, const float* bias, void* y, int dtype, long long planes, int channels,
                     long long hw, void* stream);
int mk_bias_gelu_bwd(const void* x, const float* bias, const void* gy, void* gx, float* sums, float* ws, int dtype,
                     long long planes, int channels, long long hw, void* stream);

/* ---- quadrature-weighted L^p plane sums (geometric losses) ---------------------------------
 * Replace GridQuadrature.forward (makani/utils/grids.py:185-191) and the elementwise chain of
 * GeometricLpLoss.abs/rel (makani/utils/losses/lp_loss.py:61-107) and their autograd:
 *   mode 0:  sums[0][plane] = sum_i q[i] * a[plane][i] (* wgt[plane][i])
 *   mode 1:  sums[0][plane] = sum_i q[i] * |a[plane][i] - b[plane][i]|^p (* wgt[plane][i])     (b NULL = 0)
 * a, b: (planes, hw) f32 | bf16 independently (prediction bf16, target f32); q: (hw) f32 quadrature weights;
 * wgt: optional (planes, hw) f32; sums: (2, planes) f32 (second row 0); ws: planes * mk_quad_lp_chunks(hw) * 2
 * floats of scratch.  Backward: da = g[plane] * q * wgt * d|d|^p/dd (mode 0: g * q * wgt), db = -da; either may be
 * NULL; gradients are written in the dtype of the tensor they belong to. */
int mk_quad_lp_chunks(long long hw);
int mk_quad_lp_fwd(const void* a, int a_dtype, const void* b, int b_dtype, const float* wgt, const float* q,
                   float* sums, float* ws, long long planes, long long hw, int mode, float p, void* stream);
int mk_quad_lp_bwd(const void* a, int a_dtype, const void* b, int b_dtype, const float* wgt, const float* q,
                   const float* g, void* da, void* db, long long planes, long long hw, int mode, float p, void* stream);

/* ---- spectral L^p sums on the S-layout (spectral losses) ------------------------------------
 * Replace the chain |coeffs|^p * wgt, the m = 0 once / m > 0 twice Parseval sum over m and the sum over l of
 * SpectralLpLoss.abs/rel (makani/utils/losses/lp_loss.py:141-247) and their autograd, directly on the SHT output:
 *   partial[b][row] = sum over the 32 (l, m) pairs of block b with l + tri_off >= m of w(m) |c_lm|^p (* wgt[l][m][row])
 * w(m) = w0 when m + m_off == 0 (global order 0), else w1.  S: (L, M, 2, R) f32; wgt: optional (L, M, R) f32;
 * partial: (mk_spec_lp_blocks(L, M), R) f32, summed over its first axis by the caller.
 * Backward: dS = g[row] * w(m) * p * |c|^(p-2) * c (* wgt), exact zeros where l + tri_off < m. */
long long mk_spec_lp_blocks(int L, int M);
int mk_spec_lp_fwd(const float* S, const float* wgt, float* partial, int L, int M, long long R, int tri_off, int m_off,
                   float p, float w0, float w1, void* stream);
int mk_spec_lp_bwd(const float* S, const float* wgt, const float* g, float* dS, int L, int M, long long R, int tri_off,
                   int m_off, float p, float w0, float w1, void* stream);

/* ---- spectral contractions that are not matrix products over l --------------------------------
 * Activations x, y, gy: S-layout (L, M, 2, R) f32; position (l, m) is live when m <= l + tri_off, dead positions
 * are written as exact zeros and never read.
 *
 * mk_spec_sep_mul / mk_spec_sep_wgrad: the separable operators _contract_sep_lmwise ("bgixy,gixy->bgixy") and
 *   _contract_sep_lwise ("bgixy,gix->bgixy") (makani/models/common/contractions.py:26-31) and their autograd.
 *   R = B*Cp, Cp % 4 == 0.  w, gw: the weight in S-layout (L, Mw, 2, Cp), Mw = M (lm-wise) or 1 (l-wise).
 *     sep_mul:   y = x * w            (conj_w = 0: forward)      y = x * conj(w)   (conj_w = 1: input gradient of gy)
 *     sep_wgrad: gw[l][mw][c] = sum_b (and sum over live m when Mw == 1) conj(x) * gy
 *
 * mk_spec_diag_apply / mk_spec_diag_wgrad: the dense diagonal operator _contract_lmwise ("bgixy,gioxy->bgoxy",
 *   contractions.py:17-18) for ONE group.  w_c64 / gw_c64: the group's slice of the PARAMETER, (Cin, Cout, L, M)
 *   complex64, read and written in place (every weight byte crosses HBM exactly once, coalesced along (l, m)).
 *   x: Cin channels inside rows of stride x_ld per batch entry (R_x = B*x_ld), y likewise with y_ld; pointers may be
 *   offset to a group's first channel.
 *     diag_apply dgrad = 0: y[p][b][o] = sum_i x[p][b][i] * w[i][o][p]; channels [Cout, Cout + y_pad) are zeroed
 *                dgrad = 1: x is gy (Cout channels), y is gx[p][b][i] = sum_o gy[p][b][o] * conj(w[i][o][p])
 *     diag_wgrad: gw[i][o][p] = sum_b conj(x[p][b][i]) * gy[p][b][o] */
int mk_spec_sep_mul(const float* x, const float* w, float* y, int L, int M, int Mw, int B, int Cp, int tri_off, int conj_w,
                    void* stream);
int mk_spec_sep_wgrad(const float* x, const float* gy, float* gw, int L, int M, int Mw, int B, int Cp, int tri_off, void* stream);
int mk_spec_diag_apply(const float* x, const float* w_c64, float* y, int L, int M, int B, int Cin, int Cout, int x_ld, int y_ld,
                       int y_pad, int tri_off, int dgrad, void* stream);
int mk_spec_diag_wgrad(const float* x, const float* gy, float* gw_c64, int L, int M, int B, int Cin, int Cout, int x_ld, int y_ld,
                       int tri_off, void* stream);

/* ---- bf16 channel GEMMs (1x1 convolutions on NCHW planes) ---------------------------------
 * Replace nn.Conv2d(kernel_size=1) of MLP / EncoderDecoder / outer_skip / residual_transform
 * (makani/models/common/layers.py:603-643,768-823; makani/models/networks/sfnonet.py:335-338,726-730)
 * and its autograd under bf16 autocast.  All tensors bf16 except bias (f32) and dW/part (f32).
 *   mk_conv1x1_nn:   Y[b][m][n] = epi( sum_k A[m][k] X[b][k][n] ),  n = pixel (contiguous), n % 8 == 0
 *       A: (M, lda) k-contiguous, zero padded to lda (multiple of 8).  Forward: A = W; dgrad: A = W^T.
 *       epi(v) = v + bias[m]; if act: (Ypre = v), v = gelu(v); if G: v *= gelu'(G[b][m][n]); if R: v += R[b][m][n].
 *   mk_conv1x1_wgrad: dW[m][k] (+)= sum_{b,n} G[b][m][n] X[b][k][n]; `part` = scratch of
 *       mk_conv1x1_wgrad_workspace(M, K, B, N) floats, laid out as (S, M, K) split-pixel partial tiles FOLLOWED BY (S, M)
 *       partial row sums of G (S = the kernel's pixel splits; both reduced deterministically).  The query returns
 *       S*M*K + S*M; mk_conv1x1_wgrad_bias REQUIRES a scratch of the size this version of the query returns (a caller that
 *       sized it as S*M*K, the layout before the bias sums existed, would be overrun by S*M floats).
 *   mk_conv1x1_wgrad_bias: the same and, from the same pass over G, the bias gradient of the convolution
 *       db[m] = sum_{b,n} G[b][m][n] (what torch's conv backward returns as grad_bias; fp32, M entries, overwritten) —
 *       available where mk_conv1x1_wgrad_fuses_bias(M, K, B, N) returns 1 (the streaming "ring" kernel), else the caller
 *       takes the plane sums with mk_plane_sums. */
int mk_conv1x1_nn(const void* A, const void* X, void* Y, void* Ypre, const float* bias, const void* R, const void* G,
                  int M, int K, int lda, int B, long long N, int act, void* stream);
/* Y = A X (+ bias) + norm(R [+ pre_bias]): mk_conv1x1_nn whose residual operand R is the INPUT of an instance norm that nobody
 * else consumes.  coef (B * channels, 2): (sc, sh) per plane of R from mk_instnorm_stats_fused; pre_bias (channels) or NULL: the
 * constant folded in front of the norm; channels == M.  The epilogue adds bf16(bf16(R + pre_bias[c]) sc + sh), bit for bit the
 * tensor mk_instnorm_fwd_fused would have written, so Y equals the two-step result.  Ypre, G and act must be NULL / 0.  Served
 * exactly where mk_conv1x1_nn_rnorm_supported returns 1 (where mk_conv1x1_nn runs its two-group weight-stationary kernel for a
 * call with R); any other shape is an error. */
int mk_conv1x1_nn_rnorm(const void* A, const void* X, void* Y, void* Ypre, const float* bias, const void* R, const void* G,
                        int M, int K, int lda, int B, long long N, int act, const float* coef, const float* pre_bias, int channels,
                        void* stream);
int mk_conv1x1_nn_rnorm_supported(int M, int K, int lda, int B, long long N);
long long mk_conv1x1_wgrad_workspace(int M, int K, int B, long long N);
int mk_conv1x1_wgrad(const void* G, const void* X, float* dW, float* part, int M, int K, int B, long long N,
                     int accumulate, void* stream);
int mk_conv1x1_wgrad_fuses_bias(int M, int K, int B, long long N);
int mk_conv1x1_wgrad_bias(const void* G, const void* X, float* dW, float* dbias, float* part, int M, int K, int B, long long N,
                          int accumulate, void* stream);

/* ---- optimizer ------------------------------------------------------------------------
 * One fused AdamW update (torch.optim.AdamW semantics: decoupled weight decay, bias correction with
 * `step` >= 1) over a flat fp32 tensor; complex64 parameters are passed as their real view
 * (as makani views them, makani/mpu/mappings.py:467-489).  The reference's train step uses AdamW
 * (config/sfnonet.yaml:50-54) after global-norm clipping (utils/training/training_helpers.py:123-165):
 * `grad_scale` (device pointer, may be NULL) is that clipping coefficient, applied to g on the fly. */
int mk_adamw_step(float* p, const float* g, float* m, float* v, long long n, const float* grad_scale, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step, const float* step_state, void* stream);
/* Device-side step counter: `state` = 3 floats {step, 1 / (1 - beta1^step), 1 / sqrt(1 - beta2^step)} (zero-initialised by
 * the caller); one launch increments the step and refreshes the two bias corrections.  The update kernels read them when
 * `step_state` is non-NULL (and ignore `step`): no launch argument depends on the step number, which is what makes a
 * captured hipGraph of the whole train step replayable. */
int mk_adamw_advance(float* state, float beta1, float beta2, void* stream);
/* The same update over `count` tensors (host array of descriptors) in ceil(count / 48) launches: for the ~80 small
 * tensors of the model, where one launch each costs more in dispatch gaps than in HBM time. */
typedef struct MkAdamTensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long n;
    void* p_bf16;   /* optional (mk_adamw_multi only): receives bf16(updated p), the autocast operand of the next step */
    void* p_bf16_t; /* optional: receives bf16(updated p) transposed (needs cols > 0): the data-gradient GEMM's operand */
    int cols;       /* > 0: p is an (n / cols, cols) matrix; then p_bf16 has row pitch ld, p_bf16_t row pitch ld_t */
    int ld, ld_t;
} MkAdamTensor;
int mk_adamw_multi(const MkAdamTensor* tensors, int count, const float* grad_scale, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int step, const float* step_state, void* stream);
/* Global gradient norm and the clipping coefficient of makani/utils/training/training_helpers.py:123-165 over all
 * `tensors[i].g` (only g and n are read): out[0] = min(1, max_norm / (norm + 1e-6)) (1 if max_norm <= 0), out[1] = norm.
 * `partial` needs mk_grad_norm_workspace() floats.  ceil(count / 48) + 1 launches, fixed summation order. */
long long mk_grad_norm_workspace(const MkAdamTensor* tensors, int count);
int mk_grad_clip_coef(const MkAdamTensor* tensors, int count, float max_norm, float* partial, float* out, void* stream);
/* The same with `npre` buffers of ALREADY SQUARED partial sums (pre[i].g = the buffer, pre[i].n = its length; e.g. the ssq_part of
 * mk_cgemm_split2_batched_ssq) standing in for the tensors they were formed from: norm^2 = sum of squares of tensors[] + sum of pre[].
 * `partial` needs mk_grad_norm_workspace_pre() floats; count or npre may be 0. */
long long mk_grad_norm_workspace_pre(const MkAdamTensor* tensors, int count, const MkAdamTensor* pre, int npre);
int mk_grad_clip_coef_pre(const MkAdamTensor* tensors, int count, const MkAdamTensor* pre, int npre, float max_norm, float* partial,
                          float* out, void* stream);

/* ---- layer norm over the channels of an NCHW tensor ------------------------------------------------------------------
 * Replaces DistributedLayerNorm (makani/mpu/layer_norm.py:256-290: nn.LayerNorm(C) between two transposes of the NCHW
 * activation; `normalization_layer="layer_norm"`, makani/models/networks/sfnonet.py:609-613, fourcastnet3.py:95-96) and its
 * autograd without the transposes.  x, y, gy, gx: (B, C, P) planes (P = H * W grid points); stats: (B, 2, P) f32 = [mean,
 * rstd] per grid point; gamma / beta: (C) f32 or NULL.  dtypes: x f32 -> y f32; x bf16 -> y f32 (nn.LayerNorm under
 * autocast) or bf16; gy has y's dtype, gx has x's.
 * wgrad: partial[(2, C, mk_chan_layernorm_chunks(C, P))] = per-chunk sums of gy * xhat (dgamma) and gy (dbeta). */
int mk_chan_layernorm_chunks(int C, long long P);
int mk_chan_layernorm_fwd(const void* x, int x_dtype, void* y, int y_dtype, float* stats, const float* gamma, const float* beta,
                          int B, int C, long long P, float eps, void* stream);
int mk_chan_layernorm_bwd(const void* x, int x_dtype, const void* gy, int g_dtype, void* gx, const float* stats,
                          const float* gamma, int B, int C, long long P, void* stream);
int mk_chan_layernorm_wgrad(const void* x, int x_dtype, const void* gy, int g_dtype, const float* stats, float* partial, int B,
                            int C, long long P, void* stream);

/* ---- ensemble CRPS on the sphere -----------------------------------------------------------------------------------
 * Pointwise score over the ensemble dimension fused with the quadrature over the plane: replaces the kernels of
 * makani/utils/losses/crps_loss.py:124-275 ("skillspread" = type 0, the default of CRPSLoss :277-452; "probability weighted
 * moment" = 1; "naive skillspread" = 2; "gauss" = 3) and the piecewise-integrated "cdf" form of :55-122 (type 4: members in
 * rank order, optional per-member ensemble weights `ens_w` (E) — `self.ensemble_weights[idx]` of :392-396), the weighted sum
 * of :435-438 and their autograd.
 * f: (B, E, C, hw) forecasts, obs: (B, C, hw), q: (hw) quadrature weights, w: optional (B, C, hw) spatial weights.
 * grad == 0: partial[(B * C) * mk_crps_chunks(hw)] chunk sums of q * w * crps (the caller adds the chunks of a plane);
 * grad == 1: gf (shape / dtype of f) = gout[b * C + c] * q * w * d crps / d f_e.  Any 2 <= E <= 32 (members live in registers). */
int mk_crps_chunks(long long hw);
int mk_crps(const void* f, int f_dtype, const void* obs, int o_dtype, const float* q, const float* w, const float* gout,
            float* partial, void* gf, int B, int E, int C, long long hw, int type, float alpha, float eps, int grad,
            const float* ens_w, void* stream);
/* The "naive skillspread" score on COMPLEX members — SpectralCRPSLoss(absolute=False), makani/utils/losses/crps_loss.py:205-243,
 * 536-545: |.| is the complex modulus.  f (B, E, C, hw) and obs (B, C, hw) complex64 (re, im interleaved); gf like f (torch's
 * complex-gradient convention); q / w / gout / partial as mk_crps. */
int mk_crps_complex(const void* f, const void* obs, const float* q, const float* w, const float* gout, float* partial, void* gf,
                    int B, int E, int C, long long hw, float alpha, int grad, void* stream);

/* ---- ensemble energy scores (grid Lp, Sobolev, per-degree spectral L2) ------------------------------------------------
 * Replace the pair tensors of makani/utils/losses/energy_score.py:30-652 (LpEnergyScoreLoss, SobolevEnergyScoreLoss,
 * SpectralL2EnergyScoreLoss) and their autograd; three stages (makani_amd/csrc/escore.hip).
 * f: (B, E, C, N) members, kind MK_F32 | MK_BF16 | 2 = complex64 (re, im interleaved; p = 2); obs: (B, C, N) f32 (complex64
 * for kind 2); q: (N) weights; w: optional (B, C, N) f32.  The plane of N points is S segments of N / S points (S = 1, or one
 * per degree of an (L, M) plane).  K = E + E (E - 1) / 2 sums per segment: E skills, then the pairs i < j in lexicographic
 * order.  nanmode 0: a NaN observation masks the point, a NaN member counts as 0; 1: a NaN observation or member masks it.
 * 1 <= E <= 32, p >= 1.
 * mk_escore_sums:   sums (B, C, S, K) f32; ws: mk_escore_sums_workspace(...) floats of scratch (NULL when that is 0).
 * mk_escore_finish: sums -> loss (B, Cout) and table (B, Cout, S, K) = d loss / d sums (0 where a sum is below eps);
 *                   Cout = reduce ? 1 : C (channels summed in order); scale: optional (nscale = 1 | Cout) spread factors.
 * mk_escore_grad:   gf (shape / dtype of f) = gout[b][co] * q * w * sum_k table[b][co][s][k] d term_k / d f_e; 0 where masked. */
long long mk_escore_sums_workspace(int B, int E, int C, long long N, int S, int nanmode);
int mk_escore_sums(const void* f, int kind, const void* obs, const float* q, const float* w, float* sums, float* ws, int B, int E,
                   int C, long long N, int S, int nanmode, float p, void* stream);
int mk_escore_finish(const float* sums, const float* scale, int nscale, float* loss, float* table, int B, int E, int C, int S,
                     int reduce, float p, float beta, float alpha, float eps, void* stream);
int mk_escore_grad(const void* f, int kind, const void* obs, const float* q, const float* w, const float* table, const float* gout,
                   void* gf, int B, int E, int C, int Cout, long long N, int S, int nanmode, float p, void* stream);

/* Stage 2 of the Gaussian maximum mean discrepancy (GaussianMMDLoss, makani/utils/losses/mmd_loss.py:30-219) between
 * mk_escore_sums (S = 1, p = beta, nanmode 1) and mk_escore_grad: sums (B, C, 1, K) -> k = exp(-s^2 / 2 sigma) of the (optionally
 * channel-summed) sums, loss (B, Cout) = sum_e k_e / E - (E - 1 + alpha) / (E^2 (E - 1)) sum_{i<j} k_ij (0 spread for E = 1) and
 * table (B, Cout, 1, K) = d loss / d sums. */
int mk_mmd_finish(const float* sums, float* loss, float* table, int B, int E, int C, int reduce, float sigma, float alpha, void* stream);

/* ---- adjusted mean squared error in spectral space (SpectralAMSELoss, makani/utils/losses/amse_loss.py:29-114) --------
 * X, Y: (R, L, M) complex64 coefficient planes (re, im interleaved); wgt: optional (R, L, M) f32.  c_m = 1 for the global order
 * m + m_off = 0, else 2; orders m > l + tri_off are structurally zero (tri_off = l_off - m_off of a shard).
 * mk_amse_sums: sums (R, L, 3) = sum_m c_m wgt / 4 pi of |x|^2, |y|^2, Re(x conj y).
 * mk_amse_grad: t (R, L, 3) = d loss / d sums -> dX = c_m wgt / 4 pi (2 t0 x + t2 y), dY (optional) = c_m wgt / 4 pi (2 t1 y + t2 x),
 * complex64 in torch's complex-gradient convention, zeros at the structurally zero orders. */
int mk_amse_sums(const float* X, const float* Y, const float* wgt, float* sums, long long R, int L, int M, int tri_off, int m_off,
                 void* stream);
int mk_amse_grad(const float* X, const float* Y, const float* wgt, const float* t, float* dX, float* dY, long long R, int L, int M,
                 int tri_off, int m_off, void* stream);

/* ---- per-degree ensemble Gram matrix in spectral space (SpectralCoherenceLoss, makani/utils/losses/energy_score.py:655-856;
 * CoherenceRegularization and SpectralRegularization, makani/utils/losses/regularization.py:84-417; makani_amd/csrc/egram.hip).
 * f: (B, E, C, L, M) complex64 members (re, im interleaved), o: (B, C, L, M) complex64 observation, q: (L, M) f32 weights with every
 * constant folded in (1 / 4 pi, 2 for m > 0, 0 for m > l).  Fields x_0 .. x_{E-1} = members, x_E = observation, n = E + 1.
 * mk_egram_sums: G (B, C, L, K) f32, G[i][j] = sum_m q Re(conj(x_i) x_j); slots of a row: [0, n) G[i][i]; [n, n + E) G[e][E];
 *   [n + E, n + E + E (E - 1) / 2) G[i][j], i < j < E, lexicographic.  `what` truncates the row: DIAG K = n, OBS K = n + E, FULL all.
 * mk_egram_grad: dG (B, C, L, K) -> gf (B, E, C, L, M) complex64 = q (2 dG[e][e] x_e + dG[e][E] x_E + sum_{j != e} dG[e, j] x_j) in
 *   torch's complex-gradient convention; the observation gets none.
 * Orders m > l + tri_off are not read (q is 0 there) and get exact zeros in gf; tri_off >= M skips nothing.  1 <= E <= 32, more:
 * MK_EUNSUP. */
#define MK_EGRAM_DIAG 0
#define MK_EGRAM_OBS 1
#define MK_EGRAM_FULL 2
int mk_egram_sums(const void* f, const void* o, const float* q, float* G, int B, int E, int C, int L, int M, int what, int tri_off,
                  void* stream);
int mk_egram_grad(const void* f, const void* o, const float* q, const float* dG, void* gf, int B, int E, int C, int L, int M, int what,
                  int tri_off, void* stream);

/* ---- Gaussian negative log likelihood of an ensemble (EnsembleNLLLoss, makani/utils/losses/likelihood_loss.py:30-134) ----
 * f: (B, E, C, hw) members f32 | bf16, obs: (B, C, hw) f32, q: (hw), w: optional (B, C, hw) f32.
 * nll = 0.5 (log s2 + (obs - mu)^2 / s2), mu the ensemble mean, s2 = max(centred variance (correction 0), eps^2).
 * grad == 0: partial[(B * C) * mk_ens_nll_chunks(hw)] chunk sums of q * w * nll (the caller adds the chunks of a plane);
 * grad == 1: gf (shape / dtype of f) = gout[b * C + c] * q * w * d nll / d f_e (no gradient through an active clamp).  1 <= E <= 32. */
int mk_ens_nll_chunks(long long hw);
int mk_ens_nll(const void* f, int f_dtype, const float* obs, const float* q, const float* w, const float* gout, float* partial, void* gf,
               int B, int E, int C, long long hw, float eps, int grad, void* stream);

/* ---- plane sums of the geometric validation metrics (makani/utils/metrics/functions.py:29-677) ----------------------------
 * q: (N) quadrature weights, w: optional (B, C, N) f32 spatial weights, ws: workspace, out: fp32.  Every block writes the sums
 * of its chunk of a plane to ws, a second launch adds the mk_metric_chunks(N) chunks of a plane in chunk order: repeats are
 * bit-identical.  Entries of out not selected by `which` are not written.  16-byte accesses when N is a multiple of 4 and every
 * pointer is 16-byte aligned, scalar ones otherwise.  B * C <= 65535.
 * mk_metric_det_sums: x, y (B, C, N) f32 | bf16 each, bias optional (C, N) f32 (GeometricACC's climatology, :184-188).
 *   out (B, C, 5) = sum_p q w {|x - y|, (x - y)^2, x'y', x'^2, y'^2}, x' = x - bias, y' = y - bias; which: bit k selects sum k
 *   (MK_METRIC_L1 GeometricL1 :53-71, MK_METRIC_L2 GeometricRMSE :110-132, MK_METRIC_XY | XX | YY GeometricACC :184-218);
 *   ws: B * C * mk_metric_chunks(N) * 5 floats.
 * mk_metric_ens_sums: f (B, E, C, N) members f32 | bf16 read in place, obs (B, C, N) f32, 1 <= E <= 32.
 *   out (B, C, E + 3): [0] skill = sum_p q w (mu - obs)^2, [1] spread = sum_p q w sum_e (mu - f_e)^2 (GeometricSSR :394-414,
 *   GeometricSpread :287-299; mean first, then centred squares), [2 + k] = sum_p q w [r = k] for r = #{e : f_e <= obs}, the
 *   insertion index of sort + searchsorted(side="right") + one_hot (GeometricRankHistogram :639-656) for finite inputs;
 *   which: MK_METRIC_SKILL | MK_METRIC_SPREAD | MK_METRIC_HIST; ws: B * C * mk_metric_chunks(N) * (E + 3) floats. */
#define MK_METRIC_L1 1
#define MK_METRIC_L2 2
#define MK_METRIC_XY 4
#define MK_METRIC_XX 8
#define MK_METRIC_YY 16
#define MK_METRIC_SKILL 1
#define MK_METRIC_SPREAD 2
#define MK_METRIC_HIST 4
int mk_metric_chunks(long long N);
int mk_metric_det_sums(const void* x, int x_dtype, const void* y, int y_dtype, const float* bias, const float* w, const float* q,
                       float* out, float* ws, int B, int C, long long N, int which, void* stream);
int mk_metric_ens_sums(const void* f, int f_dtype, const float* obs, const float* w, const float* q, float* out, float* ws, int B,
                       int E, int C, long long N, int which, void* stream);

/* ---- a rollout step's validation metrics in one pass (makani/utils/metric.py:45-740: MetricsHandler.update) ----------------
 * mk_mrollout_sums: every plane sum that any metric handle of a MetricsHandler needs, in ONE read of the selected planes.
 *   pred (B, E, C, N) members f32 | bf16 read in place (E = 1: a deterministic prediction), tar (B, C, N) f32 | bf16,
 *   w optional (B, C, N) f32, q (N), clim optional (Ja, N) f32.  table: DEVICE int32 (J, 3) = per plane {source channel in
 *   0 .. C-1, MK_MROLL_* bits of the sums wanted from it, row of clim or -1}; a row outside these ranges yields zeros.
 *   Per point: nan = isnan(t) (only when mask_nan), t' = nan ? 0 : t, w' = q w (nan ? 0 : 1), mu = the member mean in fp32
 *   (mean first, centred on the first member).  partial[((b J + j) chunks + chunk) K + k], K = MK_MROLL_NSUM + E + 1,
 *   chunks = mk_metric_chunks(N); every k is written (0 where not selected):
 *     k = 0 sum w'   1 number of NaN points   2 sum w'|mu - t'|   3 sum w'(mu - t')^2   4, 5, 6 sum w'{x'y', x'^2, y'^2} with
 *     x' = mu - clim, y' = t' - clim   7 sum w' sum_e (mu - f_e)^2   8 sum w' crps ("skillspread", alpha = 1; needs E >= 2)
 *     9 + r  sum w' [r = #{e : f_e <= t'}], r = 0 .. E.
 *   sums: optional (B, J, K); when given, a second launch adds the chunks of a plane in chunk order into it (what a spatially
 *   split job all-reduces before the finish).  1 <= E <= 32, B * J <= 65535.
 * mk_mrollout_finish: ONE launch for all nh handles.  sums (B, J, chunks, K) (chunks = 1 for the reduced sums): the chunks are
 *   added in order, every handle's metric is formed per sample and summed over the batch, scaled, and merged into row idt of
 *   its curve and counter in buf (curve += new; MK_MROLL_KIND_RMSE: sqrt(curve^2 + new^2); counter += counts).  counts = B
 *   when has_weight == 0 and the handle's planes hold no NaN point in this batch, sum_b sums[.., 0] otherwise: decided here.
 *   hdesc: DEVICE int32 (nh, MK_MROLL_HDESC) = {kind, channels n, offset into hplanes / hscale, offset of the curve in buf,
 *   offset of the counter in buf, rollout steps}; hplanes: the plane j of every handle channel; hscale: its scale.
 *   curve (steps, n) ((steps, n, E + 1) for MK_MROLL_KIND_HIST), counter (steps, n).  Writes outside [0, buf_len) are dropped. */
#define MK_MROLL_L1 1
#define MK_MROLL_L2 2
#define MK_MROLL_ACC 4
#define MK_MROLL_SPREAD 8
#define MK_MROLL_CRPS 16
#define MK_MROLL_HIST 32
#define MK_MROLL_NSUM 9
#define MK_MROLL_HDESC 6
#define MK_MROLL_KIND_L1 0
#define MK_MROLL_KIND_RMSE 1
#define MK_MROLL_KIND_ACC 2
#define MK_MROLL_KIND_CRPS 3
#define MK_MROLL_KIND_SPREAD 4
#define MK_MROLL_KIND_SSR 5
#define MK_MROLL_KIND_HIST 6
int mk_mrollout_sums(const void* pred, int p_dtype, const void* tar, int t_dtype, const float* w, const float* q, const float* clim,
                     const int* table, float* partial, float* sums, int B, int E, int C, int J, int Ja, long long N, int mask_nan,
                     void* stream);
int mk_mrollout_finish(const float* sums, int chunks, const int* hdesc, const int* hplanes, const float* hscale, float* buf,
                       long long buf_len, int nh, int B, int E, int J, int idt, int has_weight, float acc_eps, float ssr_eps,
                       void* stream);

/* ---- spectral noise processes on the sphere (makani/models/noise.py: BaseNoiseS2 / DiffusionNoiseS2 / DummyNoiseS2 update) ----
 * state: (B, T, C, L, M, 2) f32, updated in place in one pass (makani_amd/csrc/noise.hip).  s = reflect ? -1 : 1.
 *   MK_NOISE_WHITE:   state[:, t] = s xi[t]                                                     (T levels drawn)
 *   MK_NOISE_AR:      levels 1 .. T-1 move to 0 .. T-2; new last = phi[c] old last + s sigma[c][l] xi          (1 level drawn)
 *   MK_NOISE_REPLACE: eta[t] = s sigma[c][l] xi[t]; new[0] = eta[0] / sqrt(1 - phi[c]^2); new[t] = phi[c] new[t-1] + eta[t]   (T levels)
 * sigma (C, L), phi (C) f32 (unused, may be NULL, for MK_NOISE_WHITE).
 * xi = NULL: standard normals from Philox4x32-10 + Box-Muller; rng = device int64 {seed, offset}, key = seed, counter =
 *   (g, offset + t) with g the index of a group of four consecutive elements of level t flattened as (B, C, L, M, 2).  The
 *   kernel only reads rng: enqueue mk_noise_advance(rng, levels drawn) behind it.
 * xi != NULL: the innovations are read from xi, (B, 1, C, L, M, 2) for MK_NOISE_AR and (B, T, C, L, M, 2) otherwise; rng is not read.
 * C L M 2 < 2^31.  16-byte accesses when C L M 2 is a multiple of 4 and the pointers are 16-byte aligned, scalar ones otherwise. */
#define MK_NOISE_WHITE 0
#define MK_NOISE_AR 1
#define MK_NOISE_REPLACE 2
int mk_noise_update(float* state, const float* xi, const float* sigma, const float* phi, const long long* rng, int mode, int B,
                    int T, int C, int L, int M, int reflect, void* stream);
int mk_noise_advance(long long* rng, long long n, void* stream);
/* The same update on a BOX of the state, for a sphere split over h x w ranks.  One time level of the GLOBAL array is (B, C, R, S)
 * floats (spectral processes: R = lmax, S = 2 mmax; DummyNoiseS2: R = nlat, S = nlon); this call owns rows [r0, r0 + Rl) and
 * floats [s0, s0 + Sl) of every (batch entry, channel) plane.  state: the local contiguous (B, T, C, Rl, Sl); sigma: (C, Rl), the
 * local slice; phi: (C); xi, when given, shard-shaped like state ((B, 1, C, Rl, Sl) for MK_NOISE_AR) and used as it is.
 * Counter contract: the element with flat index e in the global level (B, C, R, S) takes normal e & 3 of Philox group e >> 2 at
 *   (seed, offset + t).  A box therefore holds the numbers the whole array holds at those positions, whatever the tiling; with
 *   the box equal to the whole array this is mk_noise_update (which calls it).  Groups that straddle a row end or a box edge are
 *   evaluated by every thread that owns one of their lanes; lanes outside the box are neither loaded nor stored.
 * C R S < 2^31.  16-byte accesses when all strides and offsets, global and local, are multiples of 4 floats; 8-byte accesses when
 *   they are even (a spectral (re, im) pair never leaves its group), 16-byte ones for the groups that are whole and locally
 *   aligned; element-wise masks otherwise. */
int mk_noise_update_shard(float* state, const float* xi, const float* sigma, const float* phi, const long long* rng, int mode,
                          int B, int T, int C, int R, int S, int r0, int Rl, int s0, int Sl, int reflect, void* stream);

/* ---- DISCO convolution and S2 resampling (FourCastNet3's local operators) ----------------------------------------
 * Replace th.DiscreteContinuousConvS2's sparse contraction and th.ResampleS2 [torch-harmonics, un-vendored; call sites
 * makani/models/networks/fourcastnet3.py:189-205 (encoder), :356-381 (decoder), :518-534 (local blocks)].
 * The convolution tensor psi[k][t][(i, j)] is handed over as lists (built by makani_amd/disco.py):
 *   forward lists, sorted by (t, k):  off[t * K + k] .. off[t * K + k + 1] index (nrow, nlon, nval) = (input latitude
 *     relative to lat_lo[t], input longitude, value); lat_n[t] rows are touched, max_rows = max_t lat_n[t];
 *   transposed lists for the adjoint: per input latitude (mk_disco_bwd: entries (k, t, lon, val), any nlon_in =
 *     s * nlon_out) or per (input latitude, k) with rows relative to t_lo[i * K + k] and negated longitudes
 *     (mk_disco_bwd_same: nlon_in == nlon_out).
 * mk_disco_fwd:  y[pl * K + k][t][p] = sum_n nval[n] * x[pl][lat_lo[t] + nrow[n]][(nlon[n] + p * s) mod nlon_in]
 *   x: (planes, nlat_in, nlon_in), y: (planes * K, nlat_out, nlon_out) — the NCHW input of the channel GEMM
 *   (mk_conv1x1_nn) that applies the (out, in * K) weight; dtype f32 | bf16, fp32 accumulation.
 * mk_disco_bwd / mk_disco_bwd_same: the adjoint (gradient with respect to x), deterministic gathers.
 * mk_resample_fwd: bilinear interpolation, latitude first (rows lat_a / lat_b with weight lat_w; a row index -1 / -2 is
 *   the longitude mean of the first / last input row: the pole extension), then periodic longitude (lon_l, lon_r, lon_w).
 * mk_resample_bwd: its adjoint from the inverse stencils (CSR per input row / input column / pole). */
int mk_disco_fwd(const void* x, void* y, int dtype, const int* off, const int* nrow, const int* nlon, const float* nval,
                 const int* lat_lo, const int* lat_n, int max_rows, int planes, int K, int nlat_in, int nlon_in,
                 int nlat_out, int nlon_out, void* stream);
int mk_disco_bwd(const void* gy, void* gx, int dtype, const int* off, const int* nk, const int* nt, const int* nlon,
                 const float* nval, int planes, int K, int nlat_in, int nlon_in, int nlat_out, int nlon_out, void* stream);
int mk_disco_bwd_same(const void* gy, void* gx, int dtype, const int* off, const int* nrow, const int* nlon_l,
                      const float* nval, const int* t_lo, const int* t_n, int max_rows, int planes, int K, int nlat_in,
                      int nlon, int nlat_out, void* stream);
/* Run form of the same contraction for nlon_in == nlon_out (FourCastNet3's local blocks and decoder convolutions,
 * fourcastnet3.py:356-381,518-534; forward and adjoint): csrc/disco_runs.hip, sliding-window correlations in registers.
 *   mk_disco_runs_shape: 1 when the run-form kernels take (nlon, max_rows image rows, planes, dtype, img_bf16), with the
 *     longitudes per lane R (4 | 8) and the planes per workgroup PB (4 | 2; *PB_out preset to 2 or 4 asks for exactly
 *     that value); 0 -> use the list kernels above.
 *   lists (makani_amd/disco.py: _build_runs): seg_off[s] .. seg_off[s + 1] index runs (n, 4) = {image row, first longitude,
 *     offset into vals, groups of R values}; vals zero-padded to whole groups plus R trailing zeros.
 *   mk_disco_fwd_runs: segments s = t * K + k, image rows relative to lat_lo[t] (lat_n[t] rows, max_rows their maximum).
 *   mk_disco_bwd_runs: segments s = i * K + k with negated longitudes, image rows = output latitudes relative to
 *     t_lo[(i / lat_group) * K + k] (t_n rows: lat_group = 2 | 4 consecutive latitudes share one staged image).
 *   img_bf16: keep bf16 tensors as bf16 in the LDS row image (half the LDS per workgroup, one conversion per read).
 *   mk_disco_fwd_fused (K = 9): one stream per (output latitude, image row) shared by all basis functions (their filters
 *     live on the same longitude interval): seg_off (nlat_out + 1), runs (n, 4) = {image row relative to lat_lo[t / LG], first
 *     slot = first longitude / 4 (runs aligned to 4 longitudes), value offset, groups}, vals per group K x 4 ([k][tau]);
 *     lat_lo / lat_n per group of LG output latitudes, LG as named by mk_disco_fused_shape for the longitude count. */
int mk_disco_runs_shape(int nlon, int max_rows, int planes, int dtype, int img_bf16, int* R_out, int* PB_out);
int mk_disco_fused_shape(int nlon, int K, int max_rows, int planes, int* LG_out, int* PB_out);
int mk_disco_fwd_fused(const void* x, void* y, int dtype, const int* seg_off, const int* runs, const float* vals,
                       const int* lat_lo, const int* lat_n, int max_rows, int planes, int K, int nlat_in, int nlon, int nlat_out,
                       void* stream);
int mk_disco_fwd_runs(const void* x, void* y, int dtype, const int* seg_off, const int* runs, const float* vals,
                      const int* lat_lo, const int* lat_n, int max_rows, int planes, int K, int nlat_in, int nlon, int nlat_out,
                      int R, int PB, int img_bf16, void* stream);
int mk_disco_bwd_runs(const void* gy, void* gx, int dtype, const int* seg_off, const int* runs, const float* vals,
                      const int* t_lo, const int* t_n, int max_rows, int planes, int K, int nlat_in, int nlon, int nlat_out,
                      int R, int PB, int img_bf16, int lat_group, void* stream);
/* Grouped channel mix with a handful of channels per group (csrc/groupmix.hip): the channel mixes of FourCastNet3's encoders /
 * decoders (th.DiscreteContinuousConvS2 with groups > 1, fourcastnet3.py:189-205,356-381: 8-9 planes in and out per group).
 *   mk_group_mix:        z (B*G, RG, N) = W (G, RG, CG) x (B*G, CG, N); dtype f32 | bf16, fp32 accumulation; the data gradient is
 *                        the same call with the transposed weights.  N a multiple of 4 (f32) / 8 (bf16).
 *   mk_group_mix_wgrad:  partial (B*G * mk_group_mix_blocks(N, dtype, B*G), RG * CG) = per-block sums of dz[r][n] x[c][n]; the caller
 *                        adds the blocks of a group and the batch entries (deterministic).
 *   mk_group_mix_supported: 1 for the instantiated (CG, RG) pairs (8 | 9 each). */
int mk_group_mix_supported(int CG, int RG);
int mk_group_mix_blocks(long long N, int dtype, int BG);
int mk_group_mix(const void* x, const float* W, void* z, int dtype, int B, int G, int CG, int RG, long long N, void* stream);
int mk_group_mix_wgrad(const void* x, const void* dz, float* partial, int dtype, int B, int G, int CG, int RG, long long N,
                       void* stream);
int mk_resample_fwd(const void* x, void* y, int dtype, const int* lat_a, const int* lat_b, const float* lat_w,
                    const int* lon_l, const int* lon_r, const float* lon_w, int planes, int nlat_in, int nlon_in,
                    int nlat_out, int nlon_out, void* stream);
int mk_resample_bwd(const void* gy, void* gx, int dtype, const int* lat_off, const int* lat_t, const float* lat_wt,
                    const int* lon_off, const int* lon_p, const float* lon_wt, const int* pole_off, const int* pole_t,
                    const float* pole_wt, int planes, int nlat_in, int nlon_in, int nlat_out, int nlon_out, void* stream);

/* ---- Preprocessor2D around the network (csrc/preproc.hip; makani/models/preprocessor.py:412-687,1018-1036) ----------------
 * T = n_history + 1 time levels of J = C + U + N channels each: C = WC / T of the window win (B, WC, HW), U of the cached
 * unpredicted features unp (B, T, U, HW), N of the noise noi (B, T, N, HW); f32 | bf16 each, read in place (unp / noi may be
 * NULL when U / N is 0).  omega[t][p] = wt[t] q[p] with q (HW) the normalised quadrature weights and wt (T) the history weights.
 * Statistics mu, sigma (B, J) are fp32.  Workspaces ws are sized with mk_prep_chunks(HW); chunk sums are added in chunk order
 * (no atomics): repeats are bit-identical.  16-byte accesses when HW is a multiple of 4 and every pointer is 16-byte aligned,
 * scalar ones otherwise.  B J, T J + S, B <= 65535.
 *   mk_prep_stats:      mu = sum omega v, sigma = sqrt(sum omega (v - mu)^2); per chunk (weight, mean, M2) about a pivot, merged
 *                       by Chan's formula in fp64.  tri (B, J, 3) fp64 = (sum omega, mean, M2), what ranks of a split sphere
 *                       exchange; mu / sigma or tri may be NULL.  ws: B J mk_prep_chunks(HW) 4 floats.
 *   mk_prep_assemble:   out (B, T J + S, HW): channel t J + j = (v - mu[b][j]) / sigma[b][j], channel T J + s = stat[s] (S, HW);
 *                       mu = sigma = NULL: no normalisation.
 *   mk_prep_finish:     y = (yn - bias) sigma[b][c] + mu[b][c]; yn, y (B, Cout, HW) of one dtype, bias (Cout, HW) f32, the
 *                       statistics (B, J) with J >= Cout; bias, mu, sigma optional each.
 *   mk_prep_bwd_sums:   G (2, B, J): G[0] = gmu - (sum g) / sigma, G[1] = gsig - (sum g xn) / sigma with g (B, T J + S, HW) the
 *                       gradient of out, xn recomputed, gmu / gsig (B, J) optional.  ws: B J mk_prep_chunks(HW) 2 floats.
 *                       need: bit 0 the window's channels, bit 1 the noise channels; channels without a gradient tensor are
 *                       not read (their sums are 0), so unp may be NULL here and in mk_prep_bwd_apply, noi when it gets none.
 *   mk_prep_bwd_apply:  dv = g / sigma + omega (G[0] + xn G[1]) into dwin (shape of win) and, when given, dnoi (shape of noi);
 *                       g or G may be NULL; mu = sigma = NULL: dv = g.
 *   mk_prep_finish_bwd: gmu[b][c] = sum g, gsig[b][c] = sum g (yn - bias), written to index b J + c.  ws: B Cout chunks 2 floats. */
int mk_prep_chunks(long long HW);
int mk_prep_stats(const void* win, int win_dtype, const void* unp, int unp_dtype, const void* noi, int noi_dtype, const float* q,
                  const float* wt, float* mu, float* sigma, double* tri, float* ws, int B, int T, int WC, int U, int N, long long HW,
                  void* stream);
int mk_prep_assemble(const void* win, int win_dtype, const void* unp, int unp_dtype, const void* noi, int noi_dtype, const void* stat,
                     int stat_dtype, const float* mu, const float* sigma, void* out, int out_dtype, int B, int T, int WC, int U, int N,
                     int S, long long HW, void* stream);
int mk_prep_finish(const void* yn, int dtype, const float* bias, const float* mu, const float* sigma, void* y, int B, int Cout, int J,
                   long long HW, void* stream);
int mk_prep_bwd_sums(const void* g, int g_dtype, const void* win, int win_dtype, const void* unp, int unp_dtype, const void* noi,
                     int noi_dtype, const float* mu, const float* sigma, const float* gmu, const float* gsig, float* G, float* ws, int B,
                     int T, int WC, int U, int N, int S, int need, long long HW, void* stream);
int mk_prep_bwd_apply(const void* g, int g_dtype, const void* win, int win_dtype, const void* unp, int unp_dtype, const void* noi,
                      int noi_dtype, const float* q, const float* wt, const float* mu, const float* sigma, const float* G, void* dwin,
                      void* dnoi, int B, int T, int WC, int U, int N, int S, long long HW, void* stream);
int mk_prep_finish_bwd(const void* g, int g_dtype, const void* yn, int yn_dtype, const float* bias, float* gmu, float* gsig, float* ws,
                       int B, int Cout, int J, long long HW, void* stream);

/* ---- online rollout diagnostics (csrc/rollout.hip; makani/utils/inference/rollout_buffer.py:670-1338) ----------------------
 * Running mean and centred sum of squares (M2), fp32, updated in place by Welford's merge.  count: DEVICE pointer to the int64
 * number of samples merged before this call; the kernels only read it, the caller adds B behind the launch on the same stream.
 * With n0 = *count, n = n0 + B, d = mean_b - mean:  mean += d B / n,  m2 += m2_b + d^2 n0 B / n  (mean_b, m2_b: the batch's mean
 * and centred M2 over b, any B >= 1).  Every element is written by one thread: repeats are bit-identical.
 *   mk_welford_update: src (B, Csrc, N) f32 | bf16 read in place, y = scale[c] x[chan[c]] + bias[c] (chan (C) int32 device list of
 *                      source channels, scale, bias (C) f32; NULL each: identity), mean, m2 (C, N).  16-byte accesses when N is a
 *                      multiple of 4 and src, mean, m2 are 16-byte aligned, one point per thread otherwise.  C <= 65535.
 *   mk_power_spectrum: S (L, M, 2, R) S-layout coefficients with row = (b E + e) Cp + c ->
 *                      out[b][c][e0 + e][l] = sum_m c_m |scale[c] s + [m + m_off == 0] bias[c] one[l]|^2, out (B, C, E1, L) f32 | bf16,
 *                      c_m = 1 for the global order 0 and 2 otherwise, orders m > l + tri_off not read (tri_off = l_off - m_off of
 *                      a shard); one (L): the coefficients of the constant field 1 at order 0 (this shard's degrees).
 *   mk_zonal_welford:  F (M, nlat, 2, R) longitude spectra (norm "forward") with row = (b E + e) Cp + c ->
 *                      p_b = c_m latw[k] |scale[c] F + [m == 0] bias[c]|^2 (c_m = 2 for every m >= 1), rounded to bf16 when
 *                      round_bf16, merged over b into mean, m2 (C, E1, nlat, M) at member e0 + e.  nlat <= 65535. */
int mk_welford_update(const void* src, int dtype, const int* chan, const float* scale, const float* bias, float* mean, float* m2,
                      const long long* count, int B, int Csrc, int C, long long N, void* stream);
int mk_power_spectrum(const float* S, const float* scale, const float* bias, const float* one, void* out, int out_dtype, int L, int M,
                      int R, int Cp, int B, int E, int C, int E1, int e0, int tri_off, int m_off, void* stream);
int mk_zonal_welford(const float* F, const float* scale, const float* bias, const float* latw, float* mean, float* m2,
                     const long long* count, int round_bf16, int M, int nlat, int R, int Cp, int B, int E, int C, int E1, int e0,
                     void* stream);

/* ---- physical output constraints (csrc/constraints.hip; makani/models/parametrizations.py:193-231,
 *      makani/utils/constraints.py:91-113,288-320) ------------------------------------------------------------------------------
 * Pointwise in space: one thread per pixel, or per four consecutive pixels when HW is a multiple of 4 and every tensor pointer is
 * 16-byte aligned.  x, y, g, gx are f32 | bf16 of ONE dtype, contiguous (B, C, HW); the arithmetic is fp32.  Channels a layer
 * does not touch are copied in the same launch.  Nothing is read on the host: the launches can be captured in a graph.
 *
 * The column mix (hydrostatic wrapper and projection), x (B, Cin, HW) -> y (B, Cout, HW):
 *     u_k = s_k x[in_ch[k]] + b_k (k < K_in);   f_j = 1 + eps (qs_j x[q_ch[j]] + qb_j) (j < NQ);   u_k *= f_k (k < n_mi)
 *     v_r = [RESID] u_r + beta (sum_k M[r][k] u_k - off_r) (r < K_out);   v_r /= f_r (r < n_mo)
 *     y[out_ch[r]] = (v_r - b'_r) / s'_r;   y[q_out[j]] = Q_ROUNDTRIP ? ((qs_j x + qb_j) - qb_j) / qs_j : x[q_ch[j]];
 *     y[copy_dst[c]] = x[copy_src[c]] (c < NC)
 * with K_in + NQ + NC = Cin and K_out + NQ + NC = Cout: the three lists partition the channels on either side.  K_in, K_out <=
 * MK_CMIX_ROWS, n_mi, n_mo <= NQ <= MK_CMIX_LEVELS.  The two DEVICE tables hold, in this order,
 *     itab (MK_CMIX_ITAB + 2 NC int32): in_ch, out_ch (MK_CMIX_ROWS each), q_ch, q_out (MK_CMIX_LEVELS each), copy_src, copy_dst (NC each);
 *         the entries of the first four lists beyond their count must repeat a VALID channel (they are read, the value is dropped)
 *     ftab (MK_CMIX_FTAB f32): s, b, s', b', off (MK_CMIX_ROWS each), qs, qb (MK_CMIX_LEVELS each), M and its transpose
 *         (MK_CMIX_ROWS x MK_CMIX_ROWS each, row-major, zero beyond K_out x K_in); s, b, off are 0 and s', qs are 1 beyond their count;
 *         then the folded map that the forward reads when NQ = 0 (x -> y is affine there): W = diag(1 / s') ([RESID] I + beta M) diag(s)
 *         as a high and a low f32 limb (MK_CMIX_ROWS x MK_CMIX_ROWS each, W = high + low, zero beyond K_out x K_in) and
 *         c = ([RESID] b + beta (M b - off) - b') / s' likewise (MK_CMIX_ROWS each), both computed in fp64.  y_r = sum_k W[r][k] x_k + c_r
 *         is summed with error compensation and rounded once.
 * The channel indices are NOT checked (the tables are device memory): the caller guarantees in_ch, q_ch, copy_src < Cin and
 * out_ch, q_out, copy_dst < Cout.
 *   mk_cmix_bwd: gx (B, Cin, HW) from g (B, Cout, HW), the transpose of the above; x is read when NQ > 0 only (the terms
 *                through f), and may be NULL otherwise.
 *
 * Non-negativity on the channels with slot[c] >= 0 (slot (C) int32 device, offset (n) f32 device or NULL = 0), w = x + offset[slot[c]]:
 *   mode 0: w sigmoid(w / eps) - offset;  mode 1: leak w + (1 - leak) eps (softplus(w / eps) - ln 2) - offset;  mode 2: max(x, -offset)
 *   mk_nonneg_bwd: gx = g d/dx of the same. */
#define MK_CMIX_ROWS 32
#define MK_CMIX_LEVELS 16
#define MK_CMIX_ITAB (2 * MK_CMIX_ROWS + 2 * MK_CMIX_LEVELS)
#define MK_CMIX_FTAB (7 * MK_CMIX_ROWS + 2 * MK_CMIX_LEVELS + 4 * MK_CMIX_ROWS * MK_CMIX_ROWS)
#define MK_CMIX_RESID 1
#define MK_CMIX_Q_ROUNDTRIP 2
int mk_cmix_fwd(const void* x, void* y, int dtype, const int* itab, const float* ftab, int B, int Cin, int Cout, int K_in, int K_out, int NQ,
                int n_mi, int n_mo, int NC, int flags, float beta, float eps, long long HW, void* stream);
int mk_cmix_bwd(const void* g, const void* x, void* gx, int dtype, const int* itab, const float* ftab, int B, int Cin, int Cout, int K_in,
                int K_out, int NQ, int n_mi, int n_mo, int NC, int flags, float beta, float eps, long long HW, void* stream);
int mk_nonneg_fwd(const void* x, void* y, int dtype, const int* slot, const float* offset, int mode, float eps, float leak, int B, int C,
                  long long HW, void* stream);
int mk_nonneg_bwd(const void* g, const void* x, void* gx, int dtype, const int* slot, const float* offset, int mode, float eps, float leak,
                  int B, int C, long long HW, void* stream);

/* ---- stochastic-interpolant stepper (csrc/interpolant.hip; makani/models/stochastic_interpolant.py:102-163,343-502) -----------
 * Network input X (N, Cin, HW) with the channels [x0 (C) | x (C) | xu (U) | static (St) | s (has_s)], Cin = 2 C + U + St + has_s.
 * Pointwise in space: one thread per pixel, or per four consecutive pixels when HW is a multiple of 4 and every tensor pointer is
 * 16-byte aligned.  Tensors are f32 | bf16 by their dtype argument, contiguous; z, s and D are f32; the arithmetic is fp32.
 * Nothing is read on the host, no workspace, no atomics: the launches can be captured in a graph.  B, Cin <= 65535.
 *   mk_si_assemble: training.  x0, x1 (B, C, HW) of one dtype, z (B, C, HW), s (B, S') DEVICE memory, xu (B, U, HW), stat (St, HW)
 *                   (NULL when U / St = 0).  Row n = b S' + j:  X[n][x0 slot] = x0[b],  X[n][x slot] = (1 - s) x0 + s^2 x1 + sqrt(s) eps (1 - s) z,
 *                   D[n] (N, C, HW) = -x0 + 2 s x1 - eps sqrt(s) z,  X[n][xu slot] = xu[b],  X[n][static slot] = stat,  X[n][s slot] = s[b][j].
 *                   The coefficients are two-float values formed in fp32 from s (eps: a double, split) and the sums are compensated:
 *                   X and D are within fp32 rounding of the fp64 values of the fp32 inputs (two-float arithmetic: about 2^-44 relative
 *                   before the final rounding), also where the terms cancel.
 *   mk_si_step:     sampling.  out = X_next (B, Cin, HW): x0 slot = x0, x slot = cx x + cb b + c0 x0 + cn z, xu, static as above, s slot = s_next;
 *                   x is read at x + b x_stride + c HW (elements: the x slot of the previous input, or x0 itself), b, x0, z (B, C, HW).
 *                   b may be NULL when cb = 0, z when cn = 0 (cx = 1, the rest 0 writes the sampler's first input from x0 alone).
 *                   last != 0: out = x_new (B, C, HW), the x slot alone (U, St, has_s are ignored).
 *   mk_si_step_bwd: g the gradient of out (B, Cin, HW; last: (B, C, HW)):  gx0 = g[x0 slot] + c0 g[x slot] (last: c0 g),
 *                   gx = cx g[x slot],  gb = cb g[x slot], each (B, C, HW), each optional (NULL). */
int mk_si_assemble(const void* x0, const void* x1, int x_dtype, const float* z, const float* s, const void* xu, int xu_dtype,
                   const void* stat, int stat_dtype, void* X, int out_dtype, float* D, double eps, int B, int Sp, int C, int U, int St,
                   int has_s, long long HW, void* stream);
int mk_si_step(const void* x, long long x_stride, int x_dtype, const void* b, int b_dtype, const void* x0, int x0_dtype, const float* z,
               const void* xu, int xu_dtype, const void* stat, int stat_dtype, void* out, int out_dtype, float cx, float cb, float c0,
               float cn, float s_next, int last, int B, int C, int U, int St, int has_s, long long HW, void* stream);
int mk_si_step_bwd(const void* g, int g_dtype, void* gx0, int gx0_dtype, void* gx, int gx_dtype, void* gb, int gb_dtype, float cx, float cb,
                   float c0, int last, int B, int C, int Cin, long long HW, void* stream);

/* ---- hydrostatic-balance loss and the loss handler's preparation pass (csrc/hydro.hip; makani/utils/losses/hydrostatic_loss.py,
 *      makani/utils/loss.py:392-429) -----------------------------------------------------------------------------------------------
 * x (N, C, HW) f32 | bf16 contiguous, read in place; the arithmetic is fp32.  Per sample n and level interval k < K - 1
 *     Z_k = zs_k x[z_ch[k]] + zb_k,   T_k = ts_k x[t_ch[k]] + tb_k,   NQ = K: T_k *= f_k = 1 + eps (qs_k x[q_ch[k]] + qb_k)
 *     r_k = (Z_{k+1} - Z_k) + hl_k (T_k + T_{k+1})
 *         = hl_k (d_k + d_{k+1}) + (zs_{k+1} x[z_ch[k+1]] - zs_k x[z_ch[k]] + c_k),   d_k = T_k f_k - tb_k,
 *           c_k = zb_{k+1} - zb_k + hl_k (tb_k + tb_{k+1})
 *     out[n][k] = sum_p quad[p] w[n][k][p] r_k(p)^2
 * with wgt f32 or NULL (= 1), addressed as wgt + n w_sn + k w_sk + p (a stride of 0 broadcasts), quad (HW) f32.  2 <= K <=
 * MK_CMIX_LEVELS; NQ = 0 (dry) or K.  The two DEVICE tables:
 *     itab (MK_HYDRO_ITAB + NR int32): z_ch, t_ch, q_ch (MK_CMIX_LEVELS each; entries beyond K, and all of q_ch when NQ = 0, must
 *         repeat a VALID channel: they are read, the value is dropped), then the NR = C - 2 K - NQ channels the loss does not read
 *     ftab (MK_HYDRO_FTAB f32, MK_CMIX_LEVELS each): zs = scale_z / R_d, c (above, folded on the host in fp64: the biases, of the
 *         size of Z / R_d and T, meet there and not in fp32; the kernel adds deviations to the imbalance of the mean state), ts, tb,
 *         qs, qb, hl_k = 1/2 ln(p_{k+1} / p_k); zero beyond their count (c, hl: beyond K - 1).
 * The channel indices are NOT checked (device memory): the caller guarantees that they are < C and pairwise distinct.
 *   mk_hydro_chunks: the number of partial sums per (n, k).
 *   mk_hydro_sums:   one launch over x writes ws (N (K - 1) mk_hydro_chunks(HW) f32), a second, tiny one adds the chunks in index
 *                    order into out (N, K - 1) f32.  No atomics: repeats are bit-identical.  Nothing is read on the host.
 *   mk_hydro_grad:   gx (N, C, HW) in the dtype of x from g (N, K - 1) f32 DEVICE memory: the z, t (and q) channels, ZERO on the NR
 *                    others; every element of gx is written once, no memset beforehand.
 * Four consecutive pixels per thread (one 16-byte f32 / 8-byte bf16 access per channel) when HW, w_sn and w_sk are multiples of 4
 * and every tensor pointer is 16-byte aligned; one pixel per thread otherwise.
 *
 * The preparation pass, prd (B, E, n) members, tar (B, n), the input state at inp + b inp_stride (n elements each), all of ONE
 * dtype f32 | bf16, n = C HW points per sample, 1 <= E <= 32 (forward):
 *     MK_PREP_MEAN      mean (B, n)      = inv sum_e prd_e      (sequential fp32 sum over e, rounded once)
 *     MK_PREP_MEMBER_T  prd_t (B, E, n)  = prd_e - inp
 *     MK_PREP_MEAN_T    mean_t (B, n)    = inv sum_e prd_e - inp (from the unrounded mean)
 *     MK_PREP_TAR_T     tar_t (B, n)     = tar - inp
 * Only the outputs selected in `flags` are written (and only the inputs they need are read).
 *   mk_loss_prep_bwd: g_prd (B, E, n) = g_prd_t + inv (g_mean + g_mean_t); each of the three may be NULL (absent terms are skipped). */
#define MK_HYDRO_ITAB (3 * MK_CMIX_LEVELS)
#define MK_HYDRO_FTAB (7 * MK_CMIX_LEVELS)
#define MK_PREP_MEAN 1
#define MK_PREP_MEMBER_T 2
#define MK_PREP_MEAN_T 4
#define MK_PREP_TAR_T 8
int mk_hydro_chunks(long long HW);
int mk_hydro_sums(const void* x, int dtype, const float* wgt, long long w_sn, long long w_sk, const float* quad, float* out, float* ws,
                  const int* itab, const float* ftab, int N, int C, int K, int NQ, int NR, float eps, long long HW, void* stream);
int mk_hydro_grad(const void* x, int dtype, const float* wgt, long long w_sn, long long w_sk, const float* quad, const float* g, void* gx,
                  const int* itab, const float* ftab, int N, int C, int K, int NQ, int NR, float eps, long long HW, void* stream);
int mk_loss_prep_fwd(const void* prd, const void* tar, const void* inp, long long inp_stride, int dtype, void* mean, void* prd_t, void* mean_t,
                     void* tar_t, int flags, float inv, int B, int E, long long n, void* stream);
int mk_loss_prep_bwd(const void* g_prd_t, const void* g_mean, const void* g_mean_t, void* g_prd, int dtype, float inv, int B, int E,
                     long long n, void* stream);

/* ---- imputation of missing inputs and the output tail of FourCastNet3.1 (csrc/impute.hip; makani/models/common/imputation.py,
 *      makani/models/networks/fourcastnet3_1.py:1062-1080,1127-1131) -------------------------------------------------------------
 * Pointwise in space: one thread per pixel, or per four consecutive pixels when HW (and the mask strides) are multiples of 4 and
 * every tensor pointer is 16-byte aligned.  x, y, g, gx, d, xin are f32 | bf16 of ONE dtype, contiguous (B, C, HW); the arithmetic is
 * fp32, rounded once.  Nothing is read on the host and there are no atomics: the launches can be captured in a graph and repeats
 * are bit-identical.
 *
 * MLPImputation, x (B, C, HW) -> y (B, C, HW), NI <= MK_IMPUTE_SLOTS imputed channels imp_ch, C <= MK_IMPUTE_CHANNELS, hidden <=
 * MK_IMPUTE_HIDDEN (beyond: MK_EUNSUP):
 *     m_j = isnan(x[imp_ch[j]]) | (mask operand != 0);   xc = x with 0 at the masked entries of the imputed channels
 *     h_k = b1_k + sum_c W1[k][c] xc_c;   a_k = act(h_k);   o_j = sum_k W2[j][k] a_k;   y[imp_ch[j]] = m_j ? o_j : x[imp_ch[j]]
 * and every other entry of y is a copy of x.  act: MK_IMPUTE_ACT_GELU (exact erf), _RELU, _SILU, _SIN.  The mask operand by
 * mask_kind: MK_IMPUTE_MASK_NONE; _BOOL (one byte per element), _F32, _BF16: `mask` with Nm = 1 | NI planes of HW elements per
 * sample, sample b at element b m_sb (0: one mask for all samples); _CHANNEL: channel mask_ch of x itself (`mask` is ignored).
 * The DEVICE table tab (MK_IMPUTE_TAB 32-bit words): W1 TRANSPOSED (MK_IMPUTE_CHANNELS, MK_IMPUTE_HIDDEN) f32, b1 (MK_IMPUTE_HIDDEN),
 * W2 (MK_IMPUTE_SLOTS, MK_IMPUTE_HIDDEN), all zero beyond C, hidden, NI; then int32: imp_ch (MK_IMPUTE_SLOTS; beyond NI a VALID
 * channel: it is read, the value is dropped), slot (MK_IMPUTE_CHANNELS: j for imp_ch[j], -1 otherwise).  The channel indices are
 * NOT checked (device memory): the caller guarantees that they are < C and pairwise distinct.
 *   mk_impute_mlp_bwd: from g (B, C, HW), the saved x and the mask operand (h is recomputed):  gx_c = g_c + sum_k W1[k][c] gh_k, exactly
 *       0 at the masked entries of the imputed channels;  gW1 (hidden, C), gb1 (hidden), gW2 (NI, hidden) f32, the sums over samples
 *       and pixels: one partial sum per block in ws (mk_impute_mlp_workspace floats), added in block order by a second, tiny launch.
 *
 * ConstantImputation, w (C) f32: y = (mask | isnan(x)) ? w_c : x, the mask (kinds NONE, BOOL, F32, BF16) addressed as
 * mask + b m_sb + c m_sc + p (a stride of 0 broadcasts).  mk_impute_const_bwd: gx = masked ? 0 : g, gw (C) f32 = the sum of g over the
 * masked entries: partial sums in ws (B C mk_impute_chunks(HW) floats), added in index order.
 *
 * The output tail, d (B, Co, HW) the decoder's output, xin (B, Cin, HW) the network's input:
 *     y_c = clamp_c(d_c + [pred_ch != NULL] xin[pred_ch[c]]),   clamp_c(v) = water[c] ? soft_clamp(v + off_c) - off_c : v,
 *     soft_clamp(t) = 0 (t <= 0), t^2 (t < 1/2), t - 1/4 (otherwise)
 * pred_ch (Co) int32 DEVICE or NULL (no skip), water (Co) int32 DEVICE flags, off (Co) f32 DEVICE or NULL (= 0).
 *   mk_fcn31_tail_bwd: gd (B, Co, HW) = g clamp'(.), recomputed from d (and xin); with the skip also gxin (B, Cin, HW): gd on the
 *       channels pred_ch (pairwise distinct), ZERO on the Cin - Co others, listed in rest (int32 DEVICE): every element is written once. */
#define MK_IMPUTE_CHANNELS 256
#define MK_IMPUTE_SLOTS 8
#define MK_IMPUTE_HIDDEN 32
#define MK_IMPUTE_TAB (MK_IMPUTE_CHANNELS * MK_IMPUTE_HIDDEN + MK_IMPUTE_HIDDEN + MK_IMPUTE_SLOTS * MK_IMPUTE_HIDDEN + MK_IMPUTE_SLOTS + MK_IMPUTE_CHANNELS)
#define MK_IMPUTE_MASK_NONE 0
#define MK_IMPUTE_MASK_BOOL 1
#define MK_IMPUTE_MASK_F32 2
#define MK_IMPUTE_MASK_BF16 3
#define MK_IMPUTE_MASK_CHANNEL 4
#define MK_IMPUTE_ACT_GELU 0
#define MK_IMPUTE_ACT_RELU 1
#define MK_IMPUTE_ACT_SILU 2
#define MK_IMPUTE_ACT_SIN 3
int mk_impute_mlp_fwd(const void* x, void* y, int dtype, const float* tab, const void* mask, int mask_kind, int Nm, long long m_sb,
                      int mask_ch, int act, int B, int C, int NI, int hidden, long long HW, void* stream);
long long mk_impute_mlp_workspace(int B, int C, int NI, int hidden, long long HW);
int mk_impute_mlp_bwd(const void* g, const void* x, void* gx, float* gW1, float* gb1, float* gW2, float* ws, int dtype, const float* tab,
                      const void* mask, int mask_kind, int Nm, long long m_sb, int mask_ch, int act, int B, int C, int NI, int hidden,
                      long long HW, void* stream);
int mk_impute_chunks(long long HW);
int mk_impute_const_fwd(const void* x, void* y, int dtype, const float* w, const void* mask, int mask_kind, long long m_sb, long long m_sc,
                        int B, int C, long long HW, void* stream);
int mk_impute_const_bwd(const void* g, const void* x, void* gx, float* gw, float* ws, int dtype, const void* mask, int mask_kind,
                        long long m_sb, long long m_sc, int B, int C, long long HW, void* stream);
int mk_fcn31_tail_fwd(const void* d, const void* xin, void* y, int dtype, const int* pred_ch, const int* water, const float* off, int B,
                      int Co, int Cin, long long HW, void* stream);
int mk_fcn31_tail_bwd(const void* g, const void* d, const void* xin, void* gd, void* gxin, int dtype, const int* pred_ch, const int* water,
                      const float* off, const int* rest, int B, int Co, int Cin, long long HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAKANI_AMD_H */
