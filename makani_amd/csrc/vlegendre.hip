// Vector Legendre stage of RealVectorSHT / InverseRealVectorSHT (torch-harmonics [un-vendored]; used by the reference at
// makani/utils/losses/base_loss.py:461-469,547-554): ONE launch per direction that reads every F (S) element once and
// writes every S (F) element once.
//
// Column blocks.  A vector field of P (u, v) pairs travels as a scalar F / S tensor whose row index is
// (component, pair): F (M, nlat, 2, 2 Rp), S (L, M, 2, 2 Rp), Rp = P rounded up to 32.  Seen from one order m the
// operand is a [k][column] matrix with FOUR column blocks of Rp columns,
//     Q0 = (re, comp 0)   Q1 = (re, comp 1)   Q2 = (im, comp 0)   Q3 = (im, comp 1)
// (comp 0 / 1 = theta / phi component on the grid side, spheroidal / toroidal coefficient on the spectral side).
// With A0 = d P / d theta, A1 = m P / sin theta (both over sqrt(l (l + 1)); times the quadrature weights in the
// analysis-shaped launches) every output block is
//     out[Qo] = A0 . in[Qo]  +  sg(o) A1 . in[Q(3 - o)]                  sg = (+, -, -, +)
//     analysis  (s = A0 U - i A1 V,  t = i A1 U + A0 V)   and   synthesis (U = A0 s - i A1 t,  V = i A1 s + A0 t)
// alike (the field is sum s Psi + t Phi, Psi = (A0, i A1), Phi = r x Psi = (-i A1, A0): legendre.py), and since
// sg(3 - o) = sg(o) the transposed map of one direction is the other direction with the transposed matrices (the
// backward launches).
// A workgroup owns 128 rows x 64 columns of ALL FOUR blocks: the data tile is staged (and split into limbs) once, a
// wave multiplies "its" block by A0 and the partner block — a second fragment read of the same LDS image — by A1 into
// the same accumulator.  sg is applied by flipping the sign bits of the partner's limb fragments (the limbs of -x are
// the negated limbs of x).
//
// Same arithmetic classes as the scalar engine (csrc/xgemm2.hip, xgemm2_kernel): constant matrices pre-split into bf16
// limb planes, data split on the fly, 6 (3) bf16 MFMAs per product, fp32 accumulation; same ping-pong schedule (two
// groups of four waves alternate between the matrix pipe and split / stage), triangle and polar band skipping.
//   mode 0  analysis          in (u, v)  -> out (s, t)
//   mode 1  synthesis         in (s, t)  -> out (u, v)
//   mode 2  analysis, s only  in (u, v)  -> out s            out has TWO column blocks (re, im)
//   mode 3  synthesis, t = 0  in s       -> out (u, v)       in  has TWO column blocks: the zero toroidal half is
//                                                            neither stored nor multiplied (gradient of a scalar)
//
// The m-shard form (an azimuth rank of the h x w distributed pair, makani_amd/distributed.py): the launch covers `orders`
// consecutive orders starting at tri_off.  Batch b is the GLOBAL order b + tri_off for the triangle (rows l < m skipped in 32-row
// steps / k >= m) and the LOCAL order for everything that is addressed: limb planes (b * pl_batch), operands (b * b_batch,
// b * c_batch) and band_lo[b] / band_hi[b] — the caller hands over the slices [tri_off, tri_off + orders) of all of them.
// Orders are independent batches (no reduction crosses them, the XCD placement b % 8 is speed only), so a shard launch
// performs the same products in the same order as the full launch does for those orders: bit-equal results, and the same
// rows left unwritten (analysis never stores rows l < m; a synthesis band writes its zeros per order).
#include "xsplit.h"

namespace {

using namespace xsplit;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const f32x4 g_f32x4;
typedef __attribute__((address_space(1))) const u32x4 g_u32x4;

// out-of-range lanes load zeros from here: every global load is unconditional (see xgemm2.hip, g_zero32)
__device__ const f32x4 g_vzero32[2] = {};

constexpr int NTV = 512;
constexpr int VBM = 128;             // rows per workgroup
constexpr int VPC = 64;              // columns of every block per workgroup
constexpr int VBN = 4 * VPC;         // columns of the LDS data image

struct VLeg {
    const u16* pl[2];                // limb planes of A0, A1: [plane][batch][k][row], row contiguous
    long long pl_stride, pl_batch, pl_k;
    const float* B;                  // [batch][k][block][Rp] through b_batch / b_k
    float* C;                        // [batch][row][block][Rp] through c_batch / c_row
    long long b_batch, b_k, c_batch, c_row;
    int M, K, batch, Rp;
    int tri_mode, tri_off;
    const int* band_lo;
    const int* band_hi;
    int band_mode;
};

__device__ __forceinline__ bf16x8 xor_frag(bf16x8 v, unsigned m) {
    u32x4 u = __builtin_bit_cast(u32x4, v);
    u ^= m;
    return __builtin_bit_cast(bf16x8, u);
}

// acc0 / acc1 += a . b0 / a . b1 (two column tiles sharing the A fragment), smallest limb products first
template <int NP>
__device__ __forceinline__ void vmma2(const bf16x8* a, const bf16x8* b0, const bf16x8* b1, f32x16& c0, f32x16& c1) {
    constexpr int NPROD = NP == 3 ? 6 : 3;
    constexpr int IA[6] = {1, 0, 2, 0, 1, 0}, IB[6] = {1, 2, 0, 1, 0, 0};
    constexpr int O = NP == 3 ? 0 : 3;
#pragma unroll
    for (int q = 0; q < NPROD; ++q) {
        c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[IA[O + q]], b0[IB[O + q]], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[IA[O + q]], b1[IB[O + q]], c1, 0, 0, 0);
    }
}

template <int NP, int MODE>
__global__ __launch_bounds__(NTV) void vlegendre_kernel(const VLeg p, int tilesM, int tilesN) {
    constexpr int NIB = MODE == 3 ? 2 : 4;                 // column blocks of the input
    constexpr int NOB = MODE == 2 ? 2 : 4;                 // column blocks of the output
    constexpr bool TWO = MODE != 3;                        // two products per accumulator
    constexpr int PRA = VBM + 32, PRB = VBN + 32;          // pitches of the [k][row] limb tiles
    constexpr int PLA = BK * PRA, PLB = BK * PRB;          // elements per limb plane
    constexpr int STG = 2 * NP * PLA + NP * PLB;           // (A0, A1) x limbs + data x limbs
    static_assert(2 * STG * 2 <= 160 * 1024, "two stages must fit the LDS of a CU");
    __shared__ __attribute__((aligned(16))) u16 smem[2 * STG];

    // ---- which piece of the problem (same block order as the scalar engine: order m = b lives on XCD b % 8) ----
    const int xcd = blockIdx.x % MK_NUM_XCD, jb = blockIdx.x / MK_NUM_XCD;
    const int tpb = tilesM * tilesN;
    const int b = (jb / tpb) * MK_NUM_XCD + xcd;
    if (b >= p.batch) return;
    const int i0 = ((jb % tpb) / tilesN) * VBM;
    const int pc0 = ((jb % tpb) % tilesN) * VPC;
    const int tt = b + p.tri_off;
    int klo = 0, khi = p.K;
    if (p.tri_mode == MK_TRI_ROW_GE && i0 + VBM <= tt) return;
    if (p.tri_mode == MK_TRI_K_GE) klo = max(0, min(tt, p.K));

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = wave >> 2, cs = wave & 3;
    const int l31 = lane & 31, lh = lane >> 5;

    // rows that are stored: 32-row tiles [s0, s1); rows that are computed: tiles [t0, t1) inside them
    const int rows_end = p.M - i0;
    int s0 = 0;
    if (p.tri_mode == MK_TRI_ROW_GE) s0 = max(0, (tt - i0) / 32);
    const int s1 = min(VBM / 32, (rows_end + 31) / 32);
    int t0 = s0, t1 = s1;
    if (p.band_mode == 1) {
        klo = max(klo, p.band_lo[b]);
        khi = min(khi, p.band_hi[b]);
        if (khi < klo) khi = klo;
    } else if (p.band_mode == 2) {
        t0 = max(s0, (p.band_lo[b] - i0) >> 5);
        t1 = min(s1, (p.band_hi[b] - i0 + 31) >> 5);
        if (t1 < t0) t1 = t0;
    }
    int tile[2];
    bool live[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        tile[j] = t0 + grp + 2 * j;
        live[j] = tile[j] < t1;
    }

    // ---- the two terms of this wave's output block o = cs ----
    int m0 = 0, b0 = cs, b1 = 3 - cs;                      // (the second term always takes A1)
    unsigned negm = (cs == 1 || cs == 2) ? 0x80008000u : 0u;
    float sgn = 1.f;
    bool wact = true;
    if constexpr (MODE == 2) {                             // s_re = A0 U_re + A1 V_im;  s_im = A0 U_im - A1 V_re
        wact = cs < 2;
        b0 = cs == 0 ? 0 : 2;
        b1 = cs == 0 ? 3 : 1;
        negm = cs == 1 ? 0x80008000u : 0u;
    } else if constexpr (MODE == 3) {                      // U_re = A0 s_re, V_re = -A1 s_im, U_im = A0 s_im, V_im = A1 s_re
        m0 = cs & 1;
        b0 = (cs == 1 || cs == 2) ? 1 : 0;
        sgn = cs == 1 ? -1.f : 1.f;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][n][r] = 0.f;

    const int kt0 = klo / BK, kt1 = (khi + BK - 1) / BK;
    const int nk = kt1 - kt0;

    // ---- staging: data (fp32, split on the way to LDS) ----
    constexpr int NVEC = BK * NIB * (VPC / 4);             // float4 vectors of one k-step
    constexpr int NV = NVEC / NTV;
    static_assert(NVEC % NTV == 0 && NV >= 1, "data tile must deal evenly over the threads");
    const float* Bb = p.B + (long long)b * p.b_batch;
    f32x4 bv[NV];
    const float* bp[NV];
    int boff[NV], bkk[NV];
    unsigned bok = 0u;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const int f = tid + q * NTV;
        const int kk = f / (NIB * (VPC / 4)), w = f % (NIB * (VPC / 4));
        const int blk = w / (VPC / 4), c4 = w % (VPC / 4);
        const int col = pc0 + c4 * 4;
        bkk[q] = kk;
        bp[q] = Bb + (long long)kk * p.b_k + (long long)blk * p.Rp + col;
        boff[q] = kk * PRB + blk * VPC + c4 * 4;
        bok |= (col < p.Rp ? 1u : 0u) << q;
    }
    // ---- staging: the two constant matrices (limb planes, copied as 16-byte vectors) ----
    const int am = tid >> 8, ak = (tid >> 4) & 15, ar0 = (tid & 15) * 8;
    const int rows_valid = (int)min((long long)0x7ffffff8, p.pl_k & ~7ll);
    const bool a_ok = i0 + ar0 < rows_valid && ar0 < 32 * t1 && ar0 + 8 > 32 * t0;
    const u16* ap = (am ? p.pl[1] : p.pl[0]) + (long long)b * p.pl_batch + (long long)ak * p.pl_k + i0 + ar0;
    u32x4 av[NP];

    auto ld = [&](int kt) __attribute__((always_inline)) {
        const int k0 = kt * BK;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const bool valid = ((bok >> q) & 1u) && in_range(k0 + bkk[q], klo, khi);
            const g_f32x4* src = valid ? (const g_f32x4*)(bp[q] + (long long)k0 * p.b_k) : (const g_f32x4*)g_vzero32;
            bv[q] = src[0];
        }
        const bool ok = a_ok && k0 + ak < p.K;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const g_u32x4* src = ok ? (const g_u32x4*)(ap + (long long)k0 * p.pl_k + q * p.pl_stride) : (const g_u32x4*)g_vzero32;
            av[q] = src[0];
        }
    };
    auto st = [&](int buf) __attribute__((always_inline)) {
        u16* As = smem + buf * STG;
        u16* Bs = As + 2 * NP * PLA;
#pragma unroll
        for (int q = 0; q < NV; ++q) split_store4<NP, PLB>(Bs, boff[q], bv[q].xy, bv[q].zw);
#pragma unroll
        for (int q = 0; q < NP; ++q) *reinterpret_cast<u32x4*>(As + (am * NP + q) * PLA + ak * PRA + ar0) = av[q];
    };
    auto compute = [&](int buf) __attribute__((always_inline)) {
        const u16* As = smem + buf * STG;
        const u16* Bs = As + 2 * NP * PLA;
        if (!live[0] || !wact) return;
        bf16x8 bf0[2][NP], bf1[TWO ? 2 : 1][NP];
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) {
                bf0[n][pl] = frag<VBN, false>(Bs + pl * PLB, b0 * VPC + n * 32, lane);
                if constexpr (TWO) bf1[n][pl] = xor_frag(frag<VBN, false>(Bs + pl * PLB, b1 * VPC + n * 32, lane), negm);
            }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!live[j]) continue;
            bf16x8 af[NP];
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) af[pl] = frag<VBM, false>(As + (m0 * NP + pl) * PLA, tile[j] * 32, lane);
            __builtin_amdgcn_s_setprio(1);
            vmma2<NP>(af, bf0[0], bf0[1], acc[j][0], acc[j][1]);
            __builtin_amdgcn_s_setprio(0);
            if constexpr (TWO) {
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) af[pl] = frag<VBM, false>(As + (NP + pl) * PLA, tile[j] * 32, lane);
                __builtin_amdgcn_s_setprio(1);
                vmma2<NP>(af, bf1[0], bf1[1], acc[j][0], acc[j][1]);
                __builtin_amdgcn_s_setprio(0);
            }
        }
    };
    auto produce = [&](int i) __attribute__((always_inline)) {          // tile kt0 + i + 1 rides in the staging registers
        if (i + 1 < nk) st((i + 1) & 1);
        if (i + 2 < nk) ld(kt0 + i + 2);
    };

    if (nk > 0) {
        ld(kt0);
        st(0);
        if (nk > 1) ld(kt0 + 1);
    }
    __syncthreads();
    for (int i = 0; i < nk; ++i) {
        // one barrier per k-step; the groups run the two segments in opposite order, so that on every SIMD one wave
        // starts on the matrix pipe while its partner starts on the VALU / memory path
        if (grp == 0) {
            produce(i);
            compute(i & 1);
        } else {
            compute(i & 1);
            produce(i);
        }
        __syncthreads();
    }

    if (!wact) return;
    float* Cb = p.C + (long long)b * p.c_batch + (long long)cs * p.Rp;
    static_assert(NOB == (MODE == 2 ? 2 : 4), "waves past the output blocks have left above");
    if (p.band_mode == 2) {                                // stored rows outside the band: exact zeros
        for (int t = s0 + grp; t < s1; t += 2) {
            if (t >= t0 && t < t1) continue;
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int col = pc0 + n * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = i0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (row < p.M && col < p.Rp) Cb[(long long)row * p.c_row + col] = 0.f;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (!live[j]) continue;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int col = pc0 + n * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + tile[j] * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (row < p.M && col < p.Rp) Cb[(long long)row * p.c_row + col] = sgn * acc[j][n][r];
            }
        }
    }
}

template <int NP>
void launch_vleg(const VLeg& v, int mode, dim3 grid, int tm, int tn, hipStream_t s) {
    switch (mode) {
        case 0: hipLaunchKernelGGL((vlegendre_kernel<NP, 0>), grid, dim3(NTV), 0, s, v, tm, tn); break;
        case 1: hipLaunchKernelGGL((vlegendre_kernel<NP, 1>), grid, dim3(NTV), 0, s, v, tm, tn); break;
        case 2: hipLaunchKernelGGL((vlegendre_kernel<NP, 2>), grid, dim3(NTV), 0, s, v, tm, tn); break;
        default: hipLaunchKernelGGL((vlegendre_kernel<NP, 3>), grid, dim3(NTV), 0, s, v, tm, tn); break;
    }
}

}  // namespace

extern "C" int mk_vlegendre(const void* planes0, const void* planes1, long long pl_stride, long long pl_batch, long long pl_k,
                            int limbs, const float* in, float* out, int mode, int rows, int K, int orders, int Rp,
                            int tri_off, const int* band_lo, const int* band_hi, void* stream) {
    MK_REQUIRE(planes0 && planes1 && in && out, "vlegendre: null pointer");
    MK_REQUIRE(mode >= 0 && mode <= 3, "vlegendre: mode must be 0 (analysis), 1 (synthesis), 2 (analysis, s only), 3 (synthesis, t = 0)");
    MK_REQUIRE(limbs == 2 || limbs == 3, "vlegendre: limbs must be 2 or 3");
    MK_REQUIRE(rows > 0 && K > 0 && orders > 0 && Rp > 0 && (Rp & 31) == 0, "vlegendre: bad extents (Rp must be a multiple of 32)");
    MK_REQUIRE((pl_k & 7) == 0 && (pl_batch & 7) == 0 && (pl_stride & 7) == 0 && ((uintptr_t)planes0 & 15) == 0 &&
                   ((uintptr_t)planes1 & 15) == 0 && pl_k >= rows,
               "vlegendre: limb planes need 16-byte aligned k-rows of at least `rows` elements");
    MK_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0, "vlegendre: in / out must be 16-byte aligned");
    MK_REQUIRE((band_lo == nullptr) == (band_hi == nullptr), "vlegendre: both band arrays or none");
    const bool ana = mode == 0 || mode == 2;
    const int nib = mode == 3 ? 2 : 4, nob = mode == 2 ? 2 : 4;
    VLeg v;
    v.pl[0] = (const u16*)planes0;
    v.pl[1] = (const u16*)planes1;
    v.pl_stride = pl_stride, v.pl_batch = pl_batch, v.pl_k = pl_k;
    v.B = in, v.C = out;
    if (ana) {          // in = F (orders, K = nlat, nib Rp), out = S (rows = L, orders, nob Rp)
        v.b_batch = (long long)K * nib * Rp, v.b_k = (long long)nib * Rp;
        v.c_batch = (long long)nob * Rp, v.c_row = (long long)orders * nob * Rp;
        v.tri_mode = MK_TRI_ROW_GE;
    } else {            // in = S (K = L, orders, nib Rp), out = F (orders, rows = nlat, nob Rp)
        v.b_batch = (long long)nib * Rp, v.b_k = (long long)orders * nib * Rp;
        v.c_batch = (long long)rows * nob * Rp, v.c_row = (long long)nob * Rp;
        v.tri_mode = MK_TRI_K_GE;
    }
    v.M = rows, v.K = K, v.batch = orders, v.Rp = Rp, v.tri_off = tri_off;
    v.band_lo = band_lo, v.band_hi = band_hi;
    v.band_mode = band_lo ? (ana ? 1 : 2) : 0;
    const int tm = (rows + VBM - 1) / VBM, tn = (Rp + VPC - 1) / VPC;
    const long long nb = (long long)((orders + MK_NUM_XCD - 1) / MK_NUM_XCD) * MK_NUM_XCD * tm * tn;
    MK_REQUIRE(nb < (1ll << 31), "vlegendre: grid too large");
    dim3 grid((unsigned)nb);
    hipStream_t s = (hipStream_t)stream;
    if (limbs == 3)
        launch_vleg<3>(v, mode, grid, tm, tn, s);
    else
        launch_vleg<2>(v, mode, grid, tm, tn, s);
    return mk_check_launch("mk_vlegendre");
}
