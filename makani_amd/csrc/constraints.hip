// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (see escore.hip: the SLP vectoriser's packed-fp32 forms are kept out of this library; tests/test_packed_forms.py scans the ISA)
// Physical output constraints between the network and the loss (makani/models/parametrizations.py:193-231,
// makani/utils/constraints.py:91-113,288-320), forward and backward (gfx950).
//
// Every pixel is independent.  A thread owns P consecutive pixels of a plane (P = 4: one 16-byte f32 / 8-byte bf16 access per
// channel, when HW is a multiple of 4 and every tensor pointer is 16-byte aligned; P = 1 otherwise) and walks the channels; the
// arithmetic is fp32 whatever the element type, the result is rounded once.  Channels a layer does not touch are copied in
// the same launch: the prediction is read once and written once.
//
//   mk_cmix_fwd / mk_cmix_bwd    the column mix behind _HydrostaticBalanceWrapper and HydrostaticBalanceProjection
//       u_k  = s_k x[in_ch[k]] + b_k                         k < K_in gathered rows (physical units)
//       f_j  = 1 + eps (qs_j x[q_ch[j]] + qb_j)              j < NQ humidity rows (NQ = 0: the dry forms)
//       u_k *= f_k                                           k < n_mi            (T -> Tv)
//       v_r  = [resid] u_r + beta (sum_k M[r][k] u_k - off_r) r < K_out
//       v_r /= f_r                                           r < n_mo            (Tv -> T)
//       y[out_ch[r]] = (v_r - b'_r) / s'_r
//       y[q_out[j]]  = q_rt ? (q_phys_j - qb_j) / qs_j : x[q_ch[j]];   y[copy_dst[c]] = x[copy_src[c]]
//     The wrapper is resid = 0, beta = 1, off = 0, M = the non-trivial (2L, L + 1) block of the reference's `mapping` (rows T_0 ..
//     T_{L-1}, Z_0 .. Z_{L-1}); the projection is resid = 1, beta = -strength, M = `proj` (2L, 2L).
//     The dry forward (NQ = 0) is affine in x and is evaluated as such: y_r = sum_k W[r][k] x_k + c_r, W = diag(1 / s') ([resid] I +
//     beta M) diag(s), c = ([resid] b + beta (M b - off) - b') / s', folded on the host in fp64 from the same fp32 vectors and
//     held as two fp32 limbs each; the sum is compensated (dot2 below), so the result is the fp64 value rounded once.  The
//     formula above, taken step by step in fp32, carries an ABSOLUTE error of a few ulp of the physical magnitudes (7e4 for a
//     geopotential), which in a normalised output next to zero is many bf16 steps.  The moist forward and both backward passes
//     run the steps as written.
//     Backward is the transpose: gv_r = g_r / s'_r (/ f_r), gu_k = [resid] gv_k + beta sum_r M[r][k] gv_r, gx_k = s_k gu_k (f_k);
//     the moist forms recompute u, f and v from the saved input and add  d f_j = gu_j u_j - gv_j v_j / f_j  into the q rows.
//   The column (u, f, gv) lives in registers: every loop over it is unrolled over the compile-time capacity 2 CAP rows / CAP
//   levels (CAP = 4, 8, 16); rows beyond the count re-read the table's padding channel (a valid one: a cache hit) and are
//   zeroed by a select.  The loops over OUTPUT rows are run-time loops; the one column entry such a row needs by its own index
//   is taken with a chain of selects over compile-time indices, never by indexing the register array.  M, its transpose and
//   the affine vectors are the same for every lane: they sit in one device table and every read of it has a wave-uniform
//   address (scalar loads, no per-lane traffic).
//
//   mk_nonneg_fwd / mk_nonneg_bwd    NonNegativeConstraint on the channels with slot[c] >= 0, w = x + offset[slot[c]]
//       mode 0 "silu"      w sigmoid(w / eps) - offset
//       mode 1 "softplus"  leak w + (1 - leak) eps (softplus(w / eps) - ln 2) - offset,  softplus(t) = max(t, 0) + log1p(exp(-|t|))
//       mode 2 evaluation  max(x, -offset)
//     and the derivative of whichever ran.  sigmoid and softplus go through exp(-|t|): nothing overflows, and the tail of
//     softplus at very negative t is log1p(exp(t)) ~ exp(t), not 0.
#include "block_io.h"

namespace {

constexpr int CNT = 256;
constexpr int ROWS = MK_CMIX_ROWS, LEV = MK_CMIX_LEVELS;
// the int table: in_ch, out_ch (ROWS each), q_ch, q_out (LEV each), then copy_src (NC), copy_dst (NC)
constexpr int IT_IN = 0, IT_OUT = ROWS, IT_Q = 2 * ROWS, IT_QOUT = 2 * ROWS + LEV, IT_COPY = 2 * ROWS + 2 * LEV;
// the float table: s, b, s', b', off (ROWS each), qs, qb (LEV each), M (ROWS, ROWS), its transpose (ROWS, ROWS), then the
// folded map of the dry forward: W high and low limbs (ROWS, ROWS each), c high and low limbs (ROWS each)
constexpr int FT_INS = 0, FT_INB = ROWS, FT_OUTS = 2 * ROWS, FT_OUTB = 3 * ROWS, FT_OFF = 4 * ROWS, FT_QS = 5 * ROWS, FT_QB = 5 * ROWS + LEV,
              FT_M = 5 * ROWS + 2 * LEV, FT_MT = FT_M + ROWS * ROWS, FT_WH = FT_MT + ROWS * ROWS, FT_WL = FT_WH + ROWS * ROWS,
              FT_CH = FT_WL + ROWS * ROWS, FT_CL = FT_CH + ROWS;
static_assert(IT_COPY == MK_CMIX_ITAB && FT_CL + ROWS == MK_CMIX_FTAB, "table sizes of include/makani_amd.h");

struct Cmix {
    const int* it;
    const float* ft;
    int Cin, Cout, K_in, K_out, NQ, n_mi, n_mo, NC, resid, q_rt;
    float beta, eps;
};

// entry `r` (wave-uniform, run-time) of the first N rows of a register-resident column: selects over compile-time indices
template <int N, int NA, int P>
__device__ __forceinline__ void pick(const float (&a)[NA][P], int r, float (&o)[P]) {
    static_assert(N <= NA, "rows");
#pragma unroll
    for (int e = 0; e < P; ++e) o[e] = 0.f;
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int e = 0; e < P; ++e) o[e] = (k == r) ? a[k][e] : o[e];
    }
}

// sum_k m[k] a[k] over the whole capacity (m is zero-padded, a is zero beyond its count)
template <int N, int P>
__device__ __forceinline__ void dot(const float* __restrict__ m, const float (&a)[N][P], float (&o)[P]) {
#pragma unroll
    for (int e = 0; e < P; ++e) o[e] = 0.f;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float mk = m[k];
#pragma unroll
        for (int e = 0; e < P; ++e) o[e] = fmaf(mk, a[k][e], o[e]);
    }
}

// (s, c) += sum_k (wh[k] + wl[k]) a[k] with the value carried as the unevaluated sum s + c: the product wh a is split exactly by
// one FMA, the running sum by Knuth's two-sum, and the error terms gather in c (Ogita, Rump and Oishi's Dot2).  The result is
// that of a sum in twice the working precision, rounded once by the caller's s + c.  No contraction in here: it would fuse
// the very roundings the error terms are taken from.
template <int N, int P>
__device__ __forceinline__ void dot2(const float* __restrict__ wh, const float* __restrict__ wl, const float (&a)[N][P], float (&s)[P],
                                     float (&c)[P]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float h = wh[k], l = wl[k];
#pragma unroll
        for (int e = 0; e < P; ++e) {
            const float p = h * a[k][e], pe = fmaf(h, a[k][e], -p);
            const float t = s[e] + p, z = t - s[e], se = (s[e] - (t - z)) + (p - z);
            s[e] = t;
            c[e] = fmaf(l, a[k][e], c[e] + (se + pe));
        }
    }
}

// rows [0, n) of `src` gathered through the channel list `ch` (padded with a valid channel up to N), a[k] = 0 beyond n
template <typename T, int P, int N>
__device__ __forceinline__ void gather(const T* __restrict__ src, const int* __restrict__ ch, int n, long long hw, float (&a)[N][P]) {
#pragma unroll
    for (int k = 0; k < N; ++k) mk_ld<T, P>(src + (long long)ch[k] * hw, a[k]);
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int e = 0; e < P; ++e) a[k][e] = k < n ? a[k][e] : 0.f;
    }
}

// dst[to[c]] = src[from[c]], four planes in flight
template <typename T, int P>
__device__ __forceinline__ void copy_planes(const T* __restrict__ src, T* __restrict__ dst, const int* __restrict__ from,
                                            const int* __restrict__ to, int n, long long hw) {
    for (int c = 0; c < n; c += 4) {
        float v[4][P];
#pragma unroll
        for (int e = 0; e < 4; ++e) mk_ld<T, P>(src + (long long)from[c + e < n ? c + e : n - 1] * hw, v[e]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (c + e < n) mk_st<T, P>(dst + (long long)to[c + e] * hw, v[e]);
        }
    }
}

// u (affine, physical units) and, in the moist forms, f; the q rows of the OUTPUT are written when yb is given (forward)
template <typename T, int P, int CAP, bool MOIST>
__device__ __forceinline__ void load_column(const T* __restrict__ xb, T* __restrict__ yb, const Cmix& a, long long hw, float (&u)[2 * CAP][P],
                                            float (&f)[CAP][P]) {
    const int* __restrict__ it = a.it;
    const float* __restrict__ ft = a.ft;
    gather<T, P, 2 * CAP>(xb, it + IT_IN, a.K_in, hw, u);
#pragma unroll
    for (int k = 0; k < 2 * CAP; ++k) {
        const float s = ft[FT_INS + k], b = ft[FT_INB + k];          // (zero beyond K_in)
#pragma unroll
        for (int e = 0; e < P; ++e) u[k][e] = fmaf(s, u[k][e], b);
    }
    if constexpr (MOIST) {
        gather<T, P, CAP>(xb, it + IT_Q, a.NQ, hw, f);
#pragma unroll
        for (int j = 0; j < CAP; ++j) {
            const float qs = ft[FT_QS + j], qb = ft[FT_QB + j];
            float q[P];
#pragma unroll
            for (int e = 0; e < P; ++e) {
                const float raw = f[j][e], qp = fmaf(qs, raw, qb);
                f[j][e] = j < a.NQ ? fmaf(a.eps, qp, 1.f) : 1.f;
                q[e] = a.q_rt ? (qp - qb) / qs : raw;
            }
            if (yb && j < a.NQ) mk_st<T, P>(yb + (long long)it[IT_QOUT + j] * hw, q);
        }
    }
}

// grid (pixel groups, B)
template <typename T, int P, int CAP, bool MOIST>
__global__ __launch_bounds__(CNT) void cmix_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, Cmix a, long long hw) {
    const long long i = ((long long)blockIdx.x * CNT + threadIdx.x) * P;
    if (i >= hw) return;
    const int* __restrict__ it = a.it;
    const float* __restrict__ ft = a.ft;
    const T* xb = x + (long long)blockIdx.y * a.Cin * hw + i;
    T* yb = y + (long long)blockIdx.y * a.Cout * hw + i;
    float u[2 * CAP][P], f[MOIST ? CAP : 1][P];
    if constexpr (!MOIST) {
        // the dry forms are affine in x: y_r = sum_k W[r][k] x_k + c_r with W and c folded on the host in fp64 and held as two
        // fp32 limbs.  x is exact in fp32, so the only rounding left is the last one, and an output next to zero (a projected
        // value whose correction all but cancels it) keeps its leading digits.
        gather<T, P, 2 * CAP>(xb, it + IT_IN, a.K_in, hw, u);
        for (int r = 0; r < a.K_out; ++r) {
            float s[P], c[P];
            const float ch = ft[FT_CH + r], cl = ft[FT_CL + r];
#pragma unroll
            for (int e = 0; e < P; ++e) s[e] = ch, c[e] = cl;
            dot2<2 * CAP, P>(ft + FT_WH + r * ROWS, ft + FT_WL + r * ROWS, u, s, c);
#pragma unroll
            for (int e = 0; e < P; ++e) s[e] += c[e];
            mk_st<T, P>(yb + (long long)it[IT_OUT + r] * hw, s);
        }
        copy_planes<T, P>(xb, yb, it + IT_COPY, it + IT_COPY + a.NC, a.NC, hw);
        return;
    } else {
        load_column<T, P, CAP, true>(xb, yb, a, hw, u, f);
#pragma unroll
        for (int k = 0; k < CAP; ++k) {
#pragma unroll
            for (int e = 0; e < P; ++e) u[k][e] = k < a.n_mi ? u[k][e] * f[k][e] : u[k][e];
        }
    }
    for (int r = 0; r < a.K_out; ++r) {
        float acc[P], own[P], v[P];
        dot<2 * CAP, P>(ft + FT_M + r * ROWS, u, acc);
        if (a.resid) pick<2 * CAP>(u, r, own);
        const float off = ft[FT_OFF + r], ob = ft[FT_OUTB + r], os = ft[FT_OUTS + r];
#pragma unroll
        for (int e = 0; e < P; ++e) v[e] = fmaf(a.beta, acc[e] - off, a.resid ? own[e] : 0.f);
        if constexpr (MOIST) {
            if (r < a.n_mo) {
                float fr[P];
                pick<CAP>(f, r, fr);
#pragma unroll
                for (int e = 0; e < P; ++e) v[e] /= fr[e];
            }
        }
#pragma unroll
        for (int e = 0; e < P; ++e) v[e] = (v[e] - ob) / os;
        mk_st<T, P>(yb + (long long)it[IT_OUT + r] * hw, v);
    }
    copy_planes<T, P>(xb, yb, it + IT_COPY, it + IT_COPY + a.NC, a.NC, hw);
}

// grid (pixel groups, B).  x is read in the moist forms only.
template <typename T, int P, int CAP, bool MOIST>
__global__ __launch_bounds__(CNT) void cmix_bwd_kernel(const T* __restrict__ g, const T* __restrict__ x, T* __restrict__ gx, Cmix a, long long hw) {
    const long long i = ((long long)blockIdx.x * CNT + threadIdx.x) * P;
    if (i >= hw) return;
    const int* __restrict__ it = a.it;
    const float* __restrict__ ft = a.ft;
    const T* gb = g + (long long)blockIdx.y * a.Cout * hw + i;
    T* gxb = gx + (long long)blockIdx.y * a.Cin * hw + i;
    float gv[2 * CAP][P];
    gather<T, P, 2 * CAP>(gb, it + IT_OUT, a.K_out, hw, gv);
#pragma unroll
    for (int r = 0; r < 2 * CAP; ++r) {
        const float os = ft[FT_OUTS + r];          // (one beyond K_out)
#pragma unroll
        for (int e = 0; e < P; ++e) gv[r][e] /= os;
    }
    int k0 = 0;
    if constexpr (MOIST) {
        const T* xb = x + (long long)blockIdx.y * a.Cin * hw + i;
        float u[2 * CAP][P], f[CAP][P];
        load_column<T, P, CAP, true>(xb, nullptr, a, hw, u, f);
#pragma unroll
        for (int r = 0; r < CAP; ++r) {
#pragma unroll
            for (int e = 0; e < P; ++e) gv[r][e] = r < a.n_mo ? gv[r][e] / f[r][e] : gv[r][e];
        }
        // level j: the output row j (divided by f_j), the input row j (multiplied by f_j) and the humidity row j
        for (int j = 0; j < a.NQ; ++j) {
            float gq[P], fj[P], uj[P], gvj[P], gf[P], acc[P], gt[P];
            mk_ld<T, P>(gb + (long long)it[IT_QOUT + j] * hw, gq);
            pick<CAP>(f, j, fj);
            pick<CAP>(u, j, uj);
            pick<CAP>(gv, j, gvj);
#pragma unroll
            for (int e = 0; e < P; ++e) gf[e] = 0.f;
            if (j < a.n_mo) {          // v_j again: the quotient rule needs it
                const float* __restrict__ m = ft + FT_M + j * ROWS;
#pragma unroll
                for (int e = 0; e < P; ++e) acc[e] = 0.f;
#pragma unroll
                for (int k = 0; k < 2 * CAP; ++k) {
                    const float mk = m[k];
#pragma unroll
                    for (int e = 0; e < P; ++e) {
                        float t = u[k][e];
                        if (k < CAP) t = k < a.n_mi ? t * f[k][e] : t;
                        acc[e] = fmaf(mk, t, acc[e]);
                    }
                }
                const float off = ft[FT_OFF + j];
#pragma unroll
                for (int e = 0; e < P; ++e) {
                    const float own = j < a.n_mi ? uj[e] * fj[e] : uj[e];
                    const float v = fmaf(a.beta, acc[e] - off, a.resid ? own : 0.f);
                    gf[e] = -gvj[e] * (v / fj[e]);
                }
            }
            if (j < a.K_in) {
                dot<2 * CAP, P>(ft + FT_MT + j * ROWS, gv, acc);
                const float s = ft[FT_INS + j];
#pragma unroll
                for (int e = 0; e < P; ++e) {
                    gt[e] = fmaf(a.beta, acc[e], a.resid ? gvj[e] : 0.f);
                    if (j < a.n_mi) {
                        gf[e] = fmaf(gt[e], uj[e], gf[e]);
                        gt[e] *= fj[e];
                    }
                    gt[e] *= s;
                }
                mk_st<T, P>(gxb + (long long)it[IT_IN + j] * hw, gt);
            }
            const float qs = ft[FT_QS + j];
#pragma unroll
            for (int e = 0; e < P; ++e) gq[e] = fmaf(a.eps * qs, gf[e], gq[e]);
            mk_st<T, P>(gxb + (long long)it[IT_Q + j] * hw, gq);
        }
        k0 = a.NQ;
    }
    for (int k = k0; k < a.K_in; ++k) {
        float acc[P], own[P];
        dot<2 * CAP, P>(ft + FT_MT + k * ROWS, gv, acc);
        if (a.resid) pick<2 * CAP>(gv, k, own);
        const float s = ft[FT_INS + k];
#pragma unroll
        for (int e = 0; e < P; ++e) acc[e] = s * fmaf(a.beta, acc[e], a.resid ? own[e] : 0.f);
        mk_st<T, P>(gxb + (long long)it[IT_IN + k] * hw, acc);
    }
    copy_planes<T, P>(gb, gxb, it + IT_COPY + a.NC, it + IT_COPY, a.NC, hw);
}

// ---- non-negativity --------------------------------------------------------------------------------------------------------
// sigmoid(t) and sigmoid(-t) from one exp(-|t|)
__device__ __forceinline__ void sigmoid2(float t, float& s, float& sneg) {
    const float e = expf(-fabsf(t)), d = 1.f / (1.f + e), lo = e * d;
    s = t >= 0.f ? d : lo;
    sneg = t >= 0.f ? lo : d;
}

// grid (pixel groups, C, B).  FWD: y = clamp(x);  BWD: y = g clamp'(x)
template <typename T, int P, bool BWD>
__global__ __launch_bounds__(CNT) void nonneg_kernel(const T* __restrict__ x, const T* __restrict__ g, T* __restrict__ y,
                                                     const int* __restrict__ slot, const float* __restrict__ offset, int mode, float eps,
                                                     float leak, long long hw) {
    const long long i = ((long long)blockIdx.x * CNT + threadIdx.x) * P;
    if (i >= hw) return;
    const int c = blockIdx.y;
    const long long at = ((long long)blockIdx.z * gridDim.y + c) * hw + i;
    const int sl = slot[c];
    float v[P];
    if (sl < 0) {          // (block-uniform) an untouched channel
        mk_ld<T, P>((BWD ? g : x) + at, v);
        mk_st<T, P>(y + at, v);
        return;
    }
    const float off = offset ? offset[sl] : 0.f;
    float gv[P];
    mk_ld<T, P>(x + at, v);
    if constexpr (BWD) mk_ld<T, P>(g + at, gv);
#pragma unroll
    for (int e = 0; e < P; ++e) {
        const float w = v[e] + off, t = w / eps;
        float s, sneg, r;
        if (mode == 2) {
            r = BWD ? (v[e] >= -off ? 1.f : 0.f) : (v[e] < -off ? -off : v[e]);
        } else if (mode == 0) {
            sigmoid2(t, s, sneg);
            r = BWD ? fmaf(t * s, sneg, s) : w * s - off;
        } else {
            sigmoid2(t, s, sneg);
            const float sp = fmaxf(t, 0.f) + log1pf(expf(-fabsf(t)));
            r = BWD ? fmaf(1.f - leak, s, leak) : fmaf(leak, w, (1.f - leak) * eps * (sp - 0.69314718055994531f)) - off;
        }
        v[e] = BWD ? gv[e] * r : r;
    }
    mk_st<T, P>(y + at, v);
}

bool dt_ok(int dt) { return dt == MK_F32 || dt == MK_BF16; }

int cmix_check(const char* what, const void* a, const void* b, const void* c, int dtype, const int* itab, const float* ftab, int B, int Cin,
               int Cout, int K_in, int K_out, int NQ, int n_mi, int n_mo, int NC, long long hw) {
    MK_REQUIRE(a && b && c && itab && ftab, "%s: null pointer (the tensors and both tables are required)", what);
    MK_REQUIRE(dt_ok(dtype), "%s: the tensors are f32 or bf16", what);
    MK_REQUIRE(B > 0 && B <= 65535, "%s: B = %d outside 1 .. 65535 (one grid row per sample)", what, B);
    MK_REQUIRE(Cin > 0 && Cout > 0, "%s: Cin = %d, Cout = %d must be positive", what, Cin, Cout);
    MK_REQUIRE(hw > 0 && (hw + CNT - 1) / CNT <= 0x7fffffffLL, "%s: HW = %lld pixels per plane: not positive, or beyond the grid", what, hw);
    MK_REQUIRE(K_in >= 1 && K_in <= ROWS && K_out >= 1 && K_out <= ROWS, "%s: K_in = %d, K_out = %d outside 1 .. %d (at most %d levels)", what,
               K_in, K_out, ROWS, LEV);
    MK_REQUIRE(NQ >= 0 && NQ <= LEV, "%s: NQ = %d humidity rows outside 0 .. %d", what, NQ, LEV);
    MK_REQUIRE(n_mi >= 0 && n_mo >= 0 && n_mi <= NQ && n_mo <= NQ && n_mi <= K_in && n_mo <= K_out,
               "%s: n_mi = %d, n_mo = %d moist rows next to NQ = %d humidity rows, K_in = %d, K_out = %d", what, n_mi, n_mo, NQ, K_in, K_out);
    MK_REQUIRE(NC >= 0 && (long long)K_in + NQ + NC == Cin && (long long)K_out + NQ + NC == Cout,
               "%s: K_in + NQ + NC = %d + %d + %d is not Cin = %d, or K_out + NQ + NC is not Cout = %d (every channel is written once)", what,
               K_in, NQ, NC, Cin, Cout);
    return 0;
}

int cmix_cap(int K_in, int K_out, int NQ) {
    const int rows = K_in > K_out ? K_in : K_out;
    return (rows <= 8 && NQ <= 4) ? 4 : (rows <= 16 && NQ <= 8) ? 8 : 16;
}

template <typename T, int P, int CAP>
void cmix_launch(bool bwd, const void* a, const void* b, void* c, const Cmix& d, int B, long long hw, hipStream_t st) {
    const dim3 grid((unsigned)((hw + (long long)CNT * P - 1) / ((long long)CNT * P)), (unsigned)B);
    if (!bwd) {
        if (d.NQ > 0) hipLaunchKernelGGL((cmix_fwd_kernel<T, P, CAP, true>), grid, dim3(CNT), 0, st, (const T*)a, (T*)c, d, hw);
        else hipLaunchKernelGGL((cmix_fwd_kernel<T, P, CAP, false>), grid, dim3(CNT), 0, st, (const T*)a, (T*)c, d, hw);
    } else {
        if (d.NQ > 0) hipLaunchKernelGGL((cmix_bwd_kernel<T, P, CAP, true>), grid, dim3(CNT), 0, st, (const T*)a, (const T*)b, (T*)c, d, hw);
        else hipLaunchKernelGGL((cmix_bwd_kernel<T, P, CAP, false>), grid, dim3(CNT), 0, st, (const T*)a, (const T*)b, (T*)c, d, hw);
    }
}

template <typename T, int P>
void cmix_launch_cap(int cap, bool bwd, const void* a, const void* b, void* c, const Cmix& d, int B, long long hw, hipStream_t st) {
    if (cap == 4) cmix_launch<T, P, 4>(bwd, a, b, c, d, B, hw, st);
    else if (cap == 8) cmix_launch<T, P, 8>(bwd, a, b, c, d, B, hw, st);
    else cmix_launch<T, P, 16>(bwd, a, b, c, d, B, hw, st);
}

// a: x (forward) or g (backward); b: x (backward, moist) or unused; c: y or gx
int cmix_run(const char* what, bool bwd, const void* a, const void* b, void* c, int dtype, const int* itab, const float* ftab, int B, int Cin,
             int Cout, int K_in, int K_out, int NQ, int n_mi, int n_mo, int NC, int flags, float beta, float eps, long long hw, void* stream) {
    if (int rc = cmix_check(what, a, (bwd && NQ > 0) ? b : a, c, dtype, itab, ftab, B, Cin, Cout, K_in, K_out, NQ, n_mi, n_mo, NC, hw)) return rc;
    MK_REQUIRE(flags >= 0 && flags < 4, "%s: flags = %d (bit 0 the residual form, bit 1 the humidity round trip)", what, flags);
    const Cmix d{itab, ftab, Cin, Cout, K_in, K_out, NQ, n_mi, n_mo, NC, flags & MK_CMIX_RESID, (flags & MK_CMIX_Q_ROUNDTRIP) ? 1 : 0, beta, eps};
    hipStream_t st = (hipStream_t)stream;
    const int cap = cmix_cap(K_in, K_out, NQ);
    const bool vec = hw % 4 == 0 && mk_aligned16(a) && mk_aligned16(b) && mk_aligned16(c);
    if (dtype == MK_BF16) {
        if (vec) cmix_launch_cap<u16, 4>(cap, bwd, a, b, c, d, B, hw, st);
        else cmix_launch_cap<u16, 1>(cap, bwd, a, b, c, d, B, hw, st);
    } else {
        if (vec) cmix_launch_cap<float, 4>(cap, bwd, a, b, c, d, B, hw, st);
        else cmix_launch_cap<float, 1>(cap, bwd, a, b, c, d, B, hw, st);
    }
    return mk_check_launch(what);
}

template <typename T, bool BWD>
void nonneg_launch(bool vec, const void* x, const void* g, void* y, const int* slot, const float* offset, int mode, float eps, float leak, int B,
                   int C, long long hw, hipStream_t st) {
    const int P = vec ? 4 : 1;
    const dim3 grid((unsigned)((hw + (long long)CNT * P - 1) / ((long long)CNT * P)), (unsigned)C, (unsigned)B);
    if (vec) hipLaunchKernelGGL((nonneg_kernel<T, 4, BWD>), grid, dim3(CNT), 0, st, (const T*)x, (const T*)g, (T*)y, slot, offset, mode, eps, leak, hw);
    else hipLaunchKernelGGL((nonneg_kernel<T, 1, BWD>), grid, dim3(CNT), 0, st, (const T*)x, (const T*)g, (T*)y, slot, offset, mode, eps, leak, hw);
}

int nonneg_run(const char* what, bool bwd, const void* x, const void* g, void* y, int dtype, const int* slot, const float* offset, int mode,
               float eps, float leak, int B, int C, long long hw, void* stream) {
    MK_REQUIRE(x && y && slot && (!bwd || g), "%s: null pointer (x, %sthe result and the channel slots are required)", what, bwd ? "g, " : "");
    MK_REQUIRE(dt_ok(dtype), "%s: the tensors are f32 or bf16", what);
    MK_REQUIRE(mode >= 0 && mode <= 2, "%s: mode = %d (0 silu, 1 softplus, 2 hard clamp)", what, mode);
    MK_REQUIRE(mode == 2 || eps > 0.f, "%s: eps = %g must be positive", what, (double)eps);
    MK_REQUIRE(B > 0 && B <= 65535 && C > 0 && C <= 65535, "%s: B = %d, C = %d outside 1 .. 65535", what, B, C);
    MK_REQUIRE(hw > 0 && (hw + CNT - 1) / CNT <= 0x7fffffffLL, "%s: HW = %lld pixels per plane: not positive, or beyond the grid", what, hw);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = hw % 4 == 0 && mk_aligned16(x) && mk_aligned16(g) && mk_aligned16(y);
    if (dtype == MK_BF16) {
        if (bwd) nonneg_launch<u16, true>(vec, x, g, y, slot, offset, mode, eps, leak, B, C, hw, st);
        else nonneg_launch<u16, false>(vec, x, g, y, slot, offset, mode, eps, leak, B, C, hw, st);
    } else {
        if (bwd) nonneg_launch<float, true>(vec, x, g, y, slot, offset, mode, eps, leak, B, C, hw, st);
        else nonneg_launch<float, false>(vec, x, g, y, slot, offset, mode, eps, leak, B, C, hw, st);
    }
    return mk_check_launch(what);
}

}  // namespace

extern "C" int mk_cmix_fwd(const void* x, void* y, int dtype, const int* itab, const float* ftab, int B, int Cin, int Cout, int K_in, int K_out,
                           int NQ, int n_mi, int n_mo, int NC, int flags, float beta, float eps, long long hw, void* stream) {
    return cmix_run("mk_cmix_fwd", false, x, nullptr, y, dtype, itab, ftab, B, Cin, Cout, K_in, K_out, NQ, n_mi, n_mo, NC, flags, beta, eps, hw,
                    stream);
}

extern "C" int mk_cmix_bwd(const void* g, const void* x, void* gx, int dtype, const int* itab, const float* ftab, int B, int Cin, int Cout,
                           int K_in, int K_out, int NQ, int n_mi, int n_mo, int NC, int flags, float beta, float eps, long long hw, void* stream) {
    return cmix_run("mk_cmix_bwd", true, g, x, gx, dtype, itab, ftab, B, Cin, Cout, K_in, K_out, NQ, n_mi, n_mo, NC, flags, beta, eps, hw,
                    stream);
}

extern "C" int mk_nonneg_fwd(const void* x, void* y, int dtype, const int* slot, const float* offset, int mode, float eps, float leak, int B,
                             int C, long long hw, void* stream) {
    return nonneg_run("mk_nonneg_fwd", false, x, nullptr, y, dtype, slot, offset, mode, eps, leak, B, C, hw, stream);
}

extern "C" int mk_nonneg_bwd(const void* g, const void* x, void* gx, int dtype, const int* slot, const float* offset, int mode, float eps,
                             float leak, int B, int C, long long hw, void* stream) {
    return nonneg_run("mk_nonneg_bwd", true, x, g, gx, dtype, slot, offset, mode, eps, leak, B, C, hw, stream);
}
