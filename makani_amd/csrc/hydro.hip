// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (see escore.hip: the SLP vectoriser's packed-fp32 forms are kept out of this library; tests/test_packed_forms.py scans the ISA)
// The hydrostatic-balance loss (makani/utils/losses/hydrostatic_loss.py) and what LossHandler does to its tensors before any
// loss sees them (makani/utils/loss.py:392-429), forward and backward (gfx950).
//
//   mk_hydro_sums / mk_hydro_grad    sum over the plane of  q w r_k^2,  k < K - 1 level intervals, per sample
//       Z_k = zs_k x[z_ch[k]] + zb_k          the geopotential over R_d          T_k = ts_k x[t_ch[k]] + tb_k
//       T_k *= 1 + eps (qs_k x[q_ch[k]] + qb_k)                                   (the moist form: virtual temperature)
//       r_k = (Z_{k+1} - Z_k) + hl_k (T_k + T_{k+1}),   hl_k = 1/2 ln(p_{k+1} / p_k)
//     A thread owns P consecutive pixels (P = 4: one 16-byte f32 / 8-byte bf16 access per channel, when HW is a multiple of 4
//     and every pointer is 16-byte aligned; P = 1 otherwise) and keeps their z, t (and q) columns in registers, as
//     constraints.hip does: loops over the column are unrolled over the compile-time capacity CAP = 4, 8, 16 levels, rows beyond
//     K re-read the table's padding channel and are never written.  The large terms never meet in fp32: the biases of an
//     interval are folded on the host, in fp64, into ONE constant c_k = zb_{k+1} - zb_k + hl_k (tb_k + tb_{k+1}) (the imbalance of
//     the mean state), and the kernel adds the deviations to it in one FMA chain, the geopotential difference first:
//       r_k = hl_k (d_k + d_{k+1}) + (zs_{k+1} x_{k+1} - zs_k x_k + c_k),   d_k = ts_k x_k (+ eps q_k T_k): T_k f_k - tb_k.
//     All coefficients are the same for every lane: one device table, wave-uniform addresses (scalar loads).
//     Forward: a block walks one chunk of the plane (mk_plane_chunks), sums each interval with mk_block_sum_t0 and writes
//     part[n][k][chunk]; hydro_finish adds the chunks in index order.  No atomics: repeats are bit-identical.
//     Backward: e_k = 2 g[n][k] q w r_k;  gZ_k = e_{k-1} - e_k,  gT_k = hl_k e_k + hl_{k-1} e_{k-1};  gx[z_ch[k]] = zs_k gZ_k,
//     gx[t_ch[k]] = ts_k f_k gT_k,  gx[q_ch[k]] = qs_k eps T_k gT_k (T_k before the correction), zero on the `rest` channels:
//     every channel of gx is written once, no memset beforehand.
//
//   mk_loss_prep_fwd / mk_loss_prep_bwd    one streaming pass over the E members (and the target / input state):
//       mean = inv sum_e prd_e (sequential fp32 sum over e),  prd_t_e = prd_e - inp,  mean_t = mean - inp,  tar_t = tar - inp
//     and only the outputs selected by `flags` are written; backward  g_prd_e = g_prd_t_e + inv (g_mean + g_mean_t).
#include "block_io.h"

namespace {

constexpr int CNT = 256;
constexpr int LEV = MK_CMIX_LEVELS;
// the int table: z_ch, t_ch, q_ch (LEV each, padded with a valid channel), then the NR untouched channels
constexpr int IT_Z = 0, IT_T = LEV, IT_Q = 2 * LEV, IT_REST = 3 * LEV;
// the float table (LEV each): zs, c, ts, tb, qs, qb, hl
constexpr int FT_ZS = 0, FT_CK = LEV, FT_TS = 2 * LEV, FT_TB = 3 * LEV, FT_QS = 4 * LEV, FT_QB = 5 * LEV, FT_HL = 6 * LEV;
static_assert(IT_REST == MK_HYDRO_ITAB && FT_HL + LEV == MK_HYDRO_FTAB, "table sizes of include/makani_amd.h");

struct Hyd {
    const int* it;
    const float* ft;
    int C, K, NR;
    float eps;
    long long w_sn, w_sk;          // strides of the weight over samples and intervals (0: broadcast)
};

// the columns of P pixels: z stays raw (scaled where it is used); t becomes the DEVIATION of the (virtual) temperature from the
// bias, ts x (+ eps q T): the biases sit in the table's folded constant c_k.  td (dry physical T) and f only in the moist forms.
template <typename T, int P, int CAP, bool MOIST>
__device__ __forceinline__ void load_columns(const T* __restrict__ xb, const Hyd& a, long long hw, float (&z)[CAP][P], float (&t)[CAP][P],
                                             float (&td)[MOIST ? CAP : 1][P], float (&f)[MOIST ? CAP : 1][P]) {
    const int* __restrict__ it = a.it;
    const float* __restrict__ ft = a.ft;
#pragma unroll
    for (int k = 0; k < CAP; ++k) mk_ld<T, P>(xb + (long long)it[IT_Z + k] * hw, z[k]);
#pragma unroll
    for (int k = 0; k < CAP; ++k) mk_ld<T, P>(xb + (long long)it[IT_T + k] * hw, t[k]);
    if constexpr (MOIST) {
#pragma unroll
        for (int k = 0; k < CAP; ++k) mk_ld<T, P>(xb + (long long)it[IT_Q + k] * hw, f[k]);
#pragma unroll
        for (int k = 0; k < CAP; ++k) {
            const float s = ft[FT_TS + k], b = ft[FT_TB + k], qs = ft[FT_QS + k], qb = ft[FT_QB + k];
#pragma unroll
            for (int e = 0; e < P; ++e) {
                const float eq = a.eps * fmaf(qs, f[k][e], qb);
                td[k][e] = fmaf(s, t[k][e], b);
                t[k][e] = fmaf(s, t[k][e], eq * td[k][e]);          // T f - tb
                f[k][e] = 1.f + eq;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < CAP; ++k) {
            const float s = ft[FT_TS + k];
#pragma unroll
            for (int e = 0; e < P; ++e) t[k][e] *= s;
        }
    }
}

// r_k of P pixels (k a compile-time index): every term is of the size of a deviation, the constant of the size of the mean imbalance
template <int P, int CAP>
__device__ __forceinline__ void residual(const float* __restrict__ ft, int k, const float (&z)[CAP][P], const float (&t)[CAP][P], float (&r)[P]) {
    const float z1 = ft[FT_ZS + k + 1], z0 = ft[FT_ZS + k], ck = ft[FT_CK + k], hl = ft[FT_HL + k];
#pragma unroll
    for (int e = 0; e < P; ++e) {
        const float dz = fmaf(-z0, z[k][e], fmaf(z1, z[k + 1][e], ck));
        r[e] = fmaf(hl, t[k][e] + t[k + 1][e], dz);
    }
}

// grid (chunks, N): block (c, n) sums the pixels [c per, (c + 1) per) of sample n; per is a multiple of CNT * 4
template <typename T, int P, int CAP, bool MOIST>
__global__ __launch_bounds__(CNT) void hydro_sums_kernel(const T* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ quad,
                                                         float* __restrict__ part, Hyd a, long long hw, long long per) {
    __shared__ float red[CAP - 1][CNT / 64];
    const float* __restrict__ ft = a.ft;
    const int n = blockIdx.y, Km1 = a.K - 1;
    const long long lo = (long long)blockIdx.x * per, hi = lo + per < hw ? lo + per : hw;
    const T* xn = x + (long long)n * a.C * hw;
    const float* wn = wgt ? wgt + (long long)n * a.w_sn : nullptr;
    float acc[CAP - 1];
#pragma unroll
    for (int k = 0; k < CAP - 1; ++k) acc[k] = 0.f;
    for (long long i = lo + (long long)threadIdx.x * P; i < hi; i += (long long)CNT * P) {
        float z[CAP][P], t[CAP][P], td[MOIST ? CAP : 1][P], f[MOIST ? CAP : 1][P], qv[P], w[P];
        load_columns<T, P, CAP, MOIST>(xn + i, a, hw, z, t, td, f);
        mk_ld<float, P>(quad + i, qv);
        if (wn && a.w_sk == 0) mk_ld<float, P>(wn + i, w);
#pragma unroll
        for (int k = 0; k < CAP - 1; ++k) {
            if (k < Km1) {          // (wave-uniform)
                float r[P];
                residual<P, CAP>(ft, k, z, t, r);
                if (wn && a.w_sk != 0) mk_ld<float, P>(wn + (long long)k * a.w_sk + i, w);
#pragma unroll
                for (int e = 0; e < P; ++e) {
                    float v = r[e] * r[e];
                    if (wn) v *= w[e];
                    acc[k] = fmaf(v, qv[e], acc[k]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < CAP - 1; ++k) {
        if (k < Km1) {
            const float s = mk_block_sum_t0<CNT>(acc[k], red[k]);
            if (threadIdx.x == 0) part[((long long)n * Km1 + k) * gridDim.x + blockIdx.x] = s;
        }
    }
}

// out[j] = the chunks of row j added in index order
__global__ __launch_bounds__(CNT) void hydro_finish(const float* __restrict__ part, float* __restrict__ out, long long rows, int chunks) {
    const long long j = (long long)blockIdx.x * CNT + threadIdx.x;
    if (j >= rows) return;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[j * chunks + c];
    out[j] = s;
}

// grid (pixel groups, N)
template <typename T, int P, int CAP, bool MOIST>
__global__ __launch_bounds__(CNT) void hydro_grad_kernel(const T* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ quad,
                                                         const float* __restrict__ g, T* __restrict__ gx, Hyd a, long long hw) {
    const long long i = ((long long)blockIdx.x * CNT + threadIdx.x) * P;
    if (i >= hw) return;
    const int* __restrict__ it = a.it;
    const float* __restrict__ ft = a.ft;
    const int n = blockIdx.y, Km1 = a.K - 1;
    const T* xn = x + (long long)n * a.C * hw + i;
    T* gn = gx + (long long)n * a.C * hw + i;
    const float* wn = wgt ? wgt + (long long)n * a.w_sn + i : nullptr;
    float z[CAP][P], t[CAP][P], td[MOIST ? CAP : 1][P], f[MOIST ? CAP : 1][P], qv[P], w[P], c[CAP][P];
    load_columns<T, P, CAP, MOIST>(xn, a, hw, z, t, td, f);
    mk_ld<float, P>(quad + i, qv);
    if (wn && a.w_sk == 0) mk_ld<float, P>(wn, w);
    // c[k] = e_k = 2 g_k q w r_k, zero from K - 1 on
#pragma unroll
    for (int k = 0; k < CAP; ++k) {
#pragma unroll
        for (int e = 0; e < P; ++e) c[k][e] = 0.f;
        if (k < CAP - 1 && k < Km1) {
            float r[P];
            residual<P, CAP>(ft, k < CAP - 1 ? k : 0, z, t, r);
            if (wn && a.w_sk != 0) mk_ld<float, P>(wn + (long long)k * a.w_sk, w);
            const float gk = 2.f * g[(long long)n * Km1 + k];
#pragma unroll
            for (int e = 0; e < P; ++e) {
                float v = gk * qv[e];
                if (wn) v *= w[e];
                c[k][e] = v * r[e];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < CAP; ++k) {
        if (k < a.K) {
            const float zs = ft[FT_ZS + k], ts = ft[FT_TS + k], hl = ft[FT_HL + k], hlm = k > 0 ? ft[FT_HL + k - 1] : 0.f;
            float gz[P], gt[P];
#pragma unroll
            for (int e = 0; e < P; ++e) {
                const float cm = k > 0 ? c[k > 0 ? k - 1 : 0][e] : 0.f;
                gz[e] = zs * (cm - c[k][e]);
                gt[e] = fmaf(hl, c[k][e], hlm * cm);          // (hl_{K-1} is zero in the table)
            }
            mk_st<T, P>(gn + (long long)it[IT_Z + k] * hw, gz);
            if constexpr (MOIST) {
                float gq[P];
                const float qe = ft[FT_QS + k] * a.eps;
#pragma unroll
                for (int e = 0; e < P; ++e) {
                    gq[e] = qe * td[k][e] * gt[e];
                    gt[e] *= ts * f[k][e];
                }
                mk_st<T, P>(gn + (long long)it[IT_Q + k] * hw, gq);
            } else {
#pragma unroll
                for (int e = 0; e < P; ++e) gt[e] *= ts;
            }
            mk_st<T, P>(gn + (long long)it[IT_T + k] * hw, gt);
        }
    }
    float zero[P];
#pragma unroll
    for (int e = 0; e < P; ++e) zero[e] = 0.f;
    for (int r = 0; r < a.NR; ++r) mk_st<T, P>(gn + (long long)it[IT_REST + r] * hw, zero);
}

int hydro_check(const char* what, const void* x, const float* quad, const void* out, int dtype, const int* itab, const float* ftab, int N, int C,
                int K, int NQ, int NR, long long hw, long long w_sn, long long w_sk) {
    MK_REQUIRE(x && quad && out && itab && ftab, "%s: null pointer (x, the quadrature weights, the result and both tables are required)", what);
    MK_REQUIRE(dtype == MK_F32 || dtype == MK_BF16, "%s: x is f32 or bf16", what);
    MK_REQUIRE(N > 0 && N <= 65535, "%s: N = %d samples outside 1 .. 65535 (one grid row per sample)", what, N);
    MK_REQUIRE(K >= 2 && K <= LEV, "%s: K = %d levels outside 2 .. %d (the column lives in registers)", what, K, LEV);
    MK_REQUIRE(NQ == 0 || NQ == K, "%s: NQ = %d humidity levels: 0 (dry) or K = %d", what, NQ, K);
    MK_REQUIRE(NR >= 0 && (long long)2 * K + NQ + NR == C, "%s: 2 K + NQ + NR = 2 * %d + %d + %d is not C = %d (every channel is written once)", what,
               K, NQ, NR, C);
    MK_REQUIRE(hw > 0 && (hw + CNT - 1) / CNT <= 0x7fffffffLL, "%s: HW = %lld pixels per plane: not positive, or beyond the grid", what, hw);
    MK_REQUIRE(w_sn >= 0 && w_sk >= 0, "%s: negative weight stride", what);
    return 0;
}

int hydro_cap(int K) { return K <= 4 ? 4 : K <= 8 ? 8 : 16; }

bool hydro_vec(long long hw, const void* a, const void* b, const void* c, const void* d, long long s0, long long s1) {
    return hw % 4 == 0 && s0 % 4 == 0 && s1 % 4 == 0 && mk_aligned16(a) && mk_aligned16(b) && mk_aligned16(c) && mk_aligned16(d);
}

template <typename T, int P, int CAP>
void hydro_launch(bool grad, const void* x, const float* wgt, const float* quad, const float* g, void* out, const Hyd& d, bool moist, int N,
                  long long hw, int chunks, long long per, hipStream_t st) {
    if (!grad) {
        const dim3 grid((unsigned)chunks, (unsigned)N);
        if (moist) hipLaunchKernelGGL((hydro_sums_kernel<T, P, CAP, true>), grid, dim3(CNT), 0, st, (const T*)x, wgt, quad, (float*)out, d, hw, per);
        else hipLaunchKernelGGL((hydro_sums_kernel<T, P, CAP, false>), grid, dim3(CNT), 0, st, (const T*)x, wgt, quad, (float*)out, d, hw, per);
    } else {
        const dim3 grid((unsigned)((hw + (long long)CNT * P - 1) / ((long long)CNT * P)), (unsigned)N);
        if (moist) hipLaunchKernelGGL((hydro_grad_kernel<T, P, CAP, true>), grid, dim3(CNT), 0, st, (const T*)x, wgt, quad, g, (T*)out, d, hw);
        else hipLaunchKernelGGL((hydro_grad_kernel<T, P, CAP, false>), grid, dim3(CNT), 0, st, (const T*)x, wgt, quad, g, (T*)out, d, hw);
    }
}

template <typename T, int P>
void hydro_launch_cap(int cap, bool grad, const void* x, const float* wgt, const float* quad, const float* g, void* out, const Hyd& d, bool moist,
                      int N, long long hw, int chunks, long long per, hipStream_t st) {
    if (cap == 4) hydro_launch<T, P, 4>(grad, x, wgt, quad, g, out, d, moist, N, hw, chunks, per, st);
    else if (cap == 8) hydro_launch<T, P, 8>(grad, x, wgt, quad, g, out, d, moist, N, hw, chunks, per, st);
    else hydro_launch<T, P, 16>(grad, x, wgt, quad, g, out, d, moist, N, hw, chunks, per, st);
}

void hydro_dispatch(bool grad, const void* x, int dtype, const float* wgt, const float* quad, const float* g, void* out, const Hyd& d, bool moist,
                    int N, long long hw, int chunks, long long per, hipStream_t st) {
    const bool vec = hydro_vec(hw, x, wgt, quad, grad ? out : nullptr, d.w_sn, d.w_sk);
    const int cap = hydro_cap(d.K);
    if (dtype == MK_BF16) {
        if (vec) hydro_launch_cap<u16, 4>(cap, grad, x, wgt, quad, g, out, d, moist, N, hw, chunks, per, st);
        else hydro_launch_cap<u16, 1>(cap, grad, x, wgt, quad, g, out, d, moist, N, hw, chunks, per, st);
    } else {
        if (vec) hydro_launch_cap<float, 4>(cap, grad, x, wgt, quad, g, out, d, moist, N, hw, chunks, per, st);
        else hydro_launch_cap<float, 1>(cap, grad, x, wgt, quad, g, out, d, moist, N, hw, chunks, per, st);
    }
}

// ---- the handler's preparation pass ----------------------------------------------------------------------------------------
struct Prep {
    int E, flags;
    float inv;
    long long n, inp_stride;          // elements of one sample (C HW); elements between the input states of two samples
};

// grid (point groups of one sample, B)
template <typename T, int P, int CAP>
__global__ __launch_bounds__(CNT) void loss_prep_fwd_kernel(const T* __restrict__ prd, const T* __restrict__ tar, const T* __restrict__ inp,
                                                            T* __restrict__ mean, T* __restrict__ prd_t, T* __restrict__ mean_t,
                                                            T* __restrict__ tar_t, Prep a) {
    const long long i = ((long long)blockIdx.x * CNT + threadIdx.x) * P;
    if (i >= a.n) return;
    const long long b = blockIdx.y;
    const T* pb = prd + b * a.E * a.n + i;
    float m[CAP][P], x0[P], s[P];
#pragma unroll
    for (int e = 0; e < CAP; ++e) {
        if (e < a.E) mk_ld<T, P>(pb + (long long)e * a.n, m[e]);          // (wave-uniform)
    }
    const bool tend = (a.flags & (MK_PREP_MEMBER_T | MK_PREP_MEAN_T | MK_PREP_TAR_T)) != 0;
    if (tend) mk_ld<T, P>(inp + b * a.inp_stride + i, x0);
    if (a.flags & (MK_PREP_MEAN | MK_PREP_MEAN_T)) {
#pragma unroll
        for (int e = 0; e < P; ++e) s[e] = 0.f;
#pragma unroll
        for (int e = 0; e < CAP; ++e) {
            if (e < a.E) {
#pragma unroll
                for (int j = 0; j < P; ++j) s[j] += m[e][j];
            }
        }
#pragma unroll
        for (int j = 0; j < P; ++j) s[j] *= a.inv;
        if (a.flags & MK_PREP_MEAN) mk_st<T, P>(mean + b * a.n + i, s);
        if (a.flags & MK_PREP_MEAN_T) {
#pragma unroll
            for (int j = 0; j < P; ++j) s[j] -= x0[j];
            mk_st<T, P>(mean_t + b * a.n + i, s);
        }
    }
    if (a.flags & MK_PREP_MEMBER_T) {
        T* ob = prd_t + b * a.E * a.n + i;
#pragma unroll
        for (int e = 0; e < CAP; ++e) {
            if (e < a.E) {
                float d[P];
#pragma unroll
                for (int j = 0; j < P; ++j) d[j] = m[e][j] - x0[j];
                mk_st<T, P>(ob + (long long)e * a.n, d);
            }
        }
    }
    if (a.flags & MK_PREP_TAR_T) {
        float t[P];
        mk_ld<T, P>(tar + b * a.n + i, t);
#pragma unroll
        for (int j = 0; j < P; ++j) t[j] -= x0[j];
        mk_st<T, P>(tar_t + b * a.n + i, t);
    }
}

// grid (point groups of one sample, B)
template <typename T, int P>
__global__ __launch_bounds__(CNT) void loss_prep_bwd_kernel(const T* __restrict__ g_prd_t, const T* __restrict__ g_mean, const T* __restrict__ g_mean_t,
                                                            T* __restrict__ g_prd, Prep a) {
    const long long i = ((long long)blockIdx.x * CNT + threadIdx.x) * P;
    if (i >= a.n) return;
    const long long b = blockIdx.y;
    float s[P], v[P];
#pragma unroll
    for (int j = 0; j < P; ++j) s[j] = 0.f;
    if (g_mean) {
        mk_ld<T, P>(g_mean + b * a.n + i, v);
#pragma unroll
        for (int j = 0; j < P; ++j) s[j] += v[j];
    }
    if (g_mean_t) {
        mk_ld<T, P>(g_mean_t + b * a.n + i, v);
#pragma unroll
        for (int j = 0; j < P; ++j) s[j] += v[j];
    }
#pragma unroll
    for (int j = 0; j < P; ++j) s[j] *= a.inv;
    for (int e = 0; e < a.E; ++e) {
        const long long at = (b * a.E + e) * a.n + i;
        if (g_prd_t) {
            mk_ld<T, P>(g_prd_t + at, v);
#pragma unroll
            for (int j = 0; j < P; ++j) v[j] += s[j];
            mk_st<T, P>(g_prd + at, v);
        } else {
            mk_st<T, P>(g_prd + at, s);
        }
    }
}

int prep_check(const char* what, int dtype, int B, int E, long long n, int flags) {
    MK_REQUIRE(dtype == MK_F32 || dtype == MK_BF16, "%s: the tensors are f32 or bf16", what);
    MK_REQUIRE(B > 0 && B <= 65535, "%s: B = %d outside 1 .. 65535 (one grid row per sample)", what, B);
    MK_REQUIRE(E >= 1, "%s: E = %d members", what, E);
    MK_REQUIRE(n > 0 && (n + CNT - 1) / CNT <= 0x7fffffffLL, "%s: C * HW = %lld points per sample: not positive, or beyond the grid", what, n);
    MK_REQUIRE(flags > 0 && flags < 16, "%s: flags = %d selects no output (bits: mean, member tendencies, mean tendency, target tendency)", what,
               flags);
    return 0;
}

}  // namespace

extern "C" int mk_hydro_chunks(long long hw) { return mk_plane_chunks(hw); }

extern "C" int mk_hydro_sums(const void* x, int dtype, const float* wgt, long long w_sn, long long w_sk, const float* quad, float* out, float* ws,
                             const int* itab, const float* ftab, int N, int C, int K, int NQ, int NR, float eps, long long hw, void* stream) {
    if (int rc = hydro_check("mk_hydro_sums", x, quad, out, dtype, itab, ftab, N, C, K, NQ, NR, hw, w_sn, w_sk)) return rc;
    MK_REQUIRE(ws, "mk_hydro_sums: null workspace (N * (K - 1) * mk_hydro_chunks(HW) floats)");
    const int chunks = mk_plane_chunks(hw);
    const long long unit = (long long)CNT * 4, per = ((hw + chunks - 1) / chunks + unit - 1) / unit * unit;
    const Hyd d{itab, ftab, C, K, NR, eps, w_sn, w_sk};
    hipStream_t st = (hipStream_t)stream;
    hydro_dispatch(false, x, dtype, wgt, quad, nullptr, ws, d, NQ > 0, N, hw, chunks, per, st);
    const long long rows = (long long)N * (K - 1);
    hipLaunchKernelGGL(hydro_finish, dim3((unsigned)((rows + CNT - 1) / CNT)), dim3(CNT), 0, st, ws, out, rows, chunks);
    return mk_check_launch("mk_hydro_sums");
}

extern "C" int mk_hydro_grad(const void* x, int dtype, const float* wgt, long long w_sn, long long w_sk, const float* quad, const float* g, void* gx,
                             const int* itab, const float* ftab, int N, int C, int K, int NQ, int NR, float eps, long long hw, void* stream) {
    if (int rc = hydro_check("mk_hydro_grad", x, quad, gx, dtype, itab, ftab, N, C, K, NQ, NR, hw, w_sn, w_sk)) return rc;
    MK_REQUIRE(g, "mk_hydro_grad: null upstream gradient (N, K - 1)");
    const Hyd d{itab, ftab, C, K, NR, eps, w_sn, w_sk};
    hydro_dispatch(true, x, dtype, wgt, quad, g, gx, d, NQ > 0, N, hw, 0, 0, (hipStream_t)stream);
    return mk_check_launch("mk_hydro_grad");
}

extern "C" int mk_loss_prep_fwd(const void* prd, const void* tar, const void* inp, long long inp_stride, int dtype, void* mean, void* prd_t,
                                void* mean_t, void* tar_t, int flags, float inv, int B, int E, long long n, void* stream) {
    if (int rc = prep_check("mk_loss_prep_fwd", dtype, B, E, n, flags)) return rc;
    const bool tend = (flags & (MK_PREP_MEMBER_T | MK_PREP_MEAN_T | MK_PREP_TAR_T)) != 0;
    MK_REQUIRE(prd && (!tend || inp) && (!(flags & MK_PREP_TAR_T) || tar), "mk_loss_prep_fwd: null input (prd; inp for a tendency; tar for its tendency)");
    MK_REQUIRE((!(flags & MK_PREP_MEAN) || mean) && (!(flags & MK_PREP_MEMBER_T) || prd_t) && (!(flags & MK_PREP_MEAN_T) || mean_t) &&
                   (!(flags & MK_PREP_TAR_T) || tar_t),
               "mk_loss_prep_fwd: flags = %d selects an output whose pointer is null", flags);
    MK_REQUIRE(!tend || inp_stride >= n, "mk_loss_prep_fwd: inp_stride = %lld is below C * HW = %lld", inp_stride, n);
    const Prep a{E, flags, inv, n, tend ? inp_stride : 0};
    hipStream_t st = (hipStream_t)stream;
    const bool vec = n % 4 == 0 && a.inp_stride % 4 == 0 && mk_aligned16(prd) && mk_aligned16(tar) && mk_aligned16(inp) && mk_aligned16(mean) &&
                     mk_aligned16(prd_t) && mk_aligned16(mean_t) && mk_aligned16(tar_t);
    const int P = vec ? 4 : 1;
    const dim3 grid((unsigned)((n + (long long)CNT * P - 1) / ((long long)CNT * P)), (unsigned)B);
    const int rc = mk_with_capacity<32, 2>(E, "mk_loss_prep_fwd", [&](auto cap) {
        constexpr int CAP = decltype(cap)::value;
#define MK_PREP_GO(T, PP)                                                                                                                  \
    hipLaunchKernelGGL((loss_prep_fwd_kernel<T, PP, CAP>), grid, dim3(CNT), 0, st, (const T*)prd, (const T*)tar, (const T*)inp, (T*)mean, \
                       (T*)prd_t, (T*)mean_t, (T*)tar_t, a)
        if (dtype == MK_BF16) {
            if (vec) MK_PREP_GO(u16, 4);
            else MK_PREP_GO(u16, 1);
        } else {
            if (vec) MK_PREP_GO(float, 4);
            else MK_PREP_GO(float, 1);
        }
#undef MK_PREP_GO
        return 0;
    });
    if (rc) return rc;
    return mk_check_launch("mk_loss_prep_fwd");
}

extern "C" int mk_loss_prep_bwd(const void* g_prd_t, const void* g_mean, const void* g_mean_t, void* g_prd, int dtype, float inv, int B, int E,
                                long long n, void* stream) {
    if (int rc = prep_check("mk_loss_prep_bwd", dtype, B, E, n, 1)) return rc;
    MK_REQUIRE(g_prd, "mk_loss_prep_bwd: null result");
    const Prep a{E, 0, inv, n, 0};
    hipStream_t st = (hipStream_t)stream;
    const bool vec = n % 4 == 0 && mk_aligned16(g_prd_t) && mk_aligned16(g_mean) && mk_aligned16(g_mean_t) && mk_aligned16(g_prd);
    const int P = vec ? 4 : 1;
    const dim3 grid((unsigned)((n + (long long)CNT * P - 1) / ((long long)CNT * P)), (unsigned)B);
#define MK_PREP_GO(T, PP) \
    hipLaunchKernelGGL((loss_prep_bwd_kernel<T, PP>), grid, dim3(CNT), 0, st, (const T*)g_prd_t, (const T*)g_mean, (const T*)g_mean_t, (T*)g_prd, a)
    if (dtype == MK_BF16) {
        if (vec) MK_PREP_GO(u16, 4);
        else MK_PREP_GO(u16, 1);
    } else {
        if (vec) MK_PREP_GO(float, 4);
        else MK_PREP_GO(float, 1);
    }
#undef MK_PREP_GO
    return mk_check_launch("mk_loss_prep_bwd");
}
