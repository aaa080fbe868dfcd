// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (gfx950: v_pk_mul_f32 / v_pk_add_f32 whose src1 is a VGPR pair read through op_sel return wrong results while certain
//  matrix-core kernels run on the same compute unit — tools/pk_hazard_probe.py, docs/LAB_NOTEBOOK.md round 6.  The SLP vectoriser
//  emits exactly those forms from plain scalar code, so this file is compiled without it; tools/pk_opsel_scan.py checks the ISA.)
// Ensemble energy scores on the sphere (gfx950): the Lp score on the grid, the Sobolev score and the per-degree spectral L2 score
// of makani/utils/losses/energy_score.py:30-652, in three stages.
//
//   members f[b][e][c][n] (B, E, C, N) f32 | bf16 | complex64 (re, im interleaved), in the caller's layout
//   observations o[b][c][n] f32 (complex64 with complex members); weights q[n] and, optionally, w[b][c][n]
//   a plane of N points is cut into S segments of N / S points: S = 1 (grid Lp, Sobolev) or one segment per degree l of an
//   (L, M) coefficient plane (spectral L2: the sum runs over m only)
//
// Stage 1, mk_escore_sums: for every (b, c, segment) the K = E + E (E - 1) / 2 weighted sums
//     sums[k = e]           = sum_n wt |o - f_e|^p            (skill, e < E)
//     sums[k = pair(i, j)]  = sum_n wt |f_i - f_j|^p          (spread, i < j, pairs in lexicographic order behind the skills)
//   with wt = q[n] * w[b][c][n].  The differences are formed directly in fp32: members of a trained ensemble are close, and the
//   Gram form G_ii + G_jj - 2 G_ij cancels exactly the digits the spread lives in.  Complex members use the squared modulus
//   (p = 2).  Real p: 2 and 1 are their own instantiations, every other p >= 1 goes through exp2(p log2 |d|).
//   A thread owns one point at a time and keeps the sums in registers; 528 sums (E = 32) do not fit, so the members are cut
//   into tiles of 8 and one grid dimension walks the tile pairs (ta <= tb): a block holds two tiles, at most 64 pair sums and
//   (on the diagonal ta == tb) 8 skill sums.  E <= 8 is ONE tile: every value is read once.  Larger ensembles RE-READ member
//   tiles: T = ceil(E / 8) tiles give T (T + 1) / 2 blocks per chunk, the T diagonal ones read one tile, the others two, T^2 tile
//   reads in all — T times the single-pass member traffic (E = 16: 2x, E = 32: 4x), and the observation and weights once per
//   block; the cost of not spilling.
//   Sums are deterministic: every block writes the partial sums of its chunk (wave shuffles, then the four waves in order),
//   escore_combine adds the chunks of a segment in order.  No floating-point atomics.
//   NaN masks as the reference: mode 0 (grid) masks a point whose observation is NaN, a NaN member there counts as 0
//   (:162-167); mode 1 (spectral) masks a point where the observation or ANY member is NaN (:391-396, :576-581).  With more
//   than one tile a block does not see every member, so for mode 1 a pre-pass (escore_mask_weights) folds the mask into a
//   weight plane first.
// Stage 2, mk_escore_finish: channel reduction in channel order, the `< eps` mask, the root ^(beta / p), the skill mean and
//   the spread normalisation 2 (E - 1 + alpha) / (E^2 (E - 1)) * 1/2 (exactly 0 for E = 1), an optional per-output-channel
//   spread scale, the sum over the segments.  Writes the loss (B, C_out) and the table d loss / d sums (B, C_out, S, K), zero
//   where masked.
// Stage 3, mk_escore_grad: gf[b][e][c][n] = gout[b][co] * wt * sum_k table[b][co][s][k] * d term_k / d f_e in the members'
//   dtype; complex gradients in torch's convention (d |z|^2 = 2 z).  One block owns a tile of 8 members of its points and
//   walks all tiles for the partners: E <= 8 reads everything once, larger ensembles re-read T times.  Masked points get 0.
#include "block_io.h"

namespace {

constexpr int ENT = 256;        // threads per block
constexpr int ETILE = 8;        // members per tile
constexpr int EMAX = 32;

__device__ __forceinline__ bool isnan_v(float v) { return v != v; }
__device__ __forceinline__ bool isnan_v(float2 v) { return v.x != v.x || v.y != v.y; }

// member value types: how a value is loaded, what a NaN is replaced with, |a - b|^p and its derivative with respect to a
template <typename T>
struct Val;
template <>
struct Val<float> {
    typedef float V;       // value in registers
    typedef float O;       // observation in memory
    static __device__ __forceinline__ V ld(const float* p) { return mk_ld(p); }
    static __device__ __forceinline__ void st(float* p, V v) { mk_st(p, v); }
};
template <>
struct Val<u16> {
    typedef float V;
    typedef float O;
    static __device__ __forceinline__ V ld(const u16* p) { return mk_ld(p); }
    static __device__ __forceinline__ void st(u16* p, V v) { mk_st(p, v); }
};
template <>
struct Val<float2> {
    typedef float2 V;
    typedef float2 O;
    static __device__ __forceinline__ V ld(const float2* p) { return *p; }
    static __device__ __forceinline__ void st(float2* p, V v) { *p = v; }
};

__device__ __forceinline__ float zero_of(float) { return 0.f; }
__device__ __forceinline__ float2 zero_of(float2) { return make_float2(0.f, 0.f); }

enum { P_TWO = 0, P_ONE = 1, P_ANY = 2 };

// |a - b|^p
template <int PM>
__device__ __forceinline__ float dist_p(float a, float b, float p) {
    const float d = a - b;
    if (PM == P_TWO) return d * d;
    if (PM == P_ONE) return fabsf(d);
    return exp2f(p * log2f(fabsf(d)));          // d = 0: exp2(-inf) = 0
}
template <int PM>
__device__ __forceinline__ float dist_p(float2 a, float2 b, float) {
    const float dx = a.x - b.x, dy = a.y - b.y;
    return dx * dx + dy * dy;
}
// acc += c * d |a - b|^p / d a
template <int PM>
__device__ __forceinline__ void grad_p(float& acc, float c, float a, float b, float p) {
    const float d = a - b;
    if (PM == P_TWO) {
        acc += c * 2.f * d;
    } else {
        const float s = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);
        acc += (PM == P_ONE) ? c * s : c * s * p * exp2f((p - 1.f) * log2f(fabsf(d)));
    }
}
template <int PM>
__device__ __forceinline__ void grad_p(float2& acc, float c, float2 a, float2 b, float) {
    acc.x += c * 2.f * (a.x - b.x);
    acc.y += c * 2.f * (a.y - b.y);
}

// index of the pair (i < j) among the K sums of an ensemble of E
__device__ __forceinline__ int pair_index(int i, int j, int E) { return E + i * (2 * E - i - 1) / 2 + (j - i - 1); }

// ---- stage 1 -------------------------------------------------------------------------------------------------------------
// One block: one chunk of one segment of one plane, one tile pair.  DIAG: ta == tb (skills + the pairs inside the tile).
template <typename T, int PM, int EM, bool DIAG>
__device__ __forceinline__ void sums_body(const T* __restrict__ fa, const T* __restrict__ fb, const typename Val<T>::O* __restrict__ op,
                                          const float* __restrict__ qp, const float* __restrict__ wp, float* __restrict__ out,
                                          int E, int a0, int b0, long long estride, long long seglen, int nanmode, float p,
                                          float* red) {
    typedef typename Val<T>::V V;
    const int na = min(EM, E - a0), nb = DIAG ? na : min(EM, E - b0);
    float skill[EM], pr[EM][EM];
#pragma unroll
    for (int i = 0; i < EM; ++i) {
        skill[i] = 0.f;
#pragma unroll
        for (int j = 0; j < EM; ++j) pr[i][j] = 0.f;
    }
    for (long long n = (long long)blockIdx.x * ENT + threadIdx.x; n < seglen; n += (long long)gridDim.x * ENT) {
        V va[EM], vb[EM];
        bool bad = false;
#pragma unroll
        for (int i = 0; i < EM; ++i) {
            va[i] = (i < na) ? Val<T>::ld(fa + i * estride + n) : zero_of(V());
            if (isnan_v(va[i])) {
                bad = true;
                va[i] = zero_of(V());
            }
        }
        if (!DIAG) {
#pragma unroll
            for (int j = 0; j < EM; ++j) {
                vb[j] = (j < nb) ? Val<T>::ld(fb + j * estride + n) : zero_of(V());
                if (isnan_v(vb[j])) {
                    bad = true;
                    vb[j] = zero_of(V());
                }
            }
        }
        V o = op[n];
        bool masked = isnan_v(o);
        if (masked) o = zero_of(V());
        if (nanmode == 1) masked = masked || bad;
        const float wt = masked ? 0.f : qp[n] * (wp ? wp[n] : 1.f);
        if (DIAG) {
#pragma unroll
            for (int i = 0; i < EM; ++i) {
                skill[i] += wt * dist_p<PM>(o, va[i], p);
#pragma unroll
                for (int j = i + 1; j < EM; ++j) pr[i][j] += wt * dist_p<PM>(va[i], va[j], p);
            }
        } else {
#pragma unroll
            for (int i = 0; i < EM; ++i)
#pragma unroll
                for (int j = 0; j < EM; ++j) pr[i][j] += wt * dist_p<PM>(va[i], vb[j], p);
        }
    }
    // wave sums, then the waves in order: slot i * EM + j for the pairs, EM * EM + i for the skills
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int SLOTS = EM * EM + EM;
#pragma unroll
    for (int i = 0; i < EM; ++i) {
#pragma unroll
        for (int j = DIAG ? i + 1 : 0; j < EM; ++j) {
            float v = pr[i][j];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) red[wave * SLOTS + i * EM + j] = v;
        }
        if (DIAG) {
            float v = skill[i];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) red[wave * SLOTS + EM * EM + i] = v;
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < SLOTS) {
        const bool is_skill = t >= EM * EM;
        const int i = is_skill ? t - EM * EM : t / EM, j = is_skill ? 0 : t % EM;
        bool valid;
        int k;
        if (is_skill) {
            valid = DIAG && i < na;
            k = a0 + i;
        } else {
            valid = i < na && j < nb && (!DIAG || j > i);
            k = pair_index(a0 + i, b0 + j, E);
        }
        if (valid) {
            float s = 0.f;
            for (int w = 0; w < ENT / 64; ++w) s += red[w * SLOTS + t];
            out[k] = s;
        }
    }
}

// grid: (chunks, S, planes * npairs).  out: (planes, S, chunks, K)
template <typename T, int PM, int EM>
__global__ __launch_bounds__(ENT) void escore_sums_kernel(const T* __restrict__ f, const typename Val<T>::O* __restrict__ obs,
                                                          const float* __restrict__ q, const float* __restrict__ w,
                                                          float* __restrict__ out, int E, int C, long long seglen, int ntile,
                                                          int nanmode, float p) {
    __shared__ float red[(ENT / 64) * (EM * EM + EM)];
    const int npairs = ntile * (ntile + 1) / 2;
    const int plane = blockIdx.z / npairs, b = plane / C, c = plane % C;
    int pi = blockIdx.z % npairs, ta = 0;
    while (pi >= ntile - ta) {          // pairs (ta, tb >= ta) in lexicographic order
        pi -= ntile - ta;
        ++ta;
    }
    const int tb = ta + pi;
    const int S = gridDim.y, s = blockIdx.y;
    const long long N = seglen * S, estride = (long long)C * N;
    const T* fp = f + ((long long)b * E * C + c) * N + (long long)s * seglen;
    const long long poff = (long long)plane * N + (long long)s * seglen;
    const int K = E + E * (E - 1) / 2;
    float* op = out + (((long long)plane * S + s) * gridDim.x + blockIdx.x) * K;
    const int a0 = ta * EM, b0 = tb * EM;
    if (ta == tb)
        sums_body<T, PM, EM, true>(fp + a0 * estride, fp + a0 * estride, obs + poff, q + (long long)s * seglen, w ? w + poff : nullptr, op,
                                   E, a0, a0, estride, seglen, nanmode, p, red);
    else if constexpr (EM == ETILE)          // (smaller tiles hold the whole ensemble: one tile, no off-diagonal pair)
        sums_body<T, PM, EM, false>(fp + a0 * estride, fp + b0 * estride, obs + poff, q + (long long)s * seglen, w ? w + poff : nullptr,
                                    op, E, a0, b0, estride, seglen, nanmode, p, red);
}

// sums[r][k] = sum over the chunks of partial[r][chunk][k], in chunk order
__global__ __launch_bounds__(ENT) void escore_combine(const float* __restrict__ partial, float* __restrict__ sums, long long rows, int chunks,
                                                      int K) {
    const long long i = (long long)blockIdx.x * ENT + threadIdx.x;
    if (i >= rows * K) return;
    const long long r = i / K;
    const int k = (int)(i % K);
    float s = 0.f;
    for (int ch = 0; ch < chunks; ++ch) s += partial[(r * chunks + ch) * K + k];
    sums[i] = s;
}

// mode-1 mask of an ensemble of more than one tile: wm[b][c][n] = (observation or any member NaN) ? 0 : w (or 1)
template <typename T>
__global__ __launch_bounds__(ENT) void escore_mask_weights(const T* __restrict__ f, const typename Val<T>::O* __restrict__ obs,
                                                           const float* __restrict__ w, float* __restrict__ wm, int E, int C, long long N) {
    const int plane = blockIdx.y, b = plane / C, c = plane % C;
    const T* fp = f + ((long long)b * E * C + c) * N;
    const long long estride = (long long)C * N, poff = (long long)plane * N;
    for (long long n = (long long)blockIdx.x * ENT + threadIdx.x; n < N; n += (long long)gridDim.x * ENT) {
        bool bad = isnan_v(obs[poff + n]);
        for (int e = 0; e < E; ++e) bad = bad || isnan_v(Val<T>::ld(fp + e * estride + n));
        wm[poff + n] = bad ? 0.f : (w ? w[poff + n] : 1.f);
    }
}

// ---- stage 2 -------------------------------------------------------------------------------------------------------------
// grid: B * Cout blocks.  sums (B, C, S, K) -> loss (B, Cout), table (B, Cout, S, K)
__global__ __launch_bounds__(ENT) void escore_finish_kernel(const float* __restrict__ sums, const float* __restrict__ scale, int nscale,
                                                            float* __restrict__ loss, float* __restrict__ table, int C, int Cout, int S,
                                                            int E, float p, float beta, float alpha, float eps) {
    __shared__ float red[ENT];
    const int b = blockIdx.x / Cout, co = blockIdx.x % Cout;
    const int K = E + E * (E - 1) / 2;
    const long long SK = (long long)S * K;
    const float ex = beta / p;
    const float fskill = 1.f / (float)E;
    const float sc = scale ? scale[nscale == 1 ? 0 : co] : 1.f;
    const float fpair = (E > 1) ? -sc * ((float)E - 1.f + alpha) / ((float)E * (float)E * (float)(E - 1)) : 0.f;
    float acc = 0.f;
    for (long long i = threadIdx.x; i < SK; i += ENT) {
        float v;
        if (Cout == 1 && C > 1) {
            v = 0.f;
            for (int c = 0; c < C; ++c) v += sums[((long long)b * C + c) * SK + i];
        } else {
            v = sums[((long long)b * C + co) * SK + i];
        }
        const bool masked = v < eps;
        const float r = (ex == 0.5f) ? sqrtf(v) : powf(v, ex);
        const float fac = ((int)(i % K) < E) ? fskill : fpair;
        acc += masked ? 0.f : fac * r;
        table[((long long)b * Cout + co) * SK + i] = masked ? 0.f : fac * ex * r / v;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = ENT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[blockIdx.x] = red[0];
}

// Stage 2 of the Gaussian maximum mean discrepancy (GaussianMMDLoss, makani/utils/losses/mmd_loss.py:190-219) on the sums of
// stage 1 (S = 1, p = beta): channel sum in channel order, k = exp(-s^2 / 2 sigma), the skill mean sum_e k_e / E and the spread
// sum_{i != j} k_ij (E - 1 + alpha) / (E^2 (E - 1)) (every unordered pair twice; exactly 0 for E = 1), loss = skill - spread / 2.
// grid: B * Cout blocks.  sums (B, C, 1, K) -> loss (B, Cout), table (B, Cout, 1, K) = d loss / d sums for mk_escore_grad
__global__ __launch_bounds__(ENT) void mmd_finish_kernel(const float* __restrict__ sums, float* __restrict__ loss, float* __restrict__ table,
                                                         int C, int Cout, int E, float sigma, float alpha) {
    __shared__ float red[ENT];
    const int b = blockIdx.x / Cout, co = blockIdx.x % Cout;
    const int K = E + E * (E - 1) / 2;
    const float fskill = 1.f / (float)E;
    const float fpair = (E > 1) ? -((float)E - 1.f + alpha) / ((float)E * (float)E * (float)(E - 1)) : 0.f;
    float acc = 0.f;
    for (int i = threadIdx.x; i < K; i += ENT) {
        float v;
        if (Cout == 1 && C > 1) {
            v = 0.f;
            for (int c = 0; c < C; ++c) v += sums[((long long)b * C + c) * K + i];
        } else {
            v = sums[((long long)b * C + co) * K + i];
        }
        const float k = expf(-0.5f * v * v / sigma);
        const float fac = (i < E) ? fskill : fpair;
        acc += fac * k;
        table[((long long)b * Cout + co) * K + i] = -fac * k * v / sigma;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = ENT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[blockIdx.x] = red[0];
}

// ---- stage 3 -------------------------------------------------------------------------------------------------------------
// grid: (chunks, S, planes * ntile).  A block owns the members [a0, a0 + EM) of its points and walks every tile for the partners.
template <typename T, int PM, int EM>
__global__ __launch_bounds__(ENT) void escore_grad_kernel(const T* __restrict__ f, const typename Val<T>::O* __restrict__ obs,
                                                          const float* __restrict__ q, const float* __restrict__ w,
                                                          const float* __restrict__ table, const float* __restrict__ gout,
                                                          T* __restrict__ gf, int E, int C, int Cout, long long seglen, int ntile,
                                                          int nanmode, float p) {
    typedef typename Val<T>::V V;
    const int plane = blockIdx.z / ntile, ta = blockIdx.z % ntile, b = plane / C, c = plane % C;
    const int co = (Cout == 1) ? 0 : c;
    const int S = gridDim.y, s = blockIdx.y;
    const long long N = seglen * S, estride = (long long)C * N;
    const long long foff = ((long long)b * E * C + c) * N + (long long)s * seglen;
    const long long poff = (long long)plane * N + (long long)s * seglen;
    const int K = E + E * (E - 1) / 2;
    const float* __restrict__ tab = table + (((long long)b * Cout + co) * S + s) * K;
    const float go = gout[b * Cout + co];
    const int a0 = ta * EM, na = min(EM, E - a0);
    const T* fa = f + foff + a0 * estride;
    const float* qp = q + (long long)s * seglen;
    for (long long n = (long long)blockIdx.x * ENT + threadIdx.x; n < seglen; n += (long long)gridDim.x * ENT) {
        V o = obs[poff + n];
        bool masked = isnan_v(o);
        if (masked) o = zero_of(V());
        bool bad = false;
        V va[EM], g[EM];
        bool nan_a[EM];
#pragma unroll
        for (int i = 0; i < EM; ++i) {
            va[i] = (i < na) ? Val<T>::ld(fa + i * estride + n) : zero_of(V());
            nan_a[i] = isnan_v(va[i]);
            if (nan_a[i]) va[i] = zero_of(V());
            g[i] = zero_of(V());
            if (i < na) grad_p<PM>(g[i], tab[a0 + i], va[i], o, p);
        }
        for (int tb = 0; tb < ntile; ++tb) {
            const int b0 = tb * EM, nb = min(EM, E - b0);
            const T* fb = f + foff + b0 * estride;
#pragma unroll
            for (int j = 0; j < EM; ++j) {
                V vb = (j < nb) ? Val<T>::ld(fb + j * estride + n) : zero_of(V());
                if (isnan_v(vb)) {
                    bad = true;
                    vb = zero_of(V());
                }
#pragma unroll
                for (int i = 0; i < EM; ++i) {
                    const int gi = a0 + i, gj = b0 + j;
                    if (i < na && j < nb && gi != gj)
                        grad_p<PM>(g[i], tab[pair_index(min(gi, gj), max(gi, gj), E)], va[i], vb, p);
                }
            }
        }
        if (nanmode == 1) masked = masked || bad;
        const float wt = masked ? 0.f : go * qp[n] * (w ? w[poff + n] : 1.f);
#pragma unroll
        for (int i = 0; i < EM; ++i) {
            if (i < na) {
                V r = g[i];
                const float m = nan_a[i] ? 0.f : wt;          // an imputed member receives nothing
                if constexpr (sizeof(V) == sizeof(float2)) {
                    r.x *= m;
                    r.y *= m;
                } else {
                    r *= m;
                }
                Val<T>::st(gf + foff + (a0 + i) * estride + n, r);
            }
        }
    }
}

// the smallest instantiated tile that holds E members; more than one tile: always tiles of 8
int tile_of(int E) { return E <= 2 ? 2 : (E <= 4 ? 4 : ETILE); }

template <typename T, int PM>
int launch_sums(const T* f, const typename Val<T>::O* obs, const float* q, const float* w, float* out, int E, int C, long long seglen,
                int nanmode, float p, dim3 grid, int ntile, hipStream_t s) {
    return mk_with_capacity<ETILE>(tile_of(E), "escore_sums", [&](auto em) {
        hipLaunchKernelGGL((escore_sums_kernel<T, PM, em()>), grid, dim3(ENT), 0, s, f, obs, q, w, out, E, C, seglen, ntile, nanmode, p);
        return mk_check_launch("mk_escore_sums");
    });
}

template <typename T, int PM>
int launch_grad(const T* f, const typename Val<T>::O* obs, const float* q, const float* w, const float* table, const float* gout, T* gf,
                int E, int C, int Cout, long long seglen, int nanmode, float p, dim3 grid, int ntile, hipStream_t s) {
    return mk_with_capacity<ETILE>(tile_of(E), "escore_grad", [&](auto em) {
        hipLaunchKernelGGL((escore_grad_kernel<T, PM, em()>), grid, dim3(ENT), 0, s, f, obs, q, w, table, gout, gf, E, C, Cout, seglen, ntile,
                           nanmode, p);
        return mk_check_launch("mk_escore_grad");
    });
}

int pmode_of(float p) { return p == 2.f ? P_TWO : (p == 1.f ? P_ONE : P_ANY); }

bool common_args_ok(int kind, int B, int E, int C, long long N, int S, float p) {
    return kind >= 0 && kind <= 2 && B > 0 && E >= 1 && E <= EMAX && C > 0 && N > 0 && S > 0 && S <= 65535 && N % S == 0 &&
           (kind == 2 ? p == 2.f : p >= 1.f);
}

}  // namespace

extern "C" long long mk_escore_sums_workspace(int B, int E, int C, long long N, int S, int nanmode) {
    if (B <= 0 || E <= 0 || C <= 0 || N <= 0 || S <= 0) return 0;
    const int chunks = mk_plane_chunks(N / S);
    const long long K = E + (long long)E * (E - 1) / 2;
    long long ws = chunks > 1 ? (long long)B * C * S * chunks * K : 0;
    if (nanmode == 1 && E > ETILE) ws += (long long)B * C * N;
    return ws;
}

extern "C" int mk_escore_sums(const void* f, int kind, const void* obs, const float* q, const float* w, float* sums, float* ws, int B, int E,
                              int C, long long N, int S, int nanmode, float p, void* stream) {
    MK_REQUIRE(f && obs && q && sums && common_args_ok(kind, B, E, C, N, S, p),
               "escore_sums: bad arguments (1 <= E <= 32, p >= 1, complex members p = 2, N a multiple of S)");
    MK_REQUIRE(nanmode == 0 || nanmode == 1, "escore_sums: unknown NaN mode %d", nanmode);
    const long long seglen = N / S;
    const int chunks = mk_plane_chunks(seglen), EM = tile_of(E), ntile = (E + EM - 1) / EM, npairs = ntile * (ntile + 1) / 2;
    const int K = E + E * (E - 1) / 2;
    MK_REQUIRE((long long)B * C * npairs <= 65535, "escore_sums: too many planes");
    MK_REQUIRE(ws || mk_escore_sums_workspace(B, E, C, N, S, nanmode) == 0, "escore_sums: missing workspace");
    hipStream_t s = (hipStream_t)stream;
    float* partial = chunks > 1 ? ws : sums;
    float* wm = chunks > 1 ? ws + (long long)B * C * S * chunks * K : ws;
    const dim3 grid((unsigned)chunks, (unsigned)S, (unsigned)(B * C * npairs));
    const dim3 mgrid((unsigned)mk_plane_chunks(N), (unsigned)(B * C));
    const bool premask = nanmode == 1 && ntile > 1;
    int rc;
#define MK_ES_MASK(T)                                                                                                                 \
    if (premask) {                                                                                                                    \
        hipLaunchKernelGGL((escore_mask_weights<T>), mgrid, dim3(ENT), 0, s, (const T*)f, (const Val<T>::O*)obs, w, wm, E, C, N);     \
        rc = mk_check_launch("mk_escore_sums");                                                                                       \
        if (rc) return rc;                                                                                                            \
        w = wm;                                                                                                                       \
    }
    if (kind == 2) {
        MK_ES_MASK(float2)
        rc = launch_sums<float2, P_TWO>((const float2*)f, (const float2*)obs, q, w, partial, E, C, seglen, nanmode, p, grid, ntile, s);
    } else if (kind == MK_F32) {
        MK_ES_MASK(float)
        const int pm = pmode_of(p);
        rc = pm == P_TWO   ? launch_sums<float, P_TWO>((const float*)f, (const float*)obs, q, w, partial, E, C, seglen, nanmode, p, grid, ntile, s)
             : pm == P_ONE ? launch_sums<float, P_ONE>((const float*)f, (const float*)obs, q, w, partial, E, C, seglen, nanmode, p, grid, ntile, s)
                           : launch_sums<float, P_ANY>((const float*)f, (const float*)obs, q, w, partial, E, C, seglen, nanmode, p, grid, ntile, s);
    } else {
        MK_ES_MASK(u16)
        const int pm = pmode_of(p);
        rc = pm == P_TWO   ? launch_sums<u16, P_TWO>((const u16*)f, (const float*)obs, q, w, partial, E, C, seglen, nanmode, p, grid, ntile, s)
             : pm == P_ONE ? launch_sums<u16, P_ONE>((const u16*)f, (const float*)obs, q, w, partial, E, C, seglen, nanmode, p, grid, ntile, s)
                           : launch_sums<u16, P_ANY>((const u16*)f, (const float*)obs, q, w, partial, E, C, seglen, nanmode, p, grid, ntile, s);
    }
#undef MK_ES_MASK
    if (rc || chunks == 1) return rc;
    const long long rows = (long long)B * C * S;
    hipLaunchKernelGGL(escore_combine, dim3((unsigned)((rows * K + ENT - 1) / ENT)), dim3(ENT), 0, s, partial, sums, rows, chunks, K);
    return mk_check_launch("mk_escore_sums");
}

extern "C" int mk_escore_finish(const float* sums, const float* scale, int nscale, float* loss, float* table, int B, int E, int C, int S,
                                int reduce, float p, float beta, float alpha, float eps, void* stream) {
    MK_REQUIRE(sums && loss && table && B > 0 && E >= 1 && E <= EMAX && C > 0 && S > 0 && p >= 1.f,
               "escore_finish: bad arguments (1 <= E <= 32, p >= 1)");
    const int Cout = reduce ? 1 : C;
    MK_REQUIRE(!scale || nscale == 1 || nscale == Cout, "escore_finish: the spread scale holds %d entries for %d output channels", nscale, Cout);
    hipLaunchKernelGGL(escore_finish_kernel, dim3((unsigned)(B * Cout)), dim3(ENT), 0, (hipStream_t)stream, sums, scale, nscale, loss, table, C,
                       Cout, S, E, p, beta, alpha, eps);
    return mk_check_launch("mk_escore_finish");
}

extern "C" int mk_mmd_finish(const float* sums, float* loss, float* table, int B, int E, int C, int reduce, float sigma, float alpha,
                             void* stream) {
    MK_REQUIRE(sums && loss && table && B > 0 && E >= 1 && E <= EMAX && C > 0 && sigma > 0.f,
               "mmd_finish: bad arguments (1 <= E <= 32, sigma > 0)");
    const int Cout = reduce ? 1 : C;
    hipLaunchKernelGGL(mmd_finish_kernel, dim3((unsigned)(B * Cout)), dim3(ENT), 0, (hipStream_t)stream, sums, loss, table, C, Cout, E, sigma,
                       alpha);
    return mk_check_launch("mk_mmd_finish");
}

extern "C" int mk_escore_grad(const void* f, int kind, const void* obs, const float* q, const float* w, const float* table, const float* gout,
                              void* gf, int B, int E, int C, int Cout, long long N, int S, int nanmode, float p, void* stream) {
    MK_REQUIRE(f && obs && q && table && gout && gf && common_args_ok(kind, B, E, C, N, S, p) && (Cout == 1 || Cout == C),
               "escore_grad: bad arguments (1 <= E <= 32, p >= 1, complex members p = 2, N a multiple of S, Cout 1 or C)");
    MK_REQUIRE(nanmode == 0 || nanmode == 1, "escore_grad: unknown NaN mode %d", nanmode);
    const long long seglen = N / S;
    const int EM = tile_of(E), ntile = (E + EM - 1) / EM;
    MK_REQUIRE((long long)B * C * ntile <= 65535, "escore_grad: too many planes");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)mk_plane_chunks(seglen), (unsigned)S, (unsigned)(B * C * ntile));
    if (kind == 2)
        return launch_grad<float2, P_TWO>((const float2*)f, (const float2*)obs, q, w, table, gout, (float2*)gf, E, C, Cout, seglen, nanmode, p, grid,
                                          ntile, s);
    const int pm = pmode_of(p);
#define MK_ES_GRAD(T, PMV) \
    launch_grad<T, PMV>((const T*)f, (const float*)obs, q, w, table, gout, (T*)gf, E, C, Cout, seglen, nanmode, p, grid, ntile, s)
    if (kind == MK_F32) return pm == P_TWO ? MK_ES_GRAD(float, P_TWO) : (pm == P_ONE ? MK_ES_GRAD(float, P_ONE) : MK_ES_GRAD(float, P_ANY));
    return pm == P_TWO ? MK_ES_GRAD(u16, P_TWO) : (pm == P_ONE ? MK_ES_GRAD(u16, P_ONE) : MK_ES_GRAD(u16, P_ANY));
#undef MK_ES_GRAD
}
