// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (see escore.hip: the SLP vectoriser's packed-fp32 forms are kept out of this library; tests/test_packed_forms.py scans the ISA)
// Per-degree ensemble Gram matrix in spectral space: what SpectralCoherenceLoss (makani/utils/losses/energy_score.py:655-856),
// CoherenceRegularization and SpectralRegularization (makani/utils/losses/regularization.py:84-417) are finishes of.  amse.hip
// generalised from 2 fields to E + 1.
//
//   members f[b][e][c][l][m] (B, E, C, L, M) complex64 (re, im interleaved): the raw output of RealSHT, read in place
//   observation o[b][c][l][m] complex64; weights q[l][m] f32 (the host folds 1 / 4 pi, the factor 2 of m > 0 and the zeros of m > l in)
//   fields x_0 .. x_{E-1} = members, x_E = observation, n = E + 1
//
// mk_egram_sums: G[b][c][l][slot] = sum_m q[l][m] Re(conj(x_i[l][m]) x_j[l][m]); the slots of a row (B, C, L, K):
//     [0, n)                      G[i][i], i = 0 .. E                       (power spectral densities)
//     [n, n + E)                  G[e][E], e < E                            (member - observation cross spectra)
//     [n + E, n + E + E (E-1)/2)  G[i][j], i < j < E, lexicographic         (member - member cross spectra; pair_index of escore.hip)
//   `what` truncates the row: MK_EGRAM_DIAG K = n, MK_EGRAM_OBS K = n + E, MK_EGRAM_FULL everything.
//   Orders m > l + tri_off are not read (the caller guarantees q = 0 there; tri_off >= M: nothing is skipped).
//   One wave owns one (b, c, l) row and walks its orders 64 at a time (coalesced float2 loads); no LDS, no atomics, no workspace.
//   The fields are cut into tiles of 8 and grid dimension y walks the tiles:
//     FULL  tile pairs (ta <= tb) of the T = ceil(n / 8) tiles: a diagonal wave holds 8 + 28 sums, an off-diagonal one 64.  n <= 8
//           is ONE tile: every coefficient is read once.  Larger ensembles RE-READ tiles: T (T + 1) / 2 waves per row, the T diagonal
//           ones read one tile and the others two, T^2 tile reads in all — T times the single-pass traffic (E = 16: 3x, E = 32: 5x).
//     DIAG  the T tiles, diagonal only: every coefficient is read once for every E.
//     OBS   the ceil(E / 8) member tiles, each with the observation beside it: every member coefficient is read once for every E, the
//           observation once per member tile.
//   Every slot is written by exactly one wave.  A sum is the lane's partial sum over its orders m = lane, lane + 64, ... in
//   increasing m, then the __shfl_down ladder 32, 16, 8, 4, 2, 1: a fixed order, bit-identical from run to run.
//   No NaN masking: a NaN coefficient makes the sums of its degree NaN, as in the three reference classes.
// mk_egram_grad: dG (B, C, L, K) -> gf (B, E, C, L, M) complex64, torch's complex-gradient convention (d |z|^2 = 2 z):
//     gf_e[l][m] = q[l][m] (2 dG[e][e] x_e + dG[e][E] x_E + sum_{j != e, j < E} dG[e, j] x_j)           (slots beyond K count as 0)
//   exact zeros at the skipped orders (gf needs no memset); the observation gets no gradient.  One wave owns a row and a tile of 8
//   members and walks all other fields for the partners: E <= 8 reads everything once, larger ensembles read the members
//   ceil(E / 8) times (FULL; DIAG and OBS read them once).  The dG row is uniform over the wave: lane j loads the coefficient of
//   partner j once per own member (8 loads per wave), v_readlane broadcasts it into a scalar register where it is used.
#include <algorithm>

#include "common.h"

namespace {

constexpr int GNT = 256;        // threads per block: four rows
constexpr int GTILE = 8;        // fields per tile
constexpr int GEMAX = 32;

// slot of G[i][j], i <= j <= E, in a row
__device__ __forceinline__ int gram_slot(int i, int j, int E) {
    if (i == j) return i;
    if (j == E) return E + 1 + i;
    return 2 * E + 1 + i * (2 * E - i - 1) / 2 + (j - i - 1);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// field i of a row: member i < E, else the observation
__device__ __forceinline__ const float2* field_ptr(const float2* fm, const float2* ob, long long es, int i, int E) {
    return i < E ? fm + (long long)i * es : ob;
}

struct RowCtx {
    const float2* fm;       // member 0 of this row; member e at fm + e * es
    const float2* ob;       // the observation's row
    const float* qr;        // the weights' row
    long long es;
    int lane, mend, E;
};

// One wave: the A fields a0 .. a0 + 7 (those below alim count; the others are read from a clamped, valid field and never
// written) against themselves (DG: diagonal, PR: the pairs inside the tile) and against NBF B fields b0 .. (below n); BD: the
// diagonal of B field 0 as well.
template <bool DG, bool PR, int NBF, bool BD>
__device__ __forceinline__ void sums_body(const RowCtx& r, float* __restrict__ out, int a0, int alim, int b0, bool write_bd) {
    constexpr int NB = NBF > 0 ? NBF : 1;
    const int E = r.E, n = E + 1;
    const float2* pa[GTILE];
    const float2* pb[NB];
#pragma unroll
    for (int i = 0; i < GTILE; ++i) pa[i] = field_ptr(r.fm, r.ob, r.es, min(a0 + i, alim - 1), E);
#pragma unroll
    for (int j = 0; j < NB; ++j) pb[j] = field_ptr(r.fm, r.ob, r.es, min(b0 + j, n - 1), E);
    float dg[GTILE], pr[GTILE][GTILE], cr[GTILE][NB], bd = 0.f;
#pragma unroll
    for (int i = 0; i < GTILE; ++i) {
        dg[i] = 0.f;
#pragma unroll
        for (int j = 0; j < GTILE; ++j) pr[i][j] = 0.f;
#pragma unroll
        for (int j = 0; j < NB; ++j) cr[i][j] = 0.f;
    }
    for (int m = r.lane; m < r.mend; m += 64) {
        const float qm = r.qr[m];
        float2 xa[GTILE], wa[GTILE], xb[NB];
#pragma unroll
        for (int i = 0; i < GTILE; ++i) xa[i] = pa[i][m];
        if (NBF > 0) {
#pragma unroll
            for (int j = 0; j < NB; ++j) xb[j] = pb[j][m];
        }
#pragma unroll
        for (int i = 0; i < GTILE; ++i) wa[i] = make_float2(qm * xa[i].x, qm * xa[i].y);
#pragma unroll
        for (int i = 0; i < GTILE; ++i) {
            if (DG) dg[i] += wa[i].x * xa[i].x + wa[i].y * xa[i].y;
            if (PR) {
#pragma unroll
                for (int j = i + 1; j < GTILE; ++j) pr[i][j] += wa[i].x * xa[j].x + wa[i].y * xa[j].y;
            }
            if (NBF > 0) {
#pragma unroll
                for (int j = 0; j < NB; ++j) cr[i][j] += wa[i].x * xb[j].x + wa[i].y * xb[j].y;
            }
        }
        if (BD) bd += qm * (xb[0].x * xb[0].x + xb[0].y * xb[0].y);
    }
    const bool first = r.lane == 0;
#pragma unroll
    for (int i = 0; i < GTILE; ++i) {
        const int gi = a0 + i;
        const bool iok = gi < alim;          // (wave-uniform)
        if (DG) {
            const float s = wave_sum(dg[i]);
            if (first && iok) out[gi] = s;
        }
        if (PR) {
#pragma unroll
            for (int j = i + 1; j < GTILE; ++j) {
                const float s = wave_sum(pr[i][j]);
                if (first && a0 + j < alim) out[gram_slot(gi, a0 + j, E)] = s;
            }
        }
        if (NBF > 0) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const float s = wave_sum(cr[i][j]);
                if (first && iok && b0 + j < n) out[gram_slot(gi, b0 + j, E)] = s;
            }
        }
    }
    if (BD) {
        const float s = wave_sum(bd);
        if (first && write_bd) out[b0] = s;
    }
}

template <int WHAT>
__global__ __launch_bounds__(GNT) void egram_sums_kernel(const float2* __restrict__ f, const float2* __restrict__ o, const float* __restrict__ q,
                                                         float* __restrict__ G, long long rows, int E, int C, int L, int M, int K, int tri_off,
                                                         int T) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long row = (long long)blockIdx.x * (GNT / 64) + wave;
    if (row >= rows) return;                         // (wave-uniform; the kernel has no block barrier)
    const int l = (int)(row % L);
    const long long bc = row / L;
    const int c = (int)(bc % C);
    const long long b = bc / C;
    const long long plane = (long long)L * M;
    RowCtx r;
    r.lane = threadIdx.x & 63;
    r.E = E;
    r.es = (long long)C * plane;
    r.fm = f + (b * E * C + c) * plane + (long long)l * M;
    r.ob = o + row * M;
    r.qr = q + (long long)l * M;
    r.mend = max(0, min(M, l + tri_off + 1));
    float* out = G + row * K;
    const int n = E + 1;
    if (WHAT == MK_EGRAM_DIAG) {
        sums_body<true, false, 0, false>(r, out, (int)blockIdx.y * GTILE, n, 0, false);
    } else if (WHAT == MK_EGRAM_OBS) {
        sums_body<true, false, 1, true>(r, out, (int)blockIdx.y * GTILE, E, E, blockIdx.y == 0);
    } else {
        int ta = 0, tb = (int)blockIdx.y;            // pair index -> (ta <= tb), row ta of the upper triangle holds T - ta pairs
        while (tb >= T - ta) {
            tb -= T - ta;
            ++ta;
        }
        tb += ta;
        if (ta == tb)
            sums_body<true, true, 0, false>(r, out, ta * GTILE, n, 0, false);
        else
            sums_body<false, false, GTILE, false>(r, out, ta * GTILE, n, tb * GTILE, false);
    }
}

__device__ __forceinline__ float lane_value(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

template <int WHAT>
__global__ __launch_bounds__(GNT) void egram_grad_kernel(const float2* __restrict__ f, const float2* __restrict__ o, const float* __restrict__ q,
                                                         const float* __restrict__ dG, float2* __restrict__ gf, long long rows, int E, int C,
                                                         int L, int M, int K, int tri_off) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long row = (long long)blockIdx.x * (GNT / 64) + wave;
    if (row >= rows) return;                         // (wave-uniform)
    const int l = (int)(row % L);
    const long long bc = row / L;
    const int c = (int)(bc % C);
    const long long b = bc / C;
    const long long plane = (long long)L * M, es = (long long)C * plane;
    const long long moff = (b * E * C + c) * plane + (long long)l * M;
    const float2* fm = f + moff;
    float2* gm = gf + moff;
    const float2* ob = o + row * M;
    const float* qr = q + (long long)l * M;
    const float* dgr = dG + row * K;
    const int mend = max(0, min(M, l + tri_off + 1));
    const int n = E + 1, a0 = (int)blockIdx.y * GTILE, na = min(GTILE, E - a0);
    // lane j < n: the coefficient of partner field j in the gradient of own member a0 + i (twice the diagonal; 0 beyond K)
    float cf[GTILE];
#pragma unroll
    for (int i = 0; i < GTILE; ++i) {
        const int gi = a0 + i;
        float v = 0.f;
        if (gi < E && lane < n) {
            const int s = gram_slot(min(gi, lane), max(gi, lane), E);
            if (s < K) v = dgr[s];
            if (lane == gi) v *= 2.f;
        }
        cf[i] = v;
    }
    const float2* pa[GTILE];
#pragma unroll
    for (int i = 0; i < GTILE; ++i) pa[i] = fm + (long long)min(a0 + i, E - 1) * es;
    const float2 zero = make_float2(0.f, 0.f);
    for (int m0 = 0; m0 < M; m0 += 64) {             // (every wave-level operation below runs with the trip count of the wave)
        const int m = m0 + lane;
        if (m0 >= mend) {
            if (m < M) {
#pragma unroll
                for (int i = 0; i < GTILE; ++i)
                    if (i < na) gm[(long long)(a0 + i) * es + m] = zero;
            }
            continue;
        }
        const int mc = min(m, mend - 1);             // lanes beyond the row's end read its last order and store zeros / nothing
        const float qm = qr[mc];
        float2 xa[GTILE], acc[GTILE];
#pragma unroll
        for (int i = 0; i < GTILE; ++i) xa[i] = pa[i][mc];
#pragma unroll
        for (int i = 0; i < GTILE; ++i) {
            if (WHAT == MK_EGRAM_FULL) {
                acc[i] = zero;
#pragma unroll
                for (int j = 0; j < GTILE; ++j) {    // (beyond E the tile holds no partner: lane E carries the observation's coefficient)
                    const float cc = a0 + j < E ? lane_value(cf[i], a0 + j) : 0.f;
                    acc[i].x += cc * xa[j].x;
                    acc[i].y += cc * xa[j].y;
                }
            } else {
                const float cc = lane_value(cf[i], a0 + i);
                acc[i] = make_float2(cc * xa[i].x, cc * xa[i].y);
            }
        }
        if (WHAT != MK_EGRAM_DIAG) {
            const float2 xo = ob[mc];
#pragma unroll
            for (int i = 0; i < GTILE; ++i) {
                const float cc = lane_value(cf[i], E);
                acc[i].x += cc * xo.x;
                acc[i].y += cc * xo.y;
            }
        }
        if (WHAT == MK_EGRAM_FULL) {
            for (int j = 0; j < E; ++j) {
                if (j >= a0 && j < a0 + GTILE) continue;          // (wave-uniform; the own tile is in registers)
                const float2 xj = fm[(long long)j * es + mc];
#pragma unroll
                for (int i = 0; i < GTILE; ++i) {
                    const float cc = lane_value(cf[i], j);
                    acc[i].x += cc * xj.x;
                    acc[i].y += cc * xj.y;
                }
            }
        }
        if (m < M) {
            const bool live = m < mend;
#pragma unroll
            for (int i = 0; i < GTILE; ++i)
                if (i < na) gm[(long long)(a0 + i) * es + m] = live ? make_float2(qm * acc[i].x, qm * acc[i].y) : zero;
        }
    }
}

int egram_slots(int E, int what) {
    const int n = E + 1;
    return what == MK_EGRAM_DIAG ? n : (what == MK_EGRAM_OBS ? n + E : n + E + E * (E - 1) / 2);
}

// 0, or the error code; the triangle offset clamped to where it cannot overflow l + tri_off + 1
int egram_args(const char* who, const void* f, const void* o, const void* q, const void* g, int B, int E, int C, int L, int M, int what,
               int* tri_off) {
    MK_REQUIRE(f && o && q && g && B > 0 && E > 0 && C > 0 && L > 0 && M > 0, "%s: bad arguments", who);
    MK_REQUIRE(what == MK_EGRAM_DIAG || what == MK_EGRAM_OBS || what == MK_EGRAM_FULL, "%s: what = %d", who, what);
    MK_REQUIRE(((long long)B * C * L + GNT / 64 - 1) / (GNT / 64) < (1ll << 31), "%s: too many rows", who);
    if (E > GEMAX) {
        mk_set_error("%s: ensemble size %d (at most %d members)", who, E, GEMAX);
        return MK_EUNSUP;
    }
    *tri_off = std::max(-(L + 1), std::min(M, *tri_off));
    return 0;
}

}  // namespace

extern "C" int mk_egram_sums(const void* f, const void* o, const float* q, float* G, int B, int E, int C, int L, int M, int what, int tri_off,
                             void* stream) {
    if (const int rc = egram_args("egram_sums", f, o, q, G, B, E, C, L, M, what, &tri_off)) return rc;
    const long long rows = (long long)B * C * L;
    const int n = E + 1, T = (n + GTILE - 1) / GTILE, K = egram_slots(E, what);
    const unsigned gx = (unsigned)((rows + GNT / 64 - 1) / (GNT / 64));
#define MK_EGRAM_LAUNCH(W, GY)                                                                                                        \
    hipLaunchKernelGGL((egram_sums_kernel<W>), dim3(gx, (unsigned)(GY)), dim3(GNT), 0, (hipStream_t)stream, (const float2*)f, (const float2*)o, \
                       q, G, rows, E, C, L, M, K, tri_off, T)
    if (what == MK_EGRAM_DIAG)
        MK_EGRAM_LAUNCH(MK_EGRAM_DIAG, T);
    else if (what == MK_EGRAM_OBS)
        MK_EGRAM_LAUNCH(MK_EGRAM_OBS, (E + GTILE - 1) / GTILE);
    else
        MK_EGRAM_LAUNCH(MK_EGRAM_FULL, T * (T + 1) / 2);
#undef MK_EGRAM_LAUNCH
    return mk_check_launch("mk_egram_sums");
}

extern "C" int mk_egram_grad(const void* f, const void* o, const float* q, const float* dG, void* gf, int B, int E, int C, int L, int M,
                             int what, int tri_off, void* stream) {
    if (const int rc = egram_args("egram_grad", f, o, q, dG, B, E, C, L, M, what, &tri_off)) return rc;
    MK_REQUIRE(gf, "egram_grad: bad arguments");
    const long long rows = (long long)B * C * L;
    const int K = egram_slots(E, what);
    const dim3 grid((unsigned)((rows + GNT / 64 - 1) / (GNT / 64)), (unsigned)((E + GTILE - 1) / GTILE));
#define MK_EGRAM_LAUNCH(W)                                                                                                            \
    hipLaunchKernelGGL((egram_grad_kernel<W>), grid, dim3(GNT), 0, (hipStream_t)stream, (const float2*)f, (const float2*)o, q, dG, (float2*)gf, \
                       rows, E, C, L, M, K, tri_off)
    if (what == MK_EGRAM_DIAG)
        MK_EGRAM_LAUNCH(MK_EGRAM_DIAG);
    else if (what == MK_EGRAM_OBS)
        MK_EGRAM_LAUNCH(MK_EGRAM_OBS);
    else
        MK_EGRAM_LAUNCH(MK_EGRAM_FULL);
#undef MK_EGRAM_LAUNCH
    return mk_check_launch("mk_egram_grad");
}
