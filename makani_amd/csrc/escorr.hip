// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (as escore.hip: no packed-fp32 forms from the SLP vectoriser; tests/test_packed_forms.py scans the built library)
// The corrected per-degree spectral L2 energy score (gfx950): CorrectedSpectralL2EnergyScoreLoss of
// makani/utils/losses/energy_score.py:859-1042, the per-degree energy score whose spread term is scaled by the ratio of the
// truth's power spectrum to the ensemble's, P_true / (P_pred + eps).  Three stages on ROW-RESIDENT kernels.
//
//   members f[b][e][c][l][m] (B, E, C, L, M) complex64 (re, im interleaved), observation o[b][c][l][m], weights q[l][m] f32
//   a row is the M coefficients of one (b, c, l) of one field; a block owns the E + 1 rows of one (b, c, l)
//   K' = E + E (E - 1) / 2 + E + 1 sums per (b, c, l):  [0, E) skill_e, [E, E + P) spread_ij (i < j, lexicographic),
//   [E + P, E + P + E) pow_e, [K' - 1] pow_o
//
// Stage 1, mk_escorr_sums.  The block walks its row in chunks of MC = 128 orders.  A chunk of the E + 1 rows goes from HBM to
//   LDS once (float2 loads coalesced along m; thread t stages column t % MC of the rows t / MC, t / MC + 2, ..), NaN -> 0 on the
//   way, with the rows wq[m] = q[m] * !(observation or ANY member NaN at m) and q[m] beside them.  Then a lane owns ONE SUM and
//   one slice of the orders: item t -> (k = t % K', slice = t / K'), slices interleaved (m = slice, slice + NS, ..), NS =
//   max(1, 256 / K') — E = 2 has six sums and 42 slices, so small ensembles fill the block too; K' > 256 (E >= 22) gives a lane
//   up to three sums.  Every sum has ONE form, w[m] |A[m] - s B[m]|^2: a distance (s = 1, w = wq), or a power (s = 0, B = A,
//   w = q: the reference's spectra are NOT masked, a NaN member just counts as 0, energy_score.py:964-974).  The differences are
//   formed directly in fp32, never as a Gram form (escore.hip says why).  The accumulator stays in its register across the
//   chunks; at the end the slices of a sum are added through LDS in slice order and the block writes its K' sums.  Every
//   coefficient is read from HBM once for every E <= 32; there is no mask pre-pass, no partial sums, no combine, no workspace.
//   LDS: rows of 2 MC + 2 dwords, so row e starts at dword 2 e (mod 32): the lanes of a wave, which read different members at
//   the same m, hit different banks (E = 32: 64 dwords over 32 banks, the two-per-bank minimum of a 64-bit read of 32 lanes).
//   (E + 1) 1 032 B of rows, 34 056 B at E = 32, plus 5 - 6 KB of weights, flags, slice sums and the gradient's table.
// Stage 2, mk_escorr_finish.  One wave per (b, c_out, l): channel sums in channel order, the `< eps` mask on the distances, the
//   root ^(beta / 2), eskill = mean_e, espread = 2 sum_{i<j} (E - 1 + alpha) / (E^2 (E - 1)) (exactly 0 for E = 1), P_pred =
//   mean_e pow_e, ratio = pow_o / (P_pred + eps), the degree's loss eskill - espread ratio / 2, and the table d loss / d (every
//   sum) with d loss / d P_pred in column K'.  A second kernel adds the degrees of a (b, c_out) in l order.
// Stage 3, mk_escorr_grad.  The same staging; then a lane owns an ORDER m (consecutive float2 of a row: conflict-free) and
//   walks the members, four of its own at a time in registers against every partner from LDS; the row's table sits in LDS as a
//   symmetric E x E matrix with a zero diagonal, already times 2 gout.
//   gf_e[m] = gout { wq[m] [T_skill,e 2 (f_e - o) + sum_j T_pair(e,j) 2 (f_e - f_j)] + q[m] T_P (2 / E) f_e }
//   (torch's convention d |z|^2 = 2 z; a NaN member was imputed to 0 and sits at a masked order: its gradient is 0).
// No floating-point atomics; repeats are bit-identical.
#include "block_io.h"

namespace {

constexpr int NT = 256;                 // threads per block
constexpr int MC = 128;                 // orders per chunk
constexpr int NG = NT / MC;             // staging / gradient groups: rows g, g + NG, ..
constexpr int EMAX = 32;
constexpr int RS = 2 * MC + 2;          // dwords per LDS row
constexpr int RPT = (EMAX + 1 + NG - 1) / NG;          // rows a thread stages (17)
constexpr int KMAX = EMAX + EMAX * (EMAX - 1) / 2 + EMAX + 1;          // 561
constexpr int IPT = (KMAX + NT - 1) / NT;          // sums a lane owns at most (3)
constexpr int OWN = 4;                  // own members a gradient lane keeps in registers

__host__ __device__ __forceinline__ int nsums(int E) { return E + E * (E - 1) / 2 + E + 1; }
__host__ __device__ __forceinline__ size_t rows_bytes(int E) { return (size_t)(E + 1) * RS * sizeof(float); }

__device__ __forceinline__ int pair_index(int i, int j, int E) { return E + i * (2 * E - i - 1) / 2 + (j - i - 1); }

// One chunk of the E + 1 rows (members, then the observation) of the block's (b, c, l) into LDS, NaN -> 0, with wq and qs.
// fp: member 0's row, estride: floats2 between members, op: the observation's row, qp: the weights' row; n orders from m0.
// Barriers: one in front (the previous chunk's readers), one behind.
__device__ __forceinline__ void stage_chunk(const float2* __restrict__ fp, long long estride, const float2* __restrict__ op,
                                            const float* __restrict__ qp, int E, int m0, int n, float* rows, float* wq, float* qs,
                                            int* flag) {
    const int m = threadIdx.x % MC, g = threadIdx.x / MC;
    float2 v[RPT];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
        const int r = g + NG * u;
        v[u] = make_float2(0.f, 0.f);
        if (r <= E && m < n) v[u] = (r < E) ? fp[(long long)r * estride + m0 + m] : op[m0 + m];
    }
    bool bad = false;
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
        const int r = g + NG * u;
        if (r <= E) {
            if (v[u].x != v[u].x || v[u].y != v[u].y) {
                bad = true;
                v[u] = make_float2(0.f, 0.f);
            }
            *reinterpret_cast<float2*>(rows + r * RS + 2 * m) = v[u];
        }
    }
    flag[g * MC + m] = bad ? 1 : 0;
    __syncthreads();
    if (g == 0) {
        bool any = false;
#pragma unroll
        for (int h = 0; h < NG; ++h) any = any || flag[h * MC + m] != 0;
        const float qv = (m < n) ? qp[m0 + m] : 0.f;
        qs[m] = qv;
        wq[m] = any ? 0.f : qv;
    }
    __syncthreads();
}

// ---- stage 1 -------------------------------------------------------------------------------------------------------------
// grid: B * C * L blocks.  sums (B, C, L, K')
__global__ __launch_bounds__(NT) void escorr_sums_kernel(const float2* __restrict__ f, const float2* __restrict__ obs,
                                                         const float* __restrict__ q, float* __restrict__ sums, int E, int C, int L,
                                                         int M) {
    extern __shared__ float lds[];
    __shared__ float wq[MC], qs[MC], part[IPT * NT];
    __shared__ int flag[NT];
    float* rows = lds;
    const long long row = blockIdx.x;          // (b * C + c) * L + l
    const int l = (int)(row % L), c = (int)((row / L) % C), b = (int)(row / ((long long)L * C));
    const long long estride = (long long)C * L * M;
    const float2* fp = f + (((long long)b * E * C + c) * L + l) * M;
    const float2* op = obs + row * M;
    const float* qp = q + (long long)l * M;
    const int K = nsums(E), P = E * (E - 1) / 2;
    const int NS = (K < NT) ? NT / K : 1, items = K * NS;
    // the lane's sums: w[m] |A[m] - s B[m]|^2
    int ra[IPT], rb[IPT], sl[IPT];
    float sb[IPT], acc[IPT];
    bool unmasked[IPT];
#pragma unroll
    for (int u = 0; u < IPT; ++u) {
        const int it = threadIdx.x + u * NT;
        const int k = it % K;
        sl[u] = (it < items) ? it / K : MC;          // (a slice that starts behind every chunk: no work)
        acc[u] = 0.f;
        if (k < E) {                                  // skill: member k against the observation
            ra[u] = E, rb[u] = k, sb[u] = 1.f, unmasked[u] = false;
        } else if (k < E + P) {
            int i = 0, pi = k - E;
            while (pi >= E - 1 - i) {
                pi -= E - 1 - i;
                ++i;
            }
            ra[u] = i, rb[u] = i + 1 + pi, sb[u] = 1.f, unmasked[u] = false;
        } else {                                      // powers: the members, then the observation (row E)
            ra[u] = rb[u] = k - E - P, sb[u] = 0.f, unmasked[u] = true;
        }
        ra[u] *= RS, rb[u] *= RS;
    }
    for (int m0 = 0; m0 < M; m0 += MC) {
        const int n = min(MC, M - m0);
        stage_chunk(fp, estride, op, qp, E, m0, n, rows, wq, qs, flag);
#pragma unroll
        for (int u = 0; u < IPT; ++u) {
            const float* wrow = unmasked[u] ? qs : wq;
            for (int m = sl[u]; m < n; m += NS) {
                const float2 a = *reinterpret_cast<const float2*>(rows + ra[u] + 2 * m);
                const float2 bb = *reinterpret_cast<const float2*>(rows + rb[u] + 2 * m);
                const float dx = a.x - sb[u] * bb.x, dy = a.y - sb[u] * bb.y;
                acc[u] += wrow[m] * (dx * dx + dy * dy);
            }
        }
    }
    // the slices of a sum, in slice order
#pragma unroll
    for (int u = 0; u < IPT; ++u) {
        const int it = threadIdx.x + u * NT;
        if (it < items) part[it] = acc[u];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += NT) {
        float s = 0.f;
        for (int h = 0; h < NS; ++h) s += part[h * K + k];
        sums[row * K + k] = s;
    }
}

// ---- stage 2 -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);          // every lane ends with the same bits
    return v;
}

// grid: ceil(B * Cout * L / 4) blocks, one wave per (b, co, l).  sums (B, C, L, K') -> lossl (B, Cout, L), table (B, Cout, L, K' + 1)
__global__ __launch_bounds__(NT) void escorr_finish_kernel(const float* __restrict__ sums, float* __restrict__ lossl, float* __restrict__ table,
                                                           long long nrow, int C, int Cout, int L, int E, float beta, float alpha, float eps) {
    constexpr int KPL = (KMAX + 63) / 64;          // sums per lane (9)
    const long long r = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (r >= nrow) return;                         // (whole waves leave; no block barrier below)
    const int lane = threadIdx.x & 63;
    const int l = (int)(r % L), co = (int)((r / L) % Cout), b = (int)(r / ((long long)L * Cout));
    const int K = nsums(E), P = E * (E - 1) / 2;
    const float ex = 0.5f * beta, inv_e = 1.f / (float)E;
    const float cs = (E > 1) ? 2.f * ((float)E - 1.f + alpha) / ((float)E * (float)E * (float)(E - 1)) : 0.f;
    float d[KPL];          // d root / d sum of the lane's distances
    float eskill = 0.f, spread = 0.f, ppred = 0.f, ptrue = 0.f;
#pragma unroll
    for (int u = 0; u < KPL; ++u) {
        const int k = lane + 64 * u;
        d[u] = 0.f;
        if (k < K) {
            float v;
            if (Cout == 1 && C > 1) {
                v = 0.f;
                for (int c = 0; c < C; ++c) v += sums[(((long long)b * C + c) * L + l) * K + k];
            } else {
                v = sums[(((long long)b * C + co) * L + l) * K + k];
            }
            if (k < E + P) {
                const bool masked = v < eps;
                const float rt = masked ? 0.f : ((ex == 0.5f) ? sqrtf(v) : powf(v, ex));
                d[u] = masked ? 0.f : ex * rt / v;
                if (k < E) eskill += rt;
                else spread += rt;
            } else if (k < K - 1) {
                ppred += v;
            } else {
                ptrue = v;
            }
        }
    }
    eskill = wave_sum(eskill) * inv_e;
    const float espread = wave_sum(spread) * cs;
    ppred = wave_sum(ppred) * inv_e;
    ptrue = wave_sum(ptrue);
    const float den = 1.f / (ppred + eps), ratio = ptrue * den;
    const float tp = 0.5f * espread * ptrue * den * den;          // d loss / d P_pred
    float* tab = table + r * (K + 1);
#pragma unroll
    for (int u = 0; u < KPL; ++u) {
        const int k = lane + 64 * u;
        if (k < E) tab[k] = inv_e * d[u];
        else if (k < E + P) tab[k] = -0.5f * ratio * cs * d[u];
        else if (k < K - 1) tab[k] = tp * inv_e;
        else if (k == K - 1) tab[k] = -0.5f * espread * den;
        else if (k == K) tab[k] = tp;
    }
    if (lane == 0) lossl[r] = eskill - 0.5f * espread * ratio;
}

// grid: B * Cout blocks.  loss[b][co] = sum_l lossl[b][co][l], in l order
__global__ __launch_bounds__(NT) void escorr_degrees_kernel(const float* __restrict__ lossl, float* __restrict__ loss, int L) {
    __shared__ float buf[NT];
    float s = 0.f;
    for (int l0 = 0; l0 < L; l0 += NT) {
        const int n = min(NT, L - l0);
        __syncthreads();
        if ((int)threadIdx.x < n) buf[threadIdx.x] = lossl[(long long)blockIdx.x * L + l0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < n; ++i) s += buf[i];
    }
    if (threadIdx.x == 0) loss[blockIdx.x] = s;
}

// ---- stage 3 -------------------------------------------------------------------------------------------------------------
// grid: B * C * L blocks
__global__ __launch_bounds__(NT) void escorr_grad_kernel(const float2* __restrict__ f, const float2* __restrict__ obs,
                                                         const float* __restrict__ q, const float* __restrict__ table,
                                                         const float* __restrict__ gout, float2* __restrict__ gf, int E, int C, int Cout,
                                                         int L, int M) {
    extern __shared__ float lds[];
    __shared__ float wq[MC], qs[MC], t2[EMAX * EMAX], tsk[EMAX];
    __shared__ int flag[NT];
    float* rows = lds;
    const long long row = blockIdx.x;
    const int l = (int)(row % L), c = (int)((row / L) % C), b = (int)(row / ((long long)L * C));
    const int co = (Cout == 1) ? 0 : c;
    const long long estride = (long long)C * L * M;
    const long long foff = (((long long)b * E * C + c) * L + l) * M;
    const float2* fp = f + foff;
    const float2* op = obs + row * M;
    const float* qp = q + (long long)l * M;
    const int K = nsums(E);
    const float* __restrict__ tab = table + (((long long)b * Cout + co) * L + l) * (K + 1);
    const float go2 = 2.f * gout[b * Cout + co];
    for (int i = threadIdx.x; i < E * E; i += NT) {
        const int e = i / E, j = i % E;
        t2[i] = (e == j) ? 0.f : go2 * tab[pair_index(min(e, j), max(e, j), E)];
    }
    if ((int)threadIdx.x < E) tsk[threadIdx.x] = go2 * tab[threadIdx.x];
    const float tpc = go2 * tab[K] / (float)E;
    const int m = threadIdx.x % MC, g = threadIdx.x / MC;
    // (the first stage_chunk's barriers stand between these writes and their readers)
    for (int m0 = 0; m0 < M; m0 += MC) {
        const int n = min(MC, M - m0);
        stage_chunk(fp, estride, op, qp, E, m0, n, rows, wq, qs, flag);
        if (m >= n) continue;
        const float2 o = *reinterpret_cast<const float2*>(rows + E * RS + 2 * m);
        const float wm = wq[m], qm = qs[m];
        for (int e0 = g; e0 < E; e0 += NG * OWN) {
            float2 fe[OWN], acc[OWN];
            int er[OWN];
#pragma unroll
            for (int a = 0; a < OWN; ++a) {
                er[a] = min(e0 + NG * a, E - 1);          // (a member behind the last is computed again and not written)
                fe[a] = *reinterpret_cast<const float2*>(rows + er[a] * RS + 2 * m);
                acc[a].x = tsk[er[a]] * (fe[a].x - o.x);
                acc[a].y = tsk[er[a]] * (fe[a].y - o.y);
            }
            for (int j = 0; j < E; ++j) {
                const float2 fj = *reinterpret_cast<const float2*>(rows + j * RS + 2 * m);
#pragma unroll
                for (int a = 0; a < OWN; ++a) {
                    const float t = t2[er[a] * E + j];
                    acc[a].x += t * (fe[a].x - fj.x);
                    acc[a].y += t * (fe[a].y - fj.y);
                }
            }
#pragma unroll
            for (int a = 0; a < OWN; ++a) {
                const int e = e0 + NG * a;
                if (e < E) {
                    const float pw = qm * tpc;
                    gf[foff + (long long)e * estride + m0 + m] = make_float2(wm * acc[a].x + pw * fe[a].x, wm * acc[a].y + pw * fe[a].y);
                }
            }
        }
    }
}

bool dims_ok(int B, int E, int C, int L, int M) {
    return B > 0 && E >= 1 && E <= EMAX && C > 0 && L > 0 && M > 0 && (long long)B * C * L <= 0x7fffffffLL;
}

}  // namespace

extern "C" int mk_escorr_sums(const float* f, const float* obs, const float* q, float* sums, int B, int E, int C, int L, int M,
                              void* stream) {
    MK_REQUIRE(f && obs && q && sums && dims_ok(B, E, C, L, M), "escorr_sums: bad arguments (1 <= E <= 32, B * C * L < 2^31)");
    hipLaunchKernelGGL(escorr_sums_kernel, dim3((unsigned)((long long)B * C * L)), dim3(NT), rows_bytes(E), (hipStream_t)stream,
                       (const float2*)f, (const float2*)obs, q, sums, E, C, L, M);
    return mk_check_launch("mk_escorr_sums");
}

extern "C" int mk_escorr_finish(const float* sums, float* loss, float* lossl, float* table, int B, int E, int C, int L, int reduce,
                                float beta, float alpha, float eps, void* stream) {
    MK_REQUIRE(sums && loss && lossl && table && dims_ok(B, E, C, L, 1), "escorr_finish: bad arguments (1 <= E <= 32, B * C * L < 2^31)");
    const int Cout = reduce ? 1 : C;
    const long long nrow = (long long)B * Cout * L;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(escorr_finish_kernel, dim3((unsigned)((nrow + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, s, sums, lossl, table, nrow, C,
                       Cout, L, E, beta, alpha, eps);
    int rc = mk_check_launch("mk_escorr_finish");
    if (rc) return rc;
    hipLaunchKernelGGL(escorr_degrees_kernel, dim3((unsigned)(B * Cout)), dim3(NT), 0, s, lossl, loss, L);
    return mk_check_launch("mk_escorr_finish");
}

extern "C" int mk_escorr_grad(const float* f, const float* obs, const float* q, const float* table, const float* gout, float* gf, int B,
                              int E, int C, int Cout, int L, int M, void* stream) {
    MK_REQUIRE(f && obs && q && table && gout && gf && dims_ok(B, E, C, L, M) && (Cout == 1 || Cout == C),
               "escorr_grad: bad arguments (1 <= E <= 32, B * C * L < 2^31, Cout 1 or C)");
    hipLaunchKernelGGL(escorr_grad_kernel, dim3((unsigned)((long long)B * C * L)), dim3(NT), rows_bytes(E), (hipStream_t)stream,
                       (const float2*)f, (const float2*)obs, q, table, gout, (float2*)gf, E, C, Cout, L, M);
    return mk_check_launch("mk_escorr_grad");
}
