// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (see escore.hip: the SLP vectoriser's packed-fp32 forms are kept out of this library; tests/test_packed_forms.py scans the ISA)
// A rollout step's validation metrics in one pass: what MetricsHandler.update (makani/utils/metric.py:623-649) asks of its up
// to seven MetricRollout handles, formed from ONE read of the planes that any handle lists (gfx950).
//
//   mk_mrollout_sums     pred (B, E, C, N) f32 | bf16 read in place, tar (B, C, N) f32 | bf16, w (B, C, N) optional, q (N),
//                        clim (Ja, N) optional, table (J, 3) on the device = {channel, bits, climatology row | -1} per plane.
//                        grid (chunks, B * J): only the J listed planes are read, no gathered copy, no ensemble-mean tensor.
//       per point  nan = isnan(t), t' = nan ? 0 : t, w' = q w (nan ? 0 : 1)            (metric.py:146-160, decided per point)
//                  mu  = the member mean in fp32: mean first, centred on the first member, as metric_ens_kernel (metrics.hip)
//       partial[(b J + j) chunks + chunk][k]:  0 sum w'  1 #NaN  2 L1  3 L2 (= SSR's skill)  4 XY  5 XX  6 YY (climatology
//                  subtracted)  7 sum w' sum_e (mu - f_e)^2  8 sum w' crps_point (csrc/crps_point.h)  9 + r the E + 1 rank bins
//   mk_mrollout_finish   one launch for all handles: the chunks in chunk order, the metric per sample in the reference's order,
//                        counts_new decided on the device, merged into row idt of the curve and counter buffers in place.
//
// Conventions of csrc/metrics.hip: one thread per point (four on the 16-byte path), members in registers, capacities EM in
// {1, 2, 4, 8, 16, 32} with surplus members predicated off, every accumulation an explicit fmaf under a block-uniform bit (so
// a sum does not depend on which other sums its plane carries), chunk partials added in chunk order, no atomics, the histogram
// in per-thread LDS columns bins[k][tid].
#include "block_io.h"
#include "crps_point.h"

namespace {

constexpr int RNT = 256;
constexpr int RMAXE = 32;
constexpr int RNS = MK_MROLL_NSUM;          // sums in front of the bins

template <typename TP, typename TT, int EM, int P>
__global__ __launch_bounds__(RNT) void mrollout_kernel(const TP* __restrict__ pred, const TT* __restrict__ tar, const float* __restrict__ w,
                                                       const float* __restrict__ q, const float* __restrict__ clim,
                                                       const int* __restrict__ table, float* __restrict__ partial, int E, int C, int J,
                                                       int Ja, long long n, int mask_nan) {
    __shared__ float bins[(EM + 1) * RNT];          // bins[k][tid]
    __shared__ float red[RNS][RNT / 64];
    const int tid = threadIdx.x;
    const int row = blockIdx.y, b = row / J, j = row % J;
    int ch = table[3 * j], bits = table[3 * j + 1];
    const int cr = table[3 * j + 2];
    const bool valid = ch >= 0 && ch < C;          // (a row outside the tensor reads nothing and yields zeros)
    if (!valid) ch = 0, bits = 0;
    const long long nn = valid ? n : 0;
    const long long estride = (long long)C * n;
    const TP* fp = pred + ((long long)b * E * C + ch) * n;
    const TT* tp = tar + ((long long)b * C + ch) * n;
    const float* wp = w ? w + ((long long)b * C + ch) * n : nullptr;
    const float* bp = (clim && (bits & MK_MROLL_ACC) && cr >= 0 && cr < Ja) ? clim + (long long)cr * n : nullptr;
    const float inv_e = 1.f / (float)E;
    const bool l1 = bits & MK_MROLL_L1, l2 = bits & MK_MROLL_L2, acc = bits & MK_MROLL_ACC, spr = bits & MK_MROLL_SPREAD;
    const bool crps = (bits & MK_MROLL_CRPS) && E >= 2, hist = bits & MK_MROLL_HIST;
    if (hist) {
#pragma unroll
        for (int k = 0; k <= EM; ++k)
            if (k <= E) bins[k * RNT + tid] = 0.f;
    }
    float s[RNS];
#pragma unroll
    for (int k = 0; k < RNS; ++k) s[k] = 0.f;
    for (long long i = ((long long)blockIdx.x * RNT + tid) * P; i < nn; i += (long long)gridDim.x * RNT * P) {
        float d[EM][P], tv[P], qv[P], wv[P], bv[P];
#pragma unroll
        for (int e = 0; e < EM; ++e) {
            if (e < E) {
                mk_ld<TP, P>(fp + e * estride + i, d[e]);
            } else {
#pragma unroll
                for (int p = 0; p < P; ++p) d[e][p] = 0.f;
            }
        }
        mk_ld<TT, P>(tp + i, tv);
        mk_ld<float, P>(q + i, qv);
        if (wp) mk_ld<float, P>(wp + i, wv);
        if (bp) mk_ld<float, P>(bp + i, bv);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const bool isn = mask_nan && (tv[p] != tv[p]);
            const float t = isn ? 0.f : tv[p];
            const float wt = isn ? 0.f : (wp ? qv[p] * wv[p] : qv[p]);
            s[0] += wt;
            s[1] += isn ? 1.f : 0.f;
            const float piv = d[0][p];
            float md = 0.f;                // mu - piv
#pragma unroll
            for (int e = 0; e < EM; ++e)
                if (e < E) md += d[e][p] - piv;
            md *= inv_e;
            const float r0 = (t - piv) - md;          // t' - mu
            if (l1) s[2] = fmaf(wt, fabsf(r0), s[2]);
            if (l2) s[3] = fmaf(wt * r0, r0, s[3]);
            if (acc) {
                const float mu = piv + md;
                const float xa = bp ? mu - bv[p] : mu;
                const float ya = bp ? t - bv[p] : t;
                s[4] = fmaf(wt * xa, ya, s[4]);
                s[5] = fmaf(wt * xa, xa, s[5]);
                s[6] = fmaf(wt * ya, ya, s[6]);
            }
            if (spr) {
                float ss = 0.f;
#pragma unroll
                for (int e = 0; e < EM; ++e) {
                    const float dev = (d[e][p] - piv) - md;
                    if (e < E) ss = fmaf(dev, dev, ss);
                }
                s[7] = fmaf(wt, ss, s[7]);
            }
            if constexpr (EM >= 2) {
                if (crps) {
                    float v[EM];
#pragma unroll
                    for (int e = 0; e < EM; ++e) v[e] = d[e][p];
                    const float sc = crps_point<EM, false>(v, E, t, CRPS_SKILLSPREAD, 1.f, 1.0e-6f, nullptr);
                    s[8] = fmaf(wt, sc, s[8]);
                }
            }
            if (hist) {
                int r = 0;
#pragma unroll
                for (int e = 0; e < EM; ++e)
                    if (e < E) r += (d[e][p] <= t) ? 1 : 0;
                bins[r * RNT + tid] += wt;          // r <= E <= EM: inside this thread's column
            }
        }
    }
    const int K = RNS + E + 1;
    float* dst = partial + ((long long)row * gridDim.x + blockIdx.x) * K;
#pragma unroll
    for (int k = 0; k < RNS; ++k) {          // (every thread reaches every barrier; an unselected sum is 0)
        const float t = mk_block_sum_t0<RNT>(s[k], red[k]);
        if (tid == 0) dst[k] = t;
    }
    if (hist) {
        __syncthreads();
        const int lane = tid & 63;
        for (int k = tid >> 6; k <= E; k += RNT / 64) {          // one wave per bin: the four columns of a lane in order, then the lanes
            float v = bins[k * RNT + lane];
#pragma unroll
            for (int i = 1; i < RNT / 64; ++i) v += bins[k * RNT + i * 64 + lane];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) dst[RNS + k] = v;
        }
    } else if (tid <= E) {
        dst[RNS + tid] = 0.f;
    }
}

// sums[row][k] = the chunks of the row in chunk order
__global__ void mrollout_chunks_kernel(const float* __restrict__ partial, float* __restrict__ sums, long long rows, int chunks, int K) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * K) return;
    const long long row = t / K;
    const int k = (int)(t % K);
    float s = 0.f;
    for (int ch = 0; ch < chunks; ++ch) s += partial[(row * chunks + ch) * K + k];
    sums[t] = s;
}

// grid: one block per handle
__global__ __launch_bounds__(RNT) void mrollout_finish_kernel(const float* __restrict__ sums, int chunks, const int* __restrict__ hdesc,
                                                              const int* __restrict__ hplanes, const float* __restrict__ hscale,
                                                              float* __restrict__ buf, long long buf_len, int B, int E, int J, int idt,
                                                              int has_weight, float acc_eps, float ssr_eps) {
    const int tid = threadIdx.x;
    const int* hd = hdesc + blockIdx.x * MK_MROLL_HDESC;
    const int kind = hd[0], n = hd[1], po = hd[2], co = hd[3], cto = hd[4], steps = hd[5];
    if (n <= 0 || idt < 0 || idt >= steps) return;          // (block-uniform)
    const int K = RNS + E + 1;
    // the k-th sum of plane j of sample b: its chunks in chunk order
    auto plane_sum = [&](int b, int j, int k) {
        const float* base = sums + ((long long)b * J + j) * chunks * K + k;
        float v = 0.f;
        for (int ch = 0; ch < chunks; ++ch) v += base[(long long)ch * K];
        return v;
    };
    int mine = 0;
    for (int t = tid; t < n * B; t += RNT) {
        const int j = hplanes[po + t % n];
        if (j >= 0 && j < J && plane_sum(t / n, j, 1) > 0.f) mine = 1;
    }
    const bool from_sums = __syncthreads_or(mine) || has_weight;          // metric.py:146: any NaN among the handle's channels
    const int aux = kind == MK_MROLL_KIND_HIST ? E + 1 : 1;
    const float em1 = (float)(E - 1), ef = (float)E;
    for (int t = tid; t < n * aux; t += RNT) {
        const int ci = t / aux, a = t % aux;
        const int j = hplanes[po + ci];
        if (j < 0 || j >= J) continue;
        const float sc = hscale[po + ci];
        float val = 0.f, cnt = 0.f;
        for (int b = 0; b < B; ++b) {
            cnt += plane_sum(b, j, 0);
            if (kind == MK_MROLL_KIND_L1) {
                val += plane_sum(b, j, 2);
            } else if (kind == MK_MROLL_KIND_RMSE) {
                val += plane_sum(b, j, 3);
            } else if (kind == MK_MROLL_KIND_ACC) {
                val += plane_sum(b, j, 4) / (sqrtf(plane_sum(b, j, 5) * plane_sum(b, j, 6)) + acc_eps);
            } else if (kind == MK_MROLL_KIND_CRPS) {
                val += plane_sum(b, j, 8);
            } else if (kind == MK_MROLL_KIND_SPREAD) {
                val += sqrtf(plane_sum(b, j, 7) / em1);
            } else if (kind == MK_MROLL_KIND_SSR) {
                const float sp = plane_sum(b, j, 7) / em1;
                val += sqrtf(sp / fmaxf(plane_sum(b, j, 3) - sp / ef, ssr_eps));
            } else {
                val += plane_sum(b, j, RNS + a);
            }
        }
        if (kind == MK_MROLL_KIND_RMSE) val = sqrtf(val) * sc;
        if (kind == MK_MROLL_KIND_CRPS || kind == MK_MROLL_KIND_SPREAD) val *= sc;
        const long long at = (long long)co + ((long long)idt * n + ci) * aux + a;
        const long long ct = (long long)cto + (long long)idt * n + ci;
        if (at < 0 || at >= buf_len || ct < 0 || ct >= buf_len) continue;
        const float old = buf[at];
        buf[at] = kind == MK_MROLL_KIND_RMSE ? sqrtf(old * old + val * val) : old + val;
        if (a == 0) buf[ct] += from_sums ? cnt : (float)B;
    }
}

template <typename TP, typename TT>
int sums_launch(bool vec, dim3 grid, hipStream_t s, const TP* pred, const TT* tar, const float* w, const float* q, const float* clim,
                const int* table, float* partial, int E, int C, int J, int Ja, long long n, int mask_nan) {
    return mk_with_capacity<RMAXE, 1>(E, "mrollout_sums", [&](auto em) {
        constexpr int PV = em() < 32 ? 4 : 1;          // (metrics.hip: 32 members x 4 points would be 128 registers of members alone)
        if (vec && PV == 4)
            hipLaunchKernelGGL((mrollout_kernel<TP, TT, em(), PV>), grid, dim3(RNT), 0, s, pred, tar, w, q, clim, table, partial, E, C, J, Ja,
                               n, mask_nan);
        else
            hipLaunchKernelGGL((mrollout_kernel<TP, TT, em(), 1>), grid, dim3(RNT), 0, s, pred, tar, w, q, clim, table, partial, E, C, J, Ja,
                               n, mask_nan);
        return mk_check_launch("mk_mrollout_sums");
    });
}

}  // namespace

extern "C" int mk_mrollout_sums(const void* pred, int p_dtype, const void* tar, int t_dtype, const float* w, const float* q,
                                const float* clim, const int* table, float* partial, float* sums, int B, int E, int C, int J, int Ja,
                                long long n, int mask_nan, void* stream) {
    MK_REQUIRE(pred && tar && q && table && partial, "mrollout_sums: null pointer (pred, tar, q, table and partial are required)");
    MK_REQUIRE(E >= 1 && E <= RMAXE, "mrollout_sums: ensemble size %d outside 1 <= E <= 32", E);
    MK_REQUIRE(B > 0 && C > 0 && J > 0, "mrollout_sums: B = %d, C = %d, J = %d must be positive", B, C, J);
    MK_REQUIRE(n > 0, "mrollout_sums: N = %lld points per plane must be positive", n);
    MK_REQUIRE(clim ? Ja > 0 : Ja == 0, "mrollout_sums: %d climatology rows %s a climatology", Ja, clim ? "with" : "without");
    MK_REQUIRE_PLANES("mrollout_sums", (long long)B * J);
    MK_REQUIRE((p_dtype == MK_F32 || p_dtype == MK_BF16) && (t_dtype == MK_F32 || t_dtype == MK_BF16),
               "mrollout_sums: prediction and target are f32 or bf16");
    hipStream_t s = (hipStream_t)stream;
    const int chunks = mk_plane_chunks(n);
    const dim3 grid((unsigned)chunks, (unsigned)(B * J));
    const bool vec = n % 4 == 0 && mk_aligned16(pred) && mk_aligned16(tar) && mk_aligned16(q) && mk_aligned16(w) && mk_aligned16(clim);
    int rc;
    if (p_dtype == MK_F32)
        rc = t_dtype == MK_F32
                 ? sums_launch<float, float>(vec, grid, s, (const float*)pred, (const float*)tar, w, q, clim, table, partial, E, C, J, Ja, n, mask_nan)
                 : sums_launch<float, u16>(vec, grid, s, (const float*)pred, (const u16*)tar, w, q, clim, table, partial, E, C, J, Ja, n, mask_nan);
    else
        rc = t_dtype == MK_F32
                 ? sums_launch<u16, float>(vec, grid, s, (const u16*)pred, (const float*)tar, w, q, clim, table, partial, E, C, J, Ja, n, mask_nan)
                 : sums_launch<u16, u16>(vec, grid, s, (const u16*)pred, (const u16*)tar, w, q, clim, table, partial, E, C, J, Ja, n, mask_nan);
    if (rc || !sums) return rc;
    const long long total = (long long)B * J * (RNS + E + 1);
    hipLaunchKernelGGL(mrollout_chunks_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, partial, sums, (long long)B * J, chunks,
                       RNS + E + 1);
    return mk_check_launch("mk_mrollout_sums");
}

extern "C" int mk_mrollout_finish(const float* sums, int chunks, const int* hdesc, const int* hplanes, const float* hscale, float* buf,
                                  long long buf_len, int nh, int B, int E, int J, int idt, int has_weight, float acc_eps, float ssr_eps,
                                  void* stream) {
    MK_REQUIRE(sums && hdesc && hplanes && hscale && buf, "mrollout_finish: null pointer");
    MK_REQUIRE(chunks >= 1 && nh >= 1 && B > 0 && J > 0 && buf_len > 0, "mrollout_finish: chunks = %d, handles = %d, B = %d, J = %d, buffer of %lld",
               chunks, nh, B, J, buf_len);
    MK_REQUIRE(E >= 1 && E <= RMAXE, "mrollout_finish: ensemble size %d outside 1 <= E <= 32", E);
    MK_REQUIRE(idt >= 0, "mrollout_finish: rollout step %d is negative", idt);
    hipLaunchKernelGGL(mrollout_finish_kernel, dim3((unsigned)nh), dim3(RNT), 0, (hipStream_t)stream, sums, chunks, hdesc, hplanes, hscale, buf,
                       buf_len, B, E, J, idt, has_weight, acc_eps, ssr_eps);
    return mk_check_launch("mk_mrollout_finish");
}
