// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (see escore.hip: the SLP vectoriser's packed-fp32 forms are kept out of this library; tests/test_packed_forms.py scans the ISA)
// The plane sums behind the geometric validation metrics (makani/utils/metrics/functions.py:29-677): every metric of that file
// is a quadrature over the plane of a pointwise expression, followed by arithmetic on (B, C[, k]) numbers.  Two kernels form
// the quadratures, the rest stays with the caller (gfx950).
//
//   mk_metric_det_sums   x, y (B, C, N) f32 | bf16 each;  bias (C, N), w (B, C, N) optional;  q (N)
//       out[b][c][0..4] = sum_p q w |x - y|,  q w (x - y)^2,  q w x'y',  q w x'^2,  q w y'^2      x' = x - bias, y' = y - bias
//       (GeometricL1 :53-71, GeometricRMSE :110-132, GeometricACC :184-218); the sums named by `which` in ONE read of x and y
//   mk_metric_ens_sums   f (B, E, C, N) f32 | bf16 read in place, obs (B, C, N) f32;  w optional;  q (N);  1 <= E <= 32
//       out[b][c][0] = sum_p q w (mu - o)^2                                                 (skill,  GeometricSSR :394-400)
//       out[b][c][1] = sum_p q w sum_e (mu - f_e)^2                                         (spread, :287-293, :401)
//       out[b][c][2 + k] = sum_p q w [r = k],  r = #{e : f_e <= o},  k = 0 .. E             (GeometricRankHistogram :639-656)
//
// One thread owns one point (four consecutive points on the 16-byte path) and holds its E members in registers, as
// csrc/crps.hip and csrc/ensnll.hip do.  Mean first, then the centred squares, all relative to the first member (ensnll.hip
// gives the reasoning).  r counts comparisons of the loaded values: for finite inputs that is the insertion index of
// searchsorted(sorted members, o, side="right"); no sort, no one-hot tensor.  The histogram lives in a per-thread LDS column
// bins[k][tid]: the data-dependent index r never indexes a register array, no two lanes share an address (bank = tid mod 32),
// no atomics.  After the loop every bin is summed over the threads in a fixed order.
// Sums are deterministic: every block writes the sums of its chunk to the workspace, a second launch adds the chunks of a
// plane in chunk order.  The arithmetic of one sum does not depend on which other sums are selected (`which` is a run-time,
// block-uniform value and every accumulation is an explicit fmaf), so all-at-once equals one-at-a-time bit for bit.
// 16-byte path (P = 4): N a multiple of 4 and every pointer 16-byte aligned; otherwise one point per thread (P = 1).
#include "block_io.h"

namespace {

constexpr int MNT = 256;
constexpr int MMAXE = 32;
constexpr int MDET = 5;              // sums of mk_metric_det_sums

// grid: (chunks, planes = B * C).  partial[(plane * chunks + chunk) * 5 + k]
template <typename TX, typename TY, int P>
__global__ __launch_bounds__(MNT) void metric_det_kernel(const TX* __restrict__ x, const TY* __restrict__ y, const float* __restrict__ bias,
                                                         const float* __restrict__ w, const float* __restrict__ q,
                                                         float* __restrict__ partial, int C, long long n, int which) {
    __shared__ float red[MDET][MNT / 64];
    const int plane = blockIdx.y, c = plane % C;
    const TX* xp = x + (long long)plane * n;
    const TY* yp = y + (long long)plane * n;
    const float* wp = w ? w + (long long)plane * n : nullptr;
    const float* bp = (bias && (which & 28)) ? bias + (long long)c * n : nullptr;
    float s[MDET] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (long long i = ((long long)blockIdx.x * MNT + threadIdx.x) * P; i < n; i += (long long)gridDim.x * MNT * P) {
        float xv[P], yv[P], qv[P], wv[P], bv[P];
        mk_ld<TX, P>(xp + i, xv);
        mk_ld<TY, P>(yp + i, yv);
        mk_ld<float, P>(q + i, qv);
        if (wp) mk_ld<float, P>(wp + i, wv);
        if (bp) mk_ld<float, P>(bp + i, bv);
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const float wt = wp ? qv[j] * wv[j] : qv[j];
            const float d = xv[j] - yv[j];
            const float a = bp ? xv[j] - bv[j] : xv[j];
            const float b = bp ? yv[j] - bv[j] : yv[j];
            if (which & 1) s[0] = fmaf(wt, fabsf(d), s[0]);
            if (which & 2) s[1] = fmaf(wt * d, d, s[1]);
            if (which & 4) s[2] = fmaf(wt * a, b, s[2]);
            if (which & 8) s[3] = fmaf(wt * a, a, s[3]);
            if (which & 16) s[4] = fmaf(wt * b, b, s[4]);
        }
    }
    float* dst = partial + ((long long)plane * gridDim.x + blockIdx.x) * MDET;
#pragma unroll
    for (int k = 0; k < MDET; ++k)
        if (which & (1 << k)) {          // (which is uniform: every thread reaches the barrier)
            const float t = mk_block_sum_t0<MNT>(s[k], red[k]);
            if (threadIdx.x == 0) dst[k] = t;
        }
}

// grid: (chunks, planes = B * C).  EM: compiled capacity, members e >= E are predicated off.
// partial[(plane * chunks + chunk) * (E + 3) + k]: k = 0 skill, 1 spread, 2 + r the bins
template <typename TF, int EM, int P>
__global__ __launch_bounds__(MNT) void metric_ens_kernel(const TF* __restrict__ f, const float* __restrict__ obs, const float* __restrict__ w,
                                                         const float* __restrict__ q, float* __restrict__ partial, int E, int C,
                                                         long long n, int which) {
    __shared__ float bins[(EM + 1) * MNT];          // bins[k][tid]
    __shared__ float red[2][MNT / 64];
    const int tid = threadIdx.x;
    const int plane = blockIdx.y, b = plane / C, c = plane % C;
    const long long estride = (long long)C * n;
    const TF* fp = f + ((long long)b * E * C + c) * n;
    const float* op = obs + (long long)plane * n;
    const float* wp = w ? w + (long long)plane * n : nullptr;
    const float inv_e = 1.f / (float)E;
    const bool moments = (which & 3) != 0, hist = (which & 4) != 0;
    if (hist) {
#pragma unroll
        for (int k = 0; k <= EM; ++k)
            if (k <= E) bins[k * MNT + tid] = 0.f;
    }
    float skill = 0.f, spread = 0.f;
    for (long long i = ((long long)blockIdx.x * MNT + tid) * P; i < n; i += (long long)gridDim.x * MNT * P) {
        float d[EM][P], ov[P], qv[P], wv[P];
#pragma unroll
        for (int e = 0; e < EM; ++e) {
            if (e < E) {
                mk_ld<TF, P>(fp + e * estride + i, d[e]);
            } else {
#pragma unroll
                for (int j = 0; j < P; ++j) d[e][j] = 0.f;
            }
        }
        mk_ld<float, P>(op + i, ov);
        mk_ld<float, P>(q + i, qv);
        if (wp) mk_ld<float, P>(wp + i, wv);
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const float wt = wp ? qv[j] * wv[j] : qv[j];
            if (hist) {
                int r = 0;
#pragma unroll
                for (int e = 0; e < EM; ++e)
                    if (e < E) r += (d[e][j] <= ov[j]) ? 1 : 0;
                bins[r * MNT + tid] += wt;          // r <= E <= EM: inside this thread's column
            }
            if (moments) {
                const float piv = d[0][j];
                float md = 0.f;                // mu - piv
#pragma unroll
                for (int e = 0; e < EM; ++e)
                    if (e < E) md += d[e][j] - piv;
                md *= inv_e;
                float ss = 0.f;
#pragma unroll
                for (int e = 0; e < EM; ++e) {
                    const float dev = (d[e][j] - piv) - md;
                    if (e < E) ss = fmaf(dev, dev, ss);
                }
                const float r0 = (ov[j] - piv) - md;
                skill = fmaf(wt * r0, r0, skill);
                spread = fmaf(wt, ss, spread);
            }
        }
    }
    const int K = E + 3;
    float* dst = partial + ((long long)plane * gridDim.x + blockIdx.x) * K;
    if (which & 1) {
        const float t = mk_block_sum_t0<MNT>(skill, red[0]);
        if (tid == 0) dst[0] = t;
    }
    if (which & 2) {
        const float t = mk_block_sum_t0<MNT>(spread, red[1]);
        if (tid == 0) dst[1] = t;
    }
    if (hist) {
        __syncthreads();
        const int lane = tid & 63;
        for (int k = tid >> 6; k <= E; k += MNT / 64) {          // one wave per bin: the four columns of a lane in order, then the lanes
            float v = bins[k * MNT + lane];
#pragma unroll
            for (int i = 1; i < MNT / 64; ++i) v += bins[k * MNT + i * 64 + lane];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) dst[2 + k] = v;
        }
    }
}

// out[plane][k] = the chunks of the plane in chunk order, for the selected k: bit min(k, nsel - 1) of which
__global__ void metric_finish_kernel(const float* __restrict__ partial, float* __restrict__ out, long long planes, int chunks, int K, int which,
                                     int nsel) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= planes * K) return;
    const int k = (int)(t % K);
    if (!((which >> (k < nsel ? k : nsel - 1)) & 1)) return;
    const long long plane = t / K;
    float s = 0.f;
    for (int ch = 0; ch < chunks; ++ch) s += partial[(plane * chunks + ch) * K + k];
    out[t] = s;
}

int finish(const float* ws, float* out, long long planes, int chunks, int K, int which, int nsel, hipStream_t s, const char* what) {
    const long long total = planes * K;
    hipLaunchKernelGGL(metric_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ws, out, planes, chunks, K, which, nsel);
    return mk_check_launch(what);
}

template <typename TX, typename TY>
int det_launch(bool vec, dim3 grid, hipStream_t s, const void* x, const void* y, const float* bias, const float* w, const float* q, float* ws,
               int C, long long n, int which) {
    if (vec)
        hipLaunchKernelGGL((metric_det_kernel<TX, TY, 4>), grid, dim3(MNT), 0, s, (const TX*)x, (const TY*)y, bias, w, q, ws, C, n, which);
    else
        hipLaunchKernelGGL((metric_det_kernel<TX, TY, 1>), grid, dim3(MNT), 0, s, (const TX*)x, (const TY*)y, bias, w, q, ws, C, n, which);
    return mk_check_launch("mk_metric_det_sums");
}

template <typename TF>
int ens_launch(bool vec, dim3 grid, hipStream_t s, const TF* f, const float* obs, const float* w, const float* q, float* ws, int E, int C,
               long long n, int which) {
    return mk_with_capacity(E, "metric_ens_sums", [&](auto em) {
        constexpr int PV = em() < 32 ? 4 : 1;          // 32 members x 4 points would be 128 registers of members alone: one point
        if (vec && PV == 4)
            hipLaunchKernelGGL((metric_ens_kernel<TF, em(), PV>), grid, dim3(MNT), 0, s, f, obs, w, q, ws, E, C, n, which);
        else
            hipLaunchKernelGGL((metric_ens_kernel<TF, em(), 1>), grid, dim3(MNT), 0, s, f, obs, w, q, ws, E, C, n, which);
        return mk_check_launch("mk_metric_ens_sums");
    });
}

}  // namespace

extern "C" int mk_metric_chunks(long long n) { return mk_plane_chunks(n); }

extern "C" int mk_metric_det_sums(const void* x, int x_dtype, const void* y, int y_dtype, const float* bias, const float* w, const float* q,
                                  float* out, float* ws, int B, int C, long long n, int which, void* stream) {
    MK_REQUIRE(x && y && q && out && ws, "metric_det_sums: null pointer (x, y, q, out and ws are required)");
    MK_REQUIRE(B > 0 && C > 0, "metric_det_sums: B = %d, C = %d must be positive", B, C);
    MK_REQUIRE(n > 0, "metric_det_sums: N = %lld points per plane must be positive", n);
    MK_REQUIRE_PLANES("metric_det_sums", (long long)B * C);
    MK_REQUIRE((x_dtype == MK_F32 || x_dtype == MK_BF16) && (y_dtype == MK_F32 || y_dtype == MK_BF16), "metric_det_sums: x and y are f32 or bf16");
    MK_REQUIRE(which > 0 && which < 32, "metric_det_sums: which = %d selects no sum or an unknown one (bits 0..4)", which);
    hipStream_t s = (hipStream_t)stream;
    const int chunks = mk_metric_chunks(n);
    const dim3 grid((unsigned)chunks, (unsigned)(B * C));
    const bool vec = n % 4 == 0 && mk_aligned16(x) && mk_aligned16(y) && mk_aligned16(q) && mk_aligned16(w) && mk_aligned16(bias);
    int rc;
    if (x_dtype == MK_F32)
        rc = y_dtype == MK_F32 ? det_launch<float, float>(vec, grid, s, x, y, bias, w, q, ws, C, n, which)
                               : det_launch<float, u16>(vec, grid, s, x, y, bias, w, q, ws, C, n, which);
    else
        rc = y_dtype == MK_F32 ? det_launch<u16, float>(vec, grid, s, x, y, bias, w, q, ws, C, n, which)
                               : det_launch<u16, u16>(vec, grid, s, x, y, bias, w, q, ws, C, n, which);
    if (rc) return rc;
    return finish(ws, out, (long long)B * C, chunks, MDET, which, MDET, s, "mk_metric_det_sums");
}

extern "C" int mk_metric_ens_sums(const void* f, int f_dtype, const float* obs, const float* w, const float* q, float* out, float* ws, int B,
                                  int E, int C, long long n, int which, void* stream) {
    MK_REQUIRE(f && obs && q && out && ws, "metric_ens_sums: null pointer (f, obs, q, out and ws are required)");
    MK_REQUIRE(E >= 1 && E <= MMAXE, "metric_ens_sums: ensemble size %d outside 1 <= E <= 32", E);
    MK_REQUIRE(B > 0 && C > 0, "metric_ens_sums: B = %d, C = %d must be positive", B, C);
    MK_REQUIRE(n > 0, "metric_ens_sums: N = %lld points per plane must be positive", n);
    MK_REQUIRE_PLANES("metric_ens_sums", (long long)B * C);
    MK_REQUIRE(f_dtype == MK_F32 || f_dtype == MK_BF16, "metric_ens_sums: members are f32 or bf16");
    MK_REQUIRE(which > 0 && which < 8, "metric_ens_sums: which = %d selects no sum or an unknown one (bits 0..2)", which);
    hipStream_t s = (hipStream_t)stream;
    const int chunks = mk_metric_chunks(n);
    const dim3 grid((unsigned)chunks, (unsigned)(B * C));
    const bool vec = n % 4 == 0 && mk_aligned16(f) && mk_aligned16(obs) && mk_aligned16(q) && mk_aligned16(w);
    const int rc = f_dtype == MK_F32 ? ens_launch<float>(vec, grid, s, (const float*)f, obs, w, q, ws, E, C, n, which)
                                     : ens_launch<u16>(vec, grid, s, (const u16*)f, obs, w, q, ws, E, C, n, which);
    if (rc) return rc;
    return finish(ws, out, (long long)B * C, chunks, E + 3, which, 3, s, "mk_metric_ens_sums");
}
