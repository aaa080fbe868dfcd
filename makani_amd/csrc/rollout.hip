// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (see escore.hip: the SLP vectoriser's packed-fp32 forms are kept out of this library; tests/test_packed_forms.py scans the ISA)
// Online rollout diagnostics (makani/utils/inference/rollout_buffer.py:670-1338): the running mean and centred sum of squares
// (M2) per lead time of the de-normalised fields (TemporalAverageBuffer), of the angular power spectrum (SpectrumAverageBuffer)
// and of the latitude-weighted longitude spectrum (ZonalSpectrumAverageBuffer).  Three HBM-streaming kernels:
//
//   mk_welford_update   src (B, Csrc, N) f32 | bf16 read in place (optional channel list and per-channel scale / bias) ->
//                       mean, m2 (C, N) fp32 updated in place.  Per element: y_b = scale x_b + bias, the batch's mean and centred
//                       M2 by a running update over b (any B >= 1), then the merge with the n0 = *count samples seen before:
//                       d = mean_b - mean, mean += d B / n, m2 += m2_b + d^2 n0 B / n, n = n0 + B.
//   mk_power_spectrum   S-layout coefficients (L, M, 2, R), row r = sample * Cp + c, sample = b * E + e ->
//                       out[b][c][e0 + e][l] = sum_m c_m |scale_c s + [m + m_off == 0] bias_c one[l]|^2, c_m = 1 for the global
//                       order 0 and 2 otherwise; orders m > l + tri_off are structurally zero and are not read.  one[l] is the
//                       transform of the constant field 1: the affine map of the fields is applied to their coefficients.
//   mk_zonal_welford    F-layout longitude spectra (M, nlat, 2, R) -> p_b = c_m latw[k] |scale_c F + [m == 0] bias_c|^2 (c_m = 2
//                       for every m >= 1), its batch statistics over b merged into mean, m2 (C, E1, nlat, M) as above.
//
// count is a DEVICE pointer: no kernel argument depends on the number of samples seen, the caller adds B behind the launch on
// the same stream, and an update can be captured in a graph.  The ratios B / n and n0 B / n are formed in fp64 and rounded once.
// Every output element is written by exactly one thread and every sum runs in a fixed order: repeats are bit-identical.
#include "block_io.h"

namespace {

constexpr int RNT = 256;          // threads per block
constexpr int ZM = 64, ZQMAX = 48;   // zonal tile: orders x at most ZQMAX + 1 rows ((member, channel) pairs)

struct Merge {
    float a, b;                   // B / n and n0 B / n
};
__device__ __forceinline__ Merge merge_ratios(const long long* count, int B) {
    const long long n0 = *count;
    const double n = (double)(n0 + B);
    Merge r;
    r.a = (float)((double)B / n);
    r.b = (float)((double)n0 * (double)B / n);
    return r;
}
// one more value of a batch: (mu, q) = mean and centred sum of squares of the values so far, inv = 1 / their number
__device__ __forceinline__ void batch_push(float y, float inv, float& mu, float& q) {
    const float d = y - mu;
    mu += d * inv;
    q += d * (y - mu);
}
__device__ __forceinline__ void running_merge(float& mean, float& m2, float mu, float q, const Merge& r) {
    const float d = mu - mean;
    mean += d * r.a;
    m2 += q + d * d * r.b;
}

template <typename T, int P>
__global__ __launch_bounds__(RNT) void welford_kernel(const T* __restrict__ src, const int* __restrict__ chan, const float* __restrict__ scale,
                                                      const float* __restrict__ bias, float* __restrict__ mean, float* __restrict__ m2,
                                                      const long long* __restrict__ count, int B, int Csrc, long long N) {
    const int c = blockIdx.y;
    const long long n = ((long long)blockIdx.x * RNT + threadIdx.x) * P;
    if (n >= N) return;                              // (P = 4 only with N % 4 == 0: a group never straddles the end)
    const int cs = chan ? chan[c] : c;
    const float s = scale ? scale[c] : 1.f, o = bias ? bias[c] : 0.f;
    float mu[P], q[P];
#pragma unroll
    for (int j = 0; j < P; ++j) mu[j] = q[j] = 0.f;
    const T* p = src + (long long)cs * N + n;
    const long long step = (long long)Csrc * N;
    for (int b = 0; b < B; ++b) {
        float v[P];
        mk_ld<T, P>(p + b * step, v);
        const float inv = 1.f / (float)(b + 1);
#pragma unroll
        for (int j = 0; j < P; ++j) batch_push(fmaf(s, v[j], o), inv, mu[j], q[j]);
    }
    const Merge r = merge_ratios(count, B);
    const long long at = (long long)c * N + n;
    float a[P], v[P];
    mk_ld<float, P>(mean + at, a);
    mk_ld<float, P>(m2 + at, v);
#pragma unroll
    for (int j = 0; j < P; ++j) running_merge(a[j], v[j], mu[j], q[j], r);
    mk_st<float, P>(mean + at, a);
    mk_st<float, P>(m2 + at, v);
}

// one block: one degree l and 64 rows; wave w adds the orders w, w + 4, .. of its rows (256-byte row segments), the four partial sums
// are added in wave order
template <typename TO>
__global__ __launch_bounds__(RNT) void power_kernel(const float* __restrict__ S, const float* __restrict__ scale, const float* __restrict__ bias,
                                                    const float* __restrict__ one, TO* __restrict__ out, int L, int M, int R, int Cp, int C,
                                                    int E, int E1, int e0, int nrows, int tri_off, int m_off) {
    __shared__ float part[RNT / 64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = blockIdx.y;
    const int r = blockIdx.x * 64 + lane;
    const int samp = r / Cp, c = r - samp * Cp;
    const bool live = r < nrows && c < C;            // (the rows c >= C of a sample are padding)
    const int mend = max(0, min(M, l + tri_off + 1));
    float acc = 0.f;
    if (live) {
        const float s = scale ? scale[c] : 1.f;
        const float o = bias ? bias[c] * one[l] : 0.f;
        const float* p = S + (long long)l * M * 2 * R + r;
        for (int m = wave; m < mend; m += RNT / 64) {
            const bool zero = (m + m_off) == 0;
            float re = s * p[(long long)m * 2 * R];
            const float im = s * p[((long long)m * 2 + 1) * R];
            if (zero) re += o;
            acc += (zero ? 1.f : 2.f) * (re * re + im * im);
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && live) {
        float t = part[0][lane];
        for (int w = 1; w < RNT / 64; ++w) t += part[w][lane];
        const int b = samp / E, e = samp - b * E;
        mk_st<TO>(out + (((long long)b * C + c) * E1 + e0 + e) * L + l, t);
    }
}

// one block: one latitude, ZM orders, qt (member, channel) rows (zonal_rows_per_tile: the E Cp rows cut into equal tiles of at most
// ZQMAX rows, qt odd).  F is unit-stride in the row, the running buffers in the order, so the tile is turned in LDS.  Items
// (order, row) are dealt to the threads row-fastest: consecutive lanes read consecutive rows of one order and go on with the next
// order, so no lane idles on a ragged row count, and write tile[order * qt + row] = consecutive dwords.  Afterwards 64 lanes with
// consecutive orders of one row read dwords qt apart.  ds_write_b32 / ds_read_b32 see 32 banks per 32-lane half: 32 consecutive
// dwords, and 32 dwords an odd stride apart, are 32 different banks — no conflict in either direction, no padding column.
template <bool RB>
__global__ __launch_bounds__(RNT) void zonal_kernel(const float* __restrict__ F, const float* __restrict__ scale, const float* __restrict__ bias,
                                                    const float* __restrict__ latw, float* __restrict__ mean, float* __restrict__ m2,
                                                    const long long* __restrict__ count, int M, int nlat, int R, int Cp, int C, int B, int E,
                                                    int E1, int e0, int qt) {
    extern __shared__ float zonal_tile[];            // batch means [ZM][qt], then batch M2 [ZM][qt]
    float* tmu = zonal_tile;
    float* tq = zonal_tile + ZM * qt;
    const int t = threadIdx.x;
    const int k = blockIdx.z, m0 = blockIdx.x * ZM, q0 = blockIdx.y * qt;
    const int nq = E * Cp;                           // rows between two batch entries of one (member, channel)
    const float wk = latw[k];
    for (int i = t; i < ZM * qt; i += RNT) {
        const int ml = i / qt, ql = i - ml * qt;
        const int m = m0 + ml, qi = q0 + ql, e = qi / Cp, c = qi - e * Cp;
        float mu = 0.f, q = 0.f;
        if (m < M && qi < nq && c < C) {
            const float s = scale ? scale[c] : 1.f, o = (bias && m == 0) ? bias[c] : 0.f;
            const float cm = (m == 0 ? 1.f : 2.f) * wk;
            const float* p = F + ((long long)m * nlat + k) * 2 * R + qi;
            for (int b = 0; b < B; ++b) {
                const float re = fmaf(s, p[(long long)b * nq], o);
                const float im = s * p[R + (long long)b * nq];
                float y = cm * (re * re + im * im);
                if (RB) y = bf16_to_f32(f32_to_bf16(y));
                batch_push(y, 1.f / (float)(b + 1), mu, q);
            }
        }
        tmu[i] = mu;
        tq[i] = q;
    }
    __syncthreads();
    const int ml = t & (ZM - 1), m = m0 + ml;
    if (m >= M) return;                              // (after the only barrier)
    const Merge r = merge_ratios(count, B);
    for (int ql = t / ZM; ql < qt; ql += RNT / ZM) {
        const int qi = q0 + ql, e = qi / Cp, c = qi - e * Cp;
        if (qi >= nq || c >= C) continue;
        const long long at = (((long long)c * E1 + e0 + e) * nlat + k) * M + m;
        float a = mean[at], v = m2[at];
        running_merge(a, v, tmu[ml * qt + ql], tq[ml * qt + ql], r);
        mean[at] = a;
        m2[at] = v;
    }
}

// rows per tile: the nq rows in ceil(nq / ZQMAX) equal tiles, rounded up to an odd count
int zonal_rows_per_tile(long long nq) {
    const long long tiles = (nq + ZQMAX - 1) / ZQMAX;
    return (int)((nq + tiles - 1) / tiles) | 1;
}

template <typename T>
void welford_launch(bool vec, dim3 grid, hipStream_t s, const void* src, const int* chan, const float* scale, const float* bias, float* mean,
                    float* m2, const long long* count, int B, int Csrc, long long N) {
    if (vec) hipLaunchKernelGGL((welford_kernel<T, 4>), grid, dim3(RNT), 0, s, (const T*)src, chan, scale, bias, mean, m2, count, B, Csrc, N);
    else hipLaunchKernelGGL((welford_kernel<T, 1>), grid, dim3(RNT), 0, s, (const T*)src, chan, scale, bias, mean, m2, count, B, Csrc, N);
}

}  // namespace

extern "C" int mk_welford_update(const void* src, int dtype, const int* chan, const float* scale, const float* bias, float* mean, float* m2,
                                 const long long* count, int B, int Csrc, int C, long long N, void* stream) {
    MK_REQUIRE(src && mean && m2 && count, "welford_update: null pointer");
    MK_REQUIRE(dtype == MK_F32 || dtype == MK_BF16, "welford_update: unknown dtype %d", dtype);
    MK_REQUIRE(B >= 1 && Csrc >= 1 && C >= 1 && N >= 1, "welford_update: bad shape (B %d, Csrc %d, C %d, N %lld)", B, Csrc, C, N);
    MK_REQUIRE(chan || C <= Csrc, "welford_update: %d channels selected from %d without a channel list", C, Csrc);
    MK_REQUIRE_PLANES("welford_update", C);
    const bool vec = N % 4 == 0 && mk_aligned16(src) && mk_aligned16(mean) && mk_aligned16(m2);
    const long long per = (long long)RNT * (vec ? 4 : 1), blocks = (N + per - 1) / per;
    MK_REQUIRE(blocks < (1ll << 31), "welford_update: N = %lld points per channel exceed the grid", N);
    const dim3 grid((unsigned)blocks, (unsigned)C);
    if (dtype == MK_BF16) welford_launch<u16>(vec, grid, (hipStream_t)stream, src, chan, scale, bias, mean, m2, count, B, Csrc, N);
    else welford_launch<float>(vec, grid, (hipStream_t)stream, src, chan, scale, bias, mean, m2, count, B, Csrc, N);
    return mk_check_launch("mk_welford_update");
}

extern "C" int mk_power_spectrum(const float* S, const float* scale, const float* bias, const float* one, void* out, int out_dtype, int L,
                                 int M, int R, int Cp, int B, int E, int C, int E1, int e0, int tri_off, int m_off, void* stream) {
    MK_REQUIRE(S && out, "power_spectrum: null pointer");
    MK_REQUIRE(!bias || one, "power_spectrum: a bias needs the transform of the constant field (one)");
    MK_REQUIRE(out_dtype == MK_F32 || out_dtype == MK_BF16, "power_spectrum: unknown dtype %d", out_dtype);
    MK_REQUIRE(L >= 1 && L <= 65535 && M >= 1 && B >= 1 && E >= 1 && C >= 1, "power_spectrum: bad shape (L %d, M %d, B %d, E %d, C %d)", L, M,
               B, E, C);
    MK_REQUIRE(Cp >= C && (long long)B * E * Cp <= R, "power_spectrum: %d x %d samples of %d rows do not fit the %d rows of S", B, E, Cp, R);
    MK_REQUIRE(e0 >= 0 && e0 + E <= E1, "power_spectrum: members [%d, %d + %d) leave the output's [0, %d)", e0, e0, E, E1);
    MK_REQUIRE(m_off >= 0, "power_spectrum: negative order offset %d", m_off);
    const int nrows = B * E * Cp;
    const dim3 grid((unsigned)((nrows + 63) / 64), (unsigned)L);
    if (out_dtype == MK_BF16)
        hipLaunchKernelGGL((power_kernel<u16>), grid, dim3(RNT), 0, (hipStream_t)stream, S, scale, bias, one, (u16*)out, L, M, R, Cp, C, E, E1,
                           e0, nrows, tri_off, m_off);
    else
        hipLaunchKernelGGL((power_kernel<float>), grid, dim3(RNT), 0, (hipStream_t)stream, S, scale, bias, one, (float*)out, L, M, R, Cp, C, E,
                           E1, e0, nrows, tri_off, m_off);
    return mk_check_launch("mk_power_spectrum");
}

extern "C" int mk_zonal_welford(const float* F, const float* scale, const float* bias, const float* latw, float* mean, float* m2,
                                const long long* count, int round_bf16, int M, int nlat, int R, int Cp, int B, int E, int C, int E1, int e0,
                                void* stream) {
    MK_REQUIRE(F && latw && mean && m2 && count, "zonal_welford: null pointer");
    MK_REQUIRE(M >= 1 && nlat >= 1 && nlat <= 65535 && B >= 1 && E >= 1 && C >= 1, "zonal_welford: bad shape (M %d, nlat %d, B %d, E %d, C %d)",
               M, nlat, B, E, C);
    MK_REQUIRE(Cp >= C && (long long)B * E * Cp <= R, "zonal_welford: %d x %d samples of %d rows do not fit the %d rows of F", B, E, Cp, R);
    MK_REQUIRE(e0 >= 0 && e0 + E <= E1, "zonal_welford: members [%d, %d + %d) leave the buffers' [0, %d)", e0, e0, E, E1);
    const long long nq = (long long)E * Cp;
    const int qt = zonal_rows_per_tile(nq);
    const long long tiles = (nq + qt - 1) / qt;
    MK_REQUIRE(tiles <= 65535, "zonal_welford: %d x %d rows exceed the grid", E, Cp);
    const dim3 grid((unsigned)((M + ZM - 1) / ZM), (unsigned)tiles, (unsigned)nlat);
    const size_t lds = 2 * sizeof(float) * ZM * qt;
    if (round_bf16)
        hipLaunchKernelGGL((zonal_kernel<true>), grid, dim3(RNT), lds, (hipStream_t)stream, F, scale, bias, latw, mean, m2, count, M, nlat, R,
                           Cp, C, B, E, E1, e0, qt);
    else
        hipLaunchKernelGGL((zonal_kernel<false>), grid, dim3(RNT), lds, (hipStream_t)stream, F, scale, bias, latw, mean, m2, count, M, nlat, R,
                           Cp, C, B, E, E1, e0, qt);
    return mk_check_launch("mk_zonal_welford");
}
