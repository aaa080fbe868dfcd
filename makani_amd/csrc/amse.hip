// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (see escore.hip: the SLP vectoriser's packed-fp32 forms are kept out of this library; tests/test_packed_forms.py scans the ISA)
// Adjusted mean squared error in spectral space (SpectralAMSELoss, makani/utils/losses/amse_loss.py:29-114, arXiv:2501.19374):
// the per-degree power of prediction and target and their co-spectrum, and the gradient of whatever is built from them.
//
//   X, Y: coefficient planes (R, L, M) complex64 (re, im interleaved), R = B * C rows; wgt: optional (R, L, M) f32
//   mk_amse_sums: sums[r][l][0] = sum_m c_m w |x|^2 / 4 pi,  [1] = the same of y,  [2] = sum_m c_m w Re(x conj(y)) / 4 pi
//     c_m = 1 for the GLOBAL order m + m_off = 0 and 2 otherwise (Parseval for a real field; an azimuth shard that does not
//     hold order 0 doubles everything, :85-92); orders m > l + tri_off are structurally zero and are not read (tri_off =
//     l_off - m_off of the shard, 0 serial).
//   mk_amse_grad: with t[r][l][k] = d loss / d sums[r][l][k] (times the incoming gradient)
//     dX = c_m w / 4 pi (2 t0 x + t2 y),   dY = c_m w / 4 pi (2 t1 y + t2 x)     (torch's complex-gradient convention)
//     one pass over X and Y; dY only when asked for; exact zeros at the structurally zero orders.
// The finish of :100-110 (roots, coherence, the sum over l) works on the (B, C, L, 3) sums in torch: with a split sphere the
// sums are added over the azimuth group before it and the loss over the polar group after it.
// One wave owns one (r, l) row and walks its orders 64 at a time (coalesced float2 loads); the three sums are reduced by wave
// shuffles in a fixed order: deterministic, no atomics.
#include "common.h"

namespace {

constexpr int ANT = 256;                             // threads per block: four rows
constexpr float INV_AREA = 0.07957747154594768f;     // 1 / 4 pi

template <bool GRAD>
__global__ __launch_bounds__(ANT) void amse_kernel(const float2* __restrict__ X, const float2* __restrict__ Y, const float* __restrict__ wgt,
                                                   const float* __restrict__ t, float* __restrict__ sums, float2* __restrict__ dX,
                                                   float2* __restrict__ dY, long long rows, int L, int M, int tri_off, int m_off) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * (ANT / 64) + wave;
    if (row >= rows) return;                         // (wave-uniform; the kernel has no block barrier)
    const int l = (int)(row % L);
    const int mend = max(0, min(M, l + tri_off + 1));
    const long long base = row * M;
    if (GRAD) {
        const float t0 = t[row * 3], t1 = t[row * 3 + 1], t2 = t[row * 3 + 2];
        for (int m = lane; m < M; m += 64) {
            float2 gx = make_float2(0.f, 0.f), gy = make_float2(0.f, 0.f);
            if (m < mend) {
                const float2 x = X[base + m], y = Y[base + m];
                float cw = (m + m_off) == 0 ? INV_AREA : 2.f * INV_AREA;
                if (wgt) cw *= wgt[base + m];
                gx = make_float2(cw * (2.f * t0 * x.x + t2 * y.x), cw * (2.f * t0 * x.y + t2 * y.y));
                gy = make_float2(cw * (2.f * t1 * y.x + t2 * x.x), cw * (2.f * t1 * y.y + t2 * x.y));
            }
            dX[base + m] = gx;
            if (dY) dY[base + m] = gy;
        }
    } else {
        float a = 0.f, b = 0.f, c = 0.f;
        for (int m = lane; m < mend; m += 64) {
            const float2 x = X[base + m], y = Y[base + m];
            float cw = (m + m_off) == 0 ? INV_AREA : 2.f * INV_AREA;
            if (wgt) cw *= wgt[base + m];
            a += cw * (x.x * x.x + x.y * x.y);
            b += cw * (y.x * y.x + y.y * y.y);
            c += cw * (x.x * y.x + x.y * y.y);
        }
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_down(a, o, 64);
            b += __shfl_down(b, o, 64);
            c += __shfl_down(c, o, 64);
        }
        if (lane == 0) {
            sums[row * 3] = a;
            sums[row * 3 + 1] = b;
            sums[row * 3 + 2] = c;
        }
    }
}

bool amse_args_ok(long long R, int L, int M) { return R > 0 && L > 0 && M > 0 && (R * L + ANT / 64 - 1) / (ANT / 64) < (1ll << 31); }

}  // namespace

extern "C" int mk_amse_sums(const float* X, const float* Y, const float* wgt, float* sums, long long R, int L, int M, int tri_off, int m_off,
                            void* stream) {
    MK_REQUIRE(X && Y && sums && amse_args_ok(R, L, M), "amse_sums: bad arguments");
    const long long rows = R * L;
    hipLaunchKernelGGL((amse_kernel<false>), dim3((unsigned)((rows + ANT / 64 - 1) / (ANT / 64))), dim3(ANT), 0, (hipStream_t)stream,
                       (const float2*)X, (const float2*)Y, wgt, (const float*)nullptr, sums, (float2*)nullptr, (float2*)nullptr, rows, L, M,
                       tri_off, m_off);
    return mk_check_launch("mk_amse_sums");
}

extern "C" int mk_amse_grad(const float* X, const float* Y, const float* wgt, const float* t, float* dX, float* dY, long long R, int L, int M,
                            int tri_off, int m_off, void* stream) {
    MK_REQUIRE(X && Y && t && dX && amse_args_ok(R, L, M), "amse_grad: bad arguments");
    const long long rows = R * L;
    hipLaunchKernelGGL((amse_kernel<true>), dim3((unsigned)((rows + ANT / 64 - 1) / (ANT / 64))), dim3(ANT), 0, (hipStream_t)stream,
                       (const float2*)X, (const float2*)Y, wgt, t, (float*)nullptr, (float2*)dX, (float2*)dY, rows, L, M, tri_off, m_off);
    return mk_check_launch("mk_amse_grad");
}
