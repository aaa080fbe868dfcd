// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (see escore.hip: the SLP vectoriser's packed-fp32 forms are kept out of this library; tests/test_packed_forms.py scans the ISA)
// Gaussian negative log likelihood of an ensemble on the sphere (EnsembleNLLLoss, makani/utils/losses/likelihood_loss.py:30-134):
// the pointwise score over the ensemble dimension and the quadrature over the plane, fused (gfx950).
//
//   members f[b][e][c][p] (B, E, C, HW) f32 | bf16, read in place      observations o[b][c][p] f32
//   mu = mean_e f_e,  s2 = max(mean_e (f_e - mu)^2, eps^2)   (torch.var_mean(correction=0), torch.clamp)
//   nll = 0.5 (log s2 + (o - mu)^2 / s2)
//   out[b * C + c] = sum_p q[p] * w[b][c][p] * nll                                        (w optional)
//   gf[b][e][c][p] = gout[b * C + c] * q[p] * w * d nll / d f_e;  the clamp passes no gradient where it clamps
//
// One thread owns one point and holds its E <= 32 members in registers, as csrc/crps.hip does.  The mean comes first, then the
// centred sum of squares — never sum x^2 - (sum x)^2 / E, which cancels exactly the digits the spread of a trained ensemble
// lives in.  Everything is taken relative to the first member (f_e - f_0 is exact for close members), so the deviations keep
// their relative accuracy when the members share a large common part (the "gauss" branch of crps.hip, same reasoning).
// No NaN masks: the reference has none.  E = 1: the variance is 0, the clamp is active everywhere.
// Sums are deterministic: every block writes the sum of its chunk (wave shuffles, then the four waves in order), the caller
// adds the chunks of a plane in order.
#include "block_io.h"

namespace {

constexpr int NNT = 256;
constexpr int NMAXE = 32;

// grid: (chunks, planes = B * C).  EM: compiled capacity, members e >= E are predicated off.
template <typename TF, int EM, bool GRAD>
__global__ __launch_bounds__(NNT) void ens_nll_kernel(const TF* __restrict__ f, const float* __restrict__ obs, const float* __restrict__ q,
                                                      const float* __restrict__ w, const float* __restrict__ gout, float* __restrict__ partial,
                                                      TF* __restrict__ gf, int E, int C, long long hw, float eps2) {
    __shared__ float red[NNT / 64];
    const int plane = blockIdx.y, b = plane / C, c = plane % C;
    const long long estride = (long long)C * hw;
    const long long foff = ((long long)b * E * C + c) * hw;
    const TF* fp = f + foff;
    const float* op = obs + (long long)plane * hw;
    const float* wp = w ? w + (long long)plane * hw : nullptr;
    const float go = GRAD ? gout[plane] : 0.f;
    const float inv_e = 1.f / (float)E;
    float sum = 0.f;
    for (long long p = (long long)blockIdx.x * NNT + threadIdx.x; p < hw; p += (long long)gridDim.x * NNT) {
        float d[EM];
#pragma unroll
        for (int e = 0; e < EM; ++e) d[e] = (e < E) ? mk_ld(fp + e * estride + p) : 0.f;
        const float piv = d[0];
        float md = 0.f;                // mu - piv
#pragma unroll
        for (int e = 0; e < EM; ++e)
            if (e < E) md += d[e] - piv;
        md *= inv_e;
        float var = 0.f;
#pragma unroll
        for (int e = 0; e < EM; ++e) {
            d[e] = (d[e] - piv) - md;  // from here on d holds the deviations from the mean
            if (e < E) var += d[e] * d[e];
        }
        var *= inv_e;
        const bool clamped = var < eps2;
        const float s2 = clamped ? eps2 : var;
        const float r = (op[p] - piv) - md;
        const float inv = 1.f / s2;
        const float wt = q[p] * (wp ? wp[p] : 1.f);
        if (GRAD) {
            const float dmu = -r * inv;
            const float ds2 = clamped ? 0.f : 0.5f * (inv - r * r * inv * inv);
            const float sc = go * wt * inv_e;
            TF* gp = gf + foff;
#pragma unroll
            for (int e = 0; e < EM; ++e)
                if (e < E) mk_st(gp + e * estride + p, sc * (dmu + 2.f * ds2 * d[e]));
        } else {
            sum += wt * 0.5f * (logf(s2) + r * r * inv);
        }
    }
    if (!GRAD) {
        const float t = mk_block_sum_t0<NNT>(sum, red);
        if (threadIdx.x == 0) partial[(long long)plane * gridDim.x + blockIdx.x] = t;
    }
}

template <typename TF, bool GRAD>
int nll_launch(int E, dim3 grid, hipStream_t s, const TF* f, const float* obs, const float* q, const float* w, const float* gout, float* partial,
               TF* gf, int C, long long hw, float eps2) {
    return mk_with_capacity(E, "ens_nll", [&](auto em) {
        hipLaunchKernelGGL((ens_nll_kernel<TF, em(), GRAD>), grid, dim3(NNT), 0, s, f, obs, q, w, gout, partial, gf, E, C, hw, eps2);
        return mk_check_launch("mk_ens_nll");
    });
}

}  // namespace

extern "C" int mk_ens_nll_chunks(long long hw) { return mk_plane_chunks(hw); }

extern "C" int mk_ens_nll(const void* f, int f_dtype, const float* obs, const float* q, const float* w, const float* gout, float* partial,
                          void* gf, int B, int E, int C, long long hw, float eps, int grad, void* stream) {
    MK_REQUIRE(f && obs && q && B > 0 && E >= 1 && E <= NMAXE && C > 0 && hw > 0, "ens_nll: bad arguments (1 <= E <= 32)");
    MK_REQUIRE(grad ? (gout && gf) : (partial != nullptr), "ens_nll: missing output");
    MK_REQUIRE_PLANES("ens_nll", (long long)B * C);
    MK_REQUIRE(f_dtype == MK_F32 || f_dtype == MK_BF16, "ens_nll: members are f32 or bf16");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)mk_ens_nll_chunks(hw), (unsigned)(B * C));
    const float eps2 = (float)((double)eps * (double)eps);
    if (f_dtype == MK_F32)
        return grad ? nll_launch<float, true>(E, grid, s, (const float*)f, obs, q, w, gout, partial, (float*)gf, C, hw, eps2)
                    : nll_launch<float, false>(E, grid, s, (const float*)f, obs, q, w, gout, partial, (float*)gf, C, hw, eps2);
    return grad ? nll_launch<u16, true>(E, grid, s, (const u16*)f, obs, q, w, gout, partial, (u16*)gf, C, hw, eps2)
                : nll_launch<u16, false>(E, grid, s, (const u16*)f, obs, q, w, gout, partial, (u16*)gf, C, hw, eps2);
}
