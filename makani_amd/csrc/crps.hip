// Ensemble CRPS on the sphere: pointwise score over the ensemble dimension + quadrature over the plane, fused (gfx950).
//
// Replaces the kernels of makani/utils/losses/crps_loss.py ("skillspread" :124-162 — the default of CRPSLoss :277-452 —,
// "probability weighted moment" :164-203, "naive skillspread" :205-243, "gauss" :245-275) together with the quadrature sum
// `torch.sum(crps * quad_weight * spatial_weights, dim=-1)` (:435-438) and their autograd.
//
//   forecasts f[b][e][c][p]  (B, E, C, HW) f32 | bf16      observations o[b][c][p] (f32 | bf16)
//   out[b * C + c] = sum_p q[p] * w[b][c][p] * crps(o, f[:, p])                      (w optional)
//   gf[b][e][c][p] = gout[b * C + c] * q[p] * w * d crps / d f_e
//
// One thread owns one point: the E <= 32 members live in registers, ranks come from E^2 comparisons (ordinal ranks with the
// stable tie order of torch.argsort, as rankdata() of the reference), everything else is a handful of flops: the kernel reads
// (E + 1) values and, in backward, writes E — HBM-bound.  A NaN observation scores 0 and yields zero gradients, as the
// reference's masking does.  "cdf" (crps_loss.py:55-122, the form FourCastNet3's first pre-training stage uses,
// config/fourcastnet3.yaml:151-163): the members are put in rank order and the piecewise integral of (F - H)^2 is accumulated
// exactly as the reference's loop does (same branch conditions), optionally with per-member ensemble weights; its gradient
// is the derivative of that loop with respect to the sorted members, scattered back through the ranks.
// Ensemble sizes: every E in 2..32 — the kernels are instantiated for EM in {2, 4, 8, 16, 32} and run any E <= EM with the
// surplus members predicated off.
#include "block_io.h"
#include "crps_point.h"

namespace {

constexpr int CNT = 256;
constexpr int MAXE = 32;

// grid: (chunks, planes = B * C).  Forward: partial[plane][chunk]; backward: gf written in place of the loop.
template <typename TF, typename TO, int EM, bool GRAD>
__global__ __launch_bounds__(CNT) void crps_kernel(const TF* __restrict__ f, const TO* __restrict__ obs, const float* __restrict__ q,
                                                   const float* __restrict__ w, const float* __restrict__ gout, float* __restrict__ partial,
                                                   TF* __restrict__ gf, int E, int C, long long hw, int type, float alpha, float eps,
                                                   const float* __restrict__ ew) {
    __shared__ float red[CNT / 64];
    const int plane = blockIdx.y, b = plane / C, c = plane % C;
    const long long estride = (long long)C * hw;
    const TF* fp = f + ((long long)b * E * C + c) * hw;
    const TO* op = obs + (long long)plane * hw;
    const float* wp = w ? w + (long long)plane * hw : nullptr;
    const float go = GRAD ? gout[plane] : 0.f;
    float sum = 0.f;
    for (long long p = (long long)blockIdx.x * CNT + threadIdx.x; p < hw; p += (long long)gridDim.x * CNT) {
        float v[EM];
#pragma unroll
        for (int e = 0; e < EM; ++e) v[e] = (e < E) ? mk_ld(fp + e * estride + p) : 0.f;
        const float s = crps_point<EM, GRAD>(v, E, mk_ld(op + p), type, alpha, eps, ew);
        const float wt = q[p] * (wp ? wp[p] : 1.f);
        if (GRAD) {
            TF* gp = gf + ((long long)b * E * C + c) * hw;
#pragma unroll
            for (int e = 0; e < EM; ++e)
                if (e < E) mk_st(gp + e * estride + p, go * wt * v[e]);
        } else {
            sum += wt * s;
        }
    }
    if (!GRAD) {
        const float t = mk_block_sum_t0<CNT>(sum, red);
        if (threadIdx.x == 0) partial[(long long)plane * gridDim.x + blockIdx.x] = t;
    }
}

// "naive skillspread" on COMPLEX members (SpectralCRPSLoss(absolute=False), crps_loss.py:205-243,536-545: the score of the
// spherical-harmonic coefficients themselves instead of their absolute values): |.| is the complex modulus,
//   crps = mean_e |o - f_e| - (E - 1 + alpha) / (2 E^2 (E - 1)) sum_{i,j} |f_i - f_j|,
// gradient in torch's convention (d / d re + i d / d im; the derivative of |z| is z / |z|, 0 at z = 0).
// f: (B, E, C, hw) complex64 (re, im interleaved), obs: (B, C, hw) complex64; gf like f.
template <int EM, bool GRAD>
__global__ __launch_bounds__(CNT) void crps_cplx_kernel(const float2* __restrict__ f, const float2* __restrict__ obs,
                                                        const float* __restrict__ q, const float* __restrict__ w,
                                                        const float* __restrict__ gout, float* __restrict__ partial,
                                                        float2* __restrict__ gf, int E, int C, long long hw, float alpha) {
    __shared__ float red[CNT / 64];
    const int plane = blockIdx.y, b = plane / C, c = plane % C;
    const long long estride = (long long)C * hw;
    const float2* fp = f + ((long long)b * E * C + c) * hw;
    const float2* op = obs + (long long)plane * hw;
    const float* wp = w ? w + (long long)plane * hw : nullptr;
    const float go = GRAD ? gout[plane] : 0.f;
    const float inv_e = 1.f / (float)E;
    const float coef = ((float)E - 1.f + alpha) / (float)((long long)E * E * (E - 1));
    float sum = 0.f;
    for (long long p = (long long)blockIdx.x * CNT + threadIdx.x; p < hw; p += (long long)gridDim.x * CNT) {
        float2 v[EM];
#pragma unroll
        for (int e = 0; e < EM; ++e) v[e] = (e < E) ? fp[e * estride + p] : make_float2(0.f, 0.f);
        float2 o = op[p];
        const bool masked = (o.x != o.x) || (o.y != o.y);
        if (masked) o = make_float2(0.f, 0.f);
        // Branch-free and every unordered pair once (the two ordered pairs contribute the same distance and opposite
        // gradients): members e >= E carry the mask 0.  The first version walked the E^2 ordered pairs under `j < E && j != e`
        // and `rr > 0` branches; fully unrolled at 32 members that was 1 024 conditional blocks, and hipcc spent five of the
        // library's seven minutes of build time on this one kernel.
        float skill = 0.f, spread = 0.f;
        float2 g[EM];
        float mk[EM];
#pragma unroll
        for (int e = 0; e < EM; ++e) {
            mk[e] = (e < E) ? 1.f : 0.f;
            const float dx = v[e].x - o.x, dy = v[e].y - o.y;
            const float r = sqrtf(dx * dx + dy * dy);
            skill += mk[e] * r;
            const float ir = (GRAD && r > 0.f) ? mk[e] * inv_e / r : 0.f;
            g[e] = make_float2(dx * ir, dy * ir);
        }
#pragma unroll
        for (int e = 0; e < EM; ++e) {
#pragma unroll
            for (int j = e + 1; j < EM; ++j) {
                const float ex = v[e].x - v[j].x, ey = v[e].y - v[j].y;
                const float rr = sqrtf(ex * ex + ey * ey);
                const float m = mk[e] * mk[j];
                spread += 2.f * m * rr;
                if (GRAD) {
                    const float cr = (rr > 0.f) ? coef * m / rr : 0.f;
                    g[e].x -= cr * ex;
                    g[e].y -= cr * ey;
                    g[j].x += cr * ex;
                    g[j].y += cr * ey;
                }
            }
        }
        const float wt = q[p] * (wp ? wp[p] : 1.f);
        if (GRAD) {
            float2* gp = gf + ((long long)b * E * C + c) * hw;
#pragma unroll
            for (int e = 0; e < EM; ++e)
                if (e < E) gp[e * estride + p] = masked ? make_float2(0.f, 0.f) : make_float2(go * wt * g[e].x, go * wt * g[e].y);
        } else {
            sum += masked ? 0.f : wt * (skill * inv_e - 0.5f * coef * spread);
        }
    }
    if (!GRAD) {
        const float t = mk_block_sum_t0<CNT>(sum, red);
        if (threadIdx.x == 0) partial[(long long)plane * gridDim.x + blockIdx.x] = t;
    }
}

template <typename TF, typename TO, bool GRAD>
int launch_e(int E, dim3 grid, hipStream_t s, const TF* f, const TO* obs, const float* q, const float* w, const float* gout,
             float* partial, TF* gf, int C, long long hw, int type, float alpha, float eps, const float* ew) {
    return mk_with_capacity(E, "crps", [&](auto em) {
        hipLaunchKernelGGL((crps_kernel<TF, TO, em(), GRAD>), grid, dim3(CNT), 0, s, f, obs, q, w, gout, partial, gf, E, C, hw, type, alpha,
                           eps, ew);
        return mk_check_launch("mk_crps");
    });
}

}  // namespace

extern "C" int mk_crps_chunks(long long hw) { return mk_plane_chunks(hw); }

// grad == 0: partial (planes * mk_crps_chunks(hw)) f32 receives the chunk sums (the caller adds them up);
// grad == 1: gf (same shape and dtype as f) receives gout[plane] * q * w * dcrps/df
// ens_w: optional (E,) f32 per-member weights, used by type 4 ("cdf") only
extern "C" int mk_crps(const void* f, int f_dtype, const void* obs, int o_dtype, const float* q, const float* w, const float* gout,
                       float* partial, void* gf, int B, int E, int C, long long hw, int type, float alpha, float eps, int grad,
                       const float* ens_w, void* stream) {
    MK_REQUIRE(f && obs && q && B > 0 && E >= 2 && E <= MAXE && C > 0 && hw > 0, "crps: bad arguments (2 <= E <= 32)");
    MK_REQUIRE(type >= 0 && type <= 4, "crps: unknown score type %d", type);
    MK_REQUIRE(!ens_w || type == CRPS_CDF, "crps: ensemble weights are defined for the cdf form only");
    MK_REQUIRE(grad ? (gout && gf) : (partial != nullptr), "crps: missing output");
    MK_REQUIRE_PLANES("crps", (long long)B * C);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)mk_crps_chunks(hw), (unsigned)(B * C));
#define MK_CRPS_GO(TF, TO)                                                                                                          \
    return grad ? launch_e<TF, TO, true>(E, grid, s, (const TF*)f, (const TO*)obs, q, w, gout, partial, (TF*)gf, C, hw, type, alpha, eps, ens_w) \
                : launch_e<TF, TO, false>(E, grid, s, (const TF*)f, (const TO*)obs, q, w, gout, partial, (TF*)gf, C, hw, type, alpha, eps, ens_w)
    if (f_dtype == MK_F32 && o_dtype == MK_F32) MK_CRPS_GO(float, float);
    if (f_dtype == MK_BF16 && o_dtype == MK_F32) MK_CRPS_GO(u16, float);
    if (f_dtype == MK_BF16 && o_dtype == MK_BF16) MK_CRPS_GO(u16, u16);
    if (f_dtype == MK_F32 && o_dtype == MK_BF16) MK_CRPS_GO(float, u16);
#undef MK_CRPS_GO
    mk_set_error("crps: unsupported dtype combination");
    return MK_EINVAL;
}

// The complex "naive skillspread" score (see crps_cplx_kernel): f (B, E, C, hw) and obs (B, C, hw) complex64, q / w / gout /
// partial / gf as mk_crps (gf complex64).  2 <= E <= 32.
extern "C" int mk_crps_complex(const void* f, const void* obs, const float* q, const float* w, const float* gout, float* partial,
                               void* gf, int B, int E, int C, long long hw, float alpha, int grad, void* stream) {
    MK_REQUIRE(f && obs && q && B > 0 && E >= 2 && E <= MAXE && C > 0 && hw > 0, "crps_complex: bad arguments (2 <= E <= 32)");
    MK_REQUIRE(grad ? (gout && gf) : (partial != nullptr), "crps_complex: missing output");
    MK_REQUIRE_PLANES("crps_complex", (long long)B * C);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)mk_crps_chunks(hw), (unsigned)(B * C));
    return mk_with_capacity(E, "crps_complex", [&](auto em) {
        if (grad)
            hipLaunchKernelGGL((crps_cplx_kernel<em(), true>), grid, dim3(CNT), 0, s, (const float2*)f, (const float2*)obs, q, w, gout, partial,
                               (float2*)gf, E, C, hw, alpha);
        else
            hipLaunchKernelGGL((crps_cplx_kernel<em(), false>), grid, dim3(CNT), 0, s, (const float2*)f, (const float2*)obs, q, w, gout, partial,
                               (float2*)gf, E, C, hw, alpha);
        return mk_check_launch("mk_crps_complex");
    });
}
