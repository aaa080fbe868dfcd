// The score of one point of the ensemble CRPS forms (makani/utils/losses/crps_loss.py:55-275), shared by csrc/crps.hip (the
// losses) and csrc/mrollout.hip (the fused validation metrics): one definition, so both score a point with the same arithmetic.
#pragma once
#include "block_io.h"

enum { CRPS_SKILLSPREAD = 0, CRPS_PWM = 1, CRPS_NAIVE = 2, CRPS_GAUSS = 3, CRPS_CDF = 4 };

static __device__ __forceinline__ float sgn(float x) { return (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f); }

// score of one point and (GRAD) its derivative with respect to every member, written back into f[].
// EM = compiled capacity, E <= EM = members present (members e >= E are ignored; callers load them as zeros).
// ew: per-member ensemble weights of the "cdf" form (nullptr = uniform)
template <int EM, bool GRAD>
__device__ __forceinline__ float crps_point(float (&f)[EM], int E, float obs, int type, float alpha, float eps,
                                            const float* __restrict__ ew) {
    const bool masked = type != CRPS_GAUSS && type != CRPS_CDF && obs != obs;      // NaN observation (gauss / cdf of the reference do not mask)
    const float o = masked ? 0.f : obs;
    const float inv_e = 1.f / (float)E;
    float skill = 0.f;
#pragma unroll
    for (int e = 0; e < EM; ++e)
        if (e < E) skill += fabsf(o - f[e]);
    skill *= inv_e;
    float score;
    float g[EM];
    if (type == CRPS_GAUSS) {
        // everything relative to the first member: f_e - f_0 is exact for close members, so the deviations from the mean keep
        // their relative accuracy.  f_e - mean(f) directly carries the rounding of the mean (half an ulp of |f|); with two
        // members 1e-3 apart around 10 that is 1e-3 of the deviation, and of the gradient's (f_e - mu) / sigma term
        const float piv = f[0];
        float md = 0.f;                // mu - piv
#pragma unroll
        for (int e = 0; e < EM; ++e)
            if (e < E) md += f[e] - piv;
        md *= inv_e;
        float var = 0.f;
#pragma unroll
        for (int e = 0; e < EM; ++e) {
            f[e] = (f[e] - piv) - md;  // from here on f holds the deviations
            if (e < E) var += f[e] * f[e];
        }
        var *= inv_e;
        const float sraw = sqrtf(var);
        const float sigma = fmaxf(sraw, eps);
        const float z = ((obs - piv) - md) / sigma;
        const float pdf = 0.3989422804014327f * __expf(-0.5f * z * z);
        const float cdf2m1 = erff(z * 0.7071067811865476f);
        score = sigma * (z * cdf2m1 + 2.f * pdf - 0.5641895835477563f);
        if (GRAD) {
            const float dmu = -cdf2m1, dsig = 2.f * pdf - 0.5641895835477563f;
#pragma unroll
            for (int e = 0; e < EM; ++e)
                g[e] = dmu * inv_e + ((sraw > eps) ? dsig * f[e] * inv_e / sigma : 0.f);
        }
    } else {
        // ordinal ranks 1..E: members smaller than f_e, plus equal members that come before e
        float acc = 0.f;               // sum_e (2 r_e - E - 1) f_e   (skillspread / naive)   or   sum_e (r_e - 1) f_e   (pwm)
        float mean = 0.f;
        float coef[EM];
        int rank[EM];
#pragma unroll
        for (int e = 0; e < EM; ++e) {
            int r = 1;
            float ssum = 0.f;          // sum_j sign(f_e - f_j)   (naive form: zero contribution from ties)
#pragma unroll
            for (int j = 0; j < EM; ++j) {
                if (j < E) {
                    r += (f[j] < f[e] || (f[j] == f[e] && j < e)) ? 1 : 0;
                    ssum += sgn(f[e] - f[j]);
                }
            }
            rank[e] = r;
            coef[e] = (type == CRPS_PWM) ? (float)(r - 1) : ((type == CRPS_NAIVE) ? ssum : (float)(2 * r - E - 1));
            if (e < E) {
                acc += coef[e] * f[e];
                mean += f[e];
            }
        }
        mean *= inv_e;
        if (type == CRPS_CDF) {
            // members (and their weights) in rank order; then the reference's loop (crps_loss.py:84-117), prev_forecast of the
            // first step is the constant 0, forecast_cdf advances by w_n / sum(w)
            float total = 0.f;
#pragma unroll
            for (int e = 0; e < EM; ++e)
                if (e < E) total += ew ? ew[e] : 1.f;
            float obs_cdf = 0.f, fc = 0.f, prev = 0.f, integ = 0.f, last = 0.f;
            float gs[EM];              // gradient with respect to the n-th sorted member
#pragma unroll
            for (int n = 0; n < EM; ++n) {
                gs[n] = 0.f;
                if (n < E) {
                    float fo = 0.f, wn = 0.f;
#pragma unroll
                    for (int e = 0; e < EM; ++e) {
                        const bool hit = e < E && rank[e] == n + 1;
                        fo = hit ? f[e] : fo;
                        wn = hit ? (ew ? ew[e] : 1.f) : wn;
                    }
                    const bool cond = (obs < fo) && fabsf(obs_cdf) < 1.0e-7f;
                    const float d = fc - obs_cdf;
                    integ += cond ? ((obs - prev) * fc * fc + (fo - obs) * (fc - 1.f) * (fc - 1.f)) : ((fo - prev) * d * d);
                    if (GRAD) {
                        gs[n] = cond ? (fc - 1.f) * (fc - 1.f) : d * d;
                        const float gp = cond ? -fc * fc : -d * d;
                        if (n > 0) gs[n - 1] += gp;
                    }
                    obs_cdf = cond ? 1.f : obs_cdf;
                    fc += wn / total;
                    prev = fo;
                    last = fo;
                }
            }
            // a NaN observation propagates (the reference's torch.clamp(observation - forecast, min=0) does; fmaxf would
            // drop it and report a finite, meaningless score): NaN score, zero gradients.  The zero gradients DEPART from the
            // reference's backward on purpose: there only the clamp term's gradient vanishes and the piecewise-integral terms still
            // hand finite, non-zero gradients to the members of a point whose score is NaN; a training step that masks NaN
            // scores would then still be pulled by those points.  Here a point without an observation moves nothing.
            const bool obs_nan = obs != obs;
            score = obs_nan ? obs : integ + fmaxf(obs - last, 0.f);
            if (GRAD) {
#pragma unroll
                for (int e = 0; e < EM; ++e) {
                    float ge = 0.f;
#pragma unroll
                    for (int n = 0; n < EM; ++n) ge = (n < E && rank[e] == n + 1) ? gs[n] : ge;
                    g[e] = obs_nan ? 0.f : ge - ((rank[e] == E && obs > last) ? 1.f : 0.f);
                }
            }
        } else if (type == CRPS_PWM) {
            const float c1 = 1.f / (float)(E * (E - 1));
            score = skill + mean - 2.f * acc * c1;
            if (GRAD) {
#pragma unroll
                for (int e = 0; e < EM; ++e) g[e] = sgn(f[e] - o) * inv_e + inv_e - 2.f * coef[e] * c1;
            }
        } else {
            // espread = 2 mean((2r - E - 1) f) (E - 1 + alpha) / (E (E - 1));  naive: sum_ij |f_i - f_j| (E - 1 + alpha) / (E^2 (E - 1))
            const float c = ((float)E - 1.f + alpha) / (float)(E * (E - 1));
            score = skill - acc * inv_e * c;
            if (GRAD) {
#pragma unroll
                for (int e = 0; e < EM; ++e) g[e] = sgn(f[e] - o) * inv_e - coef[e] * inv_e * c;
            }
        }
    }
    if (GRAD) {
#pragma unroll
        for (int e = 0; e < EM; ++e) f[e] = masked ? 0.f : g[e];
    }
    return masked ? 0.f : score;
}
