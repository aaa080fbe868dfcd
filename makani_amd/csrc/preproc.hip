// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (see escore.hip: the SLP vectoriser's packed-fp32 forms are kept out of this library; tests/test_packed_forms.py scans the ISA)
// Preprocessor2D around the network (makani/models/preprocessor.py:412-687,1018-1036; makani/models/stepper.py:76-136,224-284):
// history statistics, the assembled network input, the de-normalised prediction, and their autograd (gfx950).
//
// One time level holds J = C + U + N channels: C of the window (B, T C, HW), U of the cached unpredicted features (B, T, U, HW),
// N of the noise (B, T, N, HW).  Channel (b, t, j) is read IN PLACE from whichever of the three tensors holds j; no concatenated
// intermediate exists.  omega[t][p] = wt[t] q[p], sum omega = 1.
//
//   mk_prep_stats      mu[b][j] = sum omega v,  sigma[b][j] = sqrt(sum omega (v - mu)^2)
//       A block owns pixels [c0, c1) of one (b, j) over all T levels.  Pass 1 forms W = sum omega and d = sum omega (v - K) / W
//       against a pivot K (the block's first value), pass 2 M2 = sum omega ((v - K) - d)^2 over the same pixels (the block has
//       just read them: the second pass is served by the L2).  The chunks (W, K, d, M2) of a plane are merged in chunk order by
//       Chan's formula in fp64 with mean = K + d; no sum of v^2 is ever formed, no atomics, repeats are bit-identical.
//       mu = W mean (the reference does not divide by sum omega), sigma = sqrt(M2).  tri (B, J, 3) fp64 = (W, mean, M2) is what
//       the ranks of a split sphere exchange.
//   mk_prep_assemble   out (B, T J + S, HW): channel k < T J is (v - mu[b][j]) / sigma[b][j] of (t, j) = (k / J, k % J), channel
//       k >= T J the static plane k - T J.  mu = sigma = NULL: no normalisation (mode "none", and the append / static methods).
//   mk_prep_finish     y = (yn - bias) sigma[b][c] + mu[b][c]; bias (Cout, HW), mu, sigma optional each.
//   mk_prep_bwd_sums   G[0][b][j] = gmu - (sum g) / sigma,  G[1][b][j] = gsig - (sum g xn) / sigma,  xn recomputed from v; only for
//       the channels that have a gradient tensor (`need`): the unpredicted features are never read in backward
//   mk_prep_bwd_apply  dv = g / sigma + omega (G[0] + xn G[1]); to the window, and to the noise when dnoi is given
//   mk_prep_finish_bwd gmu[b][c] = sum g,  gsig[b][c] = sum g (yn - bias)                      (d yn = g sigma is mk_prep_finish)
//
// The streaming kernels (assemble, finish, bwd_apply) cut a plane into chunks of 2048 pixels, the reduction kernels into chunks of
// 8192; mk_prep_chunks sizes the workspaces for the finer cut.
// 16-byte path (P = 4): HW a multiple of 4 and every pointer 16-byte aligned, so that every plane base is aligned for its
// element type; otherwise one pixel per thread (P = 1).  All element offsets are 64-bit.
#include "block_io.h"

namespace {

constexpr int PNT = 256;
constexpr int PPIX = 2048;          // pixels of one chunk (two 16-byte rounds of the block)
constexpr int PMAXCH = 512;
constexpr int PREDPIX = 4 * PPIX;   // pixels of one chunk of the reduction kernels: eight 16-byte rounds, four of them in flight

struct PSrc {
    const void *win, *unp, *noi;
    int win_dt, unp_dt, noi_dt;
    int T, C, U, N;
};

// plane (b, t, j) of the three sources
__device__ __forceinline__ const void* p_plane(const PSrc& s, int b, int t, int j, long long hw, int& dt) {
    const long long bt = (long long)b * s.T + t;
    if (j < s.C) {
        dt = s.win_dt;
        const long long e = (bt * s.C + j) * hw;
        return s.win_dt == MK_BF16 ? (const void*)((const u16*)s.win + e) : (const void*)((const float*)s.win + e);
    }
    if (j < s.C + s.U) {
        dt = s.unp_dt;
        const long long e = (bt * s.U + (j - s.C)) * hw;
        return s.unp_dt == MK_BF16 ? (const void*)((const u16*)s.unp + e) : (const void*)((const float*)s.unp + e);
    }
    dt = s.noi_dt;
    const long long e = (bt * s.N + (j - s.C - s.U)) * hw;
    return s.noi_dt == MK_BF16 ? (const void*)((const u16*)s.noi + e) : (const void*)((const float*)s.noi + e);
}

__device__ __forceinline__ const void* p_at(const void* base, int dt, long long e) {
    return dt == MK_BF16 ? (const void*)((const u16*)base + e) : (const void*)((const float*)base + e);
}
__device__ __forceinline__ void* p_at(void* base, int dt, long long e) {
    return dt == MK_BF16 ? (void*)((u16*)base + e) : (void*)((float*)base + e);
}

// the element type is a run-time value here
template <int P>
__device__ __forceinline__ void p_ld(const void* base, int dt, long long i, float (&v)[P]) {
    if (dt == MK_BF16) mk_ld<u16, P>((const u16*)base + i, v);
    else mk_ld<float, P>((const float*)base + i, v);
}

template <int P>
__device__ __forceinline__ void p_st(void* base, int dt, long long i, const float (&v)[P]) {
    if (dt == MK_BF16) mk_st<u16, P>((u16*)base + i, v);
    else mk_st<float, P>((float*)base + i, v);
}

// pixels [c0, c1) of chunk `chunk`: `per` is a multiple of 4
__device__ __forceinline__ void p_range(long long hw, long long per, int chunk, long long& c0, long long& c1) {
    c0 = (long long)chunk * per;
    c1 = c0 + per < hw ? c0 + per : hw;
}

// grid (chunks, B J).  partial[(plane * chunks + chunk) * 4 + {W, K, d, M2}]
template <int P>
__global__ __launch_bounds__(PNT) void prep_stats_kernel(PSrc s, const float* __restrict__ q, const float* __restrict__ wt,
                                                         float* __restrict__ partial, int J, long long hw, long long per) {
    __shared__ float red[PNT / 64];
    const int plane = blockIdx.y, b = plane / J, j = plane % J;
    long long c0, c1;
    p_range(hw, per, blockIdx.x, c0, c1);
    float* dst = partial + ((long long)plane * gridDim.x + blockIdx.x) * 4;
    if (c0 >= c1) {          // (block-uniform) an empty chunk: weight 0, skipped by the merge
        if (threadIdx.x == 0) dst[0] = dst[1] = dst[2] = dst[3] = 0.f;
        return;
    }
    int dt0;
    const void* p0 = p_plane(s, b, 0, j, hw, dt0);
    float piv[1];
    p_ld<1>(p0, dt0, c0, piv);
    const float K = piv[0];
    float W = 0.f, S = 0.f;
    for (int t = 0; t < s.T; ++t) {
        int dt;
        const void* vp = p_plane(s, b, t, j, hw, dt);
        const float wtt = wt[t];
#pragma unroll 4
        for (long long i = c0 + (long long)threadIdx.x * P; i < c1; i += PNT * P) {
            float v[P], qv[P];
            p_ld<P>(vp, dt, i, v);
            p_ld<P>(q, MK_F32, i, qv);
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const float om = wtt * qv[k];
                W += om;
                S = fmaf(om, v[k] - K, S);
            }
        }
    }
    W = mk_block_sum_all<PNT>(W, red);
    S = mk_block_sum_all<PNT>(S, red);
    const float d = W > 0.f ? S / W : 0.f;
    float M2 = 0.f;
    for (int t = 0; t < s.T; ++t) {
        int dt;
        const void* vp = p_plane(s, b, t, j, hw, dt);
        const float wtt = wt[t];
#pragma unroll 4
        for (long long i = c0 + (long long)threadIdx.x * P; i < c1; i += PNT * P) {
            float v[P], qv[P];
            p_ld<P>(vp, dt, i, v);
            p_ld<P>(q, MK_F32, i, qv);
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const float e = (v[k] - K) - d;
                M2 = fmaf(wtt * qv[k] * e, e, M2);
            }
        }
    }
    M2 = mk_block_sum_all<PNT>(M2, red);
    if (threadIdx.x == 0) dst[0] = W, dst[1] = K, dst[2] = d, dst[3] = M2;
}

// one thread per (b, j): Chan's merge of the chunks in chunk order, fp64
__global__ void prep_stats_merge_kernel(const float* __restrict__ partial, float* __restrict__ mu, float* __restrict__ sigma,
                                        double* __restrict__ tri, long long planes, int chunks) {
    const long long plane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (plane >= planes) return;
    double W = 0.0, mean = 0.0, M2 = 0.0;
    for (int ch = 0; ch < chunks; ++ch) {
        const float* p = partial + (plane * chunks + ch) * 4;
        const double w = (double)p[0];
        if (!(w > 0.0)) continue;
        const double m = (double)p[1] + (double)p[2];
        const double Wn = W + w, delta = m - mean;
        mean += delta * (w / Wn);
        M2 += (double)p[3] + delta * delta * (W * w / Wn);
        W = Wn;
    }
    if (tri) tri[plane * 3] = W, tri[plane * 3 + 1] = mean, tri[plane * 3 + 2] = M2;
    if (mu) mu[plane] = (float)(W * mean);
    if (sigma) sigma[plane] = (float)sqrt(M2);
}

// grid (chunks, T J + S, B)
template <int P>
__global__ __launch_bounds__(PNT) void prep_assemble_kernel(PSrc s, const void* __restrict__ stat, int stat_dt, const float* __restrict__ mu,
                                                            const float* __restrict__ sigma, void* __restrict__ out, int out_dt, int J, int S,
                                                            long long hw, long long per) {
    const int k = blockIdx.y, b = blockIdx.z, TJ = s.T * J;
    long long c0, c1;
    p_range(hw, per, blockIdx.x, c0, c1);
    void* op = p_at(out, out_dt, ((long long)b * (TJ + S) + k) * hw);
    const void* vp;
    int dt;
    float m = 0.f, sg = 1.f;
    bool norm = false;
    if (k < TJ) {
        const int t = k / J, j = k % J;
        vp = p_plane(s, b, t, j, hw, dt);
        if (mu) m = mu[(long long)b * J + j], sg = sigma[(long long)b * J + j], norm = true;
    } else {
        dt = stat_dt;
        vp = p_at(stat, stat_dt, (long long)(k - TJ) * hw);
    }
    for (long long i = c0 + (long long)threadIdx.x * P; i < c1; i += PNT * P) {
        float v[P];
        p_ld<P>(vp, dt, i, v);
        if (norm) {
#pragma unroll
            for (int e = 0; e < P; ++e) v[e] = (v[e] - m) / sg;
        }
        p_st<P>(op, out_dt, i, v);
    }
}

// grid (chunks, Cout, B).  stat index b * J + c
template <int P>
__global__ __launch_bounds__(PNT) void prep_finish_kernel(const void* __restrict__ yn, int dt, const float* __restrict__ bias,
                                                          const float* __restrict__ mu, const float* __restrict__ sigma, void* __restrict__ y,
                                                          int J, long long hw, long long per) {
    const int c = blockIdx.y, b = blockIdx.z, Cout = gridDim.y;
    long long c0, c1;
    p_range(hw, per, blockIdx.x, c0, c1);
    const long long e0 = ((long long)b * Cout + c) * hw;
    const void* xp = p_at(yn, dt, e0);
    void* yp = p_at(y, dt, e0);
    const float* bp = bias ? bias + (long long)c * hw : nullptr;
    const float m = mu ? mu[(long long)b * J + c] : 0.f, sg = sigma ? sigma[(long long)b * J + c] : 1.f;
    for (long long i = c0 + (long long)threadIdx.x * P; i < c1; i += PNT * P) {
        float v[P], bv[P];
        p_ld<P>(xp, dt, i, v);
        if (bp) {
            p_ld<P>(bp, MK_F32, i, bv);
#pragma unroll
            for (int e = 0; e < P; ++e) v[e] -= bv[e];
        }
        if (sigma || mu) {
#pragma unroll
            for (int e = 0; e < P; ++e) v[e] = fmaf(v[e], sg, m);
        }
        p_st<P>(yp, dt, i, v);
    }
}

// grid (chunks, B J).  partial[(plane * chunks + chunk) * 2 + {sum g, sum g xn}];  g (B, T J + S, HW).  need: bit 0 the window's
// channels, bit 1 the noise channels; the others (and the unpredicted channels always) are not read and give zero sums
template <int P>
__global__ __launch_bounds__(PNT) void prep_bwd_sums_kernel(const void* __restrict__ g, int g_dt, PSrc s, const float* __restrict__ mu,
                                                            const float* __restrict__ sigma, float* __restrict__ partial, int J, int S,
                                                            int need, long long hw, long long per) {
    __shared__ float red[PNT / 64];
    const int plane = blockIdx.y, b = plane / J, j = plane % J;
    if (!(j < s.C ? (need & 1) : (j >= s.C + s.U ? (need & 2) : 0))) {          // (block-uniform) no gradient tensor behind channel j
        if (threadIdx.x == 0) {
            float* dst = partial + ((long long)plane * gridDim.x + blockIdx.x) * 2;
            dst[0] = dst[1] = 0.f;
        }
        return;
    }
    long long c0, c1;
    p_range(hw, per, blockIdx.x, c0, c1);
    const float m = mu[plane], sg = sigma[plane];
    float A = 0.f, X = 0.f;
    for (int t = 0; t < s.T; ++t) {
        int dt;
        const void* vp = p_plane(s, b, t, j, hw, dt);
        const void* gp = p_at(g, g_dt, ((long long)b * (s.T * J + S) + (long long)t * J + j) * hw);
#pragma unroll 4
        for (long long i = c0 + (long long)threadIdx.x * P; i < c1; i += PNT * P) {
            float v[P], gv[P];
            p_ld<P>(vp, dt, i, v);
            p_ld<P>(gp, g_dt, i, gv);
#pragma unroll
            for (int e = 0; e < P; ++e) {
                A += gv[e];
                X = fmaf(gv[e], (v[e] - m) / sg, X);
            }
        }
    }
    A = mk_block_sum_all<PNT>(A, red);
    X = mk_block_sum_all<PNT>(X, red);
    if (threadIdx.x == 0) {
        float* dst = partial + ((long long)plane * gridDim.x + blockIdx.x) * 2;
        dst[0] = A, dst[1] = X;
    }
}

// grid (chunks, B Cin).  partial as above with sum g, sum g (yn - bias);  plane = b * Cin + c
template <int P>
__global__ __launch_bounds__(PNT) void prep_finish_bwd_kernel(const void* __restrict__ g, int g_dt, const void* __restrict__ yn, int yn_dt,
                                                              const float* __restrict__ bias, float* __restrict__ partial, int Cin, long long hw,
                                                              long long per) {
    __shared__ float red[PNT / 64];
    const int plane = blockIdx.y, c = plane % Cin;
    long long c0, c1;
    p_range(hw, per, blockIdx.x, c0, c1);
    const void* gp = p_at(g, g_dt, (long long)plane * hw);
    const void* xp = p_at(yn, yn_dt, (long long)plane * hw);
    const float* bp = bias ? bias + (long long)c * hw : nullptr;
    float A = 0.f, X = 0.f;
#pragma unroll 4
    for (long long i = c0 + (long long)threadIdx.x * P; i < c1; i += PNT * P) {
        float v[P], gv[P], bv[P];
        p_ld<P>(xp, yn_dt, i, v);
        p_ld<P>(gp, g_dt, i, gv);
        if (bp) p_ld<P>(bp, MK_F32, i, bv);
#pragma unroll
        for (int e = 0; e < P; ++e) {
            A += gv[e];
            X = fmaf(gv[e], bp ? v[e] - bv[e] : v[e], X);
        }
    }
    A = mk_block_sum_all<PNT>(A, red);
    X = mk_block_sum_all<PNT>(X, red);
    if (threadIdx.x == 0) {
        float* dst = partial + ((long long)plane * gridDim.x + blockIdx.x) * 2;
        dst[0] = A, dst[1] = X;
    }
}

// one thread per (b, c < Cin): the chunks of the plane in chunk order (fp64), written to index b * J + c.
// sigma given (normalisation): out0 = add0 - A / sigma, out1 = add1 - X / sigma;  otherwise out0 = A, out1 = X.
__global__ void prep_sums_finish_kernel(const float* __restrict__ partial, const float* __restrict__ sigma, const float* __restrict__ add0,
                                        const float* __restrict__ add1, float* __restrict__ out0, float* __restrict__ out1, long long planes,
                                        int chunks, int Cin, int J) {
    const long long plane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (plane >= planes) return;
    double A = 0.0, X = 0.0;
    for (int ch = 0; ch < chunks; ++ch) {
        A += (double)partial[(plane * chunks + ch) * 2];
        X += (double)partial[(plane * chunks + ch) * 2 + 1];
    }
    const long long idx = (plane / Cin) * J + plane % Cin;
    if (sigma) {
        const double sg = (double)sigma[idx];
        out0[idx] = (float)((add0 ? (double)add0[idx] : 0.0) - A / sg);
        out1[idx] = (float)((add1 ? (double)add1[idx] : 0.0) - X / sg);
    } else {
        out0[idx] = (float)A;
        out1[idx] = (float)X;
    }
}

// grid (chunks, T J, B).  G (2, B, J) or NULL; g (B, T J + S, HW) or NULL; mu = sigma = NULL: no normalisation (dv = g)
template <int P>
__global__ __launch_bounds__(PNT) void prep_bwd_apply_kernel(const void* __restrict__ g, int g_dt, PSrc s, const float* __restrict__ q,
                                                             const float* __restrict__ wt, const float* __restrict__ mu,
                                                             const float* __restrict__ sigma, const float* __restrict__ G, void* __restrict__ dwin,
                                                             void* __restrict__ dnoi, int B, int J, int S, long long hw, long long per) {
    const int k = blockIdx.y, b = blockIdx.z, t = k / J, j = k % J;
    void* dp;
    int d_dt;
    const long long bt = (long long)b * s.T + t;
    if (j < s.C) {          // (block-uniform) only planes with a gradient tensor are written
        if (!dwin) return;
        d_dt = s.win_dt;
        dp = p_at(dwin, d_dt, (bt * s.C + j) * hw);
    } else if (j >= s.C + s.U) {
        if (!dnoi) return;
        d_dt = s.noi_dt;
        dp = p_at(dnoi, d_dt, (bt * s.N + (j - s.C - s.U)) * hw);
    } else {
        return;
    }
    long long c0, c1;
    p_range(hw, per, blockIdx.x, c0, c1);
    int dt;
    const void* vp = p_plane(s, b, t, j, hw, dt);
    const void* gp = g ? p_at(g, g_dt, ((long long)b * (s.T * J + S) + k) * hw) : nullptr;
    const bool norm = mu != nullptr;
    const float m = norm ? mu[(long long)b * J + j] : 0.f, sg = norm ? sigma[(long long)b * J + j] : 1.f;
    const float Gm = G ? G[(long long)b * J + j] : 0.f, Gs = G ? G[((long long)B + b) * J + j] : 0.f;
    const float wtt = G ? wt[t] : 0.f;
    for (long long i = c0 + (long long)threadIdx.x * P; i < c1; i += PNT * P) {
        float v[P], gv[P], qv[P], r[P];
#pragma unroll
        for (int e = 0; e < P; ++e) r[e] = 0.f;
        if (gp) {
            p_ld<P>(gp, g_dt, i, gv);
#pragma unroll
            for (int e = 0; e < P; ++e) r[e] = norm ? gv[e] / sg : gv[e];
        }
        if (G) {
            p_ld<P>(vp, dt, i, v);
            p_ld<P>(q, MK_F32, i, qv);
#pragma unroll
            for (int e = 0; e < P; ++e) r[e] = fmaf(wtt * qv[e], fmaf((v[e] - m) / sg, Gs, Gm), r[e]);
        }
        p_st<P>(dp, d_dt, i, r);
    }
}

bool dt_ok(int dt) { return dt == MK_F32 || dt == MK_BF16; }

// the reduction kernels take four chunks of the streaming kernels at a time (their workspaces, sized with mk_prep_chunks, hold more)
int red_chunks(long long hw) {
    const long long c = (hw + PREDPIX - 1) / PREDPIX;
    return (int)(c < 1 ? 1 : (c > PMAXCH ? PMAXCH : c));
}

long long per_chunk(long long hw, int chunks) {
    const long long per = (hw + chunks - 1) / chunks;
    return (per + 3) / 4 * 4;
}

// the shared validation of the source description; fills s and J
int make_src(const char* what, PSrc& s, int& J, const void* win, int win_dt, const void* unp, int unp_dt, const void* noi, int noi_dt, int B,
             int T, int WC, int U, int N, long long hw, bool need_unp = true, bool need_noi = true) {
    MK_REQUIRE(B > 0 && T > 0, "%s: B = %d, T = n_history + 1 = %d must be positive", what, B, T);
    MK_REQUIRE(WC > 0 && WC % T == 0, "%s: the window has %d channels, not a positive multiple of T = %d", what, WC, T);
    MK_REQUIRE(U >= 0 && N >= 0, "%s: U = %d, N = %d must not be negative", what, U, N);
    MK_REQUIRE(hw > 0, "%s: HW = %lld pixels per plane must be positive", what, hw);
    MK_REQUIRE(win, "%s: null pointer (the window is required)", what);
    MK_REQUIRE((U == 0 || unp || !need_unp) && (N == 0 || noi || !need_noi), "%s: null pointer (U = %d unpredicted and N = %d noise channels need their tensors)", what,
               U, N);
    MK_REQUIRE(dt_ok(win_dt) && (U == 0 || !unp || dt_ok(unp_dt)) && (N == 0 || !noi || dt_ok(noi_dt)), "%s: the sources are f32 or bf16",
               what);
    s.win = win, s.unp = unp, s.noi = noi;
    s.win_dt = win_dt, s.unp_dt = unp_dt, s.noi_dt = noi_dt;
    s.T = T, s.C = WC / T, s.U = U, s.N = N;
    J = s.C + U + N;
    MK_REQUIRE((long long)B * J <= 65535 && (long long)T * J <= 65535, "%s: B J = %lld or T J = %lld exceed the grid limit of 65535", what,
               (long long)B * J, (long long)T * J);
    return 0;
}

bool src_vec(const PSrc& s, long long hw) { return hw % 4 == 0 && mk_aligned16(s.win) && mk_aligned16(s.unp) && mk_aligned16(s.noi); }

}  // namespace

extern "C" int mk_prep_chunks(long long hw) {
    const long long c = (hw + PPIX - 1) / PPIX;
    return (int)(c < 1 ? 1 : (c > PMAXCH ? PMAXCH : c));
}

extern "C" int mk_prep_stats(const void* win, int win_dt, const void* unp, int unp_dt, const void* noi, int noi_dt, const float* q,
                             const float* wt, float* mu, float* sigma, double* tri, float* ws, int B, int T, int WC, int U, int N, long long hw,
                             void* stream) {
    PSrc s;
    int J;
    if (int rc = make_src("prep_stats", s, J, win, win_dt, unp, unp_dt, noi, noi_dt, B, T, WC, U, N, hw)) return rc;
    MK_REQUIRE(q && wt && ws, "prep_stats: null pointer (q, wt and ws are required)");
    MK_REQUIRE((mu && sigma) || tri, "prep_stats: null pointer (mu and sigma, or tri, are required)");
    hipStream_t st = (hipStream_t)stream;
    const int chunks = red_chunks(hw);
    const long long per = per_chunk(hw, chunks);
    const dim3 grid((unsigned)chunks, (unsigned)(B * J));
    if (src_vec(s, hw) && mk_aligned16(q))
        hipLaunchKernelGGL((prep_stats_kernel<4>), grid, dim3(PNT), 0, st, s, q, wt, ws, J, hw, per);
    else
        hipLaunchKernelGGL((prep_stats_kernel<1>), grid, dim3(PNT), 0, st, s, q, wt, ws, J, hw, per);
    if (int rc = mk_check_launch("mk_prep_stats")) return rc;
    const long long planes = (long long)B * J;
    hipLaunchKernelGGL(prep_stats_merge_kernel, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, st, ws, mu, sigma, tri, planes, chunks);
    return mk_check_launch("mk_prep_stats");
}

extern "C" int mk_prep_assemble(const void* win, int win_dt, const void* unp, int unp_dt, const void* noi, int noi_dt, const void* stat,
                                int stat_dt, const float* mu, const float* sigma, void* out, int out_dt, int B, int T, int WC, int U, int N,
                                int S, long long hw, void* stream) {
    PSrc s;
    int J;
    if (int rc = make_src("prep_assemble", s, J, win, win_dt, unp, unp_dt, noi, noi_dt, B, T, WC, U, N, hw)) return rc;
    MK_REQUIRE(S >= 0 && (long long)T * J + S <= 65535, "prep_assemble: S = %d static channels: negative, or T J + S beyond 65535", S);
    MK_REQUIRE(out && (S == 0 || stat), "prep_assemble: null pointer (out, and the static planes when S > 0, are required)");
    MK_REQUIRE(dt_ok(out_dt) && (S == 0 || dt_ok(stat_dt)), "prep_assemble: out and the static planes are f32 or bf16");
    MK_REQUIRE((mu == nullptr) == (sigma == nullptr), "prep_assemble: mu and sigma come together");
    MK_REQUIRE(B <= 65535, "prep_assemble: B = %d exceeds the grid limit of 65535", B);
    hipStream_t st = (hipStream_t)stream;
    const int chunks = mk_prep_chunks(hw);
    const long long per = per_chunk(hw, chunks);
    const dim3 grid((unsigned)chunks, (unsigned)(T * J + S), (unsigned)B);
    if (src_vec(s, hw) && mk_aligned16(stat) && mk_aligned16(out))
        hipLaunchKernelGGL((prep_assemble_kernel<4>), grid, dim3(PNT), 0, st, s, stat, stat_dt, mu, sigma, out, out_dt, J, S, hw, per);
    else
        hipLaunchKernelGGL((prep_assemble_kernel<1>), grid, dim3(PNT), 0, st, s, stat, stat_dt, mu, sigma, out, out_dt, J, S, hw, per);
    return mk_check_launch("mk_prep_assemble");
}

extern "C" int mk_prep_finish(const void* yn, int dtype, const float* bias, const float* mu, const float* sigma, void* y, int B, int Cout, int J,
                              long long hw, void* stream) {
    MK_REQUIRE(yn && y, "prep_finish: null pointer (yn and y are required)");
    MK_REQUIRE(dt_ok(dtype), "prep_finish: yn is f32 or bf16");
    MK_REQUIRE(B > 0 && B <= 65535 && Cout > 0 && Cout <= 65535, "prep_finish: B = %d, Cout = %d outside 1 .. 65535", B, Cout);
    MK_REQUIRE(J >= Cout, "prep_finish: the statistics have J = %d channels, fewer than Cout = %d", J, Cout);
    MK_REQUIRE(hw > 0, "prep_finish: HW = %lld pixels per plane must be positive", hw);
    hipStream_t st = (hipStream_t)stream;
    const int chunks = mk_prep_chunks(hw);
    const long long per = per_chunk(hw, chunks);
    const dim3 grid((unsigned)chunks, (unsigned)Cout, (unsigned)B);
    if (hw % 4 == 0 && mk_aligned16(yn) && mk_aligned16(y) && mk_aligned16(bias))
        hipLaunchKernelGGL((prep_finish_kernel<4>), grid, dim3(PNT), 0, st, yn, dtype, bias, mu, sigma, y, J, hw, per);
    else
        hipLaunchKernelGGL((prep_finish_kernel<1>), grid, dim3(PNT), 0, st, yn, dtype, bias, mu, sigma, y, J, hw, per);
    return mk_check_launch("mk_prep_finish");
}

extern "C" int mk_prep_bwd_sums(const void* g, int g_dt, const void* win, int win_dt, const void* unp, int unp_dt, const void* noi, int noi_dt,
                                const float* mu, const float* sigma, const float* gmu, const float* gsig, float* G, float* ws, int B, int T,
                                int WC, int U, int N, int S, int need, long long hw, void* stream) {
    PSrc s;
    int J;
    MK_REQUIRE(need > 0 && need < 4, "prep_bwd_sums: need = %d names no gradient (bit 0 window, bit 1 noise)", need);
    if (int rc = make_src("prep_bwd_sums", s, J, win, win_dt, unp, unp_dt, noi, noi_dt, B, T, WC, U, N, hw, false, (need & 2) != 0)) return rc;
    MK_REQUIRE(S >= 0, "prep_bwd_sums: S = %d static channels must not be negative", S);
    MK_REQUIRE(g && mu && sigma && G && ws, "prep_bwd_sums: null pointer (g, mu, sigma, G and ws are required)");
    MK_REQUIRE(dt_ok(g_dt), "prep_bwd_sums: g is f32 or bf16");
    hipStream_t st = (hipStream_t)stream;
    const int chunks = red_chunks(hw);
    const long long per = per_chunk(hw, chunks);
    const dim3 grid((unsigned)chunks, (unsigned)(B * J));
    if (src_vec(s, hw) && mk_aligned16(g))
        hipLaunchKernelGGL((prep_bwd_sums_kernel<4>), grid, dim3(PNT), 0, st, g, g_dt, s, mu, sigma, ws, J, S, need, hw, per);
    else
        hipLaunchKernelGGL((prep_bwd_sums_kernel<1>), grid, dim3(PNT), 0, st, g, g_dt, s, mu, sigma, ws, J, S, need, hw, per);
    if (int rc = mk_check_launch("mk_prep_bwd_sums")) return rc;
    const long long planes = (long long)B * J;
    hipLaunchKernelGGL(prep_sums_finish_kernel, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, st, ws, sigma, gmu, gsig, G, G + planes,
                       planes, chunks, J, J);
    return mk_check_launch("mk_prep_bwd_sums");
}

extern "C" int mk_prep_bwd_apply(const void* g, int g_dt, const void* win, int win_dt, const void* unp, int unp_dt, const void* noi, int noi_dt,
                                 const float* q, const float* wt, const float* mu, const float* sigma, const float* G, void* dwin, void* dnoi,
                                 int B, int T, int WC, int U, int N, int S, long long hw, void* stream) {
    PSrc s;
    int J;
    if (int rc = make_src("prep_bwd_apply", s, J, win, win_dt, unp, unp_dt, noi, noi_dt, B, T, WC, U, N, hw, false, dnoi != nullptr)) return rc;
    MK_REQUIRE(S >= 0, "prep_bwd_apply: S = %d static channels must not be negative", S);
    MK_REQUIRE(g || G, "prep_bwd_apply: null pointer (g or G is required)");
    MK_REQUIRE(dwin || dnoi, "prep_bwd_apply: null pointer (dwin or dnoi is required)");
    MK_REQUIRE(!dnoi || N > 0, "prep_bwd_apply: a noise gradient without noise channels");
    MK_REQUIRE(!g || dt_ok(g_dt), "prep_bwd_apply: g is f32 or bf16");
    MK_REQUIRE((mu == nullptr) == (sigma == nullptr), "prep_bwd_apply: mu and sigma come together");
    MK_REQUIRE(!G || (mu && q && wt), "prep_bwd_apply: null pointer (G needs mu, sigma, q and wt)");
    MK_REQUIRE(B <= 65535, "prep_bwd_apply: B = %d exceeds the grid limit of 65535", B);
    hipStream_t st = (hipStream_t)stream;
    const int chunks = mk_prep_chunks(hw);
    const long long per = per_chunk(hw, chunks);
    const dim3 grid((unsigned)chunks, (unsigned)(T * J), (unsigned)B);
    if (src_vec(s, hw) && mk_aligned16(g) && mk_aligned16(q) && mk_aligned16(dwin) && mk_aligned16(dnoi))
        hipLaunchKernelGGL((prep_bwd_apply_kernel<4>), grid, dim3(PNT), 0, st, g, g_dt, s, q, wt, mu, sigma, G, dwin, dnoi, B, J, S, hw, per);
    else
        hipLaunchKernelGGL((prep_bwd_apply_kernel<1>), grid, dim3(PNT), 0, st, g, g_dt, s, q, wt, mu, sigma, G, dwin, dnoi, B, J, S, hw, per);
    return mk_check_launch("mk_prep_bwd_apply");
}

extern "C" int mk_prep_finish_bwd(const void* g, int g_dt, const void* yn, int yn_dt, const float* bias, float* gmu, float* gsig, float* ws,
                                  int B, int Cout, int J, long long hw, void* stream) {
    MK_REQUIRE(g && yn && gmu && gsig && ws, "prep_finish_bwd: null pointer (g, yn, gmu, gsig and ws are required)");
    MK_REQUIRE(dt_ok(g_dt) && dt_ok(yn_dt), "prep_finish_bwd: g and yn are f32 or bf16");
    MK_REQUIRE(B > 0 && Cout > 0 && (long long)B * Cout <= 65535, "prep_finish_bwd: B = %d, Cout = %d: not positive, or B Cout beyond 65535", B,
               Cout);
    MK_REQUIRE(J >= Cout, "prep_finish_bwd: the statistics have J = %d channels, fewer than Cout = %d", J, Cout);
    MK_REQUIRE(hw > 0, "prep_finish_bwd: HW = %lld pixels per plane must be positive", hw);
    hipStream_t st = (hipStream_t)stream;
    const int chunks = red_chunks(hw);
    const long long per = per_chunk(hw, chunks);
    const dim3 grid((unsigned)chunks, (unsigned)(B * Cout));
    if (hw % 4 == 0 && mk_aligned16(g) && mk_aligned16(yn) && mk_aligned16(bias))
        hipLaunchKernelGGL((prep_finish_bwd_kernel<4>), grid, dim3(PNT), 0, st, g, g_dt, yn, yn_dt, bias, ws, Cout, hw, per);
    else
        hipLaunchKernelGGL((prep_finish_bwd_kernel<1>), grid, dim3(PNT), 0, st, g, g_dt, yn, yn_dt, bias, ws, Cout, hw, per);
    if (int rc = mk_check_launch("mk_prep_finish_bwd")) return rc;
    const long long planes = (long long)B * Cout;
    hipLaunchKernelGGL(prep_sums_finish_kernel, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, st, ws, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, gmu, gsig, planes, chunks, Cout, J);
    return mk_check_launch("mk_prep_finish_bwd");
}
