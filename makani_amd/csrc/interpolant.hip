// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (see escore.hip: the SLP vectoriser's packed-fp32 forms are kept out of this library; tests/test_packed_forms.py scans the ISA)
// The stochastic-interpolant stepper around the network (makani/models/stochastic_interpolant.py:102-163,343-502; Chen et al.,
// Probabilistic forecasting with stochastic interpolants and Foellmer processes), gfx950.
//
// Network input X (N, Cin, HW), channels [x0 (C) | x (C) | xu (U) | static (St) | s (1)], Cin = 2 C + U + St + has_s (the s plane is
// absent in the time-aware form).  Schedule: alpha = 1 - s, beta = s^2, sigma = eps (1 - s), gamma = sqrt(s) sigma,
// d alpha = -1, d beta = 2 s, d gamma = -eps sqrt(s).
//
//   mk_si_assemble  training: row n = b S' + j of X and of the drift target D (N, C, HW) f32 from x0, x1 (B, C, HW), z (B, C, HW) f32 and
//       s (B, S') f32 in device memory:  X[x0 slot] = x0,  X[x slot] = alpha x0 + beta x1 + gamma z,  D = -x0 + 2 s x1 - eps sqrt(s) z.
//       A thread holds x0, x1, z of its pixels of one channel and loops over j: every source element is read once.
//       The coefficients are formed from s in fp32 as two-float values and the three-term sums are compensated (si_dot3): X and D
//       are within fp32 rounding of the fp64 values, also where the terms cancel.
//       Further blocks copy xu (B, U, HW) to the S' rows of b, broadcast static (St, HW) over N and fill the s plane.
//   mk_si_step      sampling: X_next (B, Cin, HW) with x slot = cx x + cb b + c0 x0 + cn z; x is read through a pointer and a batch
//       stride (the x slot of X_prev, or x0 on step 0), b is the network output; the s plane is filled with s_next.
//       `last`: only x_new (B, C, HW) is written.  The coefficients are host values; b / z may be NULL when cb / cn = 0
//       (cx = 1 and the rest 0 writes the sampler's first input from x0 alone).
//   mk_si_step_bwd  g_x0 = g[x0 slot] + c0 g[x slot],  g_x = cx g[x slot],  g_b = cb g[x slot]  (`last`: g is the gradient of x_new and
//       has no x0 slot); each result is optional.  The xu, static and s slots carry no gradient.
//
// Grid (chunks, planes, B) with mk_plane_chunks(HW) chunks of a plane.  16-byte path (P = 4): HW a multiple of 4 and every pointer
// 16-byte aligned, so that every plane base is aligned for its element type; otherwise one pixel per thread (P = 1).  All
// element offsets are 64-bit.  Arithmetic is fp32 whatever the storage type.  No atomics, no workspace, nothing read on the host.
#include "block_io.h"

namespace {

constexpr int SNT = 256;

__device__ __forceinline__ const void* s_at(const void* base, int dt, long long e) {
    return dt == MK_BF16 ? (const void*)((const u16*)base + e) : (const void*)((const float*)base + e);
}
__device__ __forceinline__ void* s_at(void* base, int dt, long long e) {
    return dt == MK_BF16 ? (void*)((u16*)base + e) : (void*)((float*)base + e);
}

// the element type is a run-time value here
template <int P>
__device__ __forceinline__ void s_ld(const void* base, int dt, long long i, float (&v)[P]) {
    if (dt == MK_BF16) mk_ld<u16, P>((const u16*)base + i, v);
    else mk_ld<float, P>((const float*)base + i, v);
}
template <int P>
__device__ __forceinline__ void s_st(void* base, int dt, long long i, const float (&v)[P]) {
    if (dt == MK_BF16) mk_st<u16, P>((u16*)base + i, v);
    else mk_st<float, P>((float*)base + i, v);
}

// pixels [c0, c1) of chunk `chunk`: `per` is a multiple of 4
__device__ __forceinline__ void s_range(long long hw, long long per, int chunk, long long& c0, long long& c1) {
    c0 = (long long)chunk * per;
    c1 = c0 + per < hw ? c0 + per : hw;
}

// A coefficient as the unevaluated sum h + l of two floats (fp32 arithmetic throughout, the square root correctly rounded), and
// sum_k (h_k + l_k) v_k with the products split exactly by one FMA, the running sum by Knuth's two-sum and the error terms gathered
// (the dot2 of constraints.hip): the result is that of about twice the working precision (some 2^-44 relative), rounded to fp32.  An interpolant value next to
// zero between states of O(1) would otherwise carry the absolute error of the O(1) terms, several bf16 steps of the small value.
// No contraction in here: it would fuse the very roundings the error terms are taken from.
struct SiPair {
    float h, l;
};

__device__ __forceinline__ SiPair si_mul(SiPair a, SiPair b) {
#pragma clang fp contract(off)
    const float p = a.h * b.h;
    return SiPair{p, fmaf(a.h, b.h, -p) + (a.h * b.l + a.l * b.h)};
}

struct SiSched {
    SiPair al, be, ga, db, dg;
};

__device__ __forceinline__ SiSched si_schedule(float s, SiPair eps) {
#pragma clang fp contract(off)
    SiSched c;
    const float ah = 1.0f - s;
    c.al = SiPair{ah, (1.0f - ah) - s};          // (|1| >= |s|: the fast two-sum is exact)
    const float bh = s * s;
    c.be = SiPair{bh, fmaf(s, s, -bh)};
    const float rh = __fsqrt_rn(s);
    const SiPair rt{rh, rh > 0.f ? fmaf(-rh, rh, s) / (2.0f * rh) : 0.f};
    c.ga = si_mul(rt, si_mul(eps, c.al));
    c.db = SiPair{2.0f * s, 0.f};
    const SiPair er = si_mul(eps, rt);
    c.dg = SiPair{-er.h, -er.l};
    return c;
}

__device__ __forceinline__ float si_dot3(SiPair a, float x, SiPair b, float y, SiPair c, float z) {
#pragma clang fp contract(off)
    const float p1 = a.h * x, p2 = b.h * y, p3 = c.h * z;
    const float e = (fmaf(a.h, x, -p1) + a.l * x) + (fmaf(b.h, y, -p2) + b.l * y) + (fmaf(c.h, z, -p3) + c.l * z);
    const float s1 = p1 + p2, t1 = s1 - p1, r1 = (p1 - (s1 - t1)) + (p2 - t1);
    const float s2 = s1 + p3, t2 = s2 - s1, r2 = (s1 - (s2 - t2)) + (p3 - t2);
    return s2 + ((r1 + r2) + e);
}

struct SiDims {
    int C, U, St, has_s;
    long long hw, per;
};

// grid (chunks, C + U + St + has_s, B)
template <int P>
__global__ __launch_bounds__(SNT) void si_assemble_kernel(const void* __restrict__ x0, const void* __restrict__ x1, int x_dt,
                                                          const float* __restrict__ z, const float* __restrict__ s,
                                                          const void* __restrict__ xu, int xu_dt, const void* __restrict__ stat, int st_dt,
                                                          void* __restrict__ X, int out_dt, float* __restrict__ D, SiPair eps, int Sp,
                                                          SiDims d) {
    const int k = blockIdx.y, b = blockIdx.z, C = d.C;
    const long long hw = d.hw;
    const int Cin = 2 * C + d.U + d.St + d.has_s;
    long long c0, c1;
    s_range(hw, d.per, blockIdx.x, c0, c1);
    const long long n0 = (long long)b * Sp;          // first row of this batch entry
    const float* sb = s + n0;
    if (k < C) {          // (block-uniform) the interpolant and the drift of channel k
        const long long e = ((long long)b * C + k) * hw;
        const void* p0 = s_at(x0, x_dt, e);
        const void* p1 = s_at(x1, x_dt, e);
        const float* pz = z + e;
        for (long long i = c0 + (long long)threadIdx.x * P; i < c1; i += SNT * P) {
            float a[P], t[P], zz[P];
            s_ld<P>(p0, x_dt, i, a);
            s_ld<P>(p1, x_dt, i, t);
            mk_ld<float, P>(pz + i, zz);
            for (int j = 0; j < Sp; ++j) {
                const SiSched c = si_schedule(sb[j], eps);
                const SiPair m1{-1.0f, 0.f};
                float xi[P], dr[P];
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    xi[q] = si_dot3(c.al, a[q], c.be, t[q], c.ga, zz[q]);
                    dr[q] = si_dot3(m1, a[q], c.db, t[q], c.dg, zz[q]);
                }
                const long long row = (n0 + j) * Cin;
                s_st<P>(s_at(X, out_dt, (row + k) * hw), out_dt, i, a);
                s_st<P>(s_at(X, out_dt, (row + C + k) * hw), out_dt, i, xi);
                mk_st<float, P>(D + ((n0 + j) * C + k) * hw + i, dr);
            }
        }
        return;
    }
    const int ku = k - C;
    const void* src = nullptr;
    int dt = MK_F32;
    if (ku < d.U) src = s_at(xu, xu_dt, ((long long)b * d.U + ku) * hw), dt = xu_dt;
    else if (ku < d.U + d.St) src = s_at(stat, st_dt, (long long)(ku - d.U) * hw), dt = st_dt;
    const long long slot = (long long)C + k;          // behind the x0 and x slots
    for (long long i = c0 + (long long)threadIdx.x * P; i < c1; i += SNT * P) {
        float v[P];
        if (src) s_ld<P>(src, dt, i, v);
        for (int j = 0; j < Sp; ++j) {
            if (!src) {          // the s plane
                const float sv = sb[j];
#pragma unroll
                for (int q = 0; q < P; ++q) v[q] = sv;
            }
            s_st<P>(s_at(X, out_dt, ((n0 + j) * Cin + slot) * hw), out_dt, i, v);
        }
    }
}

struct SiCoef {
    float cx, cb, c0, cn, s_next;
};

// grid (chunks, last ? C : C + U + St + has_s, B).  out: X_next (B, Cin, HW), or x_new (B, C, HW) when `last`
template <int P>
__global__ __launch_bounds__(SNT) void si_step_kernel(const void* __restrict__ xp, long long xp_stride, int xp_dt, const void* __restrict__ bn,
                                                      int b_dt, const void* __restrict__ x0, int x0_dt, const float* __restrict__ z,
                                                      const void* __restrict__ xu, int xu_dt, const void* __restrict__ stat, int st_dt,
                                                      void* __restrict__ out, int out_dt, SiCoef c, int last, SiDims d) {
    const int k = blockIdx.y, b = blockIdx.z, C = d.C;
    const long long hw = d.hw;
    const int Cin = 2 * C + d.U + d.St + d.has_s;
    long long c0, c1;
    s_range(hw, d.per, blockIdx.x, c0, c1);
    if (k < C) {          // (block-uniform)
        const long long e = ((long long)b * C + k) * hw;
        const void* px = s_at(xp, xp_dt, (long long)b * xp_stride + (long long)k * hw);
        const void* pb = bn ? s_at(bn, b_dt, e) : nullptr;          // (cb = 0 without b, cn = 0 without z: the launcher checks)
        const void* p0 = s_at(x0, x0_dt, e);
        const float* pz = z ? z + e : nullptr;
        const bool need0 = !last || c.c0 != 0.0f;
        void* o0 = last ? nullptr : s_at(out, out_dt, ((long long)b * Cin + k) * hw);
        void* ox = last ? s_at(out, out_dt, e) : s_at(out, out_dt, ((long long)b * Cin + C + k) * hw);
        for (long long i = c0 + (long long)threadIdx.x * P; i < c1; i += SNT * P) {
            float xv[P], bv[P], a[P], zz[P], r[P];
            s_ld<P>(px, xp_dt, i, xv);
#pragma unroll
            for (int q = 0; q < P; ++q) a[q] = bv[q] = zz[q] = 0.f;
            if (pb) s_ld<P>(pb, b_dt, i, bv);
            if (pz) mk_ld<float, P>(pz + i, zz);
            if (need0) s_ld<P>(p0, x0_dt, i, a);
#pragma unroll
            for (int q = 0; q < P; ++q) r[q] = fmaf(c.cn, zz[q], fmaf(c.c0, a[q], fmaf(c.cb, bv[q], c.cx * xv[q])));
            if (o0) s_st<P>(o0, out_dt, i, a);
            s_st<P>(ox, out_dt, i, r);
        }
        return;
    }
    const int ku = k - C;
    const void* src = nullptr;
    int dt = MK_F32;
    if (ku < d.U) src = s_at(xu, xu_dt, ((long long)b * d.U + ku) * hw), dt = xu_dt;
    else if (ku < d.U + d.St) src = s_at(stat, st_dt, (long long)(ku - d.U) * hw), dt = st_dt;
    void* op = s_at(out, out_dt, ((long long)b * Cin + C + k) * hw);
    for (long long i = c0 + (long long)threadIdx.x * P; i < c1; i += SNT * P) {
        float v[P];
        if (src) {
            s_ld<P>(src, dt, i, v);
        } else {
#pragma unroll
            for (int q = 0; q < P; ++q) v[q] = c.s_next;
        }
        s_st<P>(op, out_dt, i, v);
    }
}

// grid (chunks, C, B).  g: (B, Cin, HW), or (B, C, HW) when `last`
template <int P>
__global__ __launch_bounds__(SNT) void si_step_bwd_kernel(const void* __restrict__ g, int g_dt, void* __restrict__ gx0, int gx0_dt,
                                                          void* __restrict__ gx, int gx_dt, void* __restrict__ gb, int gb_dt, SiCoef c,
                                                          int last, int Cin, SiDims d) {
    const int k = blockIdx.y, b = blockIdx.z, C = d.C;
    const long long hw = d.hw;
    long long c0, c1;
    s_range(hw, d.per, blockIdx.x, c0, c1);
    const long long e = ((long long)b * C + k) * hw;
    const void* g0 = last ? nullptr : s_at(g, g_dt, ((long long)b * Cin + k) * hw);
    const void* g1 = last ? s_at(g, g_dt, e) : s_at(g, g_dt, ((long long)b * Cin + C + k) * hw);
    for (long long i = c0 + (long long)threadIdx.x * P; i < c1; i += SNT * P) {
        float u[P], v[P], r[P];
        s_ld<P>(g1, g_dt, i, v);
        if (gx0) {
#pragma unroll
            for (int q = 0; q < P; ++q) u[q] = 0.f;
            if (g0) s_ld<P>(g0, g_dt, i, u);
#pragma unroll
            for (int q = 0; q < P; ++q) r[q] = fmaf(c.c0, v[q], u[q]);
            s_st<P>(s_at(gx0, gx0_dt, e), gx0_dt, i, r);
        }
        if (gx) {
#pragma unroll
            for (int q = 0; q < P; ++q) r[q] = c.cx * v[q];
            s_st<P>(s_at(gx, gx_dt, e), gx_dt, i, r);
        }
        if (gb) {
#pragma unroll
            for (int q = 0; q < P; ++q) r[q] = c.cb * v[q];
            s_st<P>(s_at(gb, gb_dt, e), gb_dt, i, r);
        }
    }
}

bool dt_ok(int dt) { return dt == MK_F32 || dt == MK_BF16; }

// the shared validation of the layout; fills d
int make_dims(const char* what, SiDims& d, int B, int C, int U, int St, int has_s, long long hw, const void* xu, int xu_dt, const void* stat,
              int st_dt) {
    MK_REQUIRE(B > 0 && B <= 65535 && C > 0, "%s: B = %d outside 1 .. 65535, or C = %d not positive", what, B, C);
    MK_REQUIRE(U >= 0 && St >= 0 && (has_s == 0 || has_s == 1), "%s: U = %d, St = %d must not be negative, has_s = %d is 0 or 1", what, U, St,
               has_s);
    MK_REQUIRE(2LL * C + U + St + has_s <= 65535, "%s: Cin = %lld exceeds the grid limit of 65535", what, 2LL * C + U + St + has_s);
    MK_REQUIRE(hw > 0, "%s: HW = %lld pixels per plane must be positive", what, hw);
    MK_REQUIRE((U == 0 || xu) && (St == 0 || stat), "%s: null pointer (U = %d unpredicted and St = %d static channels need their tensors)", what,
               U, St);
    MK_REQUIRE((U == 0 || dt_ok(xu_dt)) && (St == 0 || dt_ok(st_dt)), "%s: xu and static are f32 or bf16", what);
    const int chunks = mk_plane_chunks(hw);
    d.C = C, d.U = U, d.St = St, d.has_s = has_s, d.hw = hw;
    d.per = ((hw + chunks - 1) / chunks + 3) / 4 * 4;
    return 0;
}

}  // namespace

extern "C" int mk_si_assemble(const void* x0, const void* x1, int x_dt, const float* z, const float* s, const void* xu, int xu_dt,
                              const void* stat, int stat_dt, void* X, int out_dt, float* D, double eps_d, int B, int Sp, int C, int U, int St,
                              int has_s, long long hw, void* stream) {
    SiDims d;
    const float eps_h = (float)eps_d;
    const SiPair eps{eps_h, (float)(eps_d - (double)eps_h)};
    if (int rc = make_dims("si_assemble", d, B, C, U, St, has_s, hw, xu, xu_dt, stat, stat_dt)) return rc;
    MK_REQUIRE(Sp > 0 && (long long)B * Sp <= 2147483647LL, "si_assemble: S' = %d time samples: not positive, or B S' beyond 2^31 - 1", Sp);
    MK_REQUIRE(x0 && x1 && z && s && X && D, "si_assemble: null pointer (x0, x1, z, s, X and D are required)");
    MK_REQUIRE(dt_ok(x_dt) && dt_ok(out_dt), "si_assemble: x0 / x1 and X are f32 or bf16");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)mk_plane_chunks(hw), (unsigned)(C + U + St + has_s), (unsigned)B);
    const bool vec = hw % 4 == 0 && mk_aligned16(x0) && mk_aligned16(x1) && mk_aligned16(z) && mk_aligned16(xu) && mk_aligned16(stat) &&
                     mk_aligned16(X) && mk_aligned16(D);
    if (vec)
        hipLaunchKernelGGL((si_assemble_kernel<4>), grid, dim3(SNT), 0, st, x0, x1, x_dt, z, s, xu, xu_dt, stat, stat_dt, X, out_dt, D, eps, Sp, d);
    else
        hipLaunchKernelGGL((si_assemble_kernel<1>), grid, dim3(SNT), 0, st, x0, x1, x_dt, z, s, xu, xu_dt, stat, stat_dt, X, out_dt, D, eps, Sp, d);
    return mk_check_launch("mk_si_assemble");
}

extern "C" int mk_si_step(const void* x, long long x_stride, int x_dt, const void* b, int b_dt, const void* x0, int x0_dt, const float* z,
                          const void* xu, int xu_dt, const void* stat, int stat_dt, void* out, int out_dt, float cx, float cb, float c0,
                          float cn, float s_next, int last, int B, int C, int U, int St, int has_s, long long hw, void* stream) {
    SiDims d;
    if (last) U = St = has_s = 0;          // x_new (B, C, HW) has no feature slots
    if (int rc = make_dims("si_step", d, B, C, U, St, has_s, hw, xu, xu_dt, stat, stat_dt)) return rc;
    MK_REQUIRE(x && x0 && out, "si_step: null pointer (x, x0 and out are required)");
    MK_REQUIRE((b || cb == 0.0f) && (z || cn == 0.0f), "si_step: null pointer (b is required unless cb = 0, z unless cn = 0)");
    MK_REQUIRE(dt_ok(x_dt) && (!b || dt_ok(b_dt)) && dt_ok(x0_dt) && dt_ok(out_dt), "si_step: x, b, x0 and out are f32 or bf16");
    MK_REQUIRE(x_stride >= (long long)C * hw, "si_step: the batch stride of x, %lld elements, is below C HW = %lld", x_stride,
               (long long)C * hw);
    hipStream_t st = (hipStream_t)stream;
    const SiCoef c{cx, cb, c0, cn, s_next};
    const dim3 grid((unsigned)mk_plane_chunks(hw), (unsigned)(C + U + St + has_s), (unsigned)B);
    const bool vec = hw % 4 == 0 && x_stride % 4 == 0 && mk_aligned16(x) && mk_aligned16(b) && mk_aligned16(x0) && mk_aligned16(z) &&
                     mk_aligned16(xu) && mk_aligned16(stat) && mk_aligned16(out);
    if (vec)
        hipLaunchKernelGGL((si_step_kernel<4>), grid, dim3(SNT), 0, st, x, x_stride, x_dt, b, b_dt, x0, x0_dt, z, xu, xu_dt, stat, stat_dt, out,
                           out_dt, c, last ? 1 : 0, d);
    else
        hipLaunchKernelGGL((si_step_kernel<1>), grid, dim3(SNT), 0, st, x, x_stride, x_dt, b, b_dt, x0, x0_dt, z, xu, xu_dt, stat, stat_dt, out,
                           out_dt, c, last ? 1 : 0, d);
    return mk_check_launch("mk_si_step");
}

extern "C" int mk_si_step_bwd(const void* g, int g_dt, void* gx0, int gx0_dt, void* gx, int gx_dt, void* gb, int gb_dt, float cx, float cb,
                              float c0, int last, int B, int C, int Cin, long long hw, void* stream) {
    SiDims d;
    if (int rc = make_dims("si_step_bwd", d, B, C, 0, 0, 0, hw, nullptr, MK_F32, nullptr, MK_F32)) return rc;
    MK_REQUIRE(g && (gx0 || gx || gb), "si_step_bwd: null pointer (g and one of gx0, gx, gb are required)");
    MK_REQUIRE(dt_ok(g_dt) && (!gx0 || dt_ok(gx0_dt)) && (!gx || dt_ok(gx_dt)) && (!gb || dt_ok(gb_dt)),
               "si_step_bwd: g, gx0, gx and gb are f32 or bf16");
    MK_REQUIRE(last || (Cin >= 2 * C && Cin <= 65535), "si_step_bwd: Cin = %d is below 2 C = %d, or beyond 65535", Cin, 2 * C);
    hipStream_t st = (hipStream_t)stream;
    const SiCoef c{cx, cb, c0, 0.f, 0.f};
    const dim3 grid((unsigned)mk_plane_chunks(hw), (unsigned)C, (unsigned)B);
    const bool vec = hw % 4 == 0 && mk_aligned16(g) && mk_aligned16(gx0) && mk_aligned16(gx) && mk_aligned16(gb);
    if (vec)
        hipLaunchKernelGGL((si_step_bwd_kernel<4>), grid, dim3(SNT), 0, st, g, g_dt, gx0, gx0_dt, gx, gx_dt, gb, gb_dt, c, last ? 1 : 0, Cin, d);
    else
        hipLaunchKernelGGL((si_step_bwd_kernel<1>), grid, dim3(SNT), 0, st, g, g_dt, gx0, gx0_dt, gx, gx_dt, gb, gb_dt, c, last ? 1 : 0, Cin, d);
    return mk_check_launch("mk_si_step_bwd");
}
