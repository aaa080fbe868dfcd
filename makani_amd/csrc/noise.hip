// MK_HIPCC_FLAGS: -fno-slp-vectorize
// Spectral noise processes on the sphere (makani/models/noise.py: BaseNoiseS2.update, DiffusionNoiseS2.update,
// DummyNoiseS2 "constant_random"): draw standard normals and apply the state update in ONE pass over the state, in place.
// The reference's torch formulation (normal_, 3-5 element-wise passes, cat / einsum over the history, copy_) moves 7-10
// state-sized transfers; this kernel reads the state at most once and writes it once.
//
// Generator: Philox4x32-10, counter-based, no state in the kernel.  rng = device int64 {seed, offset}.
//   key     = (seed_lo, seed_hi)
//   counter = (g_lo, g_hi, offset_lo, offset_hi);  g = index of a group of four consecutive fp32 elements of ONE drawn time
//             level, flattened in the reference's memory order (B, C, L, M, 2); a partial tail group uses its leading outputs.
//   One time level consumes one offset: level t of a T-level draw uses offset + t.  The update kernel only READS rng;
//   mk_noise_advance (one thread, enqueued behind it on the same stream) adds to the offset, so the pair is stream-ordered
//   and replays from a captured graph.
// Normals: Box-Muller on exactly representable uniforms, u1 = ((x0 >> 8) + 1) 2^-24 in (0, 1], u2 = (x1 >> 8) 2^-24 in [0, 1):
//   r = sqrt(-2 ln u1), z0 = r cospi(2 u2), z1 = r sinpi(2 u2); (x2, x3) -> (z2, z3).  |z| <= sqrt(48 ln 2) = 5.77.
//   logf / sincospif are the accurate library forms, so an fp64 restatement from the same u agrees to fp32 rounding.
//
// One thread owns its four elements across all T time levels: every mode is in place without a cross-thread hazard.
#include "common.h"

namespace {
constexpr int NT = 256;

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t* out) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float& za, float& zb) {
    const float u1 = (float)((xa >> 8) + 1u) * 0x1p-24f;       // exact: 24-bit integers
    const float u2 = (float)(xb >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    za = r * c;
    zb = r * s;
}

// four standard normals of group g at `offset`
__device__ __forceinline__ void draw4(unsigned long long g, unsigned long long offset, unsigned long long seed, float* z) {
    uint32_t x[4];
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), x);
    box_muller(x[0], x[1], z[0], z[1]);
    box_muller(x[2], x[3], z[2], z[3]);
}

template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, const long long* off, const bool* ok, float* v) {
    if (VEC) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(p + off[0]);
        v[0] = x[0], v[1] = x[1], v[2] = x[2], v[3] = x[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ok[j] ? p[off[j]] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, const long long* off, const bool* ok, const float* v) {
    if (VEC) {
        *reinterpret_cast<f32x4*>(p + off[0]) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ok[j]) p[off[j]] = v[j];
    }
}

// state (B, T, C, L, M, 2) f32, updated in place.  xi: optional innovations instead of drawn ones, (B, xT, C, L, M, 2) with
// xT = 1 for MK_NOISE_AR and T otherwise.  sigma (C, L), phi (C).  clm2 = C L M 2 elements per (batch entry, time level).
// VEC: clm2 % 4 == 0 and 16-byte aligned pointers -> a group never leaves its batch entry; grid = (groups per entry, B).
// Otherwise grid = groups of the whole level, every element finds its own batch entry, channel and degree.
template <int MODE, bool VEC>
__global__ __launch_bounds__(NT) void noise_update_kernel(float* __restrict__ state, const float* __restrict__ xi,
                                                          const float* __restrict__ sigma, const float* __restrict__ phi,
                                                          const long long* __restrict__ rng, int B, int T, int L, int M,
                                                          unsigned clm2, float sgn) {
    const int xT = MODE == MK_NOISE_AR ? 1 : T;
    const unsigned m2 = 2u * (unsigned)M;
    unsigned long long g;
    long long off[4], xoff[4];
    bool ok[4];
    float sg[4], ph[4];
    if (VEC) {
        const unsigned gpb = clm2 >> 2;                             // groups per batch entry
        const unsigned gi = blockIdx.x * NT + threadIdx.x;
        if (gi >= gpb) return;
        const unsigned b = blockIdx.y;
        g = (unsigned long long)b * gpb + gi;
        const unsigned rem = gi * 4u;
        off[0] = (long long)b * T * clm2 + rem;
        xoff[0] = (long long)b * xT * clm2 + rem;
        if (MODE != MK_NOISE_WHITE) {
            // elements 0, 1 are one coefficient (re, im), elements 2, 3 the next one: possibly the next degree or channel
            const unsigned q = rem / m2, r = rem - q * m2;
            unsigned c = q / (unsigned)L, l = q - c * (unsigned)L;
            sg[0] = sg[1] = sigma[c * L + l], ph[0] = ph[1] = phi[c];
            if (r + 2u >= m2) {
                if (++l == (unsigned)L) l = 0, ++c;
            }
            sg[2] = sg[3] = sigma[c * L + l], ph[2] = ph[3] = phi[c];
        }
    } else {
        g = (unsigned long long)blockIdx.x * NT + threadIdx.x;
        const long long n1 = (long long)B * clm2;
        if ((long long)(4ull * g) >= n1) return;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long e = (long long)(4ull * g) + j;
            ok[j] = e < n1;
            const long long b = ok[j] ? e / clm2 : 0;
            const unsigned rem = ok[j] ? (unsigned)(e - b * clm2) : 0u;
            off[j] = b * T * clm2 + rem;
            xoff[j] = b * xT * clm2 + rem;
            if (MODE != MK_NOISE_WHITE) {
                const unsigned q = rem / m2;
                const unsigned c = q / (unsigned)L, l = q - c * (unsigned)L;
                sg[j] = sigma[c * L + l], ph[j] = phi[c];
            }
        }
    }
    unsigned long long seed = 0, offset = 0;
    if (!xi) seed = (unsigned long long)rng[0], offset = (unsigned long long)rng[1];

    float z[4], v[4];
    if (MODE == MK_NOISE_WHITE) {
        for (int t = 0; t < T; ++t) {
            if (xi) load4<VEC>(xi + (long long)t * clm2, xoff, ok, z);
            else draw4(g, offset + (unsigned long long)t, seed, z);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = sgn * z[j];
            store4<VEC>(state + (long long)t * clm2, off, ok, v);
        }
    } else if (MODE == MK_NOISE_AR) {
        // levels 1 .. T-1 move down to 0 .. T-2; the new last level continues the old last one
        for (int t = 0; t + 1 < T; ++t) {
            load4<VEC>(state + (long long)(t + 1) * clm2, off, ok, v);
            store4<VEC>(state + (long long)t * clm2, off, ok, v);
        }
        if (T == 1) load4<VEC>(state, off, ok, v);               // (T > 1: v holds the old last level)
        if (xi) load4<VEC>(xi, xoff, ok, z);
        else draw4(g, offset, seed, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ph[j] * v[j] + sgn * (sg[j] * z[j]);
        store4<VEC>(state + (long long)(T - 1) * clm2, off, ok, v);
    } else {
        // stationary start, then the AR recurrence: equal to the Toeplitz "discount" product of the reference
        for (int t = 0; t < T; ++t) {
            if (xi) load4<VEC>(xi + (long long)t * clm2, xoff, ok, z);
            else draw4(g, offset + (unsigned long long)t, seed, z);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float eta = sgn * (sg[j] * z[j]);
                v[j] = t == 0 ? eta / sqrtf(1.0f - ph[j] * ph[j]) : ph[j] * v[j] + eta;
            }
            store4<VEC>(state + (long long)t * clm2, off, ok, v);
        }
    }
}

__global__ void noise_advance_kernel(long long* __restrict__ rng, long long n) {
    rng[1] = (long long)((unsigned long long)rng[1] + (unsigned long long)n);       // 64-bit: the carry out of the low word included
}

template <int MODE>
void launch_update(bool vec, dim3 grid, hipStream_t s, float* state, const float* xi, const float* sigma, const float* phi,
                   const long long* rng, int B, int T, int L, int M, unsigned clm2, float sgn) {
    if (vec)
        hipLaunchKernelGGL((noise_update_kernel<MODE, true>), grid, dim3(NT), 0, s, state, xi, sigma, phi, rng, B, T, L, M, clm2, sgn);
    else
        hipLaunchKernelGGL((noise_update_kernel<MODE, false>), grid, dim3(NT), 0, s, state, xi, sigma, phi, rng, B, T, L, M, clm2, sgn);
}
}  // namespace

extern "C" int mk_noise_update(float* state, const float* xi, const float* sigma, const float* phi, const long long* rng,
                               int mode, int B, int T, int C, int L, int M, int reflect, void* stream) {
    MK_REQUIRE(state, "noise_update: null state pointer");
    MK_REQUIRE(xi || rng, "noise_update: null rng pointer (and no innovations given)");
    MK_REQUIRE(mode == MK_NOISE_WHITE || mode == MK_NOISE_AR || mode == MK_NOISE_REPLACE, "noise_update: unknown mode %d", mode);
    MK_REQUIRE(mode == MK_NOISE_WHITE || (sigma && phi), "noise_update: null sigma / phi pointer");
    MK_REQUIRE(B >= 1 && C >= 1 && L >= 1 && M >= 1, "noise_update: bad shape (B %d, C %d, L %d, M %d)", B, C, L, M);
    MK_REQUIRE(T >= 1, "noise_update: T = %d, need T >= 1", T);
    const long long per = 2ll * C * L * M;
    MK_REQUIRE(per < (1ll << 31), "noise_update: C L M 2 = %lld elements per time level, need < 2^31", per);
    const unsigned clm2 = (unsigned)per;
    const bool vec = per % 4 == 0 && B <= 65535 && (((uintptr_t)state | (uintptr_t)xi) & 15) == 0;
    const long long groups = vec ? per / 4 : ((long long)B * per + 3) / 4;
    const long long blocks = (groups + NT - 1) / NT;
    MK_REQUIRE(blocks < (1ll << 31), "noise_update: too many blocks");
    const dim3 grid((unsigned)blocks, vec ? (unsigned)B : 1u);
    const float sgn = reflect ? -1.f : 1.f;
    hipStream_t s = (hipStream_t)stream;
    if (mode == MK_NOISE_WHITE) launch_update<MK_NOISE_WHITE>(vec, grid, s, state, xi, sigma, phi, rng, B, T, L, M, clm2, sgn);
    else if (mode == MK_NOISE_AR) launch_update<MK_NOISE_AR>(vec, grid, s, state, xi, sigma, phi, rng, B, T, L, M, clm2, sgn);
    else launch_update<MK_NOISE_REPLACE>(vec, grid, s, state, xi, sigma, phi, rng, B, T, L, M, clm2, sgn);
    return mk_check_launch("mk_noise_update");
}

extern "C" int mk_noise_advance(long long* rng, long long n, void* stream) {
    MK_REQUIRE(rng, "noise_advance: null pointer");
    hipLaunchKernelGGL(noise_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, rng, n);
    return mk_check_launch("mk_noise_advance");
}
