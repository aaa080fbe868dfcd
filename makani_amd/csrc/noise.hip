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
//             On a sphere split over h x w ranks (mk_noise_update_shard) the level is the GLOBAL one: element e of it takes
//             normal e & 3 of group e >> 2 wherever it is stored, so the field does not depend on the layout.
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

// What one launch covers.  One drawn time level of the GLOBAL array is (B, C, R, S) floats; the launch owns rows [r0, r0 + Rl) and
// floats [s0, s0 + Sl) of every (b, c) plane, held locally as (B, T, C, Rl, Sl).  A RUN is a stretch that is contiguous in the
// global level AND in the local one: a row segment (Sl floats), all rows of a plane when the box has whole rows (Rl S floats), the
// whole batch entry when the box is the whole array (C R S floats: the serial case).  Threads map to the Philox groups that touch a
// run, so a group that straddles a run's end is evaluated once per run it touches and every thread keeps the lanes inside its run.
struct NoiseBox {
    unsigned Cn, Rn;                    // runs per batch entry = Cn Rn: (1, 1), (C, 1) or (C, Rl)
    unsigned runlen, G, tpb;            // floats per run, threads per run (>= the groups that touch one), threads per batch entry
    unsigned lvl_g, plane_g, row_g, first_g;        // global: C R S, R S, S, r0 S + s0
    unsigned Rl, Sl, lvl;               // local: lvl = C Rl Sl floats per (batch entry, time level)
    int B, T;
    int wide;                           // ACC == 2: a whole, locally 16-byte aligned group may use one 16-byte access
};

// ACC = floats per access.  4: every group is whole and aligned, globally and locally.  2: everything is even, so lanes (0, 1) and
// (2, 3) stand or fall together and are 8-byte aligned — the (re, im) pairs of a spectral state.  1: element-wise masks.
// p points at lane 0 of the group (inside the allocation only where ok[0]); lanes that are not ok are never touched.
template <int ACC>
__device__ __forceinline__ void load4(const float* __restrict__ p, const bool* ok, bool wide, float* v) {
    if (ACC == 4 || (ACC == 2 && wide)) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(p);
        v[0] = x[0], v[1] = x[1], v[2] = x[2], v[3] = x[3];
    } else if (ACC == 2) {
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            f32x2 x = {0.f, 0.f};
            if (ok[j]) x = *reinterpret_cast<const f32x2*>(p + j);
            v[j] = x[0], v[j + 1] = x[1];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ok[j] ? p[j] : 0.f;
    }
}

template <int ACC>
__device__ __forceinline__ void store4(float* __restrict__ p, const bool* ok, bool wide, const float* v) {
    if (ACC == 4 || (ACC == 2 && wide)) {
        *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    } else if (ACC == 2) {
#pragma unroll
        for (int j = 0; j < 4; j += 2)
            if (ok[j]) *reinterpret_cast<f32x2*>(p + j) = f32x2{v[j], v[j + 1]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ok[j]) p[j] = v[j];
    }
}

// state (B, T, C, Rl, Sl) f32, updated in place.  xi: optional innovations instead of drawn ones, (B, xT, C, Rl, Sl) with xT = 1
// for MK_NOISE_AR and T otherwise.  sigma (C, Rl), phi (C).  grid = (threads of one batch entry / NT, batch entries over y and z).
template <int MODE, int ACC>
__global__ __launch_bounds__(NT) void noise_update_kernel(float* __restrict__ state, const float* __restrict__ xi,
                                                          const float* __restrict__ sigma, const float* __restrict__ phi,
                                                          const long long* __restrict__ rng, const NoiseBox bx, float sgn) {
    const int T = bx.T, xT = MODE == MK_NOISE_AR ? 1 : T;
    const unsigned tid = blockIdx.x * NT + threadIdx.x;
    const unsigned b = blockIdx.z * gridDim.y + blockIdx.y;
    if (tid >= bx.tpb || b >= (unsigned)bx.B) return;
    const unsigned run = tid / bx.G, j = tid - run * bx.G;
    const unsigned c = run / bx.Rn, rl = run - c * bx.Rn;
    // where the run starts: in the global level (the counter), and in one local (batch entry, time level)
    const unsigned long long gstart = (unsigned long long)b * bx.lvl_g + (c * bx.plane_g + rl * bx.row_g + bx.first_g);
    const unsigned lstart = (c * bx.Rl + rl) * bx.Sl;
    const unsigned long long g = (gstart >> 2) + j;
    const long long k0 = 4ll * j - (long long)(gstart & 3u);     // lane 0 of the group, relative to the run: -3 ... runlen + 2
    const long long runlen = bx.runlen;
    if (k0 >= runlen) return;
    bool ok[4];
    float sg[4], ph[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ok[q] = ACC == 4 || (k0 + q >= 0 && k0 + q < runlen);
    if (MODE != MK_NOISE_WHITE) {
        // (c, local row) of a lane from its place in the local level; a pair shares them (Sl is even where ACC >= 2)
        constexpr int STEP = ACC == 1 ? 1 : 2;
#pragma unroll
        for (int q = 0; q < 4; q += STEP) {
            const long long k = min(max(k0 + q, 0ll), runlen - 1);
            const unsigned row = (lstart + (unsigned)k) / bx.Sl;            // c Rl + local row: the index into sigma
            sg[q] = sigma[row], ph[q] = phi[row / bx.Rl];
            if (STEP == 2) sg[q + 1] = sg[q], ph[q + 1] = ph[q];
        }
    }
    const long long inrun = lstart + k0;
    const bool wide = ACC == 2 && bx.wide && ok[0] && ok[2] && (inrun & 3) == 0;
    float* const st = state + ((long long)b * T * bx.lvl + inrun);
    const float* const xs = xi ? xi + ((long long)b * xT * bx.lvl + inrun) : nullptr;
    const long long lvl = bx.lvl;
    unsigned long long seed = 0, offset = 0;
    if (!xi) seed = (unsigned long long)rng[0], offset = (unsigned long long)rng[1];

    float z[4], v[4];
    if (MODE == MK_NOISE_WHITE) {
        for (int t = 0; t < T; ++t) {
            if (xi) load4<ACC>(xs + t * lvl, ok, wide, z);
            else draw4(g, offset + (unsigned long long)t, seed, z);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = sgn * z[q];
            store4<ACC>(st + t * lvl, ok, wide, v);
        }
    } else if (MODE == MK_NOISE_AR) {
        // levels 1 .. T-1 move down to 0 .. T-2; the new last level continues the old last one
        for (int t = 0; t + 1 < T; ++t) {
            load4<ACC>(st + (t + 1) * lvl, ok, wide, v);
            store4<ACC>(st + t * lvl, ok, wide, v);
        }
        if (T == 1) load4<ACC>(st, ok, wide, v);                 // (T > 1: v holds the old last level)
        if (xi) load4<ACC>(xs, ok, wide, z);
        else draw4(g, offset, seed, z);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = ph[q] * v[q] + sgn * (sg[q] * z[q]);
        store4<ACC>(st + (T - 1) * lvl, ok, wide, v);
    } else {
        // stationary start, then the AR recurrence: equal to the Toeplitz "discount" product of the reference
        for (int t = 0; t < T; ++t) {
            if (xi) load4<ACC>(xs + t * lvl, ok, wide, z);
            else draw4(g, offset + (unsigned long long)t, seed, z);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float eta = sgn * (sg[q] * z[q]);
                v[q] = t == 0 ? eta / sqrtf(1.0f - ph[q] * ph[q]) : ph[q] * v[q] + eta;
            }
            store4<ACC>(st + t * lvl, ok, wide, v);
        }
    }
}

__global__ void noise_advance_kernel(long long* __restrict__ rng, long long n) {
    rng[1] = (long long)((unsigned long long)rng[1] + (unsigned long long)n);       // 64-bit: the carry out of the low word included
}

template <int MODE>
void launch_update(int acc, dim3 grid, hipStream_t s, float* state, const float* xi, const float* sigma, const float* phi,
                   const long long* rng, const NoiseBox& bx, float sgn) {
    if (acc == 4) hipLaunchKernelGGL((noise_update_kernel<MODE, 4>), grid, dim3(NT), 0, s, state, xi, sigma, phi, rng, bx, sgn);
    else if (acc == 2) hipLaunchKernelGGL((noise_update_kernel<MODE, 2>), grid, dim3(NT), 0, s, state, xi, sigma, phi, rng, bx, sgn);
    else hipLaunchKernelGGL((noise_update_kernel<MODE, 1>), grid, dim3(NT), 0, s, state, xi, sigma, phi, rng, bx, sgn);
}

// the arguments are checked by the two entries; C R S < 2^31 and the box lies inside (R, S)
int noise_launch(const char* what, float* state, const float* xi, const float* sigma, const float* phi, const long long* rng,
                 int mode, int B, int T, int C, int R, int S, int r0, int Rl, int s0, int Sl, int reflect, void* stream) {
    const bool rows = s0 == 0 && Sl == S, planes = rows && r0 == 0 && Rl == R;
    NoiseBox bx;
    bx.Cn = planes ? 1u : (unsigned)C;
    bx.Rn = rows ? 1u : (unsigned)Rl;
    bx.runlen = (unsigned)(planes ? (long long)C * R * S : rows ? (long long)Rl * S : (long long)Sl);
    bx.lvl_g = (unsigned)((long long)C * R * S), bx.plane_g = (unsigned)((long long)R * S), bx.row_g = (unsigned)S;
    bx.first_g = (unsigned)((long long)r0 * S + s0);
    bx.Rl = (unsigned)Rl, bx.Sl = (unsigned)Sl, bx.lvl = (unsigned)((long long)C * Rl * Sl);
    bx.B = B, bx.T = T;
    // every start of a run, global and local, and every stride between levels and batch entries; an odd row length keeps the
    // element-wise path (a pair of lanes shares one sigma row)
    const unsigned a = bx.lvl_g | bx.lvl | bx.runlen | bx.first_g | (bx.Cn > 1 ? bx.plane_g | (unsigned)(Rl * Sl) : 0u) |
                       (bx.Rn > 1 ? bx.row_g | bx.Sl : 0u) | (bx.Sl & 1u);
    const uintptr_t ptrs = (uintptr_t)state | (uintptr_t)xi;
    const int acc = (a & 3u) == 0 && (ptrs & 15) == 0 ? 4 : (a & 1u) == 0 && (ptrs & 7) == 0 ? 2 : 1;
    bx.wide = acc == 2 && (bx.lvl & 3u) == 0 && (ptrs & 15) == 0;
    bx.G = (bx.runlen + (acc == 4 ? 0u : acc == 2 ? 2u : 3u) + 3u) >> 2;      // a run starts up to 0 / 2 / 3 floats into its first group
    const unsigned long long tpb = (unsigned long long)bx.Cn * bx.Rn * bx.G;  // <= (C Rl Sl + 6 C Rl) / 4 < 2^31
    bx.tpb = (unsigned)tpb;
    const unsigned gy = (unsigned)(B < 65535 ? B : 65535), gz = ((unsigned)B + gy - 1) / gy;
    MK_REQUIRE(tpb < (1ull << 31) && gz <= 65535u, "%s: too many blocks", what);
    const dim3 grid((bx.tpb + NT - 1) / NT, gy, gz);
    const float sgn = reflect ? -1.f : 1.f;
    hipStream_t s = (hipStream_t)stream;
    if (mode == MK_NOISE_WHITE) launch_update<MK_NOISE_WHITE>(acc, grid, s, state, xi, sigma, phi, rng, bx, sgn);
    else if (mode == MK_NOISE_AR) launch_update<MK_NOISE_AR>(acc, grid, s, state, xi, sigma, phi, rng, bx, sgn);
    else launch_update<MK_NOISE_REPLACE>(acc, grid, s, state, xi, sigma, phi, rng, bx, sgn);
    return mk_check_launch(what);
}
}  // namespace

extern "C" int mk_noise_update_shard(float* state, const float* xi, const float* sigma, const float* phi, const long long* rng,
                                     int mode, int B, int T, int C, int R, int S, int r0, int Rl, int s0, int Sl, int reflect,
                                     void* stream) {
    MK_REQUIRE(state, "noise_update_shard: null state pointer");
    MK_REQUIRE(xi || rng, "noise_update_shard: null rng pointer (and no innovations given)");
    MK_REQUIRE(mode == MK_NOISE_WHITE || mode == MK_NOISE_AR || mode == MK_NOISE_REPLACE, "noise_update_shard: unknown mode %d", mode);
    MK_REQUIRE(mode == MK_NOISE_WHITE || (sigma && phi), "noise_update_shard: null sigma / phi pointer");
    MK_REQUIRE(B >= 1 && C >= 1 && R >= 1 && S >= 1, "noise_update_shard: bad shape (B %d, C %d, R %d, S %d)", B, C, R, S);
    MK_REQUIRE(T >= 1, "noise_update_shard: T = %d, need T >= 1", T);
    MK_REQUIRE(r0 >= 0 && Rl >= 1 && Rl <= R - r0, "noise_update_shard: rows [%d, %d + %d) leave the global [0, %d)", r0, r0, Rl, R);
    MK_REQUIRE(s0 >= 0 && Sl >= 1 && Sl <= S - s0, "noise_update_shard: floats [%d, %d + %d) leave the global row [0, %d)", s0, s0, Sl, S);
    const long long per = (long long)C * R * S;
    MK_REQUIRE(per < (1ll << 31), "noise_update_shard: C R S = %lld elements per global time level, need < 2^31", per);
    return noise_launch("mk_noise_update_shard", state, xi, sigma, phi, rng, mode, B, T, C, R, S, r0, Rl, s0, Sl, reflect, stream);
}

// the whole array as one box: rows = degrees, floats per row = 2 M
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
    return noise_launch("mk_noise_update", state, xi, sigma, phi, rng, mode, B, T, C, L, 2 * M, 0, L, 0, 2 * M, reflect, stream);
}

extern "C" int mk_noise_advance(long long* rng, long long n, void* stream) {
    MK_REQUIRE(rng, "noise_advance: null pointer");
    hipLaunchKernelGGL(noise_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, rng, n);
    return mk_check_launch("mk_noise_advance");
}
