// Element access, block sums and launch plumbing shared by the loss, metric, norm and preprocessing kernels (gfx950).
// A new kernel of that kind includes this header instead of common.h and writes none of the following itself.
#pragma once
#include <type_traits>

#include "common.h"

// ---- f32 | bf16 element <-> float ------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ float mk_ld(const T* p) {
    static_assert(std::is_same<T, float>::value || std::is_same<T, u16>::value, "f32 or bf16 (u16) elements");
    if constexpr (std::is_same<T, u16>::value) return bf16_to_f32(*p);
    else return *p;
}
template <typename T>
__device__ __forceinline__ void mk_st(T* p, float v) {
    static_assert(std::is_same<T, float>::value || std::is_same<T, u16>::value, "f32 or bf16 (u16) elements");
    if constexpr (std::is_same<T, u16>::value) *p = f32_to_bf16(v);
    else *p = v;
}

// P consecutive elements.  P = 4 is ONE 16-byte (f32) or 8-byte (bf16) access: p must be aligned to it.  bf16 comes in as four
// shifts / masks of the two dwords and goes out through pack_bf16x2 (one conversion per pair, the bits of the element form).
template <typename T, int P>
__device__ __forceinline__ void mk_ld(const T* p, float (&v)[P]) {
    static_assert(P == 1 || P == 4, "one element or one vector access");
    if constexpr (P == 1) {
        v[0] = mk_ld<T>(p);
    } else if constexpr (std::is_same<T, u16>::value) {
        const s16x4 r = *reinterpret_cast<const s16x4*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = bf16_to_f32((u16)r[j]);
    } else {
        const f32x4 r = *reinterpret_cast<const f32x4*>(p);
        v[0] = r[0], v[1] = r[1], v[2] = r[2], v[3] = r[3];
    }
}
template <typename T, int P>
__device__ __forceinline__ void mk_st(T* p, const float (&v)[P]) {
    static_assert(P == 1 || P == 4, "one element or one vector access");
    if constexpr (P == 1) {
        mk_st<T>(p, v[0]);
    } else if constexpr (std::is_same<T, u16>::value) {
        uint2 r;
        r.x = pack_bf16x2(v[0], v[1]);
        r.y = pack_bf16x2(v[2], v[3]);
        *reinterpret_cast<uint2*>(p) = r;
    } else {
        f32x4 r;
        r[0] = v[0], r[1] = v[1], r[2] = v[2], r[3] = v[3];
        *reinterpret_cast<f32x4*>(p) = r;
    }
}

// ---- the block's sum of one per-thread value -------------------------------------------------------------------
// ONE order everywhere, which is what makes the results reproducible: the 64 lanes of a wave by shuffles (32, 16, .. 1), lane 0
// of every wave writes red[wave], then the NT / 64 waves are added in index order starting from 0.f.  red holds NT / 64 floats.
// Every thread of the block must reach the call (a block-uniform condition around it is fine).  Two shapes, which differ in who
// receives the total and in whether red may be reused.

// The total is returned to THREAD 0 (0.f to the others); one barrier.  There is NO barrier in front of the write to red: a
// second sum of the same block needs a red row of its own (metrics.hip: one row per sum).
template <int NT>
__device__ __forceinline__ float mk_block_sum_t0(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0) {
        for (int i = 0; i < NT / 64; ++i) t += red[i];
    }
    return t;
}

// N sums at once behind ONE barrier, each in the order above; the totals are returned to THREAD 0 in place (the other threads
// keep partial values).  red holds one row of NT / 64 floats per sum; as with mk_block_sum_t0 there is no barrier in front of
// the writes, so a caller that sums repeatedly alternates between two such blocks of rows (impute.hip).
template <int NT, int N>
__device__ __forceinline__ void mk_block_sums_t0(float (&v)[N], float (*red)[NT / 64]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            float t = 0.f;
            for (int i = 0; i < NT / 64; ++i) t += red[k][i];
            v[k] = t;
        }
    }
}

// The total is returned to EVERY thread; two barriers.  The one in front of the write to red waits for the readers of the
// previous sum, so consecutive sums of a block may share one red.
template <int NT>
__device__ __forceinline__ float mk_block_sum_all(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < NT / 64; ++i) t += red[i];
    return t;
}

// ---- host side -------------------------------------------------------------------------------------------------
// blocks along a plane of n points: about four points per thread of a 256-thread block, at most 64
static inline int mk_plane_chunks(long long n) {
    const long long c = (n + 1023) / 1024;
    return (int)(c < 1 ? 1 : (c > 64 ? 64 : c));
}

static inline bool mk_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// one grid row per plane
#define MK_REQUIRE_PLANES(what, planes) \
    MK_REQUIRE((long long)(planes) <= 65535, what ": %lld planes (B * C) exceed the plane limit of 65535 (one grid row per plane)", (long long)(planes))

// fn(std::integral_constant<int, N>()) for the smallest compiled capacity N in {2, 4, 8, .. MAXCAP} that holds E members; fn
// launches the kernel instantiated for N and returns the status
template <int MAXCAP = 32, int N = 2, typename F>
int mk_with_capacity(int E, const char* what, F&& fn) {
    if (E <= N) return fn(std::integral_constant<int, N>());
    if constexpr (2 * N <= MAXCAP) {
        return mk_with_capacity<MAXCAP, 2 * N>(E, what, fn);
    } else {
        mk_set_error("%s: ensemble size %d exceeds the register-resident limit of %d members", what, E, MAXCAP);
        return MK_EUNSUP;
    }
}
