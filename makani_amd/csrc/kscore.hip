// MK_HIPCC_FLAGS: -fno-slp-vectorize
// Kernel score of an ensemble (KernelScoreLoss, makani/utils/losses/crps_loss.py:1022-1247): every member and the observation
// are filtered by a depthwise DISCO convolution (one output per (channel, basis function), fixed 0 / 1 selection weight) and the
// filtered fields are scored by the pointwise ensemble CRPS under the quadrature.  Here the sparse stencil and the score are ONE
// pass: the filtered ensemble (B E, C K, H, W) never exists in memory (gfx950).
//
//   y[x][k][t][p]   = sum_{i, l} v[k][t][i][l] x[i][(j0(t, i) + l + p) mod W]         x = observation, member 0 .. E - 1
//   out[b][c]       = sum_{k, t, p} q[t][p] w[b][c K + k][t][p] crps(y[obs], y[members])
//   g[e][k][t][p]   = gout[b][c] q w d crps / d y_e                                     (GRAD pass, into the workspace)
//   gx[e][i][j]     = sum_{k, t, l} v[k][t][i][l] g[e][k][t][(j - j0 - l) mod W]        (adjoint, gather form)
//
// The filter (makani_amd/disco.py: convolution_tensor, in_shape == out_shape) comes as CHUNKS: per (output row t, input row i)
// the taps of all K basis functions form one circular run in longitude, cut on the host into pieces of at most KS_CH taps,
// zero-padded to a multiple of four; a chunk is {input row, first longitude, taps, offset of its [K][taps] values}.  Near the
// poles a run is the whole circle: it is just more chunks through the same two LDS buffers.
//
// Forward: a workgroup owns one plane (b, c), one output row, KS_TP = 64 longitudes and a group of basis functions; WAVE w owns
// basis function k (chunk descriptors and filter values are wave-uniform: scalar loads), LANE the longitude.  Per chunk the
// segment [tile + run) of the E + 1 fields (observation = field 0) is staged into LDS as 16-byte (f32) / 8-byte (bf16) vectors,
// widened to fp32 once; the loads of chunk n + 1 are in flight (registers) while chunk n is contracted, one barrier per chunk.
// A thread keeps its E + 1 accumulators in registers: they ARE the f[EM] of crps_point.  Block sums in one order, partial sums per
// block, a block-order finish: no atomics, bit-identical repeats.
// Adjoint: same staging with the K workspace planes of one member as fields (eight at a time), a thread owns one of 256 input
// longitudes and adds over k, t and the run in a fixed order.
#include "crps_point.h"

namespace {

constexpr int KS_CH = 64;                       // taps per chunk
constexpr int KS_TP = 64;                       // longitudes per forward tile (one wave)
constexpr int KS_FS = KS_TP + KS_CH + 4;        // floats per staged field: tile + run halo + alignment slack
constexpr int KS_NTMAX = 512;                   // forward block: 4 .. 8 waves
constexpr int KS_NTMIN = 256;
constexpr int KS_KW = KS_NTMAX / 64;            // basis functions per workgroup
constexpr int KS_TPA = 256;                     // longitudes per adjoint tile = its block
constexpr int KS_FSA = KS_TPA + KS_CH + 4;
constexpr int KS_KA = 8;                        // workspace planes staged at a time in the adjoint
constexpr long long KS_WS_CAP_BYTES = 640ll << 20;      // the GRAD workspace: one plane at (E = 16, K = 9, 721 x 1440) is 571 MiB

// four consecutive longitudes pos .. pos + 3 (mod W) of a row; vec: W % 4 == 0, pos % 4 == 0 and the row is aligned
template <typename T>
__device__ __forceinline__ void ks_fetch4(const T* __restrict__ row, int pos, int W, bool vec, float (&v)[4]) {
    pos %= W;
    if (vec) {
        mk_ld<T, 4>(row + pos, v);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int p = pos + j;
            p = p >= W ? p - W : p;
            v[j] = mk_ld<T>(row + p);
        }
    }
}
__device__ __forceinline__ void ks_fetch4(const void* row, bool bf16, int pos, int W, bool vec, float (&v)[4]) {
    if (bf16) ks_fetch4<u16>((const u16*)row, pos, W, vec, v);
    else ks_fetch4<float>((const float*)row, pos, W, vec, v);
}

// first staged longitude of a chunk for the tile that starts at p0, and the offset d of the tile's first tap behind it
__device__ __forceinline__ int ks_window(int p0, int jstart, int W, bool vec, int& d) {
    int s = p0 + jstart;
    s = s >= W ? s - W : s;
    d = vec ? (s & 3) : 0;
    return s - d;
}

// grid (tiles, H, planes * KG); block 64 * max(4, waves that own a basis function)
template <int EM, bool GRAD>
__global__ __launch_bounds__(KS_NTMAX) void kscore_fwd_kernel(const void* __restrict__ f, int f_bf16, const void* __restrict__ obs, int o_bf16,
                                                             const int4* __restrict__ desc, const int* __restrict__ doff,
                                                             const float* __restrict__ vals, const float* __restrict__ q,
                                                             const float* __restrict__ w, long long w_sb, long long w_sc,
                                                             const float* __restrict__ gout, float* __restrict__ partial,
                                                             float* __restrict__ ws, int E, int C, int K, int H, int W, int KG, int plane0,
                                                             int type, float alpha, const float* __restrict__ ew, int vec) {
    constexpr int NF = EM + 1;
    constexpr int QW = KS_FS / 4;
    constexpr int NQ = (NF * QW + KS_NTMIN - 1) / KS_NTMIN;
    __shared__ __attribute__((aligned(16))) float img[2][NF][KS_FS];
    __shared__ float red[KS_NTMAX / 64];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pl = blockIdx.z / KG, kg = blockIdx.z % KG;
    const int plane = plane0 + pl, b = plane / C, c = plane % C;
    const int t = blockIdx.y, p0 = blockIdx.x * KS_TP;
    const int kw = (K + KG - 1) / KG;                   // basis functions of a group: its first kw waves own one each
    const int k = kg * kw + wave;
    const bool live_k = wave < kw && k < K;
    const int kc = live_k ? k : 0;
    const long long hw = (long long)H * W;
    const int esz = f_bf16 ? 2 : 4, osz = o_bf16 ? 2 : 4;
    const char* fb = (const char*)f + ((long long)b * E * C + c) * hw * esz;
    const char* ob = (const char*)obs + (long long)plane * hw * osz;
    const long long estride = (long long)C * hw * esz;
    const int nf = E + 1;
    if (tid < KS_NTMAX / 64) red[tid] = 0.f;

    const int c_lo = doff[t], c_hi = doff[t + 1];
    float pre[NQ][4];
    auto fetch = [&](int ci) {
        const int4 dsc = desc[ci];
        int d;
        const int sa = ks_window(p0, dsc.y, W, vec, d);
        const int nq = (d + KS_TP + dsc.z + 2) >> 2;
#pragma unroll
        for (int r = 0; r < NQ; ++r) {
            const int idx = tid + r * nt, fld = idx / QW, qq = idx - fld * QW;
            if (fld < nf && qq < nq) {
                if (fld == 0) ks_fetch4(ob + (long long)dsc.x * W * osz, o_bf16, sa + 4 * qq, W, vec, pre[r]);
                else ks_fetch4(fb + (fld - 1) * estride + (long long)dsc.x * W * esz, f_bf16, sa + 4 * qq, W, vec, pre[r]);
            }
        }
    };
    auto commit = [&](int ci, int buf) {
        const int4 dsc = desc[ci];
        int d;
        ks_window(p0, dsc.y, W, vec, d);
        const int nq = (d + KS_TP + dsc.z + 2) >> 2;
#pragma unroll
        for (int r = 0; r < NQ; ++r) {
            const int idx = tid + r * nt, fld = idx / QW, qq = idx - fld * QW;
            if (fld < nf && qq < nq) {
                f32x4 v4;
                v4[0] = pre[r][0], v4[1] = pre[r][1], v4[2] = pre[r][2], v4[3] = pre[r][3];
                *reinterpret_cast<f32x4*>(&img[buf][fld][4 * qq]) = v4;
            }
        }
    };

    float acc[NF];
#pragma unroll
    for (int x = 0; x < NF; ++x) acc[x] = 0.f;
    if (c_lo < c_hi) {
        fetch(c_lo);
        commit(c_lo, 0);
    }
    __syncthreads();
    for (int ci = c_lo; ci < c_hi; ++ci) {
        const int buf = (ci - c_lo) & 1;
        if (ci + 1 < c_hi) fetch(ci + 1);
        if (live_k) {
            const int4 dsc = desc[ci];
            int d;
            ks_window(p0, dsc.y, W, vec, d);
            const float* vk = vals + dsc.w + (long long)kc * dsc.z;
            const int n = dsc.z;
#pragma unroll
            for (int x = 0; x < NF; ++x) {
                if (x < nf) {
                    const float* row = &img[buf][x][d + lane];
                    float a = 0.f;                       // a chunk's sum on its own: shorter chains, smaller rounding error
                    for (int l = 0; l < n; l += 4) {
                        a = fmaf(vk[l], row[l], a);
                        a = fmaf(vk[l + 1], row[l + 1], a);
                        a = fmaf(vk[l + 2], row[l + 2], a);
                        a = fmaf(vk[l + 3], row[l + 3], a);
                    }
                    acc[x] += a;
                }
            }
        }
        if (ci + 1 < c_hi) commit(ci + 1, buf ^ 1);
        __syncthreads();
    }

    const int p = p0 + lane;
    const bool live = live_k && p < W;
    // weights and addresses first: across the E^2 rank comparisons of crps_point only per-thread values stay live
    float wt = 0.f;
    if (live) {
        const long long pt = (long long)t * W + p;
        wt = q[pt] * (w ? w[b * w_sb + ((long long)c * K + k) * w_sc + pt] : 1.f);
        if (GRAD) wt *= gout[plane];
    }
    float* gp = GRAD ? ws + (((long long)pl * E * K + kc) * H + t) * W + p : nullptr;
    const long long gstride = (long long)K * hw;
    float m[EM];
#pragma unroll
    for (int e = 0; e < EM; ++e) m[e] = (e < E) ? acc[e + 1] : 0.f;
    const float o = acc[0];
    float s;
    if (E == 1) {                                        // |o - f| (crps_loss.py:1165-1167)
        s = fabsf(o - m[0]);
        if (GRAD) m[0] = sgn(m[0] - o);
    } else {
        s = crps_point<EM, GRAD>(m, E, o, type, alpha, 0.f, ew);
    }
    if (GRAD) {
        if (live) {
#pragma unroll
            for (int e = 0; e < EM; ++e)
                if (e < E) gp[e * gstride] = wt * m[e];
        }
    } else {
        const float tot = mk_block_sum_t0<KS_NTMAX>(live ? wt * s : 0.f, red);
        if (tid == 0) partial[(((long long)plane * H + t) * gridDim.x + blockIdx.x) * KG + kg] = tot;
    }
}

// out[plane] = the plane's partial sums added in index order: thread j adds j, j + 256, ..., then the block sum
__global__ __launch_bounds__(256) void kscore_finish_kernel(const float* __restrict__ partial, float* __restrict__ out, long long n) {
    __shared__ float red[256 / 64];
    const float* pp = partial + (long long)blockIdx.x * n;
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) s += pp[i];
    const float tot = mk_block_sum_t0<256>(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// grid (tiles of 256, H, planes of the group * E); ws (P, E, K, H, W) f32 -> gx (B, E, C, H, W) in the dtype of the forecasts
template <typename T>
__global__ __launch_bounds__(KS_TPA) void kscore_adj_kernel(const float* __restrict__ ws, T* __restrict__ gx, const int4* __restrict__ desc,
                                                           const int* __restrict__ doff, const float* __restrict__ vals, int E, int C,
                                                           int K, int H, int W, int plane0, int vec) {
    constexpr int QW = KS_FSA / 4;
    constexpr int NQ = (KS_KA * QW + KS_TPA - 1) / KS_TPA;
    __shared__ __attribute__((aligned(16))) float img[2][KS_KA][KS_FSA];
    const int tid = threadIdx.x;
    const int pl = blockIdx.z / E, e = blockIdx.z % E;
    const int plane = plane0 + pl, b = plane / C, c = plane % C;
    const int i = blockIdx.y, p0 = blockIdx.x * KS_TPA;
    const long long hw = (long long)H * W;
    const float* gb = ws + ((long long)pl * E + e) * K * hw;
    const int KG = (K + KS_KA - 1) / KS_KA;
    const int c_lo = doff[i], n_it = (doff[i + 1] - c_lo) * KG;

    float pre[NQ][4];
    auto fetch = [&](int it) {
        const int4 dsc = desc[c_lo + it / KG];
        const int k0 = (it % KG) * KS_KA, nk = min(KS_KA, K - k0);
        int d;
        const int sa = ks_window(p0, dsc.y, W, vec, d);
        const int nq = (d + KS_TPA + dsc.z + 2) >> 2;
#pragma unroll
        for (int r = 0; r < NQ; ++r) {
            const int idx = tid + r * KS_TPA, fld = idx / QW, qq = idx - fld * QW;
            if (fld < nk && qq < nq) ks_fetch4<float>(gb + (k0 + fld) * hw + (long long)dsc.x * W, sa + 4 * qq, W, vec, pre[r]);
        }
    };
    auto commit = [&](int it, int buf) {
        const int4 dsc = desc[c_lo + it / KG];
        const int k0 = (it % KG) * KS_KA, nk = min(KS_KA, K - k0);
        int d;
        ks_window(p0, dsc.y, W, vec, d);
        const int nq = (d + KS_TPA + dsc.z + 2) >> 2;
#pragma unroll
        for (int r = 0; r < NQ; ++r) {
            const int idx = tid + r * KS_TPA, fld = idx / QW, qq = idx - fld * QW;
            if (fld < nk && qq < nq) {
                f32x4 v4;
                v4[0] = pre[r][0], v4[1] = pre[r][1], v4[2] = pre[r][2], v4[3] = pre[r][3];
                *reinterpret_cast<f32x4*>(&img[buf][fld][4 * qq]) = v4;
            }
        }
    };

    float a = 0.f;
    if (n_it > 0) {
        fetch(0);
        commit(0, 0);
    }
    __syncthreads();
    for (int it = 0; it < n_it; ++it) {
        const int buf = it & 1;
        if (it + 1 < n_it) fetch(it + 1);
        const int4 dsc = desc[c_lo + it / KG];
        const int k0 = (it % KG) * KS_KA, nk = min(KS_KA, K - k0);
        int d;
        ks_window(p0, dsc.y, W, vec, d);
        const int n = dsc.z;
        for (int x = 0; x < nk; ++x) {
            const float* vk = vals + dsc.w + (long long)(k0 + x) * n;
            const float* row = &img[buf][x][d + tid];
            float al = 0.f;
            for (int l = 0; l < n; l += 4) {
                al = fmaf(vk[l], row[l], al);
                al = fmaf(vk[l + 1], row[l + 1], al);
                al = fmaf(vk[l + 2], row[l + 2], al);
                al = fmaf(vk[l + 3], row[l + 3], al);
            }
            a += al;
        }
        if (it + 1 < n_it) commit(it + 1, buf ^ 1);
        __syncthreads();
    }
    const int p = p0 + tid;
    if (p < W) mk_st<T>(gx + (((long long)b * E + e) * C + c) * hw + (long long)i * W + p, a);
}

int ks_kgroups(int K) { return (K + KS_KW - 1) / KS_KW; }
int ks_waves(int K) {
    const int kg = ks_kgroups(K), nw = (K + kg - 1) / kg;
    return nw < KS_NTMIN / 64 ? KS_NTMIN / 64 : nw;
}
int ks_tiles(int W) { return (W + KS_TP - 1) / KS_TP; }

// the vector path: whole quads never straddle the wrap and every row starts on a 16-byte (f32) / 8-byte (bf16) boundary
bool ks_vec(const void* p, int dtype, int W) { return W % 4 == 0 && ((uintptr_t)p & (dtype == MK_BF16 ? 7 : 15)) == 0; }

struct KsArgs {
    const void *f, *obs;
    int f_dtype, o_dtype;
    const int4* desc;
    const int* doff;
    const float *vals, *q, *w;
    long long w_sb, w_sc;
    int B, E, C, K, H, W, type;
    float alpha;
    const float* ew;
};

template <bool GRAD>
int ks_launch_fwd(const KsArgs& a, const float* gout, float* partial, float* ws, int plane0, int planes, hipStream_t s) {
    const int KG = ks_kgroups(a.K);
    const dim3 grid((unsigned)ks_tiles(a.W), (unsigned)a.H, (unsigned)(planes * KG)), block((unsigned)(64 * ks_waves(a.K)));
    const int vec = ks_vec(a.f, a.f_dtype, a.W) && ks_vec(a.obs, a.o_dtype, a.W);
    return mk_with_capacity(a.E, "kscore", [&](auto em) {
        hipLaunchKernelGGL((kscore_fwd_kernel<em(), GRAD>), grid, block, 0, s, a.f, (int)(a.f_dtype == MK_BF16), a.obs,
                           (int)(a.o_dtype == MK_BF16), a.desc, a.doff, a.vals, a.q, a.w, a.w_sb, a.w_sc, gout, partial, ws, a.E, a.C, a.K,
                           a.H, a.W, KG, plane0, a.type, a.alpha, a.ew, vec);
        return mk_check_launch("mk_kscore");
    });
}

int ks_check(const KsArgs& a) {
    MK_REQUIRE(a.f && a.obs && a.desc && a.doff && a.vals && a.q, "kscore: missing operand");
    MK_REQUIRE(a.B > 0 && a.C > 0 && a.K > 0 && a.H > 0 && a.W >= 4 && a.H <= 65535, "kscore: bad shape (W >= 4, H <= 65535)");
    MK_REQUIRE(a.E >= 1, "kscore: the ensemble needs at least one member");
    MK_REQUIRE((a.f_dtype == MK_F32 || a.f_dtype == MK_BF16) && (a.o_dtype == MK_F32 || a.o_dtype == MK_BF16), "kscore: f32 or bf16 fields");
    MK_REQUIRE(a.type == CRPS_SKILLSPREAD || a.type == CRPS_PWM || a.type == CRPS_NAIVE || a.type == CRPS_CDF,
               "kscore: score type %d (built: skillspread, probability weighted moment, naive skillspread, cdf)", a.type);
    MK_REQUIRE(!a.ew || a.type == CRPS_CDF, "kscore: ensemble weights are defined for the cdf form only");
    return 0;
}

}  // namespace

extern "C" int mk_kscore_chunk(void) { return KS_CH; }

// partial sums of one plane in forward
extern "C" long long mk_kscore_partials(int K, int H, int W) { return (long long)H * ks_tiles(W) * ks_kgroups(K); }

// planes (b, c) per GRAD pass: as many as keep the (P, E, K, H, W) f32 workspace under the cap, at least one
extern "C" int mk_kscore_planes(int planes, int E, int K, int H, int W) {
    if (E < 1 || K < 1 || H < 1 || W < 1) return 1;
    long long P = KS_WS_CAP_BYTES / ((long long)E * K * H * W * 4);
    const int zper = E > ks_kgroups(K) ? E : ks_kgroups(K);          // grid rows a plane takes (GRAD pass, adjoint)
    P = P > 65535 / zper ? 65535 / zper : P;
    P = P > planes ? planes : P;
    return (int)(P < 1 ? 1 : P);
}

// floats of the GRAD workspace
extern "C" long long mk_kscore_workspace(int planes, int E, int K, int H, int W) {
    return (long long)mk_kscore_planes(planes, E, K, H, W) * E * K * H * W;
}

extern "C" int mk_kscore_fwd(const void* f, int f_dtype, const void* obs, int o_dtype, const int* desc, const int* doff, const float* vals,
                             const float* q, const float* w, long long w_sb, long long w_sc, float* partial, float* out, int B, int E, int C,
                             int K, int H, int W, int type, float alpha, const float* ens_w, void* stream) {
    const KsArgs a{f, obs, f_dtype, o_dtype, (const int4*)desc, doff, vals, q, w, w_sb, w_sc, B, E, C, K, H, W, type, alpha, ens_w};
    if (int rc = ks_check(a)) return rc;
    MK_REQUIRE(partial && out, "kscore: missing output");
    MK_REQUIRE((long long)B * C * ks_kgroups(K) <= 65535, "kscore: %lld planes x %d basis groups exceed the grid limit of 65535",
               (long long)B * C, ks_kgroups(K));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ks_launch_fwd<false>(a, nullptr, partial, nullptr, 0, B * C, s)) return rc;
    hipLaunchKernelGGL(kscore_finish_kernel, dim3((unsigned)(B * C)), dim3(256), 0, s, partial, out, mk_kscore_partials(K, H, W));
    return mk_check_launch("mk_kscore_fwd");
}

// gx (shape / dtype of f) = the gradient of sum_{b, c} gout[b][c] out[b][c] with respect to the forecasts.  desc_t / doff_t / vals_t:
// the chunks of the TRANSPOSED filter (segments = input rows, rows = output rows, longitudes negated).  ws: mk_kscore_workspace floats.
extern "C" int mk_kscore_bwd(const void* f, int f_dtype, const void* obs, int o_dtype, const int* desc, const int* doff, const float* vals,
                             const int* desc_t, const int* doff_t, const float* vals_t, const float* q, const float* w, long long w_sb,
                             long long w_sc, const float* gout, float* ws, void* gx, int B, int E, int C, int K, int H, int W, int type,
                             float alpha, const float* ens_w, void* stream) {
    const KsArgs a{f, obs, f_dtype, o_dtype, (const int4*)desc, doff, vals, q, w, w_sb, w_sc, B, E, C, K, H, W, type, alpha, ens_w};
    if (int rc = ks_check(a)) return rc;
    MK_REQUIRE(desc_t && doff_t && vals_t && gout && ws && gx, "kscore: missing backward operand");
    MK_REQUIRE(E <= 32, "kscore: ensemble size %d exceeds the register-resident limit of 32 members", E);      // (P below assumes it)
    hipStream_t s = (hipStream_t)stream;
    const int planes = B * C, P = mk_kscore_planes(planes, E, K, H, W);
    const int vec = W % 4 == 0 && mk_aligned16(ws);
    for (int plane0 = 0; plane0 < planes; plane0 += P) {
        const int np = planes - plane0 < P ? planes - plane0 : P;
        if (int rc = ks_launch_fwd<true>(a, gout, nullptr, ws, plane0, np, s)) return rc;
        const dim3 grid((unsigned)((W + KS_TPA - 1) / KS_TPA), (unsigned)H, (unsigned)(np * E));
        if (f_dtype == MK_BF16)
            hipLaunchKernelGGL(kscore_adj_kernel<u16>, grid, dim3(KS_TPA), 0, s, ws, (u16*)gx, (const int4*)desc_t, doff_t, vals_t, E, C, K, H,
                               W, plane0, vec);
        else
            hipLaunchKernelGGL(kscore_adj_kernel<float>, grid, dim3(KS_TPA), 0, s, ws, (float*)gx, (const int4*)desc_t, doff_t, vals_t, E, C, K,
                               H, W, plane0, vec);
        if (int rc = mk_check_launch("mk_kscore_bwd")) return rc;
    }
    return 0;
}
