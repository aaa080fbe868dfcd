// MK_HIPCC_FLAGS: -fno-slp-vectorize
// (see escore.hip: the SLP vectoriser's packed-fp32 forms are kept out of this library; tests/test_packed_forms.py scans the ISA)
// Imputation of missing input values (makani/models/common/imputation.py) and the output tail of FourCastNet3.1
// (makani/models/networks/fourcastnet3_1.py:1062-1080,1127-1131), forward and backward (gfx950).
//
// Every pixel is independent.  A thread owns P consecutive pixels of a plane (P = 4: one 16-byte f32 / 8-byte bf16 access per
// channel, when HW is a multiple of 4 and every tensor pointer is 16-byte aligned; P = 1 otherwise); the arithmetic is fp32
// whatever the element type, the result is rounded once.
//
//   mk_impute_mlp_fwd    MLPImputation in one launch: x is read once, y is written once
//       m_j  = isnan(x[imp_ch[j]]) | (mask operand != 0)                   j < NI imputed channels
//       xc_c = x_c, with 0 at the masked entries of the imputed channels   c < C
//       h_k  = b1_k + sum_c W1[k][c] xc_c,  a_k = act(h_k)                 k < hidden
//       o_j  = sum_k W2[j][k] a_k
//       y[imp_ch[j]] = m_j ? o_j : x[imp_ch[j]];   every other channel is copied while the thread walks the channels
//     The imputed channels and their masks are loaded first and stay in registers (NI <= 8); the hidden column h lives in
//     registers, unrolled over a compile-time capacity HC (4, 8, 16, 32).  W1 (transposed: the HC weights of a channel are
//     consecutive), b1, W2, imp_ch and the channel -> slot map sit in ONE device table and every read of it has a wave-uniform
//     address (scalar loads).  The entry an imputed channel needs by its run-time slot is taken with a chain of selects over
//     compile-time indices, never by indexing a register array.
//   mk_impute_mlp_bwd    recomputes h from the saved x and mask (first walk over the channels), then
//       go_j = m_j ? g[imp_ch[j]] : 0,  ga_k = sum_j W2[j][k] go_j,  gh_k = ga_k act'(h_k)
//       gW2[j][k] = sum go_j a_k,  gb1_k = sum gh_k,  gW1[k][c] = sum gh_k xc_c          (sums over samples and pixels)
//       gx_c = g_c + sum_k W1[k][c] gh_k;   exactly 0 at the masked entries of the imputed channels
//     in a second walk over the channels, which reads x again, reads g and writes gx.  The weight sums are taken in that same walk:
//     per channel the block adds its threads' gh_k xc_c (mk_block_sums_t0: HC sums behind one barrier) and thread 0 writes the
//     partial sum of the block; a second, tiny launch adds the blocks' partial sums in index order.  No atomics.
//   mk_impute_const_fwd / _bwd    ConstantImputation: y = (mask | isnan(x)) ? w_c : x;  gx = masked ? 0 : g,  gw_c = sum of g over
//     the masked entries (partial sums per chunk of a plane, added in index order).
//   mk_fcn31_tail_fwd / _bwd      y_c = clamp_c(d_c + [skip] xin[pred_ch[c]]), clamp_c the identity or soft_clamp(v + off_c) - off_c.
#include "block_io.h"

namespace {

constexpr int CNT = 256;
constexpr int CMAX = MK_IMPUTE_CHANNELS, NIC = MK_IMPUTE_SLOTS, HID = MK_IMPUTE_HIDDEN;
// the table (32-bit words): W1 transposed (CMAX, HID), b1 (HID), W2 (NIC, HID), all f32 and zero beyond their counts; then int32:
// imp_ch (NIC, padded with a valid channel), slot (CMAX: j for imp_ch[j], -1 for every other channel)
constexpr int T_W1 = 0, T_B1 = CMAX * HID, T_W2 = T_B1 + HID, T_IMP = T_W2 + NIC * HID, T_SLOT = T_IMP + NIC;
static_assert(T_SLOT + CMAX == MK_IMPUTE_TAB, "table size of include/makani_amd.h");

struct Imp {
    const float* tab;
    const void* mask;          // the mask operand (kind 1 .. 3), unused otherwise
    long long m_sb;            // its stride over samples in elements (0: one mask for every sample)
    int kind, Nm, mask_ch;
    int C, NI, act;
};

// the mask operand of P pixels: kind 1 bool (one byte each), 2 f32, 3 bf16 (any nonzero value counts)
template <int P>
__device__ __forceinline__ void ld_mask(int kind, const void* p, long long at, bool (&m)[P]) {
    if (kind == MK_IMPUTE_MASK_BOOL) {
        const unsigned char* q = static_cast<const unsigned char*>(p) + at;
        if constexpr (P == 4) {
            const unsigned r = *reinterpret_cast<const unsigned*>(q);
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = ((r >> (8 * e)) & 0xffu) != 0u;
        } else {
            m[0] = q[0] != 0;
        }
    } else {
        float v[P];
        if (kind == MK_IMPUTE_MASK_F32) mk_ld<float, P>(static_cast<const float*>(p) + at, v);
        else mk_ld<u16, P>(static_cast<const u16*>(p) + at, v);
#pragma unroll
        for (int e = 0; e < P; ++e) m[e] = v[e] != 0.f;
    }
}

// the imputed channels of P pixels and their masks; xi comes back with 0 at the masked entries (an unmasked entry is what was read)
template <typename T, int P>
__device__ __forceinline__ void load_imputed(const T* __restrict__ xb, const Imp& a, int b, long long i, long long hw, float (&xi)[NIC][P],
                                             bool (&m)[NIC][P]) {
    const int* __restrict__ it = reinterpret_cast<const int*>(a.tab + T_IMP);
#pragma unroll
    for (int j = 0; j < NIC; ++j) mk_ld<T, P>(xb + (long long)it[j] * hw, xi[j]);
    bool m0[P];
#pragma unroll
    for (int e = 0; e < P; ++e) m0[e] = false;
    if (a.kind == MK_IMPUTE_MASK_CHANNEL) {
        float v[P];
        mk_ld<T, P>(xb + (long long)a.mask_ch * hw, v);
#pragma unroll
        for (int e = 0; e < P; ++e) m0[e] = v[e] != 0.f;
    } else if (a.kind != MK_IMPUTE_MASK_NONE && a.Nm == 1) {
        ld_mask<P>(a.kind, a.mask, (long long)b * a.m_sb + i, m0);
    }
    const bool per_channel = a.kind != MK_IMPUTE_MASK_NONE && a.kind != MK_IMPUTE_MASK_CHANNEL && a.Nm > 1;
#pragma unroll
    for (int j = 0; j < NIC; ++j) {
        bool mj[P];
#pragma unroll
        for (int e = 0; e < P; ++e) mj[e] = m0[e];
        if (per_channel && j < a.NI) ld_mask<P>(a.kind, a.mask, (long long)b * a.m_sb + (long long)j * hw + i, mj);
#pragma unroll
        for (int e = 0; e < P; ++e) {
            m[j][e] = j < a.NI && (mj[e] || xi[j][e] != xi[j][e]);
            xi[j][e] = m[j][e] ? 0.f : xi[j][e];
        }
    }
}

// entry `sl` (wave-uniform, run-time) of a register-resident column: selects over compile-time indices
template <int P>
__device__ __forceinline__ void pick(const float (&a)[NIC][P], int sl, float (&o)[P]) {
#pragma unroll
    for (int j = 0; j < NIC; ++j) {
#pragma unroll
        for (int e = 0; e < P; ++e) o[e] = (j == sl) ? a[j][e] : o[e];
    }
}
template <int P>
__device__ __forceinline__ void pick(const bool (&a)[NIC][P], int sl, bool (&o)[P]) {
#pragma unroll
    for (int j = 0; j < NIC; ++j) {
#pragma unroll
        for (int e = 0; e < P; ++e) o[e] = (j == sl) ? a[j][e] : o[e];
    }
}

__device__ __forceinline__ float sigmoid_pair(float t, float& sneg) {
    const float e = expf(-fabsf(t)), d = 1.f / (1.f + e), lo = e * d;
    sneg = t >= 0.f ? lo : d;
    return t >= 0.f ? d : lo;
}

// a = act(h) and d = act'(h).  0 exact-erf GELU, 1 ReLU, 2 SiLU, 3 sin
template <int ACT>
__device__ __forceinline__ void act_pair(float h, float& a, float& d) {
    if constexpr (ACT == MK_IMPUTE_ACT_GELU) {
        const float cdf = 0.5f * (1.f + erff(h * 0.70710678118654752f));
        a = h * cdf;
        d = fmaf(h * 0.39894228040143268f, expf(-0.5f * h * h), cdf);
    } else if constexpr (ACT == MK_IMPUTE_ACT_RELU) {
        a = h > 0.f ? h : 0.f;
        d = h > 0.f ? 1.f : 0.f;
    } else if constexpr (ACT == MK_IMPUTE_ACT_SILU) {
        float sneg;
        const float s = sigmoid_pair(h, sneg);
        a = h * s;
        d = fmaf(h * s, sneg, s);
    } else {
        a = sinf(h);
        d = cosf(h);
    }
}

// row K of the column and the rows after it.  A recursion over the compile-time index, not a loop: with erff inlined the body is
// beyond what the unroller takes on at 32 rows of 4 pixels, and a loop left rolled would index the register arrays (scratch).
template <int ACT, int P, int HC, bool DERIV, int K = 0>
__device__ __forceinline__ void activate_as(float (&h)[HC][P], float (&dh)[DERIV ? HC : 1][P]) {
    if constexpr (K < HC) {
#pragma unroll
        for (int e = 0; e < P; ++e) {
            float a, d;
            act_pair<ACT>(h[K][e], a, d);
            h[K][e] = a;
            if constexpr (DERIV) dh[K][e] = d;
        }
        activate_as<ACT, P, HC, DERIV, K + 1>(h, dh);
    }
}

// h -> a in place; the derivative into dh when DERIV.  `act` is wave-uniform: one branch, then straight-line code
template <int P, int HC, bool DERIV>
__device__ __forceinline__ void activate(int act, float (&h)[HC][P], float (&dh)[DERIV ? HC : 1][P]) {
    if (act == MK_IMPUTE_ACT_GELU) activate_as<MK_IMPUTE_ACT_GELU, P, HC, DERIV>(h, dh);
    else if (act == MK_IMPUTE_ACT_RELU) activate_as<MK_IMPUTE_ACT_RELU, P, HC, DERIV>(h, dh);
    else if (act == MK_IMPUTE_ACT_SILU) activate_as<MK_IMPUTE_ACT_SILU, P, HC, DERIV>(h, dh);
    else activate_as<MK_IMPUTE_ACT_SIN, P, HC, DERIV>(h, dh);
}

// h_k = b1_k + sum_c W1[k][c] xc_c over the channels, four planes in flight; COPY: the channels that are not imputed go to yb
template <typename T, int P, int HC, bool COPY>
__device__ __forceinline__ void hidden_column(const T* __restrict__ xb, T* __restrict__ yb, const Imp& a, long long hw, const float (&xi)[NIC][P],
                                              float (&h)[HC][P]) {
    const float* __restrict__ ft = a.tab;
    const int* __restrict__ slot = reinterpret_cast<const int*>(a.tab + T_SLOT);
#pragma unroll
    for (int k = 0; k < HC; ++k) {
        const float b = ft[T_B1 + k];
#pragma unroll
        for (int e = 0; e < P; ++e) h[k][e] = b;
    }
    for (int c0 = 0; c0 < a.C; c0 += 4) {
        float v[4][P];
#pragma unroll
        for (int u = 0; u < 4; ++u) mk_ld<T, P>(xb + (long long)(c0 + u < a.C ? c0 + u : a.C - 1) * hw, v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u;
            if (c < a.C) {          // (wave-uniform)
                const int sl = slot[c];
                if (sl >= 0) {
                    pick<P>(xi, sl, v[u]);
                } else if constexpr (COPY) {
                    mk_st<T, P>(yb + (long long)c * hw, v[u]);
                }
                const float* __restrict__ w = ft + T_W1 + c * HID;
#pragma unroll
                for (int k = 0; k < HC; ++k) {
                    const float wk = w[k];
#pragma unroll
                    for (int e = 0; e < P; ++e) h[k][e] = fmaf(wk, v[u][e], h[k][e]);
                }
            }
        }
    }
}

// grid (pixel groups, B)
template <typename T, int P, int HC>
__global__ __launch_bounds__(CNT) void impute_mlp_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, Imp a, long long hw) {
    const long long i = ((long long)blockIdx.x * CNT + threadIdx.x) * P;
    if (i >= hw) return;
    const float* __restrict__ ft = a.tab;
    const int* __restrict__ it = reinterpret_cast<const int*>(a.tab + T_IMP);
    const int b = blockIdx.y;
    const T* xb = x + (long long)b * a.C * hw + i;
    T* yb = y + (long long)b * a.C * hw + i;
    float xi[NIC][P], h[HC][P], none[1][P];
    bool m[NIC][P];
    load_imputed<T, P>(xb, a, b, i, hw, xi, m);
    hidden_column<T, P, HC, true>(xb, yb, a, hw, xi, h);
    activate<P, HC, false>(a.act, h, none);
#pragma unroll
    for (int j = 0; j < NIC; ++j) {
        if (j < a.NI) {          // (wave-uniform)
            const float* __restrict__ w = ft + T_W2 + j * HID;
            float o[P];
#pragma unroll
            for (int e = 0; e < P; ++e) o[e] = 0.f;
#pragma unroll
            for (int k = 0; k < HC; ++k) {
                const float wk = w[k];
#pragma unroll
                for (int e = 0; e < P; ++e) o[e] = fmaf(wk, h[k][e], o[e]);
            }
#pragma unroll
            for (int e = 0; e < P; ++e) o[e] = m[j][e] ? o[e] : xi[j][e];
            mk_st<T, P>(yb + (long long)it[j] * hw, o);
        }
    }
}

// grid (pixel groups, B).  part: one row per block (B * gridDim.x rows), laid out as gW1 (HC, C) | gb1 (HC) | gW2 (NI, HC)
// of THIS block; every thread of the block stays to the end (the block sums), a thread beyond the plane contributes zeros.
template <typename T, int P, int HC>
__global__ __launch_bounds__(CNT) void impute_mlp_bwd_kernel(const T* __restrict__ g, const T* __restrict__ x, T* __restrict__ gx,
                                                             float* __restrict__ part, Imp a, long long hw) {
    constexpr int G = HC <= 8 ? 4 : 2;          // channels per block sum in the second walk
    __shared__ float red[2][G * HC][CNT / 64];
    const long long i0 = ((long long)blockIdx.x * CNT + threadIdx.x) * P;
    const bool live = i0 < hw;
    const long long i = live ? i0 : 0;          // a thread beyond the plane reads valid memory and writes nothing
    const float* __restrict__ ft = a.tab;
    const int* __restrict__ it = reinterpret_cast<const int*>(a.tab + T_IMP);
    const int* __restrict__ slot = reinterpret_cast<const int*>(a.tab + T_SLOT);
    const int b = blockIdx.y;
    const T* xb = x + (long long)b * a.C * hw + i;
    const T* gb = g + (long long)b * a.C * hw + i;
    T* gxb = gx + (long long)b * a.C * hw + i;
    const int stride = HC * a.C + HC + a.NI * HC;
    float* pb = part + ((long long)b * gridDim.x + blockIdx.x) * stride;
    float xi[NIC][P], go[NIC][P], h[HC][P], dh[HC][P];
    bool m[NIC][P];
    int par = 0;
    load_imputed<T, P>(xb, a, b, i, hw, xi, m);
    hidden_column<T, P, HC, false>(xb, nullptr, a, hw, xi, h);
    activate<P, HC, true>(a.act, h, dh);          // h is a from here on
#pragma unroll
    for (int j = 0; j < NIC; ++j) mk_ld<T, P>(gb + (long long)it[j] * hw, go[j]);
#pragma unroll
    for (int j = 0; j < NIC; ++j) {
#pragma unroll
        for (int e = 0; e < P; ++e) go[j][e] = (live && m[j][e]) ? go[j][e] : 0.f;
    }
    // gW2[j][k] = sum go_j a_k
#pragma unroll
    for (int j = 0; j < NIC; ++j) {
        if (j < a.NI) {          // (block-uniform)
            float s[HC];
#pragma unroll
            for (int k = 0; k < HC; ++k) {
                s[k] = 0.f;
#pragma unroll
                for (int e = 0; e < P; ++e) s[k] = fmaf(go[j][e], h[k][e], s[k]);
            }
            mk_block_sums_t0<CNT, HC>(s, red[par]);
            par ^= 1;
            if (threadIdx.x == 0) {
#pragma unroll
                for (int k = 0; k < HC; ++k) pb[HC * a.C + HC + j * HC + k] = s[k];
            }
        }
    }
    // gh_k = act'(h_k) sum_j W2[j][k] go_j   (into dh); gb1_k = sum gh_k
#pragma unroll
    for (int k = 0; k < HC; ++k) {
        float ga[P];
#pragma unroll
        for (int e = 0; e < P; ++e) ga[e] = 0.f;
#pragma unroll
        for (int j = 0; j < NIC; ++j) {
            const float w = ft[T_W2 + j * HID + k];          // (zero beyond NI)
#pragma unroll
            for (int e = 0; e < P; ++e) ga[e] = fmaf(w, go[j][e], ga[e]);
        }
#pragma unroll
        for (int e = 0; e < P; ++e) dh[k][e] *= ga[e];
    }
    {
        float s[HC];
#pragma unroll
        for (int k = 0; k < HC; ++k) {
            s[k] = 0.f;
#pragma unroll
            for (int e = 0; e < P; ++e) s[k] += dh[k][e];
        }
        mk_block_sums_t0<CNT, HC>(s, red[par]);
        par ^= 1;
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < HC; ++k) pb[HC * a.C + k] = s[k];
        }
    }
    // the second walk: gx_c = g_c + sum_k W1[k][c] gh_k (0 at the masked entries of an imputed channel), gW1[k][c] = sum gh_k xc_c.
    // G channels per barrier: their 2 G loads are in flight together and their G HC sums share one block sum.
    for (int c0 = 0; c0 < a.C; c0 += G) {
        float v[G][P], gv[G][P], s[G * HC];
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const long long at = (long long)(c0 + u < a.C ? c0 + u : a.C - 1) * hw;
            mk_ld<T, P>(xb + at, v[u]);
            mk_ld<T, P>(gb + at, gv[u]);
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int c = c0 + u < a.C ? c0 + u : a.C - 1;          // (a channel beyond C repeats the last one; nothing of it is kept)
            const bool keep = c0 + u < a.C;          // (block-uniform)
            const int sl = slot[c];
            bool mc[P];
#pragma unroll
            for (int e = 0; e < P; ++e) mc[e] = false;
            if (sl >= 0) {
                pick<P>(xi, sl, v[u]);
                pick<P>(m, sl, mc);
            }
            const float* __restrict__ w = ft + T_W1 + c * HID;
            float acc[P];
#pragma unroll
            for (int e = 0; e < P; ++e) acc[e] = 0.f;
#pragma unroll
            for (int k = 0; k < HC; ++k) {
                const float wk = w[k];
                float t = 0.f;
#pragma unroll
                for (int e = 0; e < P; ++e) {
                    acc[e] = fmaf(wk, dh[k][e], acc[e]);
                    t = fmaf(dh[k][e], v[u][e], t);
                }
                s[u * HC + k] = t;
            }
#pragma unroll
            for (int e = 0; e < P; ++e) acc[e] = mc[e] ? 0.f : gv[u][e] + acc[e];
            if (live && keep) mk_st<T, P>(gxb + (long long)c * hw, acc);
        }
        mk_block_sums_t0<CNT, G * HC>(s, red[par]);
        par ^= 1;
        if (threadIdx.x == 0) {
#pragma unroll
            for (int u = 0; u < G; ++u) {
                if (c0 + u < a.C) {
#pragma unroll
                    for (int k = 0; k < HC; ++k) pb[k * a.C + c0 + u] = s[u * HC + k];
                }
            }
        }
    }
}

// out[q] = the rows' entry q: FIN_S slices of consecutive rows are added in row order by one thread each (the loads of a slice do
// not wait for one another's sums), then the slices in slice order; the order depends on the row count alone.  The block layout
// (gW1 (HC, C) | gb1 (HC) | gW2 (NI, HC)) is unpacked into gW1 (hidden, C), gb1 (hidden), gW2 (NI, hidden).
constexpr int FIN_Q = 16, FIN_S = CNT / FIN_Q;
__global__ __launch_bounds__(CNT) void impute_mlp_finish(const float* __restrict__ part, float* __restrict__ gW1, float* __restrict__ gb1,
                                                         float* __restrict__ gW2, long long rows, int HC, int C, int NI, int hidden) {
    __shared__ float red[FIN_S][FIN_Q];
    const int stride = HC * C + HC + NI * HC;
    const int tq = threadIdx.x % FIN_Q, ts = threadIdx.x / FIN_Q;
    const int q = blockIdx.x * FIN_Q + tq;
    const long long per = (rows + FIN_S - 1) / FIN_S;
    const long long lo = ts * per, hi = lo + per < rows ? lo + per : rows;
    float s = 0.f;
    if (q < stride) {
        for (long long r = lo; r < hi; ++r) s += part[r * stride + q];
    }
    red[ts][tq] = s;
    __syncthreads();
    if (ts != 0 || q >= stride) return;
    float* dst;
    if (q < HC * C) {
        const int k = q / C, c = q - k * C;
        if (k >= hidden) return;
        dst = gW1 + k * C + c;
    } else if (q < HC * C + HC) {
        const int k = q - HC * C;
        if (k >= hidden) return;
        dst = gb1 + k;
    } else {
        const int r = q - HC * C - HC, j = r / HC, k = r - j * HC;
        if (k >= hidden) return;
        dst = gW2 + j * hidden + k;
    }
    float t = 0.f;
    for (int i = 0; i < FIN_S; ++i) t += red[i][tq];
    *dst = t;
}

// ---- constant imputation ---------------------------------------------------------------------------------------------------
struct Cmask {
    const void* mask;
    int kind;
    long long m_sb, m_sc;          // strides over samples and channels in elements (0: broadcast)
};

// grid (pixel groups, C, B)
template <typename T, int P>
__global__ __launch_bounds__(CNT) void impute_const_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ w, Cmask a,
                                                               long long hw) {
    const long long i = ((long long)blockIdx.x * CNT + threadIdx.x) * P;
    if (i >= hw) return;
    const int c = blockIdx.y, b = blockIdx.z;
    const long long at = ((long long)b * gridDim.y + c) * hw + i;
    const float wc = w[c];
    float v[P];
    bool m[P];
    mk_ld<T, P>(x + at, v);
#pragma unroll
    for (int e = 0; e < P; ++e) m[e] = false;
    if (a.kind != MK_IMPUTE_MASK_NONE) ld_mask<P>(a.kind, a.mask, (long long)b * a.m_sb + (long long)c * a.m_sc + i, m);
#pragma unroll
    for (int e = 0; e < P; ++e) v[e] = (m[e] || v[e] != v[e]) ? wc : v[e];
    mk_st<T, P>(y + at, v);
}

// grid (chunks, C, B): block (q, c, b) owns the pixels [q per, (q + 1) per) of plane (b, c); per is a multiple of CNT * 4
template <typename T, int P>
__global__ __launch_bounds__(CNT) void impute_const_bwd_kernel(const T* __restrict__ g, const T* __restrict__ x, T* __restrict__ gx,
                                                               float* __restrict__ part, Cmask a, long long hw, long long per) {
    __shared__ float red[CNT / 64];
    const int c = blockIdx.y, b = blockIdx.z;
    const long long base = ((long long)b * gridDim.y + c) * hw;
    const long long mbase = (long long)b * a.m_sb + (long long)c * a.m_sc;
    const long long lo = (long long)blockIdx.x * per, hi = lo + per < hw ? lo + per : hw;
    float acc = 0.f;
    for (long long i = lo + (long long)threadIdx.x * P; i < hi; i += (long long)CNT * P) {
        float v[P], gv[P];
        bool m[P];
        mk_ld<T, P>(x + base + i, v);
        mk_ld<T, P>(g + base + i, gv);
#pragma unroll
        for (int e = 0; e < P; ++e) m[e] = false;
        if (a.kind != MK_IMPUTE_MASK_NONE) ld_mask<P>(a.kind, a.mask, mbase + i, m);
#pragma unroll
        for (int e = 0; e < P; ++e) {
            const bool me = m[e] || v[e] != v[e];
            acc += me ? gv[e] : 0.f;
            gv[e] = me ? 0.f : gv[e];
        }
        mk_st<T, P>(gx + base + i, gv);
    }
    const float s = mk_block_sum_t0<CNT>(acc, red);
    if (threadIdx.x == 0) part[((long long)c * gridDim.z + b) * gridDim.x + blockIdx.x] = s;
}

// out[j] = the n partial sums of row j added in index order
__global__ __launch_bounds__(CNT) void rows_finish(const float* __restrict__ part, float* __restrict__ out, int rows, long long n) {
    const int j = blockIdx.x * CNT + threadIdx.x;
    if (j >= rows) return;
    float s = 0.f;
    for (long long q = 0; q < n; ++q) s += part[j * n + q];
    out[j] = s;
}

// ---- the output tail -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float soft_clamp(float t) { return t >= 0.5f ? t - 0.25f : (t > 0.f ? t * t : 0.f); }
__device__ __forceinline__ float soft_clamp_d(float t) { return t >= 0.5f ? 1.f : (t > 0.f ? 2.f * t : 0.f); }

// grid (pixel groups, Co, B).  pred (Co) or NULL: no skip
template <typename T, int P>
__global__ __launch_bounds__(CNT) void tail_fwd_kernel(const T* __restrict__ d, const T* __restrict__ xin, T* __restrict__ y,
                                                       const int* __restrict__ pred, const int* __restrict__ water, const float* __restrict__ off,
                                                       int Cin, long long hw) {
    const long long i = ((long long)blockIdx.x * CNT + threadIdx.x) * P;
    if (i >= hw) return;
    const int c = blockIdx.y, b = blockIdx.z;
    const long long at = ((long long)b * gridDim.y + c) * hw + i;
    float v[P];
    mk_ld<T, P>(d + at, v);
    if (pred) {
        float r[P];
        mk_ld<T, P>(xin + ((long long)b * Cin + pred[c]) * hw + i, r);
#pragma unroll
        for (int e = 0; e < P; ++e) v[e] += r[e];
    }
    if (water[c]) {          // (block-uniform)
        const float o = off ? off[c] : 0.f;
#pragma unroll
        for (int e = 0; e < P; ++e) v[e] = soft_clamp(v[e] + o) - o;
    }
    mk_st<T, P>(y + at, v);
}

// grid (pixel groups, Co + NZ, B): rows [0, Co) write gd (and, with the skip, the same values into gxin[pred[c]]); rows beyond
// write zeros into the NZ channels of gxin that no output reads (rest).  d and xin are read on the water channels only.
template <typename T, int P>
__global__ __launch_bounds__(CNT) void tail_bwd_kernel(const T* __restrict__ g, const T* __restrict__ d, const T* __restrict__ xin,
                                                       T* __restrict__ gd, T* __restrict__ gxin, const int* __restrict__ pred,
                                                       const int* __restrict__ water, const float* __restrict__ off, const int* __restrict__ rest,
                                                       int Co, int Cin, long long hw) {
    const long long i = ((long long)blockIdx.x * CNT + threadIdx.x) * P;
    if (i >= hw) return;
    const int c = blockIdx.y, b = blockIdx.z;
    float v[P];
    if (c >= Co) {
#pragma unroll
        for (int e = 0; e < P; ++e) v[e] = 0.f;
        mk_st<T, P>(gxin + ((long long)b * Cin + rest[c - Co]) * hw + i, v);
        return;
    }
    const long long at = ((long long)b * Co + c) * hw + i;
    mk_ld<T, P>(g + at, v);
    if (water[c]) {
        const float o = off ? off[c] : 0.f;
        float t[P];
        mk_ld<T, P>(d + at, t);
        if (pred) {
            float r[P];
            mk_ld<T, P>(xin + ((long long)b * Cin + pred[c]) * hw + i, r);
#pragma unroll
            for (int e = 0; e < P; ++e) t[e] += r[e];
        }
#pragma unroll
        for (int e = 0; e < P; ++e) v[e] *= soft_clamp_d(t[e] + o);
    }
    mk_st<T, P>(gd + at, v);
    if (pred) mk_st<T, P>(gxin + ((long long)b * Cin + pred[c]) * hw + i, v);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
bool dt_ok(int dt) { return dt == MK_F32 || dt == MK_BF16; }

int hidden_cap(int hidden) { return hidden <= 4 ? 4 : hidden <= 8 ? 8 : hidden <= 16 ? 16 : 32; }

int plane_check(const char* what, int dtype, int B, long long hw) {
    MK_REQUIRE(dt_ok(dtype), "%s: the tensors are f32 or bf16", what);
    MK_REQUIRE(B > 0 && B <= 65535, "%s: B = %d outside 1 .. 65535 (one grid row per sample)", what, B);
    MK_REQUIRE(hw > 0 && (hw + CNT - 1) / CNT <= 0x7fffffffLL, "%s: HW = %lld pixels per plane: not positive, or beyond the grid", what, hw);
    return 0;
}

int mask_check(const char* what, const void* mask, int kind, bool channel_ok) {
    MK_REQUIRE(kind >= MK_IMPUTE_MASK_NONE && kind <= (channel_ok ? MK_IMPUTE_MASK_CHANNEL : MK_IMPUTE_MASK_BF16),
               "%s: mask kind %d (0 none, 1 bool, 2 f32, 3 bf16%s)", what, kind, channel_ok ? ", 4 a channel of x" : "");
    MK_REQUIRE(mask || kind == MK_IMPUTE_MASK_NONE || kind == MK_IMPUTE_MASK_CHANNEL, "%s: mask kind %d without a mask", what, kind);
    return 0;
}

int mlp_check(const char* what, const void* a, const void* b, const float* tab, const void* mask, int kind, int Nm, long long m_sb, int mask_ch,
              int act, int dtype, int B, int C, int NI, int hidden, long long hw) {
    MK_REQUIRE(a && b && tab, "%s: null pointer (the tensors and the table are required)", what);
    if (int rc = plane_check(what, dtype, B, hw)) return rc;
    if (int rc = mask_check(what, mask, kind, true)) return rc;
    if (C < 1 || C > CMAX || NI < 1 || NI > NIC || NI > C || hidden < 1 || hidden > HID) {
        mk_set_error("%s: C = %d, NI = %d, hidden = %d outside 1 .. %d channels, 1 .. %d imputed channels, 1 .. %d hidden units", what, C, NI,
                     hidden, CMAX, NIC, HID);
        return MK_EUNSUP;
    }
    MK_REQUIRE(act >= MK_IMPUTE_ACT_GELU && act <= MK_IMPUTE_ACT_SIN, "%s: activation %d (0 gelu, 1 relu, 2 silu, 3 sin)", what, act);
    if (kind == MK_IMPUTE_MASK_CHANNEL) MK_REQUIRE(mask_ch >= 0 && mask_ch < C, "%s: mask channel %d outside 0 .. %d", what, mask_ch, C - 1);
    if (kind >= MK_IMPUTE_MASK_BOOL && kind <= MK_IMPUTE_MASK_BF16) {
        MK_REQUIRE(Nm == 1 || Nm == NI, "%s: the mask has %d planes, not 1 or NI = %d", what, Nm, NI);
        MK_REQUIRE(m_sb == 0 || m_sb >= (long long)Nm * hw, "%s: mask sample stride %lld is neither 0 nor at least Nm HW", what, m_sb);
    }
    return 0;
}

template <typename T, int P>
void mlp_fwd_launch(int cap, const void* x, void* y, const Imp& d, int B, long long hw, hipStream_t st) {
    const dim3 grid((unsigned)((hw + (long long)CNT * P - 1) / ((long long)CNT * P)), (unsigned)B);
    if (cap == 4) hipLaunchKernelGGL((impute_mlp_fwd_kernel<T, P, 4>), grid, dim3(CNT), 0, st, (const T*)x, (T*)y, d, hw);
    else if (cap == 8) hipLaunchKernelGGL((impute_mlp_fwd_kernel<T, P, 8>), grid, dim3(CNT), 0, st, (const T*)x, (T*)y, d, hw);
    else if (cap == 16) hipLaunchKernelGGL((impute_mlp_fwd_kernel<T, P, 16>), grid, dim3(CNT), 0, st, (const T*)x, (T*)y, d, hw);
    else if constexpr (P == 1) hipLaunchKernelGGL((impute_mlp_fwd_kernel<T, 1, 32>), grid, dim3(CNT), 0, st, (const T*)x, (T*)y, d, hw);
}

template <typename T, int P>
void mlp_bwd_launch(int cap, const void* g, const void* x, void* gx, float* part, const Imp& d, int B, long long hw, hipStream_t st) {
    const dim3 grid((unsigned)((hw + (long long)CNT * P - 1) / ((long long)CNT * P)), (unsigned)B);
    if (cap == 4) hipLaunchKernelGGL((impute_mlp_bwd_kernel<T, P, 4>), grid, dim3(CNT), 0, st, (const T*)g, (const T*)x, (T*)gx, part, d, hw);
    else if (cap == 8) hipLaunchKernelGGL((impute_mlp_bwd_kernel<T, P, 8>), grid, dim3(CNT), 0, st, (const T*)g, (const T*)x, (T*)gx, part, d, hw);
    else if (cap == 16) hipLaunchKernelGGL((impute_mlp_bwd_kernel<T, P, 16>), grid, dim3(CNT), 0, st, (const T*)g, (const T*)x, (T*)gx, part, d, hw);
    else if constexpr (P == 1) hipLaunchKernelGGL((impute_mlp_bwd_kernel<T, 1, 32>), grid, dim3(CNT), 0, st, (const T*)g, (const T*)x, (T*)gx, part, d, hw);
}

// the vector forms need every address a multiple of the access: HW, the mask's sample stride and every pointer.  (The MLP kernels
// take them up to the 16-row capacity: 32 rows of four pixels, twice in the backward pass, do not fit the register file, and the
// one-pixel form of that capacity does without scratch.)
bool vec_ok(long long hw, long long m_sb, long long m_sc, const void* a, const void* b, const void* c, const void* mask) {
    return hw % 4 == 0 && m_sb % 4 == 0 && m_sc % 4 == 0 && mk_aligned16(a) && mk_aligned16(b) && mk_aligned16(c) && mk_aligned16(mask);
}

long long mlp_blocks(long long hw, bool vec) {
    const long long per = (long long)CNT * (vec ? 4 : 1);
    return (hw + per - 1) / per;
}

}  // namespace

extern "C" int mk_impute_mlp_fwd(const void* x, void* y, int dtype, const float* tab, const void* mask, int mask_kind, int Nm, long long m_sb,
                                 int mask_ch, int act, int B, int C, int NI, int hidden, long long hw, void* stream) {
    if (int rc = mlp_check("mk_impute_mlp_fwd", x, y, tab, mask, mask_kind, Nm, m_sb, mask_ch, act, dtype, B, C, NI, hidden, hw)) return rc;
    const Imp d{tab, mask, m_sb, mask_kind, Nm, mask_ch, C, NI, act};
    hipStream_t st = (hipStream_t)stream;
    const int cap = hidden_cap(hidden);
    const bool vec = cap <= 16 && vec_ok(hw, m_sb, 0, x, y, nullptr, mask);
    if (dtype == MK_BF16) {
        if (vec) mlp_fwd_launch<u16, 4>(cap, x, y, d, B, hw, st);
        else mlp_fwd_launch<u16, 1>(cap, x, y, d, B, hw, st);
    } else {
        if (vec) mlp_fwd_launch<float, 4>(cap, x, y, d, B, hw, st);
        else mlp_fwd_launch<float, 1>(cap, x, y, d, B, hw, st);
    }
    return mk_check_launch("mk_impute_mlp_fwd");
}

extern "C" long long mk_impute_mlp_workspace(int B, int C, int NI, int hidden, long long hw) {
    if (B < 1 || C < 1 || NI < 1 || hidden < 1 || hw < 1) return 0;
    const int cap = hidden_cap(hidden);
    return (long long)B * mlp_blocks(hw, false) * ((long long)cap * C + cap + (long long)NI * cap);          // (the P = 1 grid: the larger one)
}

extern "C" int mk_impute_mlp_bwd(const void* g, const void* x, void* gx, float* gW1, float* gb1, float* gW2, float* ws, int dtype,
                                 const float* tab, const void* mask, int mask_kind, int Nm, long long m_sb, int mask_ch, int act, int B, int C,
                                 int NI, int hidden, long long hw, void* stream) {
    if (int rc = mlp_check("mk_impute_mlp_bwd", g, x, tab, mask, mask_kind, Nm, m_sb, mask_ch, act, dtype, B, C, NI, hidden, hw)) return rc;
    MK_REQUIRE(gx && gW1 && gb1 && gW2 && ws, "mk_impute_mlp_bwd: null pointer (gx, the three weight gradients and the workspace are required)");
    const Imp d{tab, mask, m_sb, mask_kind, Nm, mask_ch, C, NI, act};
    hipStream_t st = (hipStream_t)stream;
    const int cap = hidden_cap(hidden);
    const bool vec = cap <= 16 && vec_ok(hw, m_sb, 0, g, x, gx, mask);
    if (dtype == MK_BF16) {
        if (vec) mlp_bwd_launch<u16, 4>(cap, g, x, gx, ws, d, B, hw, st);
        else mlp_bwd_launch<u16, 1>(cap, g, x, gx, ws, d, B, hw, st);
    } else {
        if (vec) mlp_bwd_launch<float, 4>(cap, g, x, gx, ws, d, B, hw, st);
        else mlp_bwd_launch<float, 1>(cap, g, x, gx, ws, d, B, hw, st);
    }
    const int stride = cap * C + cap + NI * cap;
    hipLaunchKernelGGL(impute_mlp_finish, dim3((unsigned)((stride + FIN_Q - 1) / FIN_Q)), dim3(CNT), 0, st, (const float*)ws, gW1, gb1, gW2,
                       (long long)B * mlp_blocks(hw, vec), cap, C, NI, hidden);
    return mk_check_launch("mk_impute_mlp_bwd");
}

namespace {

int const_check(const char* what, const void* a, const void* b, const float* w, const void* mask, int kind, long long m_sb, long long m_sc,
                int dtype, int B, int C, long long hw) {
    MK_REQUIRE(a && b && w, "%s: null pointer (the tensors and the fill values are required)", what);
    if (int rc = plane_check(what, dtype, B, hw)) return rc;
    if (int rc = mask_check(what, mask, kind, false)) return rc;
    MK_REQUIRE(C > 0 && C <= 65535, "%s: C = %d outside 1 .. 65535", what, C);
    MK_REQUIRE(m_sb >= 0 && m_sc >= 0, "%s: negative mask strides", what);
    return 0;
}

}  // namespace

extern "C" int mk_impute_const_fwd(const void* x, void* y, int dtype, const float* w, const void* mask, int mask_kind, long long m_sb,
                                   long long m_sc, int B, int C, long long hw, void* stream) {
    if (int rc = const_check("mk_impute_const_fwd", x, y, w, mask, mask_kind, m_sb, m_sc, dtype, B, C, hw)) return rc;
    const Cmask d{mask, mask_kind, m_sb, m_sc};
    hipStream_t st = (hipStream_t)stream;
    const bool vec = vec_ok(hw, m_sb, m_sc, x, y, nullptr, mask);
    const int P = vec ? 4 : 1;
    const dim3 grid((unsigned)((hw + (long long)CNT * P - 1) / ((long long)CNT * P)), (unsigned)C, (unsigned)B);
    if (dtype == MK_BF16) {
        if (vec) hipLaunchKernelGGL((impute_const_fwd_kernel<u16, 4>), grid, dim3(CNT), 0, st, (const u16*)x, (u16*)y, w, d, hw);
        else hipLaunchKernelGGL((impute_const_fwd_kernel<u16, 1>), grid, dim3(CNT), 0, st, (const u16*)x, (u16*)y, w, d, hw);
    } else {
        if (vec) hipLaunchKernelGGL((impute_const_fwd_kernel<float, 4>), grid, dim3(CNT), 0, st, (const float*)x, (float*)y, w, d, hw);
        else hipLaunchKernelGGL((impute_const_fwd_kernel<float, 1>), grid, dim3(CNT), 0, st, (const float*)x, (float*)y, w, d, hw);
    }
    return mk_check_launch("mk_impute_const_fwd");
}

extern "C" int mk_impute_chunks(long long hw) { return mk_plane_chunks(hw); }

extern "C" int mk_impute_const_bwd(const void* g, const void* x, void* gx, float* gw, float* ws, int dtype, const void* mask, int mask_kind,
                                   long long m_sb, long long m_sc, int B, int C, long long hw, void* stream) {
    if (int rc = const_check("mk_impute_const_bwd", g, x, gw, mask, mask_kind, m_sb, m_sc, dtype, B, C, hw)) return rc;
    MK_REQUIRE(gx && ws, "mk_impute_const_bwd: null pointer (gx and the workspace of B * C * mk_impute_chunks(HW) floats are required)");
    const Cmask d{mask, mask_kind, m_sb, m_sc};
    hipStream_t st = (hipStream_t)stream;
    const bool vec = vec_ok(hw, m_sb, m_sc, g, x, gx, mask);
    const int chunks = mk_plane_chunks(hw);
    const long long unit = (long long)CNT * 4;
    const long long per = ((hw + chunks - 1) / chunks + unit - 1) / unit * unit;
    const dim3 grid((unsigned)chunks, (unsigned)C, (unsigned)B);
    float* part = ws;
    if (dtype == MK_BF16) {
        if (vec) hipLaunchKernelGGL((impute_const_bwd_kernel<u16, 4>), grid, dim3(CNT), 0, st, (const u16*)g, (const u16*)x, (u16*)gx, part, d, hw, per);
        else hipLaunchKernelGGL((impute_const_bwd_kernel<u16, 1>), grid, dim3(CNT), 0, st, (const u16*)g, (const u16*)x, (u16*)gx, part, d, hw, per);
    } else {
        if (vec) hipLaunchKernelGGL((impute_const_bwd_kernel<float, 4>), grid, dim3(CNT), 0, st, (const float*)g, (const float*)x, (float*)gx, part, d, hw, per);
        else hipLaunchKernelGGL((impute_const_bwd_kernel<float, 1>), grid, dim3(CNT), 0, st, (const float*)g, (const float*)x, (float*)gx, part, d, hw, per);
    }
    hipLaunchKernelGGL(rows_finish, dim3((unsigned)((C + CNT - 1) / CNT)), dim3(CNT), 0, st, (const float*)part, gw, C, (long long)B * chunks);
    return mk_check_launch("mk_impute_const_bwd");
}

namespace {

int tail_check(const char* what, const void* a, const void* b, const void* xin, const int* pred, const int* water, int dtype, int B, int Co,
               int Cin, long long hw) {
    MK_REQUIRE(a && b && water, "%s: null pointer (the tensors and the water flags are required)", what);
    if (int rc = plane_check(what, dtype, B, hw)) return rc;
    MK_REQUIRE(Co > 0 && Co <= 65535, "%s: Co = %d outside 1 .. 65535", what, Co);
    MK_REQUIRE(!pred || (xin && Cin >= Co && Cin <= 65535), "%s: the skip needs the input and Co = %d <= Cin = %d <= 65535", what, Co, Cin);
    return 0;
}

}  // namespace

extern "C" int mk_fcn31_tail_fwd(const void* d, const void* xin, void* y, int dtype, const int* pred_ch, const int* water, const float* off, int B,
                                 int Co, int Cin, long long hw, void* stream) {
    if (int rc = tail_check("mk_fcn31_tail_fwd", d, y, xin, pred_ch, water, dtype, B, Co, Cin, hw)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = vec_ok(hw, 0, 0, d, y, pred_ch ? xin : nullptr, nullptr);
    const int P = vec ? 4 : 1;
    const dim3 grid((unsigned)((hw + (long long)CNT * P - 1) / ((long long)CNT * P)), (unsigned)Co, (unsigned)B);
    if (dtype == MK_BF16) {
        if (vec) hipLaunchKernelGGL((tail_fwd_kernel<u16, 4>), grid, dim3(CNT), 0, st, (const u16*)d, (const u16*)xin, (u16*)y, pred_ch, water, off, Cin, hw);
        else hipLaunchKernelGGL((tail_fwd_kernel<u16, 1>), grid, dim3(CNT), 0, st, (const u16*)d, (const u16*)xin, (u16*)y, pred_ch, water, off, Cin, hw);
    } else {
        if (vec) hipLaunchKernelGGL((tail_fwd_kernel<float, 4>), grid, dim3(CNT), 0, st, (const float*)d, (const float*)xin, (float*)y, pred_ch, water, off, Cin, hw);
        else hipLaunchKernelGGL((tail_fwd_kernel<float, 1>), grid, dim3(CNT), 0, st, (const float*)d, (const float*)xin, (float*)y, pred_ch, water, off, Cin, hw);
    }
    return mk_check_launch("mk_fcn31_tail_fwd");
}

extern "C" int mk_fcn31_tail_bwd(const void* g, const void* d, const void* xin, void* gd, void* gxin, int dtype, const int* pred_ch,
                                 const int* water, const float* off, const int* rest, int B, int Co, int Cin, long long hw, void* stream) {
    if (int rc = tail_check("mk_fcn31_tail_bwd", g, gd, xin, pred_ch, water, dtype, B, Co, Cin, hw)) return rc;
    MK_REQUIRE(d, "mk_fcn31_tail_bwd: null pointer (the saved decoder output is required)");
    MK_REQUIRE(!pred_ch || (gxin && (rest || Cin == Co)), "mk_fcn31_tail_bwd: the skip needs gxin and the list of the Cin - Co other channels");
    hipStream_t st = (hipStream_t)stream;
    const int NZ = pred_ch ? Cin - Co : 0;
    MK_REQUIRE(Co + NZ <= 65535, "mk_fcn31_tail_bwd: Co + (Cin - Co) = %d beyond 65535 grid rows", Co + NZ);
    const bool vec = vec_ok(hw, 0, 0, g, gd, d, nullptr) && (!pred_ch || (mk_aligned16(xin) && mk_aligned16(gxin)));
    const int P = vec ? 4 : 1;
    const dim3 grid((unsigned)((hw + (long long)CNT * P - 1) / ((long long)CNT * P)), (unsigned)(Co + NZ), (unsigned)B);
    if (dtype == MK_BF16) {
        if (vec) hipLaunchKernelGGL((tail_bwd_kernel<u16, 4>), grid, dim3(CNT), 0, st, (const u16*)g, (const u16*)d, (const u16*)xin, (u16*)gd, (u16*)gxin, pred_ch, water, off, rest, Co, Cin, hw);
        else hipLaunchKernelGGL((tail_bwd_kernel<u16, 1>), grid, dim3(CNT), 0, st, (const u16*)g, (const u16*)d, (const u16*)xin, (u16*)gd, (u16*)gxin, pred_ch, water, off, rest, Co, Cin, hw);
    } else {
        if (vec) hipLaunchKernelGGL((tail_bwd_kernel<float, 4>), grid, dim3(CNT), 0, st, (const float*)g, (const float*)d, (const float*)xin, (float*)gd, (float*)gxin, pred_ch, water, off, rest, Co, Cin, hw);
        else hipLaunchKernelGGL((tail_bwd_kernel<float, 1>), grid, dim3(CNT), 0, st, (const float*)g, (const float*)d, (const float*)xin, (float*)gd, (float*)gxin, pred_ch, water, off, rest, Co, Cin, hw);
    }
    return mk_check_launch("mk_fcn31_tail_bwd");
}
