// Column-block repack of the vector transform's operands (gfx950): the pack and unpack side of the pair-axis exchanges of
// DistributedRealVectorSHT / DistributedInverseRealVectorSHT (makani_amd/distributed.py).
//
// The last axis of a vector F / S tensor is [re/im][kind][Rp] (csrc/vlegendre.hip): `blocks` = 4 (2 for the s-only / t = 0
// forms) column blocks of Rp columns each, Rp = pairs rounded up to 32.  Splitting or joining PAIRS over the ranks of a group
// therefore touches every block of every row.  One launch copies, for outer x inner rows of `blocks` blocks,
//     dst[o][i][blk][dst_c0 + c] = src[o][i][blk][src_c0 + c]        c in [0, ncols)
// where the blocks of src / dst are src_rp / dst_rp wide, a row is blocks * rp floats, the inner rows follow one another and
// src / dst each have their own OUTER stride (an arriving slab lands in a latitude range of the result, which is not the
// outermost axis).  `zero_tail`: the columns [dst_c0 + ncols, dst_rp) of every block are written as exact zeros (the Legendre
// kernel reads the pad columns of its operand).  Nothing else of dst is touched.
//   pack    src = the padded operand, src_c0 = the peer's first pair   -> dst = the send slab, dst_rp = ncols (no padding:
//           only valid pairs cross the fabric)
//   unpack  src = an arrived slab (src_rp = ncols)                     -> dst = the padded operand at the sender's pair offset
// The distributed pair uses the kernel for unpack and for a rank's own share (operand to operand); its pack is a strided copy,
// which measured faster than this kernel (docs/LAB_NOTEBOOK.md 6.13).
// A pure stream: every element is read once and written once, 16-byte accesses when every extent, offset and stride is a
// multiple of 4 floats and both bases are 16-byte aligned, 4-byte ones otherwise.  No host reads, no allocation: safe inside a
// captured hipGraph.
#include "common.h"

namespace {

constexpr int VR_NT = 256;

// V floats per access; I: index type (unsigned while the element count fits, long long beyond)
template <int V, typename I>
__global__ __launch_bounds__(VR_NT) void vcols_repack_kernel(const float* __restrict__ src, float* __restrict__ dst, I total, I wv,
                                                             I rows_in, int ncols, long long src_outer, long long dst_outer,
                                                             int src_rp, int dst_rp, int src_c0, int dst_c0) {
    // element i = ((o * rows_in + ib) * wv + cv): o the outer index, ib = inner row * blocks + block, cv the column vector
    for (I i = (I)blockIdx.x * VR_NT + threadIdx.x; i < total; i += (I)gridDim.x * VR_NT) {
        const I q = i / wv;
        const int c = (int)(i - q * wv) * V;
        const I o = q / rows_in;
        const I ib = q - o * rows_in;
        float* d = dst + (long long)o * dst_outer + (long long)ib * dst_rp + dst_c0 + c;
        if (c < ncols) {
            const float* s = src + (long long)o * src_outer + (long long)ib * src_rp + src_c0 + c;
            if constexpr (V == 4)
                *reinterpret_cast<f32x4*>(d) = *reinterpret_cast<const f32x4*>(s);
            else
                *d = *s;
        } else {
            if constexpr (V == 4)
                *reinterpret_cast<f32x4*>(d) = f32x4{0.f, 0.f, 0.f, 0.f};
            else
                *d = 0.f;
        }
    }
}

template <int V>
void launch_repack(const float* src, float* dst, long long rows, long long rows_in, int wcols, int ncols, long long src_outer,
                   long long dst_outer, int src_rp, int dst_rp, int src_c0, int dst_c0, hipStream_t s) {
    const long long wv = wcols / V, total = rows * wv;
    const long long want = (total + VR_NT - 1) / VR_NT;
    const unsigned grid = (unsigned)(want < 256 * 32 ? want : 256 * 32);          // 32 workgroups per CU, then a grid-stride loop
    if (total < (1ll << 31) - (long long)grid * VR_NT)
        hipLaunchKernelGGL((vcols_repack_kernel<V, unsigned>), dim3(grid), dim3(VR_NT), 0, s, src, dst, (unsigned)total, (unsigned)wv,
                           (unsigned)rows_in, ncols, src_outer, dst_outer, src_rp, dst_rp, src_c0, dst_c0);
    else
        hipLaunchKernelGGL((vcols_repack_kernel<V, long long>), dim3(grid), dim3(VR_NT), 0, s, src, dst, total, wv, rows_in, ncols,
                           src_outer, dst_outer, src_rp, dst_rp, src_c0, dst_c0);
}

}  // namespace

extern "C" int mk_vcols_repack(const float* src, float* dst, long long outer, long long inner, int blocks, int ncols,
                               long long src_outer, int src_rp, int src_c0, long long dst_outer, int dst_rp, int dst_c0,
                               int zero_tail, void* stream) {
    MK_REQUIRE(outer >= 0 && inner >= 0 && blocks >= 1 && ncols >= 0, "vcols_repack: negative extent");
    MK_REQUIRE(src_c0 >= 0 && dst_c0 >= 0 && src_c0 + (long long)ncols <= src_rp && dst_c0 + (long long)ncols <= dst_rp,
               "vcols_repack: columns [%d, %d + %d) / [%d, %d + %d) leave a block of %d / %d", src_c0, src_c0, ncols, dst_c0, dst_c0,
               ncols, src_rp, dst_rp);
    const long long rows_in = inner * blocks;
    MK_REQUIRE(rows_in < (1ll << 31), "vcols_repack: inner * blocks must fit 31 bits");
    MK_REQUIRE(outer <= 1 || (src_outer >= rows_in * src_rp && dst_outer >= rows_in * dst_rp),
               "vcols_repack: an outer stride is smaller than inner * blocks * rp (rows would overlap)");
    const int wcols = zero_tail ? dst_rp - dst_c0 : ncols;               // columns written per block
    if (outer == 0 || inner == 0 || ncols == 0) return 0;               // nothing to move: no launch
    MK_REQUIRE(src && dst, "vcols_repack: null pointer");
    const bool v4 = ((ncols | wcols | src_rp | dst_rp | src_c0 | dst_c0) & 3) == 0 && ((src_outer | dst_outer) & 3) == 0 &&
                    (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (v4)
        launch_repack<4>(src, dst, outer * rows_in, rows_in, wcols, ncols, src_outer, dst_outer, src_rp, dst_rp, src_c0, dst_c0, s);
    else
        launch_repack<1>(src, dst, outer * rows_in, rows_in, wcols, ncols, src_outer, dst_outer, src_rp, dst_rp, src_c0, dst_c0, s);
    return mk_check_launch("mk_vcols_repack");
}
