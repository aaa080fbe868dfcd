// Which kernel mk_conv1x1_nn launches for a shape.  Plain C++ without HIP, so that the CPU suite can compile this file on its
// own and check the table of the networks' shapes (tests/test_host_logic.py).
#pragma once

enum class ConvNnKernel {
    astat73,    // weight-stationary kernel for the 73-channel edges (K padded to lda = 80): 5 k16-steps, one 96-row chunk per tile
    astat2,     // weight-stationary, two wave groups: one multiplies while the other runs its epilogue
    astat1,     // weight-stationary, one group (MAKANI_AMD_ASTAT2=0 only)
    ring,       // persistent ring kernel, one 512-thread workgroup per CU
    tile        // 128-row tile kernel
};

// pre: activation with the pre-activation stored as a second output; has_r / has_g: residual / gelu' epilogue operand.
// astat2_env: MAKANI_AMD_ASTAT2 (negative = unset; 0 = the one-group kernel; 1 = the two-group kernel also on shard-sized grids).
// What the two-group kernel gains over the one-group kernel: profiles/r04_ab_astat2.txt and docs/LAB_NOTEBOOK.md round 6.
inline ConvNnKernel conv_nn_plan(int M, int K, int lda, int B, long long N, bool pre, bool has_r, bool has_g, int astat2_env) {
    // weights stationary in registers: 384-row slabs of at least 256 rows, 32-bit byte offsets inside a batch entry of the output,
    // at most one epilogue operand
    const bool stationary = M >= 256 && (long long)M * N * 2 < (1ll << 31) && N >= 64 && !(has_r && has_g);
    if (stationary && lda == 80 && K > 64 && K <= 80 && (long long)K * N * 2 < (1ll << 32) && !((has_r || has_g) && pre))
        return ConvNnKernel::astat73;
    // shard-sized grids (one rank of h4 w2 holds 14 400 ... 32 400 pixels of the internal grid): for 384 <- 384 the ring kernel beats the
    // weight-stationary ones by 10 - 25 % there (plain 14.5 / 16.3 us against 18.8 / 21.8, + skip operand 16.3 / 18.4 against 18.2 / 24.3:
    // profiles/r05_ab_conv_shard_kernel_choice.txt); from 115 200 pixels on the stationary kernels win everywhere
    const bool small_ring = M == 384 && (long long)B * N <= 32768 && !pre && astat2_env != 1;
    if (stationary && K == 384 && !small_ring) return astat2_env == 0 ? ConvNnKernel::astat1 : ConvNnKernel::astat2;
    if (K >= 64 && M >= 192 && N * 2 * 64 < (1ll << 31) && (long long)M * lda * 2 < (1ll << 31) && N >= 256) return ConvNnKernel::ring;
    return ConvNnKernel::tile;
}
