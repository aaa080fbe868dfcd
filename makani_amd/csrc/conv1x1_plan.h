// Which kernel mk_conv1x1_nn launches for a shape.  Plain C++ without HIP, so that the CPU suite can compile this file on its
// own and check the table of the networks' shapes (tests/test_host_logic.py).  Below it the plan of the weight gradient
// (wgrad_plan), which tests/test_conv_exact_cases.py checks the exact-data case tables against.
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

// mk_conv1x1_nn_rnorm (the skip GEMM that normalises its residual operand where it adds it) exists on the two-group kernel only:
// true exactly where the plain call with a residual operand plans it.
inline bool conv_nn_rnorm_supported(int M, int K, int lda, int B, long long N, int astat2_env) {
    return conv_nn_plan(M, K, lda, B, N, /*pre=*/false, /*has_r=*/true, /*has_g=*/false, astat2_env) == ConvNnKernel::astat2;
}

// Tile height of the ring kernel (output channels per tile; the tile is 256 pixels wide): 256 where M is made of whole 256-row tiles
// or is large, else 192 — and ONE 384-row tile where that would be two of 192 under a long contraction (384 <- 768, the MLP's second
// layer and the data gradient of its first).  Per 256 pixels the two 192-row tiles ingest 2 x (192 x K weights + K x 256 activations),
// the 384-row tile 384 x K + K x 256: 10 bytes per output element instead of 14, and the memory path of the CU is what bounds the
// kernel (docs/LAB_NOTEBOOK.md 6.12).  The 384-row tile has 192 accumulator registers per lane: it exists
// without epilogue operands only (has_epilogue: activation, stored pre-activation, residual or gelu' operand; a bias is none), and
// it halves the tile count, so it needs as many tiles as the persistent grid has workgroups (256) — the shards of one rank keep
// two tiles.  K = 384 stays with 192 rows: full grids of it run weight-stationary, only shards reach the ring kernel.
// ring384_env: MAKANI_AMD_RING384 (negative = unset; 0 = never the 384-row tile, for A/B runs).
inline int conv_nn_ring_rows(int M, int K, int B, long long N, bool has_epilogue, int ring384_env) {
    const int rows = ((M % 256 == 0) || M > 576) ? 256 : 192;
    const long long tiles384 = ((N + 255) / 256) * B;
    if (rows == 192 && M > 192 && M <= 384 && K >= 512 && !has_epilogue && tiles384 >= 256 && ring384_env != 0) return 384;
    return rows;
}

// ---- host-side plan of the weight gradient (mk_conv1x1_wgrad, mk_conv1x1_wgrad_bias) ----------
struct WgPlan {
    bool ring;          // ring kernel (big tiles) or the 128 x 128 tile kernel
    bool swap;          // ring: P = X, Q = G
    int tp;             // ring: slab height (256 / 192)
    int slabs;
    int qslabs;         // ring: 384-row slabs of Q
    long long S;        // pixel splits (all batch entries)
    long long chunk;    // pixels per split
};

inline WgPlan wgrad_plan(int M, int K, int B, long long N) {
    WgPlan pl{};
    const int big = M > K ? M : K, small = M > K ? K : M;
    // ring kernel: the smaller channel count fits one 384-row tile, the other one is cut into slabs; 32-bit byte
    // offsets inside one batch entry; at least a few pixel tiles per split
    if (big >= 96 && N * 2 * 384 < (1ll << 31) && N >= 2048) {
        pl.ring = true;
        int q, pr;                                   // rows of Q (384-row slabs; one slab = held in full) and of P (slabs of tp)
        if (big <= 384) { q = big; pr = small; }
        else if (small <= 384) { q = small; pr = big; }
        else { q = big; pr = small; }                // both large (FourCastNet3): the longer operand in 384-row slabs
        // Q = X (k) unless that puts the larger operand in P's place the wrong way round
        const bool q_is_x = (K == q) && !(M == q && M > K);
        pl.swap = !q_is_x;
        pl.tp = (pr > 192 && pr % 256 != 192 && (pr % 192 != 0 || pr % 256 == 0)) ? 256 : 192;
        if (pr <= 192) pl.tp = 192;
        pl.slabs = (pr + pl.tp - 1) / pl.tp;
        pl.qslabs = (q + 383) / 384;
        long long per_b = 256 / ((long long)pl.slabs * pl.qslabs * B);
        if (per_b < 1) per_b = 1;
        // at least 512 pixels (8 tiles of 64) per split.  1024 left most of the chip idle on shard-sized grids (14 400 pixels per rank
        // at h4 w2: 45 workgroups); 512: -20 ... -25 % per launch there, +-1 % at 115 200 pixels and above, 256 / 128 no better
        // (profiles/r05_ab_wgrad_shard_minpx.txt)
        const long long maxs = (N + 511) / 512;
        if (per_b > maxs) per_b = maxs;
        long long chunk = ((N + per_b - 1) / per_b + 63) / 64 * 64;
        per_b = (N + chunk - 1) / chunk;             // no empty splits
        pl.chunk = chunk;
        pl.S = per_b * B;
        return pl;
    }
    const int tiles = ((M + 127) / 128) * ((K + 127) / 128);
    long long per_b = 1024 / ((long long)tiles * B);
    if (per_b < 1) per_b = 1;
    const long long maxs = (N + 2047) / 2048;        // at least 2048 pixels per split
    if (per_b > maxs) per_b = maxs;
    long long chunk = (N + per_b - 1) / per_b;
    chunk = (chunk + 127) / 128 * 128;
    pl.chunk = chunk;
    pl.S = per_b * B;
    return pl;
}
