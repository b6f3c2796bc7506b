// Host arithmetic of the training operators (mdx_train.hip, mdx_train_rows.hip, mdx_train_fused.hip) that more than one place has to agree on: where the split partials of a
// weight gradient live, which tile class a queued weight gradient takes, how many partial rows the LayerNorm backward leaves, how the
// deferred reduction numbers its blocks, which shapes the row-owner GEMM takes, and the grid of the fused row-owner operators.  Plain C++17, no HIP and no torch: mdx_train.hip
// (launchers and reduce_deferred_kernel), mdx_train_fused.hip (launchers) and mdx_fast.cpp (buffer sizes, the gradient sink's record table) include it, and
// tools/train_plan_host_check.cpp builds it on its own with a host compiler and enumerates it.  The functions are constexpr, so the
// device compiler accepts them inside a kernel as they are.
#pragma once
#include <cstdint>

constexpr int W_MC = 32;        // rows of G and X the fp32 weight-gradient kernel stages per step: its row chunk
constexpr int HW_MC = 64;       // ... the half-precision weight-gradient kernels
constexpr int RED_CHUNK = 256;  // partials one reduction stage sums; more go through a first stage of ceil(S / RED_CHUNK) chunk sums
constexpr int MDX_LN_RPW = 16;  // rows per wave in the LayerNorm backward (16: 9.7 k waves for E = 155 k rows; 64 left the chip half empty)
constexpr int RED_ELEMS = 128;  // output elements per block of the deferred reduction (32 lanes x 4 elements)

constexpr int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- split partials of a weight gradient dW (N,K) = G (M,N)^T X (M,K) ---------------------------------------------------------------
// The M rows are cut into S ranges of `mper` rows (a multiple of the kernel's row chunk).  The partial area, in floats from its start:
//   [S][N*K] products | [nc][N*K] chunk sums of the first reduction stage (at stage_off) | [S][N] bias partials (at bias_off) |
//   [nc][N] their chunk sums (at bias_off + S*N);   nc = ceil(S / RED_CHUNK), total = (S + nc) * (N*K + N).
struct SplitLayout {
  int64_t mper, S, nc, stage_off, bias_off, total;
};
constexpr SplitLayout split_layout_rows(int64_t M, int64_t N, int64_t K, int64_t mper) {
  const int64_t S = ceil_div(M > 1 ? M : 1, mper), nc = ceil_div(S, RED_CHUNK);
  return {mper, S, nc, S * N * K, (S + nc) * N * K, (S + nc) * (N * K + N)};
}
// `splits` is the caller's wish (an upper bound of S): rows per range = ceil(M / splits), rounded up to the row chunk
constexpr SplitLayout split_layout(int64_t M, int64_t N, int64_t K, int64_t splits, int chunk) {
  const int64_t mper = ceil_div(M > 1 ? M : 1, splits > 1 ? splits : 1);
  return split_layout_rows(M, N, K, ceil_div(mper, chunk) * chunk);
}

// ---- the weight-gradient queue (wgrad_grouped_kernel) ---------------------------------------------------------------------------------
// Tile class of a contraction, its tiles (gx along K, gy along N), its row ranges and blocks.  dt: bit 0 G float16, bit 1 X float16;
// `aligned`: both operands start on 16 bytes.  Classes 0..3: transpose-read kernel with tiles 128x128, 128x64, 64x128, 64x64;
// 4: converting kernel, 64x64; 5 / 6: transpose-read kernel with 32x64 / 64x32 tiles; 7: one output row or one input column.
struct WgradPlan {
  int kind;
  int64_t gx, gy;
  SplitLayout lay;
  int64_t blocks;
};
// Rows per block by tile class (0 = the caller's): the classes with few, small tiles per row range do not fill the chip at the queue's
// 2,048 rows per block.  Measured per class (us per step, 2,048 -> shipped): 64x128 170 -> 165, 64x64 171 -> 156, converting 64x64
// 318 -> 240, 32x64 133 -> 113, 64x32 72 -> 81; the deferred reduction 214 -> 227 (profiles/HISTORY.md, round 6 third session).
// A scaled column sum (class 7) has ONE block per row range and a partial of at most 256 floats: with 2,048 rows per block the six
// 154,666 x 256 jobs of a step were 456 blocks on 256 CUs (two blocks = 32 KB of loads in flight per CU, 1.6 TB/s); 256 rows per block
// give eight times the blocks for 0.6 MB of partials per job.
constexpr int WGRAD_ROWS[8] = {0, 0, 1024, 1024, 512, 1024, 1024, 256};
constexpr WgradPlan wgrad_plan(int64_t M, int64_t N, int64_t K, int64_t splits, int dt, int64_t ldg, int64_t ldx, bool aligned) {
  int kind = 4;
  int64_t tn = 64, tk = 64;
  const bool tr = (dt & 3) == 3 && ldg % 8 == 0 && ldx % 8 == 0 && aligned;   // float16 on both sides, rows on 16 bytes
  if (tr && N % 64 == 0 && K % 64 == 0) {
    // 128-wide tiles where the layer allows (the 128 x 128 class runs at two waves per SIMD, 172 registers)
    tn = N % 128 == 0 ? 128 : 64;
    tk = K % 128 == 0 ? 128 : 64;
    kind = (tn == 128 ? 0 : 2) + (tk == 128 ? 0 : 1);
  } else if (tr && ((N == 32 && K == 64) || (N == 64 && K == 32))) {
    tn = N, tk = K;
    kind = N == 32 ? 5 : 6;
  } else if ((N == 1 && K % 4 == 0 && K <= 256) || (K == 1 && N % 4 == 0 && N <= 256)) {
    tn = N, tk = K;   // one block per row range
    kind = 7;
  }
  SplitLayout lay = split_layout(M, N, K, splits, HW_MC);
  if (WGRAD_ROWS[kind] > 0 && lay.mper > WGRAD_ROWS[kind]) lay = split_layout_rows(M, N, K, WGRAD_ROWS[kind]);
  const int64_t gx = ceil_div(K, tk), gy = ceil_div(N, tn);
  return {kind, gx, gy, lay, gx * gy * lay.S};
}

// ---- LayerNorm backward ---------------------------------------------------------------------------------------------------------------
// One workgroup of four waves per 4 * MDX_LN_RPW rows; each leaves one partial row [dgamma | dbeta] of 2F floats in the workspace, and
// more than RED_CHUNK of them need the chunk sums' planes behind them.
constexpr int64_t ln_bwd_rows(int64_t M) { return ceil_div(ceil_div(M, MDX_LN_RPW), 4); }
constexpr int64_t ln_bwd_ws_floats(int64_t M, int64_t F) {
  const int64_t nr = ln_bwd_rows(M);
  return (nr > 1 ? nr : 1) * 2 * F + (nr > RED_CHUNK ? ceil_div(nr, RED_CHUNK) * 2 * F : 0);
}

// ---- record table of the deferred reduction (reduce_deferred_kernel; built by mdx_fast.cpp) ------------------------------------------
// A record of S partials of `elems` outputs takes red_blocks(elems) blocks; a chunked record (S > RED_CHUNK) takes that for each of its
// ceil(S / RED_CHUNK) chunks and stores chunk c's sum in plane red_chunk_plane(S, c) of its partial area (planes are `pstride` floats
// apart): the planes a SplitLayout's stage_off and ln_bwd_ws_floats reserve.
constexpr int64_t red_blocks(int64_t elems) { return (int64_t)(((uint64_t)elems + RED_ELEMS - 1) / RED_ELEMS); }   // (unsigned: a shift on the device)
constexpr int64_t red_chunk_plane(int64_t S, int64_t c) { return S + c; }

// ---- row-owner GEMM (hgemm_nt_rows_kernel) ---------------------------------------------------------------------------------------------
// The shapes it is instantiated for and worth launching at: K in {32, 64, 128, 256}, N in {32, 64, 128, 256}, at least 1,024 rows.
constexpr bool rows_gemm_shape(int64_t M, int64_t N, int64_t K) {
  return M >= 1024 && (K == 32 || K == 64 || K == 128 || K == 256) && (N == 32 || N == 64 || N == 128 || N == 256);
}

// ---- fused row-owner operators (mdx_train_fused.hip) ---------------------------------------------------------------------------------
// A wave owns 16-row tiles and walks them with a stride of grid x waves.  A forward launches min(wg_per_cu x #CUs, ceil(tiles / waves))
// workgroups, at least one; a backward always #CUs (one partial row of LayerNorm-parameter gradients per workgroup, whether it had a
// tile or not).  rounds: trips of the tile loop of the grid's first wave; last_tiles: tiles of the last round (the other waves of that
// round are past the end); last_rows: rows of the last tile.
struct FusedGrid {
  int grid, waves, tiles, rounds, last_tiles, last_rows;
};
constexpr FusedGrid fused_grid(int64_t E, int n_cus, int wg_per_cu, int waves, bool backward) {
  const int64_t tiles = ceil_div(E > 0 ? E : 0, 16);
  const int64_t want = ceil_div(tiles, waves), cap = (int64_t)wg_per_cu * n_cus;
  const int64_t grid = backward ? n_cus : (want < cap ? (want > 1 ? want : 1) : cap);
  const int64_t nw = grid * waves, rounds = ceil_div(tiles, nw);
  return {(int)grid, waves, (int)tiles, (int)rounds, (int)(tiles ? tiles - (rounds - 1) * nw : 0), (int)(tiles ? E - 16 * (tiles - 1) : 0)};
}
