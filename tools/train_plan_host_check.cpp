// Stand-alone check of the training operators' host arithmetic (moldiff_amd/csrc/mdx_train_plan.h, the header mdx_train.hip and
// mdx_fast.cpp compile): the split-partial layout, the weight-gradient queue's plan, the LayerNorm backward's partial rows and
// workspace, the deferred reduction's record table, the row-owner GEMM's shapes and the grid of the fused row-owner operators
// (mdx_train_fused.hip).  No HIP, no GPU; tests/test_train_plan_host.py
// builds and runs it, and it can be built with a host sanitizer:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/train_plan_host_check.cpp -o /tmp/train_plan_host_check
//     /tmp/train_plan_host_check
//
// Everything is enumerated over a grid of sizes around the tile, chunk and stage boundaries: these are structural facts (the row ranges
// tile the rows, the regions of a partial area do not overlap and end at its reported size), not recorded numbers.
#include <cstdio>
#include <vector>

#include "../moldiff_amd/csrc/mdx_train_plan.h"

static int failures = 0;
#define EXPECT(c, ...)                                       \
  do {                                                       \
    if (!(c)) {                                              \
      if (++failures <= 20) {                                \
        std::printf("FAILED line %d: %s  [", __LINE__, #c);  \
        std::printf(__VA_ARGS__);                            \
        std::printf("]\n");                                  \
      }                                                      \
    }                                                        \
  } while (0)

static long layouts = 0, plans = 0, chunked = 0;

// the facts every consumer of a layout relies on, whatever chose `mper`
static void check_layout(const SplitLayout& L, int64_t M, int64_t N, int64_t K, int chunk) {
  ++layouts;
  const int64_t rows = M > 1 ? M : 1, NK = N * K;
  EXPECT(L.mper > 0 && L.mper % chunk == 0, "M %lld mper %lld chunk %d", (long long)M, (long long)L.mper, chunk);
  EXPECT(L.S >= 1 && (L.S - 1) * L.mper < rows && rows <= L.S * L.mper, "M %lld S %lld mper %lld", (long long)M, (long long)L.S, (long long)L.mper);
  EXPECT(L.nc >= 1 && (L.nc - 1) * RED_CHUNK < L.S && L.S <= L.nc * RED_CHUNK, "S %lld nc %lld", (long long)L.S, (long long)L.nc);
  // products | their first-stage planes | bias partials | their first-stage planes: back to back, ending at `total`
  const int64_t beg[4] = {0, L.stage_off, L.bias_off, L.bias_off + L.S * N};
  const int64_t len[4] = {L.S * NK, L.nc * NK, L.S * N, L.nc * N};
  for (int r = 0; r < 4; ++r) {
    const int64_t end = beg[r] + len[r];
    EXPECT(beg[r] >= 0 && end <= L.total, "region %d [%lld, %lld) total %lld", r, (long long)beg[r], (long long)end, (long long)L.total);
    EXPECT(end == (r < 3 ? beg[r + 1] : L.total), "region %d ends at %lld", r, (long long)end);
  }
  if (L.S > RED_CHUNK) {   // a chunked record's chunk planes sit where the layout reserved them (weight: pstride N*K; bias: pstride N)
    ++chunked;
    for (int64_t c = 0; c < L.nc; ++c) {
      EXPECT(red_chunk_plane(L.S, c) * NK == L.stage_off + c * NK, "S %lld c %lld", (long long)L.S, (long long)c);
      EXPECT(L.bias_off + red_chunk_plane(L.S, c) * N == beg[3] + c * N && beg[3] + (c + 1) * N <= L.total, "S %lld c %lld", (long long)L.S, (long long)c);
    }
  }
}

int main() {
  const int64_t Ms[] = {0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 6279, 154666, 600000 /* 293 ranges of 2,048 rows */};
  const int64_t NKs[] = {1, 4, 6, 16, 32, 54, 64, 128, 256};
  const int chunks[] = {W_MC, HW_MC};
  // tiles of the queue's classes (0 = the layer's own width: class 7)
  const int TN[8] = {128, 128, 64, 64, 64, 32, 64, 0}, TK[8] = {128, 64, 128, 64, 64, 64, 32, 0};
  bool seen_kind[8] = {}, seen_chunked_split = false;
  for (int64_t M : Ms)
    for (int64_t N : NKs)
      for (int64_t K : NKs) {
        const int64_t splits_of[] = {1, 2, 7, ceil_div(M, 2048)};
        for (int64_t splits : splits_of) {
          const int64_t sp = splits > 1 ? splits : 1;
          for (int chunk : chunks) {
            const SplitLayout L = split_layout(M, N, K, splits, chunk);
            check_layout(L, M, N, K, chunk);
            seen_chunked_split |= L.S > RED_CHUNK;
            // `splits` bounds S, so the exact area is never larger than the bound the extension used to allocate
            EXPECT(L.S <= sp, "M %lld splits %lld S %lld", (long long)M, (long long)splits, (long long)L.S);
            EXPECT(L.total <= (sp + ceil_div(sp, 256)) * (N * K + N), "M %lld N %lld K %lld splits %lld", (long long)M, (long long)N, (long long)K, (long long)splits);
            EXPECT(L.mper == ceil_div(ceil_div(M > 1 ? M : 1, sp), chunk) * chunk, "mper %lld", (long long)L.mper);
          }
          for (int dt = 0; dt < 4; ++dt)
            for (int aligned = 0; aligned < 2; ++aligned) {
              const WgradPlan p = wgrad_plan(M, N, K, splits, dt, N, K, aligned != 0);
              ++plans;
              EXPECT(p.kind >= 0 && p.kind < 8, "kind %d", p.kind);
              if (p.kind < 0 || p.kind > 7) continue;
              seen_kind[p.kind] = true;
              check_layout(p.lay, M, N, K, HW_MC);
              const int64_t tn = TN[p.kind] ? TN[p.kind] : N, tk = TK[p.kind] ? TK[p.kind] : K;
              EXPECT(p.gx == ceil_div(K, tk) && p.gy == ceil_div(N, tn), "kind %d N %lld K %lld gx %lld gy %lld", p.kind, (long long)N, (long long)K, (long long)p.gx, (long long)p.gy);
              EXPECT(p.blocks == p.gx * p.gy * p.lay.S, "blocks %lld", (long long)p.blocks);
              // the transpose-read classes read whole tiles of float16 rows on 16 bytes
              if (p.kind != 4 && p.kind != 7) EXPECT(dt == 3 && aligned && N % tn == 0 && K % tk == 0, "kind %d dt %d N %lld K %lld", p.kind, dt, (long long)N, (long long)K);
              if (p.kind == 7) EXPECT((N == 1 && K % 4 == 0) || (K == 1 && N % 4 == 0), "kind 7 N %lld K %lld", (long long)N, (long long)K);
              // rows per block: the caller's, cut to the class's where it has one
              const int64_t want = split_layout(M, N, K, splits, HW_MC).mper, cap = WGRAD_ROWS[p.kind];
              EXPECT(p.lay.mper == (cap > 0 && want > cap ? cap : want), "kind %d mper %lld want %lld", p.kind, (long long)p.lay.mper, (long long)want);
            }
        }
        // the row-owner GEMM's shapes, written the way its launcher dispatches: K / 32 in {1, 2, 4, 8}, N / 16 in {2, 4, 8, 16}
        const int64_t kt = K / 32, ft = N / 16;
        const bool ok = M >= 1024 && K % 32 == 0 && N % 16 == 0 && (kt == 1 || kt == 2 || kt == 4 || kt == 8) && (ft == 2 || ft == 4 || ft == 8 || ft == 16);
        EXPECT(rows_gemm_shape(M, N, K) == ok, "M %lld N %lld K %lld", (long long)M, (long long)N, (long long)K);
      }
  for (int k = 0; k < 8; ++k) EXPECT(seen_kind[k], "tile class %d never chosen", k);
  EXPECT(seen_chunked_split && chunked > 0, "no layout with S > RED_CHUNK");

  // LayerNorm backward: one partial row per workgroup of 4 * MDX_LN_RPW rows; the workspace holds them and, beyond RED_CHUNK rows, the
  // chunk planes of a chunked record (pstride 2F)
  for (int64_t M : Ms)
    for (int64_t F : {1, 32, 54, 64, 128, 256, 1024}) {
      const int64_t nr = ln_bwd_rows(M), per = 4 * MDX_LN_RPW, ws = ln_bwd_ws_floats(M, F);
      EXPECT(nr * per >= M && (M <= 0 || (nr - 1) * per < M), "M %lld rows %lld", (long long)M, (long long)nr);
      EXPECT(ws >= (nr > 1 ? nr : 1) * 2 * F, "M %lld F %lld ws %lld", (long long)M, (long long)F, (long long)ws);
      if (nr > RED_CHUNK)
        for (int64_t c = 0; c < ceil_div(nr, RED_CHUNK); ++c)
          EXPECT(red_chunk_plane(nr, c) * 2 * F >= nr * 2 * F && (red_chunk_plane(nr, c) + 1) * 2 * F <= ws, "M %lld F %lld c %lld", (long long)M, (long long)F, (long long)c);
    }
  EXPECT(ln_bwd_rows(154666) > RED_CHUNK, "the edge rows do not reach the chunked case");

  // record table: blocks of RED_ELEMS outputs
  for (int64_t e : {1, 127, 128, 129, 256 * 256, 256 * 256 + 1, 2 * 1024})
    EXPECT(red_blocks(e) * RED_ELEMS >= e && (red_blocks(e) - 1) * RED_ELEMS < e, "elems %lld", (long long)e);

  // fused row-owner operators: the rounds of the grid's waves tile the tiles (all rounds but the last are full, the last is not empty),
  // a forward launches no workgroup without a tile in the first round and never more than wg_per_cu per CU, a backward one per CU
  for (int64_t E : {0, 1, 15, 16, 17, 62, 64, 414, 512, 1744, 1788, 32768, 32769, 154666, (1 << 23) - 1})
    for (int n_cus : {1, 2, 3, 5, 64, 256, 304})
      for (int per_cu : {1, 2})
        for (int waves : {4, 8, 12})
          for (int bwd = 0; bwd < 2; ++bwd) {
            const FusedGrid g = fused_grid(E, n_cus, per_cu, waves, bwd != 0);
            const int64_t tiles = ceil_div(E, 16), nw = (int64_t)g.grid * g.waves;
            EXPECT(g.waves == waves && g.tiles == tiles && g.grid >= 1, "E %lld grid %d", (long long)E, g.grid);
            EXPECT(bwd ? g.grid == n_cus : g.grid <= per_cu * n_cus && (int64_t)(g.grid - 1) * waves < (tiles > 1 ? tiles : 1), "E %lld cus %d grid %d",
                   (long long)E, n_cus, g.grid);
            EXPECT(!bwd && tiles > (int64_t)(g.grid) * waves ? g.grid == per_cu * n_cus : true, "E %lld cus %d grid %d", (long long)E, n_cus, g.grid);
            if (tiles == 0) {
              EXPECT(g.rounds == 0 && g.last_tiles == 0 && g.last_rows == 0, "empty");
            } else {
              EXPECT(g.last_tiles >= 1 && g.last_tiles <= nw && (g.rounds - 1) * nw + g.last_tiles == tiles, "E %lld rounds %d last %d", (long long)E,
                     g.rounds, g.last_tiles);
              EXPECT(g.last_rows >= 1 && g.last_rows <= 16 && 16 * (tiles - 1) + g.last_rows == E, "E %lld last rows %d", (long long)E, g.last_rows);
            }
          }

  if (failures) {
    std::printf("train_plan_host_check: %d failures\n", failures);
    return 1;
  }
  std::printf("train_plan_host_check ok: %ld layouts (%ld chunked), %ld plans\n", layouts, chunked, plans);
  return 0;
}
