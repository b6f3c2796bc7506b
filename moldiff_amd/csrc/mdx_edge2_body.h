// Body of the row-owner edge kernel A and its launcher, shared by the exact fp32 build (mdx_edge2.hip) and the split float16
// build (mdx_edge2s.hip): the two differ only in the matrix products, so the including file defines
//     E2_KERNEL               the kernel's name
//     E2_S                    the stream-pack member of the weight block: s or ss
//     E2_GEMM(KT, FT)         the GEMM primitive over an operand of KT 16-wide tiles: rgemm<KT, FT, RR> (mdx_row.h) or
//                             rgemm_s<(KT + 1) / 2, FT> (mdx_split.h)
//     E2_X(KT, x)             declares x, the storage of such an operand: f32x4 x[KT][RR] or XS<(KT + 1) / 2> x
//     E2_OPERAND(KT, x, y)    declares x, the operand made of the fp32 accumulators y[KT][RR]: an alias of y (auto& x = y) or
//                             E2_X(KT, x); to_xs<KT>(x, y)
//     STAMP(i)                phase stamp i of the 48-slot trace record (slot 46/47: wall clock at entry/exit); ((void)0) in the library
// and includes this file inside its anonymous namespace.  mdx_edge2b_body.h (kernel B) takes the same macros, with STAMPB.
//
// Same math, same argument blocks (EdgeAArgs / EdgeBArgs) as mdx_edge.hip's tile kernels, different work decomposition (mdx_row.h):
//   edge kernel A  (reference models/graph.py:352-357 edge_embs, :42-47 NodeBlock message path,
//                   :133-141/:278,:282 the two EdgeBlock BondFFNs, :50 / :283 the by-left segment sums (EA_AGG))
//   edge kernel B  (models/graph.py:286-294 EdgeBlock tail, :384-393 PosUpdate)
// One WAVE owns 16*RR consecutive edges of the (left,right)-sorted edge list and computes every layer for them; its
// activations stay in registers from the He tile load to the M / F / He'' / Fe stores.  No LDS tile, no barrier.
// LDS is only a wave-private parking area for sigmoid(gate) while the message chain runs (16 KiB per wave at 16 rows).
// Everything that is not a matrix product (smearing, biases, LayerNorm, gates, segment sums, stores) is the same fp32 code in both
// builds; in the split build an operand that feeds several GEMMs (He') is converted once.

// FLAGS (EA_*) is a template parameter: with run-time section flags every section sits behind a branch and the values that
// cross it (He', the tile, the weight ring) get spilled around the control flow.
template <int FLAGS>
__global__ __launch_bounds__(MDX_WG, MDX_WPS) void E2_KERNEL(const EdgeAArgs a, const EdgePlan plan, const WorkQA wq) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q0 = lane >> 4;
  const int E = a.E;
  constexpr bool do_emb = FLAGS & EA_EMB, do_node = FLAGS & EA_NODE, do_ffn = FLAGS & EA_FFN, do_agg = FLAGS & EA_AGG;
  // The BondFFN tape stores (round 3) are compiled into the tape instantiation only.  Round 2's three stores (tSG, tHE, M / F[1]
  // with EA_AGG) stay behind their run-time pointer tests in every instantiation: compiling them out of the denoiser's kernel as
  // well measured 0.8 % SLOWER on the same box (6.94 vs 6.89 ms per step; the register allocation of a 256-VGPR kernel is that
  // sensitive -- 5 spilled registers instead of 4), so the form that measured best ships.
  constexpr bool do_tape = FLAGS & EA_TAPE;
  constexpr bool do_tape_ffn = FLAGS & EA_TAPE_FFN;  // unconditional stores: no pointer tests inside the BondFFN sections
  // the tape is read back by the backward a whole forward later: streaming (non-temporal) stores keep its 870 MB per launch from
  // displacing weights and node rows in L2 (guided step 26.00 -> 25.90 ms)
  constexpr bool TAPE_NT = do_tape;
  // centred packs (mdx_row.h row_layernorm_centred): never with the tape, whose pre-LayerNorm values the backward re-normalises
  const bool lnc = !do_tape && a.w.lnc;
#define TAPE_ST(p, v) do { if (TAPE_NT) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p)); else stg4(p, v); } while (0)
  // rows of item u: RR graph-aligned units of the plan's table, one per row tile (EA_AGG; load_tile_units, mdx_row.h), or 16 RR
  // consecutive rows of the batch
  int ucnt_next[RR];
  auto tile_of = [&](int u) {
    if constexpr (do_agg) return load_tile_units(a, u, c, ucnt_next);
    else return load_tile(a.l, a.r, a.te, u * ROWS, E, c);
  };
  f32x4* park = reinterpret_cast<f32x4*>(smem + (size_t)wave * PARK_FLOATS) + lane;
  const unsigned lane_off = 16u * lane;
  auto W = [&](const float* p) { return make_ws(p, lane_off); };
  const EdgeAS& S = a.w.E2_S;  // stream packs of this build

  // fixed LDS layout (offsets in floats) so every constant address is cbase + immediate
  float* cb = smem + 4 * PARK_FLOATS;
  const float* c_soff = lds_put<0, 16>(cb, a.soff, tid);
  const float* c_scoef = lds_put<16, 16>(cb, a.scoef, tid);
  const float* c_bemb = cb + 32;
  if (do_emb) lds_put<32, 64>(cb, a.w.bemb, tid);
  const float *c_bg1 = cb + 96, *c_wtg1 = c_bg1 + 256, *c_gg = c_bg1 + 512, *c_gb = c_bg1 + 768, *c_bg2 = c_bg1 + 1024,
              *c_eb1 = c_bg1 + 1280, *c_eg = c_bg1 + 1536, *c_ebe = c_bg1 + 1792, *c_eb2 = c_bg1 + 2048, *c_bm = c_bg1 + 2304;
  if (do_node) {
    lds_put<96, 256>(cb, a.w.bg1, tid); lds_put<96 + 256, 256>(cb, a.w.wtg1, tid); lds_put<96 + 512, 256>(cb, a.w.gg, tid);
    lds_put<96 + 768, 256>(cb, a.w.gb, tid); lds_put<96 + 1024, 256>(cb, a.w.bg2, tid); lds_put<96 + 1280, 256>(cb, a.w.en.b1, tid);
    lds_put<96 + 1536, 256>(cb, a.w.en.g, tid); lds_put<96 + 1792, 256>(cb, a.w.en.be, tid);
    lds_put<96 + 2048, 256>(cb, a.w.en.b2, tid); lds_put<96 + 2304, 256>(cb, a.w.bm, tid);
  }
  constexpr int FO = 96 + 2560, FS = 640;  // per BondFFN: bg1 32 | wtg1 32 | gg 32 | gb 32 | ib1 128 | ig 128 | ibe 128 | ib2 64 | bg2 64
  const float *f_bg1[2], *f_wtg1[2], *f_gg[2], *f_gb[2], *f_ib1[2], *f_ig[2], *f_ibe[2], *f_ib2[2], *f_bg2[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const float* fb = cb + FO + FS * s;
    f_bg1[s] = fb; f_wtg1[s] = fb + 32; f_gg[s] = fb + 64; f_gb[s] = fb + 96; f_ib1[s] = fb + 128; f_ig[s] = fb + 256;
    f_ibe[s] = fb + 384; f_ib2[s] = fb + 512; f_bg2[s] = fb + 576;
  }
  if (do_ffn) {
    const FfnW& w0 = a.w.ffn[0];
    const FfnW& w1 = a.w.ffn[1];
    lds_put<FO, 32>(cb, w0.bg1, tid); lds_put<FO + 32, 32>(cb, w0.wtg1, tid); lds_put<FO + 64, 32>(cb, w0.gg, tid);
    lds_put<FO + 96, 32>(cb, w0.gb, tid); lds_put<FO + 128, 128>(cb, w0.inter.b1, tid); lds_put<FO + 256, 128>(cb, w0.inter.g, tid);
    lds_put<FO + 384, 128>(cb, w0.inter.be, tid); lds_put<FO + 512, 64>(cb, w0.inter.b2, tid); lds_put<FO + 576, 64>(cb, w0.bg2, tid);
    lds_put<FO + FS, 32>(cb, w1.bg1, tid); lds_put<FO + FS + 32, 32>(cb, w1.wtg1, tid); lds_put<FO + FS + 64, 32>(cb, w1.gg, tid);
    lds_put<FO + FS + 96, 32>(cb, w1.gb, tid); lds_put<FO + FS + 128, 128>(cb, w1.inter.b1, tid);
    lds_put<FO + FS + 256, 128>(cb, w1.inter.g, tid); lds_put<FO + FS + 384, 128>(cb, w1.inter.be, tid);
    lds_put<FO + FS + 512, 64>(cb, w1.inter.b2, tid); lds_put<FO + FS + 576, 64>(cb, w1.bg2, tid);
  }
  __syncthreads();  // the only barrier of the kernel: constants visible to every wave

  // persistent wave; slots are XCD-contiguous so that neighbouring units (same molecule -> same node rows) share an L2
  // (static split; with a work queue the wave draws its items from its pair's counter instead)
  const bool dyn = wq.q.ctr != nullptr;
  const int slot = xcd_remap(blockIdx.x, gridDim.x) * 4 + wave;
  WorkPair wp{};
  int nitems, xcnt = 0, xnt = 0, mode, mode_next, unit;
  if (dyn) {
    wp = wq_pair(wq.q);
    xcnt = wp.end - wp.beg;
    xnt = wq_tail(xcnt, wp.waves, wq.tail8);
    const int i0 = wq_take(wq_request(wp.line, lane));
    nitems = i0 < xcnt + xnt ? 1 : 0;
    unit = wp.beg + wq_item(i0, xcnt, xnt, mode);
  } else {
    nitems = plan_items(plan, slot);
    unit = plan_item(plan, slot, 0, mode);
  }
  if (nitems <= 0) {
    if (dyn) wq_leave(wp, lane);
    return;
  }

  // first stream of a unit (the tail of every unit primes it again for the next one)
  const float* wfirst = do_emb ? S.Wemb : do_node ? S.Wg1e : S.ffn[0].Wbl;
  WRing ring;
  ring_prime(ring, W(wfirst));
  Prolog pr;
  pr.t = tile_of(unit);
  prolog_rows(pr, a, q0);

#pragma unroll 1
  for (int it = 0;; ++it) {
    int q = q0;
    asm volatile("" : "+v"(q));  // opaque per iteration: lane-dependent address parts stay next to their loads instead of
                                 // being hoisted out of the persistent loop into (spilled) registers
    const RowTile t = pr.t;
    int ucnt[RR];
#pragma unroll
    for (int rt = 0; rt < RR; ++rt) ucnt[rt] = do_agg ? __builtin_amdgcn_readfirstlane(ucnt_next[rt]) : 0;
    const int ureq = dyn ? wq_request(wp.line, lane) : 0;  // the next item, consumed where its tile is requested
    const bool inode = do_node && (mode & 1), iffn = do_ffn && (mode & 10);
    const int sfirst = (mode & 2) ? 0 : 1, slast = (mode & 8) ? 1 : 0;  // BondFFN sections of this item (wave-uniform)
    STAMP(46);
    STAMP(0);
    // ---- He' = edge_embs([He | smear(d)]) ; hx = He' as the operand of the six GEMMs it feeds -----------------
    f32x4 hep[4][RR];
    if (do_emb) {
      f32x4 x[5][RR];
      const f32x4 off = lds4(c_soff + 4 * q), coef = lds4(c_scoef + 4 * q);
#pragma unroll
      for (int rt = 0; rt < RR; ++rt) {
#pragma unroll
        for (int g = 0; g < 4; ++g) x[g][rt] = pr.x[g][rt];
        const float u0 = fminf(fmaxf(pr.d[rt], a.smear_start), a.cutoff);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float u = u0 - off[s];
          x[4][rt][s] = expf(coef[s] * (u * u));
        }
      }
      E2_OPERAND(5, xs, x);  // K = 80 (the split operand is zero-padded to 96)
      row_bias<4, RR>(hep, c_bemb, q);
      STAMP(1);
      E2_GEMM(5, 4)(hep, xs, W(S.Wemb), ring, W(inode ? S.Wg1e : iffn ? S.ffn[sfirst].Wbl : wfirst));
      STAMP(2);
      if (mode & 4) row_store<4, RR>(hep, a.He_out, t.row, t.valid, 64, q);
    } else {
#pragma unroll
      for (int rt = 0; rt < RR; ++rt)
#pragma unroll
        for (int g = 0; g < 4; ++g) hep[g][rt] = pr.x[g][rt];
    }
    E2_OPERAND(4, hx, hep);

    // ---- NodeBlock message path: M = msg_net(edge_net(He') * h[r]) * sigmoid(gate([He' | x[r] | t])) --------
    if (inode) {
      f32x4 y[16][RR], z[16][RR];
      {  // gate layer 1: accumulator starts at b + gx[r] + t*wt (the hoisted node part and the time column)
        row_gather<16, RR>(y, a.NT + MDX_NT_GX, t.ri, MDX_NTW, q);
        float tg[RR];
#pragma unroll
        for (int rt = 0; rt < RR; ++rt) tg[rt] = a.tn_r ? a.tn_r[t.row[rt]] : t.tt[rt];  // the NodeBlock gate sees node_time[col]
#pragma unroll
        for (int ft = 0; ft < 16; ++ft) {
          const f32x4 b = lds4(c_bg1 + 16 * ft + 4 * q), wt = lds4(c_wtg1 + 16 * ft + 4 * q);
#pragma unroll
          for (int rt = 0; rt < RR; ++rt) y[ft][rt] = (b + y[ft][rt]) + splat4(tg[rt]) * wt;
        }
      }
      STAMP(3);
      E2_GEMM(4, 16)(y, hx, W(S.Wg1e), ring, W(S.Wg2));
      STAMP(4);
      row_layernorm_sel<16, RR>(lnc, y, c_gg, c_gb, q);
      {
        E2_OPERAND(16, ys, y);
        row_bias<16, RR>(z, c_bg2, q);
        STAMP(5);
        E2_GEMM(16, 16)(z, ys, W(S.Wg2), ring, W(S.W1));
        STAMP(6);
      }
#pragma unroll
      for (int ft = 0; ft < 16; ++ft)
#pragma unroll
        for (int rt = 0; rt < RR; ++rt) {
          const f32x4 sg = fast_sigmoid4(z[ft][rt]);
          if (a.tSG && t.valid[rt]) TAPE_ST(a.tSG + (size_t)t.row[rt] * MDX_ND + 16 * ft + 4 * q, sg);
          park[(ft * RR + rt) * 64] = sg;
        }
      // edge_net
      row_bias<16, RR>(y, c_eb1, q);
      STAMP(7);
      E2_GEMM(4, 16)(y, hx, W(S.W1), ring, W(S.W2));
      STAMP(8);
      row_layernorm_sel<16, RR>(lnc, y, c_eg, c_ebe, q);
      {
        E2_OPERAND(16, ys, y);
        row_bias<16, RR>(z, c_eb2, q);
        STAMP(9);
        E2_GEMM(16, 16)(z, ys, W(S.W2), ring, W(S.Wm));
        STAMP(10);
      }
      if (a.tHE) row_store<16, RR, TAPE_NT>(z, a.tHE, t.row, t.valid, MDX_ND, q);
      row_gather<16, RR>(y, a.H, t.ri, MDX_ND, q);
      mul_inplace<16>(z, y);
      // msg_net, gated
      {
        E2_OPERAND(16, zs, z);
        row_bias<16, RR>(y, c_bm, q);
        STAMP(11);
        E2_GEMM(16, 16)(y, zs, W(S.Wm), ring, W(iffn ? S.ffn[sfirst].Wbl : wfirst));
        STAMP(12);
      }
#pragma unroll
      for (int ft = 0; ft < 16; ++ft)
#pragma unroll
        for (int rt = 0; rt < RR; ++rt) y[ft][rt] = y[ft][rt] * park[(ft * RR + rt) * 64];
      if constexpr (do_agg) {
        // aggr[v] = sum over v's edge run of M (models/graph.py:50), the part of it that lies in each row tile's unit: segmented
        // sum over the tile's rows, one partial row per left node stored by the last row of its segment
        if (a.M) row_store<16, RR, TAPE_NT>(y, a.M, t.row, t.valid, MDX_ND, q);  // the guidance tape keeps M itself
        static_for<0, RR>([&](auto rc) {
          constexpr int rt = decltype(rc)::value;
          seg_sum_store<16, RR, rt>(y, smem + (size_t)wave * PARK_FLOATS, lane, ucnt[rt], t.li[rt], t.pf[rt] + RR * unit + rt, a.P);
        });
      } else {
        row_store<16, RR>(y, a.M, t.row, t.valid, MDX_ND, q);
      }
      STAMP(13);
    }
    // next unit's tile: indices, He rows and edge lengths are requested here, ahead of the BondFFN sections, and arrive under
    // their GEMMs (requested inside a section they would sit behind that section's run-time condition: spills)
    int unext;
    bool more;
    if (dyn) {
      const int i = wq_take(ureq);
      more = i < xcnt + xnt;
      mode_next = mode;
      unext = more ? wp.beg + wq_item(i, xcnt, xnt, mode_next) : unit;  // last item: the look-ahead repeats this unit's rows
    } else {
      more = it + 1 < nitems;
      unext = plan_item(plan, slot, min(it + 1, nitems - 1), mode_next);
    }
    pr.t = tile_of(unext);
    prolog_rows(pr, a, q);

    // ---- EdgeBlock BondFFNs: F_s = inter_s((W_bl He') * nl_s[idx_s]) * sigmoid(gate_s([He' | x[idx_s] | t])) ----
    if (iffn) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (!(mode & (s ? 8 : 2))) continue;
        const FfnS& ws = S.ffn[s];
        int idx[RR];
#pragma unroll
        for (int rt = 0; rt < RR; ++rt) idx[rt] = s ? t.ri[rt] : t.li[rt];
        f32x4 bl[8][RR], nl[8][RR], g1[2][RR];
        row_gather<8, RR>(nl, a.NT + (s ? MDX_NT_NLR : MDX_NT_NLL), idx, MDX_NTW, q);
        row_gather<2, RR>(g1, a.NT + (s ? MDX_NT_GXR : MDX_NT_GXL), idx, MDX_NTW, q);
#pragma unroll
        for (int ft = 0; ft < 2; ++ft) {
          const f32x4 b = lds4(f_bg1[s] + 16 * ft + 4 * q), wt = lds4(f_wtg1[s] + 16 * ft + 4 * q);
#pragma unroll
          for (int rt = 0; rt < RR; ++rt) g1[ft][rt] = (b + g1[ft][rt]) + splat4(t.tt[rt]) * wt;
        }
        row_zero<8, RR>(bl);
        STAMP(14 + 10 * s);
        E2_GEMM(4, 8)(bl, hx, W(ws.Wbl), ring, W(ws.Wg1e));
        STAMP(15 + 10 * s);
        if constexpr (do_tape_ffn) row_store<8, RR, TAPE_NT>(bl, a.tBL[s], t.row, t.valid, 128, q);
        mul_inplace<8>(bl, nl);
        E2_GEMM(4, 2)(g1, hx, W(ws.Wg1e), ring, W(ws.W1));
        STAMP(16 + 10 * s);
        row_layernorm_sel<2, RR>(lnc, g1, f_gg[s], f_gb[s], q);
        f32x4 h[8][RR];
        {
          E2_OPERAND(8, bs, bl);
          row_bias<8, RR>(h, f_ib1[s], q);
          STAMP(17 + 10 * s);
          E2_GEMM(8, 8)(h, bs, W(ws.W1), ring, W(ws.W2));
          STAMP(18 + 10 * s);
        }
        if constexpr (do_tape_ffn) row_store<8, RR, TAPE_NT>(h, a.tH1[s], t.row, t.valid, 128, q);
        row_layernorm_sel<8, RR>(lnc, h, f_ig[s], f_ibe[s], q);
        f32x4 o[4][RR], g2[4][RR];
        {
          E2_OPERAND(8, hs, h);
          row_bias<4, RR>(o, f_ib2[s], q);
          STAMP(19 + 10 * s);
          E2_GEMM(8, 4)(o, hs, W(ws.W2), ring, W(ws.Wg2));
          STAMP(20 + 10 * s);
        }
        if constexpr (do_tape_ffn) row_store<4, RR, TAPE_NT>(o, a.tO[s], t.row, t.valid, 64, q);
        {
          E2_OPERAND(2, gs, g1);
          row_bias<4, RR>(g2, f_bg2[s], q);
          E2_GEMM(2, 4)(g2, gs, W(ws.Wg2), ring, W(s < slast ? S.ffn[1].Wbl : wfirst));
          STAMP(21 + 10 * s);
        }
#pragma unroll
        for (int ft = 0; ft < 4; ++ft)
#pragma unroll
          for (int rt = 0; rt < RR; ++rt) o[ft][rt] = o[ft][rt] * fast_sigmoid4(g2[ft][rt]);
        if constexpr (do_agg) {
          if (s == 1) {  // SR[v] = sum over v's edge run of bond_ffn_right (graph.py:283): same segments as M
            if (a.F[1]) row_store<4, RR>(o, a.F[1], t.row, t.valid, 64, q);
            static_for<0, RR>([&](auto rc) {
              constexpr int rt = decltype(rc)::value;
              seg_sum_store<4, RR, rt>(o, smem + (size_t)wave * PARK_FLOATS, lane, ucnt[rt], t.li[rt], t.pf[rt] + RR * unit + rt, a.PR);
            });
          } else {
            row_store<4, RR>(o, a.F[s], t.row, t.valid, 64, q);
          }
        } else {
          row_store<4, RR>(o, a.F[s], t.row, t.valid, 64, q);
        }
        STAMP(22 + 10 * s);
      }
    }
    STAMP(40);
    STAMP(47);
    if (!more) break;
    unit = unext;
    mode = mode_next;
  }
  if (dyn) wq_leave(wp, lane);
#undef TAPE_ST
}

template <int FLAGS>
void launch_a2(const EdgeAArgs& a, hipStream_t s) {
  static bool attr = false;
  constexpr int lds = (4 * PARK_FLOATS + EA_CONST_FLOATS) * 4;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)E2_KERNEL<FLAGS>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr = true;
  }
  const int nunits = (FLAGS & EA_AGG) ? (a.nunits + RR - 1) / RR : (a.E + ROWS - 1) / ROWS;  // work items (RR units each)
  if (nunits <= 0) return;
  const int grid = row_owner_grid(nunits, mdx_num_cus(), MDX_WPS);
  constexpr bool all = (FLAGS & ~(EA_AGG | EA_TAPE | EA_TAPE_FFN)) == (EA_EMB | EA_NODE | EA_FFN);
  const EdgePlan plan = make_plan(nunits, grid * 4, all);
  WorkQA wq{};
  wq.q = make_workq(a.wq, nunits, grid, mdx_num_cus());
  if (a.wq && all) wq.tail8 = EA_WQ_TAIL8;  // units cut by section at the end of each pair's list: 10 eighths of a unit per wave
  hipLaunchKernelGGL(E2_KERNEL<FLAGS>, dim3(grid), dim3(MDX_WG), lds, s, a, plan, wq);
}
