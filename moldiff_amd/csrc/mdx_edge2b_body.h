// Body of the row-owner edge kernel B and its launcher: EdgeBlock tail + PosUpdate (reference models/graph.py:286-294 and
// :384-393), shared by the exact fp32 build (mdx_edge2b.hip) and the split float16 build (mdx_edge2bs.hip).  The including file
// defines E2_KERNEL, E2_S, E2_GEMM, E2_X, E2_OPERAND and STAMPB as described in mdx_edge2_body.h (design notes there and in
// mdx_row.h), and
//     E2_PUT_PAIR(x, ftp, xb, xn)   puts the product of the tile pairs xb, xn into an E2_X(16, x) operand as its feature tiles
//                                   2 ftp, 2 ftp + 1: the two x[2 ftp + j] assignments, or to_xs<2> of the product into k-group ftp
// and includes this file inside its anonymous namespace.
constexpr int EB_CONST_FLOATS = 4 * 64 + 5 * 32 + 4 * 256;
constexpr int EB_PAIR_FLOATS = 2048;  // one feature-tile pair of a 64-input stream, fp32 and split packs alike

struct PrologB {
  RowTile t;
  f32x4 he[4][RR];
};

template <int FLAGS>
__global__ __launch_bounds__(MDX_WG, MDX_WPS) void E2_KERNEL(const EdgeBArgs a, const int nunits, const WorkQ wq) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q0 = lane >> 4;
  const int E = a.E;
  constexpr bool do_edge = FLAGS & EB_EDGE, do_pos = FLAGS & EB_POS;
  const unsigned lane_off = 16u * lane;
  auto W = [&](const float* p) { return make_ws(p, lane_off); };
  const EdgeBS& S = a.w.E2_S;  // stream packs of this build
  // centred packs of the PosUpdate gate and inter layers (mdx_row.h row_layernorm_centred).  The EdgeBlock tail's LayerNorm keeps
  // the two-pass form: its addends SL / SR are sums of gated products, which no weight pack can centre.
  const bool lnc = a.w.lnc;

  float* cb = smem;
  const float *c_bself = cb, *c_lng = cb + 64, *c_lnb = cb + 128, *c_bout = cb + 192;
  if (do_edge) {
    lds_put<0, 64>(cb, a.w.bself, tid); lds_put<64, 64>(cb, a.w.lng, tid); lds_put<128, 64>(cb, a.w.lnb, tid);
    lds_put<192, 64>(cb, a.w.bout, tid);
  }
  const float *c_bg1 = cb + 256, *c_wtg1 = cb + 288, *c_gg = cb + 320, *c_gb = cb + 352, *c_wg2 = cb + 384, *c_bi1 = cb + 416,
              *c_ig = cb + 672, *c_ib = cb + 928, *c_wi2 = cb + 1184;
  if (do_pos) {
    lds_put<256, 32>(cb, a.w.bg1, tid); lds_put<288, 32>(cb, a.w.wtg1, tid); lds_put<320, 32>(cb, a.w.gg, tid);
    lds_put<352, 32>(cb, a.w.gb, tid); lds_put<384, 32>(cb, a.w.wg2, tid); lds_put<416, 256>(cb, a.w.bi1, tid);
    lds_put<672, 256>(cb, a.w.ig, tid); lds_put<928, 256>(cb, a.w.ib, tid); lds_put<1184, 256>(cb, a.w.wi2, tid);
  }
  __syncthreads();

  // units of this wave: drawn from its pair's counter (mdx_row.h, WorkQ), or a contiguous range of the static split
  const bool dyn = wq.ctr != nullptr;
  WorkPair wp{};
  int ubeg, uend;
  if (dyn) {
    wp = wq_pair(wq);
    uend = wp.end;
    ubeg = wp.beg + wq_take(wq_request(wp.line, lane));
  } else {
    const int nslots = gridDim.x * 4;
    const int slot0 = xcd_remap(blockIdx.x, gridDim.x) * 4 + wave;
    static_range(nunits, nslots, slot0, ubeg, uend);
  }
  if (ubeg >= uend) {
    if (dyn) wq_leave(wp, lane);
    return;
  }

  const float* wfirst = do_edge ? S.Wself : S.Wbl;
  WRing ring;
  ring_prime(ring, W(wfirst));
  PrologB pr;
  pr.t = load_tile(a.l, a.r, a.te, ubeg * ROWS, E, c);
  row_gather<4, RR>(pr.he, a.Hep, pr.t.row, 64, q0);

#pragma unroll 1
  for (int unit = ubeg;;) {
    int q = q0;
    asm volatile("" : "+v"(q));  // see kernel A (mdx_edge2_body.h)
    const RowTile t = pr.t;
    const int ureq = dyn ? wq_request(wp.line, lane) : 0;  // consumed where the next tile is loaded
    STAMPB(46);
    STAMPB(0);
    f32x4 he[4][RR];  // He' on entry, He'' after the EdgeBlock tail
#pragma unroll
    for (int rt = 0; rt < RR; ++rt)
#pragma unroll
      for (int g = 0; g < 4; ++g) he[g][rt] = pr.he[g][rt];

    // PosUpdate inputs that only depend on the tile's indices: requested first, consumed after the EdgeBlock tail
    f32x4 aa[4][RR], bb[4][RR];
    float rx[RR], ry[RR], rz[RR], dd[RR];
    if (do_pos) {
      row_gather<4, RR>(aa, a.Lf, t.li, 64, q);
      row_gather<4, RR>(bb, a.Rf, t.ri, 64, q);
#pragma unroll
      for (int rt = 0; rt < RR; ++rt) {
        if (a.rel_in) {
          rx[rt] = a.rel_in[3 * (size_t)t.row[rt] + 0]; ry[rt] = a.rel_in[3 * (size_t)t.row[rt] + 1]; rz[rt] = a.rel_in[3 * (size_t)t.row[rt] + 2];
          dd[rt] = a.dist_in[t.row[rt]];
        } else {
          rx[rt] = a.pos[3 * t.li[rt] + 0] - a.pos[3 * t.ri[rt] + 0];
          ry[rt] = a.pos[3 * t.li[rt] + 1] - a.pos[3 * t.ri[rt] + 1];
          rz[rt] = a.pos[3 * t.li[rt] + 2] - a.pos[3 * t.ri[rt] + 2];
          dd[rt] = sqrtf(rx[rt] * rx[rt] + ry[rt] * ry[rt] + rz[rt] * rz[rt]);
        }
      }
    }

    // ---- EdgeBlock tail: He'' = He' + out_transform(relu(LN(SL[l] + SR[r] + nfl[l] + nfr[r] + self_ffn(He')))) ----
    if (do_edge) {
      f32x4 u[4][RR], v[4][RR], v2[4][RR], v3[4][RR];
      row_gather<4, RR>(u, a.SL, t.li, 64, q);
      row_gather<4, RR>(v, a.SR, t.ri, 64, q);
      row_gather<4, RR>(v2, a.NT + MDX_NT_NFL, t.li, MDX_NTW, q);
      row_gather<4, RR>(v3, a.NT + MDX_NT_NFR, t.ri, MDX_NTW, q);
#pragma unroll
      for (int ft = 0; ft < 4; ++ft) {
        const f32x4 bs = lds4(c_bself + 16 * ft + 4 * q);
#pragma unroll
        for (int rt = 0; rt < RR; ++rt) u[ft][rt] = (((u[ft][rt] + v[ft][rt]) + v2[ft][rt]) + v3[ft][rt]) + bs;
      }
      {
        E2_OPERAND(4, hx, he);
        STAMPB(1);
        E2_GEMM(4, 4)(u, hx, W(S.Wself), ring, W(S.Wout));
        STAMPB(2);
      }
      row_layernorm<4, RR>(u, c_lng, c_lnb, q);
      {
        E2_OPERAND(4, us, u);
        row_bias<4, RR>(v, c_bout, q);
        STAMPB(3);
        E2_GEMM(4, 4)(v, us, W(S.Wout), ring, W(do_pos ? S.Wbl : wfirst));
        STAMPB(4);
      }
#pragma unroll
      for (int ft = 0; ft < 4; ++ft)
#pragma unroll
        for (int rt = 0; rt < RR; ++rt) {
          if (!(FLAGS & EB_DELTA)) v[ft][rt] = v[ft][rt] + he[ft][rt];
          he[ft][rt] = v[ft][rt];
        }
      row_store<4, RR>(he, a.He_out, t.row, t.valid, 64, q);
    }
    int unext = dyn ? wp.beg + wq_take(ureq) : unit + 1;
    const bool more = unext < uend;
    if (!more) unext = unit;  // last unit of the wave: the look-ahead loads repeat this unit's rows
    pr.t = load_tile(a.l, a.r, a.te, unext * ROWS, E, c);  // next unit's indices travel under the PosUpdate GEMMs

    // ---- PosUpdate: w = inter((W_bl He'') * (W_nl a)) * sigmoid(gate([He'' | a | t])), a = Lf[l] * Rf[r]; Fe = w rel / d / (d+1) ----
    if (do_pos) {
      mul_inplace<4>(aa, bb);
      E2_OPERAND(4, hx, he);
      E2_OPERAND(4, ax, aa);
      // x = (W_bl He'') * (W_nl a), the operand of the inter layer, formed one pair of feature tiles at a time from the two streams
      // alternately, so the two (rows x 256) products are never both live.  (Written as one 64->256 GEMM followed by pairwise
      // 64->32 GEMMs the compiler sinks each pair's W_bl MFMAs down to their use -- same schedule, but with the weight ring loaded
      // in the old order and spilled; stated explicitly, the ring order is the execution order.)
      E2_X(16, x);
      STAMPB(5);
      static_for<0, 8>([&](auto fc) {
        constexpr int ftp = decltype(fc)::value;
        constexpr int PF = EB_PAIR_FLOATS;
        f32x4 xb[2][RR], xn[2][RR];
        row_zero<2, RR>(xb);
        E2_GEMM(4, 2)(xb, hx, W(S.Wbl + ftp * PF), ring, W(S.Wnl + ftp * PF));
        row_zero<2, RR>(xn);
        E2_GEMM(4, 2)(xn, ax, W(S.Wnl + ftp * PF), ring, W(ftp < 7 ? S.Wbl + (ftp + 1) * PF : S.Wg1h));
        E2_PUT_PAIR(x, ftp, xb, xn);
      });
      STAMPB(6);
      STAMPB(7);
      // gate: ((b + t wt) + W_h He'') + W_a a, LN(32), ReLU, 32 -> 1
      f32x4 h[16][RR], g1[2][RR];
#pragma unroll
      for (int ft = 0; ft < 2; ++ft) {
        const f32x4 b = lds4(c_bg1 + 16 * ft + 4 * q), wt = lds4(c_wtg1 + 16 * ft + 4 * q);
#pragma unroll
        for (int rt = 0; rt < RR; ++rt) g1[ft][rt] = b + splat4(t.tt[rt]) * wt;
      }
      E2_GEMM(4, 2)(g1, hx, W(S.Wg1h), ring, W(S.Wg1a));
      E2_GEMM(4, 2)(g1, ax, W(S.Wg1a), ring, W(S.Wi1));
      STAMPB(8);
      row_layernorm_sel<2, RR>(lnc, g1, c_gg, c_gb, q);
      float gate[RR], wd[RR];
      row_dot<2, RR>(g1, c_wg2, q, gate);
      row_bias<16, RR>(h, c_bi1, q);
      STAMPB(9);
      E2_GEMM(16, 16)(h, x, W(S.Wi1), ring, W(wfirst));
      STAMPB(10);
      row_gather<4, RR>(pr.he, a.Hep, pr.t.row, 64, q);  // next unit's He' rows: their latency hides under the LayerNorm below
      row_layernorm_sel<16, RR>(lnc, h, c_ig, c_ib, q);
      row_dot<16, RR>(h, c_wi2, q, wd);
      if (q == 0) {
#pragma unroll
        for (int rt = 0; rt < RR; ++rt) {
          if (!t.valid[rt]) continue;
          const float w = (wd[rt] + a.w.bi2) * sigmoidf_(gate[rt] + a.w.bg2);
          const float d = dd[rt], dp = d + 1.0f;
          float* fe = a.Fe + 3 * (size_t)t.row[rt];
          fe[0] = w * rx[rt] / d / dp;
          fe[1] = w * ry[rt] / d / dp;
          fe[2] = w * rz[rt] / d / dp;
        }
      }
    } else {
      row_gather<4, RR>(pr.he, a.Hep, pr.t.row, 64, q);
    }
    STAMPB(40);
    STAMPB(47);
    if (!more) break;
    unit = unext;
  }
  if (dyn) wq_leave(wp, lane);
}

template <int FLAGS>
void launch_b2(const EdgeBArgs& a, hipStream_t s) {
  const int nunits = (a.E + ROWS - 1) / ROWS;
  const int grid = row_owner_grid(nunits, mdx_num_cus(), MDX_WPS);
  hipLaunchKernelGGL(E2_KERNEL<FLAGS>, dim3(grid), dim3(MDX_WG), EB_CONST_FLOATS * 4, s, a, nunits,
                     make_workq(a.wq, nunits, grid, mdx_num_cus()));
}
