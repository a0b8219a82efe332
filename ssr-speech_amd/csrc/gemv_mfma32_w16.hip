// gemv_mfma32_w16.hip — the two-panel matrix-core GEMV of gemv_mfma32.hip (17..32 rows) over PACKED bf16 WEIGHTS: the bf16 weight stream
// of the 17..32-row decode step (DESIGN.md Part I.12).
//
//   y[b][n] = epi( sum_k pro(x)[b][k] * float(Wt16[n][k]) + bias[n] ),   16 < B <= 32
//
// Only the bytes that are streamed change. The layout is the 5..16-row stream's (include/ssrhip.h SSRHIP_WT16_INDEX, the arena's
// ensure_wt16_copies): no second packer and no second copy. bf16 -> fp32 is a 16-bit shift (`d << 16` / `d & 0xffff0000`) and exact;
// activations, accumulation, bias and the KV cache stay fp32; and every kernel below issues EXACTLY the MFMA sequence of its gemv_rows32_*
// counterpart for the same k-steps: kstep2 / kpair2 per panel on one widened weight fragment, ln_slice / ln_apply per panel with ONE barrier
// for both, the part[panel][tile][wave][lane] sums in wave order (pair form: merge_pair2), pair_fold, panel_args with the
// gemv_mfma_tile.h epilogue per panel, and the launchers' common qualifier gemv_wt_qualify — on
// the same launch plan (gemv_rows_plan with ln_keeps_x = false). So a launch here equals ssrhip_gemv at the same row count on the fp32
// streaming-order copy of the rounded master bit for bit (tests/test_gpu_wt32.py compares with torch.equal).
//
// How a lane reads the layout is gemv_mfma_w16.hip's: plain form, loads h = 0 and h = 1 of a quad carry k-steps 4q (load 0, low half),
// 4q + 1 (load 1, low), 4q + 2 (load 0, high), 4q + 3 (load 1, high) — 16 MFMAs per load against two panels; pair form, one load carries
// the fp32 kernel's k-step pairs (4q, 4q + 1) and (4q + 2, 4q + 3) — 32 MFMAs per load. A quad past the end of K is clamped to the last
// quad with its x zeroed.
//
// Loads in flight per wave, x in registers, plain forms: WT32_DL = 8 (8 KiB). With both x panels resident the fp32 kernels are 8 k-steps
// ahead (DEP32); 8 packed loads are 16 k-steps — a wave's whole tile at K <= 2048, the 16-row kernels' look-ahead — in the same 32
// registers. The ring of 4 (the fp32 32-row kernels' 8 k-steps with half the bytes) would be a second set of kernels and is left out. The
// pair forms request a wave's whole slice (a group when streaming) at entry, as in fp32. The plain STREAMING form keeps the fp32 kernel's
// groups of 8 k-steps, i.e. 4 loads: its instruction counts are held against gemv_rows32_stream<false> (tests/test_wt32_isa.py), and no
// launch of the decode step takes it. Kept from gemv_mfma.hip's round 5: kv_pos of both panels are the wave's oldest loads, the
// epilogue operands are requested before the weight loop, no weight load sits under a run-time branch, the last tile is a separate code
// path, the pipeline does not drain between tiles. The recorded negatives (SSRHIP_GEMVM_EDGE, _WFIRST, _DEP8, SSRHIP_GEMVM_W16_DEPTH) have
// no form here. No bf16 MFMA and no v_dot2: either would round x.
#include <stdlib.h>
#include "common.h"
#include "gemv_mfma_tile.h"

namespace {

constexpr int WT32_DL = 8;      // weight loads in flight per wave in the plain forms

// K <= 2048 (SPWX = 16 k-steps per wave): gemv_rows32_xreg over bf16 — both x panels of the wave's K slice in VGPRs for all tiles.
template <int PRO, bool PAIR>
__global__ __launch_bounds__(512) void wt32_xreg_kernel(const GemvWt16 pw) {
  constexpr int SPWX = 16, LPT = SPWX / 2, DL = WT32_DL;      // plain form: LPT weight loads per tile and wave
  static_assert(LPT % DL == 0, "the ring must divide a tile's loads");
  __shared__ float red[2][2][8][16];
  __shared__ f4v part[2][MAXT][8][64];
  const GemvR& p = pw.r;
  const ssrhip_gemv_args& a = p.a;
  const ssrhip_gemv_args a0p = panel_args(a, 0), a1p = panel_args(a, 1);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, ks = lane >> 4;
  const int grp = blockIdx.y;
  const int K = a.K;
  const int u_lo = (int)((long long)blockIdx.x * p.units / p.wgs), u_hi = (int)((long long)(blockIdx.x + 1) * p.units / p.wgs);
  const int nun = u_hi - u_lo;
  if (nun <= 0) return;                                                 // uniform; only when wgs > units
  const int ntile = (nun + 1) >> 1;
  const int row_lo = u_lo * 8;
  const int last = p.steps - 1;
  const int tbase = wave * SPWX;
  const int lastq = (K >> 6) - 1, qbase = tbase >> 2;
  const uint16_t* wbase = pw.w16 + (size_t)grp * ((size_t)p.units * 8) * K;
  const float* xb0 = panel_xptr(a, grp, 0, c, ks);
  const float* xb1 = panel_xptr(a, grp, 1, c, ks);
  const int xstep = a.x_tiled ? 256 : 16;

  wt16_v4u w[PAIR ? SPWX / 4 : DL];                                     // pair form: SPWX / 4 loads, all requested at entry
  float4 x0[SPWX], x1[SPWX];
  const int kvpos0 = tile_kvpos(a0p, lane), kvpos1 = tile_kvpos(a1p, lane);   // the wave's oldest loads (QKV launch only)
  __builtin_amdgcn_sched_barrier(0);
  const uint16_t* wp = wt16_ptr(wbase, row_lo, nun, 0, c, ks, K) + (PAIR ? (c >> 3) * 256 : 0);
#pragma unroll
  for (int t = 0; t < SPWX; ++t) x0[t] = ld4(xb0 + min(tbase + t, last) * xstep);
#pragma unroll
  for (int t = 0; t < SPWX; ++t) x1[t] = ld4(xb1 + min(tbase + t, last) * xstep);
  __builtin_amdgcn_sched_barrier(0);
  if (PAIR) {
#pragma unroll
    for (int i = 0; i < SPWX / 4; ++i) w[i] = ldw_nt(wp + min(qbase + i, lastq) * 512);     // one quad (two k-step pairs) per load
  } else {
#pragma unroll
    for (int i = 0; i < DL; ++i) w[i] = ldw_nt(wp + wt16_off(qbase, i, lastq));
  }
  __builtin_amdgcn_sched_barrier(0);
  const bool epi_mine = wave < ntile;
  const int mine_rows = epi_mine ? tile_rows_of(wave, nun) : 0;
  const TileEpi e0 = tile_epilogue_fetch(a0p, p.hd, grp, row_lo + wave * 16, mine_rows, lane, kvpos0);
  const TileEpi e1 = tile_epilogue_fetch(a1p, p.hd, grp, row_lo + wave * 16, mine_rows, lane, kvpos1);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < SPWX; ++t) {
    asm volatile("" : "+v"(x0[t].x), "+v"(x0[t].y), "+v"(x0[t].z), "+v"(x0[t].w));
    asm volatile("" : "+v"(x1[t].x), "+v"(x1[t].y), "+v"(x1[t].z), "+v"(x1[t].w));
  }
#pragma unroll
  for (int t = 0; t < SPWX; ++t)
    if (tbase + t > last) { x0[t] = make_float4(0.f, 0.f, 0.f, 0.f); x1[t] = x0[t]; }

  if (PRO == SSRHIP_PRO_LAYERNORM) {
    // per panel: the 16-row kernel's LayerNorm (per-wave two-pass, slices merged by the pairwise-update identity), ONE barrier for both
    float m0, q0, m1, q1;
    ln_slice<SPWX>(x0, tbase, last, &m0, &q0);
    ln_slice<SPWX>(x1, tbase, last, &m1, &q1);
    if (ks == 0) { red[0][0][wave][c] = m0; red[0][1][wave][c] = q0; red[1][0][wave][c] = m1; red[1][1][wave][c] = q1; }
    __syncthreads();
    ln_apply<SPWX>(x0, red[0], p.nw, c, tbase, last, K, a.ln_eps);
    ln_apply<SPWX>(x1, red[1], p.nw, c, tbase, last, K, a.ln_eps);
  }

  if (PAIR) {
    f4v aA0 = {0.f, 0.f, 0.f, 0.f}, aB0 = aA0, aA1 = aA0, aB1 = aA0;
#pragma unroll
    for (int i = 0; i < SPWX / 4; ++i) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {                                       // the fp32 kernel's pair 2i + g = k-steps (4i + 2g, 4i + 2g + 1)
        const int t = 4 * i + 2 * g;
        kpair2(wt16_widen(w[i], g), x0[t], x0[t + 1], x1[t], x1[t + 1], aA0, aB0, aA1, aB1);
      }
    }
    part[0][0][wave][lane] = pair_fold(aA0, aB0);
    part[1][0][wave][lane] = pair_fold(aA1, aB1);
    __syncthreads();
    merge_pair2(a0p, a1p, part[0][0], part[1][0], p.nw, p.hd, e0, e1, wave, lane);
    return;
  }
  // k-step t of a tile reads load m = 2 (t / 4) + t % 2, half g = (t / 2) % 2. A load is used up after its high half (g = 1) and its
  // registers are refilled at once. All tiles but the last: the refills past this tile's loads fetch the head of the next tile
  for (int tile = 0; tile < ntile - 1; ++tile) {
    const uint16_t* wn = wt16_ptr(wbase, row_lo, nun, tile + 1, c, ks, K);
    f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, b0 = a0, b1 = a0;
#pragma unroll
    for (int t = 0; t < SPWX; ++t) {
      const int m = 2 * (t >> 2) + (t & 1), g = (t >> 1) & 1;
      kstep2(wt16_widen(w[m % DL], g), x0[t], x1[t], a0, a1, b0, b1);
      if (g == 1) {
        if (m + DL < LPT) w[m % DL] = ldw_nt(wp + wt16_off(qbase, m + DL, lastq));
        else w[m % DL] = ldw_nt(wn + wt16_off(qbase, m + DL - LPT, lastq));
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    part[0][tile][wave][lane] = a0 + a1;
    part[1][tile][wave][lane] = b0 + b1;
    wp = wn;
  }
  {
    f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, b0 = a0, b1 = a0;
#pragma unroll
    for (int t = 0; t < SPWX; ++t) {
      const int m = 2 * (t >> 2) + (t & 1), g = (t >> 1) & 1;
      kstep2(wt16_widen(w[m % DL], g), x0[t], x1[t], a0, a1, b0, b1);
      if (g == 1 && m + DL < LPT) w[m % DL] = ldw_nt(wp + wt16_off(qbase, m + DL, lastq));
      __builtin_amdgcn_sched_barrier(0);
    }
    part[0][ntile - 1][wave][lane] = a0 + a1;
    part[1][ntile - 1][wave][lane] = b0 + b1;
  }
  __syncthreads();
  for (int tile = wave; tile < ntile; tile += p.nw) {
    f4v s0 = part[0][tile][0][lane], s1 = part[1][tile][0][lane];
    for (int v = 1; v < p.nw; ++v) { s0 += part[0][tile][v][lane]; s1 += part[1][tile][v][lane]; }
    if (tile == wave) {
      tile_epilogue_finish(a0p, e0, s0, p.hd);
      tile_epilogue_finish(a1p, e1, s1, p.hd);
    } else {
      const int rows = (2 * tile + 1 < nun) ? 16 : 8;
      tile_epilogue(a0p, p.hd, grp, row_lo + tile * 16, rows, lane, s0);
      tile_epilogue(a1p, p.hd, grp, row_lo + tile * 16, rows, lane, s1);
    }
  }
}

// K > 2048 without a LayerNorm prologue (FFN2, K = 8192): gemv_rows32_stream over bf16 — both x panels are streamed beside W (L2 hits) in
// the fp32 kernel's groups: 16 k-steps in the pair form (2 x 16 x loads and 4 weight loads per group), 8 in the plain form (2 x 8 x loads
// and 4 weight loads: the fp32 kernel's look-ahead with half the bytes), all refilled while the group is consumed.
template <bool PAIR>
__global__ __launch_bounds__(512) void wt32_stream_kernel(const GemvWt16 pw) {
  constexpr int DEP = PAIR ? 16 : 8;              // k-steps per group, as in gemv_rows32_stream (a group is whole quads)
  __shared__ f4v part[2][MAXT][8][64];
  const GemvR& p = pw.r;
  const ssrhip_gemv_args& a = p.a;
  const ssrhip_gemv_args a0p = panel_args(a, 0), a1p = panel_args(a, 1);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, ks = lane >> 4;
  const int grp = blockIdx.y;
  const int K = a.K;
  const int u_lo = (int)((long long)blockIdx.x * p.units / p.wgs), u_hi = (int)((long long)(blockIdx.x + 1) * p.units / p.wgs);
  const int nun = u_hi - u_lo;
  if (nun <= 0) return;
  const int ntile = (nun + 1) >> 1;
  const int row_lo = u_lo * 8;
  const int last = p.steps - 1;
  const int tbase = wave * p.spw;                 // host: spw is a multiple of 16 k-steps
  const int ngrp = p.spw / DEP;
  const int lastq = (K >> 6) - 1, qbase = tbase >> 2;
  const uint16_t* wbase = pw.w16 + (size_t)grp * ((size_t)p.units * 8) * K;
  const float* xp0 = panel_xptr(a, grp, 0, c, ks);
  const float* xp1 = panel_xptr(a, grp, 1, c, ks);
  const int xstep = a.x_tiled ? 256 : 16;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

  float4 x0[DEP], x1[DEP];
  const int kvpos0 = tile_kvpos(a0p, lane), kvpos1 = tile_kvpos(a1p, lane);
  __builtin_amdgcn_sched_barrier(0);
  const uint16_t* wp = wt16_ptr(wbase, row_lo, nun, 0, c, ks, K) + (PAIR ? (c >> 3) * 256 : 0);
#pragma unroll
  for (int i = 0; i < DEP; ++i) { x0[i] = ld4(xp0 + min(tbase + i, last) * xstep); x1[i] = ld4(xp1 + min(tbase + i, last) * xstep); }
  __builtin_amdgcn_sched_barrier(0);
  if (PAIR) {
    // one 8-row unit per workgroup: per group of 16 k-steps 4 weight loads (a quad = two k-step pairs each) + 2 x 16 x loads
    wt16_v4u wq[DEP / 4];
#pragma unroll
    for (int i = 0; i < DEP / 4; ++i) wq[i] = ldw_nt(wp + min(qbase + i, lastq) * 512);
    __builtin_amdgcn_sched_barrier(0);
    const TileEpi e0 = tile_epilogue_fetch(a0p, p.hd, grp, row_lo, wave == 0 ? 8 : 0, lane, kvpos0);
    const TileEpi e1 = tile_epilogue_fetch(a1p, p.hd, grp, row_lo, wave == 0 ? 8 : 0, lane, kvpos1);
    __builtin_amdgcn_sched_barrier(0);
    f4v aA0 = {0.f, 0.f, 0.f, 0.f}, aB0 = aA0, aA1 = aA0, aB1 = aA0;
    for (int g = 0; g < ngrp - 1; ++g) {                                   // all groups but the last: refill for group g + 1
      const int kb = tbase + g * DEP, kbn = kb + DEP, qn = kbn >> 2;
#pragma unroll
      for (int j = 0; j < DEP / 2; ++j) {                                  // the fp32 kernel's pair j = k-steps (2j, 2j + 1) of the group
        const bool out = kb + 2 * j > last;                                // steps is even: a pair is in or out as a whole
        kpair2(wt16_widen(wq[j >> 1], j & 1), out ? z4 : x0[2 * j], out ? z4 : x0[2 * j + 1], out ? z4 : x1[2 * j], out ? z4 : x1[2 * j + 1],
               aA0, aB0, aA1, aB1);
        x0[2 * j] = ld4(xp0 + min(kbn + 2 * j, last) * xstep);
        x0[2 * j + 1] = ld4(xp0 + min(kbn + 2 * j + 1, last) * xstep);
        x1[2 * j] = ld4(xp1 + min(kbn + 2 * j, last) * xstep);
        x1[2 * j + 1] = ld4(xp1 + min(kbn + 2 * j + 1, last) * xstep);
        if (j & 1) wq[j >> 1] = ldw_nt(wp + min(qn + (j >> 1), lastq) * 512);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    {
      const int kb = tbase + (ngrp - 1) * DEP;
#pragma unroll
      for (int j = 0; j < DEP / 2; ++j) {
        const bool out = kb + 2 * j > last;
        kpair2(wt16_widen(wq[j >> 1], j & 1), out ? z4 : x0[2 * j], out ? z4 : x0[2 * j + 1], out ? z4 : x1[2 * j], out ? z4 : x1[2 * j + 1],
               aA0, aB0, aA1, aB1);
      }
    }
    part[0][0][wave][lane] = pair_fold(aA0, aB0);
    part[1][0][wave][lane] = pair_fold(aA1, aB1);
    __syncthreads();
    merge_pair2(a0p, a1p, part[0][0], part[1][0], p.nw, p.hd, e0, e1, wave, lane);
    return;
  }
  constexpr int NL = DEP / 2;                     // weight loads per group
  wt16_v4u w[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) w[i] = ldw_nt(wp + wt16_off(qbase, i, lastq));
  __builtin_amdgcn_sched_barrier(0);
  const bool epi_mine = wave < ntile;
  const int mine_rows = epi_mine ? tile_rows_of(wave, nun) : 0;
  const TileEpi e0 = tile_epilogue_fetch(a0p, p.hd, grp, row_lo + wave * 16, mine_rows, lane, kvpos0);
  const TileEpi e1 = tile_epilogue_fetch(a1p, p.hd, grp, row_lo + wave * 16, mine_rows, lane, kvpos1);
  __builtin_amdgcn_sched_barrier(0);
  const int total = ntile * ngrp;
  f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, b0 = a0, b1 = a0;
  int tile = 0, kg = 0;
  for (int g = 0; g < total - 1; ++g) {
    // group g = (tile, kg); the refills fetch group g + 1
    int tile_n = tile, kg_n = kg + 1;
    if (kg_n == ngrp) { kg_n = 0; tile_n = tile + 1; }
    const uint16_t* wn = (tile_n == tile) ? wp : wt16_ptr(wbase, row_lo, nun, tile_n, c, ks, K);
    const int kb = tbase + kg * DEP, kbn = tbase + kg_n * DEP, qn = kbn >> 2;
#pragma unroll
    for (int t = 0; t < DEP; ++t) {
      const int m = 2 * (t >> 2) + (t & 1), h = (t >> 1) & 1;
      const bool out = kb + t > last;                                      // uniform: k-steps past the end of K contribute nothing
      kstep2(wt16_widen(w[m], h), out ? z4 : x0[t], out ? z4 : x1[t], a0, a1, b0, b1);
      const int kk = min(kbn + t, last);
      x0[t] = ld4(xp0 + kk * xstep);
      x1[t] = ld4(xp1 + kk * xstep);
      if (h == 1) w[m] = ldw_nt(wn + wt16_off(qn, m, lastq));
      __builtin_amdgcn_sched_barrier(0);
    }
    if (kg_n == 0) {                                                      // uniform: tile finished
      part[0][tile][wave][lane] = a0 + a1;
      part[1][tile][wave][lane] = b0 + b1;
      a0 = (f4v){0.f, 0.f, 0.f, 0.f}; a1 = a0; b0 = a0; b1 = a0;
    }
    tile = tile_n; kg = kg_n; wp = wn;
  }
  {
    const int kb = tbase + kg * DEP;
#pragma unroll
    for (int t = 0; t < DEP; ++t) {
      const int m = 2 * (t >> 2) + (t & 1), h = (t >> 1) & 1;
      const bool out = kb + t > last;
      kstep2(wt16_widen(w[m], h), out ? z4 : x0[t], out ? z4 : x1[t], a0, a1, b0, b1);
    }
    part[0][ntile - 1][wave][lane] = a0 + a1;
    part[1][ntile - 1][wave][lane] = b0 + b1;
  }
  __syncthreads();
  for (int tile = wave; tile < ntile; tile += p.nw) {
    f4v s0 = part[0][tile][0][lane], s1 = part[1][tile][0][lane];
    for (int v = 1; v < p.nw; ++v) { s0 += part[0][tile][v][lane]; s1 += part[1][tile][v][lane]; }
    if (tile == wave) {
      tile_epilogue_finish(a0p, e0, s0, p.hd);
      tile_epilogue_finish(a1p, e1, s1, p.hd);
    } else {
      const int rows = (2 * tile + 1 < nun) ? 16 : 8;
      tile_epilogue(a0p, p.hd, grp, row_lo + tile * 16, rows, lane, s0);
      tile_epilogue(a1p, p.hd, grp, row_lo + tile * 16, rows, lane, s1);
    }
  }
}

// the packed kernels' contract: the check and the plan of ssrhip_gemv_mfma32_launch
int wt32_qualify(const ssrhip_gemv_args* a, RowsPlan* pl) {
  return gemv_wt_qualify(a, "ssrhip_gemv_wt32", 17, 32, 2048, /*ln_keeps_x=*/false, /*v1_refuses=*/false, pl);
}

}  // namespace

extern "C" int ssrhip_gemv_wt32_applicable(const ssrhip_gemv_args* a) {
  if (!a) return 0;
  RowsPlan pl;
  return wt32_qualify(a, &pl) == 0 ? 1 : 0;
}

extern "C" int ssrhip_gemv_wt32(const ssrhip_gemv_args* a, const uint16_t* Wt16, ssrhip_stream_t stream) {
  SSR_REQUIRE(a && Wt16, "ssrhip_gemv_wt32: null argument");
  RowsPlan pl;
  if (int rc = wt32_qualify(a, &pl)) return rc;
  const GemvWt16 q = {pl.r, Wt16};
  hipStream_t s = (hipStream_t)stream;
  const GemvR& r = pl.r;
  dim3 grid(r.wgs, a->groups), block(r.nw * 64);
  // the dispatch of ssrhip_gemv_mfma32_launch
  if (!pl.xreg && pl.pair) hipLaunchKernelGGL(wt32_stream_kernel<true>, grid, block, 0, s, q);
  else if (!pl.xreg) hipLaunchKernelGGL(wt32_stream_kernel<false>, grid, block, 0, s, q);
  else if (a->pro == SSRHIP_PRO_LAYERNORM) hipLaunchKernelGGL((wt32_xreg_kernel<SSRHIP_PRO_LAYERNORM, false>), grid, block, 0, s, q);
  else if (pl.pair) hipLaunchKernelGGL((wt32_xreg_kernel<SSRHIP_PRO_NONE, true>), grid, block, 0, s, q);
  else hipLaunchKernelGGL((wt32_xreg_kernel<SSRHIP_PRO_NONE, false>), grid, block, 0, s, q);
  SSR_LAUNCH_CHECK();
  return 0;
}
