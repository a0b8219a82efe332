// gemv_mfma32.hip — the fused weight-streaming GEMV for 17..32 rows: 16 utterances x CFG rows decoded in lock-step on one GPU,
// the weights read ONCE per step for all of them.
//
//   y[b][n] = epi( sum_k pro(x)[b][k] * W[n][k] + bias[n] ),   16 < B <= 32
//
// Same structure as the 5..16-row rows-per-workgroup kernels of gemv_mfma.hip (gemv_rows_xreg_kernel / gemv_rows_stream_kernel): rows dealt
// in 8-row units per workgroup, K split over <= 8 waves, rolling weight requests, the LayerNorm on register-resident x (ln_slice / ln_apply
// per panel), the split epilogue; kstep2 / kpair2 / merge_pair2 (gemv_mfma_tile.h) are the two-panel forms of the
// 16-row kernels' kstep1 / kpair1 / merge_pair.
// The one difference: the batch is two 16-column panels (include/ssrhip.h SSRHIP_TILED_P) and every weight fragment a lane loads feeds BOTH
// column tiles — 8 v_mfma_f32_16x16x4_f32 per float4 of W instead of 4 (16 instead of 8 in the k-step-pair form), into two accumulator sets,
// against x panel 0 and x panel 1. The HBM stream is the 16-row launch's; the matrix work doubles.
//
// Bit-identity: each output column gets exactly the arithmetic of the 16-row kernel — same wave K-split, same a0 / a1 interleave (or the
// same k-step pairs where the 16-row dispatcher picks them), same wave-order merge, same LayerNorm expressions — and an fp32 MFMA column
// does not depend on the other columns. Row b of a 32-row launch is therefore bit-identical to the same row in a 16-row launch. The host
// plan (waves, workgroups, pair form) is the 16-row dispatcher's, so that the pair decision, which changes the order, is the same too.
//
// Registers (one 8-wave workgroup per CU: up to 256 VGPR + AGPR per lane): both x panels of a K <= 2048 wave slice stay resident
// (2 x 16 float4 = 128) beside two accumulator sets and both panels' epilogue operands; the weight pipeline is 8 loads deep (16 in the
// k-step-pair forms), the depth that fits without scratch. K > 2048 (FFN2) streams both panels beside W.
// Columns >= B are clamped on load (row-major x) or read from the padded panel (tiled x) and masked on store.
#include <stdlib.h>
#include "common.h"
#include "gemv_mfma_tile.h"

namespace {

// Weight loads in flight per wave in the one-tile-per-k-step forms. 16 (the 16-row kernels' depth) does not fit 256 registers beside both
// x panels and both epilogues without scratch, so the depth is halved (8 KiB per wave, 64 KiB per CU); the k-step-pair forms keep theirs.
constexpr int DEP32 = 8;

// K <= 2048 (SPWX = 16 k-steps per wave): both x panels of the wave's K slice in VGPRs for all of the workgroup's tiles.
template <int PRO, bool PAIR>
__global__ __launch_bounds__(512) void gemv_rows32_xreg(const GemvR p) {
  constexpr int SPWX = 16, DEP = PAIR ? SPWX / 2 : DEP32;
  __shared__ float red[2][2][8][16];
  __shared__ f4v part[2][MAXT][8][64];
  const ssrhip_gemv_args& a = p.a;
  const ssrhip_gemv_args a0p = panel_args(a, 0), a1p = panel_args(a, 1);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, ks = lane >> 4;
  const int grp = blockIdx.y;
  const int N = a.N, K = a.K;
  const int u_lo = (int)((long long)blockIdx.x * p.units / p.wgs), u_hi = (int)((long long)(blockIdx.x + 1) * p.units / p.wgs);
  const int nun = u_hi - u_lo;
  if (nun <= 0) return;                                                 // uniform; only when wgs > units
  const int ntile = (nun + 1) >> 1;
  const int row_lo = u_lo * 8;
  const int last = p.steps - 1;
  const int tbase = wave * SPWX;
  const float* wbase = a.W + (size_t)grp * (a.w_tiled ? (size_t)p.units * 8 : (size_t)N) * K;
  const int wstep = a.w_tiled ? 128 : 16;
  const float* xb0 = panel_xptr(a, grp, 0, c, ks);
  const float* xb1 = panel_xptr(a, grp, 1, c, ks);
  const int xstep = a.x_tiled ? 256 : 16;

  float4 w[PAIR ? SPWX / 2 : DEP];
  float4 x0[SPWX], x1[SPWX];
  const int kvpos0 = tile_kvpos(a0p, lane), kvpos1 = tile_kvpos(a1p, lane);   // the wave's oldest loads (QKV launch only)
  __builtin_amdgcn_sched_barrier(0);
  const float* wp = tile_wptr(wbase, row_lo, nun, 0, c, ks, N, K, a.w_tiled) + (PAIR ? (c >> 3) * 128 : 0);
#pragma unroll
  for (int t = 0; t < SPWX; ++t) x0[t] = ld4(xb0 + min(tbase + t, last) * xstep);
#pragma unroll
  for (int t = 0; t < SPWX; ++t) x1[t] = ld4(xb1 + min(tbase + t, last) * xstep);
  __builtin_amdgcn_sched_barrier(0);
  if (PAIR) {
#pragma unroll
    for (int i = 0; i < SPWX / 2; ++i) w[i] = ld_nt(wp + min(tbase + 2 * i, last - 1) * wstep);   // host: steps even
  } else {
#pragma unroll
    for (int i = 0; i < DEP; ++i) w[i] = ld_nt(wp + min(tbase + i, last) * wstep);
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
    for (int i = 0; i < SPWX / 2; ++i) kpair2(w[i], x0[2 * i], x0[2 * i + 1], x1[2 * i], x1[2 * i + 1], aA0, aB0, aA1, aB1);
    part[0][0][wave][lane] = pair_fold(aA0, aB0);
    part[1][0][wave][lane] = pair_fold(aA1, aB1);
    __syncthreads();
    merge_pair2(a0p, a1p, part[0][0], part[1][0], p.nw, p.hd, e0, e1, wave, lane);
    return;
  }
  // all tiles but the last: the refills past this tile's k-range fetch the head of the next tile
  for (int tile = 0; tile < ntile - 1; ++tile) {
    const float* wn = tile_wptr(wbase, row_lo, nun, tile + 1, c, ks, N, K, a.w_tiled);
    f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, b0 = a0, b1 = a0;
#pragma unroll
    for (int t = 0; t < SPWX; ++t) {
      kstep2(w[t % DEP], x0[t], x1[t], a0, a1, b0, b1);
      if (t + DEP < SPWX) w[t % DEP] = ld_nt(wp + min(tbase + t + DEP, last) * wstep);
      else w[t % DEP] = ld_nt(wn + min(tbase + t + DEP - SPWX, last) * wstep);
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
      kstep2(w[t % DEP], x0[t], x1[t], a0, a1, b0, b1);
      if (t + DEP < SPWX) w[t % DEP] = ld_nt(wp + min(tbase + t + DEP, last) * wstep);
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

// K > 2048 without a LayerNorm prologue (FFN2, K = 8192): both x panels are streamed beside W (L2 hits), 16 k-steps of each in flight.
template <bool PAIR>
__global__ __launch_bounds__(512) void gemv_rows32_stream(const GemvR p) {
  constexpr int DEP = PAIR ? 16 : DEP32;     // k-steps per refill group (the k order of a column does not depend on it)
  __shared__ f4v part[2][MAXT][8][64];
  const ssrhip_gemv_args& a = p.a;
  const ssrhip_gemv_args a0p = panel_args(a, 0), a1p = panel_args(a, 1);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, ks = lane >> 4;
  const int grp = blockIdx.y;
  const int N = a.N, K = a.K;
  const int u_lo = (int)((long long)blockIdx.x * p.units / p.wgs), u_hi = (int)((long long)(blockIdx.x + 1) * p.units / p.wgs);
  const int nun = u_hi - u_lo;
  if (nun <= 0) return;
  const int ntile = (nun + 1) >> 1;
  const int row_lo = u_lo * 8;
  const int last = p.steps - 1;
  const int tbase = wave * p.spw;
  const int ngrp = p.spw / DEP;                  // groups of DEP k-steps per tile for this wave
  const float* wbase = a.W + (size_t)grp * (a.w_tiled ? (size_t)p.units * 8 : (size_t)N) * K;
  const int wstep = a.w_tiled ? 128 : 16;
  const float* xp0 = panel_xptr(a, grp, 0, c, ks);
  const float* xp1 = panel_xptr(a, grp, 1, c, ks);
  const int xstep = a.x_tiled ? 256 : 16;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

  float4 x0[DEP], x1[DEP];
  const int kvpos0 = tile_kvpos(a0p, lane), kvpos1 = tile_kvpos(a1p, lane);
  __builtin_amdgcn_sched_barrier(0);
  const float* wp = tile_wptr(wbase, row_lo, nun, 0, c, ks, N, K, a.w_tiled) + (PAIR ? (c >> 3) * 128 : 0);
  if (PAIR) {
    // one 8-row unit per workgroup: per group of 16 k-steps 8 weight loads (k-step pairs) + 2 x 16 x loads
    float4 wq[DEP / 2];
#pragma unroll
    for (int i = 0; i < DEP; ++i) { x0[i] = ld4(xp0 + min(tbase + i, last) * xstep); x1[i] = ld4(xp1 + min(tbase + i, last) * xstep); }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < DEP / 2; ++i) wq[i] = ld_nt(wp + min(tbase + 2 * i, last - 1) * wstep);
    __builtin_amdgcn_sched_barrier(0);
    const TileEpi e0 = tile_epilogue_fetch(a0p, p.hd, grp, row_lo, wave == 0 ? 8 : 0, lane, kvpos0);
    const TileEpi e1 = tile_epilogue_fetch(a1p, p.hd, grp, row_lo, wave == 0 ? 8 : 0, lane, kvpos1);
    __builtin_amdgcn_sched_barrier(0);
    f4v aA0 = {0.f, 0.f, 0.f, 0.f}, aB0 = aA0, aA1 = aA0, aB1 = aA0;
    for (int g = 0; g < ngrp - 1; ++g) {                                   // all groups but the last: refill for group g + 1
      const int kb = tbase + g * DEP, kbn = kb + DEP;
#pragma unroll
      for (int i = 0; i < DEP / 2; ++i) {
        const bool out = kb + 2 * i > last;                                // steps is even: a pair is in or out as a whole
        kpair2(wq[i], out ? z4 : x0[2 * i], out ? z4 : x0[2 * i + 1], out ? z4 : x1[2 * i], out ? z4 : x1[2 * i + 1], aA0, aB0, aA1, aB1);
        x0[2 * i] = ld4(xp0 + min(kbn + 2 * i, last) * xstep);
        x0[2 * i + 1] = ld4(xp0 + min(kbn + 2 * i + 1, last) * xstep);
        x1[2 * i] = ld4(xp1 + min(kbn + 2 * i, last) * xstep);
        x1[2 * i + 1] = ld4(xp1 + min(kbn + 2 * i + 1, last) * xstep);
        wq[i] = ld_nt(wp + min(kbn + 2 * i, last - 1) * wstep);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    {
      const int kb = tbase + (ngrp - 1) * DEP;
#pragma unroll
      for (int i = 0; i < DEP / 2; ++i) {
        const bool out = kb + 2 * i > last;
        kpair2(wq[i], out ? z4 : x0[2 * i], out ? z4 : x0[2 * i + 1], out ? z4 : x1[2 * i], out ? z4 : x1[2 * i + 1], aA0, aB0, aA1, aB1);
      }
    }
    part[0][0][wave][lane] = pair_fold(aA0, aB0);
    part[1][0][wave][lane] = pair_fold(aA1, aB1);
    __syncthreads();
    merge_pair2(a0p, a1p, part[0][0], part[1][0], p.nw, p.hd, e0, e1, wave, lane);
    return;
  }
  float4 w[DEP];
#pragma unroll
  for (int i = 0; i < DEP; ++i) { x0[i] = ld4(xp0 + min(tbase + i, last) * xstep); x1[i] = ld4(xp1 + min(tbase + i, last) * xstep); }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < DEP; ++i) w[i] = ld_nt(wp + min(tbase + i, last) * wstep);
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
    const float* wn = (tile_n == tile) ? wp : tile_wptr(wbase, row_lo, nun, tile_n, c, ks, N, K, a.w_tiled);
    const int kb = tbase + kg * DEP, kbn = tbase + kg_n * DEP;
#pragma unroll
    for (int t = 0; t < DEP; ++t) {
      const bool out = kb + t > last;                                      // uniform: k-steps past the end of K contribute nothing
      kstep2(w[t], out ? z4 : x0[t], out ? z4 : x1[t], a0, a1, b0, b1);
      const int kk = min(kbn + t, last);
      x0[t] = ld4(xp0 + kk * xstep);
      x1[t] = ld4(xp1 + kk * xstep);
      w[t] = ld_nt(wn + kk * wstep);
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
      const bool out = kb + t > last;
      kstep2(w[t], out ? z4 : x0[t], out ? z4 : x1[t], a0, a1, b0, b1);
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

}  // namespace

// called by ssrhip_gemv for 16 < B (validated here)
int ssrhip_gemv_mfma32_launch(const ssrhip_gemv_args* a, hipStream_t s) {
  if (int rc = gemv_rows_check(a, 17, 32, 2048)) return rc;
  // the plan is the one the 16-row launcher takes for this shape: the k-step-pair decision changes the accumulation order, and a row must
  // get the same arithmetic at 32 rows as at 16
  RowsPlan pl;
  if (int rc = gemv_rows_plan(a, /*ln_keeps_x=*/false, ssr_num_cu(), ssr_rows_knobs_get(), &pl)) return rc;
  const GemvR& r = pl.r;
  dim3 grid(r.wgs, a->groups), block(r.nw * 64);
  if (!pl.xreg && pl.pair) hipLaunchKernelGGL(gemv_rows32_stream<true>, grid, block, 0, s, r);
  else if (!pl.xreg) hipLaunchKernelGGL(gemv_rows32_stream<false>, grid, block, 0, s, r);
  else if (a->pro == SSRHIP_PRO_LAYERNORM) hipLaunchKernelGGL((gemv_rows32_xreg<SSRHIP_PRO_LAYERNORM, false>), grid, block, 0, s, r);
  else if (pl.pair) hipLaunchKernelGGL((gemv_rows32_xreg<SSRHIP_PRO_NONE, true>), grid, block, 0, s, r);
  else hipLaunchKernelGGL((gemv_rows32_xreg<SSRHIP_PRO_NONE, false>), grid, block, 0, s, r);
  SSR_LAUNCH_CHECK();
  return 0;
}
