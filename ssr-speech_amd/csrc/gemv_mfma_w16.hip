// gemv_mfma_w16.hip — the rows-per-workgroup matrix-core GEMV of gemv_mfma.hip (5..16 rows) over PACKED bf16 WEIGHTS: the bf16 weight
// stream of the 5..16-row decode step (DESIGN.md Part I.11).
//
//   y[b][n] = epi( sum_k pro(x)[b][k] * float(Wt16[n][k]) + bias[n] ),   5 <= B <= 16
//
// Only the bytes that are streamed change. bf16 -> fp32 is a 16-bit shift (`d << 16` for the low half of a dword, `d & 0xffff0000` for the
// high half) and exact; activations, accumulation, bias and the KV cache stay fp32; and every kernel below issues EXACTLY the MFMA sequence
// of its fp32 counterpart for the same k-steps — the same a0 / a1 (aA / aB) alternation, the same x operand per MFMA, the same LayerNorm
// statistics per 256-column slice merged in wave order, the same part[tile][wave][lane] sums in wave order, the same xor32 fold of the pair
// form, the same epilogue — by calling the fp32 kernels' own pieces (gemv_mfma_tile.h: ln_slice / ln_apply, kstep1, kpair1, pair_fold, merge_pair)
// on a widened weight fragment — on the same launch plan (gemv_rows_plan). So a launch here equals ssrhip_gemv on the fp32
// streaming-order copy of the rounded master bit for bit (tests/test_gpu_wt16.py compares with torch.equal).
//
// Layout (include/ssrhip.h SSRHIP_WT16_INDEX): rows in 8-row units (zero-padded), K in QUADS of four k-steps (64 floats; K % 64 == 0).
// The 512-byte block (unit u, quad q, h) holds at 16-byte piece ks*8 + c the four weights of k-step 4q + h followed by the four of k-step
// 4q + h + 2 (row 8u + c, k-slot ks). One layout feeds both kernel forms with 1 KiB wave-level loads:
//   plain  lanes c >= 8 belong to the next unit. A lane issues loads h = 0 and h = 1 of a quad and consumes k-steps 4q (load 0, low
//          half), 4q + 1 (load 1, low), 4q + 2 (load 0, high), 4q + 3 (load 1, high): 8 MFMAs per load, two 512-byte runs per wave load;
//   pair   (every workgroup owns ONE 8-row unit) lanes c < 8 load piece h = 0, lanes c >= 8 piece h = 1 of the same (u, q): one contiguous
//          KiB. The low halves are the fp32 kernel's k-step pair (4q, 4q + 1), the high halves its pair (4q + 2, 4q + 3): 16 MFMAs per load.
// A wave's K slice starts at a multiple of 16 k-steps, so it is quad-aligned; a quad past the end of K is clamped to the last quad (its x
// is zeroed as in the fp32 kernels, a product of zero adds nothing to a sum that starts at +0).
//
// What gemv_mfma.hip's round-5 findings paid for is kept: kv_pos is the wave's oldest load, the page-table entry and bias / residual are
// requested before the weight loop, no weight load sits under a run-time branch, the last tile is a separate code path (no load predicated,
// none wasted), the pipeline does not drain between tiles. Loads in flight per wave: DL = 8 (8 KiB: the fp32 kernels' 16 k-steps ahead
// with half the bytes); the other candidate, 16 loads = the fp32 kernels' 16 KiB, exists for the two-tile LayerNorm launches as an opt-in
// (wt16_xreg_kernel NT = 2). The recorded negatives of the fp32 unit (SSRHIP_GEMVM_EDGE, _WFIRST, _DEP8, SSRHIP_GEMVM_V=1) have no bf16 form.
// No bf16 MFMA and no v_dot2: either would round x.
#include <stdlib.h>
#include "common.h"
#include "gemv_mfma_tile.h"

namespace {

// x in registers (K <= 2048: SPWX = 16 k-steps per wave; LayerNorm launches up to K = 4096: SPWX = 32): gemv_rows_xreg_kernel over bf16.
// NT = 0: a ring of DL loads that rolls over the workgroup's tiles. NT = 2 (host-selected when EVERY workgroup owns exactly two tiles: QKV,
// FFN1 at 830M): no ring — both tiles' loads, 2 x SPWX / 2 = 16 per wave (16 KiB, the fp32 kernels' bytes in flight), are requested at
// entry. Same MFMA sequence; the opt-in arm of the loads-in-flight measurement (SSRHIP_GEMVM_W16_DEPTH=16, DESIGN.md Part I.11).
template <int PRO, int SPWX, int DL, bool PAIR, int NT = 0>
__global__ __launch_bounds__(512) void wt16_xreg_kernel(const GemvWt16 pw) {
  constexpr int LPT = SPWX / 2;                     // plain form: weight loads per tile and wave
  static_assert(LPT % DL == 0 && SPWX % 16 == 0, "the ring must divide a tile's loads; slices are quad-aligned");
  static_assert(NT == 0 || (NT == 2 && !PAIR), "all-at-entry form: two tiles, plain");
  __shared__ float red[2][8][16];
  __shared__ f4v part[MAXT][8][64];
  const GemvR& p = pw.r;
  const ssrhip_gemv_args& a = p.a;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, ks = lane >> 4;
  const int grp = blockIdx.y;
  const int K = a.K, B = a.B;
  const int u_lo = (int)((long long)blockIdx.x * p.units / p.wgs), u_hi = (int)((long long)(blockIdx.x + 1) * p.units / p.wgs);
  const int nun = u_hi - u_lo;
  if (nun <= 0) return;                                                 // uniform; only when wgs > units
  const int ntile = (nun + 1) >> 1;
  const int row_lo = u_lo * 8;
  const int last = p.steps - 1;
  const int tbase = wave * SPWX;
  const int lastq = (K >> 6) - 1, qbase = tbase >> 2;
  const uint16_t* wbase = pw.w16 + (size_t)grp * ((size_t)p.units * 8) * K;
  const float* xbase = a.x_tiled ? a.x + (size_t)grp * K * 16 : a.x + (size_t)grp * K;
  const unsigned xvoff = a.x_tiled ? (unsigned)(ks * 16 + c) * 4 : (unsigned)min(c, B - 1) * (unsigned)a.x_stride + ks * 4;
  const int xstep = a.x_tiled ? 256 : 16;

  wt16_v4u w[NT == 2 ? 2 * LPT : (SPWX / 4 > DL ? SPWX / 4 : DL)];      // pair form: SPWX / 4 loads, all requested at entry; plain form: a ring of DL
  float4 xr[SPWX];
  const int kvpos = tile_kvpos(a, lane);                                // the wave's oldest load (QKV launch only)
  __builtin_amdgcn_sched_barrier(0);
  const uint16_t* wp = wt16_ptr(wbase, row_lo, nun, 0, c, ks, K) + (PAIR ? (c >> 3) * 256 : 0);
#pragma unroll
  for (int t = 0; t < SPWX; ++t) xr[t] = ld4(xbase + min(tbase + t, last) * xstep + xvoff);
  __builtin_amdgcn_sched_barrier(0);
  if (PAIR) {
#pragma unroll
    for (int i = 0; i < SPWX / 4; ++i) w[i] = ldw_nt(wp + min(qbase + i, lastq) * 512);     // one quad (two k-step pairs) per load
  } else if (NT == 2) {
    const uint16_t* wn = wt16_ptr(wbase, row_lo, nun, 1, c, ks, K);
#pragma unroll
    for (int i = 0; i < LPT; ++i) w[i] = ldw_nt(wp + wt16_off(qbase, i, lastq));
#pragma unroll
    for (int i = 0; i < LPT; ++i) w[LPT + i] = ldw_nt(wn + wt16_off(qbase, i, lastq));
  } else {
#pragma unroll
    for (int i = 0; i < DL; ++i) w[i] = ldw_nt(wp + wt16_off(qbase, i, lastq));
  }
  __builtin_amdgcn_sched_barrier(0);
  // what this wave's epilogue (tile `wave`) will need, requested now (behind the first weight loads, used after the last MFMA)
  const bool epi_mine = wave < ntile;
  const TileEpi epi0 = tile_epilogue_fetch(a, p.hd, grp, row_lo + wave * 16, epi_mine ? tile_rows_of(wave, nun) : 0, lane, kvpos);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < SPWX; ++t) asm volatile("" : "+v"(xr[t].x), "+v"(xr[t].y), "+v"(xr[t].z), "+v"(xr[t].w));
#pragma unroll
  for (int t = 0; t < SPWX; ++t)
    if (tbase + t > last) xr[t] = make_float4(0.f, 0.f, 0.f, 0.f);

  if (PRO == SSRHIP_PRO_LAYERNORM) {
    // gemv_rows_xreg_kernel's LayerNorm: per-wave two-pass statistics of the K slice, merged in wave order (Chan)
    float mw, q;
    ln_slice<SPWX>(xr, tbase, last, &mw, &q);
    if (ks == 0) { red[0][wave][c] = mw; red[1][wave][c] = q; }
    __syncthreads();
    ln_apply<SPWX>(xr, red, p.nw, c, tbase, last, K, a.ln_eps);
  }

  if (PAIR) {
    f4v aA = {0.f, 0.f, 0.f, 0.f}, aB = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < SPWX / 4; ++i) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {                                       // the fp32 kernel's pair 2i + g = k-steps (4i + 2g, 4i + 2g + 1)
        const float4 wv = wt16_widen(w[i], g), xa = xr[4 * i + 2 * g], xb = xr[4 * i + 2 * g + 1];
        kpair1(wv, xa, xb, aA, aB);
      }
    }
    const f4v acc = pair_fold(aA, aB);
    part[0][wave][lane] = acc;
    __syncthreads();
    merge_pair(a, part[0], p.nw, p.hd, epi0, wave, lane);
    return;
  }
  // k-step t of a tile reads load m = 2 (t / 4) + t % 2, half g = (t / 2) % 2
  if (NT == 2) {
#pragma unroll
    for (int tile = 0; tile < 2; ++tile) {
      f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < SPWX; ++t) {
        const int m = 2 * (t >> 2) + (t & 1), g = (t >> 1) & 1;
        const float4 wv = wt16_widen(w[tile * LPT + m], g), xv = xr[t];
        kstep1(wv, xv, a0, a1);
        __builtin_amdgcn_sched_barrier(0);
      }
      part[tile][wave][lane] = a0 + a1;
    }
  } else {
  // a load is used up after its high half (g = 1) and its registers are refilled at once. All tiles but the last: the refills past this
  // tile's loads fetch the head of the next tile
  for (int tile = 0; tile < ntile - 1; ++tile) {
    const uint16_t* wn = wt16_ptr(wbase, row_lo, nun, tile + 1, c, ks, K);
    f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < SPWX; ++t) {
      const int m = 2 * (t >> 2) + (t & 1), g = (t >> 1) & 1;
      const float4 wv = wt16_widen(w[m % DL], g), xv = xr[t];
      kstep1(wv, xv, a0, a1);
      if (g == 1) {
        if (m + DL < LPT) w[m % DL] = ldw_nt(wp + wt16_off(qbase, m + DL, lastq));
        else w[m % DL] = ldw_nt(wn + wt16_off(qbase, m + DL - LPT, lastq));
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    part[tile][wave][lane] = a0 + a1;
    wp = wn;
  }
  {
    f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < SPWX; ++t) {
      const int m = 2 * (t >> 2) + (t & 1), g = (t >> 1) & 1;
      const float4 wv = wt16_widen(w[m % DL], g), xv = xr[t];
      kstep1(wv, xv, a0, a1);
      if (g == 1 && m + DL < LPT) w[m % DL] = ldw_nt(wp + wt16_off(qbase, m + DL, lastq));
      __builtin_amdgcn_sched_barrier(0);
    }
    part[ntile - 1][wave][lane] = a0 + a1;
  }
  }
  __syncthreads();
  for (int tile = wave; tile < ntile; tile += p.nw) {
    f4v acc = part[tile][0][lane];
    for (int v = 1; v < p.nw; ++v) acc += part[tile][v][lane];
    if (tile == wave) tile_epilogue_finish(a, epi0, acc, p.hd);
    else tile_epilogue(a, p.hd, grp, row_lo + tile * 16, (2 * tile + 1 < nun) ? 16 : 8, lane, acc);
  }
}

// K > 2048 without a LayerNorm prologue (FFN2, K = 8192): gemv_rows_stream_kernel over bf16 — x is streamed beside W in groups of 16
// k-steps: per group 16 x loads (L2) and 8 weight loads (4 in the pair form), all of them refilled while the group is consumed.
template <bool PAIR>
__global__ __launch_bounds__(512) void wt16_stream_kernel(const GemvWt16 pw) {
  constexpr int DEP = 16;                         // k-steps per group
  __shared__ f4v part[MAXT][8][64];
  const GemvR& p = pw.r;
  const ssrhip_gemv_args& a = p.a;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, ks = lane >> 4;
  const int grp = blockIdx.y;
  const int K = a.K, B = a.B;
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
  const float* xp = (a.x_tiled ? a.x + (size_t)grp * K * 16 : a.x + (size_t)grp * K) +
                    (a.x_tiled ? (unsigned)(ks * 16 + c) * 4 : (unsigned)min(c, B - 1) * (unsigned)a.x_stride + ks * 4);
  const int xstep = a.x_tiled ? 256 : 16;

  float4 xr[DEP];
  const int kvpos = tile_kvpos(a, lane);                                // the wave's oldest load (QKV launch only)
  __builtin_amdgcn_sched_barrier(0);
  const uint16_t* wp = wt16_ptr(wbase, row_lo, nun, 0, c, ks, K) + (PAIR ? (c >> 3) * 256 : 0);
  if (PAIR) {
    // one 8-row unit per workgroup: per group of 16 k-steps 4 weight loads (a quad = two k-step pairs each) + 16 x loads
    wt16_v4u wq[DEP / 4];
#pragma unroll
    for (int i = 0; i < DEP; ++i) xr[i] = ld4(xp + min(tbase + i, last) * xstep);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < DEP / 4; ++i) wq[i] = ldw_nt(wp + min(qbase + i, lastq) * 512);
    __builtin_amdgcn_sched_barrier(0);
    const TileEpi epi0 = tile_epilogue_fetch(a, p.hd, grp, row_lo, wave == 0 ? 8 : 0, lane, kvpos);
    __builtin_amdgcn_sched_barrier(0);
    f4v aA = {0.f, 0.f, 0.f, 0.f}, aB = {0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < ngrp - 1; ++g) {                                   // all groups but the last: refill for group g + 1
      const int kb = tbase + g * DEP, kbn = kb + DEP, qn = kbn >> 2;
#pragma unroll
      for (int j = 0; j < DEP / 2; ++j) {                                  // the fp32 kernel's pair j = k-steps (2j, 2j + 1) of the group
        const float4 wv = wt16_widen(wq[j >> 1], j & 1);
        float4 xa = xr[2 * j], xb = xr[2 * j + 1];
        if (kb + 2 * j > last) { xa = make_float4(0.f, 0.f, 0.f, 0.f); xb = xa; }   // steps is even: a pair is in or out as a whole
        kpair1(wv, xa, xb, aA, aB);
        xr[2 * j] = ld4(xp + min(kbn + 2 * j, last) * xstep);
        xr[2 * j + 1] = ld4(xp + min(kbn + 2 * j + 1, last) * xstep);
        if (j & 1) wq[j >> 1] = ldw_nt(wp + min(qn + (j >> 1), lastq) * 512);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    {
      const int kb = tbase + (ngrp - 1) * DEP;
#pragma unroll
      for (int j = 0; j < DEP / 2; ++j) {
        const float4 wv = wt16_widen(wq[j >> 1], j & 1);
        float4 xa = xr[2 * j], xb = xr[2 * j + 1];
        if (kb + 2 * j > last) { xa = make_float4(0.f, 0.f, 0.f, 0.f); xb = xa; }
        kpair1(wv, xa, xb, aA, aB);
      }
    }
    f4v acc;                                                              // pair_fold's sum, written out as in gemv_rows_stream_kernel<true>
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = aA[e] + xor32_f(aB[e]);
    part[0][wave][lane] = acc;
    __syncthreads();
    merge_pair(a, part[0], p.nw, p.hd, epi0, wave, lane);
    return;
  }
  constexpr int NL = DEP / 2;                     // weight loads per group
  wt16_v4u w[NL];
#pragma unroll
  for (int i = 0; i < DEP; ++i) xr[i] = ld4(xp + min(tbase + i, last) * xstep);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < NL; ++i) w[i] = ldw_nt(wp + wt16_off(qbase, i, lastq));
  __builtin_amdgcn_sched_barrier(0);
  const bool epi_mine = wave < ntile;
  const TileEpi epi0 = tile_epilogue_fetch(a, p.hd, grp, row_lo + wave * 16, epi_mine ? tile_rows_of(wave, nun) : 0, lane, kvpos);
  __builtin_amdgcn_sched_barrier(0);
  const int total = ntile * ngrp;
  f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
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
      const float4 wv = wt16_widen(w[m], h);
      float4 xv = xr[t];
      if (kb + t > last) xv = make_float4(0.f, 0.f, 0.f, 0.f);           // uniform: k-steps past the end of K contribute nothing
      kstep1(wv, xv, a0, a1);
      xr[t] = ld4(xp + min(kbn + t, last) * xstep);
      if (h == 1) w[m] = ldw_nt(wn + wt16_off(qn, m, lastq));
      __builtin_amdgcn_sched_barrier(0);
    }
    if (kg_n == 0) {                                                      // uniform: tile finished
      part[tile][wave][lane] = a0 + a1;
      a0 = (f4v){0.f, 0.f, 0.f, 0.f};
      a1 = (f4v){0.f, 0.f, 0.f, 0.f};
    }
    tile = tile_n; kg = kg_n; wp = wn;
  }
  {
    const int kb = tbase + kg * DEP;
#pragma unroll
    for (int t = 0; t < DEP; ++t) {
      const int m = 2 * (t >> 2) + (t & 1), h = (t >> 1) & 1;
      const float4 wv = wt16_widen(w[m], h);
      float4 xv = xr[t];
      if (kb + t > last) xv = make_float4(0.f, 0.f, 0.f, 0.f);
      kstep1(wv, xv, a0, a1);
    }
    part[ntile - 1][wave][lane] = a0 + a1;
  }
  __syncthreads();
  for (int tile = wave; tile < ntile; tile += p.nw) {
    f4v acc = part[tile][0][lane];
    for (int v = 1; v < p.nw; ++v) acc += part[tile][v][lane];
    if (tile == wave) tile_epilogue_finish(a, epi0, acc, p.hd);
    else tile_epilogue(a, p.hd, grp, row_lo + tile * 16, (2 * tile + 1 < nun) ? 16 : 8, lane, acc);
  }
}

constexpr int WT16_DL = 8;      // weight loads in flight per wave (8 KiB)

// SSRHIP_GEMVM_W16_DEPTH=16 (read at every call, i.e. at graph capture): the LayerNorm launches at K <= 2048 whose workgroups own exactly
// two tiles each take the all-at-entry form (16 loads = 16 KiB per wave); every other value, and every other launch, is the ring of 8
bool wt16_depth16() { const char* e = getenv("SSRHIP_GEMVM_W16_DEPTH"); return e && atoi(e) == 16; }

// the packed kernels' contract: the check and the plan of ssrhip_gemv_mfma_launch's rows-per-workgroup kernels (SSRHIP_GEMVM_V=1, the
// per-tile kernel of round 1, has no bf16 form)
int wt16_qualify(const ssrhip_gemv_args* a, RowsPlan* pl) {
  return gemv_wt_qualify(a, "ssrhip_gemv_wt16", 5, 16, 4096, /*ln_keeps_x=*/true, /*v1_refuses=*/true, pl);
}

}  // namespace

extern "C" int ssrhip_gemv_wt16_applicable(const ssrhip_gemv_args* a) {
  if (!a) return 0;
  RowsPlan pl;
  return wt16_qualify(a, &pl) == 0 ? 1 : 0;
}

extern "C" int ssrhip_gemv_wt16(const ssrhip_gemv_args* a, const uint16_t* Wt16, ssrhip_stream_t stream) {
  SSR_REQUIRE(a && Wt16, "ssrhip_gemv_wt16: null argument");
  RowsPlan pl;
  if (int rc = wt16_qualify(a, &pl)) return rc;
  const GemvWt16 q = {pl.r, Wt16};
  hipStream_t s = (hipStream_t)stream;
  const GemvR& r = pl.r;
  const bool ln = a->pro == SSRHIP_PRO_LAYERNORM;
  const bool x16 = r.spw == 16;                          // (x in registers) 16 k-steps of it per wave: K <= 2048
  dim3 grid(r.wgs, a->groups), block(r.nw * 64);
  // the dispatch of ssrhip_gemv_mfma_launch without its opt-in experiments
  if (!pl.xreg && pl.pair) hipLaunchKernelGGL(wt16_stream_kernel<true>, grid, block, 0, s, q);
  else if (!pl.xreg) hipLaunchKernelGGL(wt16_stream_kernel<false>, grid, block, 0, s, q);
  else if (pl.pair && !ln && x16) hipLaunchKernelGGL((wt16_xreg_kernel<SSRHIP_PRO_NONE, 16, WT16_DL, true>), grid, block, 0, s, q);
  else if (ln && x16 && r.units % r.wgs == 0 && (r.units / r.wgs == 3 || r.units / r.wgs == 4) && wt16_depth16())
    hipLaunchKernelGGL((wt16_xreg_kernel<SSRHIP_PRO_LAYERNORM, 16, WT16_DL, false, 2>), grid, block, 0, s, q);
  else if (ln && x16) hipLaunchKernelGGL((wt16_xreg_kernel<SSRHIP_PRO_LAYERNORM, 16, WT16_DL, false>), grid, block, 0, s, q);
  else if (ln) hipLaunchKernelGGL((wt16_xreg_kernel<SSRHIP_PRO_LAYERNORM, 32, WT16_DL, false>), grid, block, 0, s, q);
  else if (x16) hipLaunchKernelGGL((wt16_xreg_kernel<SSRHIP_PRO_NONE, 16, WT16_DL, false>), grid, block, 0, s, q);
  else hipLaunchKernelGGL((wt16_xreg_kernel<SSRHIP_PRO_NONE, 32, WT16_DL, false>), grid, block, 0, s, q);
  SSR_LAUNCH_CHECK();
  return 0;
}
