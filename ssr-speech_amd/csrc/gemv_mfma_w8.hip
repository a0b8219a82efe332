// gemv_mfma_w8.hip — the rows-per-workgroup matrix-core GEMV of gemv_mfma.hip (5..16 rows) over PACKED OCP e4m3 CODES with one power-of-two
// scale per output row: the e4m3 weight stream of the 5..16-row decode step (DESIGN.md Part I.22).
//
//   y[b][n] = epi( sum_k pro(x)[b][k] * (float(Wt8[n][k]) * scale[n]) + bias[n] ),   5 <= B <= 16
//
// Only the bytes that are streamed change. A code is widened by v_cvt_pk_f32_fp8 (exact) and MULTIPLIED BY ITS ROW'S SCALE BEFORE IT ENTERS
// THE MFMA: code * 2^e is exact and is the fp32 master, so every kernel below hands kstep1 / kpair1 (gemv_mfma_tile.h) the very operands the
// fp32 kernel reads from the streaming-order copy of the master, in the same order, on the same launch plan (gemv_rows_plan) — the same
// a0 / a1 (aA / aB) alternation, LayerNorm statistics, part[tile][wave][lane] sums in wave order, xor32 fold and epilogue. A launch here
// equals ssrhip_gemv on the fp32 streaming-order copy of code * scale bit for bit, without a caveat about subnormal partial sums (the scale
// never touches a sum). A lane's weight row is fixed per tile, so the scale is one float per lane and tile; it is requested AHEAD of that
// tile's first codes (then it is the older load and waiting for it drains nothing), its row index clamped to N - 1 (padded rows hold code 0
// and are never stored).
//
// Layout (include/ssrhip.h SSRHIP_WT8_INDEX): rows in 8-row units (zero-padded), K in OCTETS of eight k-steps (128 codes; K % 128 == 0).
// The 512-byte block (unit u, octet o, h) holds at 16-byte piece ks*8 + c, as dword g, the four codes of k-step 8o + 2g + h (row 8u + c,
// k-slot ks). One layout feeds both kernel forms with 1 KiB wave-level loads:
//   plain  lanes c >= 8 belong to the next unit. A lane issues loads h = 0 and h = 1 of an octet; dword g of load h is k-step 8o + 2g + h:
//          16 MFMAs per load, two 512-byte runs per wave load;
//   pair   (every workgroup owns ONE 8-row unit) lanes c < 8 load piece h = 0, lanes c >= 8 piece h = 1 of the same (u, o): one contiguous
//          KiB. Dword g is the fp32 kernel's k-step pair (8o + 2g, 8o + 2g + 1): 32 MFMAs per load.
// A wave's K slice starts at a multiple of 16 k-steps, so it is octet-aligned; an octet past the end of K is clamped to the last octet (its
// x is zeroed as in the fp32 kernels, a product of zero adds nothing to a sum that starts at +0).
//
// What gemv_mfma.hip's round-5 findings paid for is kept: kv_pos is the wave's oldest load, the page-table entry and bias / residual are
// requested before the weight loop, no load sits under a run-time branch, the last tile is a separate code path (no load predicated, none
// wasted), the pipeline does not drain between tiles. Loads in flight per wave: ONE TILE AHEAD — while a tile is consumed, every used-up
// load is re-requested at once for the same slot of the next tile: SPWX / 4 loads = 4 KiB at 16 k-steps per wave, 8 KiB at 32; the
// streaming kernel keeps one group of 16 k-steps ahead (4 loads, 2 in the pair form). No fp8 / bf16 MFMA and no v_dot: either would round x.
#include <stdlib.h>
#include "common.h"
#include "gemv_mfma_tile.h"

namespace {

typedef unsigned wt8_v4u __attribute__((ext_vector_type(4)));
typedef float wt8_v2f __attribute__((ext_vector_type(2)));

struct GemvWt8 {
  GemvR r;               // the fp32 launch's parameter, from the same plan
  const uint8_t* w8;     // [groups][units * 8][K] codes in SSRHIP_WT8_INDEX order
  const float* scale;    // [groups][N]: 2^e of each output row
};

// 16 packed codes of a streamed-once weight block: non-temporal 16-byte load (global_load_dwordx4 ... nt)
__device__ __forceinline__ wt8_v4u ldw8_nt(const uint8_t* p) { return __builtin_nontemporal_load(reinterpret_cast<const wt8_v4u*>(p)); }

// the float4 of one k-step: the four codes of one dword (code m in byte m), widened exactly and scaled exactly: the fp32 master's values
__device__ __forceinline__ float4 wt8_wide(const unsigned d, const float sc) {
  const wt8_v2f lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)d, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)d, true);
  return make_float4(lo.x * sc, lo.y * sc, hi.x * sc, hi.y * sc);
}

// the weight row of this lane in tile `tile` (tile_wptr's row: an 8-row tile duplicates its rows in lanes c >= 8)
__device__ __forceinline__ int wt8_row(int row_lo, int nun, int tile, int c) {
  const int rows = (2 * tile + 1 < nun) ? 16 : 8;
  return row_lo + tile * 16 + (c & (rows - 1));
}

// per-lane pointer to (row of this lane in tile `tile`, k-slot of this lane) of the packed matrix: block (unit, octet 0, h = 0)
__device__ __forceinline__ const uint8_t* wt8_ptr(const uint8_t* wbase, int row_lo, int nun, int tile, int c, int ks, int K) {
  const int rr = wt8_row(row_lo, nun, tile, c);
  return wbase + (size_t)(rr >> 3) * 8 * K + (ks * 8 + (rr & 7)) * 16;    // units are zero-padded: no row clamp
}

// this lane's scale in tile `tile`; sg = the group's scales [N]
__device__ __forceinline__ float wt8_scale(const float* sg, int row_lo, int nun, int tile, int c, int N) {
  return sg[min(wt8_row(row_lo, nun, tile, c), N - 1)];
}

// byte offset of load m (m = 2 * octet + h, counted from the wave's first octet `obase`) behind wt8_ptr; octets past the end are clamped
__device__ __forceinline__ int wt8_off(int obase, int m, int lasto) { return (min(obase + (m >> 1), lasto) * 2 + (m & 1)) * 512; }

// In front of the streaming kernels' group loop: wait for every load of the entry (x, scale, codes, epilogue operands) — s_waitcnt vmcnt(0).
// The first group needs its x and codes anyway. Without it the compiler merges, at the loop header, the entry's state (behind the first
// codes come the epilogue's loads, which sit under the lane's row predicate: an unknown number) with the back edge's and waits at EVERY
// group as if for the entry: `vmcnt(1)` (pair form) / `vmcnt(4)`, i.e. for the x loads issued a few instructions earlier (read off the
// ISA). With it the loop waits for what the back edge left in flight. (simm16: vmcnt 0, expcnt 7, lgkmcnt 15 = no wait on those two.)
__device__ __forceinline__ void wt8_entry_wait() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// x in registers (K <= 2048: SPWX = 16 k-steps per wave; LayerNorm launches up to K = 4096: SPWX = 32): gemv_rows_xreg_kernel over codes.
// k-step t of a tile reads load m = 2 (t / 8) + t % 2, dword g = (t / 2) % 4.
template <int PRO, int SPWX, bool PAIR>
__global__ __launch_bounds__(512) void wt8_xreg_kernel(const GemvWt8 pw) {
  constexpr int LPT = SPWX / 4;                     // plain form: weight loads per tile and wave (= the loads in flight)
  constexpr int NLD = PAIR ? SPWX / 8 : LPT;        // pair form: one octet (four k-step pairs) per load, all requested at entry
  static_assert(SPWX % 16 == 0, "slices are octet-aligned");
  __shared__ float red[2][8][16];
  __shared__ f4v part[MAXT][8][64];
  const GemvR& p = pw.r;
  const ssrhip_gemv_args& a = p.a;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, ks = lane >> 4;
  const int grp = blockIdx.y;
  const int K = a.K, B = a.B, N = a.N;
  const int u_lo = (int)((long long)blockIdx.x * p.units / p.wgs), u_hi = (int)((long long)(blockIdx.x + 1) * p.units / p.wgs);
  const int nun = u_hi - u_lo;
  if (nun <= 0) return;                                                 // uniform; only when wgs > units
  const int ntile = (nun + 1) >> 1;
  const int row_lo = u_lo * 8;
  const int last = p.steps - 1;
  const int tbase = wave * SPWX;
  const int lasto = (K >> 7) - 1, obase = tbase >> 3;
  const uint8_t* wbase = pw.w8 + (size_t)grp * ((size_t)p.units * 8) * K;
  const float* sg = pw.scale + (size_t)grp * N;
  const float* xbase = a.x_tiled ? a.x + (size_t)grp * K * 16 : a.x + (size_t)grp * K;
  const unsigned xvoff = a.x_tiled ? (unsigned)(ks * 16 + c) * 4 : (unsigned)min(c, B - 1) * (unsigned)a.x_stride + ks * 4;
  const int xstep = a.x_tiled ? 256 : 16;

  wt8_v4u w[NLD];
  float4 xr[SPWX];
  const int kvpos = tile_kvpos(a, lane);                                // the wave's oldest load (QKV launch only)
  __builtin_amdgcn_sched_barrier(0);
  const uint8_t* wp = wt8_ptr(wbase, row_lo, nun, 0, c, ks, K) + (PAIR ? (c >> 3) * 512 : 0);
#pragma unroll
  for (int t = 0; t < SPWX; ++t) xr[t] = ld4(xbase + min(tbase + t, last) * xstep + xvoff);
  __builtin_amdgcn_sched_barrier(0);
  float sc = wt8_scale(sg, row_lo, nun, 0, c, N);                       // ahead of the tile's first codes
  __builtin_amdgcn_sched_barrier(0);
  if (PAIR) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) w[i] = ldw8_nt(wp + min(obase + i, lasto) * 1024);
  } else {
#pragma unroll
    for (int i = 0; i < NLD; ++i) w[i] = ldw8_nt(wp + wt8_off(obase, i, lasto));
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
    for (int i = 0; i < NLD; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {                                       // the fp32 kernel's pair 4i + g = k-steps (8i + 2g, 8i + 2g + 1)
        const float4 wv = wt8_wide(w[i][g], sc), xa = xr[8 * i + 2 * g], xb = xr[8 * i + 2 * g + 1];
        kpair1(wv, xa, xb, aA, aB);
      }
    }
    const f4v acc = pair_fold(aA, aB);
    part[0][wave][lane] = acc;
    __syncthreads();
    merge_pair(a, part[0], p.nw, p.hd, epi0, wave, lane);
    return;
  }
  // a load is used up after its last dword (g = 3) and its registers are refilled at once with the same load of the next tile, whose
  // scale was requested just before the first of them
  for (int tile = 0; tile < ntile - 1; ++tile) {
    const uint8_t* wn = wt8_ptr(wbase, row_lo, nun, tile + 1, c, ks, K);
    const float sn = wt8_scale(sg, row_lo, nun, tile + 1, c, N);
    __builtin_amdgcn_sched_barrier(0);
    f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < SPWX; ++t) {
      const int m = 2 * (t >> 3) + (t & 1), g = (t >> 1) & 3;
      const float4 wv = wt8_wide(w[m][g], sc), xv = xr[t];
      kstep1(wv, xv, a0, a1);
      if (g == 3) w[m] = ldw8_nt(wn + wt8_off(obase, m, lasto));
      __builtin_amdgcn_sched_barrier(0);
    }
    part[tile][wave][lane] = a0 + a1;
    sc = sn;
  }
  {
    f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < SPWX; ++t) {
      const int m = 2 * (t >> 3) + (t & 1), g = (t >> 1) & 3;
      const float4 wv = wt8_wide(w[m][g], sc), xv = xr[t];
      kstep1(wv, xv, a0, a1);
      __builtin_amdgcn_sched_barrier(0);
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

// K > 2048 without a LayerNorm prologue (FFN2, K = 8192): gemv_rows_stream_kernel over codes — x is streamed beside the codes in groups of
// 16 k-steps: per group 16 x loads (L2) and 4 weight loads (2 in the pair form), all of them refilled while the group is consumed.
template <bool PAIR>
__global__ __launch_bounds__(512) void wt8_stream_kernel(const GemvWt8 pw) {
  constexpr int DEP = 16;                         // k-steps per group
  __shared__ f4v part[MAXT][8][64];
  const GemvR& p = pw.r;
  const ssrhip_gemv_args& a = p.a;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, ks = lane >> 4;
  const int grp = blockIdx.y;
  const int K = a.K, B = a.B, N = a.N;
  const int u_lo = (int)((long long)blockIdx.x * p.units / p.wgs), u_hi = (int)((long long)(blockIdx.x + 1) * p.units / p.wgs);
  const int nun = u_hi - u_lo;
  if (nun <= 0) return;
  const int ntile = (nun + 1) >> 1;
  const int row_lo = u_lo * 8;
  const int last = p.steps - 1;
  const int tbase = wave * p.spw;                 // host: spw is a multiple of 16 k-steps
  const int ngrp = p.spw / DEP;
  const int lasto = (K >> 7) - 1, obase = tbase >> 3;
  const uint8_t* wbase = pw.w8 + (size_t)grp * ((size_t)p.units * 8) * K;
  const float* sg = pw.scale + (size_t)grp * N;
  const float* xp = (a.x_tiled ? a.x + (size_t)grp * K * 16 : a.x + (size_t)grp * K) +
                    (a.x_tiled ? (unsigned)(ks * 16 + c) * 4 : (unsigned)min(c, B - 1) * (unsigned)a.x_stride + ks * 4);
  const int xstep = a.x_tiled ? 256 : 16;

  float4 xr[DEP];
  const int kvpos = tile_kvpos(a, lane);                                // the wave's oldest load (QKV launch only)
  __builtin_amdgcn_sched_barrier(0);
  const uint8_t* wp = wt8_ptr(wbase, row_lo, nun, 0, c, ks, K) + (PAIR ? (c >> 3) * 512 : 0);
  if (PAIR) {
    // one 8-row unit per workgroup: per group of 16 k-steps 2 weight loads (an octet = four k-step pairs each) + 16 x loads
    wt8_v4u wq[DEP / 8];
#pragma unroll
    for (int i = 0; i < DEP; ++i) xr[i] = ld4(xp + min(tbase + i, last) * xstep);
    __builtin_amdgcn_sched_barrier(0);
    const float sc = wt8_scale(sg, row_lo, nun, 0, c, N);                 // ahead of the first codes
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < DEP / 8; ++i) wq[i] = ldw8_nt(wp + min(obase + i, lasto) * 1024);
    __builtin_amdgcn_sched_barrier(0);
    const TileEpi epi0 = tile_epilogue_fetch(a, p.hd, grp, row_lo, wave == 0 ? 8 : 0, lane, kvpos);
    __builtin_amdgcn_sched_barrier(0);
    wt8_entry_wait();
    f4v aA = {0.f, 0.f, 0.f, 0.f}, aB = {0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < ngrp - 1; ++g) {                                   // all groups but the last: refill for group g + 1
      const int kb = tbase + g * DEP, kbn = kb + DEP, on = kbn >> 3;
#pragma unroll
      for (int j = 0; j < DEP / 2; ++j) {                                  // the fp32 kernel's pair j = k-steps (2j, 2j + 1) of the group
        const float4 wv = wt8_wide(wq[j >> 2][j & 3], sc);
        float4 xa = xr[2 * j], xb = xr[2 * j + 1];
        if (kb + 2 * j > last) { xa = make_float4(0.f, 0.f, 0.f, 0.f); xb = xa; }   // steps is even: a pair is in or out as a whole
        kpair1(wv, xa, xb, aA, aB);
        xr[2 * j] = ld4(xp + min(kbn + 2 * j, last) * xstep);
        xr[2 * j + 1] = ld4(xp + min(kbn + 2 * j + 1, last) * xstep);
        if ((j & 3) == 3) wq[j >> 2] = ldw8_nt(wp + min(on + (j >> 2), lasto) * 1024);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    {
      const int kb = tbase + (ngrp - 1) * DEP;
#pragma unroll
      for (int j = 0; j < DEP / 2; ++j) {
        const float4 wv = wt8_wide(wq[j >> 2][j & 3], sc);
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
  constexpr int NL = DEP / 4;                     // weight loads per group
  wt8_v4u w[NL];
#pragma unroll
  for (int i = 0; i < DEP; ++i) xr[i] = ld4(xp + min(tbase + i, last) * xstep);
  __builtin_amdgcn_sched_barrier(0);
  float sc = wt8_scale(sg, row_lo, nun, 0, c, N);                         // ahead of the tile's first codes
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < NL; ++i) w[i] = ldw8_nt(wp + wt8_off(obase, i, lasto));
  __builtin_amdgcn_sched_barrier(0);
  const bool epi_mine = wave < ntile;
  const TileEpi epi0 = tile_epilogue_fetch(a, p.hd, grp, row_lo + wave * 16, epi_mine ? tile_rows_of(wave, nun) : 0, lane, kvpos);
  __builtin_amdgcn_sched_barrier(0);
  const int total = ntile * ngrp;
  wt8_entry_wait();
  f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  int tile = 0, kg = 0;
  for (int g = 0; g < total - 1; ++g) {
    // group g = (tile, kg); the refills fetch group g + 1, behind the scale of ITS tile (every group asks: a cached dword, no branch)
    int tile_n = tile, kg_n = kg + 1;
    if (kg_n == ngrp) { kg_n = 0; tile_n = tile + 1; }
    const uint8_t* wn = (tile_n == tile) ? wp : wt8_ptr(wbase, row_lo, nun, tile_n, c, ks, K);
    const float sn = wt8_scale(sg, row_lo, nun, tile_n, c, N);
    __builtin_amdgcn_sched_barrier(0);
    const int kb = tbase + kg * DEP, kbn = tbase + kg_n * DEP, on = kbn >> 3;
#pragma unroll
    for (int t = 0; t < DEP; ++t) {
      const int m = 2 * (t >> 3) + (t & 1), h = (t >> 1) & 3;
      const float4 wv = wt8_wide(w[m][h], sc);
      float4 xv = xr[t];
      if (kb + t > last) xv = make_float4(0.f, 0.f, 0.f, 0.f);           // uniform: k-steps past the end of K contribute nothing
      kstep1(wv, xv, a0, a1);
      xr[t] = ld4(xp + min(kbn + t, last) * xstep);
      if (h == 3) w[m] = ldw8_nt(wn + wt8_off(on, m, lasto));
      __builtin_amdgcn_sched_barrier(0);
    }
    if (kg_n == 0) {                                                      // uniform: tile finished
      part[tile][wave][lane] = a0 + a1;
      a0 = (f4v){0.f, 0.f, 0.f, 0.f};
      a1 = (f4v){0.f, 0.f, 0.f, 0.f};
    }
    tile = tile_n; kg = kg_n; wp = wn; sc = sn;
  }
  {
    const int kb = tbase + kg * DEP;
#pragma unroll
    for (int t = 0; t < DEP; ++t) {
      const int m = 2 * (t >> 3) + (t & 1), h = (t >> 1) & 3;
      const float4 wv = wt8_wide(w[m][h], sc);
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

// the packed kernels' contract: the check and the plan of ssrhip_gemv_mfma_launch's rows-per-workgroup kernels, with whole octets of K
// (SSRHIP_GEMVM_V=1, the per-tile kernel of round 1, has no packed form)
int wt8_qualify(const ssrhip_gemv_args* a, RowsPlan* pl) {
  return gemv_wt_qualify(a, "ssrhip_gemv_wt8", 5, 16, 4096, /*ln_keeps_x=*/true, /*v1_refuses=*/true, pl, /*k_mult=*/128);
}

}  // namespace

extern "C" int ssrhip_gemv_wt8_applicable(const ssrhip_gemv_args* a) {
  if (!a) return 0;
  RowsPlan pl;
  return wt8_qualify(a, &pl) == 0 ? 1 : 0;
}

extern "C" int ssrhip_gemv_wt8(const ssrhip_gemv_args* a, const uint8_t* Wt8, const float* scale, ssrhip_stream_t stream) {
  SSR_REQUIRE(a && Wt8 && scale, "ssrhip_gemv_wt8: null argument");
  RowsPlan pl;
  if (int rc = wt8_qualify(a, &pl)) return rc;
  const GemvWt8 q = {pl.r, Wt8, scale};
  hipStream_t s = (hipStream_t)stream;
  const GemvR& r = pl.r;
  const bool ln = a->pro == SSRHIP_PRO_LAYERNORM;
  const bool x16 = r.spw == 16;                          // (x in registers) 16 k-steps of it per wave: K <= 2048
  dim3 grid(r.wgs, a->groups), block(r.nw * 64);
  // the dispatch of ssrhip_gemv_wt16 without its all-at-entry arm
  if (!pl.xreg && pl.pair) hipLaunchKernelGGL(wt8_stream_kernel<true>, grid, block, 0, s, q);
  else if (!pl.xreg) hipLaunchKernelGGL(wt8_stream_kernel<false>, grid, block, 0, s, q);
  else if (pl.pair && !ln && x16) hipLaunchKernelGGL((wt8_xreg_kernel<SSRHIP_PRO_NONE, 16, true>), grid, block, 0, s, q);
  else if (ln && x16) hipLaunchKernelGGL((wt8_xreg_kernel<SSRHIP_PRO_LAYERNORM, 16, false>), grid, block, 0, s, q);
  else if (ln) hipLaunchKernelGGL((wt8_xreg_kernel<SSRHIP_PRO_LAYERNORM, 32, false>), grid, block, 0, s, q);
  else if (x16) hipLaunchKernelGGL((wt8_xreg_kernel<SSRHIP_PRO_NONE, 16, false>), grid, block, 0, s, q);
  else hipLaunchKernelGGL((wt8_xreg_kernel<SSRHIP_PRO_NONE, 32, false>), grid, block, 0, s, q);
  SSR_LAUNCH_CHECK();
  return 0;
}
