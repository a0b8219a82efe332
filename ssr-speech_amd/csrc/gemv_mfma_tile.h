// gemv_mfma_tile.h — pieces shared by the matrix-core GEMV kernels (gemv_mfma.hip: 5..16 rows, gemv_mfma32.hip: 17..32 rows, and their
// bf16 weight streams gemv_mfma_w16.hip / gemv_mfma32_w16.hip, and the e4m3 stream gemv_mfma_w8.hip): the 16x16x4 fp32 MFMA, the k-slot reduction, the per-lane weight pointer of
// a tile and the split tile epilogue; the pieces of the rows-per-workgroup kernels (LayerNorm on register-resident x, the MFMA groups of a
// k-step and of a k-step pair, the pair form's merge tail) for one panel and for two; the loads and the widening of the packed bf16 layout;
// and, for the host, the argument check and the launch plan of those kernels and the qualifier of the two bf16 launchers.
#pragma once
#include "common.h"

// The two environment knobs of the rows-per-workgroup launch plan, read once per process for both launchers
struct ssr_rows_knobs {
  int wpc;       // tuning knob: 512-thread workgroups per CU (1..4, default 1)
  bool nopair;   // A/B knob: 8-row tiles with duplicated rows instead of k-step pairs
};
inline const ssr_rows_knobs& ssr_rows_knobs_get() {
  static const ssr_rows_knobs k = [] {
    const char* w = getenv("SSRHIP_GEMVM_WPC");
    return ssr_rows_knobs{(w && atoi(w) >= 1 && atoi(w) <= 4) ? atoi(w) : 1, getenv("SSRHIP_GEMVM_NOPAIR") != nullptr};
  }();
  return k;
}

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

// sum over the 4 lanes that share lane%16 (the 4 k-slots of one batch column)
__device__ __forceinline__ float kslot_sum(float v) {
  v += xor16_f(v);
  v += xor32_f(v);
  return v;
}

// Epilogue of one 16x16 output tile: this lane holds rows r0 = row0 + 4*(lane/16) .. r0+3 of batch column c = lane%16
// (only the first `tile_rows` rows of the tile are real: 16, or 8 when the tile's rows 8..15 duplicate 0..7).
// Split in two so that everything the epilogue has to FETCH — bias, the residual, and for the QKV launch the cache address
// (kv_pos -> page table -> pool: two dependent loads) — is requested before the weight loop and has long arrived when the
// last MFMA retires; otherwise that latency chain (1-2 us) sits in the tail of every launch with the HBM idle.
struct TileEpi {
  float* dst;
  float bias[4], res[4];
  int nvalid;        // 0: this lane stores nothing
  int kv_which, kv_cc, kv_pos, kv_page;   // QKV launch, K / V rows (kv_which = 1 | 2): dst is resolved in tile_epilogue_finish
};

// the QKV launch: K / V rows go to the paged cache, as fp32 (QKV_APPEND) or as rounded 2-byte entries (QKV_APPEND16)
__host__ __device__ __forceinline__ bool epi_appends(int epi) { return epi == SSRHIP_EPI_QKV_APPEND || epi == SSRHIP_EPI_QKV_APPEND16; }

// kv_pos of this lane's batch column for the QKV launch (0 otherwise): request it BEFORE the x / W loads (see tile_epilogue_fetch)
__device__ __forceinline__ int tile_kvpos(const ssrhip_gemv_args& a, int lane) {
  return epi_appends(a.epi) ? a.kv_pos[min(lane & 15, a.B - 1)] : 0;
}

__device__ __forceinline__ TileEpi tile_epilogue_fetch(const ssrhip_gemv_args& a, int hd, int grp, int row0, int tile_rows, int lane, int kvpos) {
  TileEpi e;
  const int c = lane & 15, ks = lane >> 4;
  const int N = a.N, K = a.K, B = a.B;
  const int r0 = row0 + ks * 4;
  e.dst = nullptr;
  e.kv_which = 0; e.kv_cc = 0; e.kv_pos = kvpos; e.kv_page = 0;
  // QKV launch: the address of a K / V row needs kv_pos[c] -> page table -> pool, two DEPENDENT loads. `kvpos` was requested by the caller
  // as the wave's OLDEST load (in front of x and W); the table entry is requested here by EVERY lane (branch-free: q rows and idle lanes
  // read a valid entry they never use) and first used in tile_epilogue_finish — so neither wait drains anything. Rounds 2-4 requested
  // both here, back to back, under the lane's row predicate: each was followed by `s_waitcnt vmcnt(0)`, i.e. every wave of the LN + QKV
  // launch drained its x slice and its first 16 weight loads — twice — before the LayerNorm could start; and a load under a divergent
  // branch makes hipcc wait for it (`vmcnt(0)`) in the OTHER branch before it may reuse the destination register (read off the ISA,
  // round 5; the 2-row kernel had the same disease, csrc/gemv.hip).
  if (epi_appends(a.epi)) e.kv_page = a.kv.table[(size_t)min(c, B - 1) * a.kv.max_pages + (kvpos / SSRHIP_PAGE)];
  const bool live = c < B && r0 < N && ks * 4 < tile_rows;
  e.nvalid = live ? min(4, N - r0) : 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { e.bias[j] = 0.f; e.res[j] = 0.f; }
  if (!live) return e;
  if (epi_appends(a.epi)) {
    const int D = K, which = r0 / D, cc = r0 % D;
    e.kv_which = which;                                                // 0: a q row (plain store below); 1 | 2: resolved in tile_epilogue_finish
    e.kv_cc = cc;
    e.dst = a.y + (size_t)c * a.y_stride + cc;
  } else if (a.y_tiled) {
    e.dst = a.y + (size_t)grp * N * 16 + SSRHIP_TILED(c, r0);
  } else {
    e.dst = a.y + (size_t)c * a.y_stride + (size_t)grp * N + r0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < e.nvalid) {
      if (a.bias) e.bias[j] = a.bias[(size_t)grp * N + r0 + j];
      if (a.epi == SSRHIP_EPI_RESIDUAL) e.res[j] = e.dst[j];
    }
  }
  return e;
}

__device__ __forceinline__ void tile_epilogue_finish(const ssrhip_gemv_args& a, const TileEpi& e0, f4v acc, int hd) {
  if (e0.nvalid == 0) return;
  TileEpi e = e0;
  const bool kv16 = e.kv_which && a.epi == SSRHIP_EPI_QKV_APPEND16;    // a K / V row of a cache of 2-byte entries: same element offset, half the bytes
  if (e.kv_which) {
    const size_t off = ((((size_t)e.kv_page * a.kv.n_layer + a.layer) * 2 + (e.kv_which - 1)) * a.kv.n_head + e.kv_cc / hd) * SSRHIP_PAGE + (e.kv_pos % SSRHIP_PAGE);
    const size_t el = off * a.kv.head_dim + (e.kv_cc % hd);
    e.dst = kv16 ? reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(a.kv.pool) + el) : a.kv.pool + el;
  }
  float v[4] = {acc[0], acc[1], acc[2], acc[3]};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] += e.bias[j];
    if (a.act == SSRHIP_ACT_RELU) v[j] = fmaxf(v[j], 0.f);
    else if (a.act == SSRHIP_ACT_GELU_ERF) v[j] = 0.5f * v[j] * (1.0f + erff(v[j] * 0.70710678118654752440f));
    v[j] = e.res[j] + v[j];                         // res == 0 unless EPI_RESIDUAL (same operand order as the fused add: y + v)
  }
  if (kv16) {     // N == 3K and K % 16 == 0: a K / V lane always holds four rows of one head, at an element offset that is a multiple of 4
    *reinterpret_cast<uint2*>(e.dst) = bf16x4_rne(v[0], v[1], v[2], v[3]);
    return;
  }
  if (e.nvalid == 4 && ((reinterpret_cast<size_t>(e.dst) & 15) == 0)) {
    *reinterpret_cast<float4*>(e.dst) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < e.nvalid) e.dst[j] = v[j];
  }
}

__device__ __forceinline__ void tile_epilogue(const ssrhip_gemv_args& a, int hd, int grp, int row0, int tile_rows, int lane, f4v acc) {
  const TileEpi e = tile_epilogue_fetch(a, hd, grp, row0, tile_rows, lane, tile_kvpos(a, lane));
  tile_epilogue_finish(a, e, acc, hd);
}

__device__ __forceinline__ f4v mfma4(float a, float b, f4v c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// per-lane pointer to (row of this lane in tile `tile`, k-slot of this lane) of the weight matrix
__device__ __forceinline__ const float* tile_wptr(const float* wbase, int row_lo, int nun, int tile, int c, int ks, int N, int K, int w_tiled) {
  const int rows = (2 * tile + 1 < nun) ? 16 : 8;
  const int rr = row_lo + tile * 16 + (c & (rows - 1));
  if (w_tiled) return wbase + (size_t)(rr >> 3) * 8 * K + (ks * 8 + (rr & 7)) * 4;   // streaming order: see SSRHIP_WTILED_INDEX (units are zero-padded)
  return wbase + (size_t)min(rr, N - 1) * K + ks * 4;
}

// ---- pieces of the rows-per-workgroup kernels, one 16-column panel (5..16 rows: gemv_mfma.hip and its bf16 stream gemv_mfma_w16.hip) ----

// rows of tile `tile` of a workgroup that owns `nun` 8-row units: two units to a 16-row tile, an odd last unit as an 8-row tile
__device__ __forceinline__ int tile_rows_of(int tile, int nun) { return (2 * tile + 1 < nun) ? 16 : 8; }

// one k-step of a 16-row tile: two accumulators in turn, so that consecutive MFMAs do not depend on each other
__device__ __forceinline__ void kstep1(const float4 wv, const float4 xv, f4v& a0, f4v& a1) {
  a0 = mfma4(wv.x, xv.x, a0);
  a1 = mfma4(wv.y, xv.y, a1);
  a0 = mfma4(wv.z, xv.z, a0);
  a1 = mfma4(wv.w, xv.w, a1);
}

// one k-step PAIR (see gemv_rows_xreg_kernel's PAIR): lanes c < 8 hold the weights of k-step 2i, lanes c >= 8 those of 2i + 1 for the same
// 8 rows; the MFMAs against xa = x[2i] are right in tile rows 0..7 (aA), those against xb = x[2i + 1] in rows 8..15 (aB)
__device__ __forceinline__ void kpair1(const float4 wv, const float4 xa, const float4 xb, f4v& aA, f4v& aB) {
  aA = mfma4(wv.x, xa.x, aA);
  aB = mfma4(wv.x, xb.x, aB);
  aA = mfma4(wv.y, xa.y, aA);
  aB = mfma4(wv.y, xb.y, aB);
  aA = mfma4(wv.z, xa.z, aA);
  aB = mfma4(wv.z, xb.z, aB);
  aA = mfma4(wv.w, xa.w, aA);
  aB = mfma4(wv.w, xb.w, aB);
}

__device__ __forceinline__ f4v pair_fold(f4v aA, f4v aB) {
  f4v acc;
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = aA[e] + xor32_f(aB[e]);          // rows 0..7 (lanes < 32) = own rows + rows 8..15 of lane + 32
  return acc;
}

// The merge tail of the k-step-pair form (one 8-row unit per workgroup), behind the barrier that completes part[wave][lane]: wave 0 adds
// the K-slices of the nw waves in wave order (deterministic) and finishes on the epilogue operands `e` it fetched at entry
__device__ __forceinline__ void merge_pair(const ssrhip_gemv_args& a, const f4v (&part)[8][64], int nw, int hd, const TileEpi& e, int wave, int lane) {
  if (wave != 0) return;
  f4v sum = part[0][lane];
  for (int v = 1; v < nw; ++v) sum += part[v][lane];
  tile_epilogue_finish(a, e, sum, hd);
}

// ---- two 16-column panels per launch (17..32 rows): gemv_mfma32.hip and its bf16 stream gemv_mfma32_w16.hip ----

// The launch seen from one 16-column panel: panel 1 is rows 16..B-1 as a (B-16)-row launch, so the 16-row tile epilogue applies unchanged.
__device__ __forceinline__ ssrhip_gemv_args panel_args(const ssrhip_gemv_args& a, int p) {
  ssrhip_gemv_args q = a;
  if (p == 0) { q.B = 16; return q; }
  q.B = a.B - 16;
  q.y = a.y + (a.y_tiled ? (size_t)16 * a.N * a.groups : (size_t)16 * a.y_stride);
  if (a.kv_pos) q.kv_pos = a.kv_pos + 16;
  if (a.kv.table) q.kv.table = a.kv.table + (size_t)16 * a.kv.max_pages;
  return q;
}

// per-lane x pointer of panel p at k-step 0 (tiled: one contiguous KiB per wave instruction per k-step; row-major: row clamped to B-1)
__device__ __forceinline__ const float* panel_xptr(const ssrhip_gemv_args& a, int grp, int p, int c, int ks) {
  if (a.x_tiled) return a.x + (size_t)p * 16 * a.K * a.groups + (size_t)grp * a.K * 16 + (unsigned)(ks * 16 + c) * 4;
  return a.x + (size_t)grp * a.K + (size_t)min(16 * p + c, a.B - 1) * a.x_stride + ks * 4;
}

// two-pass LayerNorm statistics of one panel's wave slice (the 16-row kernels call it for their one panel)
template <int SPWX>
__device__ __forceinline__ void ln_slice(const float4 (&xr)[SPWX], int tbase, int last, float* mw_out, float* q_out) {
  const int nval = max(0, min(SPWX, last + 1 - tbase)) * 16;
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < SPWX; ++t) s += (xr[t].x + xr[t].y) + (xr[t].z + xr[t].w);
  s = kslot_sum(s);
  const float mw = nval > 0 ? s / (float)nval : 0.f;
  float q = 0.f;
#pragma unroll
  for (int t = 0; t < SPWX; ++t) {
    if (tbase + t <= last) {
      const float dx = xr[t].x - mw, dy = xr[t].y - mw, dz = xr[t].z - mw, dw = xr[t].w - mw;
      q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  }
  *mw_out = mw;
  *q_out = kslot_sum(q);
}

template <int SPWX>
__device__ __forceinline__ void ln_apply(float4 (&xr)[SPWX], const float (&red)[2][8][16], int nw, int c, int tbase, int last, int K, float eps) {
  float mean = 0.f;
  for (int v = 0; v < nw; ++v) mean += red[0][v][c] * (float)(max(0, min(SPWX, last + 1 - v * SPWX)) * 16);
  mean /= (float)K;
  float var = 0.f;
  for (int v = 0; v < nw; ++v) {
    const float d = red[0][v][c] - mean;
    var += red[1][v][c] + (float)(max(0, min(SPWX, last + 1 - v * SPWX)) * 16) * d * d;
  }
  var /= (float)K;
  const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
  for (int t = 0; t < SPWX; ++t) {
    if (tbase + t <= last) {
      xr[t].x = (xr[t].x - mean) * rstd;
      xr[t].y = (xr[t].y - mean) * rstd;
      xr[t].z = (xr[t].z - mean) * rstd;
      xr[t].w = (xr[t].w - mean) * rstd;
    }
  }
}

// one k-step against both panels: the a0 / a1 interleave of the 16-row kernels, once per panel, on the same weight fragment
__device__ __forceinline__ void kstep2(const float4 wv, const float4 xa, const float4 xb, f4v& a0, f4v& a1, f4v& b0, f4v& b1) {
  a0 = mfma4(wv.x, xa.x, a0);
  a1 = mfma4(wv.y, xa.y, a1);
  b0 = mfma4(wv.x, xb.x, b0);
  b1 = mfma4(wv.y, xb.y, b1);
  a0 = mfma4(wv.z, xa.z, a0);
  a1 = mfma4(wv.w, xa.w, a1);
  b0 = mfma4(wv.z, xb.z, b0);
  b1 = mfma4(wv.w, xb.w, b1);
}

// one k-step PAIR against both panels (k-step-pair form, see gemv_rows_xreg_kernel's PAIR): per panel the aA / aB order of the 16-row kernel
__device__ __forceinline__ void kpair2(const float4 wv, const float4 xa0, const float4 xb0, const float4 xa1, const float4 xb1,
                                       f4v& aA0, f4v& aB0, f4v& aA1, f4v& aB1) {
  aA0 = mfma4(wv.x, xa0.x, aA0);
  aB0 = mfma4(wv.x, xb0.x, aB0);
  aA1 = mfma4(wv.x, xa1.x, aA1);
  aB1 = mfma4(wv.x, xb1.x, aB1);
  aA0 = mfma4(wv.y, xa0.y, aA0);
  aB0 = mfma4(wv.y, xb0.y, aB0);
  aA1 = mfma4(wv.y, xa1.y, aA1);
  aB1 = mfma4(wv.y, xb1.y, aB1);
  aA0 = mfma4(wv.z, xa0.z, aA0);
  aB0 = mfma4(wv.z, xb0.z, aB0);
  aA1 = mfma4(wv.z, xa1.z, aA1);
  aB1 = mfma4(wv.z, xb1.z, aB1);
  aA0 = mfma4(wv.w, xa0.w, aA0);
  aB0 = mfma4(wv.w, xb0.w, aB0);
  aA1 = mfma4(wv.w, xa1.w, aA1);
  aB1 = mfma4(wv.w, xb1.w, aB1);
}

// merge_pair for two panels: both panels' sums in one wave-order loop, then panel 0's epilogue, then panel 1's
__device__ __forceinline__ void merge_pair2(const ssrhip_gemv_args& a0p, const ssrhip_gemv_args& a1p, const f4v (&part0)[8][64], const f4v (&part1)[8][64],
                                            int nw, int hd, const TileEpi& e0, const TileEpi& e1, int wave, int lane) {
  if (wave != 0) return;
  f4v s0 = part0[0][lane], s1 = part1[0][lane];
  for (int v = 1; v < nw; ++v) { s0 += part0[v][lane]; s1 += part1[v][lane]; }
  tile_epilogue_finish(a0p, e0, s0, hd);
  tile_epilogue_finish(a1p, e1, s1, hd);
}

// ---- host: one argument check and one launch plan for the rows-per-workgroup kernels at 5..32 rows ----

// Parameter of the rows-per-workgroup kernels (gemv_rows_*_kernel at 5..16 rows, gemv_rows32_* at 17..32)
struct GemvR {
  ssrhip_gemv_args a;
  int nw;       // waves per workgroup (K split)
  int steps;    // K / 16 MFMA k-steps in total
  int spw;      // k-steps per wave (stream kernel: multiple of 16)
  int units;    // ceil(N / 8) 8-row units per group
  int wgs;      // workgroups per group (gridDim.x)
  int hd;
};

constexpr int MAXT = 4;     // 16-row tiles per workgroup (LDS: MAXT x 8 waves x 1 KiB of partial sums, per column panel)

// ---- packed bf16 weights (include/ssrhip.h SSRHIP_WT16_INDEX): gemv_mfma_w16.hip (5..16 rows) and gemv_mfma32_w16.hip (17..32 rows) ----

typedef unsigned wt16_v4u __attribute__((ext_vector_type(4)));

struct GemvWt16 {
  GemvR r;               // the fp32 launch's parameter, from the same plan
  const uint16_t* w16;   // [groups][units * 8][K] in SSRHIP_WT16_INDEX order
};

// 8 packed bf16 of a streamed-once weight block: non-temporal 16-byte load (global_load_dwordx4 ... nt)
__device__ __forceinline__ wt16_v4u ldw_nt(const uint16_t* p) { return __builtin_nontemporal_load(reinterpret_cast<const wt16_v4u*>(p)); }

// the float4 of one k-step: half g of a 16-byte piece (g = 0: dwords 0, 1; g = 1: dwords 2, 3); element 2m in the low half of a dword
__device__ __forceinline__ float4 wt16_widen(const wt16_v4u u, int g) {
  const unsigned d0 = g ? u.z : u.x, d1 = g ? u.w : u.y;
  return make_float4(__uint_as_float(d0 << 16), __uint_as_float(d0 & 0xffff0000u), __uint_as_float(d1 << 16), __uint_as_float(d1 & 0xffff0000u));
}

// per-lane pointer to (row of this lane in tile `tile`, k-slot of this lane) of the packed matrix: block (unit, quad 0, h = 0)
__device__ __forceinline__ const uint16_t* wt16_ptr(const uint16_t* wbase, int row_lo, int nun, int tile, int c, int ks, int K) {
  const int rows = (2 * tile + 1 < nun) ? 16 : 8;
  const int rr = row_lo + tile * 16 + (c & (rows - 1));
  return wbase + (size_t)(rr >> 3) * 8 * K + (ks * 8 + (rr & 7)) * 8;     // units are zero-padded: no row clamp
}

// uint16 offset of load m (m = 2 * quad + h, counted from the wave's first quad `qbase`) behind wt16_ptr; quads past the end are clamped
__device__ __forceinline__ int wt16_off(int qbase, int m, int lastq) { return (min(qbase + (m >> 1), lastq) * 2 + (m & 1)) * 256; }

// What ssrhip_gemv has not checked when it hands 5..32 rows to a matrix-core launcher. Runs before the first HIP runtime call.
// [b_lo, b_hi]: the rows the launcher's kernels take; ln_kmax: the largest K whose LayerNorm prologue they fuse.
inline int gemv_rows_check(const ssrhip_gemv_args* a, int b_lo, int b_hi, int ln_kmax) {
  SSR_REQUIRE(a->B >= b_lo && a->B <= b_hi, "ssrhip_gemv: B=%d rows not in {1,2,4} or 5..32", a->B);
  SSR_REQUIRE(a->K % 16 == 0, "ssrhip_gemv (B>4): K=%d must be a multiple of 16", a->K);
  SSR_REQUIRE(a->pro == SSRHIP_PRO_NONE || a->pro == SSRHIP_PRO_LAYERNORM,
              "ssrhip_gemv (B>4): the split-KV combine prologue is not fused; run ssrhip_attn_combine first");
  SSR_REQUIRE(a->x, "ssrhip_gemv: x is null");
  SSR_REQUIRE(!a->y_tiled || (a->N % 4 == 0 && !epi_appends(a->epi)), "ssrhip_gemv: tiled y needs N %% 4 == 0 and is not available for the q output");
  if (a->pro == SSRHIP_PRO_LAYERNORM) {
    SSR_REQUIRE(a->K <= ln_kmax, "ssrhip_gemv (B=%d): LayerNorm prologue needs K=%d <= %d", a->B, a->K, ln_kmax);
    SSR_REQUIRE(!a->ln_w && !a->ln_b, "ssrhip_gemv (B>4): LayerNorm gamma/beta must be folded into W/bias (ln_w == ln_b == NULL)");
  }
  SSR_REQUIRE(a->epi >= SSRHIP_EPI_STORE && a->epi <= SSRHIP_EPI_QKV_APPEND16, "ssrhip_gemv: unknown epilogue %d", a->epi);
  if (epi_appends(a->epi)) {
    SSR_REQUIRE(a->N == 3 * a->K && a->groups == 1 && a->kv.pool && a->kv.table && a->kv_pos && a->kv.head_dim > 0 && a->kv.head_dim % 4 == 0,
                "ssrhip_gemv: QKV epilogue needs N==3K and a kv cache");
  }
  return 0;
}

struct RowsPlan {
  GemvR r;      // the kernel parameter: grid = (r.wgs, a.groups), block = r.nw * 64
  bool xreg;    // every wave keeps its x slice in registers (r.spw = 16 or 32 k-steps of it); else x is streamed beside W
  bool pair;    // k-step pairs per weight load: it changes the accumulation order, so a row must get the same answer at every row count
};

// The plan is a function of the SHAPE alone (N, K, groups, prologue, weight layout), never of B: that is what makes row b of a 32-row
// launch bit-identical to row b of a 16-row launch (tests/test_gpu_rows32.py). The one thing that differs between the two row counts:
// ln_keeps_x — at 5..16 rows a LayerNorm launch keeps x in registers up to K = 4096 (32 k-steps per wave); at 17..32 rows two panels of
// 32 k-steps do not fit, the launcher refuses LayerNorm beyond K = 2048 and x is in registers for K <= 2048 only.
inline int gemv_rows_plan(const ssrhip_gemv_args* a, bool ln_keeps_x, int num_cu, const ssr_rows_knobs& knobs, RowsPlan* out) {
  GemvR& r = out->r;
  r.a = *a;
  r.steps = a->K / 16;
  r.hd = a->kv.head_dim > 0 ? a->kv.head_dim : 1;
  r.units = (a->N + 7) / 8;
  out->xreg = a->K <= 2048 || (ln_keeps_x && a->pro == SSRHIP_PRO_LAYERNORM);
  if (out->xreg) {
    r.spw = a->K <= 2048 ? 16 : 32;                      // k-steps of x a wave keeps in registers
    r.nw = (r.steps + r.spw - 1) / r.spw;
  } else {
    r.nw = 8;
    r.spw = ((r.steps + 7) / 8 + 15) / 16 * 16;
  }
  // one 512-thread workgroup per CU (two when the K split leaves it <= 4 waves), all groups together
  int target = num_cu * knobs.wpc * (r.nw <= 4 ? 2 : 1) / a->groups;
  if (target < 1) target = 1;
  r.wgs = r.units < target ? r.units : target;
  const int need = (r.units + 2 * MAXT - 1) / (2 * MAXT);   // LDS holds MAXT tiles of partials per workgroup
  if (r.wgs < need) r.wgs = need;
  SSR_REQUIRE(r.wgs <= 65535 * 32, "ssrhip_gemv (B>4): N too large");
  // every workgroup owns exactly one 8-row unit (out-proj, FFN2) and the weights are in streaming order: k-step pairs per load
  out->pair = a->w_tiled && r.units <= r.wgs && r.steps % 2 == 0 && !knobs.nopair;
  return 0;
}

// The packed weight streams (bf16: ssrhip_gemv_wt16 at 5..16 rows, ssrhip_gemv_wt32 at 17..32; e4m3: ssrhip_gemv_wt8 at 5..16): does `a` take the packed kernels?
// 0: it qualifies (then *pl is its launch plan), 1: it does not, < 0: contract error. No HIP call before the answer is 0.
// `who` is the entry point's name in the error texts; [b_lo, b_hi], ln_kmax, ln_keeps_x as in gemv_rows_check / gemv_rows_plan — the
// check and the plan of the fp32 launcher at the same row count: the same refusals, the same grid, waves, K slices and pair decision.
// v1_refuses: SSRHIP_GEMVM_V=1 (the per-tile kernel of 5..16 rows, which has no bf16 form) makes the answer 1.
// k_mult: the packed layout's block of K (64 floats = a quad of k-steps for bf16; the e4m3 stream of gemv_mfma_w8.hip passes 128, an octet).
inline int gemv_wt_qualify(const ssrhip_gemv_args* a, const char* who, int b_lo, int b_hi, int ln_kmax, bool ln_keeps_x, bool v1_refuses, RowsPlan* pl,
                           int k_mult = 64) {
  SSR_REQUIRE(a && a->W && a->y, "%s: null argument", who);
  SSR_REQUIRE(a->N > 0 && a->groups >= 1 && a->K > 0, "%s: bad N/K/groups", who);
  if (a->B < b_lo || a->B > b_hi || a->w_tiled != 1 || a->K % k_mult != 0) return 1;
  if (v1_refuses) {
    static const bool v1 = [] { const char* e = getenv("SSRHIP_GEMVM_V"); return e && atoi(e) == 1; }();
    if (v1) return 1;
  }
  if (int rc = gemv_rows_check(a, b_lo, b_hi, ln_kmax)) return rc;
  return gemv_rows_plan(a, ln_keeps_x, ssr_num_cu(), ssr_rows_knobs_get(), pl);
}

}  // namespace
