// gemv_mfma_tile.h — pieces shared by the matrix-core GEMV kernels (gemv_mfma.hip: 5..16 rows, gemv_mfma32.hip: 17..32 rows):
// the 16x16x4 fp32 MFMA, the k-slot reduction, the per-lane weight pointer of a tile and the split tile epilogue; and, for the host, the
// argument check and the launch plan of the rows-per-workgroup kernels, which both launchers take from here.
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

// kv_pos of this lane's batch column for the QKV launch (0 otherwise): request it BEFORE the x / W loads (see tile_epilogue_fetch)
__device__ __forceinline__ int tile_kvpos(const ssrhip_gemv_args& a, int lane) {
  return (a.epi == SSRHIP_EPI_QKV_APPEND) ? a.kv_pos[min(lane & 15, a.B - 1)] : 0;
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
  if (a.epi == SSRHIP_EPI_QKV_APPEND) e.kv_page = a.kv.table[(size_t)min(c, B - 1) * a.kv.max_pages + (kvpos / SSRHIP_PAGE)];
  const bool live = c < B && r0 < N && ks * 4 < tile_rows;
  e.nvalid = live ? min(4, N - r0) : 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { e.bias[j] = 0.f; e.res[j] = 0.f; }
  if (!live) return e;
  if (a.epi == SSRHIP_EPI_QKV_APPEND) {
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
  if (e.kv_which) {
    const size_t off = ((((size_t)e.kv_page * a.kv.n_layer + a.layer) * 2 + (e.kv_which - 1)) * a.kv.n_head + e.kv_cc / hd) * SSRHIP_PAGE + (e.kv_pos % SSRHIP_PAGE);
    e.dst = a.kv.pool + off * a.kv.head_dim + (e.kv_cc % hd);
  }
  float v[4] = {acc[0], acc[1], acc[2], acc[3]};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] += e.bias[j];
    if (a.act == SSRHIP_ACT_RELU) v[j] = fmaxf(v[j], 0.f);
    else if (a.act == SSRHIP_ACT_GELU_ERF) v[j] = 0.5f * v[j] * (1.0f + erff(v[j] * 0.70710678118654752440f));
    v[j] = e.res[j] + v[j];                         // res == 0 unless EPI_RESIDUAL (same operand order as the fused add: y + v)
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

// What ssrhip_gemv has not checked when it hands 5..32 rows to a matrix-core launcher. Runs before the first HIP runtime call.
// [b_lo, b_hi]: the rows the launcher's kernels take; ln_kmax: the largest K whose LayerNorm prologue they fuse.
inline int gemv_rows_check(const ssrhip_gemv_args* a, int b_lo, int b_hi, int ln_kmax) {
  SSR_REQUIRE(a->B >= b_lo && a->B <= b_hi, "ssrhip_gemv: B=%d rows not in {1,2,4} or 5..32", a->B);
  SSR_REQUIRE(a->K % 16 == 0, "ssrhip_gemv (B>4): K=%d must be a multiple of 16", a->K);
  SSR_REQUIRE(a->pro == SSRHIP_PRO_NONE || a->pro == SSRHIP_PRO_LAYERNORM,
              "ssrhip_gemv (B>4): the split-KV combine prologue is not fused; run ssrhip_attn_combine first");
  SSR_REQUIRE(a->x, "ssrhip_gemv: x is null");
  SSR_REQUIRE(!a->y_tiled || (a->N % 4 == 0 && a->epi != SSRHIP_EPI_QKV_APPEND), "ssrhip_gemv: tiled y needs N %% 4 == 0 and is not available for the q output");
  if (a->pro == SSRHIP_PRO_LAYERNORM) {
    SSR_REQUIRE(a->K <= ln_kmax, "ssrhip_gemv (B=%d): LayerNorm prologue needs K=%d <= %d", a->B, a->K, ln_kmax);
    SSR_REQUIRE(!a->ln_w && !a->ln_b, "ssrhip_gemv (B>4): LayerNorm gamma/beta must be folded into W/bias (ln_w == ln_b == NULL)");
  }
  if (a->epi == SSRHIP_EPI_QKV_APPEND) {
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

}  // namespace
