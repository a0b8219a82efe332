// gemv_mfma_tile.h — pieces shared by the matrix-core GEMV kernels (gemv_mfma.hip: 5..16 rows, gemv_mfma32.hip: 17..32 rows):
// the 16x16x4 fp32 MFMA, the k-slot reduction, the per-lane weight pointer of a tile and the split tile epilogue.
#pragma once
#include "common.h"

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

}  // namespace
