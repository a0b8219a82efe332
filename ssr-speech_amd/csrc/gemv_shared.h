// gemv_shared.h — what the <= 4-row weight-streaming GEMV kernels of gemv.hip (fp32 weights) and gemv_w16.hip (packed bf16 weights) have
// in common: the launch descriptor, the host plan and argument check of the segment path, the geometry of the segment kernels, their
// LayerNorm prologue, the per-unit reduction, the per-row epilogue and the late loads of the merge prologue.
// One definition, so that the two translation units plan a launch alike and finish a row with the same operations in the same order
// (bit-identical results). What differs stays in the kernels: the streaming loops and weight rings (fp32 float4 / packed 16-byte pieces).
#pragma once
#include "common.h"

namespace {

struct GemvK {
  ssrhip_gemv_args a;
  int nslice;     // waves cooperating on one row (K split), 1|2|4
  int slice_len;  // floats per slice (multiple of 4)
  int nch;        // float4 chunks per lane per slice (<= 8)
  int groups_x;   // wave-groups along N (= gridDim.x * 4/nslice)
  int hd;         // head_dim (QKV epilogue / combine prologue)
  int seg_shift;  // segment kernel: log2(K / 1024)
  int rows_max;   // segment kernel: most rows a workgroup owns (sizes the LDS partials)
  long long* prof;          // -DSSR_GEMV_PROFILE builds only (ssrhip_debug_gemv_prof): 8 wall_clock64 stamps per workgroup, or NULL
  int rows_per, rows_rem;   // segment / front kernels: N / groups_x and N % groups_x (workgroup b owns rows_per + (b < rows_rem) rows)
};

__device__ __forceinline__ float apply_act(float v, int act) {
  if (act == SSRHIP_ACT_RELU) return fmaxf(v, 0.f);
  if (act == SSRHIP_ACT_GELU_ERF) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
  return v;
}

// per-row epilogue operands requested together with the weight row (they sit on the tail of every row otherwise)
struct RowEpi { float bias, resid; };

__device__ __forceinline__ void finalize(const GemvK& p, int g, int n, int b, float v, const RowEpi& e, float* const (&kvb)[2]) {
  const ssrhip_gemv_args& a = p.a;
  v += e.bias;
  v = apply_act(v, a.act);
  if (a.epi == SSRHIP_EPI_STORE) {
    a.y[(size_t)b * a.y_stride + (size_t)g * a.N + n] = v;
  } else if (a.epi == SSRHIP_EPI_RESIDUAL) {
    a.y[(size_t)b * a.y_stride + (size_t)g * a.N + n] = e.resid + v;
  } else {  // QKV append: rows [0,D) -> q, [D,2D) -> k cache, [2D,3D) -> v cache (page bases resolved once per wave)
    const int D = a.K;
    const int which = n / D, c = n % D;
    if (which == 0) a.y[(size_t)b * a.y_stride + c] = v;
    else kvb[which - 1][(size_t)(c / p.hd) * SSRHIP_PAGE * p.hd + (c % p.hd)] = v;
  }
}

// K / V base addresses (head 0) of the cache position this step appends, for the batch row `bsel` of the calling thread. The chain
// kv_pos -> page table -> pool stays on the SCALAR path for all B rows side by side: the B position words, one wait, the B table words,
// one wait — two scalar round trips whatever B — and the thread's own row is picked with selects (a branch per row made hipcc walk the
// rows' chains one after the other inside exec-masked blocks: 2 B dependent round trips).
template <int B>
__device__ __forceinline__ void kv_append_bases(const ssrhip_gemv_args& a, int bsel, float* (&kvb)[2]) {
  int pos[B], page[B];
#pragma unroll
  for (int b = 0; b < B; ++b) pos[b] = a.kv_pos[b];
#pragma unroll
  for (int b = 0; b < B; ++b) page[b] = a.kv.table[(size_t)b * a.kv.max_pages + (pos[b] / SSRHIP_PAGE)];
  size_t ok = 0, ov = 0;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const size_t k0 = ((((size_t)page[b] * a.kv.n_layer + a.layer) * 2 + 0) * a.kv.n_head) * SSRHIP_PAGE + (pos[b] % SSRHIP_PAGE);
    const size_t v0 = ((((size_t)page[b] * a.kv.n_layer + a.layer) * 2 + 1) * a.kv.n_head) * SSRHIP_PAGE + (pos[b] % SSRHIP_PAGE);
    ok = (bsel == b) ? k0 : ok;
    ov = (bsel == b) ? v0 : ov;
  }
  kvb[0] = a.kv.pool + ok * a.kv.head_dim;
  kvb[1] = a.kv.pool + ov * a.kv.head_dim;
}

// Loads of the merge prologue's COLD path (contexts beyond the SEG_CS prefetched pages), hidden from hipcc's wait-count bookkeeping: load
// and wait in one asm statement. A compiler-visible load inside those loops made hipcc put `s_waitcnt vmcnt(0)` on the HOT path as well
// (the loops' pre-headers and the first use of a prefetched partial behind them): every out-projection drained its whole weight slice
// before the merge arithmetic, a barrier and an LDS round trip instead of under them (read off the ISA, round 5). The asm wait drains the
// queue too — but only when a late page exists.
__device__ __forceinline__ float4 ld4_late(const float* p) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  v4f v;
  asm volatile("global_load_dwordx4 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float2 ld2_late(const float* p) {
  typedef float v2f __attribute__((ext_vector_type(2)));
  v2f v;
  asm volatile("global_load_dwordx2 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
  return make_float2(v.x, v.y);
}
constexpr int SEG = 1024;            // floats per unit
constexpr int SEG_TH = 512, SEG_NW = 8;
template <int B> struct SegCS { static constexpr int v = (B <= 2) ? 6 : 2; };   // pages prefetched by the combine prologue (register budget: 128)


// ---- device pieces of the segment kernels. Every kernel calls them at the program point where its own copy used to stand: the order of
// the loads against the weight requests is part of the tuning. Each was taken over only where hipcc's registers, memory
// operations and wait counts stayed as they were (profiles/seg_gemv_refactor_ab.md); the split-KV merge prologue did not pass in any
// form and stays written out in its four kernels (gemv_seg_kernel, gemv_pair_merge_kernel, w16_seg_kernel, w16_pair_merge_kernel).

// bias / residual of the (row n, batch row b) a thread finalises: the wave's OLDEST loads (gemv_seg_kernel explains why)
__device__ __forceinline__ RowEpi seg_epi_fetch(const ssrhip_gemv_args& a, int g, int n, int b) {
  RowEpi e;
  e.bias = a.bias ? a.bias[(size_t)g * a.N + n] : 0.f;
  e.resid = (a.epi == SSRHIP_EPI_RESIDUAL) ? a.y[(size_t)b * a.y_stride + (size_t)g * a.N + n] : 0.f;
  return e;
}

// the wave's slice of x: segment `seg` of the B rows at x, x + stride, ... (global memory, or the LDS copy a prologue left)
template <int B, typename I>
__device__ __forceinline__ void seg_load_x(float4 (&xr)[B][4], const float* x, I stride, int seg, int lane) {
#pragma unroll
  for (int b = 0; b < B; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i) xr[b][i] = ld4(x + b * stride + seg * SEG + (i * 64 + lane) * 4);
}

// LayerNorm (gamma / beta folded into W / bias by the host) without staging x: a wave normalises its own segment in registers —
// per-segment two-pass statistics, exchanged through LDS (ONE barrier, in here), merged exactly (Chan)
template <int B>
__device__ __forceinline__ void seg_layernorm(float4 (&xr)[B][4], float* aux, int S, int K, float eps, int wave, int lane) {
  float m[B], q[B];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    float s0 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s0 += (xr[b][i].x + xr[b][i].y) + (xr[b][i].z + xr[b][i].w);
    m[b] = wave_sum(s0) * (1.0f / SEG);
    float q0 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float dx = xr[b][i].x - m[b], dy = xr[b][i].y - m[b], dz = xr[b][i].z - m[b], dw = xr[b][i].w - m[b];
      q0 += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    q[b] = wave_sum(q0);
    if (wave < S && lane == 0) { aux[(wave * B + b) * 2] = m[b]; aux[(wave * B + b) * 2 + 1] = q[b]; }   // wave w < S holds segment w
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < B; ++b) {
    float mean = 0.f, M2 = 0.f, dev = 0.f;
    for (int s2 = 0; s2 < S; ++s2) mean += aux[(s2 * B + b) * 2];
    mean /= (float)S;
    for (int s2 = 0; s2 < S; ++s2) { const float dm = aux[(s2 * B + b) * 2] - mean; M2 += aux[(s2 * B + b) * 2 + 1]; dev = fmaf(dm, dm, dev); }
    const float var = (M2 + (float)SEG * dev) / (float)K;
    const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      xr[b][i] = make_float4((xr[b][i].x - mean) * rstd, (xr[b][i].y - mean) * rstd, (xr[b][i].z - mean) * rstd, (xr[b][i].w - mean) * rstd);
  }
}

// one unit done: wave all-reduce per row, lane b keeps row b's sum and parks it in part[u][b] (u = local_row * S + seg)
template <int B>
__device__ __forceinline__ void seg_park(const float (&acc)[B][2], float* part, int u, int lane) {
  float mine = 0.f;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const float sum = wave_sum(acc[b][0] + acc[b][1]);
    if (lane == b) mine = sum;
  }
  if (lane < B) part[lane + u * B] = mine;                        // (written part[u * B + lane], hipcc gives gemv_segu_kernel<2, NONE, ..> one VGPR less)
}

// behind the barrier: thread (local row rfin, batch row bfin) adds the row's S segments in k order and applies the epilogue
template <int B>
__device__ __forceinline__ void seg_finish_row(const GemvK& p, int g, const float* part, int S, int rfin, int nfin, int bfin, const RowEpi& efin,
                                               float* const (&kvb)[2]) {
  float v = 0.f;
  for (int s2 = 0; s2 < S; ++s2) v += part[(rfin * S + s2) * B + bfin];
  finalize(p, g, nfin, bfin, v, efin, kvb);
}

// ---- host side: the launch plan of the segment path (no HIP call, no environment: a function of the arguments alone)

// the descriptor of a launch whose G workgroups (per group) split the N rows into contiguous blocks, S = K / 1024 segments per row
inline void seg_fill(GemvK* k, const ssrhip_gemv_args* a, int S, int G) {
  k->a = *a;
  k->nslice = S;
  k->slice_len = SEG;
  k->nch = 4;
  k->groups_x = G;
  k->hd = (a->kv.head_dim > 0) ? a->kv.head_dim : 1;
  k->seg_shift = (S == 1) ? 0 : (S == 2) ? 1 : (S == 4) ? 2 : 3;
  k->rows_max = (a->N + G - 1) / G;
  k->prof = nullptr;
  k->rows_per = a->N / G;
  k->rows_rem = a->N % G;
}

struct SegPlan {
  GemvK k; int G; size_t smem;                      // generic form (gemv_seg_kernel / w16_seg_kernel): grid (G, groups)
  int segu_nuw, segu_G1; size_t segu_smem;          // straight-line form (one workgroup per CU, segu_nuw units per wave): fits iff segu_nuw in {4,6,8};
};                                                  // whoever takes it re-fills the descriptor: seg_fill(&k, a, k.nslice, segu_G1)

// Does the segment path take `a` (B in {1,2,4}, checked by the caller), and with what geometry? `why` receives a refusal as text.
// combine_two_per_cu: two workgroups per CU behind the merge prologue too. By default that prologue runs at ONE: it makes EVERY workgroup
// read all the attention partials (~100 KB at 6 pages) — with two per CU that is 3x the CU's share of the weights through its 64 B/clk L2 port.
inline bool seg_plan(const ssrhip_gemv_args* a, int num_cu, bool combine_two_per_cu, SegPlan* out, const char** why) {
  auto no = [&](const char* w) { *why = w; return false; };
  const int B = a->B;
  if (a->K % SEG != 0) return no("K is not a multiple of 1024");
  const int S = a->K / SEG;
  if (S != 1 && S != 2 && S != 4 && S != 8) return no("K / 1024 not in {1, 2, 4, 8}");
  if (a->pro == SSRHIP_PRO_LAYERNORM && a->ln_w != nullptr) return no("LayerNorm gamma / beta not folded into the weights");
  const int H = a->kv.head_dim > 0 ? a->K / a->kv.head_dim : 0;
  if (a->pro == SSRHIP_PRO_ATTN_COMBINE && (a->K != 2048 || a->max_splits < 1 || a->groups != 1 || B * H > SEG_TH || a->kv.head_dim % 4 != 0))
    return no("split-KV merge prologue needs K = 2048, one group, B * H <= 512");
  int G = (2 * num_cu) / a->groups;                                // two resident workgroups per CU over all groups
  if (a->pro == SSRHIP_PRO_ATTN_COMBINE && !combine_two_per_cu) G = num_cu;
  if (G > a->N) G = a->N;                                          // fewer rows than workgroups: one row each
  if (G < 1) G = 1;
  if ((a->N + G - 1) / G * B > SEG_TH) return no("too many rows per workgroup");
  seg_fill(&out->k, a, S, G);
  out->G = G;
  size_t smem = (size_t)out->k.rows_max * S * B * sizeof(float);   // the parked partial sums, then the prologue's scratch
  if (a->pro == SSRHIP_PRO_LAYERNORM) smem += (size_t)S * B * 2 * sizeof(float);
  if (a->pro == SSRHIP_PRO_ATTN_COMBINE) smem += ((size_t)B * a->K + (size_t)B * H * a->max_splits) * sizeof(float);
  out->smem = (smem + 15) / 16 * 16;
  // one workgroup per CU, NUW units per wave as straight-line code, when the shape divides evenly
  const int G1 = num_cu / a->groups;
  out->segu_nuw = 0;
  out->segu_G1 = G1;
  out->segu_smem = 0;
  if (a->pro != SSRHIP_PRO_ATTN_COMBINE && G1 >= 1 && a->N % G1 == 0 && ((a->N / G1) * S) % SEG_NW == 0) {
    const int nuw = (a->N / G1) * S / SEG_NW;
    if (nuw == 4 || nuw == 6 || nuw == 8) {
      out->segu_nuw = nuw;
      out->segu_smem = (((size_t)(a->N / G1) * S * B + (size_t)S * B * 2) * sizeof(float) + 15) / 16 * 16;
    }
  }
  *why = "";
  return true;
}

// the contract of ssrhip_gemv / ssrhip_gemv_w16 for B in {1,2,4} rows, behind the callers' own null / N / K / groups / B tests
inline int gemv_small_check(const ssrhip_gemv_args* a, const char* who) {
  SSR_REQUIRE(a->epi != SSRHIP_EPI_QKV_APPEND16, "%s: the 2-byte KV append (EPI_QKV_APPEND16) exists for 5..32 rows only (B=%d)", who, a->B);
  SSR_REQUIRE(!a->x_tiled && !a->y_tiled && !a->w_tiled, "%s: the tiled activation / weight layouts are for 5..32 rows only", who);
  SSR_REQUIRE(a->pro != SSRHIP_PRO_ATTN_COMBINE || (a->kv.head_dim > 0 && a->K <= 2048 && a->B * (a->K / a->kv.head_dim) <= 256), "%s: combine prologue needs K <= 2048 and B*H <= 256", who);
  SSR_REQUIRE(a->K > 0 && a->K % 4 == 0 && a->K <= 8192, "%s: K=%d must be a multiple of 4, <= 8192", who, a->K);
  if (a->pro != SSRHIP_PRO_NONE) {
    SSR_REQUIRE(a->groups == 1 || a->pro == SSRHIP_PRO_LAYERNORM, "%s: combine prologue needs groups==1", who);
    if (a->pro == SSRHIP_PRO_LAYERNORM) SSR_REQUIRE(a->x && ((a->ln_w && a->ln_b) || (!a->ln_w && !a->ln_b)), "%s: LayerNorm prologue needs x and either both or none of ln_w/ln_b", who);
    if (a->pro == SSRHIP_PRO_ATTN_COMBINE) {
      SSR_REQUIRE(a->part_o && a->part_ml && a->row_len && a->kv.head_dim > 0 && a->K % a->kv.head_dim == 0 && a->kv.head_dim % 4 == 0,
                  "%s: combine prologue needs part_o, part_ml, row_len, kv.head_dim", who);
    }
  } else {
    SSR_REQUIRE(a->x, "%s: x is null", who);
  }
  if (a->epi == SSRHIP_EPI_QKV_APPEND) {
    SSR_REQUIRE(a->N == 3 * a->K && a->groups == 1 && a->kv.pool && a->kv.table && a->kv_pos && a->kv.head_dim > 0,
                "%s: QKV epilogue needs N==3K and a kv cache", who);
  }
  return 0;
}

}  // namespace
