// gemv_shared.h — what the <= 4-row weight-streaming GEMV kernels of gemv.hip (fp32 weights) and gemv_w16.hip (packed bf16 weights) have
// in common: the launch descriptor, the geometry of the segment kernels, the per-row epilogue and the late loads of the merge prologue.
// One definition, so that the two translation units finish a row with the same operations in the same order (bit-identical results).
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

}  // namespace
