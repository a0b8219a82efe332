// gemv_pair4.hip — pair launches of the 4-row decode step (two utterances x CFG, or four without), fp32 weights, gfx950.
//
// gemv.hip's pair launches (gemv_pair_kernel / gemv_pair_merge_kernel: TWO consecutive GEMVs of the step in ONE launch, the all-to-all edge
// between them inside the launch) at four batch rows. Same structure: 256 workgroups, one per CU, 8 streaming waves + 4 edge waves, the two
// roles the two arms of ONE wave-uniform branch with every barrier written in both arms; the hand-off is gemv_pair.h's protocol with
// 8192 granules per buffer (pair_edge_role<4, SA, NPRE>), the streaming phases are gemv_pair.h's with the WsF32 policy. Two forms:
//   * pair4_kernel<NUWB>:        A = FFN2 + residual (K = 8192, N = 2048), B = folded LayerNorm + Linear, N in {4096, 6144, 8192}
//                                (head-MLP1 with GELU, QKV with the K / V append, FFN1 with ReLU);
//   * pair4_merge_kernel<NUWB>:  A = split-KV merge prologue + out-projection + residual (K = 2048), B = FFN1.
// What the launches replace at 4 rows is gemv_seg_kernel<4, PRO, false> (gemv.hip): per unit, per segment, per statistic and per output the
// SAME operations in the same order — seg_park<4>, seg_layernorm<4>, seg_finish_row<4>, finalize, the merge with SegCS<4> = 2 prefetched
// pages — so the results are bit-identical (tests/test_gpu_pair4.py compares whole buffers). Which workgroup computes an output changes
// (8 rows of A and N / 256 rows of B per workgroup instead of a balanced split over 512), the order of its arithmetic does not.
// Registers: 12 waves per workgroup = 3 per SIMD = at most 168 VGPRs. x of four rows takes 64, a ring of DEPTH units DEPTH x 16:
// PAIR4_DEPTH units in flight per wave (the counts hipcc reports are in profiles/pair4_isa.md; tests/test_pair4_isa.py holds them to
// 168 and to no scratch).
#include <stdlib.h>
#include "common.h"
#include "gemv_shared.h"
#include "gemv_pair_host.h"

namespace {

constexpr int PAIR4_DEPTH = 4;   // units in the ring of a streaming wave
static_assert(PAIR4_DEPTH == PAIR_DEPTH, "gemv_pair.h's streaming phases are written for a ring of PAIR_DEPTH units");
constexpr int PAIR4_PF = 3;      // of B's first units, those posted behind barrier (1b), in front of the gather's loads (gemv.hip: PAIR_PF)

// A = FFN2 + residual (K = 8192): 8 rows per workgroup, wave w owns segment w of every row (unit j = row j), as gemv_seg_kernel<4, PRO_NONE,
// false> orders a row's units
template <int NUWB>
__global__ __launch_bounds__(PAIR_TH) void pair4_kernel(const PairK p) {
  constexpr int B = PAIR4_B, DEPTH = PAIR4_DEPTH, NUWA = 8;
  constexpr int RA = 8, SA = 8, SHA = 3;
  constexpr int RB = NUWB * SEG_NW / 2;
  __shared__ float partA[RA * SA * B];
  __shared__ float partB[RB * 2 * B];
  __shared__ float aux[2 * B * 2];
  __shared__ __attribute__((aligned(16))) float xs[B * PAIR_D];
  __shared__ size_t kvoff[B * 2];
  const ssrhip_gemv_args& a = p.a.a;
  const ssrhip_gemv_args& bb = p.b.a;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  if (wave < SEG_NW) {
    const int rA0 = (int)blockIdx.x * RA;
    const float* WgA = a.W + (size_t)rA0 * a.K + wave * SEG + lane * 4;
    // ---- 0. B's epilogue operand of the (row, b) this thread finalises: the wave's oldest load
    RowEpi efinB = {0.f, 0.f};
    efinB.bias = bb.bias ? bb.bias[(int)blockIdx.x * RB + min(t / B, RB - 1)] : 0.f;
    // ---- 1. the wave's slice of A's input (L2), then its first DEPTH units (HBM, non-temporal)
    float4 xr[B][4];
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[b][i] = ld4(a.x + (size_t)b * a.x_stride + wave * SEG + (i * 64 + lane) * 4);
    float4 w[DEPTH][4];
    // ---- 2. A's units
    pair_stream_a<WsF32, B, NUWA, SHA>(WgA, a.K, w, xr, NoScales(), partA, wave, lane);
    __syncthreads();                                                // (1) A's partial sums are parked
    pair_stream_b<WsF32, B, NUWB, 0, PAIR4_PF>(p, bb.W, NoScales(), t, lane, wave, xr, w, efinB, partB, aux, xs, kvoff);
  } else {
    pair_edge_role<B, SA, 0>(p, wave - SEG_NW, lane, partA, xs, kvoff);
  }
}

// A = split-KV merge + out-projection + residual (K = 2048): gemv_seg_kernel<4, PRO_ATTN_COMBINE, false> at one workgroup per CU, operation
// for operation — thread t owns float4 column t * 4 of the four rows in the merge (SegCS<4> = 2 pages prefetched, the rest loaded late),
// wave w the units w and w + 8 (both requested at entry). The merged rows pass through the LDS buffer that later receives x' (its A-phase
// use ends before barrier (1)). No early units of B: the ring's four slots and x of four rows leave no registers for them.
template <int NUWB>
__global__ __launch_bounds__(PAIR_TH) void pair4_merge_kernel(const PairK p) {
  constexpr int B = PAIR4_B, DEPTH = PAIR4_DEPTH, SEG_CS = SegCS<B>::v;
  constexpr int RA = 8, SA = 2;                                    // A: 8 rows per workgroup, K = 2048 = 2 segments, 16 units = 2 per wave (SHA = 1)
  constexpr int RB = NUWB * SEG_NW / 2;
  extern __shared__ __attribute__((aligned(16))) float wtab[];     // [B * H][max_splits] merge weights
  __shared__ float partA[RA * SA * B];
  __shared__ float partB[RB * 2 * B];
  __shared__ float aux[2 * B * 2];
  __shared__ __attribute__((aligned(16))) float xs[B * PAIR_D];
  __shared__ size_t kvoff[B * 2];
  const ssrhip_gemv_args& a = p.a.a;
  const ssrhip_gemv_args& bb = p.b.a;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  if (wave >= SEG_NW) {
    pair_edge_role<B, SA, 2>(p, wave - SEG_NW, lane, partA, xs, kvoff);
  } else {
    const int K = a.K, rA0 = (int)blockIdx.x * RA, seg = wave & (SA - 1);
    const float* WgA = a.W + (size_t)rA0 * K + seg * SEG + lane * 4;
    RowEpi efinB = {0.f, 0.f};
    efinB.bias = bb.bias ? bb.bias[(int)blockIdx.x * RB + min(t / B, RB - 1)] : 0.f;
    // ---- 1. the attention partials this thread merges (L2): (m, l) of its (row, head), the first SEG_CS pages of its column
    // (gemv_seg_kernel's merge, written out here too: see the note there)
    const int hd = p.a.hd, H = K / hd, MS = a.max_splits;
    float4 co[B][SEG_CS];
    float2 cml[SEG_CS];
    int ns[B];
#pragma unroll
    for (int b = 0; b < B; ++b) ns[b] = (a.row_len[b] + SSRHIP_PAGE - 1) / SSRHIP_PAGE;
    {
      const int tt = t % (B * H);
      const float* ml = a.part_ml + (size_t)tt * MS * 2;
#pragma unroll
      for (int i = 0; i < SEG_CS; ++i) cml[i] = *reinterpret_cast<const float2*>(ml + 2 * min(i, MS - 1));
      const int e = t * 4, h = e / hd, d = e % hd;
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const float* po = a.part_o + (((size_t)b * H + h) * MS) * hd + d;
#pragma unroll
        for (int s2 = 0; s2 < SEG_CS; ++s2) co[b][s2] = ld4(po + (size_t)min(s2, MS - 1) * hd);
      }
    }
    // ---- 2. the wave's two units of A, both now
    float4 w[DEPTH][4];
    pair_merge_request<WsF32, NUWB, 0>(WgA, K, bb.W, bb.K, w, wave, lane);
    // ---- 3. merge, under the latency of the units. EVERY thread computes the softmax-merge weights of (row, head) = t % (B * H), threads
    // 0 .. B * H - 1 store them (gemv_pair_merge_kernel explains why)
    {
      const int tt = t % (B * H);
      const bool keep = t < B * H;
      const int rr = tt / H;
      int n = ns[0];
#pragma unroll
      for (int b = 1; b < B; ++b) n = (rr == b) ? ns[b] : n;
      const float* ml = a.part_ml + (size_t)tt * MS * 2;
      float M = -INFINITY;
#pragma unroll
      for (int i = 0; i < SEG_CS; ++i)
        if (i < n) M = fmaxf(M, cml[i].x);
      for (int s2 = SEG_CS; s2 < n; ++s2) M = fmaxf(M, ld2_late(ml + 2 * s2).x);
      float den = 0.f;
#pragma unroll
      for (int i = 0; i < SEG_CS; ++i)
        if (i < n) den = fmaf(expf(cml[i].x - M), cml[i].y, den);
      for (int s2 = SEG_CS; s2 < n; ++s2) { const float2 v = ld2_late(ml + 2 * s2); den = fmaf(expf(v.x - M), v.y, den); }
      const float inv = 1.0f / den;
#pragma unroll
      for (int i = 0; i < SEG_CS; ++i)
        if (keep && i < n) wtab[tt * MS + i] = expf(cml[i].x - M) * inv;
      for (int s2 = SEG_CS; s2 < n; ++s2) { const float wv = expf(ld2_late(ml + 2 * s2).x - M) * inv; if (keep) wtab[tt * MS + s2] = wv; }
    }
    __syncthreads();                                                // (A1)
    {
      const int e = t * 4, h = e / hd, d = e % hd;
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const float* wt = wtab + (b * H + h) * MS;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int s2 = 0; s2 < SEG_CS; ++s2) {
          const bool in = s2 < ns[b];                               // a page beyond the row must not count (0 * NaN)
          const float ws = in ? wt[s2] : 0.f;
          acc.x = fmaf(ws, in ? co[b][s2].x : 0.f, acc.x);
          acc.y = fmaf(ws, in ? co[b][s2].y : 0.f, acc.y);
          acc.z = fmaf(ws, in ? co[b][s2].z : 0.f, acc.z);
          acc.w = fmaf(ws, in ? co[b][s2].w : 0.f, acc.w);
        }
        const float* po = a.part_o + (((size_t)b * H + h) * MS) * hd + d;
        for (int s2 = SEG_CS; s2 < ns[b]; ++s2) {                   // rows of more than SEG_CS pages: the rest, loaded late
          const float ws = wt[s2];
          const float4 o = ld4_late(po + (size_t)s2 * hd);
          acc.x = fmaf(ws, o.x, acc.x);
          acc.y = fmaf(ws, o.y, acc.y);
          acc.z = fmaf(ws, o.z, acc.z);
          acc.w = fmaf(ws, o.w, acc.w);
        }
        *reinterpret_cast<float4*>(xs + b * K + e) = acc;
      }
    }
    __syncthreads();                                                // (A2)
    float4 xr[B][4];
    seg_load_x<B>(xr, xs, K, seg, lane);
    // ---- 4. A's two units, written out: through pair_units (gemv_pair.h) hipcc swaps an LDS read of x' with a weight request behind
    // barrier (2) and adds two waits (profiles/pair_refactor_ab.md)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float acc[B][2];
#pragma unroll
      for (int b = 0; b < B; ++b) acc[b][0] = acc[b][1] = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int b = 0; b < B; ++b) acc[b][i & 1] = dot4(w[j][i], xr[b][i], acc[b][i & 1]);
      seg_park<B>(acc, partA, wave + SEG_NW * j, lane);
    }
    __syncthreads();                                                // (1) A's partial sums are parked
    pair_stream_b<WsF32, B, NUWB, 0, PAIR4_PF>(p, bb.W, NoScales(), t, lane, wave, xr, w, efinB, partB, aux, xs, kvoff);
  }
}

thread_local char g_pair4_why[200] = "";
PairForm<PairK> g_pair4_form = {{pair4_kernel<4>, pair4_kernel<6>, pair4_kernel<8>}, pair4_merge_kernel<8>, nullptr, false, "4-row pair", PAIR4_WTAB_MAX, false, nullptr, ""};

// ssrhip_gemv_pair_applicable's rules with B == 4: the shape rules of the 4-row forms (gemv_pair_host.h pair4_shape_plan: the 2-row
// question with the row count set to 2, then the merge's (row, head) table and its LDS) and the occupancy of the 4-row kernels
// (33-50 KB of LDS). Units per wave of B, or 0 with the reason in g_pair4_why.
int pair4_plan(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, bool* merge) {
  const int nuwb = pair4_shape_plan(g_pair4_why, a, b, merge);
  if (!nuwb) return 0;
  if (const char* why = pair_occupancy_refusal(g_pair4_form)) return pair_refuse(g_pair4_why, why);
  g_pair4_why[0] = 0;
  return nuwb;
}

}  // namespace

const char* ssrhip_gemv_pair4_why() { return g_pair4_why; }   // why the last question on this thread was answered with no (engine.hip reports it)

extern "C" int ssrhip_gemv_pair4_applicable(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b) {
  if (!a || !b) return 0;
  bool merge;
  return pair4_plan(a, b, &merge) ? 1 : 0;
}

extern "C" int ssrhip_gemv_pair4(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, void* ws, int32_t buf, int32_t buf_next, ssrhip_stream_t stream) {
  if (int rc = pair_entry_check("ssrhip_gemv_pair4", a, b, ws != nullptr, buf, buf_next)) return rc;
  bool merge = false;
  const int nuwb = pair4_plan(a, b, &merge);
  if (!nuwb) return 1;
  PairK p;
  pair_fill(p, a, b, merge, ws, buf, buf_next, PAIR4_GRAN);
  return pair_launch(g_pair4_form, p, merge, nuwb, PAIR4_B, a, (hipStream_t)stream);
}

extern "C" int ssrhip_gemv_pair4_status(const void* ws, ssrhip_stream_t stream) {   // ssrhip_gemv_pair_status at this workspace's size
  return pair_status(ws, SSRHIP_PAIR4_WS_BYTES, 3 * (size_t)PAIR4_GRAN * 8, "ssrhip_gemv_pair4_status", stream);
}
