// gemv_pair_w8.hip — the pair launches of gemv.hip (two consecutive GEMVs of the 2-row decode step in ONE launch, the all-to-all edge
// inside it) over PACKED e4m3 CODES with one power-of-two scale per output row (SSRHIP_W8_INDEX): the opt-in pairing of an e4m3 weight
// stream, DESIGN.md Part I.20, gfx950.
//
// NOTHING about the hand-off changes against gemv_pair_kernel / gemv_pair_merge_kernel (and their bf16 twins of gemv_pair_w16.hip): the
// same 256 workgroups x 12 waves, the same barriers in both arms of the one wave-uniform branch, the same edge role (waves 8-11), the same
// granule protocol, workspace and buffer cycle. Only the bytes waves 0-7 stream change, how they are widened (v_cvt_pk_f32_fp8, exact) and
// one multiply where a partial sum is parked:
//   w8_pair_kernel<NUWB>           A = FFN2 (K = 8192), the streaming of w8_segu_kernel<2, PRO_NONE, 8, 4>;
//                                  B = QKV / head-MLP1 / FFN1, pair_stream_b<WsE4, ..>: w8_segu_kernel<2, PRO_LAYERNORM, NUWB, 4>'s arithmetic
//   w8_pair_merge_kernel<8, EARLY> A = split-KV merge + out-projection (K = 2048), w8_seg_kernel<2, PRO_ATTN_COMBINE> at one workgroup
//                                  per CU; B = FFN1; EARLY = 2: B's first two units requested at entry into the ring slots A leaves free
// Each phase runs the fmaf / wave_sum sequence of the w8 kernel it mirrors and multiplies the (row, segment) partial sum by the row's
// s[n] = 2^e where it is parked (partA for A, partB for B; a plain multiply, the library is built with -ffp-contract=off). The edge role
// therefore publishes and gathers already-scaled fp32 values and does not know about scales. A multiplication by 2^e commutes with every
// fp32 rounding as long as nothing is subnormal or overflows, so a pair launch here, two ssrhip_gemv_w8 launches and
// ssrhip_gemv_pair on the masters q * 2^e give the same bits (tests/test_gpu_w8_pair.py compares whole buffers with np.array_equal).
//
// Scales: every scale a wave will need — A's (8 in the FFN2 form, 2 in the merge form) and B's NUWB — is requested at KERNEL ENTRY, ahead
// of the first codes, and held across the A phase. So a row's scale is always an older load than that row's codes (I.18's rule: waiting
// for it never drains the ring), also for the merge form's early units of B. A sched_barrier behind the scale loads keeps the scheduler
// from moving them behind the first codes (it did). They are vector loads and cost 8 + NUWB (merge form: 2 + 8) VGPRs held across the
// A phase; the ring is 16 VGPRs where the fp32 form's is 64, and every kernel stays below its fp32 counterpart (DESIGN.md I.20 has the counts).
// Units in flight are the fp32 / bf16 forms' COUNTS — ring 4, PF 3, EARLY 2 — at a quarter / half the bytes each: one 16-byte load per
// unit and lane. -DSSR_W8_PAIR_PF=4 builds the lab form with all four units behind barrier (1b); it is not shipped and not measured.
//
// This file holds what is specific to the e4m3 stream: the kernels' entry text with the scale requests, the kernel argument with codes and
// scales and the form's table, "why" text and applicability question. Everything else is shared: the edge role (pair_edge_role<B, SA,
// NPRE>), the sweep, PairK, the PAIR_* constants and the streaming phases (pair_stream_a, pair_merge_request, pair_units, pair_stream_b) in
// csrc/gemv_pair.h, instantiated here with the WsE4 policy of csrc/gemv_wstream.h (its load_scales / fence are the scales-at-entry hook),
// which also holds gemv_w8.hip's widening; the host side in csrc/gemv_pair_host.h (profiles/pair_refactor_ab.md).
#include <stdlib.h>
#include "common.h"
#include "gemv_shared.h"
#include "gemv_pair_host.h"

namespace {

#ifndef SSR_W8_PAIR_PF
#define SSR_W8_PAIR_PF PAIR_PF
#endif
constexpr int W8_PAIR_PF = SSR_W8_PAIR_PF;   // units posted behind barrier (1b); the lab macro overrides the fp32 forms' count

struct W8PairK {
  PairK k;
  const uint8_t* Wa8;     // A's codes [2048][K_A] in SSRHIP_W8_INDEX order
  const float* sa;        // A's scales [2048]
  const uint8_t* Wb8;     // B's codes [N_B][2048]
  const float* sb;        // B's scales [N_B]
};

// The two ROLES are the two arms of ONE (wave-uniform) branch and every barrier is written in both arms (gemv.hip says what the other
// form cost). A = FFN2 + residual (K = 8192): w8_segu_kernel<2, PRO_NONE, 8, 4> — 8 units per wave, a ring of 4, one 16-byte load per unit.
template <int NUWB>
__global__ __launch_bounds__(PAIR_TH, 2) void w8_pair_kernel(const W8PairK q) {
  constexpr int B = 2, DEPTH = PAIR_DEPTH, NUWA = PAIR_NUWA;
  constexpr int RA = 8, SA = 8, SHA = 3;                           // A: 8 rows per workgroup, K = 8192 = 8 segments, wave w owns segment w
  constexpr int RB = NUWB * SEG_NW / 2;
  __shared__ float partA[RA * SA * B];
  __shared__ float partB[RB * 2 * B];
  __shared__ float aux[2 * B * 2];
  __shared__ __attribute__((aligned(16))) float xs[B * PAIR_D];
  __shared__ size_t kvoff[B * 2];
  const PairK& p = q.k;
  const ssrhip_gemv_args& a = p.a.a;
  const ssrhip_gemv_args& bb = p.b.a;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  if (wave < SEG_NW) {
    const int rA0 = (int)blockIdx.x * RA;
    const uint8_t* WgA = q.Wa8 + (size_t)rA0 * a.K + wave * SEG + lane * 16;
    // ---- 0. B's epilogue operand of the (row, b) this thread finalises (wave 0's threads do): the wave's oldest load
    RowEpi efinB = {0.f, 0.f};
    efinB.bias = bb.bias ? bb.bias[(int)blockIdx.x * RB + min(t / B, RB - 1)] : 0.f;
    // ---- 1. the wave's slice of A's input (L2), every scale it will need (A's rows, then B's), then its first DEPTH units (HBM, non-temporal)
    float4 xr[B][4];
    seg_load_x<B>(xr, a.x, (size_t)a.x_stride, wave, lane);
    float scA[NUWA], scB[NUWB];
    WsE4::load_scales<NUWA, SHA>(scA, q.sa, rA0, wave);
    WsE4::load_scales<NUWB, 1>(scB, q.sb + (size_t)((int)blockIdx.x * RB), 0, wave);
    WsE4::fence();                                                  // the scales are requested BEFORE any code: the scheduler must not swap them
    w8_v4u w[DEPTH];
    // ---- 2. A's units
    pair_stream_a<WsE4, B, NUWA, SHA>(WgA, a.K, w, xr, scA, partA, wave, lane);
    __syncthreads();                                                // (1) A's scaled partial sums are parked
    pair_stream_b<WsE4, B, NUWB, 0, W8_PAIR_PF>(p, q.Wb8, scB, t, lane, wave, xr, w, efinB, partB, aux, xs, kvoff);
  } else {
    pair_edge_role<B, SA, 0>(p, wave - SEG_NW, lane, partA, xs, kvoff);
  }
}

// A = split-KV merge + out-projection + residual (K = 2048): w8_seg_kernel<2, PRO_ATTN_COMBINE> at one workgroup per CU, operation for
// operation — thread t owns float4 column t * 4 of both rows in the merge, wave w the units w and w + 8 (both requested at entry). The
// merge prologue is written out once more (its fifth home; gemv_shared.h says why it cannot be a helper), in gemv_pair_merge_kernel's
// form: EVERY thread computes the weights of (row, head) = t % (B * H), threads 0 .. B * H - 1 store them.
template <int NUWB, int EARLY = 0, int PFX = W8_PAIR_PF>
__global__ __launch_bounds__(PAIR_TH, 2) void w8_pair_merge_kernel(const W8PairK q) {
  constexpr int B = 2, DEPTH = PAIR_DEPTH, SEG_CS = SegCS<B>::v;
  constexpr int RA = 8, SA = 2, SHA = 1;                           // A: 8 rows per workgroup, K = 2048 = 2 segments, 16 units = 2 per wave
  constexpr int RB = NUWB * SEG_NW / 2;
  extern __shared__ __attribute__((aligned(16))) float wtab[];     // [B * H][max_splits] merge weights
  __shared__ float partA[RA * SA * B];
  __shared__ float partB[RB * 2 * B];
  __shared__ float aux[2 * B * 2];
  __shared__ __attribute__((aligned(16))) float xs[B * PAIR_D];
  __shared__ size_t kvoff[B * 2];
  const PairK& p = q.k;
  const ssrhip_gemv_args& a = p.a.a;
  const ssrhip_gemv_args& bb = p.b.a;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  if (wave >= SEG_NW) {
    pair_edge_role<B, SA, 2>(p, wave - SEG_NW, lane, partA, xs, kvoff);
  } else {
    const int K = a.K, rA0 = (int)blockIdx.x * RA, seg = wave & (SA - 1);
    const uint8_t* WgA = q.Wa8 + (size_t)rA0 * K + seg * SEG + lane * 16;
    RowEpi efinB = {0.f, 0.f};
    efinB.bias = bb.bias ? bb.bias[(int)blockIdx.x * RB + min(t / B, RB - 1)] : 0.f;
    // ---- 1. the attention partials this thread merges (L2): (m, l) of its (row, head), the first SEG_CS pages of its column
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
    // ---- 2. every scale the wave will need (A's two rows, then B's NUWB), then the wave's two units of A, both now
    float scA[2], scB[NUWB];
    WsE4::load_scales<2, SHA>(scA, q.sa, rA0, wave);
    WsE4::load_scales<NUWB, 1>(scB, q.sb + (size_t)((int)blockIdx.x * RB), 0, wave);
    WsE4::fence();                                                  // the scales are requested BEFORE any code: the scheduler must not swap them
    w8_v4u w[DEPTH];
    pair_merge_request<WsE4, NUWB, EARLY>(WgA, K, q.Wb8, bb.K, w, wave, lane);
    // ---- 3. merge, under the latency of the units
    {
      const int tt = t % (B * H);
      const bool keep = t < B * H;
      const int n = ns[tt / H];
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
        for (int s2 = SEG_CS; s2 < ns[b]; ++s2) {
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
    // ---- 4. A's two units
    pair_units<WsE4, B, 2, SHA, 0>(WgA, K, w, xr, scA, partA, wave, lane);
    __syncthreads();                                                // (1) A's scaled partial sums are parked
    pair_stream_b<WsE4, B, NUWB, EARLY, PFX>(p, q.Wb8, scB, t, lane, wave, xr, w, efinB, partB, aux, xs, kvoff);
  }
}

thread_local char g_w8_pair_why[200] = "";
PairForm<W8PairK> g_w8_pair_form = {{w8_pair_kernel<4>, w8_pair_kernel<6>, w8_pair_kernel<8>}, w8_pair_merge_kernel<8, 2>, w8_pair_merge_kernel<8, 0>,
                                    true, "e4m3 pair", 16 * 1024, false, nullptr, ""};

// units per wave of B, or 0 with the reason in g_w8_pair_why (gemv_pair_host.h pair_packed_plan)
int w8_pair_plan(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, bool* merge) {
  return pair_packed_plan(g_w8_pair_form, g_w8_pair_why, a, b, ssrhip_gemv_w8_applicable,
                          "the e4m3 weight stream does not take these launches (ssrhip_gemv_w8_applicable; SSRHIP_GEMV_SEG=0 turns it off)", merge);
}

}  // namespace

const char* ssrhip_gemv_pair_w8_why() { return g_w8_pair_why; }   // why the last question on this thread was answered with no (engine.hip reports it)

extern "C" int ssrhip_gemv_pair_w8_applicable(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b) {
  if (!a || !b) return 0;
  bool merge;
  return w8_pair_plan(a, b, &merge) ? 1 : 0;
}

extern "C" int ssrhip_gemv_pair_w8(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, const uint8_t* Wa8, const float* scale_a, const uint8_t* Wb8,
                                   const float* scale_b, void* ws, int32_t buf, int32_t buf_next, ssrhip_stream_t stream) {
  if (int rc = pair_entry_check("ssrhip_gemv_pair_w8", a, b, Wa8 && scale_a && Wb8 && scale_b && ws, buf, buf_next)) return rc;
  bool merge = false;
  const int nuwb = w8_pair_plan(a, b, &merge);
  if (!nuwb) return 1;
  W8PairK q;
  pair_fill(q.k, a, b, merge, ws, buf, buf_next, PAIR_GRAN);
  q.Wa8 = Wa8;
  q.sa = scale_a;
  q.Wb8 = Wb8;
  q.sb = scale_b;
  return pair_launch(g_w8_pair_form, q, merge, nuwb, 2, a, (hipStream_t)stream);
}
