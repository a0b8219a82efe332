// gemv_pair4_pk.hip — pair launches of the 4-row decode step (two utterances x CFG, or four without) over the PACKED weight streams:
// bf16 copies (SSRHIP_W16_INDEX) and e4m3 codes with one power-of-two scale per output row (SSRHIP_W8_INDEX). The opt-in pairing of a
// 4-row engine that streams packed weights, DESIGN.md Part I.26, gfx950.
//
// gemv_pair4.hip's launches with the streaming loops of gemv_pair_w16.hip / gemv_pair_w8.hip: 256 workgroups, one per CU, 8 streaming
// waves + 4 edge waves, the two roles the two arms of ONE wave-uniform branch with every barrier written in both arms; the hand-off is
// gemv_pair.h's protocol at four rows (pair_edge_role<4, SA, NPRE>, granule index n * 4 + row, 8192 granules per buffer: the workspace,
// buffer cycle and status poll of the fp32 4-row form, SSRHIP_PAIR4_WS_BYTES); the streaming phases are gemv_pair.h's with the WsB16 /
// WsE4 policies of gemv_wstream.h at B = 4, ring PAIR_DEPTH, PAIR_PF units behind barrier (1b). One kernel text per form, templated on
// the policy; the kernels are its instantiations under the names the launch tables and the ISA test use:
//   pair4_w16_kernel<NUWB>, pair4_w8_kernel<NUWB>                       A = FFN2 + residual (K = 8192, N = 2048), B = folded LayerNorm +
//                                                                      Linear, N in {4096, 6144, 8192} (head-MLP1, QKV + append, FFN1);
//   pair4_w16_merge_kernel<8, EARLY>, pair4_w8_merge_kernel<8, EARLY>   A = split-KV merge + out-projection + residual (K = 2048), B = FFN1;
//                                                                      EARLY = 2: B's first two units requested at entry into the
//                                                                      ring slots A leaves free (the packed rings are 32 / 16 VGPRs
//                                                                      where the fp32 ring's 64 left no room for them at four rows).
// What the launches replace at 4 rows is w16_segu_kernel<4, PRO, NUW, 2> / w16_seg_kernel<4, PRO_ATTN_COMBINE> and their w8 twins: per
// unit, per segment, per statistic and per output the SAME operations in the same order (w16_piece / w8_unit, the park of the stream with
// e4m3's multiply by the row's scale where the partial sum is parked, seg_layernorm<4>, seg_finish_row<4>, the merge with SegCS<4> = 2
// prefetched pages). The ring depth differs (2 there): that changes what is in flight, not the arithmetic. So a pair launch here, two
// ssrhip_gemv_w16 / ssrhip_gemv_w8 launches at B = 4 and ssrhip_gemv_pair4 on the equivalent fp32 masters give the same bits
// (tests/test_gpu_pair4_pk.py compares whole buffers). e4m3: every scale a wave will need is requested at kernel entry, ahead of the
// first codes. Registers: profiles/pair4_pk_isa.md; tests/test_pair4_pk_isa.py holds them to 168 and to no scratch.
#include <stdlib.h>
#include "common.h"
#include "gemv_shared.h"
#include "gemv_pair_host.h"

namespace {

// the kernel argument of both streams: the packed matrices in the stream's order and, e4m3 only, their per-row scales (bf16: null)
struct Pair4PkK {
  PairK k;
  const void* Wa;         // A's packed weights [2048][K_A]: uint16_t (SSRHIP_W16_INDEX) or uint8_t codes (SSRHIP_W8_INDEX)
  const void* Wb;         // B's [N_B][2048]
  const float* sa;        // e4m3: A's scales [2048]
  const float* sb;        // e4m3: B's scales [N_B]
};

// what a wave holds of its N units' scales: floats for the e4m3 stream, nothing for bf16 (the policy's load_scales takes either)
template <class S, int N> struct PkScales { typedef NoScales T; };
template <int N> struct PkScales<WsE4, N> { typedef float T[N]; };

// A = FFN2 + residual (K = 8192): 8 rows per workgroup, wave w owns segment w of every row (unit j = row j)
template <class S, int NUWB>
__device__ __forceinline__ void pair4_pk_ffn2(const Pair4PkK& q) {
  constexpr int B = PAIR4_B, NUWA = PAIR_NUWA;
  constexpr int RA = 8, SA = 8, SHA = 3;
  constexpr int RB = NUWB * SEG_NW / 2;
  typedef typename S::Elem Elem;
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
    const Elem* WgA = (const Elem*)q.Wa + (size_t)rA0 * a.K + wave * SEG + lane * S::LANE;
    // ---- 0. B's epilogue operand of the (row, b) this thread finalises: the wave's oldest load
    RowEpi efinB = {0.f, 0.f};
    efinB.bias = bb.bias ? bb.bias[(int)blockIdx.x * RB + min(t / B, RB - 1)] : 0.f;
    // ---- 1. the wave's slice of A's input (L2), every scale it will need (A's rows, then B's), then its first units (HBM, non-temporal)
    float4 xr[B][4];
    seg_load_x<B>(xr, a.x, (size_t)a.x_stride, wave, lane);
    typename PkScales<S, NUWA>::T scA;
    typename PkScales<S, NUWB>::T scB;
    S::template load_scales<NUWA, SHA>(scA, q.sa, rA0, wave);
    S::template load_scales<NUWB, 1>(scB, q.sb + (size_t)((int)blockIdx.x * RB), 0, wave);
    S::fence();                                                     // the scales are requested BEFORE any code
    typename S::Slot w[PAIR_DEPTH];
    // ---- 2. A's units
    pair_stream_a<S, B, NUWA, SHA>(WgA, a.K, w, xr, scA, partA, wave, lane);
    __syncthreads();                                                // (1) A's (scaled) partial sums are parked
    pair_stream_b<S, B, NUWB, 0, PAIR_PF>(p, (const Elem*)q.Wb, scB, t, lane, wave, xr, w, efinB, partB, aux, xs, kvoff);
  } else {
    pair_edge_role<B, SA, 0>(p, wave - SEG_NW, lane, partA, xs, kvoff);
  }
}

// A = split-KV merge + out-projection + residual (K = 2048): the stream's seg kernel <4, PRO_ATTN_COMBINE> at one workgroup per CU,
// operation for operation — thread t owns float4 column t * 4 of the four rows in the merge (SegCS<4> = 2 pages prefetched, the rest
// loaded late), wave w the units w and w + 8 (both requested at entry). The merge prologue is written out once more, in
// pair4_merge_kernel's form (gemv_shared.h says why it is not a helper): EVERY thread computes the weights of (row, head) = t % (B * H),
// threads 0 .. B * H - 1 store them. The merged rows pass through the LDS buffer that later receives x'.
template <class S, int NUWB, int EARLY>
__device__ __forceinline__ void pair4_pk_merge(const Pair4PkK& q) {
  constexpr int B = PAIR4_B, SEG_CS = SegCS<B>::v;
  constexpr int RA = 8, SA = 2, SHA = 1;                           // A: 8 rows per workgroup, K = 2048 = 2 segments, 16 units = 2 per wave
  constexpr int RB = NUWB * SEG_NW / 2;
  typedef typename S::Elem Elem;
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
    const Elem* WgA = (const Elem*)q.Wa + (size_t)rA0 * K + seg * SEG + lane * S::LANE;
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
    // ---- 2. every scale the wave will need (A's two rows, then B's NUWB), then the wave's two units of A (and B's early ones), all now
    typename PkScales<S, 2>::T scA;
    typename PkScales<S, NUWB>::T scB;
    S::template load_scales<2, SHA>(scA, q.sa, rA0, wave);
    S::template load_scales<NUWB, 1>(scB, q.sb + (size_t)((int)blockIdx.x * RB), 0, wave);
    S::fence();                                                     // the scales are requested BEFORE any code
    typename S::Slot w[PAIR_DEPTH];
    pair_merge_request<S, NUWB, EARLY>(WgA, K, (const Elem*)q.Wb, bb.K, w, wave, lane);
    // ---- 3. merge, under the latency of the units
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
    // ---- 4. A's two units
    pair_units<S, B, 2, SHA, 0>(WgA, K, w, xr, scA, partA, wave, lane);
    __syncthreads();                                                // (1) A's (scaled) partial sums are parked
    pair_stream_b<S, B, NUWB, EARLY, PAIR_PF>(p, (const Elem*)q.Wb, scB, t, lane, wave, xr, w, efinB, partB, aux, xs, kvoff);
  }
}

template <int NUWB>
__global__ __launch_bounds__(PAIR_TH) void pair4_w16_kernel(const Pair4PkK q) { pair4_pk_ffn2<WsB16, NUWB>(q); }
template <int NUWB, int EARLY>
__global__ __launch_bounds__(PAIR_TH) void pair4_w16_merge_kernel(const Pair4PkK q) { pair4_pk_merge<WsB16, NUWB, EARLY>(q); }
template <int NUWB>
__global__ __launch_bounds__(PAIR_TH) void pair4_w8_kernel(const Pair4PkK q) { pair4_pk_ffn2<WsE4, NUWB>(q); }
template <int NUWB, int EARLY>
__global__ __launch_bounds__(PAIR_TH) void pair4_w8_merge_kernel(const Pair4PkK q) { pair4_pk_merge<WsE4, NUWB, EARLY>(q); }

thread_local char g_pair4_w16_why[200] = "";
thread_local char g_pair4_w8_why[200] = "";
PairForm<Pair4PkK> g_pair4_w16_form = {{pair4_w16_kernel<4>, pair4_w16_kernel<6>, pair4_w16_kernel<8>}, pair4_w16_merge_kernel<8, 2>, pair4_w16_merge_kernel<8, 0>,
                                       true, "4-row bf16 pair", PAIR4_WTAB_MAX, false, nullptr, ""};
PairForm<Pair4PkK> g_pair4_w8_form = {{pair4_w8_kernel<4>, pair4_w8_kernel<6>, pair4_w8_kernel<8>}, pair4_w8_merge_kernel<8, 2>, pair4_w8_merge_kernel<8, 0>,
                                      true, "4-row e4m3 pair", PAIR4_WTAB_MAX, false, nullptr, ""};

// The packed 4-row question: the 4-row shape rules (pair4_shape_plan: B == 4, the 2-row question on the same descriptors, the merge's
// table and LDS) AND the stream's own applicability for both launches (SSRHIP_GEMV_SEG=0 turns it off) AND a CU takes every
// instantiation of the form. Units per wave of B, or 0 with the reason in `why` (the form's thread-local text).
int pair4_pk_plan(PairForm<Pair4PkK>& f, char (&why)[200], const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, int (*stream_applicable)(const ssrhip_gemv_args*),
                  const char* stream_refusal, bool* merge) {
  const int nuwb = pair4_shape_plan(why, a, b, merge);
  if (!nuwb) return 0;
  if (!stream_applicable(a) || !stream_applicable(b)) return pair_refuse(why, stream_refusal);
  if (const char* w = pair_occupancy_refusal(f)) return pair_refuse(why, w);
  why[0] = 0;
  return nuwb;
}
int pair4_w16_plan(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, bool* merge) {
  return pair4_pk_plan(g_pair4_w16_form, g_pair4_w16_why, a, b, ssrhip_gemv_w16_applicable,
                       "the bf16 weight stream does not take these launches (ssrhip_gemv_w16_applicable; SSRHIP_GEMV_SEG=0 turns it off)", merge);
}
int pair4_w8_plan(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, bool* merge) {
  return pair4_pk_plan(g_pair4_w8_form, g_pair4_w8_why, a, b, ssrhip_gemv_w8_applicable,
                       "the e4m3 weight stream does not take these launches (ssrhip_gemv_w8_applicable; SSRHIP_GEMV_SEG=0 turns it off)", merge);
}

int pair4_pk_go(PairForm<Pair4PkK>& f, const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, bool merge, int nuwb, const void* Wa, const float* sa, const void* Wb,
                const float* sb, void* ws, int buf, int buf_next, ssrhip_stream_t stream) {
  Pair4PkK q;
  pair_fill(q.k, a, b, merge, ws, buf, buf_next, PAIR4_GRAN);
  q.Wa = Wa;
  q.Wb = Wb;
  q.sa = sa;
  q.sb = sb;
  return pair_launch(f, q, merge, nuwb, PAIR4_B, a, (hipStream_t)stream);
}

}  // namespace

// why the last question on this thread was answered with no (engine.hip reports it)
const char* ssrhip_gemv_pair4_w16_why() { return g_pair4_w16_why; }
const char* ssrhip_gemv_pair4_w8_why() { return g_pair4_w8_why; }

extern "C" int ssrhip_gemv_pair4_w16_applicable(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b) {
  if (!a || !b) return 0;
  bool merge;
  return pair4_w16_plan(a, b, &merge) ? 1 : 0;
}

extern "C" int ssrhip_gemv_pair4_w16(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, const uint16_t* Wa16, const uint16_t* Wb16, void* ws, int32_t buf,
                                     int32_t buf_next, ssrhip_stream_t stream) {
  if (int rc = pair_entry_check("ssrhip_gemv_pair4_w16", a, b, Wa16 && Wb16 && ws, buf, buf_next)) return rc;
  bool merge = false;
  const int nuwb = pair4_w16_plan(a, b, &merge);
  if (!nuwb) return 1;
  return pair4_pk_go(g_pair4_w16_form, a, b, merge, nuwb, Wa16, nullptr, Wb16, nullptr, ws, buf, buf_next, stream);
}

extern "C" int ssrhip_gemv_pair4_w8_applicable(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b) {
  if (!a || !b) return 0;
  bool merge;
  return pair4_w8_plan(a, b, &merge) ? 1 : 0;
}

extern "C" int ssrhip_gemv_pair4_w8(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, const uint8_t* Wa8, const float* scale_a, const uint8_t* Wb8,
                                    const float* scale_b, void* ws, int32_t buf, int32_t buf_next, ssrhip_stream_t stream) {
  if (int rc = pair_entry_check("ssrhip_gemv_pair4_w8", a, b, Wa8 && scale_a && Wb8 && scale_b && ws, buf, buf_next)) return rc;
  bool merge = false;
  const int nuwb = pair4_w8_plan(a, b, &merge);
  if (!nuwb) return 1;
  return pair4_pk_go(g_pair4_w8_form, a, b, merge, nuwb, Wa8, scale_a, Wb8, scale_b, ws, buf, buf_next, stream);
}
