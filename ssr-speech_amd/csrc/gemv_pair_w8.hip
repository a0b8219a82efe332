// gemv_pair_w8.hip — the pair launches of gemv.hip (two consecutive GEMVs of the 2-row decode step in ONE launch, the all-to-all edge
// inside it) over PACKED e4m3 CODES with one power-of-two scale per output row (SSRHIP_W8_INDEX): the opt-in pairing of an e4m3 weight
// stream, DESIGN.md Part I.20, gfx950.
//
// NOTHING about the hand-off changes against gemv_pair_kernel / gemv_pair_merge_kernel (and their bf16 twins of gemv_pair_w16.hip): the
// same 256 workgroups x 12 waves, the same barriers in both arms of the one wave-uniform branch, the same edge role (waves 8-11), the same
// granule protocol, workspace and buffer cycle. Only the bytes waves 0-7 stream change, how they are widened (v_cvt_pk_f32_fp8, exact) and
// one multiply where a partial sum is parked:
//   w8_pair_kernel<NUWB>           A = FFN2 (K = 8192), the streaming of w8_segu_kernel<2, PRO_NONE, 8, 4>;
//                                  B = QKV / head-MLP1 / FFN1, pair_stream_b's sequence with w8_segu_kernel<2, PRO_LAYERNORM, NUWB, 4>'s arithmetic
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
// The edge role (pair_edge_role<SA, NPRE>), the sweep, PairK, the PAIR_* constants and the time-bounded spin are gemv.hip's own, shared
// through csrc/gemv_pair.h: they are weight-agnostic.
#include <stdlib.h>
#include "common.h"
#include "gemv_shared.h"
#include "gemv_pair.h"

namespace {

#ifndef SSR_W8_PAIR_PF
#define SSR_W8_PAIR_PF PAIR_PF
#endif
constexpr int W8_PAIR_PF = SSR_W8_PAIR_PF;   // units posted behind barrier (1b); the lab macro overrides the fp32 forms' count

// ---- gemv_w8.hip's widening once more (it lives in that file's anonymous namespace, and that file stays as it is)
typedef unsigned w8_v4u __attribute__((ext_vector_type(4)));
typedef float w8_v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ w8_v4u ld16_nt(const uint8_t* p) { return __builtin_nontemporal_load(reinterpret_cast<const w8_v4u*>(p)); }
// the float4 of one dword: code m sits in byte m
__device__ __forceinline__ float4 w8_wide(const unsigned d) {
  const w8_v2f lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)d, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)d, true);
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}
// one unit against the lane's x: gemv_seg_kernel's `acc[b][i & 1] = dot4(w[i], xr[b][i], acc[b][i & 1])` for i = 0..3
template <int B>
__device__ __forceinline__ void w8_unit(const w8_v4u u, const float4 (&xr)[B][4], float (&acc)[B][2]) {
  const float4 w0 = w8_wide(u.x), w1 = w8_wide(u.y), w2 = w8_wide(u.z), w3 = w8_wide(u.w);
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b][0] = dot4(w0, xr[b][0], acc[b][0]);
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b][1] = dot4(w1, xr[b][1], acc[b][1]);
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b][0] = dot4(w2, xr[b][2], acc[b][0]);
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b][1] = dot4(w3, xr[b][3], acc[b][1]);
}
// one unit done: seg_park with the row's scale applied to the partial sum that is parked (u = local_row * S + seg)
template <int B>
__device__ __forceinline__ void w8_park(const float (&acc)[B][2], float sc, float* part, int u, int lane) {
  float mine = 0.f;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const float sum = wave_sum(acc[b][0] + acc[b][1]);
    if (lane == b) mine = sum;
  }
  if (lane < B) part[lane + u * B] = mine * sc;
}

struct W8PairK {
  PairK k;
  const uint8_t* Wa8;     // A's codes [2048][K_A] in SSRHIP_W8_INDEX order
  const float* sa;        // A's scales [2048]
  const uint8_t* Wb8;     // B's codes [N_B][2048]
  const float* sb;        // B's scales [N_B]
};

// the NUWB scales of this wave's units of B: unit j works on row (wave + 8 j) / 2 of the workgroup's RB rows (SB = 2 segments per row)
template <int NUWB>
__device__ __forceinline__ void w8_pair_scales_b(const W8PairK& q, int wave, float (&scB)[NUWB]) {
  constexpr int RB = NUWB * SEG_NW / 2;
  const float* Sg = q.sb + (size_t)((int)blockIdx.x * RB);
#pragma unroll
  for (int j = 0; j < NUWB; ++j) scB[j] = Sg[(wave + SEG_NW * j) >> 1];
}

// ---- the streaming role from barrier (1) on: pair_stream_b's sequence over packed codes — B = LayerNorm + Linear on x'
// (w8_segu_kernel<2, PRO_LAYERNORM, NUWB, 4>'s arithmetic). EARLY / PFX as in gemv.hip: unit j lives in w[(j + EARLY) % DEPTH].
template <int NUWB, int EARLY = 0, int PFX = W8_PAIR_PF>
__device__ __forceinline__ void w8_pair_stream_b(const W8PairK& q, int t, int lane, int wave, float4 (&xr)[2][4], w8_v4u (&w)[PAIR_DEPTH],
                                                 const float (&scB)[NUWB], const RowEpi& efinB, float* partB, float* aux, const float* xs,
                                                 const size_t* kvoff) {
  constexpr int B = 2, DEPTH = PAIR_DEPTH, PF = PFX, SB = 2, SHB = 1, RB = NUWB * SEG_NW / SB;
  static_assert(PFX >= EARLY && PFX <= PAIR_DEPTH, "units requested at (1b) start behind the early ones and fit the ring");
  static_assert(EARLY == 0 || EARLY == 2, "ring slots 2 and 3 are the ones the merge form's A phase leaves free");
  const PairK& p = q.k;
  const ssrhip_gemv_args& bb = p.b.a;
  const int rB0 = (int)blockIdx.x * RB, segB = wave & (SB - 1);
  const int bfin = t % B, rfinB = min(t / B, RB - 1), nfinB = rB0 + rfinB;
  const uint8_t* WgB = q.Wb8 + (size_t)rB0 * bb.K + segB * SEG + lane * 16;
  __syncthreads();                                                  // (1b) wave 8 has issued the publish
  // B's first units: PF of them now, the rest behind the gather
#pragma unroll
  for (int j = EARLY; j < PF; ++j) w[(j + EARLY) % DEPTH] = ld16_nt(WgB + (size_t)((wave + SEG_NW * j) >> SHB) * bb.K);
  __syncthreads();                                                  // (2) x' is in LDS
  seg_load_x<B>(xr, xs, PAIR_D, segB, lane);
#pragma unroll
  for (int j = PF; j < DEPTH; ++j) w[(j + EARLY) % DEPTH] = ld16_nt(WgB + (size_t)((wave + SEG_NW * j) >> SHB) * bb.K);
  seg_layernorm<B>(xr, aux, SB, bb.K, bb.ln_eps, wave, lane);       // its barrier is (3)
  // units
#pragma unroll
  for (int j = 0; j < NUWB; ++j) {
    w8_v4u& wj = w[(j + EARLY) % DEPTH];
    float acc[B][2];
#pragma unroll
    for (int b = 0; b < B; ++b) acc[b][0] = acc[b][1] = 0.f;
    w8_unit<B>(wj, xr, acc);
    if (j + DEPTH < NUWB) {
      __builtin_amdgcn_sched_barrier(0);                            // use, THEN overwrite in place
      wj = ld16_nt(WgB + (size_t)((wave + SEG_NW * (j + DEPTH)) >> SHB) * bb.K);
      __builtin_amdgcn_sched_barrier(0);
    }
    w8_park<B>(acc, scB[j], partB, wave + SEG_NW * j, lane);
  }
  __syncthreads();                                                  // (4)
  if (t < RB * B) {
    // K / V append addresses: resolved by the edge role (wave 9) while this role streamed
    float* kvb[2] = {bb.kv.pool + kvoff[bfin * 2], bb.kv.pool + kvoff[bfin * 2 + 1]};
    seg_finish_row<B>(p.b, 0, partB, SB, rfinB, nfinB, bfin, efinB, kvb);
  }
}

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
#pragma unroll
    for (int j = 0; j < NUWA; ++j) scA[j] = q.sa[rA0 + ((wave + SEG_NW * j) >> SHA)];
    w8_pair_scales_b<NUWB>(q, wave, scB);
    __builtin_amdgcn_sched_barrier(0);                              // the scales are requested BEFORE any code: the scheduler must not swap them
    w8_v4u w[DEPTH];
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) w[j] = ld16_nt(WgA + (size_t)((wave + SEG_NW * j) >> SHA) * a.K);
    // ---- 2. A's units
#pragma unroll
    for (int j = 0; j < NUWA; ++j) {
      w8_v4u& wj = w[j % DEPTH];
      float acc[B][2];
#pragma unroll
      for (int b = 0; b < B; ++b) acc[b][0] = acc[b][1] = 0.f;
      w8_unit<B>(wj, xr, acc);
      if (j + DEPTH < NUWA) {
        __builtin_amdgcn_sched_barrier(0);
        wj = ld16_nt(WgA + (size_t)((wave + SEG_NW * (j + DEPTH)) >> SHA) * a.K);
        __builtin_amdgcn_sched_barrier(0);
      }
      w8_park<B>(acc, scA[j], partA, wave + SEG_NW * j, lane);
    }
    __syncthreads();                                                // (1) A's scaled partial sums are parked
    w8_pair_stream_b<NUWB>(q, t, lane, wave, xr, w, scB, efinB, partB, aux, xs, kvoff);
  } else {
    pair_edge_role<SA, 0>(p, wave - SEG_NW, lane, partA, xs, kvoff);
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
    pair_edge_role<SA, 2>(p, wave - SEG_NW, lane, partA, xs, kvoff);
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
#pragma unroll
    for (int j = 0; j < 2; ++j) scA[j] = q.sa[rA0 + ((wave + SEG_NW * j) >> SHA)];
    w8_pair_scales_b<NUWB>(q, wave, scB);
    __builtin_amdgcn_sched_barrier(0);                              // the scales are requested BEFORE any code: the scheduler must not swap them
    w8_v4u w[DEPTH];
#pragma unroll
    for (int j = 0; j < 2; ++j) w[j] = ld16_nt(WgA + (size_t)((wave + SEG_NW * j) >> SHA) * K);
    if constexpr (EARLY == 2) {
      // B's units 0 and 1 (w8_pair_stream_b's addresses: SB = 2 segments per row, unit u = row (wave + 8 u) / 2 of this workgroup's RB rows)
      const uint8_t* WgB = q.Wb8 + (size_t)((int)blockIdx.x * RB) * bb.K + (wave & 1) * SEG + lane * 16;
#pragma unroll
      for (int j = 0; j < 2; ++j) w[2 + j] = ld16_nt(WgB + (size_t)((wave + SEG_NW * j) >> 1) * bb.K);
    }
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
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float acc[B][2];
#pragma unroll
      for (int b = 0; b < B; ++b) acc[b][0] = acc[b][1] = 0.f;
      w8_unit<B>(w[j], xr, acc);
      w8_park<B>(acc, scA[j], partA, wave + SEG_NW * j, lane);
    }
    __syncthreads();                                                // (1) A's scaled partial sums are parked
    w8_pair_stream_b<NUWB, EARLY, PFX>(q, t, lane, wave, xr, w, scB, efinB, partB, aux, xs, kvoff);
  }
}

thread_local char g_w8_pair_why[200] = "";

// Can the new instantiations keep a workgroup on a CU? Asked once per process, as gemv.hip's pair_device_refusal does for the fp32 forms
// (which ssrhip_gemv_pair_applicable has asked before this is reached: CU count and CU masks are its part).
const char* w8_pair_device_refusal() {
  static const char* verdict = nullptr;
  static bool asked = false;
  if (asked) return verdict;
  asked = true;
  static char buf[200];
  int nb[5] = {0, 0, 0, 0, 0};
  hipError_t e0 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb[0], w8_pair_kernel<4>, PAIR_TH, 0);
  hipError_t e1 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb[1], w8_pair_kernel<6>, PAIR_TH, 0);
  hipError_t e2 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb[2], w8_pair_kernel<8>, PAIR_TH, 0);
  hipError_t e3 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb[3], w8_pair_merge_kernel<8, 2>, PAIR_TH, 16 * 1024);
  hipError_t e4 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb[4], w8_pair_merge_kernel<8, 0>, PAIR_TH, 16 * 1024);
  if (e0 != hipSuccess || e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess || nb[0] < 1 || nb[1] < 1 || nb[2] < 1 || nb[3] < 1 || nb[4] < 1) {
    snprintf(buf, sizeof(buf), "the occupancy calculator places %d / %d / %d / %d / %d workgroups of the e4m3 pair kernels on a CU (need >= 1 each)", nb[0], nb[1], nb[2], nb[3], nb[4]);
    return verdict = buf;
  }
  return verdict = nullptr;
}

// ssrhip_gemv_pair_applicable (shapes, >= 256 CUs, no CU mask, SSRHIP_GEMV_PAIR) AND ssrhip_gemv_w8_applicable for both launches
// (SSRHIP_GEMV_SEG=0 turns it off) AND a CU takes every instantiation
bool w8_pair_qualifies(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b) {
  auto no = [](const char* why) { snprintf(g_w8_pair_why, sizeof(g_w8_pair_why), "%s", why); return false; };
  if (!ssrhip_gemv_pair_applicable(a, b)) return no(ssrhip_gemv_pair_why());
  if (!ssrhip_gemv_w8_applicable(a) || !ssrhip_gemv_w8_applicable(b)) return no("the e4m3 weight stream does not take these launches (ssrhip_gemv_w8_applicable; SSRHIP_GEMV_SEG=0 turns it off)");
  if (const char* why = w8_pair_device_refusal()) return no(why);
  g_w8_pair_why[0] = 0;
  return true;
}

}  // namespace

const char* ssrhip_gemv_pair_w8_why() { return g_w8_pair_why; }   // why the last question on this thread was answered with no (engine.hip reports it)

extern "C" int ssrhip_gemv_pair_w8_applicable(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b) {
  if (!a || !b) return 0;
  return w8_pair_qualifies(a, b) ? 1 : 0;
}

extern "C" int ssrhip_gemv_pair_w8(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, const uint8_t* Wa8, const float* scale_a, const uint8_t* Wb8,
                                   const float* scale_b, void* ws, int32_t buf, int32_t buf_next, ssrhip_stream_t stream) {
  SSR_REQUIRE(a && b && Wa8 && scale_a && Wb8 && scale_b && ws, "ssrhip_gemv_pair_w8: null argument");
  SSR_REQUIRE(buf >= 0 && buf < 3 && buf_next >= 0 && buf_next < 3 && buf != buf_next, "ssrhip_gemv_pair_w8: granule buffers %d -> %d (0..2, different)", buf, buf_next);
  SSR_REQUIRE(a->epi != SSRHIP_EPI_QKV_APPEND16 && b->epi != SSRHIP_EPI_QKV_APPEND16, "ssrhip_gemv_pair_w8: the 2-byte KV append (EPI_QKV_APPEND16) exists for 5..32 rows only");
  if (!w8_pair_qualifies(a, b)) return 1;
  // what pair_nuwb (gemv.hip) derived for the pair it accepted
  const bool merge = a->pro == SSRHIP_PRO_ATTN_COMBINE;
  const int nuwb = (b->N / 256) * 2 / SEG_NW;
  W8PairK q;
  PairK& p = q.k;
  seg_fill(&p.a, a, merge ? 2 : 8, 256);                            // one workgroup per CU: 8 rows of A, N / 256 rows of B
  seg_fill(&p.b, b, 2, 256);
  unsigned long long* gran = (unsigned long long*)ws;
  p.gran = gran + (size_t)buf * PAIR_GRAN;
  p.gran_next = gran + (size_t)buf_next * PAIR_GRAN;
  p.gave_up = (int*)(gran + 3 * (size_t)PAIR_GRAN);
  q.Wa8 = Wa8;
  q.sa = scale_a;
  q.Wb8 = Wb8;
  q.sb = scale_b;
  hipStream_t s = (hipStream_t)stream;
  if (merge) {
    const size_t sm = ((size_t)2 * (a->K / a->kv.head_dim) * a->max_splits * sizeof(float) + 15) / 16 * 16;
    const char* ee = getenv("SSRHIP_GEMV_PAIR_EARLY");             // read at every call (graph capture), as on the fp32 and bf16 forms
    if (ee && ee[0] == '0') hipLaunchKernelGGL((w8_pair_merge_kernel<8, 0>), dim3(256), dim3(PAIR_TH), sm, s, q);
    else hipLaunchKernelGGL((w8_pair_merge_kernel<8, 2>), dim3(256), dim3(PAIR_TH), sm, s, q);
  } else if (nuwb == 4) hipLaunchKernelGGL((w8_pair_kernel<4>), dim3(256), dim3(PAIR_TH), 0, s, q);
  else if (nuwb == 6) hipLaunchKernelGGL((w8_pair_kernel<6>), dim3(256), dim3(PAIR_TH), 0, s, q);
  else hipLaunchKernelGGL((w8_pair_kernel<8>), dim3(256), dim3(PAIR_TH), 0, s, q);
  SSR_LAUNCH_CHECK();
  return 0;
}
