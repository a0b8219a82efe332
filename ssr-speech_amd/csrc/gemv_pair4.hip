// gemv_pair4.hip — pair launches of the 4-row decode step (two utterances x CFG, or four without), fp32 weights, gfx950.
//
// gemv.hip's pair launches (gemv_pair_kernel / gemv_pair_merge_kernel: TWO consecutive GEMVs of the step in ONE launch, the all-to-all edge
// between them inside the launch) at four batch rows. Same structure: 256 workgroups, one per CU, 8 streaming waves + 4 edge waves, the two
// roles the two arms of ONE wave-uniform branch with every barrier written in both arms; the hand-off is gemv_pair.h's protocol with
// 8192 granules per buffer (gemv_pair4.h). Two forms:
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
#include "gemv_pair4.h"

namespace {

constexpr int PAIR4_DEPTH = 4;   // units in the ring of a streaming wave
constexpr int PAIR4_PF = 3;      // of B's first units, those posted behind barrier (1b), in front of the gather's loads (gemv.hip: PAIR_PF)

// ---- the streaming role from barrier (1) on: B = LayerNorm + Linear on x' (gemv_seg_kernel<4, PRO_LAYERNORM, false>, operation for operation)
template <int NUWB>
__device__ __forceinline__ void pair4_stream_b(const PairK& p, int t, int lane, int wave, float4 (&xr)[PAIR4_B][4], float4 (&w)[PAIR4_DEPTH][4],
                                               const RowEpi& efinB, float* partB, float* aux, const float* xs, const size_t* kvoff) {
  constexpr int B = PAIR4_B, DEPTH = PAIR4_DEPTH, PF = (PAIR4_PF < NUWB ? PAIR4_PF : NUWB), SB = 2, SHB = 1, RB = NUWB * SEG_NW / SB;
  static_assert(DEPTH <= NUWB, "units in flight");
  const ssrhip_gemv_args& bb = p.b.a;
  const int rB0 = (int)blockIdx.x * RB, segB = wave & (SB - 1);
  const int bfin = t % B, rfinB = min(t / B, RB - 1), nfinB = rB0 + rfinB;
  const float* WgB = bb.W + (size_t)rB0 * bb.K + segB * SEG + lane * 4;
  __syncthreads();                                                  // (1b) wave 8 has issued the publish
  // B's first units: PF of them now, the rest behind the gather
#pragma unroll
  for (int j = 0; j < PF; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) w[j % DEPTH][i] = ld_nt(WgB + (size_t)((wave + SEG_NW * j) >> SHB) * bb.K + i * 256);
  __syncthreads();                                                  // (2) x' is in LDS
  seg_load_x<B>(xr, xs, PAIR_D, segB, lane);
#pragma unroll
  for (int j = PF; j < DEPTH; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) w[j % DEPTH][i] = ld_nt(WgB + (size_t)((wave + SEG_NW * j) >> SHB) * bb.K + i * 256);
  seg_layernorm<B>(xr, aux, SB, bb.K, bb.ln_eps, wave, lane);       // its barrier is (3)
  // units
#pragma unroll
  for (int j = 0; j < NUWB; ++j) {
    float4 (&wj)[4] = w[j % DEPTH];
    float acc[B][2];
#pragma unroll
    for (int b = 0; b < B; ++b) acc[b][0] = acc[b][1] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int b = 0; b < B; ++b) acc[b][i & 1] = dot4(wj[i], xr[b][i], acc[b][i & 1]);
      if (j + DEPTH < NUWB) {
        __builtin_amdgcn_sched_barrier(0);
        wj[i] = ld_nt(WgB + (size_t)((wave + SEG_NW * (j + DEPTH)) >> SHB) * bb.K + i * 256);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    seg_park<B>(acc, partB, wave + SEG_NW * j, lane);
  }
  __syncthreads();                                                  // (4)
  if (t < RB * B) {
    // K / V append addresses: resolved by the edge role (wave 9) while this role streamed
    float* kvb[2] = {bb.kv.pool + kvoff[bfin * 2], bb.kv.pool + kvoff[bfin * 2 + 1]};
    seg_finish_row<B>(p.b, 0, partB, SB, rfinB, nfinB, bfin, efinB, kvb);
  }
}

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
#pragma unroll
    for (int j = 0; j < DEPTH; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) w[j][i] = ld_nt(WgA + (size_t)((wave + SEG_NW * j) >> SHA) * a.K + i * 256);
    // ---- 2. A's units
#pragma unroll
    for (int j = 0; j < NUWA; ++j) {
      float4 (&wj)[4] = w[j % DEPTH];
      float acc[B][2];
#pragma unroll
      for (int b = 0; b < B; ++b) acc[b][0] = acc[b][1] = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int b = 0; b < B; ++b) acc[b][i & 1] = dot4(wj[i], xr[b][i], acc[b][i & 1]);
        if (j + DEPTH < NUWA) {
          __builtin_amdgcn_sched_barrier(0);
          wj[i] = ld_nt(WgA + (size_t)((wave + SEG_NW * (j + DEPTH)) >> SHA) * a.K + i * 256);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      seg_park<B>(acc, partA, wave + SEG_NW * j, lane);
    }
    __syncthreads();                                                // (1) A's partial sums are parked
    pair4_stream_b<NUWB>(p, t, lane, wave, xr, w, efinB, partB, aux, xs, kvoff);
  } else {
    pair4_edge_role<SA, 0>(p, wave - SEG_NW, lane, partA, xs, kvoff);
  }
}

// A = split-KV merge + out-projection + residual (K = 2048): gemv_seg_kernel<4, PRO_ATTN_COMBINE, false> at one workgroup per CU, operation
// for operation — thread t owns float4 column t * 4 of the four rows in the merge (SegCS<4> = 2 pages prefetched, the rest loaded late),
// wave w the units w and w + 8 (both requested at entry). The merged rows pass through the LDS buffer that later receives x' (its A-phase
// use ends before barrier (1)). No early units of B: the ring's four slots and x of four rows leave no registers for them.
template <int NUWB>
__global__ __launch_bounds__(PAIR_TH) void pair4_merge_kernel(const PairK p) {
  constexpr int B = PAIR4_B, DEPTH = PAIR4_DEPTH, SEG_CS = SegCS<B>::v;
  constexpr int RA = 8, SA = 2, SHA = 1;                           // A: 8 rows per workgroup, K = 2048 = 2 segments, 16 units = 2 per wave
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
    pair4_edge_role<SA, 2>(p, wave - SEG_NW, lane, partA, xs, kvoff);
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
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) w[j][i] = ld_nt(WgA + (size_t)((wave + SEG_NW * j) >> SHA) * K + i * 256);
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
    // ---- 4. A's two units
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
    pair4_stream_b<NUWB>(p, t, lane, wave, xr, w, efinB, partB, aux, xs, kvoff);
  }
}

constexpr size_t PAIR4_WTAB_MAX = 16 * 1024;   // merge weights in dynamic LDS, next to ~34 KB of static buffers

thread_local char g_pair4_why[200] = "";

// Can a CU take a workgroup of every 4-row instantiation (12 waves, their registers and 33-50 KB of LDS)? Asked once per process, as
// gemv.hip's pair_device_refusal does for the 2-row forms (CU count and CU masks are its part: ssrhip_gemv_pair_applicable asks them first).
const char* pair4_device_refusal() {
  static const char* verdict = nullptr;
  static bool asked = false;
  if (asked) return verdict;
  asked = true;
  static char buf[200];
  int nb[4] = {0, 0, 0, 0};
  hipError_t e0 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb[0], pair4_kernel<4>, PAIR_TH, 0);
  hipError_t e1 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb[1], pair4_kernel<6>, PAIR_TH, 0);
  hipError_t e2 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb[2], pair4_kernel<8>, PAIR_TH, 0);
  hipError_t e3 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb[3], pair4_merge_kernel<8>, PAIR_TH, PAIR4_WTAB_MAX);
  if (e0 != hipSuccess || e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || nb[0] < 1 || nb[1] < 1 || nb[2] < 1 || nb[3] < 1) {
    snprintf(buf, sizeof(buf), "the occupancy calculator places %d / %d / %d / %d workgroups of the 4-row pair kernels on a CU (need >= 1 each)", nb[0], nb[1], nb[2], nb[3]);
    return verdict = buf;
  }
  return verdict = nullptr;
}

// ssrhip_gemv_pair_applicable's rules with B == 4: the 2-row question is put with the row count set to 2 (shapes, >= 256 CUs, no CU mask,
// SSRHIP_GEMV_PAIR = 0 / 1 / 2), then what four rows change — the merge's (row, head) table and its LDS — and the occupancy of the new kernels
bool pair4_qualifies(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b) {
  auto no = [](const char* why) { snprintf(g_pair4_why, sizeof(g_pair4_why), "%s", why); return false; };
  if (a->B != PAIR4_B || b->B != PAIR4_B) return no("not a 4-row launch (the 4-row pair kernels take B = 4 only)");
  ssrhip_gemv_args a2 = *a, b2 = *b;
  a2.B = b2.B = 2;
  if (!ssrhip_gemv_pair_applicable(&a2, &b2)) return no(ssrhip_gemv_pair_why());
  if (a->pro == SSRHIP_PRO_ATTN_COMBINE) {
    const int H = a->K / a->kv.head_dim;
    if (PAIR4_B * H > SEG_TH) return no("merge form: more than 512 (row, head) pairs");
    if ((size_t)PAIR4_B * H * a->max_splits * sizeof(float) > PAIR4_WTAB_MAX) return no("merge weights exceed 16 KB of LDS (context too long for the 4-row merge form)");
  }
  if (const char* why = pair4_device_refusal()) return no(why);
  g_pair4_why[0] = 0;
  return true;
}

}  // namespace

const char* ssrhip_gemv_pair4_why() { return g_pair4_why; }   // why the last question on this thread was answered with no (engine.hip reports it)

extern "C" int ssrhip_gemv_pair4_applicable(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b) {
  if (!a || !b) return 0;
  return pair4_qualifies(a, b) ? 1 : 0;
}

extern "C" int ssrhip_gemv_pair4(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, void* ws, int32_t buf, int32_t buf_next, ssrhip_stream_t stream) {
  SSR_REQUIRE(a && b && ws, "ssrhip_gemv_pair4: null argument");
  SSR_REQUIRE(buf >= 0 && buf < 3 && buf_next >= 0 && buf_next < 3 && buf != buf_next, "ssrhip_gemv_pair4: granule buffers %d -> %d (0..2, different)", buf, buf_next);
  SSR_REQUIRE(a->epi != SSRHIP_EPI_QKV_APPEND16 && b->epi != SSRHIP_EPI_QKV_APPEND16, "ssrhip_gemv_pair4: the 2-byte KV append (EPI_QKV_APPEND16) exists for 5..32 rows only");
  if (!pair4_qualifies(a, b)) return 1;
  const bool merge = a->pro == SSRHIP_PRO_ATTN_COMBINE;
  const int nuwb = (b->N / 256) * 2 / SEG_NW;
  PairK p;
  seg_fill(&p.a, a, merge ? 2 : 8, 256);                            // one workgroup per CU: 8 rows of A, N / 256 rows of B
  seg_fill(&p.b, b, 2, 256);
  unsigned long long* gran = (unsigned long long*)ws;
  p.gran = gran + (size_t)buf * PAIR4_GRAN;
  p.gran_next = gran + (size_t)buf_next * PAIR4_GRAN;
  p.gave_up = (int*)(gran + 3 * (size_t)PAIR4_GRAN);
  hipStream_t s = (hipStream_t)stream;
  if (merge) {
    const size_t sm = ((size_t)PAIR4_B * (a->K / a->kv.head_dim) * a->max_splits * sizeof(float) + 15) / 16 * 16;
    hipLaunchKernelGGL((pair4_merge_kernel<8>), dim3(256), dim3(PAIR_TH), sm, s, p);
  } else if (nuwb == 4) hipLaunchKernelGGL((pair4_kernel<4>), dim3(256), dim3(PAIR_TH), 0, s, p);
  else if (nuwb == 6) hipLaunchKernelGGL((pair4_kernel<6>), dim3(256), dim3(PAIR_TH), 0, s, p);
  else hipLaunchKernelGGL((pair4_kernel<8>), dim3(256), dim3(PAIR_TH), 0, s, p);
  SSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssrhip_gemv_pair4_status(const void* ws, ssrhip_stream_t stream) {
  SSR_REQUIRE(ws, "ssrhip_gemv_pair4_status: null workspace");
  int flag = 0;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) { ssrhip_set_error("ssrhip_gemv_pair4_status: stream synchronize failed"); return -1; }
  if (hipMemcpy(&flag, (const char*)ws + 3 * (size_t)PAIR4_GRAN * 8, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
    ssrhip_set_error("ssrhip_gemv_pair4_status: copy failed");
    return -1;
  }
  if (flag) {   // reported once; tags and flag back to "nothing published" (ssrhip_gemv_pair_status, at this workspace's size)
    if (hipMemset(const_cast<void*>(ws), 0, SSRHIP_PAIR4_WS_BYTES) != hipSuccess) { ssrhip_set_error("ssrhip_gemv_pair4_status: re-zeroing the workspace failed"); return -1; }
  }
  return flag ? 1 : 0;
}
