// gemv_w8.hip — the <= 4-row weight-streaming GEMV of gemv.hip over PACKED OCP e4m3 CODES with one power-of-two scale per output row (the
// opt-in e4m3 weight stream of the decode step; DESIGN.md Part I.18), gfx950.
//
//   y[b][n] = epi( s[n] * sum_k pro(x)[b][k] * float(q[n][k]) + bias[n] ),   s[n] = 2^e(n)
//
// The step is HBM-bound on its weights; a 1-byte weight halves the bytes of the bf16 stream (gemv_w16.hip). e4m3 -> fp32 is exact
// (v_cvt_pk_f32_fp8, two codes per instruction), and a multiplication by a power of two commutes with every fp32 rounding as long as no
// intermediate value is subnormal or overflows. So a kernel that widens the codes in registers, runs the SAME fmaf sequence, wave_sum and
// k-ordered sum over segments as the fp32 kernel, and multiplies each (row, segment) partial sum by s[n] where it is parked in LDS, is
// bit-identical to the fp32 kernel run on the masters q * 2^e (what every other path of an e4m3 model reads). The caveat is real: a partial
// sum below 2^-126 / s, or a master that is itself subnormal, rounds differently on the two sides; weights and activations of a network
// are nowhere near it. The multiply is a plain multiply (the library is built with -ffp-contract=off). Activations, biases, accumulation,
// LayerNorm statistics, the split-KV merge and every epilogue stay fp32 and are the code of csrc/gemv_shared.h, untouched.
//
// Layout (include/ssrhip.h SSRHIP_W8_INDEX): the unit of work is the fp32 kernels' (row, 1024-element segment of K) = 1 KiB = ONE wave-level
// load; lane l's 16 bytes hold that lane's four float4 of the fp32 kernel in order (dword i = elements i * 256 + 4l .. 4l + 3 of the
// segment) — after widening the lane owns the same pieces of x, xr[b][0..3], as in gemv_seg_kernel / gemv_segu_kernel.
//
// Two kernels, the two forms of gemv_w16.hip:
//   w8_segu_kernel  one 8-wave workgroup per CU, NUW units per wave as straight-line code, DEPTH of them in flight;
//   w8_seg_kernel   the generic form: balanced contiguous rows per workgroup, ragged tails, groups, the split-KV merge prologue.
// Streaming discipline as in DESIGN.md I.2: every weight load is unconditional inside its block and countable, re-requests overwrite a
// used piece in place, no predicated loads. A row's scale is requested just BEFORE the row's codes, so that it is the older load and
// waiting for it never drains the ring. The VALU cost of widening is 8 conversions per 1 KiB unit and lane, beside 16 * B FMAs.
// No v_dot2-like form: it would round x and break the arithmetic contract.
#include <stdlib.h>
#include "common.h"
#include "gemv_shared.h"
#include "gemv_wstream.h"

namespace {

struct W8K {
  GemvK k;
  const uint8_t* W8;     // [groups][N][K] codes in SSRHIP_W8_INDEX order
  const float* scale;    // [groups][N]: 2^e of each output row
};

constexpr int W8_RING = 4;   // units in flight per wave in the generic form: 4 KiB, the bytes of w16_seg_kernel's ring of two

// ---------------------------------------------------------------------------------------------------------------
// The generic segment form (gemv_seg_kernel / w16_seg_kernel): 512-thread workgroups, each owning a contiguous block of rows; wave w works
// on segment w % S and on the units w, w + 8, w + 16, ... of its workgroup. A wave keeps W8_RING units in flight, all requested at kernel
// entry (clamped to the workgroup's last unit). Re-requests happen in place, in blocks that are entered only when the successor unit
// exists — none is wasted, none is predicated.
template <int B, int PRO>
__global__ __launch_bounds__(SEG_TH, (PRO == SSRHIP_PRO_ATTN_COMBINE) ? 2 : 4) void w8_seg_kernel(const W8K q) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int SEG_CS = SegCS<B>::v;
  const GemvK& p = q.k;
  const ssrhip_gemv_args& a = p.a;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int g = blockIdx.y;
  const int K = a.K, N = a.N, S = p.nslice;
  const int r0 = (int)blockIdx.x * p.rows_per + min((int)blockIdx.x, p.rows_rem);
  const int nrows = p.rows_per + ((int)blockIdx.x < p.rows_rem ? 1 : 0), nu = nrows * S;      // host guarantees N >= G: nrows >= 1
  const int seg = wave & (S - 1), sh = p.seg_shift;
  float* part = smem;                                              // [rows_max][S][B]
  float* aux = smem + p.rows_max * S * B;                          // prologue scratch
  const uint8_t* Wg = q.W8 + ((size_t)g * N + r0) * K + seg * SEG + lane * 16;   // unit of local row c: + c * K
  const float* Sg = q.scale + (size_t)g * N + r0;                  // scale of local row c: Sg[c]

  // ---- 0. epilogue operands of the (row, b) this thread finalises: the wave's oldest loads (see gemv_seg_kernel)
  const int bfin = t % B, rfin = min(t / B, nrows - 1), nfin = r0 + rfin;
  const RowEpi efin = seg_epi_fetch(a, g, nfin, bfin);
  // ---- 1. activations (L2)
  float4 xr[B][4];
  float4 co[(PRO == SSRHIP_PRO_ATTN_COMBINE) ? B : 1][SEG_CS];
  float2 cml[SEG_CS];
  int ns[(PRO == SSRHIP_PRO_ATTN_COMBINE) ? B : 1];
  if constexpr (PRO != SSRHIP_PRO_ATTN_COMBINE) {
    seg_load_x<B>(xr, a.x + (size_t)g * K, (size_t)a.x_stride, seg, lane);
  } else {                                                         // K == 2048: thread t owns float4 column t * 4 of every row
    const int hd = p.hd, H = K / hd, MS = a.max_splits;
#pragma unroll
    for (int b = 0; b < B; ++b) ns[b] = (a.row_len[b] + SSRHIP_PAGE - 1) / SSRHIP_PAGE;
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
  // ---- 2. the wave's first W8_RING units, unconditional (clamped to the workgroup's last unit); each row's scale ahead of its codes
  w8_v4u w[W8_RING];
  float sc[W8_RING];
  int u = wave;
#pragma unroll
  for (int j = 0; j < W8_RING; ++j) {
    const int c = min(u + SEG_NW * j, nu - 1) >> sh;
    sc[j] = Sg[c];
    w[j] = ld16_nt(Wg + (size_t)c * K);
  }
  float* kvb[2] = {nullptr, nullptr};
  if (a.epi == SSRHIP_EPI_QKV_APPEND) kv_append_bases<B>(a, bfin, kvb);
  // ---- 3. prologue math, under the latency of the first units
  if constexpr (PRO == SSRHIP_PRO_LAYERNORM) seg_layernorm<B>(xr, aux, S, K, a.ln_eps, wave, lane);
  if constexpr (PRO == SSRHIP_PRO_ATTN_COMBINE) {                  // gemv_seg_kernel's merge, operation for operation (written out: see the note there)
    const int hd = p.hd, H = K / hd, MS = a.max_splits;
    float* xs = aux;                                               // [B][K]
    float* wtab = aux + B * K;                                     // [B*H][MS]
    if (t < B * H) {
      const int n = ns[t / H];
      const float* ml = a.part_ml + (size_t)t * MS * 2;
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
        if (i < n) wtab[t * MS + i] = expf(cml[i].x - M) * inv;
      for (int s2 = SEG_CS; s2 < n; ++s2) wtab[t * MS + s2] = expf(ld2_late(ml + 2 * s2).x - M) * inv;
    }
    __syncthreads();
    const int e = t * 4, h = e / hd, d = e % hd;
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const float* wt = wtab + (b * H + h) * MS;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int s2 = 0; s2 < SEG_CS; ++s2) {
        const bool in = s2 < ns[b];                                   // a page beyond the row must not count (0 * NaN)
        const float ws = in ? wt[s2] : 0.f;
        acc.x = fmaf(ws, in ? co[b][s2].x : 0.f, acc.x);
        acc.y = fmaf(ws, in ? co[b][s2].y : 0.f, acc.y);
        acc.z = fmaf(ws, in ? co[b][s2].z : 0.f, acc.z);
        acc.w = fmaf(ws, in ? co[b][s2].w : 0.f, acc.w);
      }
      const float* po = a.part_o + (((size_t)b * H + h) * MS) * hd + d;
      for (int s2 = SEG_CS; s2 < ns[b]; ++s2) {                    // contexts beyond the prefetched pages: the rest, loaded late
        const float ws = wt[s2];
        const float4 o = ld4_late(po + (size_t)s2 * hd);
        acc.x = fmaf(ws, o.x, acc.x);
        acc.y = fmaf(ws, o.y, acc.y);
        acc.z = fmaf(ws, o.z, acc.z);
        acc.w = fmaf(ws, o.w, acc.w);
      }
      *reinterpret_cast<float4*>(xs + b * K + e) = acc;
    }
    __syncthreads();
    seg_load_x<B>(xr, xs, K, seg, lane);
  }
  // ---- 4. stream the units through the ring
  // unit `un` sits in slot j; when `next` >= 0 the slot is re-requested for unit `next` right after its use, in place (scale first)
  auto unit = [&](w8_v4u& wj, float& scj, int un, int next) {
    float acc[B][2];
#pragma unroll
    for (int b = 0; b < B; ++b) acc[b][0] = acc[b][1] = 0.f;
    w8_unit<B>(wj, xr, acc);
    const float s_now = scj;
    if (next >= 0) {
      const int c = next >> sh;
      __builtin_amdgcn_sched_barrier(0);                            // use, THEN overwrite in place
      scj = Sg[c];
      wj = ld16_nt(Wg + (size_t)c * K);
      __builtin_amdgcn_sched_barrier(0);
    }
    w8_park<B>(acc, s_now, part, un, lane);
  };
  while (u + (2 * W8_RING - 1) * SEG_NW < nu) {                     // every ring slot has a successor
#pragma unroll
    for (int j = 0; j < W8_RING; ++j) unit(w[j], sc[j], u + SEG_NW * j, u + SEG_NW * (j + W8_RING));
    u += W8_RING * SEG_NW;
  }
#pragma unroll
  for (int j = 0; j < W8_RING; ++j) {                               // at most 2 * W8_RING - 1 units left: the first slots are refilled once
    const int un = u + SEG_NW * j, nx = un + SEG_NW * W8_RING;
    if (un < nu) {
      if (nx < nu) unit(w[j], sc[j], un, nx);
      else unit(w[j], sc[j], un, -1);
    }
  }
#pragma unroll
  for (int j = 0; j < W8_RING - 1; ++j) {
    const int un = u + SEG_NW * (j + W8_RING);
    if (un < nu) unit(w[j], sc[j], un, -1);
  }
  __syncthreads();
  if (t < nrows * B) seg_finish_row<B>(p, g, part, S, rfin, nfin, bfin, efin, kvb);
}

// ---------------------------------------------------------------------------------------------------------------
// The straight-line form (gemv_segu_kernel / w16_segu_kernel): ONE 8-wave workgroup per CU, NUW units per wave known at compile time, DEPTH
// units (KiB) in flight per wave, a unit's 16-byte piece re-requested for unit j + DEPTH right after unit j used it. With DEPTH = NUW every
// unit is requested at kernel entry and the loop has no re-request at all. The NUW scales of the wave's rows are requested at entry, ahead
// of the codes. Measured (DESIGN.md Part I.18, profiles/w8_launch_bench_rows*.json, profiles/w8_decode_ab_830m.log): a ring of 4 units is
// the fastest at 1 and 2 rows (LN + QKV 6.34 us against 6.55 for 2 and 6.57 for every unit), rings of 2 and 4 tie at 4 rows, every unit at
// entry loses everywhere. Defaults: 4 at 1 and 2 rows, 2 at 4 rows; all three stay instantiated behind SSRHIP_GEMV_W8_DEPTH for re-measuring.
template <int B, int PRO, int NUW, int DEPTH>
__global__ __launch_bounds__(SEG_TH, 2) void w8_segu_kernel(const W8K q) {
  static_assert(PRO == SSRHIP_PRO_NONE || PRO == SSRHIP_PRO_LAYERNORM, "the split-KV merge prologue stays on w8_seg_kernel");
  static_assert(DEPTH >= 1 && DEPTH <= NUW, "units in flight");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const GemvK& p = q.k;
  const ssrhip_gemv_args& a = p.a;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int g = blockIdx.y;
  const int K = a.K, N = a.N, S = p.nslice, sh = p.seg_shift;
  const int nrows = p.rows_per;                                    // exact: the host takes this kernel only when N % G == 0
  const int r0 = (int)blockIdx.x * nrows;
  const int seg = wave & (S - 1);
  float* part = smem;                                              // [nrows][S][B]
  float* aux = smem + nrows * S * B;                               // LayerNorm statistics of the S segments
  const uint8_t* Wg = q.W8 + ((size_t)g * N + r0) * K + seg * SEG + lane * 16;
  const float* Sg = q.scale + (size_t)g * N + r0;

  const int bfin = t % B, rfin = min(t / B, nrows - 1), nfin = r0 + rfin;
  const RowEpi efin = seg_epi_fetch(a, g, nfin, bfin);
  float4 xr[B][4];
  seg_load_x<B>(xr, a.x + (size_t)g * K, (size_t)a.x_stride, seg, lane);
  float sc[NUW];
#pragma unroll
  for (int j = 0; j < NUW; ++j) sc[j] = Sg[(wave + SEG_NW * j) >> sh];
  w8_v4u w[DEPTH];
#pragma unroll
  for (int j = 0; j < DEPTH; ++j) w[j] = ld16_nt(Wg + (size_t)((wave + SEG_NW * j) >> sh) * K);
  float* kvb[2] = {nullptr, nullptr};
  if (a.epi == SSRHIP_EPI_QKV_APPEND) kv_append_bases<B>(a, bfin, kvb);
  if constexpr (PRO == SSRHIP_PRO_LAYERNORM) seg_layernorm<B>(xr, aux, S, K, a.ln_eps, wave, lane);
#pragma unroll
  for (int j = 0; j < NUW; ++j) {
    w8_v4u& wj = w[j % DEPTH];
    float acc[B][2];
#pragma unroll
    for (int b = 0; b < B; ++b) acc[b][0] = acc[b][1] = 0.f;
    w8_unit<B>(wj, xr, acc);
    if (j + DEPTH < NUW) {
      __builtin_amdgcn_sched_barrier(0);
      wj = ld16_nt(Wg + (size_t)((wave + SEG_NW * (j + DEPTH)) >> sh) * K);
      __builtin_amdgcn_sched_barrier(0);
    }
    w8_park<B>(acc, sc[j], part, wave + SEG_NW * j, lane);          // unit u = local_row * S + seg
  }
  __syncthreads();
  if (t < nrows * B) seg_finish_row<B>(p, g, part, S, rfin, nfin, bfin, efin, kvb);
}

// Does `a` qualify, i.e. would ssrhip_gemv take it with its segment kernels? The rule of ssrhip_gemv_w16 (gemv_w16.hip w16_plan).
bool w8_plan(const ssrhip_gemv_args* a, int num_cu, SegPlan* pl) {
  const char* why;
  if (a->B != 1 && a->B != 2 && a->B != 4) return false;
  if (a->x_tiled || a->y_tiled || a->w_tiled) return false;          // tiled layouts are for 5..32 rows
  if (!seg_plan(a, num_cu, false, pl, &why)) return false;           // one workgroup per CU behind the merge prologue, always
  if (const char* e = getenv("SSRHIP_GEMV_SEG")) if (e[0] == '0') return false;
  return true;
}

template <int B>
void w8_launch(const SegPlan& pl, const uint8_t* W8, const float* scale, hipStream_t s) {
  const ssrhip_gemv_args* a = &pl.k.a;
  W8K q;
  q.k = pl.k;
  q.W8 = W8;
  q.scale = scale;
  // one workgroup per CU, NUW units per wave straight-line, when the shape divides evenly (the shapes gemv_segu_kernel takes at 2 rows)
  int depth = (B == 4) ? 2 : 4;                                     // SSRHIP_GEMV_W8_DEPTH = 2 | 4 (default: 4, 2 at 4 rows): units in flight per wave; 8: every unit
  if (const char* e = getenv("SSRHIP_GEMV_W8_DEPTH")) depth = atoi(e);    // at entry; 0: never this form. Read at every call.
  if (depth != 0 && pl.segu_nuw) {
    const int nuw = pl.segu_nuw;
    seg_fill(&q.k, a, pl.k.nslice, pl.segu_G1);
    const size_t sm = pl.segu_smem;
    const dim3 g1(pl.segu_G1, a->groups);
#define W8U_LAUNCH(PRO_, NUW_)                                                                                                        \
    do {                                                                                                                               \
      if (depth == 2) hipLaunchKernelGGL((w8_segu_kernel<B, PRO_, NUW_, 2>), g1, dim3(SEG_TH), sm, s, q);                               \
      else if (depth == 8) hipLaunchKernelGGL((w8_segu_kernel<B, PRO_, NUW_, NUW_>), g1, dim3(SEG_TH), sm, s, q);                       \
      else hipLaunchKernelGGL((w8_segu_kernel<B, PRO_, NUW_, 4>), g1, dim3(SEG_TH), sm, s, q);                                          \
    } while (0)
    if (a->pro == SSRHIP_PRO_LAYERNORM) {
      if (nuw == 4) W8U_LAUNCH(SSRHIP_PRO_LAYERNORM, 4); else if (nuw == 6) W8U_LAUNCH(SSRHIP_PRO_LAYERNORM, 6); else W8U_LAUNCH(SSRHIP_PRO_LAYERNORM, 8);
    } else {
      if (nuw == 4) W8U_LAUNCH(SSRHIP_PRO_NONE, 4); else if (nuw == 6) W8U_LAUNCH(SSRHIP_PRO_NONE, 6); else W8U_LAUNCH(SSRHIP_PRO_NONE, 8);
    }
#undef W8U_LAUNCH
    return;
  }
  const dim3 grid(pl.G, a->groups);
  switch (a->pro) {
    case SSRHIP_PRO_LAYERNORM: hipLaunchKernelGGL((w8_seg_kernel<B, SSRHIP_PRO_LAYERNORM>), grid, dim3(SEG_TH), pl.smem, s, q); break;
    case SSRHIP_PRO_ATTN_COMBINE: hipLaunchKernelGGL((w8_seg_kernel<B, SSRHIP_PRO_ATTN_COMBINE>), grid, dim3(SEG_TH), pl.smem, s, q); break;
    default: hipLaunchKernelGGL((w8_seg_kernel<B, SSRHIP_PRO_NONE>), grid, dim3(SEG_TH), pl.smem, s, q); break;
  }
}

}  // namespace

extern "C" int ssrhip_gemv_w8_applicable(const ssrhip_gemv_args* a) {
  SegPlan pl;
  return (a && w8_plan(a, ssr_num_cu(), &pl)) ? 1 : 0;
}

extern "C" int ssrhip_gemv_w8(const ssrhip_gemv_args* a, const uint8_t* W8, const float* scale, ssrhip_stream_t stream) {
  SSR_REQUIRE(a && a->W && a->y && W8 && scale, "ssrhip_gemv_w8: null argument");
  SSR_REQUIRE(a->N > 0 && a->groups >= 1 && a->K > 0, "ssrhip_gemv_w8: bad N/K/groups");
  SSR_REQUIRE(a->B == 1 || a->B == 2 || a->B == 4, "ssrhip_gemv_w8: B=%d not in {1,2,4} (the e4m3 weight stream exists for the <= 4-row step only)", a->B);
  if (int rc = gemv_small_check(a, "ssrhip_gemv_w8")) return rc;    // the contract of ssrhip_gemv: what it would refuse is refused here too
  SegPlan pl;
  if (!w8_plan(a, ssr_num_cu(), &pl)) return 1;
  hipStream_t s = (hipStream_t)stream;
  switch (a->B) {
    case 1: w8_launch<1>(pl, W8, scale, s); break;
    case 2: w8_launch<2>(pl, W8, scale, s); break;
    default: w8_launch<4>(pl, W8, scale, s); break;
  }
  SSR_LAUNCH_CHECK();
  return 0;
}
