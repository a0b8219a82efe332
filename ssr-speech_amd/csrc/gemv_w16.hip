// gemv_w16.hip — the <= 4-row weight-streaming GEMV of gemv.hip over PACKED bf16 WEIGHTS (the opt-in bf16 weight stream of the decode
// step; DESIGN.md Part I.10), gfx950.
//
//   y[b][n] = epi( sum_k pro(x)[b][k] * float(W16[n][k]) + bias[n] )
//
// The step is HBM-bound on its weights; a 2-byte weight halves the bytes. bf16 -> fp32 is a 16-bit shift and exact, so a kernel that
// streams the packed weights, widens them in registers and then runs the SAME fmaf sequence in the SAME order as the fp32 kernel is
// bit-identical to the fp32 kernel run on the rounded weights (the fp32 "masters" every other path of a bf16 model reads). Activations,
// biases, accumulation, LayerNorm statistics, the split-KV merge and every epilogue stay fp32 and are the code of gemv.hip, operation for
// operation (csrc/gemv_shared.h holds what the two translation units share; tests/test_gpu_w16.py compares with torch.equal).
//
// Layout (include/ssrhip.h SSRHIP_W16_INDEX): the unit of work is the fp32 kernels' (row, 1024-element segment of K); its 2 KiB are two
// wave-level loads of one contiguous KiB each, and lane l's 16 bytes of load j hold the fp32 kernel's float4 #2j followed by #2j+1 of that
// lane — after the shift the lane owns the same pieces of x, xr[b][i], as in gemv_seg_kernel / gemv_segu_kernel.
//
// Two kernels, the two forms the fp32 dispatch (gemv.hip try_seg) uses for these shapes:
//   w16_segu_kernel  one 8-wave workgroup per CU, NUW units per wave as straight-line code (QKV, FFN1, FFN2, head-MLP1 at 830M; unlike the
//                    fp32 form at 1 and 4 rows too: 4 rows gain 1.3-2.6 us per launch over the generic form, 1 row about breaks even);
//   w16_seg_kernel   the generic form: balanced contiguous rows per workgroup, ragged tails, groups, the split-KV merge prologue.
// Streaming discipline as in DESIGN.md I.2: every weight load is unconditional inside its block and countable, re-requests overwrite a
// used piece in place, no predicated loads. The VALU cost of widening is 8 bit operations per 2 KiB unit and lane, beside 16 * B FMAs.
// No v_dot2 form: it would round x to bf16 and break the arithmetic contract.
#include <stdlib.h>
#include "common.h"
#include "gemv_shared.h"
#include "gemv_wstream.h"

namespace {

struct W16K {
  GemvK k;
  const uint16_t* W16;   // [groups][N][K] in SSRHIP_W16_INDEX order
};

// ---------------------------------------------------------------------------------------------------------------
// The generic segment form (gemv_seg_kernel): 512-thread workgroups, each owning a contiguous block of rows; wave w works on segment
// w % S and on the units w, w + 8, w + 16, ... of its workgroup. The fp32 form keeps ONE unit (4 KiB) in flight per wave and was tuned on
// bytes; a w16 unit is 2 KiB, so a wave keeps TWO units in flight here (a ring of two, 4 x 16 bytes per lane: the same registers and the
// same bytes in flight). Both are requested at kernel entry (clamped to the workgroup's last unit), which is also what the fp32 `TWO`
// variant does for the out-projection behind its merge prologue. Re-requests happen in place, in blocks that are entered only when the
// successor unit exists — none is wasted, none is predicated.
template <int B, int PRO>
__global__ __launch_bounds__(SEG_TH, (PRO == SSRHIP_PRO_ATTN_COMBINE) ? 2 : 4) void w16_seg_kernel(const W16K q) {
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
  const uint16_t* Wg = q.W16 + ((size_t)g * N + r0) * K + seg * SEG + lane * 8;   // unit of local row c: + c * K; piece j: + j * 512

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
  // ---- 2. the wave's first two units, unconditional (clamped to the workgroup's last unit)
  w16_v4u w0[2], w1[2];
  int u = wave;
  {
    const int c0 = min(u, nu - 1) >> sh, c1 = min(u + SEG_NW, nu - 1) >> sh;
#pragma unroll
    for (int j = 0; j < 2; ++j) w0[j] = ld16_nt(Wg + (size_t)c0 * K + j * 512);
#pragma unroll
    for (int j = 0; j < 2; ++j) w1[j] = ld16_nt(Wg + (size_t)c1 * K + j * 512);
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
      const float* w = wtab + (b * H + h) * MS;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int s2 = 0; s2 < SEG_CS; ++s2) {
        const bool in = s2 < ns[b];                                   // a page beyond the row must not count (0 * NaN)
        const float ws = in ? w[s2] : 0.f;
        acc.x = fmaf(ws, in ? co[b][s2].x : 0.f, acc.x);
        acc.y = fmaf(ws, in ? co[b][s2].y : 0.f, acc.y);
        acc.z = fmaf(ws, in ? co[b][s2].z : 0.f, acc.z);
        acc.w = fmaf(ws, in ? co[b][s2].w : 0.f, acc.w);
      }
      const float* po = a.part_o + (((size_t)b * H + h) * MS) * hd + d;
      for (int s2 = SEG_CS; s2 < ns[b]; ++s2) {                    // contexts beyond the prefetched pages: the rest, loaded late
        const float ws = w[s2];
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
  // ---- 4. stream the units through the ring of two
  // unit `un` sits in `w`; when `next` >= 0 every 16-byte piece is re-requested for unit `next` right after its use, in place
  auto unit = [&](w16_v4u (&w)[2], int un, int next) {
    float acc[B][2];
#pragma unroll
    for (int b = 0; b < B; ++b) acc[b][0] = acc[b][1] = 0.f;
    if (next >= 0) {
      const uint16_t* wn = Wg + (size_t)(next >> sh) * K;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        w16_piece<B>(w[j], j, xr, acc);
        __builtin_amdgcn_sched_barrier(0);                          // use, THEN overwrite in place
        w[j] = ld16_nt(wn + j * 512);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j) w16_piece<B>(w[j], j, xr, acc);
    }
    seg_park<B>(acc, part, un, lane);
  };
  while (u + 3 * SEG_NW < nu) {                                     // both ring slots have a successor
    unit(w0, u, u + 2 * SEG_NW);
    unit(w1, u + SEG_NW, u + 3 * SEG_NW);
    u += 2 * SEG_NW;
  }
  if (u + 2 * SEG_NW < nu) {                                        // three units left: only the first slot is refilled
    unit(w0, u, u + 2 * SEG_NW);
    unit(w1, u + SEG_NW, -1);
    unit(w0, u + 2 * SEG_NW, -1);
  } else {
    if (u < nu) unit(w0, u, -1);
    if (u + SEG_NW < nu) unit(w1, u + SEG_NW, -1);
  }
  __syncthreads();
  if (t < nrows * B) seg_finish_row<B>(p, g, part, S, rfin, nfin, bfin, efin, kvb);
}

// ---------------------------------------------------------------------------------------------------------------
// The straight-line form (gemv_segu_kernel): ONE 8-wave workgroup per CU, NUW units per wave known at compile time, DEPTH units in flight,
// a 16-byte piece re-requested for unit j + DEPTH right after unit j used it. The fp32 form's DEPTH 4 is 16 KiB in flight per wave; the
// same bytes are 8 w16 units, and NUW <= 8: with DEPTH = NUW every unit is requested at kernel entry and the loop has no re-request at
// all (8 x 2 uint4 = 64 VGPRs, the fp32 ring's registers). Measured (DESIGN.md Part I.10, profiles/w16_decode_ab_830m.log): that form LOSES
// to a ring of 4 units = 8 KiB in flight per wave — the step's launches are short (half the bytes), and what a launch requests beyond the
// latency-bandwidth product only lengthens its ramp, as gemv.hip found for fp32. DEPTH 4 is the default at 1 and 2 rows, DEPTH 2 at 4 rows
// (where the FMAs of a unit take twice as long and two units already cover the latency: 10.0 against 10.9 us for LN + QKV); the other
// depths stay instantiated behind SSRHIP_GEMV_W16_DEPTH for re-measuring.
template <int B, int PRO, int NUW, int DEPTH>
__global__ __launch_bounds__(SEG_TH, 2) void w16_segu_kernel(const W16K q) {
  static_assert(PRO == SSRHIP_PRO_NONE || PRO == SSRHIP_PRO_LAYERNORM, "the split-KV merge prologue stays on w16_seg_kernel");
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
  const uint16_t* Wg = q.W16 + ((size_t)g * N + r0) * K + seg * SEG + lane * 8;

  const int bfin = t % B, rfin = min(t / B, nrows - 1), nfin = r0 + rfin;
  const RowEpi efin = seg_epi_fetch(a, g, nfin, bfin);
  float4 xr[B][4];
  seg_load_x<B>(xr, a.x + (size_t)g * K, (size_t)a.x_stride, seg, lane);
  w16_v4u w[DEPTH][2];
#pragma unroll
  for (int j = 0; j < DEPTH; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) w[j][i] = ld16_nt(Wg + (size_t)((wave + SEG_NW * j) >> sh) * K + i * 512);
  float* kvb[2] = {nullptr, nullptr};
  if (a.epi == SSRHIP_EPI_QKV_APPEND) kv_append_bases<B>(a, bfin, kvb);
  if constexpr (PRO == SSRHIP_PRO_LAYERNORM) seg_layernorm<B>(xr, aux, S, K, a.ln_eps, wave, lane);
#pragma unroll
  for (int j = 0; j < NUW; ++j) {
    w16_v4u (&wj)[2] = w[j % DEPTH];
    float acc[B][2];
#pragma unroll
    for (int b = 0; b < B; ++b) acc[b][0] = acc[b][1] = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      w16_piece<B>(wj[i], i, xr, acc);
      if (j + DEPTH < NUW) {
        __builtin_amdgcn_sched_barrier(0);
        wj[i] = ld16_nt(Wg + (size_t)((wave + SEG_NW * (j + DEPTH)) >> sh) * K + i * 512);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    float mine = 0.f;                                              // seg_park, written out: through the helper hipcc gives <1, LN, 6|8, 2> two more VGPRs
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const float sum = wave_sum(acc[b][0] + acc[b][1]);
      if (lane == b) mine = sum;
    }
    if (lane < B) part[(wave + SEG_NW * j) * B + lane] = mine;     // unit u = local_row * S + seg
  }
  __syncthreads();
  if (t < nrows * B) seg_finish_row<B>(p, g, part, S, rfin, nfin, bfin, efin, kvb);
}

// Does `a` qualify, i.e. would ssrhip_gemv take it with its segment kernels? seg_plan (gemv_shared.h) is the decision of gemv.hip's try_seg;
// the fp32 dispatch must be on those kernels too (SSRHIP_GEMV_SEG != 0, read at every call): the row-per-wave kernels add in another order
// and the promise is bit-identity with ssrhip_gemv.
bool w16_plan(const ssrhip_gemv_args* a, int num_cu, SegPlan* pl) {
  const char* why;
  if (a->B != 1 && a->B != 2 && a->B != 4) return false;
  if (a->x_tiled || a->y_tiled || a->w_tiled) return false;          // tiled layouts are for 5..32 rows
  if (!seg_plan(a, num_cu, false, pl, &why)) return false;           // one workgroup per CU behind the merge prologue, always
  if (const char* e = getenv("SSRHIP_GEMV_SEG")) if (e[0] == '0') return false;
  return true;
}

template <int B>
void w16_launch(const SegPlan& pl, const uint16_t* W16, hipStream_t s) {
  const ssrhip_gemv_args* a = &pl.k.a;
  W16K q;
  q.k = pl.k;
  q.W16 = W16;
  // one workgroup per CU, NUW units per wave straight-line, when the shape divides evenly (the shapes gemv_segu_kernel takes at 2 rows)
  int depth = (B == 4) ? 2 : 4;                                     // SSRHIP_GEMV_W16_DEPTH = 2 | 4 (default: 4, 2 at 4 rows): units in flight per wave; 8: every unit
  if (const char* e = getenv("SSRHIP_GEMV_W16_DEPTH")) depth = atoi(e);   // at entry; 0: never this form. Read at every call.
  if (depth != 0 && pl.segu_nuw) {
    const int nuw = pl.segu_nuw;
    seg_fill(&q.k, a, pl.k.nslice, pl.segu_G1);
    const size_t sm = pl.segu_smem;
    const dim3 g1(pl.segu_G1, a->groups);
#define W16U_LAUNCH(PRO_, NUW_)                                                                                                       \
    do {                                                                                                                               \
      if (depth == 2) hipLaunchKernelGGL((w16_segu_kernel<B, PRO_, NUW_, 2>), g1, dim3(SEG_TH), sm, s, q);                              \
      else if (depth == 8) hipLaunchKernelGGL((w16_segu_kernel<B, PRO_, NUW_, NUW_>), g1, dim3(SEG_TH), sm, s, q);                      \
      else hipLaunchKernelGGL((w16_segu_kernel<B, PRO_, NUW_, 4>), g1, dim3(SEG_TH), sm, s, q);                                         \
    } while (0)
    if (a->pro == SSRHIP_PRO_LAYERNORM) {
      if (nuw == 4) W16U_LAUNCH(SSRHIP_PRO_LAYERNORM, 4); else if (nuw == 6) W16U_LAUNCH(SSRHIP_PRO_LAYERNORM, 6); else W16U_LAUNCH(SSRHIP_PRO_LAYERNORM, 8);
    } else {
      if (nuw == 4) W16U_LAUNCH(SSRHIP_PRO_NONE, 4); else if (nuw == 6) W16U_LAUNCH(SSRHIP_PRO_NONE, 6); else W16U_LAUNCH(SSRHIP_PRO_NONE, 8);
    }
#undef W16U_LAUNCH
    return;
  }
  const dim3 grid(pl.G, a->groups);
  switch (a->pro) {
    case SSRHIP_PRO_LAYERNORM: hipLaunchKernelGGL((w16_seg_kernel<B, SSRHIP_PRO_LAYERNORM>), grid, dim3(SEG_TH), pl.smem, s, q); break;
    case SSRHIP_PRO_ATTN_COMBINE: hipLaunchKernelGGL((w16_seg_kernel<B, SSRHIP_PRO_ATTN_COMBINE>), grid, dim3(SEG_TH), pl.smem, s, q); break;
    default: hipLaunchKernelGGL((w16_seg_kernel<B, SSRHIP_PRO_NONE>), grid, dim3(SEG_TH), pl.smem, s, q); break;
  }
}

}  // namespace

extern "C" int ssrhip_gemv_w16_applicable(const ssrhip_gemv_args* a) {
  SegPlan pl;
  return (a && w16_plan(a, ssr_num_cu(), &pl)) ? 1 : 0;
}

extern "C" int ssrhip_gemv_w16(const ssrhip_gemv_args* a, const uint16_t* W16, ssrhip_stream_t stream) {
  SSR_REQUIRE(a && a->W && a->y && W16, "ssrhip_gemv_w16: null argument");
  SSR_REQUIRE(a->N > 0 && a->groups >= 1 && a->K > 0, "ssrhip_gemv_w16: bad N/K/groups");
  SSR_REQUIRE(a->B == 1 || a->B == 2 || a->B == 4, "ssrhip_gemv_w16: B=%d not in {1,2,4} (the bf16 weight stream exists for the <= 4-row step only)", a->B);
  if (int rc = gemv_small_check(a, "ssrhip_gemv_w16")) return rc;   // the contract of ssrhip_gemv: what it would refuse is refused here too
  SegPlan pl;
  if (!w16_plan(a, ssr_num_cu(), &pl)) return 1;
  hipStream_t s = (hipStream_t)stream;
  switch (a->B) {
    case 1: w16_launch<1>(pl, W16, s); break;
    case 2: w16_launch<2>(pl, W16, s); break;
    default: w16_launch<4>(pl, W16, s); break;
  }
  SSR_LAUNCH_CHECK();
  return 0;
}
