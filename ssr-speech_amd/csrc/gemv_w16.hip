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

namespace {

typedef unsigned w16_v4u __attribute__((ext_vector_type(4)));

// 8 packed bf16 of a streamed-once weight row: non-temporal 16-byte load (global_load_dwordx4 ... nt)
__device__ __forceinline__ w16_v4u ld16_nt(const uint16_t* p) { return __builtin_nontemporal_load(reinterpret_cast<const w16_v4u*>(p)); }

// the two float4 of one 16-byte piece: element 2m sits in the low half of dword m (shift), element 2m + 1 in the high half (mask)
__device__ __forceinline__ float4 w16_lo(const w16_v4u u) {
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ float4 w16_hi(const w16_v4u u) {
  return make_float4(__uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u), __uint_as_float(u.w << 16), __uint_as_float(u.w & 0xffff0000u));
}

// piece j (j = 0, 1) of a unit against the lane's x: gemv_seg_kernel's `acc[b][i & 1] = dot4(w[i], xr[b][i], acc[b][i & 1])` for i = 2j, 2j + 1
template <int B>
__device__ __forceinline__ void w16_piece(const w16_v4u u, int j, const float4 (&xr)[B][4], float (&acc)[B][2]) {
  const float4 w0 = w16_lo(u), w1 = w16_hi(u);
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b][0] = dot4(w0, xr[b][2 * j], acc[b][0]);
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b][1] = dot4(w1, xr[b][2 * j + 1], acc[b][1]);
}

// per-segment two-pass LayerNorm statistics, exchanged through LDS and merged exactly (Chan): the arithmetic of gemv_seg_kernel
template <int B>
__device__ __forceinline__ void w16_layernorm(float4 (&xr)[B][4], float* aux, int S, int K, float eps, int wave, int lane) {
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
  RowEpi efin = {0.f, 0.f};
  const int bfin = t % B, rfin = min(t / B, nrows - 1), nfin = r0 + rfin;
  efin.bias = a.bias ? a.bias[(size_t)g * N + nfin] : 0.f;
  efin.resid = (a.epi == SSRHIP_EPI_RESIDUAL) ? a.y[(size_t)bfin * a.y_stride + (size_t)g * N + nfin] : 0.f;
  // ---- 1. activations (L2)
  float4 xr[B][4];
  float4 co[(PRO == SSRHIP_PRO_ATTN_COMBINE) ? B : 1][SEG_CS];
  float2 cml[SEG_CS];
  int ns[(PRO == SSRHIP_PRO_ATTN_COMBINE) ? B : 1];
  if constexpr (PRO != SSRHIP_PRO_ATTN_COMBINE) {
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[b][i] = ld4(a.x + (size_t)b * a.x_stride + (size_t)g * K + seg * SEG + (i * 64 + lane) * 4);
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
  if constexpr (PRO == SSRHIP_PRO_LAYERNORM) w16_layernorm<B>(xr, aux, S, K, a.ln_eps, wave, lane);
  if constexpr (PRO == SSRHIP_PRO_ATTN_COMBINE) {                  // gemv_seg_kernel's merge, operation for operation
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
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[b][i] = *reinterpret_cast<const float4*>(xs + b * K + seg * SEG + (i * 64 + lane) * 4);
  }
  // ---- 4. stream the units through the ring of two
  auto reduce_park = [&](float (&acc)[B][2], int un) {
    float mine = 0.f;
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const float sum = wave_sum(acc[b][0] + acc[b][1]);
      if (lane == b) mine = sum;
    }
    if (lane < B) part[un * B + lane] = mine;                      // un = local_row * S + seg
  };
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
    reduce_park(acc, un);
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
  if (t < nrows * B) {
    float v = 0.f;
    for (int s2 = 0; s2 < S; ++s2) v += part[(rfin * S + s2) * B + bfin];
    finalize(p, g, nfin, bfin, v, efin, kvb);
  }
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

  RowEpi efin = {0.f, 0.f};
  const int bfin = t % B, rfin = min(t / B, nrows - 1), nfin = r0 + rfin;
  efin.bias = a.bias ? a.bias[(size_t)g * N + nfin] : 0.f;
  efin.resid = (a.epi == SSRHIP_EPI_RESIDUAL) ? a.y[(size_t)bfin * a.y_stride + (size_t)g * N + nfin] : 0.f;
  float4 xr[B][4];
#pragma unroll
  for (int b = 0; b < B; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i) xr[b][i] = ld4(a.x + (size_t)b * a.x_stride + (size_t)g * K + seg * SEG + (i * 64 + lane) * 4);
  w16_v4u w[DEPTH][2];
#pragma unroll
  for (int j = 0; j < DEPTH; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) w[j][i] = ld16_nt(Wg + (size_t)((wave + SEG_NW * j) >> sh) * K + i * 512);
  float* kvb[2] = {nullptr, nullptr};
  if (a.epi == SSRHIP_EPI_QKV_APPEND) kv_append_bases<B>(a, bfin, kvb);
  if constexpr (PRO == SSRHIP_PRO_LAYERNORM) w16_layernorm<B>(xr, aux, S, K, a.ln_eps, wave, lane);
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
    float mine = 0.f;
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const float sum = wave_sum(acc[b][0] + acc[b][1]);
      if (lane == b) mine = sum;
    }
    if (lane < B) part[(wave + SEG_NW * j) * B + lane] = mine;     // unit u = local_row * S + seg
  }
  __syncthreads();
  if (t < nrows * B) {
    float v = 0.f;
    for (int s2 = 0; s2 < S; ++s2) v += part[(rfin * S + s2) * B + bfin];
    finalize(p, g, nfin, bfin, v, efin, kvb);
  }
}

// Does `a` qualify, i.e. would gemv.hip's try_seg take it? (`why` receives the answer as text.) The fp32 dispatch must be on its
// segment kernels too (SSRHIP_GEMV_SEG != 0): the row-per-wave kernels add in another order and the promise is bit-identity with ssrhip_gemv.
bool w16_qualifies(const ssrhip_gemv_args* a, int num_cu, const char** why) {
  auto no = [&](const char* w) { *why = w; return false; };
  if (a->B != 1 && a->B != 2 && a->B != 4) return no("B not in {1, 2, 4}");
  if (a->x_tiled || a->y_tiled || a->w_tiled) return no("tiled layouts are for 5..32 rows");
  if (a->K % SEG != 0) return no("K is not a multiple of 1024");
  const int S = a->K / SEG;
  if (S != 1 && S != 2 && S != 4 && S != 8) return no("K / 1024 not in {1, 2, 4, 8}");
  if (a->pro == SSRHIP_PRO_LAYERNORM && a->ln_w != nullptr) return no("LayerNorm gamma / beta not folded into the weights");
  const int H = a->kv.head_dim > 0 ? a->K / a->kv.head_dim : 0;
  if (a->pro == SSRHIP_PRO_ATTN_COMBINE && (a->K != 2048 || a->max_splits < 1 || a->groups != 1 || a->B * H > SEG_TH || a->kv.head_dim % 4 != 0))
    return no("split-KV merge prologue needs K = 2048, one group, B * H <= 512");
  int G = (2 * num_cu) / a->groups;
  if (a->pro == SSRHIP_PRO_ATTN_COMBINE) G = num_cu;
  if (G > a->N) G = a->N;
  if (G < 1) G = 1;
  if ((a->N + G - 1) / G * a->B > SEG_TH) return no("too many rows per workgroup");
  if (const char* e = getenv("SSRHIP_GEMV_SEG")) if (e[0] == '0') return no("SSRHIP_GEMV_SEG=0");
  *why = "";
  return true;
}

// the contract of ssrhip_gemv for <= 4 rows (same checks: a launch that ssrhip_gemv would refuse is refused here too)
int w16_check(const ssrhip_gemv_args* a, const uint16_t* W16) {
  SSR_REQUIRE(a && a->W && a->y && W16, "ssrhip_gemv_w16: null argument");
  SSR_REQUIRE(a->N > 0 && a->groups >= 1 && a->K > 0, "ssrhip_gemv_w16: bad N/K/groups");
  SSR_REQUIRE(a->B == 1 || a->B == 2 || a->B == 4, "ssrhip_gemv_w16: B=%d not in {1,2,4} (the bf16 weight stream exists for the <= 4-row step only)", a->B);
  SSR_REQUIRE(!a->x_tiled && !a->y_tiled && !a->w_tiled, "ssrhip_gemv_w16: the tiled activation / weight layouts are for 5..32 rows only");
  SSR_REQUIRE(a->pro != SSRHIP_PRO_ATTN_COMBINE || (a->kv.head_dim > 0 && a->K <= 2048 && a->B * (a->K / a->kv.head_dim) <= 256), "ssrhip_gemv_w16: combine prologue needs K <= 2048 and B*H <= 256");
  SSR_REQUIRE(a->K % 4 == 0 && a->K <= 8192, "ssrhip_gemv_w16: K=%d must be a multiple of 4, <= 8192", a->K);
  if (a->pro != SSRHIP_PRO_NONE) {
    SSR_REQUIRE(a->groups == 1 || a->pro == SSRHIP_PRO_LAYERNORM, "ssrhip_gemv_w16: combine prologue needs groups==1");
    if (a->pro == SSRHIP_PRO_LAYERNORM) SSR_REQUIRE(a->x && ((a->ln_w && a->ln_b) || (!a->ln_w && !a->ln_b)), "ssrhip_gemv_w16: LayerNorm prologue needs x and either both or none of ln_w/ln_b");
    if (a->pro == SSRHIP_PRO_ATTN_COMBINE) {
      SSR_REQUIRE(a->part_o && a->part_ml && a->row_len && a->kv.head_dim > 0 && a->K % a->kv.head_dim == 0 && a->kv.head_dim % 4 == 0,
                  "ssrhip_gemv_w16: combine prologue needs part_o, part_ml, row_len, kv.head_dim");
    }
  } else {
    SSR_REQUIRE(a->x, "ssrhip_gemv_w16: x is null");
  }
  if (a->epi == SSRHIP_EPI_QKV_APPEND) {
    SSR_REQUIRE(a->N == 3 * a->K && a->groups == 1 && a->kv.pool && a->kv.table && a->kv_pos && a->kv.head_dim > 0,
                "ssrhip_gemv_w16: QKV epilogue needs N==3K and a kv cache");
  }
  return 0;
}

template <int B>
void w16_launch(const ssrhip_gemv_args* a, const uint16_t* W16, int num_cu, hipStream_t s) {
  const int S = a->K / SEG;
  const int H = a->kv.head_dim > 0 ? a->K / a->kv.head_dim : 0;
  int G = (2 * num_cu) / a->groups;                                // two resident workgroups per CU over all groups ...
  if (a->pro == SSRHIP_PRO_ATTN_COMBINE) G = num_cu;               // ... one behind the merge prologue (every workgroup reads all the partials)
  if (G > a->N) G = a->N;
  if (G < 1) G = 1;
  const int rows_max = (a->N + G - 1) / G;
  W16K q;
  q.W16 = W16;
  GemvK& p = q.k;
  p.a = *a;
  p.nslice = S;
  p.slice_len = SEG;
  p.nch = 4;
  p.seg_shift = (S == 1) ? 0 : (S == 2) ? 1 : (S == 4) ? 2 : 3;
  p.rows_max = rows_max;
  p.rows_per = a->N / G;
  p.rows_rem = a->N % G;
  p.prof = nullptr;
  p.groups_x = G;
  p.hd = (a->kv.head_dim > 0) ? a->kv.head_dim : 1;
  size_t smem = (size_t)rows_max * S * B * sizeof(float);
  if (a->pro == SSRHIP_PRO_LAYERNORM) smem += (size_t)S * B * 2 * sizeof(float);
  if (a->pro == SSRHIP_PRO_ATTN_COMBINE) smem += ((size_t)B * a->K + (size_t)B * H * a->max_splits) * sizeof(float);
  smem = (smem + 15) / 16 * 16;
  {
    // one workgroup per CU, NUW units per wave straight-line, when the shape divides evenly (the shapes gemv_segu_kernel takes at 2 rows)
    int depth = (B == 4) ? 2 : 4;                                   // SSRHIP_GEMV_W16_DEPTH = 2 | 4 (default: 4, 2 at 4 rows): units in flight per wave; 8: every unit
    if (const char* e = getenv("SSRHIP_GEMV_W16_DEPTH")) depth = atoi(e);   // at entry; 0: never this form. Read at every call.
    const bool off = depth == 0;
    const int G1 = num_cu / a->groups;
    if (!off && a->pro != SSRHIP_PRO_ATTN_COMBINE && G1 >= 1 && a->N % G1 == 0 && ((a->N / G1) * S) % SEG_NW == 0) {
      const int nuw = (a->N / G1) * S / SEG_NW;
      if (nuw == 4 || nuw == 6 || nuw == 8) {
        p.rows_max = p.rows_per = a->N / G1;
        p.rows_rem = 0;
        p.groups_x = G1;
        size_t sm = (size_t)p.rows_per * S * B * sizeof(float) + (size_t)S * B * 2 * sizeof(float);
        sm = (sm + 15) / 16 * 16;
        const dim3 g1(G1, a->groups);
#define W16U_LAUNCH(PRO_, NUW_)                                                                                                       \
        do {                                                                                                                           \
          if (depth == 2) hipLaunchKernelGGL((w16_segu_kernel<B, PRO_, NUW_, 2>), g1, dim3(SEG_TH), sm, s, q);                          \
          else if (depth == 8) hipLaunchKernelGGL((w16_segu_kernel<B, PRO_, NUW_, NUW_>), g1, dim3(SEG_TH), sm, s, q);                  \
          else hipLaunchKernelGGL((w16_segu_kernel<B, PRO_, NUW_, 4>), g1, dim3(SEG_TH), sm, s, q);                                     \
        } while (0)
        if (a->pro == SSRHIP_PRO_LAYERNORM) {
          if (nuw == 4) W16U_LAUNCH(SSRHIP_PRO_LAYERNORM, 4); else if (nuw == 6) W16U_LAUNCH(SSRHIP_PRO_LAYERNORM, 6); else W16U_LAUNCH(SSRHIP_PRO_LAYERNORM, 8);
        } else {
          if (nuw == 4) W16U_LAUNCH(SSRHIP_PRO_NONE, 4); else if (nuw == 6) W16U_LAUNCH(SSRHIP_PRO_NONE, 6); else W16U_LAUNCH(SSRHIP_PRO_NONE, 8);
        }
#undef W16U_LAUNCH
        return;
      }
    }
  }
  const dim3 grid(G, a->groups);
  switch (a->pro) {
    case SSRHIP_PRO_LAYERNORM: hipLaunchKernelGGL((w16_seg_kernel<B, SSRHIP_PRO_LAYERNORM>), grid, dim3(SEG_TH), smem, s, q); break;
    case SSRHIP_PRO_ATTN_COMBINE: hipLaunchKernelGGL((w16_seg_kernel<B, SSRHIP_PRO_ATTN_COMBINE>), grid, dim3(SEG_TH), smem, s, q); break;
    default: hipLaunchKernelGGL((w16_seg_kernel<B, SSRHIP_PRO_NONE>), grid, dim3(SEG_TH), smem, s, q); break;
  }
}

}  // namespace

extern "C" int ssrhip_gemv_w16_applicable(const ssrhip_gemv_args* a) {
  if (!a) return 0;
  const char* why;
  return w16_qualifies(a, ssr_num_cu(), &why) ? 1 : 0;
}

extern "C" int ssrhip_gemv_w16(const ssrhip_gemv_args* a, const uint16_t* W16, ssrhip_stream_t stream) {
  if (int rc = w16_check(a, W16)) return rc;
  const int num_cu = ssr_num_cu();
  const char* why;
  if (!w16_qualifies(a, num_cu, &why)) return 1;
  hipStream_t s = (hipStream_t)stream;
  switch (a->B) {
    case 1: w16_launch<1>(a, W16, num_cu, s); break;
    case 2: w16_launch<2>(a, W16, num_cu, s); break;
    default: w16_launch<4>(a, W16, num_cu, s); break;
  }
  SSR_LAUNCH_CHECK();
  return 0;
}
