// attn.hip — single-query attention over the paged KV cache, split over pages (flash-decoding), gfx950.
//
// One workgroup (4 waves) per (page, head, row); wave w scores 32 keys of the page.
// Layout: a key/value row (head_dim fp32) is covered by LPK = head_dim/4 lanes with one float4 each, so one
// wave-instruction loads 64/LPK whole rows, fully coalesced (512 B contiguous per row at head_dim 128).
// All K and V loads of the wave's 32 keys are issued up front (the kernel is latency-, not
// bandwidth-bound: every cache element is used exactly once per step, so there is no reuse for LDS to
// exploit; LDS only carries the 4-wave merge). q.k partial products are reduced across the LPK lanes
// with xor-shuffles on NI independent values at once; softmax statistics (m, l) and the un-normalised
// output are written per page and merged by the consumer (ssrhip_gemv PRO_ATTN_COMBINE or
// ssrhip_attn_combine) — deterministic, no atomics.
// Replaces F.scaled_dot_product_attention (models/modules/activation.py:634); the additive mask the
// reference builds (models/ssr.py:227-255) is exactly "row r sees positions < row_len[r]".
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
using std::min;
#include "common.h"

namespace {

// K/V of a decode step are read exactly once per step: non-temporal loads (measured: 2 rows 8.9 -> 8.0 us per launch, 0.905 -> 0.898
// ms/step; 16 rows 35.1 -> 31.8 us at context 720, 1.475 -> 1.434 ms/step). -DSSR_ATTN_NT=0 builds the plain-load variant.
#ifndef SSR_ATTN_NT
#define SSR_ATTN_NT 1
#endif
__device__ __forceinline__ float4 ld_kv(const float* p) { return SSR_ATTN_NT ? ld_nt(p) : ld4(p); }
// The bf16 KV cache (ssrhip_attn_rows_kv16 / ssrhip_attn_prefill_kv16): the same 4 features of a key as 4 two-byte entries, one 8-byte load;
// they stay packed in registers and are widened (a 16-bit shift: exact) where the fp32 kernels use the float4
__device__ __forceinline__ uint2 ld_kv(const uint16_t* p) {
  typedef unsigned v2u __attribute__((ext_vector_type(2)));
  if (!SSR_ATTN_NT) return *reinterpret_cast<const uint2*>(p);
  const v2u v = __builtin_nontemporal_load(reinterpret_cast<const v2u*>(p));
  return make_uint2(v.x, v.y);
}
// the same load at a 32-bit BYTE offset from a workgroup-uniform base (attn_decode_kernel's 2-byte form): the request takes the base from
// scalar registers and one VGPR of offset where a 64-bit lane address takes two — 16 K and 16 V rows in flight cost 32 registers less
__device__ __forceinline__ uint2 ld_kv_at(const uint16_t* base, const unsigned byte_off) {
  return ld_kv(reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(base) + byte_off));
}
__device__ __forceinline__ float4 kv_f4(const float4 v) { return v; }
__device__ __forceinline__ float4 kv_f4(const uint2 v) { return bf16x4_widen(v); }
template <bool KV16> struct kv_types { typedef float elem; typedef float4 vec; };
template <> struct kv_types<true> { typedef uint16_t elem; typedef uint2 vec; };

// The geometry of NW waves reading one page at head_dim HD, derived here for every kernel below
template <int HD, int NW>
struct attn_geom {
  static constexpr int LPK = HD / 4;             // lanes per key row
  static constexpr int KPI = 64 / LPK;           // key rows per wave-instruction
  static constexpr int KPW = SSRHIP_PAGE / NW;   // keys of a page per wave
  static constexpr int NI = KPW / KPI;           // load instructions for the wave's keys
};
// the KPI key-row groups of a wave (lanes with equal c4) share m, so their (l, o) simply add
template <int LPK>
__device__ __forceinline__ void attn_wave_sum(float& l, float4& o) {
  if (LPK == 16) {
    l += xor16_f(l);
    o.x += xor16_f(o.x); o.y += xor16_f(o.y); o.z += xor16_f(o.z); o.w += xor16_f(o.w);
  }
  l += xor32_f(l);
  o.x += xor32_f(o.x); o.y += xor32_f(o.y); o.z += xor32_f(o.z); o.w += xor32_f(o.w);
}
// merge of the NW waves' states in LDS (row w: the wave's o, then its m and l) by the lane that owns columns c4..c4+3 (fixed wave order:
// deterministic): the un-normalised state of the whole workgroup
struct attn_state { float M, L; float4 acc; };
template <int HD, int NW>
__device__ __forceinline__ attn_state attn_merge_waves(const float (&sm)[NW][HD + 4], const int c4) {
  float M = -INFINITY;
#pragma unroll
  for (int w = 0; w < NW; ++w) M = fmaxf(M, sm[w][HD]);
  float L = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const float mw = sm[w][HD];
    const float f = (mw > -INFINITY) ? expf(mw - M) : 0.f;
    L = fmaf(f, sm[w][HD + 1], L);
    acc.x = fmaf(f, sm[w][c4 + 0], acc.x);
    acc.y = fmaf(f, sm[w][c4 + 1], acc.y);
    acc.z = fmaf(f, sm[w][c4 + 2], acc.z);
    acc.w = fmaf(f, sm[w][c4 + 3], acc.w);
  }
  return attn_state{M, L, acc};
}

// KV16 (ssrhip_attn_decode_kv16, the <= 4-row step of an engine with a bf16 cache, DESIGN.md Part I.23): a.kv.pool holds 2-byte entries (same element
// offsets), a lane's 8-byte load holds the 4 features its 16-byte load held, kept packed and widened where they are folded. The position
// this step's QKV launch appended, row_len[r] - 1, is not in the pool yet: the launch wrote it, fp32, into the landing cache `land`
// [R][1][2][n_head][SSRHIP_PAGE][HD], layer l at position l of row r's page. Every workgroup requests its (row, head)'s landing entry beside q
// (the address is arithmetic on kernel arguments: no scalar round trip in front of it), rounds it to nearest even and takes the ROUNDED
// values wherever its key index is len - 1 - base — the clamped lanes included — so nothing the pool holds at that position (stale, or
// never written) reaches the arithmetic; the one workgroup that owns the position (split == (len - 1) / SSRHIP_PAGE) stores the rounded 8
// bytes into the pool for the steps to come. No other workgroup of the launch touches these entries. `land` is not read otherwise.
template <int HD, bool SEQ, int VAT = -1, bool KV16 = false>   // SEQ: rows carry an explicit sequence id (a.row_seq != NULL: the per-row prefill path); the decode step has none
__global__ __launch_bounds__(256) void attn_decode_kernel(const ssrhip_attn_args a, const int head_fastest, const float* land) {   // VAT: see the V requests below
  static_assert(!(KV16 && SEQ), "the landing cache belongs to the decode step: row r is sequence r");
  typedef typename kv_types<KV16>::elem kv_elem;
  typedef typename kv_types<KV16>::vec kv_vec;
  typedef attn_geom<HD, 4> G;
  constexpr int LPK = G::LPK, KPI = G::KPI, NI = G::NI;   // 4 waves: 32 keys of the page each
  __shared__ __attribute__((aligned(16))) float sm[4][HD + 4];   // row stride keeps float4 stores 16-B aligned
  // Workgroup b runs on XCD b % 8 (observed, for speed only). With the page index as the fastest grid dimension and 8 pages of capacity
  // every workgroup of page p sat on XCD p: a 600-position context used 5 XCDs' L2s and fabric links and left 3 idle. `head_fastest`
  // makes the head the fastest dimension: the live (page, head, row) items spread over all XCDs whatever the context.
  const int split = head_fastest ? blockIdx.y : blockIdx.x, h = head_fastest ? blockIdx.x : blockIdx.y, r = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPK;         // which key row inside one wave-instruction
  const int c4 = (lane % LPK) * 4;    // this lane's 4 columns
  const int H = a.kv.n_head;
  // the row's length, its page id and q are requested TOGETHER, before the early exit (split < max_pages: the table entry exists and
  // holds a valid page — the engine's spare page — also beyond the row's length): one scalar-memory round trip instead of two in a row.
  // Round 4: the ISA showed FOUR serial scalar round trips in front of the first K/V request (kernel arguments fetched piecemeal, then
  // row_seq, then the table entry): the arguments are pinned into ONE batch, and the decode step's common case (row_seq == NULL) reads
  // table[r][split] without waiting for anything but the arguments. Constant address space: scalar loads (row_len / table / row_seq do
  // not change during the launch).
  typedef const int32_t __attribute__((address_space(4))) cint;
  cint* c_len = (cint*)(uintptr_t)a.row_len;
  cint* c_tab = (cint*)(uintptr_t)a.kv.table;
  cint* c_seq = (cint*)(uintptr_t)a.row_seq;
  asm volatile("; kernel arguments in one batch" :: "s"(a.q), "s"(a.kv.pool), "s"(a.kv.max_pages), "s"(a.kv.n_layer), "s"(a.layer), "s"(a.scale),
               "s"(a.part_o), "s"(a.part_ml), "s"(a.max_splits), "s"(a.q_stride), "s"(H), "s"(c_len), "s"(c_tab), "s"(c_seq), "s"(a.prefetch),
               "s"(a.prefetch_floats));
  const int len = c_len[r];
  const int page = SEQ ? c_tab[(size_t)c_seq[r] * a.kv.max_pages + split]      // rows mapped to another sequence: one more round trip
                       : c_tab[(size_t)r * a.kv.max_pages + split];            // the row's own sequence (decode step): together with its length
  const float4 q = ld4(a.q + (size_t)r * (a.q_stride ? a.q_stride : H * HD) + h * HD + c4);
  [[maybe_unused]] float4 lk4, lv4;   // KV16: this (row, head)'s landing entry, K and V
  if constexpr (KV16) {
    const float* lk = land + ((((size_t)r * 2 + 0) * H + h) * SSRHIP_PAGE + a.layer) * HD + c4;
    lk4 = ld4(lk);
    lv4 = ld4(lk + (size_t)H * SSRHIP_PAGE * HD);
  }
  [[maybe_unused]] float pfj = 0.f;   // KV16: where the prefetch touches land (see there)
  if (!SEQ && a.prefetch) {
    // Round 6: this launch is latency-bound (a few dependent round trips for 10 MB of K / V) and most of its workgroups at short contexts
    // have nothing to do at all, while the launch behind it starts by streaming 64 KB of W_o per CU from HBM. Workgroup i touches the
    // slice workgroup i of that launch will read (same XCD: i % 8) — plain loads behind the scalar requests and q, results never used: extra
    // loads the compiler does not know of only make its later waits (`vmcnt(n)` = all but the n youngest) stricter, never laxer, and the lines sit in this XCD's L2 when they are wanted.
    const unsigned wg = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    if (wg < 256u) {
      const float* pf = a.prefetch + (size_t)wg * a.prefetch_floats + threadIdx.x * 4;
      for (int i = 0; i < a.prefetch_floats; i += 1024) {
        if constexpr (KV16) {
          // the same touch, into registers that stay LIVE until the first K row has arrived (`pfj` is an operand of the statement that
          // consumes the landing entry below). The statement of the fp32 instantiations hides its load from the compiler, which is then
          // free to reuse the destination while the load is in flight; in this instantiation it did, for the K rows' addresses (read off
          // the ISA), and the late data sent those requests anywhere. Requests return in order: once a K row is here, so is every touch.
          // One dword per lane touches the same cache lines as the 16 bytes (the lanes are 16 bytes apart) and keeps one register, not four.
          asm volatile("global_load_dword %0, %1, off" : "+v"(pfj) : "v"(pf + i) : "memory");
        } else {
          float4 junk;
          asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(junk) : "v"(pf + i) : "memory");
        }
      }
    }
  }
  asm volatile("; row length and page id arrive together" :: "s"(len), "s"(page));
  const int base = split * SSRHIP_PAGE;
  if (base >= len) return;            // uniform per block
  const kv_elem* kp = reinterpret_cast<const kv_elem*>(a.kv.pool) + ((((size_t)page * a.kv.n_layer + a.layer) * 2 + 0) * H + h) * SSRHIP_PAGE * HD;
  const kv_elem* vp = kp + (size_t)H * SSRHIP_PAGE * HD;

  kv_vec kk[NI], vv[NI];
  float s[NI];
  // unconditional loads: keys beyond the row's length are read from the last valid key of the page instead (their scores are
  // masked to -inf below, so p == 0 and the duplicate V rows add nothing). Predicated loads would make hipcc drain the
  // memory queue (s_waitcnt vmcnt(0)) between groups of loads (measured: 9.6 -> 7.3 us per launch at 2 rows).
  const int jmax = min(len - base, SSRHIP_PAGE) - 1;     // >= 0: base < len
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int j = min(wave * 32 + i * KPI + sub, jmax);
    if constexpr (KV16) kk[i] = ld_kv_at(kp, (unsigned)(j * HD + c4) * 2u);
    else kk[i] = ld_kv(kp + (size_t)j * HD + c4);
  }
  // KV16: the appended position's index in this page (>= SSRHIP_PAGE: another workgroup's page) and its rounded entries. K and V of key
  // i as the arithmetic sees them: the rounded landing entry where the lane's (clamped) key index is that position, the pool's otherwise.
  // The landing entry was requested in front of the K rows and is consumed once the first K row has arrived (the empty statement ties it
  // to kk[0]; requests return in order, so it waits for nothing the first score does not wait for): left alone, hipcc hoists the rounding
  // — and with it a wait for the landing entry — above the first K request (read off the ISA): one more round trip in a row.
  const int jl = len - 1 - base;
  [[maybe_unused]] kv_vec lk16, lv16;
  if constexpr (KV16) {
    asm volatile("; the landing entry is consumed behind the first K row"
                 : "+v"(lk4.x), "+v"(lk4.y), "+v"(lk4.z), "+v"(lk4.w), "+v"(lv4.x), "+v"(lv4.y), "+v"(lv4.z), "+v"(lv4.w), "+v"(kk[0].x), "+v"(pfj));
    lk16 = bf16x4_rne(lk4.x, lk4.y, lk4.z, lk4.w);
    lv16 = bf16x4_rne(lv4.x, lv4.y, lv4.z, lv4.w);
  }
  // (in the owning workgroup jl == jmax: key i of this lane is the appended position, itself or clamped onto it, from its first index at or
  // past jmax on; one compare with a constant per key)
  const int first_landed = (jl == jmax) ? (jmax - wave * 32 - sub + KPI - 1) / KPI : NI;
  auto landed = [&](const int i) { return i >= first_landed; };
  auto key = [&](const int i) {
    if constexpr (KV16) return kv_f4(make_uint2(landed(i) ? lk16.x : kk[i].x, landed(i) ? lk16.y : kk[i].y));
    else return kk[i];
  };
  auto val = [&](const int i) {
    if constexpr (KV16) return kv_f4(make_uint2(landed(i) ? lv16.x : vv[i].x, landed(i) ? lv16.y : vv[i].y));
    else return vv[i];
  };
  // VAT >= 0: the V rows are requested when VAT of the wave's NI K rows have been consumed — pinned with scheduling fences; -1 leaves the
  // order to hipcc (which keeps ~10 K requests in flight and asks for the V rows behind the LAST K row, see below). Measured at head_dim
  // 128 on the 830M step, same box, alternating engines (profiles/r05_microbench/decode_ab_attn_vat.log): hipcc 6.84 us per launch,
  // VAT 4 / 8 / 12: 6.69 / 6.45 / 6.56 — all 16 K rows in flight from the start and the V rows' flight under the second half of the
  // score arithmetic. The decode step takes VAT = 8 (0.8095 -> 0.8033 ms/step); same arithmetic in the same order: identical tokens.
  if constexpr (VAT >= 0) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < VAT; ++i) s[i] = dot4(q, key(i), 0.f);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int j = min(wave * 32 + i * KPI + sub, jmax);
    if constexpr (KV16) vv[i] = ld_kv_at(vp, (unsigned)(j * HD + c4) * 2u);
    else vv[i] = ld_kv(vp + (size_t)j * HD + c4);
  }
  if constexpr (VAT >= 0) __builtin_amdgcn_sched_barrier(0);
  // What hipcc makes of the two loops above (read off the ISA, round 5; rounds 1-4 believed all 2 NI requests fly together): its
  // occupancy-driven scheduler consumes the K rows as they arrive, re-uses their registers and requests the V rows only once the last K
  // row has landed (77 VGPRs). Pinning all 2 NI requests in front of the first use (`sched_barrier(0)` here, 146 VGPRs) was measured on
  // the 830M step, same box, alternating engines: 7.60 -> 7.89 us per launch, 0.8224 -> 0.8243 ms/step (profiles/r05_microbench/
  // decode_ab.log, variants r4sched / pin) — SLOWER: with K first the score / softmax arithmetic runs under the V rows' flight, while 64 KB
  // + 64 KB requested at once arrive together behind one CU's 64 B/clk port and leave nothing to overlap. The compiler's order stays.
#pragma unroll
  for (int i = (VAT >= 0 ? VAT : 0); i < NI; ++i) s[i] = dot4(q, key(i), 0.f);
  // reduce each s[i] over the LPK lanes of its key row (DPP row rotations + permlane16_swap: no LDS)
#pragma unroll
  for (int i = 0; i < NI; ++i) s[i] = (LPK == 32) ? half32_sum(s[i]) : row16_sum(s[i]);
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int j = wave * 32 + i * KPI + sub;
    s[i] = ((base + j) < len) ? s[i] * a.scale : -INFINITY;
    m = fmaxf(m, s[i]);
  }
  if (LPK == 16) m = fmaxf(m, xor16_f(m));
  m = fmaxf(m, xor32_f(m));
  float l = 0.f;
  float4 o4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (m > -INFINITY) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const float p = expf(s[i] - m);   // exp(-inf) == 0 for masked keys
      const float4 v4 = val(i);
      l += p;
      o4.x = fmaf(p, v4.x, o4.x);
      o4.y = fmaf(p, v4.y, o4.y);
      o4.z = fmaf(p, v4.z, o4.z);
      o4.w = fmaf(p, v4.w, o4.w);
    }
  }
  if constexpr (KV16) {
    // the workgroup that owns the appended position promotes it: the rounded 8 bytes per lane into the pool, behind every load of this wave
    if (jl < SSRHIP_PAGE && wave == 0 && sub == 0) {
      *reinterpret_cast<uint2*>(const_cast<kv_elem*>(kp) + (size_t)jl * HD + c4) = lk16;
      *reinterpret_cast<uint2*>(const_cast<kv_elem*>(vp) + (size_t)jl * HD + c4) = lv16;
    }
  }
  attn_wave_sum<LPK>(l, o4);
  if (lane < LPK) {
    *reinterpret_cast<float4*>(&sm[wave][c4]) = o4;
  }
  if (lane == 0) { sm[wave][HD] = m; sm[wave][HD + 1] = l; }
  __syncthreads();
  // 4-wave merge by the first LPK lanes of wave 0
  if (threadIdx.x < LPK) {
    const attn_state t = attn_merge_waves<HD, 4>(sm, c4);
    const size_t pi = ((size_t)r * H + h) * a.max_splits + split;
    *reinterpret_cast<float4*>(a.part_o + pi * HD + c4) = t.acc;
    if (threadIdx.x == 0) { a.part_ml[pi * 2] = t.M; a.part_ml[pi * 2 + 1] = t.L; }
  }
}

// Merge of the per-page partials (prefill, and the 5..16-row decode step where the out-proj GEMV does not fuse it).
// One wave per workgroup, HD/4 lanes per head (2 or 4 heads per wave), one float4 of the output per lane. The (m, l) pairs
// and the partial outputs of up to 8 pages are requested together with clamped page indices (no predicated loads), so a
// workgroup needs one memory round trip per 8 pages: 5.8 -> ~3 us per launch at 16 rows (was: one workgroup per ROW looping
// over all heads and pages with dependent loads).
template <int HD>
__global__ __launch_bounds__(64) void attn_combine_kernel(const ssrhip_attn_args a, float* out) {
  constexpr int LPH = HD / 4, HPW = 64 / LPH, CH = 8;
  const int H = a.kv.n_head, D = H * HD;
  const int r = blockIdx.y;
  const int h = min((int)blockIdx.x * HPW + (int)threadIdx.x / LPH, H - 1);
  const bool live = (int)blockIdx.x * HPW + (int)threadIdx.x / LPH < H;
  const int d = (threadIdx.x % LPH) * 4;
  const int ns = (a.row_len[r] + SSRHIP_PAGE - 1) / SSRHIP_PAGE;
  const float* ml = a.part_ml + ((size_t)r * H + h) * a.max_splits * 2;
  const float* po = a.part_o + (((size_t)r * H + h) * a.max_splits) * HD + d;
  float M = -INFINITY;
  for (int s0 = 0; s0 < ns; s0 += CH) {
    float m[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) m[i] = ml[2 * min(s0 + i, ns - 1)];
#pragma unroll
    for (int i = 0; i < CH; ++i) M = fmaxf(M, m[i]);           // duplicates of page ns-1 do not change the max
  }
  float den = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s0 = 0; s0 < ns; s0 += CH) {
    float m[CH], l[CH];
    float4 o[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int s2 = min(s0 + i, ns - 1);
      m[i] = ml[2 * s2];
      l[i] = ml[2 * s2 + 1];
      o[i] = ld4(po + (size_t)s2 * HD);
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const float w = (s0 + i < ns) ? expf(m[i] - M) : 0.f;     // same order of operations as before: fixed page order
      den = fmaf(w, l[i], den);
      acc.x = fmaf(w, o[i].x, acc.x);
      acc.y = fmaf(w, o[i].y, acc.y);
      acc.z = fmaf(w, o[i].z, acc.z);
      acc.w = fmaf(w, o[i].w, acc.w);
    }
  }
  if (!live) return;
  const float inv = 1.0f / den;
  const int e = h * HD + d;
  float* dst = a.out_tiled ? out + SSRHIP_TILED_P(r, e, D) : out + (size_t)r * D + e;
  *reinterpret_cast<float4*>(dst) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused single-query attention for MANY rows (the 5..16-row decode step: 16 rows x 16 heads = 256 (row, head) pairs = one
// workgroup per CU). One 8-wave workgroup owns a whole (row, head): it walks the row's pages itself, so there are no
// per-page partials, no merge launch and every CU streams the same number of bytes (rows of a lock-step batch have similar
// lengths). rocprofv3 at 16 rows, context ~520: the split kernel + combine took 40 + 6.7 us per layer for 136 MB of K/V
// (3.4 TB/s); here the workgroup keeps two pages in flight (wave w owns keys [16w, 16w+16) of every page: 16 KB of K/V per
// page per wave, double-buffered = 256 KB per CU) and folds them into a running (m, l, o) — the online softmax — so K/V stream
// at the HBM rate. The 8 waves' states are merged once through LDS and the normalised output row is written directly in
// the layout the out-projection GEMV wants (row-major or SSRHIP_TILED).
// Loads are never predicated (see above): keys past the row's length re-read key 0 of the last page and are masked to -inf.
constexpr int ATTN_ROWS_MAX_PAGES = 256;       // 32,768 positions per row

// The page walk's pieces, shared by attn_rows_kernel and attn_rows_group_kernel (which keeps one (q, len, m, l, o) per member row).
// What the issues and folds of one (workgroup, head) have in common, filled in once in front of the walk:
template <int HD, int NW, class E>
struct attn_walk {
  const E* pool;                    // K of page 0 of this layer and head; page p lies p * page_stride behind it, its V another v_off
  size_t page_stride, v_off;
  float scale;
  int wave, sub, c4;                // the wave, the lane's key row inside one wave-instruction, the lane's 4 columns
};
// Request K and V of page pg of a row of npages pages and len positions into one buffer pair. ids = the register of page ids that holds
// page min(pg, npages - 1) (lane i of register b holds page 64b + i). A page past the last re-reads key 0 of the last page, keys past len
// the page's last valid key (never predicated, see above).
template <int HD, int NW, class E, class KV>
__device__ __forceinline__ void attn_issue(const attn_walk<HD, NW, E>& w, KV (&kk)[attn_geom<HD, NW>::NI], KV (&vv)[attn_geom<HD, NW>::NI], const int pg,
                                           const int ids, const int npages, const int len) {
  typedef attn_geom<HD, NW> G;
  // (the walk's values as locals: with w.pool .. w.c4 written at their uses hipcc orders the waits of nine kernels differently)
  const E* pool = w.pool; const size_t page_stride = w.page_stride, v_off = w.v_off; const int wave = w.wave, sub = w.sub, c4 = w.c4;
  const int pg_ = min(pg, npages - 1);
  const E* kp = pool + (size_t)__builtin_amdgcn_readlane(ids, pg_ & 63) * page_stride;
  const int jmax = (pg < npages) ? min(len - pg_ * SSRHIP_PAGE, SSRHIP_PAGE) - 1 : 0;
#pragma unroll
  for (int i = 0; i < G::NI; ++i) {
    const int j = min(wave * G::KPW + i * G::KPI + sub, jmax);
    kk[i] = ld_kv(kp + (size_t)j * HD + c4);
  }
#pragma unroll
  for (int i = 0; i < G::NI; ++i) {
    const int j = min(wave * G::KPW + i * G::KPI + sub, jmax);
    vv[i] = ld_kv(kp + v_off + (size_t)j * HD + c4);
  }
}
// The pick of that register stays text, every name a parameter: as a function — the four registers by reference, by value or in a struct —
// hipcc moves the table loads and the waits of the group kernels (profiles/attn_refactor_ab.md). PID is the int[4] of page-id registers.
#define ATTN_ISSUE(W, KK, VV, PG, PID, NPAGES, LEN)                                                                  \
  {                                                                                                                  \
    const int pb_ = min((PG), (NPAGES) - 1) >> 6;                                                                    \
    attn_issue(W, KK, VV, PG, pb_ == 0 ? PID[0] : (pb_ == 1 ? PID[1] : (pb_ == 2 ? PID[2] : PID[3])), NPAGES, LEN); \
  }
// fold page pg, held in one buffer pair, into a row's running (m, l, o) with that row's q and length: the online softmax
template <int HD, int NW, class E, class KV>
__device__ __forceinline__ void attn_fold(const attn_walk<HD, NW, E>& w, const KV (&kk)[attn_geom<HD, NW>::NI], const KV (&vv)[attn_geom<HD, NW>::NI],
                                          const int pg, const float4 q, const int len, float& m, float& l, float4& o) {
  typedef attn_geom<HD, NW> G;
  float s[G::NI];
#pragma unroll
  for (int i = 0; i < G::NI; ++i) s[i] = dot4(q, kv_f4(kk[i]), 0.f);
#pragma unroll
  for (int i = 0; i < G::NI; ++i) s[i] = (G::LPK == 32) ? half32_sum(s[i]) : row16_sum(s[i]);
  float mloc = -INFINITY;
#pragma unroll
  for (int i = 0; i < G::NI; ++i) {
    const int pos = pg * SSRHIP_PAGE + w.wave * G::KPW + i * G::KPI + w.sub;
    s[i] = (pos < len) ? s[i] * w.scale : -INFINITY;
    mloc = fmaxf(mloc, s[i]);
  }
  if (G::LPK == 16) mloc = fmaxf(mloc, xor16_f(mloc));
  mloc = fmaxf(mloc, xor32_f(mloc));
  const float mnew = fmaxf(m, mloc);
  if (mnew > -INFINITY) {
    const float al = (m > -INFINITY) ? expf(m - mnew) : 0.f;
    l *= al; o.x *= al; o.y *= al; o.z *= al; o.w *= al;
#pragma unroll
    for (int i = 0; i < G::NI; ++i) {
      const float p = expf(s[i] - mnew);
      l += p;
      o.x = fmaf(p, kv_f4(vv[i]).x, o.x); o.y = fmaf(p, kv_f4(vv[i]).y, o.y);
      o.z = fmaf(p, kv_f4(vv[i]).z, o.z); o.w = fmaf(p, kv_f4(vv[i]).w, o.w);
    }
    m = mnew;
  }
}

// normalise a merged state and store it at dst. The callers write dst out (the row's place in `out`, row-major or SSRHIP_TILED): computed in
// here, or in one function with the merge, it changes attn_rows_kernel's SGPR count or its tail's load order (profiles/attn_refactor_ab.md)
__device__ __forceinline__ void attn_store_row(float* dst, const attn_state t) {
  const float inv = 1.0f / t.L;
  *reinterpret_cast<float4*>(dst) = make_float4(t.acc.x * inv, t.acc.y * inv, t.acc.z * inv, t.acc.w * inv);
}

// KV16: a.kv.pool holds 2-byte entries (same element offsets); K/V of a page then take half the registers, so DEPTH = 4 pages in flight fit
// where the fp32 kernel holds 2. The folds run in page order whatever DEPTH is (a fold of a page past the row's last is masked: no change).
template <int HD, bool KV16 = false, int DEPTH = 2>
__global__ __launch_bounds__(512) void attn_rows_kernel(const ssrhip_attn_args a, float* out) {
  static_assert(DEPTH == 2 || (KV16 && DEPTH == 4), "pages in flight: 2, or 4 with 2-byte entries");
  typedef typename kv_types<KV16>::elem kv_elem;
  typedef typename kv_types<KV16>::vec kv_vec;
  constexpr int NW = 8, LPK = attn_geom<HD, NW>::LPK, NI = attn_geom<HD, NW>::NI;
  __shared__ __attribute__((aligned(16))) float sm[NW][HD + 4];
  const int h = blockIdx.x, r = blockIdx.y;
  const int len = __builtin_amdgcn_readfirstlane(a.row_len[r]);
  const int seq = __builtin_amdgcn_readfirstlane(a.row_seq ? a.row_seq[r] : r);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sub = lane / LPK, c4 = (lane % LPK) * 4;
  const int H = a.kv.n_head;
  const int npages = (len + SSRHIP_PAGE - 1) / SSRHIP_PAGE;           // >= 1: a decode row always sees its own key
  // the row's page ids live in 4 VGPRs (lane i of register b holds page 64b + i) and are picked with v_readlane: a table
  // lookup inside the loop would be a VECTOR load (the compiler cannot prove the table is not written by this kernel), and
  // waiting for it — or for an LDS copy of it — drains every K/V load in flight (seen in the ISA: s_waitcnt vmcnt(0))
  int pid[ATTN_ROWS_MAX_PAGES / 64];
#pragma unroll
  for (int b = 0; b < ATTN_ROWS_MAX_PAGES / 64; ++b)
    pid[b] = (b * 64 < npages) ? a.kv.table[(size_t)seq * a.kv.max_pages + min(b * 64 + lane, npages - 1)] : 0;
  const size_t head_off = (size_t)h * SSRHIP_PAGE * HD, v_off = (size_t)H * SSRHIP_PAGE * HD;
  const size_t page_stride = (size_t)a.kv.n_layer * 2 * H * SSRHIP_PAGE * HD;
  const attn_walk<HD, NW, kv_elem> w = {reinterpret_cast<const kv_elem*>(a.kv.pool) + (size_t)a.layer * 2 * H * SSRHIP_PAGE * HD + head_off,
                                        page_stride, v_off, a.scale, wave, sub, c4};
  const float4 q = ld4(a.q + (size_t)r * (a.q_stride ? a.q_stride : H * HD) + h * HD + c4);

  kv_vec kk[DEPTH][NI], vv[DEPTH][NI];
  float m = -INFINITY, l = 0.f;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);

  if constexpr (DEPTH == 2) {
    ATTN_ISSUE(w, kk[0], vv[0], 0, pid, npages, len)
    for (int pg = 0; pg < npages; pg += 2) {
      ATTN_ISSUE(w, kk[1], vv[1], pg + 1, pid, npages, len)
      attn_fold(w, kk[0], vv[0], pg, q, len, m, l, o);
      ATTN_ISSUE(w, kk[0], vv[0], pg + 2, pid, npages, len)
      attn_fold(w, kk[1], vv[1], pg + 1, q, len, m, l, o);
    }
  } else {
    ATTN_ISSUE(w, kk[0], vv[0], 0, pid, npages, len)
    ATTN_ISSUE(w, kk[1], vv[1], 1, pid, npages, len)
    ATTN_ISSUE(w, kk[2], vv[2], 2, pid, npages, len)
    for (int pg = 0; pg < npages; pg += 4) {
      ATTN_ISSUE(w, kk[3], vv[3], pg + 3, pid, npages, len)
      attn_fold(w, kk[0], vv[0], pg, q, len, m, l, o);
      ATTN_ISSUE(w, kk[0], vv[0], pg + 4, pid, npages, len)
      attn_fold(w, kk[1], vv[1], pg + 1, q, len, m, l, o);
      ATTN_ISSUE(w, kk[1], vv[1], pg + 5, pid, npages, len)
      attn_fold(w, kk[2], vv[2], pg + 2, q, len, m, l, o);
      ATTN_ISSUE(w, kk[2], vv[2], pg + 6, pid, npages, len)
      attn_fold(w, kk[3], vv[3], pg + 3, q, len, m, l, o);
    }
  }
  attn_wave_sum<LPK>(l, o);
  if (lane < LPK) *reinterpret_cast<float4*>(&sm[wave][c4]) = o;
  if (lane == 0) { sm[wave][HD] = m; sm[wave][HD + 1] = l; }
  __syncthreads();
  if (threadIdx.x < LPK) {
    const attn_state t = attn_merge_waves<HD, NW>(sm, c4);
    const int e = h * HD + c4;
    attn_store_row(a.out_tiled ? out + SSRHIP_TILED_P(r, e, H * HD) : out + (size_t)r * H * HD + e, t);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same walk for rows that SHARE their first pages (the samples of one utterance: equal text and prompt audio, so equal prompt
// K/V, DESIGN.md Part I.15). One 8-wave workgroup per (head, chunk of up to MEMBERS rows whose first n_shared table entries name the
// same pages): K/V of a shared page are loaded once and folded into every member's own (m, l, o) with that member's q; then the
// workgroup walks each member's own pages (entries n_shared.. of ITS table row), and merges and stores per member. Every fold, the
// wave sum, the merge and the store are the macros attn_rows_kernel expands, on the same keys per wave in the same page order: a
// member's result equals attn_rows_kernel's on the same (aliased) table bit for bit — sharing moves a row to another workgroup, never
// reorders its arithmetic. (A fold of a page past a row's last is an exact no-op in both kernels: every key masked, p == 0.)
// chunk_head[r] = the lowest row of r's chunk; the grid is (n_head, R) whatever the arrays hold (a captured graph keeps its grid): a
// workgroup whose row is not a head exits at once, a head finds its members with one ballot over chunk_head and a scalar bit scan.
// Members may be any rows (conditional rows are 0, 2, 4, ...), of different lengths and numbers of own pages. n_shared is read at the
// head and clamped to the FULL pages every member has (row_len / SSRHIP_PAGE), so a shared page is never a member's partial page.
// Rows beyond the first MEMBERS that name one head are not computed: the host's contract (engine.py plan_prompt_sharing).
template <int HD, int MEMBERS>
__global__ __launch_bounds__(512) void attn_rows_group_kernel(const ssrhip_attn_args a, const int32_t* __restrict__ chunk_head,
                                                              const int32_t* __restrict__ n_shared, float* out) {
  typedef float kv_elem;
  typedef float4 kv_vec;
  constexpr int NW = 8, LPK = attn_geom<HD, NW>::LPK, NI = attn_geom<HD, NW>::NI, DEPTH = 2;
  __shared__ __attribute__((aligned(16))) float sm[MEMBERS][NW][HD + 4];
  const int h = blockIdx.x, r0 = blockIdx.y;
  if (__builtin_amdgcn_readfirstlane(chunk_head[r0]) != r0) return;   // uniform: not a chunk head
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sub = lane / LPK, c4 = (lane % LPK) * 4;
  const int H = a.kv.n_head;
  // the members, in ascending row order (the head is the lowest): lane i looks at row b0 + i, the ballot is scanned bit by bit
  int mem[MEMBERS];
#pragma unroll
  for (int j = 0; j < MEMBERS; ++j) mem[j] = r0;
  int nmem = 0;
  for (int b0 = 0; b0 < a.R; b0 += 64) {
    const int ch = chunk_head[min(b0 + lane, a.R - 1)];
    unsigned long long mask = __ballot(b0 + lane < a.R && ch == r0);
    while (mask && nmem < MEMBERS) {
      const int row = b0 + __builtin_ctzll(mask);
      mask &= mask - 1;
#pragma unroll
      for (int j = 0; j < MEMBERS; ++j) if (nmem == j) mem[j] = row;
      ++nmem;
    }
  }
  nmem = __builtin_amdgcn_readfirstlane(nmem);
  int len[MEMBERS], seq[MEMBERS], npg[MEMBERS];
  float4 q[MEMBERS], o[MEMBERS];
  float m[MEMBERS], l[MEMBERS];
  int ns = __builtin_amdgcn_readfirstlane(n_shared[r0]);
#pragma unroll
  for (int j = 0; j < MEMBERS; ++j) {                                 // (slots past nmem repeat the head: loaded, never folded or stored)
    len[j] = __builtin_amdgcn_readfirstlane(a.row_len[mem[j]]);
    seq[j] = __builtin_amdgcn_readfirstlane(a.row_seq ? a.row_seq[mem[j]] : mem[j]);
    npg[j] = (len[j] + SSRHIP_PAGE - 1) / SSRHIP_PAGE;
    ns = min(ns, len[j] / SSRHIP_PAGE);
    q[j] = ld4(a.q + (size_t)mem[j] * (a.q_stride ? a.q_stride : H * HD) + h * HD + c4);
    m[j] = -INFINITY; l[j] = 0.f;
    o[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  ns = max(ns, 0);
  const size_t head_off = (size_t)h * SSRHIP_PAGE * HD, v_off = (size_t)H * SSRHIP_PAGE * HD;
  const size_t page_stride = (size_t)a.kv.n_layer * 2 * H * SSRHIP_PAGE * HD;
  const attn_walk<HD, NW, kv_elem> w = {reinterpret_cast<const kv_elem*>(a.kv.pool) + (size_t)a.layer * 2 * H * SSRHIP_PAGE * HD + head_off,
                                        page_stride, v_off, a.scale, wave, sub, c4};
  kv_vec kk[DEPTH][NI], vv[DEPTH][NI];
  int pid[ATTN_ROWS_MAX_PAGES / 64];                                  // page ids in registers, picked with v_readlane (see attn_rows_kernel)

  // ---- the shared pages, entries [0, ns) of the head's table row: whole pages for every member
  if (ns > 0) {
    const int slen = ns * SSRHIP_PAGE;
#pragma unroll
    for (int b = 0; b < ATTN_ROWS_MAX_PAGES / 64; ++b)
      pid[b] = (b * 64 < ns) ? a.kv.table[(size_t)seq[0] * a.kv.max_pages + min(b * 64 + lane, ns - 1)] : 0;
    ATTN_ISSUE(w, kk[0], vv[0], 0, pid, ns, slen)
    for (int pg = 0; pg < ns; pg += 2) {
      ATTN_ISSUE(w, kk[1], vv[1], pg + 1, pid, ns, slen)
#pragma unroll
      for (int j = 0; j < MEMBERS; ++j)
        if (j < nmem) attn_fold(w, kk[0], vv[0], pg, q[j], len[j], m[j], l[j], o[j]);
      ATTN_ISSUE(w, kk[0], vv[0], pg + 2, pid, ns, slen)
      if (pg + 1 < ns) {                                              // (a shared page is live for every member: beyond ns it must not be folded)
#pragma unroll
        for (int j = 0; j < MEMBERS; ++j)
          if (j < nmem) attn_fold(w, kk[1], vv[1], pg + 1, q[j], len[j], m[j], l[j], o[j]);
      }
    }
  }
  // ---- each member's own pages, entries [ns, its page count) of its own table row: attn_rows_kernel's loop, started at page ns
#pragma unroll
  for (int j = 0; j < MEMBERS; ++j) {
    if (j < nmem) {
#pragma unroll
      for (int b = 0; b < ATTN_ROWS_MAX_PAGES / 64; ++b)
        pid[b] = (b * 64 < npg[j]) ? a.kv.table[(size_t)seq[j] * a.kv.max_pages + min(b * 64 + lane, npg[j] - 1)] : 0;
      ATTN_ISSUE(w, kk[0], vv[0], ns, pid, npg[j], len[j])
      for (int pg = ns; pg < npg[j]; pg += 2) {
        ATTN_ISSUE(w, kk[1], vv[1], pg + 1, pid, npg[j], len[j])
        attn_fold(w, kk[0], vv[0], pg, q[j], len[j], m[j], l[j], o[j]);
        ATTN_ISSUE(w, kk[0], vv[0], pg + 2, pid, npg[j], len[j])
        attn_fold(w, kk[1], vv[1], pg + 1, q[j], len[j], m[j], l[j], o[j]);
      }
    }
  }
  // ---- per member: wave sum, the 8 waves' states through LDS (a slab per member: one barrier), merge and store by wave j
#pragma unroll
  for (int j = 0; j < MEMBERS; ++j) {
    if (j < nmem) {
      attn_wave_sum<LPK>(l[j], o[j]);
      if (lane < LPK) *reinterpret_cast<float4*>(&sm[j][wave][c4]) = o[j];
      if (lane == 0) { sm[j][wave][HD] = m[j]; sm[j][wave][HD + 1] = l[j]; }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < MEMBERS; ++j)
    if (j < nmem && wave == j && lane < LPK) {
      const attn_state t = attn_merge_waves<HD, NW>(sm[j], c4);
      const int e = h * HD + c4;
      attn_store_row(a.out_tiled ? out + SSRHIP_TILED_P(mem[j], e, H * HD) : out + (size_t)mem[j] * H * HD + e, t);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Causal PREFILL attention with K/V tile reuse (flash-style, fp32 on the matrix core). The decode kernel run once per query
// row re-reads a row's whole K/V prefix per row (28,704 workgroups, 97 us per layer for the bench prompt); here a workgroup owns
// 128 consecutive queries of one (sequence, head) — 4 waves x 32 queries — and walks the key tiles (32 keys) up to its diagonal:
//   * the K and V tiles are fetched ONCE per workgroup, coalesced, from the paged cache (the prefill scattered them there just
//     before) into LDS, one tile ahead in registers, and shared by the 4 waves;
//   * S^T = K . Q^T on v_mfma_f32_32x32x2_f32 (keys as M, queries as N, head_dim as K; the wave's Q slice lives in registers),
//     so that a lane holds 16 scores of ITS query column: the running max / sum of the online softmax are per-lane scalars
//     (one xor-32 exchange between the two half-waves), and the probabilities sit exactly where the B operand of the second
//     product wants them:  O^T = V^T . P^T  (head_dim as M, queries as N, keys as K) — no shuffle, no LDS round trip for P
//     (the k order of the second product follows the accumulator's row order; V is read from LDS in that order);
//   * the output row is normalised and stored straight into the [R][D] buffer the out-projection GEMM reads: no partials.
// Exact fp32 (v_mfma_f32 is an fmaf chain). Replaces F.scaled_dot_product_attention with the causal mask of ssr.py:227-255 for
// the prompt rows (activation.py:634).
typedef float f32x16 __attribute__((ext_vector_type(16)));

// KV16: the tile loader reads 2-byte entries (half the global bytes) and writes the same fp32 LDS tiles; everything behind it is unchanged
template <int HD, bool KV16>
__device__ __forceinline__ void attn_prefill_body(const ssrhip_attn_args& a, const int32_t* __restrict__ seq_start, float* __restrict__ out) {
  typedef typename kv_types<KV16>::elem kv_elem;
  typedef typename kv_types<KV16>::vec kv_vec;
  constexpr int KT = 32, LDK = HD + 4, F4 = HD / 4, NLD = KT * F4 / 256;     // float4 loads per thread per tile (HD 128: 4, 64: 2)
  constexpr int NJ = HD / 8, NMB = HD / 32;
  __shared__ __attribute__((aligned(16))) float Ks[KT * LDK];
  __shared__ __attribute__((aligned(16))) float Vs[KT * LDK];
  const int qb = blockIdx.x, h = blockIdx.y, seq = blockIdx.z;
  const int r0 = seq_start[seq], S = seq_start[seq + 1] - r0;
  if (qb * 128 >= S) return;                                               // uniform
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int H = a.kv.n_head, D = H * HD;
  const int qstride = a.q_stride ? a.q_stride : D;
  const int q0 = qb * 128 + wave * 32;                                     // this wave's first query position
  const int qi = q0 + li;                                                  // this lane's query (column of both products)
  const int last_q_wg = min(qb * 128 + 127, S - 1);
  const int ntile = last_q_wg / KT + 1;                                    // key tiles the workgroup walks
  const int my_last = (q0 < S) ? min(q0 + 31, S - 1) / KT : -1;            // last tile this wave needs (-1: no live query)

  // Q slice: lane (query li, half lh) holds Q[qi][8j + 4lh .. +3], j = 0..NJ-1 — the k order both operands of S^T use
  float4 qr[NJ];
  {
    const float* qp = a.q + (size_t)(r0 + min(qi, S - 1)) * qstride + h * HD + 4 * lh;
#pragma unroll
    for (int j = 0; j < NJ; ++j) qr[j] = ld4(qp + 8 * j);
  }
  // segment `seq` of the flattened rows belongs to cache sequence row_seq[first row] (a prefill of SOME of the engine's rows while the
  // others keep decoding); without row_seq segment i is sequence i
  const int32_t* tab = a.kv.table + (size_t)(a.row_seq ? a.row_seq[r0] : seq) * a.kv.max_pages;
  const size_t page_stride = (size_t)a.kv.n_layer * 2 * H * SSRHIP_PAGE * HD;
  const kv_elem* pool = reinterpret_cast<const kv_elem*>(a.kv.pool) + ((size_t)a.layer * 2 * H + h) * SSRHIP_PAGE * HD;
  const size_t v_off = (size_t)H * SSRHIP_PAGE * HD;

  kv_vec kreg[NLD], vreg[NLD];
  auto gload = [&](int kt) {                                               // tile kt -> registers (rows past S: clamped, masked later)
    const int key0 = kt * KT;
    const kv_elem* base = pool + (size_t)tab[key0 / SSRHIP_PAGE] * page_stride + (size_t)(key0 % SSRHIP_PAGE) * HD;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = i * 256 + t, row = idx / F4, c4 = idx % F4;
      const int rr = min(row, S - 1 - key0);                               // key0 + row < S (>= 0: key0 <= last query < S)
      kreg[i] = *reinterpret_cast<const kv_vec*>(base + (size_t)rr * HD + c4 * 4);
      vreg[i] = *reinterpret_cast<const kv_vec*>(base + v_off + (size_t)rr * HD + c4 * 4);
    }
  };
  f32x16 accO[NMB];
#pragma unroll
  for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) accO[mb][r] = 0.f;
  float m = -INFINITY, l = 0.f;

  gload(0);
  for (int kt = 0; kt < ntile; ++kt) {
    __syncthreads();                                                       // the previous tile is fully consumed
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = i * 256 + t, row = idx / F4, c4 = idx % F4;
      *reinterpret_cast<float4*>(Ks + row * LDK + c4 * 4) = kv_f4(kreg[i]);
      *reinterpret_cast<float4*>(Vs + row * LDK + c4 * 4) = kv_f4(vreg[i]);
    }
    __syncthreads();
    if (kt + 1 < ntile) gload(kt + 1);                                     // next tile under the MFMAs
    if (kt > my_last) continue;                                            // beyond this wave's diagonal (uniform per wave)
    // ---- S^T[key][query] = sum_k K[key][k] Q[query][k]
    f32x16 accS;
#pragma unroll
    for (int r = 0; r < 16; ++r) accS[r] = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const float4 kf = *reinterpret_cast<const float4*>(Ks + li * LDK + 8 * j + 4 * lh);
      accS = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qr[j].x, accS, 0, 0, 0);
      accS = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qr[j].y, accS, 0, 0, 0);
      accS = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qr[j].z, accS, 0, 0, 0);
      accS = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qr[j].w, accS, 0, 0, 0);
    }
    // ---- online softmax down the lane's query column: register r holds key kt*32 + (r&3) + 8(r>>2) + 4lh
    float mloc = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * KT + (r & 3) + 8 * (r >> 2) + 4 * lh;
      accS[r] = (key <= qi && key < S) ? accS[r] * a.scale : -INFINITY;     // causal: a query sees keys at positions <= its own
      mloc = fmaxf(mloc, accS[r]);
    }
    mloc = fmaxf(mloc, xor32_f(mloc));
    const float mnew = fmaxf(m, mloc);                                     // finite for every live query: key 0 is always visible
    const float alpha = (m > -INFINITY) ? expf(m - mnew) : 0.f;
    float lsum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      accS[r] = (mnew > -INFINITY) ? expf(accS[r] - mnew) : 0.f;
      lsum += accS[r];
    }
    lsum += xor32_f(lsum);
    l = l * alpha + lsum;
    m = mnew;
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) accO[mb][r] *= alpha;
    // ---- O^T[d][query] += sum_key V[key][d] P[key][query]: step s consumes the keys of accumulator register s (both halves)
#pragma unroll
    for (int sidx = 0; sidx < 16; ++sidx) {
      const float* vrow = Vs + ((sidx & 3) + 8 * (sidx >> 2) + 4 * lh) * LDK + li;
#pragma unroll
      for (int mb = 0; mb < NMB; ++mb) accO[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[mb * 32], accS[sidx], accO[mb], 0, 0, 0);
    }
  }
  if (qi >= S) return;
  const float inv = 1.0f / l;
  float* orow = out + (size_t)(r0 + qi) * D + h * HD;
#pragma unroll
  for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
    for (int g = 0; g < 4; ++g)                                            // registers 4g..4g+3 = head_dim mb*32 + 8g + 4lh + 0..3
      *reinterpret_cast<float4*>(orow + mb * 32 + 8 * g + 4 * lh) =
          make_float4(accO[mb][4 * g] * inv, accO[mb][4 * g + 1] * inv, accO[mb][4 * g + 2] * inv, accO[mb][4 * g + 3] * inv);
}

template <int HD>
__global__ __launch_bounds__(256) void attn_prefill_kernel(const ssrhip_attn_args a, const int32_t* __restrict__ seq_start, float* __restrict__ out) {
  attn_prefill_body<HD, false>(a, seq_start, out);
}
template <int HD>
__global__ __launch_bounds__(256) void attn_prefill_kv16_kernel(const ssrhip_attn_args a, const int32_t* __restrict__ seq_start, float* __restrict__ out) {
  attn_prefill_body<HD, true>(a, seq_start, out);
}

int check(const ssrhip_attn_args* a, const char* who) {
  SSR_REQUIRE(a && a->q && a->kv.pool && a->kv.table && a->row_len, "%s: null argument", who);
  SSR_REQUIRE(a->kv.head_dim == 64 || a->kv.head_dim == 128, "%s: head_dim %d not in {64,128}", who, a->kv.head_dim);
  SSR_REQUIRE(a->R > 0 && a->max_splits > 0 && a->max_splits <= a->kv.max_pages, "%s: bad R/max_splits", who);
  return 0;
}

// The A/B knobs of the launchers below, read together at EVERY launch (tests flip them inside one process; a captured graph keeps what it
// was captured with). A value a knob does not name selects its default.
constexpr int ATTN_KV16_DEPTH_DEFAULT = 2, ATTN_GROUP_MEMBERS_DEFAULT = 2;
struct attn_knobs {
  int vat;             // SSRHIP_ATTN_VAT = -1 | 4 | 12 (profiles/r05_microbench/decode_ab_attn_vat.log), else 8: at head_dim 128 without row_seq only
  bool head_fastest;   // SSRHIP_ATTN_HEAD_FASTEST=0: round 4's grid order of the split kernel
  int kv16_depth;      // SSRHIP_ATTN_KV16_DEPTH, pages in flight of the kv16 walk: 2 = the fp32 kernel's structure, 4 = the registers the 2-byte
                       // entries free hold two more pages
  int group_members;   // SSRHIP_ATTN_GROUP_MEMBERS, member rows per workgroup of ssrhip_attn_rows_group: 2, 4 or 8 (each costs its q and (m, l, o):
                       // 10 VGPRs at any head_dim). 2 by the launch bench (profiles/share_prompt_ab.md, 32 rows, context 520): the members' own
                       // walks run one after the other in ONE workgroup, each a chain of dependent round trips, so larger chunks save bytes and
                       // lose more time than the bytes were worth
};
attn_knobs read_attn_knobs() {
  const int vat = getenv_int("SSRHIP_ATTN_VAT", 8), depth = getenv_int("SSRHIP_ATTN_KV16_DEPTH", ATTN_KV16_DEPTH_DEFAULT);
  const int members = getenv_int("SSRHIP_ATTN_GROUP_MEMBERS", ATTN_GROUP_MEMBERS_DEFAULT);
  attn_knobs k;
  k.vat = (vat == 4 || vat == 12) ? vat : (vat < 0 ? -1 : 8);
  k.head_fastest = getenv_on("SSRHIP_ATTN_HEAD_FASTEST", true);
  k.kv16_depth = (depth == 2 || depth == 4) ? depth : ATTN_KV16_DEPTH_DEFAULT;
  k.group_members = (members == 2 || members == 4 || members == 8) ? members : ATTN_GROUP_MEMBERS_DEFAULT;
  return k;
}

// f(std::integral_constant<int, V>()) for the V among Vs that equals v (the checks in front of a launch leave no other v): a run-time
// head_dim, depth, member count or VAT becomes the kernel's template argument
template <int... Vs, class F>
void dispatch_int(const int v, F&& f) {
  (void)((v == Vs ? (f(std::integral_constant<int, Vs>()), true) : false) || ...);
}

// gridDim.z / gridDim.y carry the row index and are limited to 65535: longer row lists (a 16-row prefill has ~4k rows per
// sequence) are issued in slices of at most 65535 rows, each slice seeing its own sub-arrays (and its rows of *out, where there is one).
// A slice without row_seq keeps none: its row r would then be sequence r, which the decode launcher refuses; the combine reads none.
enum { MAX_GRID_ROWS = 65535 };
ssrhip_attn_args row_slice(const ssrhip_attn_args& a, int r0, int n, float** out = nullptr) {
  ssrhip_attn_args s = a;
  const size_t H = a.kv.n_head, HD = a.kv.head_dim;
  s.q = a.q + (size_t)r0 * (a.q_stride ? a.q_stride : H * HD);
  if (a.row_seq) s.row_seq = a.row_seq + r0;
  s.row_len = a.row_len + r0;
  s.part_o = a.part_o + (size_t)r0 * H * a.max_splits * HD;
  s.part_ml = a.part_ml + (size_t)r0 * H * a.max_splits * 2;
  s.R = n;
  if (out) *out += (size_t)r0 * H * HD;
  return s;
}

// ssrhip_attn_prefill and ssrhip_attn_prefill_kv16: one argument contract, one grid
int prefill_launch(const bool kv16, const ssrhip_attn_args* a, const int32_t* seq_start, int32_t n_seq, int32_t max_len, float* out, ssrhip_stream_t stream,
                   const char* who) {
  SSR_REQUIRE(a && a->q && a->kv.pool && a->kv.table && seq_start && out, "%s: null argument", who);
  SSR_REQUIRE(a->kv.head_dim == 64 || a->kv.head_dim == 128, "%s: head_dim %d not in {64,128}", who, a->kv.head_dim);
  SSR_REQUIRE(n_seq > 0 && n_seq <= 65535 && max_len > 0 && a->kv.n_head <= 65535, "%s: bad n_seq / max_len", who);
  SSR_REQUIRE((a->q_stride ? a->q_stride : a->kv.n_head * a->kv.head_dim) % 4 == 0, "%s: q_stride must be a multiple of 4", who);
  const dim3 grid((max_len + 127) / 128, a->kv.n_head, n_seq);
  dispatch_int<64, 128>(a->kv.head_dim, [&](auto HD) {
    constexpr int hd = decltype(HD)::value;
    if (kv16) hipLaunchKernelGGL(attn_prefill_kv16_kernel<hd>, grid, dim3(256), 0, (hipStream_t)stream, *a, seq_start, out);
    else hipLaunchKernelGGL(attn_prefill_kernel<hd>, grid, dim3(256), 0, (hipStream_t)stream, *a, seq_start, out);
  });
  SSR_LAUNCH_CHECK();
  return 0;
}

// ssrhip_attn_rows, ssrhip_attn_rows_kv16 and ssrhip_attn_rows_group_m: one argument contract, one 8-wave workgroup per (head, row)
enum rows_form { ROWS_FP32, ROWS_KV16, ROWS_GROUP };
int rows_launch(const rows_form form, const ssrhip_attn_args* a, const int32_t* chunk_head, const int32_t* n_shared, const int32_t members, float* out,
                ssrhip_stream_t stream, const char* who) {
  if (int e = check(a, who)) return e;
  SSR_REQUIRE(out && out != a->q, "%s: out is null or aliases q", who);
  SSR_REQUIRE(!a->out_tiled || a->R <= 32, "%s: tiled output needs R <= 32", who);
  SSR_REQUIRE(a->R <= MAX_GRID_ROWS, "%s: R too large", who);
  SSR_REQUIRE(a->kv.max_pages <= ATTN_ROWS_MAX_PAGES, "%s: more than %d pages per row", who, ATTN_ROWS_MAX_PAGES);
  if (form == ROWS_GROUP) {
    SSR_REQUIRE(chunk_head && n_shared, "%s: null chunk_head / n_shared", who);
    SSR_REQUIRE(members == 2 || members == 4 || members == 8, "%s: %d members per chunk not in {2,4,8}", who, members);
  }
  const dim3 grid(a->kv.n_head, a->R), block(512);
  const hipStream_t s = (hipStream_t)stream;
  dispatch_int<64, 128>(a->kv.head_dim, [&](auto HD) {
    constexpr int hd = decltype(HD)::value;
    if (form == ROWS_FP32) hipLaunchKernelGGL(attn_rows_kernel<hd>, grid, block, 0, s, *a, out);
    else if (form == ROWS_KV16)
      dispatch_int<2, 4>(read_attn_knobs().kv16_depth, [&](auto DEPTH) {
        hipLaunchKernelGGL((attn_rows_kernel<hd, true, decltype(DEPTH)::value>), grid, block, 0, s, *a, out);
      });
    else
      dispatch_int<2, 4, 8>(members, [&](auto MEMBERS) {
        hipLaunchKernelGGL((attn_rows_group_kernel<hd, decltype(MEMBERS)::value>), grid, block, 0, s, *a, chunk_head, n_shared, out);
      });
  });
  SSR_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int ssrhip_attn_prefill(const ssrhip_attn_args* a, const int32_t* seq_start, int32_t n_seq, int32_t max_len, float* out, ssrhip_stream_t stream) {
  return prefill_launch(false, a, seq_start, n_seq, max_len, out, stream, "ssrhip_attn_prefill");
}
extern "C" int ssrhip_attn_prefill_kv16(const ssrhip_attn_args* a, const int32_t* seq_start, int32_t n_seq, int32_t max_len, float* out, ssrhip_stream_t stream) {
  return prefill_launch(true, a, seq_start, n_seq, max_len, out, stream, "ssrhip_attn_prefill_kv16");
}
extern "C" int ssrhip_attn_rows(const ssrhip_attn_args* a, float* out, ssrhip_stream_t stream) {
  return rows_launch(ROWS_FP32, a, nullptr, nullptr, 0, out, stream, "ssrhip_attn_rows");
}
extern "C" int ssrhip_attn_rows_kv16(const ssrhip_attn_args* a, float* out, ssrhip_stream_t stream) {
  return rows_launch(ROWS_KV16, a, nullptr, nullptr, 0, out, stream, "ssrhip_attn_rows_kv16");
}
extern "C" int ssrhip_attn_group_members(void) { return read_attn_knobs().group_members; }
// the launch with the chunk size given by the caller (the decode engine: the size ITS chunks were cut for, whatever the knob says now)
extern "C" int ssrhip_attn_rows_group_m(const ssrhip_attn_args* a, const int32_t* chunk_head, const int32_t* n_shared, int32_t members, float* out,
                                        ssrhip_stream_t stream) {
  return rows_launch(ROWS_GROUP, a, chunk_head, n_shared, members, out, stream, "ssrhip_attn_rows_group");
}
extern "C" int ssrhip_attn_rows_group(const ssrhip_attn_args* a, const int32_t* chunk_head, const int32_t* n_shared, float* out, ssrhip_stream_t stream) {
  return ssrhip_attn_rows_group_m(a, chunk_head, n_shared, ssrhip_attn_group_members(), out, stream);
}

extern "C" int ssrhip_attn_decode(const ssrhip_attn_args* a, ssrhip_stream_t stream) {
  if (int e = check(a, "ssrhip_attn_decode")) return e;
  SSR_REQUIRE(a->part_o && a->part_ml, "ssrhip_attn_decode: null partial buffers");
  SSR_REQUIRE(a->R <= MAX_GRID_ROWS || a->row_seq, "ssrhip_attn_decode: more than %d rows need an explicit row_seq", MAX_GRID_ROWS);
  for (int r0 = 0; r0 < a->R; r0 += MAX_GRID_ROWS) {
    const int n = min(a->R - r0, (int)MAX_GRID_ROWS);
    const ssrhip_attn_args s = row_slice(*a, r0, n);
    const attn_knobs k = read_attn_knobs();
    const int hf = k.head_fastest;
    const dim3 grid(hf ? s.kv.n_head : s.max_splits, hf ? s.max_splits : s.kv.n_head, n);
    dispatch_int<64, 128>(s.kv.head_dim, [&](auto HD) {
      constexpr int hd = decltype(HD)::value;
      if (s.row_seq) hipLaunchKernelGGL((attn_decode_kernel<hd, true>), grid, dim3(256), 0, (hipStream_t)stream, s, hf, nullptr);
      else if constexpr (hd == 128)
        dispatch_int<-1, 4, 8, 12>(k.vat, [&](auto VAT) {
          hipLaunchKernelGGL((attn_decode_kernel<128, false, decltype(VAT)::value>), grid, dim3(256), 0, (hipStream_t)stream, s, hf, nullptr);
        });
      else hipLaunchKernelGGL((attn_decode_kernel<hd, false>), grid, dim3(256), 0, (hipStream_t)stream, s, hf, nullptr);
    });
    SSR_LAUNCH_CHECK();
  }
  return 0;
}

// The split kernel over a 2-byte pool with the landing cache of the <= 4-row step (attn_decode_kernel<HD, false, VAT, true>): the grid, the
// VAT choice and the grid order of ssrhip_attn_decode. Every contract error is answered before any HIP call.
extern "C" int ssrhip_attn_decode_kv16(const ssrhip_attn_args* a, const float* land, ssrhip_stream_t stream) {
  if (int e = check(a, "ssrhip_attn_decode_kv16")) return e;
  SSR_REQUIRE(a->part_o && a->part_ml, "ssrhip_attn_decode_kv16: null partial buffers");
  SSR_REQUIRE(land, "ssrhip_attn_decode_kv16: null landing cache");
  SSR_REQUIRE(!a->row_seq, "ssrhip_attn_decode_kv16: row_seq must be NULL (row r is sequence r: the landing cache has one page per row)");
  SSR_REQUIRE(a->R <= MAX_GRID_ROWS, "ssrhip_attn_decode_kv16: more than %d rows", MAX_GRID_ROWS);
  SSR_REQUIRE(a->layer >= 0 && a->layer < SSRHIP_PAGE && a->layer < a->kv.n_layer,
              "ssrhip_attn_decode_kv16: layer %d outside the cache's %d layers or the landing page's %d positions", a->layer, a->kv.n_layer, SSRHIP_PAGE);
  const attn_knobs k = read_attn_knobs();
  const int hf = k.head_fastest;
  const dim3 grid(hf ? a->kv.n_head : a->max_splits, hf ? a->max_splits : a->kv.n_head, a->R);
  if (a->kv.head_dim == 128)
    dispatch_int<-1, 4, 8, 12>(k.vat, [&](auto VAT) {
      hipLaunchKernelGGL((attn_decode_kernel<128, false, decltype(VAT)::value, true>), grid, dim3(256), 0, (hipStream_t)stream, *a, hf, land);
    });
  else hipLaunchKernelGGL((attn_decode_kernel<64, false, -1, true>), grid, dim3(256), 0, (hipStream_t)stream, *a, hf, land);
  SSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssrhip_attn_combine(const ssrhip_attn_args* a, float* out, ssrhip_stream_t stream) {
  if (int e = check(a, "ssrhip_attn_combine")) return e;
  SSR_REQUIRE(out && a->part_o && a->part_ml, "ssrhip_attn_combine: out or the partial buffers are null");
  SSR_REQUIRE(!a->out_tiled || a->R <= 32, "ssrhip_attn_combine: tiled output needs R <= 32");
  for (int r0 = 0; r0 < a->R; r0 += MAX_GRID_ROWS) {
    const int n = min(a->R - r0, (int)MAX_GRID_ROWS);
    float* o = out;
    const ssrhip_attn_args s = row_slice(*a, r0, n, &o);
    dispatch_int<64, 128>(s.kv.head_dim, [&](auto HD) {
      constexpr int hd = decltype(HD)::value, hpw = 256 / hd;          // heads per one-wave workgroup
      hipLaunchKernelGGL(attn_combine_kernel<hd>, dim3((s.kv.n_head + hpw - 1) / hpw, n), dim3(64), 0, (hipStream_t)stream, s, o);
    });
    SSR_LAUNCH_CHECK();
  }
  return 0;
}
