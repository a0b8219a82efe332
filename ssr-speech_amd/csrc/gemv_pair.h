// gemv_pair.h — what the pair launches have in common, whatever they stream (fp32 weights: gemv.hip at 2 rows, gemv_pair4.hip at 4;
// packed bf16: gemv_pair_w16.hip; e4m3 codes: gemv_pair_w8.hip). First everything about the hand-off that does not look at a weight —
// the PAIR_* constants, the launch descriptor, the gather sweep and the edge role (waves 8-11) with its time-bounded spin, its give-up
// flag and the reset of the next launch's granules, templated on the row count. Then the streaming role's phases (waves 0-7), written
// once against a stream policy of gemv_wstream.h: A's straight-line units, the merge form's requests and its two units, and the B phase
// from barrier (1b) to the epilogue. One definition, so that every translation unit publishes, gathers, gives up and streams alike.
// The comment block above gemv_pair_kernel (gemv.hip) describes the protocol. A piece stands here only where the kernels that call it
// kept their ISA or passed the admission rule of profiles/pair_refactor_ab.md (tools/isa_diff.py); that note also lists what stayed
// written out in the kernels and why. The host side of the launches is gemv_pair_host.h.
#pragma once
#include "common.h"
#include "gemv_shared.h"
#include "gemv_wstream.h"

namespace {

constexpr int PAIR_D = 2048, PAIR_NE = 4, PAIR_TH = SEG_TH + 64 * PAIR_NE, PAIR_GRAN = 2 * PAIR_D, PAIR_PF = 3, PAIR_DEPTH = 4, PAIR_NUWA = 8;
constexpr int PAIR4_B = 4, PAIR4_GRAN = PAIR4_B * PAIR_D;   // the 4-row launches (gemv_pair4.hip): 8192 granules per buffer
constexpr int PAIR_SPINS = 4000000;                       // a second bound only; the first is PAIR_WAIT_TICKS
constexpr long long PAIR_WAIT_TICKS = 100000000;           // 1 s of wall_clock64 (100 MHz)
struct PairK {
  GemvK a, b;
  unsigned long long* gran;        // this launch's granules [B * PAIR_D]: index n * B + row
  unsigned long long* gran_next;   // the next pair launch's buffer: reset here
  int* gave_up;
};
typedef float pair_v4f __attribute__((ext_vector_type(4)));
// eight 16-byte agent-scope loads of the sweep, issued together and waited for together; hipcc must not see them (its wait-count
// bookkeeping would otherwise serialise them against the streaming waves' loads at the join)
__device__ __forceinline__ void pair_sweep8(const unsigned long long* p, pair_v4f (&g)[8]) {
  asm volatile(
      "global_load_dwordx4 %0, %8, off sc1\n\tglobal_load_dwordx4 %1, %8, off offset:1024 sc1\n\t"
      "global_load_dwordx4 %2, %8, off offset:2048 sc1\n\tglobal_load_dwordx4 %3, %8, off offset:3072 sc1\n\t"
      "global_load_dwordx4 %4, %9, off sc1\n\tglobal_load_dwordx4 %5, %9, off offset:1024 sc1\n\t"
      "global_load_dwordx4 %6, %9, off offset:2048 sc1\n\tglobal_load_dwordx4 %7, %9, off offset:3072 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(g[0]), "=&v"(g[1]), "=&v"(g[2]), "=&v"(g[3]), "=&v"(g[4]), "=&v"(g[5]), "=&v"(g[6]), "=&v"(g[7])
      : "v"(p), "v"(p + 512)
      : "memory");
}

// ---- the edge role (waves 8-11) of a B-row launch (B = 2 or 4). SA = segments per row of A (partial sums to add), NPRE = barriers of A's
// prologue to keep company. Granules: 8-byte {value, tag = 1}, agent-scope stores, value and tag in ONE store; granule index n * B + row,
// B * 2048 per buffer; x' in LDS: B x 2048 floats. Each of the 4 edge waves gathers a quarter of the buffer, B / 2 sweeps of 1024 granules.
template <int B, int SA, int NPRE>
__device__ __forceinline__ void pair_edge_role(const PairK& p, int e, int lane, const float* partA, float* xs, size_t* kvoff) {
  static_assert(B == 2 || B == 4, "a sweep covers 1024 granules; an edge wave owns B * 512 of them");
  constexpr int RA = 8, NSW = B / 2, LB = (B == 2) ? 1 : 2;        // LB = log2(B)
  const ssrhip_gemv_args& a = p.a.a;
  const ssrhip_gemv_args& bb = p.b.a;
  const int rA0 = (int)blockIdx.x * RA;
  RowEpi efinA = {0.f, 0.f};
  if (e == 0 && lane < RA * B) {
    efinA.bias = a.bias ? a.bias[rA0 + (lane >> LB)] : 0.f;
    efinA.resid = a.y[(size_t)(lane & (B - 1)) * a.y_stride + rA0 + (lane >> LB)];
    p.gran_next[(size_t)blockIdx.x * (RA * B) + lane] = 0ull;       // reset the NEXT pair launch's granules (this workgroup's 8 * B of them)
  }
  if (bb.epi == SSRHIP_EPI_QKV_APPEND && e == 1 && lane < B) {      // kv_append_bases()'s arithmetic for batch row `lane`, as element offsets
    const int pos = bb.kv_pos[lane];
    const int page = bb.kv.table[(size_t)lane * bb.kv.max_pages + (pos / SSRHIP_PAGE)];
    const size_t k0 = ((((size_t)page * bb.kv.n_layer + bb.layer) * 2 + 0) * bb.kv.n_head) * SSRHIP_PAGE + (pos % SSRHIP_PAGE);
    const size_t v0 = ((((size_t)page * bb.kv.n_layer + bb.layer) * 2 + 1) * bb.kv.n_head) * SSRHIP_PAGE + (pos % SSRHIP_PAGE);
    kvoff[lane * 2 + 0] = k0 * bb.kv.head_dim;
    kvoff[lane * 2 + 1] = v0 * bb.kv.head_dim;
  }
#pragma unroll
  for (int i = 0; i < NPRE; ++i) __syncthreads();
  __syncthreads();                                                  // (1)
  if (e == 0 && lane < RA * B) {
    // A's epilogue — finalize()'s RESIDUAL arm — into the residual stream and, tagged, into this launch's granules
    const int r = lane >> LB, b = lane & (B - 1), n = rA0 + r;
    float v = 0.f;
    for (int s2 = 0; s2 < SA; ++s2) v += partA[(r * SA + s2) * B + b];
    v += efinA.bias;
    const float out = efinA.resid + v;
    a.y[(size_t)b * a.y_stride + n] = out;
    const unsigned long long gval = ((unsigned long long)1u << 32) | (unsigned long long)__float_as_uint(out);
    __hip_atomic_store(p.gran + (size_t)n * B + b, gval, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();                                                  // (1b)
  // gather this wave's quarter of the granules: one round trip per sweep, until every tag is this launch's. Once ANY launch on this
  // workspace has given up (results are garbage from there on and the host will raise at its next poll) the later launches do not wait
  // ~half a second each any more: a chain that cannot get its workgroups resident together costs one long stall, not one per launch
  pair_v4f g[8];
  bool done = false;
  const int max_spins = (*p.gave_up != 0) ? 64 : PAIR_SPINS;
  // the bound is TIME (round 6): ~1 s of the constant 100 MHz clock, looked at every 256 sweeps. The sweep count alone (rounds 5) meant
  // anything from 1 s on an idle GPU to well over 9 s when a hundred CUs' worth of edge waves poll the same lines (tests/test_gpu_pair_guard.py)
  const long long t_begin = wall_clock64();
  for (int spin = 0; spin < max_spins && !done; ++spin) {
    bool all = true;
#pragma unroll
    for (int h = 0; h < NSW; ++h) {
      const int base = e * (1024 * NSW) + h * 1024;
      // (the two row counts keep the address forms they had when each had a role of its own: hipcc tells them apart by an s_waitcnt in the merge kernels)
      pair_sweep8(p.gran + (NSW == 1 ? (size_t)e * 1024 : (size_t)base) + lane * 2, g);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        all = all && (__float_as_uint(g[i][1]) == 1u) && (__float_as_uint(g[i][3]) == 1u);
        const int gi = base + (i >> 2) * 512 + (i & 3) * 128 + lane * 2;   // granule index of g[i].xy (even: an even batch row of output gi / B); .zw: the next row
        xs[(gi & (B - 1)) * PAIR_D + (gi >> LB)] = g[i][0];
        xs[((gi & (B - 1)) + 1) * PAIR_D + (gi >> LB)] = g[i][2];
      }
    }
    done = __all(all);
    if (!done) {
      __builtin_amdgcn_s_sleep(2);
      if ((spin & 255) == 255 && wall_clock64() - t_begin > PAIR_WAIT_TICKS) break;
    }
  }
  if (!done && lane == 0) *p.gave_up = 1;
  __syncthreads();                                                  // (2)
  __syncthreads();                                                  // (3)
  __syncthreads();                                                  // (4)
}

// ---- the streaming role (waves 0-7), once for every stream S (WsF32 / WsB16 / WsE4 of gemv_wstream.h) and row count B. A wave's ring
// holds PAIR_DEPTH units; unit j of a phase lives in slot (j + EARLY) % PAIR_DEPTH and works on local row (wave + 8 j) >> SH of the
// phase's rows (SH = log2 of the segments per row). Wg = the lane's pointer into unit 0's row block: rows + seg * SEG + lane * S::LANE.

// NUW units, straight-line: use a piece, then re-request it in place for unit j + DEPTH; park each unit's partial sums (times sc[j])
template <class S, int B, int NUW, int SH, int EARLY, class Sc>
__device__ __forceinline__ void pair_units(const typename S::Elem* Wg, int K, typename S::Slot (&w)[PAIR_DEPTH], const float4 (&xr)[B][4],
                                           const Sc& sc, float* part, int wave, int lane) {
  constexpr int DEPTH = PAIR_DEPTH;
#pragma unroll
  for (int j = 0; j < NUW; ++j) {
    float acc[B][2];
#pragma unroll
    for (int b = 0; b < B; ++b) acc[b][0] = acc[b][1] = 0.f;
    S::template dot<B>(w[(j + EARLY) % DEPTH], xr, acc, j + DEPTH < NUW, [&] { return Wg + (size_t)((wave + SEG_NW * (j + DEPTH)) >> SH) * K; });
    S::template park<B>(acc, sc[j], part, wave + SEG_NW * j, lane);
  }
}

// the FFN2 form's A phase: the wave's first DEPTH units requested (HBM, non-temporal), then its NUWA units
template <class S, int B, int NUWA, int SHA, class Sc>
__device__ __forceinline__ void pair_stream_a(const typename S::Elem* WgA, int K, typename S::Slot (&w)[PAIR_DEPTH], const float4 (&xr)[B][4],
                                              const Sc& scA, float* partA, int wave, int lane) {
#pragma unroll
  for (int j = 0; j < PAIR_DEPTH; ++j) S::request(w[j], WgA + (size_t)((wave + SEG_NW * j) >> SHA) * K);
  pair_units<S, B, NUWA, SHA, 0>(WgA, K, w, xr, scA, partA, wave, lane);
}

// the merge form's requests at entry: the wave's two units of A (K = 2048: SHA = 1) and, EARLY = 2, B's units 0 and 1 into the ring slots
// A leaves free (pair_stream_b's addresses: 2 segments per row, unit u = row (wave + 8 u) / 2 of this workgroup's RB rows)
template <class S, int NUWB, int EARLY>
__device__ __forceinline__ void pair_merge_request(const typename S::Elem* WgA, int K, const typename S::Elem* Wb, int Kb,
                                                   typename S::Slot (&w)[PAIR_DEPTH], int wave, int lane) {
  constexpr int RB = NUWB * SEG_NW / 2;
#pragma unroll
  for (int j = 0; j < 2; ++j) S::request(w[j], WgA + (size_t)((wave + SEG_NW * j) >> 1) * K);
  if constexpr (EARLY == 2) {
    const typename S::Elem* WgB = Wb + (size_t)((int)blockIdx.x * RB) * Kb + (wave & 1) * SEG + lane * S::LANE;
#pragma unroll
    for (int j = 0; j < 2; ++j) S::request(w[2 + j], WgB + (size_t)((wave + SEG_NW * j) >> 1) * Kb);
  }
}

// from barrier (1) on: B = LayerNorm + Linear on x' (the segu kernel of the stream at <B, PRO_LAYERNORM, NUWB, 4>, operation for
// operation). Barriers (1b), (2), (4) and seg_layernorm's (3) pair with pair_edge_role's.
// EARLY (the merge forms of 2 rows): B's units 0 .. EARLY - 1 were requested at kernel ENTRY (pair_merge_request); what is requested here
// starts behind them. PFX = units in flight behind barrier (1b), i.e. in front of the gather's loads (PAIR_PF = 3 unless a lab macro says 4).
template <class S, int B, int NUWB, int EARLY, int PFX, class Sc>
__device__ __forceinline__ void pair_stream_b(const PairK& p, const typename S::Elem* Wb, const Sc& scB, int t, int lane, int wave, float4 (&xr)[B][4],
                                              typename S::Slot (&w)[PAIR_DEPTH], const RowEpi& efinB, float* partB, float* aux, const float* xs,
                                              const size_t* kvoff) {
  constexpr int DEPTH = PAIR_DEPTH, PF = PFX, SB = 2, SHB = 1, RB = NUWB * SEG_NW / SB;
  static_assert(PFX >= EARLY && PFX <= PAIR_DEPTH, "units requested at (1b) start behind the early ones and fit the ring");
  static_assert(EARLY == 0 || EARLY == 2, "ring slots 2 and 3 are the ones the merge form's A phase leaves free");
  static_assert(DEPTH <= NUWB, "units in flight");
  const ssrhip_gemv_args& bb = p.b.a;
  const int rB0 = (int)blockIdx.x * RB, segB = wave & (SB - 1);
  const int bfin = t % B, rfinB = min(t / B, RB - 1), nfinB = rB0 + rfinB;
  const typename S::Elem* WgB = Wb + (size_t)rB0 * bb.K + segB * SEG + lane * S::LANE;
  __syncthreads();                                                  // (1b) wave 8 has issued the publish
  // B's first units: PF of them now, the rest behind the gather
#pragma unroll
  for (int j = EARLY; j < PF; ++j) S::request(w[(j + EARLY) % DEPTH], WgB + (size_t)((wave + SEG_NW * j) >> SHB) * bb.K);
  __syncthreads();                                                  // (2) x' is in LDS
  seg_load_x<B>(xr, xs, PAIR_D, segB, lane);
#pragma unroll
  for (int j = PF; j < DEPTH; ++j) S::request(w[(j + EARLY) % DEPTH], WgB + (size_t)((wave + SEG_NW * j) >> SHB) * bb.K);
  seg_layernorm<B>(xr, aux, SB, bb.K, bb.ln_eps, wave, lane);       // its barrier is (3)
  pair_units<S, B, NUWB, SHB, EARLY>(WgB, bb.K, w, xr, scB, partB, wave, lane);
  __syncthreads();                                                  // (4)
  if (t < RB * B) {
    // K / V append addresses: resolved by the edge role (wave 9) while this role streamed — the kv_pos -> page table -> pool chain costs
    // the streaming waves nothing here (in gemv_segu_kernel it is two scalar round trips per wave under the first units' latency)
    float* kvb[2] = {bb.kv.pool + kvoff[bfin * 2], bb.kv.pool + kvoff[bfin * 2 + 1]};
    seg_finish_row<B>(p.b, 0, partB, SB, rfinB, nfinB, bfin, efinB, kvb);
  }
}

}  // namespace
