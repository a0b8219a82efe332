// gemv_pair.h — what the pair launches of gemv.hip (fp32 weights) and gemv_pair_w16.hip (packed bf16 weights) have in common: everything
// about the hand-off that does not look at a weight — the PAIR_* constants, the launch descriptor, the gather sweep and the edge role
// (waves 8-11) with its time-bounded spin, its give-up flag and the reset of the next launch's granules. One definition, so that the two
// translation units publish, gather and give up alike. The comment block above gemv_pair_kernel (gemv.hip) describes the protocol.
// Taken out of gemv.hip only because every kernel of gemv.hip kept its ISA (profiles/w16_pair_isa.md, tools/isa_diff.py).
#pragma once
#include "common.h"
#include "gemv_shared.h"

namespace {

constexpr int PAIR_D = 2048, PAIR_NE = 4, PAIR_TH = SEG_TH + 64 * PAIR_NE, PAIR_GRAN = 2 * PAIR_D, PAIR_PF = 3, PAIR_DEPTH = 4, PAIR_NUWA = 8;
constexpr int PAIR_SPINS = 4000000;                       // a second bound only; the first is PAIR_WAIT_TICKS
constexpr long long PAIR_WAIT_TICKS = 100000000;           // 1 s of wall_clock64 (100 MHz)
struct PairK {
  GemvK a, b;
  unsigned long long* gran;        // this launch's granules [PAIR_GRAN]: index n * 2 + row
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

// ---- the edge role (waves 8-11). SA = segments per row of A (partial sums to add), NPRE = barriers of A's prologue to keep company
template <int SA, int NPRE>
__device__ __forceinline__ void pair_edge_role(const PairK& p, int e, int lane, const float* partA, float* xs, size_t* kvoff) {
  constexpr int B = 2, RA = 8;
  const ssrhip_gemv_args& a = p.a.a;
  const ssrhip_gemv_args& bb = p.b.a;
  const int rA0 = (int)blockIdx.x * RA;
  RowEpi efinA = {0.f, 0.f};
  if (e == 0 && lane < RA * B) {
    efinA.bias = a.bias ? a.bias[rA0 + (lane >> 1)] : 0.f;
    efinA.resid = a.y[(size_t)(lane & 1) * a.y_stride + rA0 + (lane >> 1)];
    p.gran_next[(size_t)blockIdx.x * (RA * B) + lane] = 0ull;       // reset the NEXT pair launch's granules (this workgroup's 16 of them)
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
    const int r = lane >> 1, b = lane & 1, n = rA0 + r;
    float v = 0.f;
    for (int s2 = 0; s2 < SA; ++s2) v += partA[(r * SA + s2) * B + b];
    v += efinA.bias;
    const float out = efinA.resid + v;
    a.y[(size_t)b * a.y_stride + n] = out;
    const unsigned long long gval = ((unsigned long long)1u << 32) | (unsigned long long)__float_as_uint(out);
    __hip_atomic_store(p.gran + (size_t)n * 2 + b, gval, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
    pair_sweep8(p.gran + (size_t)e * 1024 + lane * 2, g);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      all = all && (__float_as_uint(g[i][1]) == 1u) && (__float_as_uint(g[i][3]) == 1u);
      const int gi = e * 1024 + (i >> 2) * 512 + (i & 3) * 128 + lane * 2;   // granule index of g[i].xy (row 0 of output gi / 2); .zw: row 1
      xs[(gi >> 1)] = g[i][0];
      xs[PAIR_D + (gi >> 1)] = g[i][2];
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

}  // namespace
