// gemv_pair4.h — the hand-off of the 4-row pair launches (gemv_pair4.hip): gemv_pair.h's protocol, unchanged in kind, at four batch rows.
// The 2-row edge role indexes granules, partial sums and epilogue lanes by `lane & 1` / `lane >> 1`; a template argument for the row count
// would have moved the 2-row kernels' code, so the 4-row role stands here on its own (the 2-row kernels keep their ISA: profiles/pair4_isa.md).
// Shared with gemv_pair.h: PairK, pair_sweep8, PAIR_D, PAIR_NE, PAIR_TH, PAIR_SPINS, PAIR_WAIT_TICKS and the three-buffer cycle.
//   * 8-byte {value, tag = 1} granules, agent-scope stores, value and tag in ONE store; granule index n * 4 + row, 8192 per buffer;
//   * every launch resets the next launch's buffer (this workgroup's 32 granules of it);
//   * the gather: each of the 4 edge waves owns 2048 granules = two sweeps of eight 16-byte loads; time-bounded spin, gave_up flag,
//     64-spin short-circuit once the flag is set;
//   * x' in LDS: 4 x 2048 floats.
#pragma once
#include "gemv_pair.h"

namespace {

constexpr int PAIR4_B = 4, PAIR4_GRAN = PAIR4_B * PAIR_D;   // 8192 granules per buffer

// ---- the edge role (waves 8-11). SA = segments per row of A (partial sums to add), NPRE = barriers of A's prologue to keep company
template <int SA, int NPRE>
__device__ __forceinline__ void pair4_edge_role(const PairK& p, int e, int lane, const float* partA, float* xs, size_t* kvoff) {
  constexpr int B = PAIR4_B, RA = 8;
  const ssrhip_gemv_args& a = p.a.a;
  const ssrhip_gemv_args& bb = p.b.a;
  const int rA0 = (int)blockIdx.x * RA;
  RowEpi efinA = {0.f, 0.f};
  if (e == 0 && lane < RA * B) {
    efinA.bias = a.bias ? a.bias[rA0 + (lane >> 2)] : 0.f;
    efinA.resid = a.y[(size_t)(lane & 3) * a.y_stride + rA0 + (lane >> 2)];
    p.gran_next[(size_t)blockIdx.x * (RA * B) + lane] = 0ull;       // reset the NEXT pair launch's granules (this workgroup's 32 of them)
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
    const int r = lane >> 2, b = lane & 3, n = rA0 + r;
    float v = 0.f;
    for (int s2 = 0; s2 < SA; ++s2) v += partA[(r * SA + s2) * B + b];
    v += efinA.bias;
    const float out = efinA.resid + v;
    a.y[(size_t)b * a.y_stride + n] = out;
    const unsigned long long gval = ((unsigned long long)1u << 32) | (unsigned long long)__float_as_uint(out);
    __hip_atomic_store(p.gran + (size_t)n * B + b, gval, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();                                                  // (1b)
  // gather this wave's quarter of the granules (2048 of them: two sweeps of 1024) until every tag is this launch's; gemv_pair.h's bounds
  pair_v4f g[8];
  bool done = false;
  const int max_spins = (*p.gave_up != 0) ? 64 : PAIR_SPINS;
  const long long t_begin = wall_clock64();
  for (int spin = 0; spin < max_spins && !done; ++spin) {
    bool all = true;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int base = e * 2048 + h * 1024;
      pair_sweep8(p.gran + (size_t)base + lane * 2, g);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        all = all && (__float_as_uint(g[i][1]) == 1u) && (__float_as_uint(g[i][3]) == 1u);
        const int gi = base + (i >> 2) * 512 + (i & 3) * 128 + lane * 2;   // granule index of g[i].xy (even: batch row 0 or 2 of output gi / 4); .zw: the next row
        xs[(gi & 3) * PAIR_D + (gi >> 2)] = g[i][0];
        xs[((gi & 3) + 1) * PAIR_D + (gi >> 2)] = g[i][2];
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

}  // namespace
