// noise.hip — the opt-in device-side source of the sampler's Exp(1) noise (DESIGN.md Part I.21): a counter-based generator writes the
// draws of steps [first_step, first_step + n_steps) of a slot straight into the engine's noise[n_utt][max_steps][K][card] buffer, where the
// sampler (embed_sample.hip, untouched) reads them through use_noise = 1. A translation unit of its own: no other kernel's code moves.
//
// The stream (include/ssrhip.h ssrhip_noise_philox; the host replica is ssr_speech_amd/philox.py): Philox4x32-10, key = the utterance's
// 64-bit seed (low word, high word), counter = (b, t, 0x6e6f6973, 0) with t the step within the utterance and b the block; word j of block
// b is element e = 4b + j of the step's flattened [K][card] tensor. w -> n = w >> 9, u = (n + 0.5) * 2^-23 (exact in fp32), q = -logf(u)
// with the precise library logarithm: q in [5.96e-8, 16.64], never 0, never inf.
#include "common.h"

namespace {

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr int NOISE_THREADS = 256;

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(PHILOX_M0, c.x), lo0 = PHILOX_M0 * c.x;
    const unsigned hi1 = __umulhi(PHILOX_M1, c.z), lo1 = PHILOX_M1 * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  return c;
}

__device__ __forceinline__ float exp1_of_word(unsigned w) {
  // (2n + 1) < 2^24 is an fp32 integer and the scale a power of two: u is exact
  const float u = (float)(2u * (w >> 9) + 1u) * 0x1p-24f;
  return -logf(u);
}

// grid = (blocks of a step / NOISE_THREADS, the longest segment's steps, segments); one Philox block = 4 elements per thread. VEC: every
// step's row starts on a 16-byte boundary and ends with a whole block (K * card % 4 == 0, an aligned buffer), so a block is ONE 16-byte
// store; otherwise scalar stores of the block's elements below K * card (the last block is ragged). The segment table travels by value in
// the kernel arguments; the launcher has checked every segment against n_utt and max_steps.
template <bool VEC>
__global__ __launch_bounds__(NOISE_THREADS) void noise_philox_kernel(const ssrhip_noise_args a) {
  const ssrhip_noise_segment s = a.seg[blockIdx.z];
  const int t = blockIdx.y;
  if (t >= s.n_steps) return;
  const int kc = a.K * a.card;
  const int b = blockIdx.x * NOISE_THREADS + threadIdx.x;
  const int e0 = 4 * b;
  if (e0 >= kc) return;
  const int step = s.first_step + t;
  const uint4 w = philox4x32_10(make_uint4((unsigned)b, (unsigned)step, 0x6e6f6973u, 0u), s.seed_lo, s.seed_hi);
  const size_t at = ((size_t)s.slot * a.max_steps + step) * (size_t)kc + e0;
  const int n = VEC ? 4 : min(4, kc - e0);
  float q[4];
  const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = exp1_of_word(ws[j]);
  if (VEC) {
    *reinterpret_cast<float4*>(a.noise + at) = make_float4(q[0], q[1], q[2], q[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) a.noise[at + j] = q[j];
  }
  if (a.words) {                                       // tests: the raw words beside the values
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) a.words[at + j] = ws[j];
  }
}

}  // namespace

extern "C" int ssrhip_noise_sizeof(void) { return (int)sizeof(ssrhip_noise_args); }

extern "C" int ssrhip_noise_philox(const ssrhip_noise_args* a, ssrhip_stream_t stream) {
  SSR_REQUIRE(a && a->noise, "ssrhip_noise_philox: null argument");
  SSR_REQUIRE(a->n_seg >= 0 && a->n_seg <= SSRHIP_NOISE_MAX_SEGMENTS, "ssrhip_noise_philox: %d segments (at most %d per launch)", a->n_seg,
              SSRHIP_NOISE_MAX_SEGMENTS);
  SSR_REQUIRE(a->n_utt >= 1 && a->max_steps >= 1 && a->K >= 1 && a->K <= SSRHIP_MAX_CODEBOOKS && a->card >= 1 &&
                  (long)a->K * a->card <= 0x7fffffffL / 4,
              "ssrhip_noise_philox: bad n_utt=%d / max_steps=%d / K=%d / card=%d", a->n_utt, a->max_steps, a->K, a->card);
  int most = 0;
  for (int i = 0; i < a->n_seg; ++i) {
    const ssrhip_noise_segment& s = a->seg[i];
    SSR_REQUIRE(s.slot >= 0 && s.slot < a->n_utt, "ssrhip_noise_philox: segment %d names slot %d of %d", i, s.slot, a->n_utt);
    SSR_REQUIRE(s.first_step >= 0 && s.n_steps >= 0, "ssrhip_noise_philox: segment %d has the negative range (%d, %d)", i, s.first_step,
                s.n_steps);
    SSR_REQUIRE((long)s.first_step + s.n_steps <= a->max_steps, "ssrhip_noise_philox: segment %d ends at step %ld of %d", i,
                (long)s.first_step + s.n_steps, a->max_steps);
    if (s.n_steps > most) most = s.n_steps;
  }
  if (most == 0) return 0;                             // nothing to draw
  SSR_REQUIRE(most <= 65535, "ssrhip_noise_philox: a segment of %d steps (at most 65535 per launch)", most);
  const int kc = a->K * a->card, blocks = (kc + 3) / 4;
  const dim3 grid((blocks + NOISE_THREADS - 1) / NOISE_THREADS, most, a->n_seg);
  if (kc % 4 == 0 && ((uintptr_t)a->noise & 15) == 0)
    hipLaunchKernelGGL(noise_philox_kernel<true>, grid, dim3(NOISE_THREADS), 0, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL(noise_philox_kernel<false>, grid, dim3(NOISE_THREADS), 0, (hipStream_t)stream, *a);
  SSR_LAUNCH_CHECK();
  return 0;
}
