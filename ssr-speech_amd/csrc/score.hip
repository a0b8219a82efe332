// score.hip — cross entropy and rank of the target per row of logits: the per-position numbers behind the reference's training loss and
// top-10 accuracy (models/ssr.py:362-366: F.cross_entropy and MulticlassAccuracy(top_k=10) over the masked positions). The masks and the
// means are host/torch bookkeeping (score.py); this kernel reads each row of logits exactly once.
//
// One wave64 per row, four rows per 256-thread workgroup. The target's logit is read first; then one pass over the row with dwordx4
// loads (a scalar tail when card is not a multiple of 4) keeps, per lane, an online max with its rescaled fp32 exp-sum and the count of
// logits strictly above the target's. The lanes then combine with the DPP / permlane reductions of common.h.
#include "common.h"

namespace {

// fold four logits into the running (max, sum of exp(x - max)) pair: one rescale when the max moves (rare after the first columns),
// then four exponentials against the current max. The -inf start rescales a zero sum (0 * exp(-inf) = 0).
__device__ __forceinline__ void online_add4(float& mx, float& sum, float4 v) {
  const float m4 = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
  if (m4 > mx) {
    sum *= expf(mx - m4);
    mx = m4;
  }
  sum += (expf(v.x - mx) + expf(v.y - mx)) + (expf(v.z - mx) + expf(v.w - mx));
}

__global__ __launch_bounds__(256) void xent_rank_kernel(const float* __restrict__ logits, int ld, int card, const int32_t* __restrict__ target,
                                                        int M, float* __restrict__ nll, int32_t* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                       // whole waves leave together: the reductions below never see a partial wave
  const float* lr = logits + (size_t)row * ld;
  const int t = target[row];
  if ((unsigned)t >= (unsigned)card) {         // a target outside the row: no read, a visible NaN (the host validates ids before launching)
    if (lane == 0) { nll[row] = NAN; rank[row] = -1; }
    return;
  }
  const float tl = lr[t];
  float mx = -INFINITY, sum = 0.f;
  int cnt = 0;
  const int c4 = card & ~3;
  for (int c = lane * 4; c < c4; c += 256) {
    const float4 v = ld4(lr + c);
    online_add4(mx, sum, v);
    cnt += (v.x > tl && c != t) + (v.y > tl && c + 1 != t) + (v.z > tl && c + 2 != t) + (v.w > tl && c + 3 != t);
  }
  const int c = c4 + lane;
  if (c < card) {
    const float v = lr[c];
    if (v > mx) {
      sum *= expf(mx - v);
      mx = v;
    }
    sum += expf(v - mx);
    cnt += v > tl && c != t;
  }
  const float gmx = wave_max(mx);
  const float part = sum > 0.f ? sum * expf(mx - gmx) : 0.f;     // lanes that saw no column hold (−inf, 0)
  const float gsum = wave_sum(part);
  const float gcnt = wave_sum((float)cnt);                       // <= card < 2^24: exact in fp32
  if (lane == 0) {
    nll[row] = (gmx - tl) + logf(gsum);
    rank[row] = (int32_t)gcnt;
  }
}

}  // namespace

extern "C" int ssrhip_xent_rank(const float* logits, int32_t ld, int32_t card, const int32_t* target, int32_t M, float* nll, int32_t* rank,
                                ssrhip_stream_t stream) {
  SSR_REQUIRE(logits && target && nll && rank, "ssrhip_xent_rank: null argument");
  SSR_REQUIRE(M > 0 && card > 0 && ld >= card && ld % 4 == 0, "ssrhip_xent_rank: bad shape (M=%d card=%d ld=%d)", M, card, ld);
  SSR_REQUIRE((reinterpret_cast<uintptr_t>(logits) & 15) == 0, "ssrhip_xent_rank: logits must be 16-byte aligned");
  hipLaunchKernelGGL(xent_rank_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld, card, target, M, nll, rank);
  SSR_LAUNCH_CHECK();
  return 0;
}
