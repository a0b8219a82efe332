// lstm_split_step.h — what a step of the split-operand LSTM recurrence does OUTSIDE its k-loop, shared by the two step kernels that differ
// only in the planes W_hh comes in: lstm_step_split_kernel (csrc/lstm_split.hip, three planes) and lstm_step_w1_kernel (csrc/lstm_w1.hip,
// one). The requests of gin / c / skip, the LDS meeting of the four partial tiles, the cell update and the split of h_t into `hsplit` are
// the same text for both, so the state a step leaves (`cbuf`, `hsplit`, `out`) has ONE format and the two kernels can take turns on it.
// The k-loops stay written out in their own units: tests/test_isa_guards.py and tests/test_lstm_w1_isa.py pin what each compiles to.
#pragma once
#include <stdlib.h>
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bfx2 __attribute__((ext_vector_type(2)));

constexpr int LS_TH = 256, LS_BN = 64, LS_UN = 16, LS_PS = 65;         // threads, batch rows / hidden units per workgroup, LDS row stride (floats)
constexpr int ls_lds() { return 4 * LS_BN * LS_PS * 4; }               // four partial tiles [n][m], rows padded to 65: conflict-free stores

__device__ __forceinline__ float sigmoid_(float v) { return 1.0f / (1.0f + expf(-v)); }

// index (in uint16 units) of the KiB block (64 lanes x 8 bf16) of `hsplit` / the three-plane `w_split`: [outer][wave][kstep][block][plane]
__device__ __forceinline__ size_t frag_block(int outer, int wave, int ks, int s, int blk, int q) {
  return (((((size_t)outer * 4 + wave) * ks + s) * 2 + blk) * 3 + q) * 512;
}

// exact three-way split of one value (gemm_split.hip's split4, one lane wide)
__device__ __forceinline__ void split1(float v, unsigned short (&p)[3]) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const f32x2 r = {v, 0.f};
    const bfx2 b = __builtin_convertvector(r, bfx2);                  // v_cvt_pk_bf16_f32 (RNE)
    const unsigned bits = __builtin_bit_cast(unsigned, b) & 0xFFFFu;
    p[q] = (unsigned short)bits;
    v -= __builtin_bit_cast(float, bits << 16);
  }
}

// ---- what the finishing phase needs, requested first: thread p = tid + 256 i finishes unit u = p % 16 of batch row bl = p / 16
// (16 consecutive lanes = 16 consecutive hidden units of one item: 64-byte runs of gin / c / skip / out)
struct ls_requests {
  float pg[4][4], pc[4], ps[4];
};
__device__ __forceinline__ void ls_request(const ssrhip_lstm_args& a, const int t, const int tid, const int ub, const int bg, ls_requests& rq) {
  const int C = a.C;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = tid + LS_TH * i, u = p & 15, bl = p >> 4;
    const int b = min(bg * LS_BN + bl, a.B - 1), j = ub * LS_UN + u;
    const float* gin = a.gin + (size_t)b * a.gin_bstride + (size_t)t * 4 * C + j;
#pragma unroll
    for (int g = 0; g < 4; ++g) rq.pg[i][g] = gin[(size_t)g * C];
    rq.pc[i] = (t == 0) ? 0.f : a.cbuf[(size_t)b * C + j];
    rq.ps[i] = a.skip ? a.skip[(size_t)b * a.skip_bstride + (size_t)t * C + j] : 0.f;
  }
}

// ---- the four partial tiles meet in LDS: part[wave][n][m]; accumulator register r of block (mb, nb) = D[32 mb + (r&3) + 8(r>>2) + 4 lh][32 nb + li];
// then every thread finishes its 4 (unit, batch) pairs: gates, cell update, out, and h_t split into `hn` at its fragment positions
__device__ __forceinline__ void ls_finish(const ssrhip_lstm_args& a, const int t, const int tid, const int wave, const int ub, const int bg,
                                          const f32x16 (&acc)[2][2], float* part, const ls_requests& rq, unsigned short* __restrict__ hn, const int KS) {
  const int lane = tid & 63, li = lane & 31, lh = lane >> 5, C = a.C;
  float* mine = part + (size_t)wave * LS_BN * LS_PS;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mine[(nb * 32 + li) * LS_PS + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh] = acc[mb][nb][r];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = tid + LS_TH * i, u = p & 15, bl = p >> 4;
    const int b = bg * LS_BN + bl, j = ub * LS_UN + u;
    float gt[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float* src = part + (size_t)bl * LS_PS + g * 16 + u;
      gt[g] = ((src[0] + src[LS_BN * LS_PS]) + (src[2 * LS_BN * LS_PS] + src[3 * LS_BN * LS_PS])) + rq.pg[i][g];     // fixed order: deterministic
    }
    if (b < a.B) {
      const float cn = sigmoid_(gt[1]) * rq.pc[i] + sigmoid_(gt[0]) * tanhf(gt[2]);
      const float hv = sigmoid_(gt[3]) * tanhf(cn);
      a.cbuf[(size_t)b * C + j] = cn;
      float o = hv + rq.ps[i];                                         // y = lstm(x) + x on the last layer (lstm.py:21-23); ps == 0 otherwise
      if (a.out_act == SSRHIP_ACT_ELU) o = elu1(o);
      a.out[(size_t)b * a.out_bstride + (size_t)t * C + j] = o;
      // h_t[b][j] as the next step's B operand: k = j -> wave j / (C/4), k-step (j % (C/4)) / 16, lane half (j % 16) / 8, element j % 8
      unsigned short pcs[3];
      split1(hv, pcs);
      const int kq = C >> 2, w2 = j / kq, s2 = (j % kq) >> 4, lh2 = (j >> 3) & 1, e2 = j & 7;
      unsigned short* dst = hn + frag_block(bg, w2, KS, s2, bl >> 5, 0) + (lh2 * 32 + (bl & 31)) * 8 + e2;
#pragma unroll
      for (int q = 0; q < 3; ++q) dst[q * 512] = pcs[q];
    }
  }
}

__global__ __launch_bounds__(256) void zero_u32_kernel(unsigned* p, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] = 0u;
}

}  // namespace
