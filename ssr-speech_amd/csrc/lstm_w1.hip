// lstm_w1.hip — the split-operand LSTM step (csrc/lstm_split.hip) for a recurrent matrix whose every value IS a bf16 value (a
// weight_dtype="bf16" codec: DESIGN.md Part I.31). The exact split of such a W_hh has two planes of zeros; this step streams the one plane
// that is left and issues the three products that remain of lstm_step_split_kernel's six:
//
//     w2h0, w0h2, w1h1, w1h0, w0h1, w0h0      ->      w0h2, w0h1, w0h0          (the survivors, in the order the list visits them)
//
// A dropped product has an all-zero A operand and a finite B operand (|h| < 1): it adds +-0 to an accumulator that started at +0 and so is
// never -0 — the accumulator keeps its bits. The products that remain meet each accumulator in the same order, and everything outside the
// k-loop is lstm_split_step.h's text: the three-plane step's result on the three planes of the same matrix BIT FOR BIT, and the same
// `hsplit` / `cbuf` state, so the two steps can take turns inside one sequence.
//
// Operands, in fragment order (one wave-level dwordx4 load = one contiguous KiB = one MFMA operand):
//     w_split [C/16 unit blocks][4 waves][KS k-steps][2 row blocks][64 lanes][8 bf16]       plane 0 of lstm_split.hip's layout, the slice q = 0
//     hsplit  [2 (t parity)][ceil(B/64)][4 waves][KS][2 batch blocks][3 planes][64 lanes][8 bf16]      lstm_split.hip's, byte for byte
// Per k-step a wave loads 2 KiB of W and 6 of h (8 loads where the three-plane step has 12) and issues 12 MFMAs (24). A k-step's MFMA block
// is half as long, so DEPTH k-steps in flight are half the prefetch distance in time: DEPTH 8 exists beside 2 and 4 (SSRHIP_LSTM_W1_DEPTH),
// and measured SLOWER than 4 at C = 512 (10.5 against 9.6 us per step at 256 items, against 11.8 for the three-plane step): it stays off.
#include <atomic>
#include "lstm_split_step.h"

namespace {

// index (in uint16 units) of the KiB block of the one-plane `w_split`: [unit block][wave][kstep][row block]
__device__ __forceinline__ size_t w1_block(int ub, int wave, int ks, int s, int mb) { return ((((size_t)ub * 4 + wave) * ks + s) * 2 + mb) * 512; }

template <int DEPTH>
__global__ __launch_bounds__(LS_TH, 1) void lstm_step_w1_kernel(const ssrhip_lstm_args a, const int t, const unsigned short* __restrict__ hp,
                                                                  unsigned short* __restrict__ hn, const int KS) {
  constexpr int PB[3] = {2, 1, 0};                                       // w0h2, w0h1, w0h0: what is left of PA / PB of the three-plane step
  extern __shared__ __attribute__((aligned(16))) float part[];           // [4 waves][64 n][LS_PS]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ub = blockIdx.x, bg = blockIdx.y;

  ls_requests rq;
  ls_request(a, t, tid, ub, bg, rq);            // gin / c / skip of the finishing phase, requested first

  // ---- the K loop: DEPTH k-steps of operands in flight (8 KiB-loads each), 12 MFMAs per k-step
  const unsigned short* wsrc = reinterpret_cast<const unsigned short*>(a.w_split) + w1_block(ub, wave, KS, 0, 0) + lane * 8;
  const unsigned short* hsrc = hp + frag_block(bg, wave, KS, 0, 0, 0) + lane * 8;
  bf16x8 fa[DEPTH][2], fb[DEPTH][2][3];
  auto load = [&](int slot, int s) {
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      fa[slot][blk] = *reinterpret_cast<const bf16x8*>(wsrc + (size_t)(s * 2 + blk) * 512);
#pragma unroll
      for (int q = 0; q < 3; ++q) fb[slot][blk][q] = *reinterpret_cast<const bf16x8*>(hsrc + ((size_t)(s * 2 + blk) * 3 + q) * 512);
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    load(d, d);
    __builtin_amdgcn_sched_barrier(0);           // slot by slot, as the loop refills them: the loop head then waits for slot 0 only
  }
  for (int s = 0; s < KS; s += DEPTH) {                                 // KS % DEPTH == 0 (checked by the launcher)
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
#pragma unroll
      for (int pq = 0; pq < 3; ++pq)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb)
            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[d][mb], fb[d][nb][PB[pq]], acc[mb][nb], 0, 0, 0);
      load(d, min(s + d + DEPTH, KS - 1));       // unconditional, as in the three-plane step: no load under a run-time branch
      __builtin_amdgcn_sched_barrier(0);         // the refill stays HERE, DEPTH - 1 MFMA blocks (384 cycles each) ahead of its use
    }
  }

  ls_finish(a, t, tid, wave, ub, bg, acc, part, rq, hn, KS);
}

std::atomic<int64_t> g_lstm_w1_launches{0};

// SSRHIP_LSTM_W1_DEPTH=8: eight k-steps in flight where KS % 8 == 0 (the codec's own C = 512). Read at every call (tests and the A/B
// tools flip it inside one process); anything else keeps lstm_split.hip's rule, DEPTH 4 where KS % 4 == 0 and 2 otherwise.
int w1_depth(int KS) {
  if (KS % 8 == 0 && getenv_int("SSRHIP_LSTM_W1_DEPTH", 0) == 8) return 8;
  return KS % 4 == 0 ? 4 : 2;
}

}  // namespace

size_t ssrhip_lstm_split_hplane_elems(int B, int C);                                   // lstm_split.hip
bool ssrhip_lstm_split_eligible(const ssrhip_lstm_args* a);

extern "C" int64_t ssrhip_lstm_w1_launches(void) { return g_lstm_w1_launches.load(); }

extern "C" int ssrhip_lstm_layer_w1(const ssrhip_lstm_args* a, ssrhip_stream_t stream) {
  SSR_REQUIRE(a && a->gin && a->w_hh && a->out && a->hbuf && a->cbuf, "ssrhip_lstm_layer_w1: null argument");
  SSR_REQUIRE(a->B > 0 && a->T > 0 && a->C > 0 && a->C % 16 == 0 && a->C <= 4096, "ssrhip_lstm_layer_w1: need C %% 16 == 0, C <= 4096");
  const int t_lo = a->t_begin, t_hi = a->t_end > 0 ? a->t_end : a->T;
  SSR_REQUIRE(t_lo >= 0 && t_lo < t_hi && t_hi <= a->T, "ssrhip_lstm_layer_w1: bad time window [%d, %d) of %d", t_lo, t_hi, a->T);
  SSR_REQUIRE(a->w_split && a->hsplit, "ssrhip_lstm_layer_w1: needs the one-plane w_split and hsplit");
  const bool small_b = a->B <= 4 && (a->C == 256 || a->C == 512 || a->C == 1024 || a->C == 2048);
  if (small_b || !ssrhip_lstm_split_eligible(a)) return 1;             // where ssrhip_lstm_layer would not take the split step: nothing launched
  hipStream_t s = (hipStream_t)stream;
  const int KS = a->C / 64;                                            // even: C % 128 == 0
  const size_t he = ssrhip_lstm_split_hplane_elems(a->B, a->C);
  unsigned short* hs = reinterpret_cast<unsigned short*>(a->hsplit);
  if (t_lo == 0) hipLaunchKernelGGL(zero_u32_kernel, dim3(1024), dim3(256), 0, s, reinterpret_cast<unsigned*>(hs), (long)he);   // both buffers: h_0 = 0
  SSR_RAISE_LDS(ls_lds(), lstm_step_w1_kernel<2>);
  SSR_RAISE_LDS(ls_lds(), lstm_step_w1_kernel<4>);
  SSR_RAISE_LDS(ls_lds(), lstm_step_w1_kernel<8>);
  const int depth = w1_depth(KS);
  dim3 grid(a->C / LS_UN, (a->B + LS_BN - 1) / LS_BN);
  for (int t = t_lo; t < t_hi; ++t) {
    const unsigned short* hp = hs + (size_t)(t & 1) * he;
    unsigned short* hn = hs + (size_t)((t + 1) & 1) * he;
    switch (depth) {
      case 8: hipLaunchKernelGGL((lstm_step_w1_kernel<8>), grid, dim3(LS_TH), ls_lds(), s, *a, t, hp, hn, KS); break;
      case 4: hipLaunchKernelGGL((lstm_step_w1_kernel<4>), grid, dim3(LS_TH), ls_lds(), s, *a, t, hp, hn, KS); break;
      default: hipLaunchKernelGGL((lstm_step_w1_kernel<2>), grid, dim3(LS_TH), ls_lds(), s, *a, t, hp, hn, KS); break;
    }
  }
  SSR_LAUNCH_CHECK();
  g_lstm_w1_launches += t_hi - t_lo;
  return 0;
}
