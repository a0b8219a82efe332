// resblock_split.hip — SEANetResnetBlock (audiocraft/modules/seanet.py:16-60; true_skip, dilation 1, kernels 3 and 1) for C = 64 and
// C = 128 channels as ONE kernel on the bf16 matrix cores with exactly split fp32 operands (round 4).
//
//     y[t] = x[t] + b1 + W1 . ELU( b3 + W3 . ELU( x[t-1 : t+2] ) )          W3: [C/2][3][C], W1: [C][C/2]
//
// The arithmetic is csrc/gemm_split.hip's: every fp32 operand is the exact sum of three bf16 pieces, the six largest cross products are
// accumulated in fp32 (error against fp64 no larger than the fp32 FMA chain's). What round 3's resblock_chain_split_kernel<128> left on
// the table (55.6 ms per call at 256 clips x 30 s against 9.6 ms of matrix time and 12.6 ms of HBM time) and what is done
// about it here:
//   * W3 / W1 were split from fp32 again by every workgroup at every k-step: the host splits them ONCE (ssrhip_resblock_args.w3_split /
//     w1_split, three bf16 planes each) and the kernel brings the tiles global -> LDS by DMA, one step ahead, no registers, no ds_write;
//   * the x window was loaded, ELU'd and split once PER TAP (three times per element): a tile of ELU(x) — 130 rows x 32 channels, three
//     bf16 planes, XOR-swizzled 64-byte rows — is built once per channel tile and the three taps read it at row offsets 0 / 1 / 2;
//   * the C/2-channel intermediate made a round trip through LDS (fp32, split again by every reading wave): stage 1 runs TRANSPOSED
//     (H^T[h][t] = W3 . ELU(x)^T, the time steps as the N dimension), so that a lane's accumulator registers are 16 hidden channels of
//     ITS time step — exactly the A operand stage 2 wants (row = time step, k = hidden channel) once W1's k order follows the
//     accumulator's row order (the host permutes W1's columns; resblock64_kernel's trick, carried over to the bf16 pipe). A wave owns
//     32 time steps through both stages; waves exchange nothing but the shared weight / input tiles;
//   * two barriers per 16-wide k-step with 12 MFMAs between them: one barrier per 32-wide step with 24 MFMAs per wave between them
//     (two at the channel-tile boundaries), 4 waves per workgroup;
//   * a 32-wide step is ~0.3 us of MFMAs, an L2 -> LDS DMA ~1 us: the weight tiles go through a ring of FOUR LDS slots, three steps ahead
//     of their use (first version: one ahead, 36.6 ms per call at C = 128 — every step waited for its tile). The DMA is issued as inline
//     asm and counted by hand (vmcnt): through the builtin hipcc makes every ds_read wait for every LDS-DMA issued before it.
// Replaces the two strided-view GEMMs (or the round-3 fused kernels) for `SEANetResnetBlock` at C in {64, 128}; results are NOT
// bit-identical to them (same class of error; tests: G7 per-module fixtures and the end-to-end codec fixtures, 2e-4 / 2e-5).
#include <stdlib.h>
#include <algorithm>
using std::min;
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bfx2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

__device__ __forceinline__ float elu_r(float v) { return elu1(v); }         // the codec's one ELU (common.h: hardware exponential, |error| <= 1.2e-7)

// the first piece alone: the value rounded (nearest even) to bf16   (gemm_split.hip round4)
__device__ __forceinline__ void round4r(const float4 v, bf16x4& out) {
  const f32x2 r[2] = {{v.x, v.y}, {v.z, v.w}};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const unsigned bits = __builtin_bit_cast(unsigned, __builtin_convertvector(r[h], bfx2));
    out[2 * h] = (short)(bits & 0xFFFFu);
    out[2 * h + 1] = (short)(bits >> 16);
  }
}
// exact three-way split of 4 consecutive values: piece p of element e in out[p][e]   (gemm_split.hip)
__device__ __forceinline__ void split4r(const float4 v, bf16x4 (&out)[3]) {
  f32x2 r[2] = {{v.x, v.y}, {v.z, v.w}};
#pragma unroll
  for (int p = 0; p < 3; ++p) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bfx2 b = __builtin_convertvector(r[h], bfx2);
      const unsigned bits = __builtin_bit_cast(unsigned, b);
      out[p][2 * h] = (short)(bits & 0xFFFFu);
      out[p][2 * h + 1] = (short)(bits >> 16);
      if (p < 2) {
        const f32x2 back = {__builtin_bit_cast(float, bits << 16), __builtin_bit_cast(float, bits & 0xFFFF0000u)};
        r[h] = r[h] - back;
      }
    }
  }
}
// NA pieces of 4 consecutive values: 3 = the exact split, 1 = the value rounded to bf16
template <int NA>
__device__ __forceinline__ void pieces4r(const float4 v, bf16x4 (&out)[NA]) {
  if constexpr (NA == 3) split4r(v, out);
  else round4r(v, out[0]);
}

constexpr int RB_BM = 128, RB_TH = 256, RB_NW = 4;        // time steps per workgroup, threads, waves
constexpr int RB_ER = RB_BM + 2 + 2;                      // rows of the ELU(x) tile (130 used; padded to a multiple of 4 for the swizzle period)
constexpr int RB_EP = RB_ER * 64;                         // bytes per bf16 plane of the tile (64-byte rows = 32 channels)
// bytes of one weight tile of NP planes: W3 [NP][C/2][32 k] = W1 [NP][C][16 k] = 32 NP C (96 C for the three planes of an fp32 weight)
constexpr int rb_wtile(int CC, int NP = 3) { return 32 * NP * CC; }
constexpr int NS1X(int CC) { return 3 * (CC / 32); }
// weight tiles in LDS = RING: the one in use + RING - 1 in flight (a 32-wide step is ~0.3 us of MFMAs, an L2 -> LDS DMA ~1 us)
// (the ELU(x) tile is the activation operand: three planes whatever the weights are — or ONE, `NA` = 1, where the activation is rounded to
// bf16 instead of split: DESIGN I.32. The 16-byte epilogue turns its blocks through 4 KB per wave at the front of the tile's region, so
// the region is never smaller than that: the ring behind it may still be read by a slower wave)
constexpr int rb_eregion(int NA = 3) { return NA * RB_EP > RB_NW * 4096 ? NA * RB_EP : RB_NW * 4096; }
constexpr int rb_lds(int CC, int RING, int NP = 3, int NA = 3) { return rb_eregion(NA) + RING * rb_wtile(CC, NP); }
static_assert(rb_lds(128, 2) == 49920 && rb_lds(128, 4) == 74496 && rb_lds(64, 2) == 37632 && rb_lds(64, 4) == 49920, "LDS of the three-plane kernels");
static_assert(rb_lds(128, 2, 1) == 33536 && rb_lds(128, 4, 1) == 41728 && rb_lds(64, 2, 1) == 29440 && rb_lds(64, 4, 1) == 33536, "LDS of the one-plane kernels");
static_assert(rb_eregion() == 3 * RB_EP && rb_eregion(1) == 16384, "the ELU(x) tile's region");
static_assert(rb_lds(128, 2, 1, 1) == 24576 && rb_lds(128, 4, 1, 1) == 32768 && rb_lds(64, 2, 1, 1) == 20480 && rb_lds(64, 4, 1, 1) == 24576, "LDS of the one-piece kernels");
typedef int i32x4r __attribute__((ext_vector_type(4)));

// LDS-DMA as inline asm: with the builtin hipcc applies its conservative alias rule — every ds_read behind an LDS-DMA first waits for
// the DMA (seen in the ISA: s_waitcnt vmcnt right behind the request), which makes a prefetch distance impossible. The asm form is
// invisible to that pass; its completion is counted by hand (wait_vm below). M0 = LDS byte address of the wave's KiB, restored afterwards.
__device__ __forceinline__ void dma_kib(const i32x4r rsrc, unsigned voff, unsigned lds_addr) {
  unsigned keep;
  asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(lds_addr), "s"(rsrc) : "memory");
}
// s_waitcnt vmcnt(n) for a wave-uniform runtime n (the instruction takes an immediate)
__device__ __forceinline__ void wait_vm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;   // n >= 12: a stricter wait is always correct
  }
}

// Cost attribution hooks for tools/resblock_lab.hip (KO = 0 in the product: every `if constexpr` below folds away): knock one component
// out and time the rest, or (RB_PROF) leave 100 MHz timestamps of wave 0's phases in LDS and dump them for a sample of the workgroups.
enum { RB_KO_WAIT = 1, RB_KO_ESTORE = 2, RB_KO_RESID = 4, RB_KO_MFMA = 8, RB_KO_DMA = 16, RB_KO_ELOAD = 32, RB_KO_STORE = 64, RB_PROF = 128 };
constexpr int RB_NSTAMP = 64;
constexpr int RB_RDEPTH = 1;                             // residual blocks (16 registers each) requested ahead of the one being stored
__device__ unsigned* g_rb_prof = nullptr;                 // [sampled workgroup][RB_NSTAMP]

#define RB_KERNEL resblock_split_dma_kernel      // three planes per matrix: the exact split of fp32 weights (ssrhip_resblock)
#define RB_NP 3
#define RB_NA 3
#include "resblock_split_kernel.h"
#undef RB_KERNEL
#undef RB_NP
// one plane per matrix (ssrhip_resblock_w1): same register budget; 29-42 KB of LDS instead of 37-74 KB, so by LDS even the ring of 4 leaves
// room for three workgroups per CU at C = 128 (three planes: two) and four at C = 64 — as many as the registers allow
#define RB_KERNEL resblock_w1_dma_kernel
#define RB_NP 1
#include "resblock_split_kernel.h"
#undef RB_KERNEL
// one plane per matrix and ONE piece per activation (ssrhip_resblock_a1, DESIGN I.32): ELU(x) and ELU(H + b3) rounded to bf16 where the
// kernels above split them, one product per k block in both stages; 20-32 KB of LDS
#undef RB_NA
#define RB_NA 1
#define RB_KERNEL resblock_a1_dma_kernel
#include "resblock_split_kernel.h"
#undef RB_KERNEL
#undef RB_NP
#undef RB_NA

}  // namespace

// launched by ssrhip_resblock (resblock.hip) when the caller supplied the weight planes
int ssrhip_resblock_split_launch(const ssrhip_resblock_args* a, hipStream_t s) {
  SSR_REQUIRE(a->C == 64 || a->C == 128, "ssrhip_resblock (split planes): C=%d not in {64, 128}", a->C);
  SSR_REQUIRE((size_t)(a->T + 2) * a->C * 4 < 0x7FFFFFF0ull, "ssrhip_resblock (split planes): item too long");
  dim3 grid((a->T + RB_BM - 1) / RB_BM, a->B);
  // Defaults: the ring of 2 (one tile ahead, three workgroups per CU; any other SSRHIP_RESBLOCK_RING: three ahead, two per CU) and the dword
  // epilogue. Both measured faster here than their A/B alternatives (profiles/r04_microbench/resblock_pmc.log, resblock_lab_ab.log)
  const int wide = ssr_codec_knobs().resblock_wide;
  if (ssr_codec_knobs().resblock_ring == 2) {
    if (a->C == 128) hipLaunchKernelGGL((resblock_split_dma_kernel<128, 2>), grid, dim3(RB_TH), rb_lds(128, 2), s, *a, wide);
    else hipLaunchKernelGGL((resblock_split_dma_kernel<64, 2>), grid, dim3(RB_TH), rb_lds(64, 2), s, *a, wide);
  } else if (a->C == 128) {
    SSR_RAISE_LDS(rb_lds(128, 4), resblock_split_dma_kernel<128, 4>);      // 74,496 B: the only form above the 64 KB a kernel gets unasked
    hipLaunchKernelGGL((resblock_split_dma_kernel<128, 4>), grid, dim3(RB_TH), rb_lds(128, 4), s, *a, wide);
  } else {
    hipLaunchKernelGGL((resblock_split_dma_kernel<64, 4>), grid, dim3(RB_TH), rb_lds(64, 4), s, *a, wide);
  }
  SSR_LAUNCH_CHECK();
  return 0;
}

void ssr_codec_w1_count(void);      // gemm_split.hip: the one-plane launch counter (ssrhip_codec_w1_launches)

// One plane per matrix: see ssrhip.h. Answers 1, launching nothing, wherever ssrhip_resblock would not take the DMA kernel above.
extern "C" int ssrhip_resblock_w1(const ssrhip_resblock_args* a, ssrhip_stream_t stream) {
  SSR_REQUIRE(a && a->x && a->y && a->b3 && a->b1, "ssrhip_resblock_w1: null argument");
  SSR_REQUIRE(a->w3_split && a->w1_split, "ssrhip_resblock_w1: w3_split and w1_split (one bf16 plane each) are both required");
  SSR_REQUIRE(a->B > 0 && a->B <= 65535 && a->T > 0, "ssrhip_resblock_w1: bad B / T");
  const codec_knobs& k = ssr_codec_knobs();
  if (!(a->C == 64 || a->C == 128) || !k.gemm_split || !k.resblock_dma) return 1;
  SSR_REQUIRE((size_t)(a->T + 2) * a->C * 4 < 0x7FFFFFF0ull, "ssrhip_resblock_w1: item too long");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((a->T + RB_BM - 1) / RB_BM, a->B);
  // The epilogue follows the three-plane launcher's switch. The ring: 2 only when SSRHIP_RESBLOCK_RING says so, else three tiles ahead —
  // the registers (146-152 at C = 128, 112 at C = 64), not the 33-42 KB of LDS, bound the workgroups per CU at either depth (3 and 4)
  const int wide = k.resblock_wide;
  if (k.resblock_w1_ring == 2) {
    if (a->C == 128) hipLaunchKernelGGL((resblock_w1_dma_kernel<128, 2>), grid, dim3(RB_TH), rb_lds(128, 2, 1), s, *a, wide);
    else hipLaunchKernelGGL((resblock_w1_dma_kernel<64, 2>), grid, dim3(RB_TH), rb_lds(64, 2, 1), s, *a, wide);
  } else if (a->C == 128) hipLaunchKernelGGL((resblock_w1_dma_kernel<128, 4>), grid, dim3(RB_TH), rb_lds(128, 4, 1), s, *a, wide);
  else hipLaunchKernelGGL((resblock_w1_dma_kernel<64, 4>), grid, dim3(RB_TH), rb_lds(64, 4, 1), s, *a, wide);
  SSR_LAUNCH_CHECK();
  ssr_codec_w1_count();
  return 0;
}

void ssr_codec_a1_count(void);      // gemm_split.hip: the bf16-activation launch counter (ssrhip_codec_a1_launches)

// One plane per matrix, one piece per activation: see ssrhip.h. ssrhip_resblock_w1's contract, conditions and ring default.
extern "C" int ssrhip_resblock_a1(const ssrhip_resblock_args* a, ssrhip_stream_t stream) {
  SSR_REQUIRE(a && a->x && a->y && a->b3 && a->b1, "ssrhip_resblock_a1: null argument");
  SSR_REQUIRE(a->w3_split && a->w1_split, "ssrhip_resblock_a1: w3_split and w1_split (one bf16 plane each) are both required");
  SSR_REQUIRE(a->B > 0 && a->B <= 65535 && a->T > 0, "ssrhip_resblock_a1: bad B / T");
  const codec_knobs& k = ssr_codec_knobs();
  if (!(a->C == 64 || a->C == 128) || !k.gemm_split || !k.resblock_dma) return 1;
  SSR_REQUIRE((size_t)(a->T + 2) * a->C * 4 < 0x7FFFFFF0ull, "ssrhip_resblock_a1: item too long");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((a->T + RB_BM - 1) / RB_BM, a->B);
  const int wide = k.resblock_wide;
  if (k.resblock_w1_ring == 2) {
    if (a->C == 128) hipLaunchKernelGGL((resblock_a1_dma_kernel<128, 2>), grid, dim3(RB_TH), rb_lds(128, 2, 1, 1), s, *a, wide);
    else hipLaunchKernelGGL((resblock_a1_dma_kernel<64, 2>), grid, dim3(RB_TH), rb_lds(64, 2, 1, 1), s, *a, wide);
  } else if (a->C == 128) hipLaunchKernelGGL((resblock_a1_dma_kernel<128, 4>), grid, dim3(RB_TH), rb_lds(128, 4, 1, 1), s, *a, wide);
  else hipLaunchKernelGGL((resblock_a1_dma_kernel<64, 4>), grid, dim3(RB_TH), rb_lds(64, 4, 1, 1), s, *a, wide);
  SSR_LAUNCH_CHECK();
  ssr_codec_a1_count();
  return 0;
}
