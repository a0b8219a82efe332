// gemv_wstream.h — the weight streams of the <= 4-row GEMV kernels: how a lane loads and widens packed bf16 pieces (gemv_w16.hip) and
// e4m3 codes (gemv_w8.hip), and, on top of that, the three stream policies (fp32, bf16, e4m3) the pair launches are written against
// (gemv_pair.h). One definition of the widening, so that the single launches and the pair launches of a stream run the same
// conversions and the same fmaf order (bit-identical results); every kernel that includes this kept its ISA when the helpers moved here
// (profiles/pair_refactor_ab.md).
#pragma once
#include "common.h"
#include "gemv_shared.h"

namespace {

// ---- packed bf16 (include/ssrhip.h SSRHIP_W16_INDEX)
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

// ---- packed e4m3 codes (include/ssrhip.h SSRHIP_W8_INDEX)
typedef unsigned w8_v4u __attribute__((ext_vector_type(4)));
typedef float w8_v2f __attribute__((ext_vector_type(2)));

// 16 codes of a streamed-once weight row: non-temporal 16-byte load (global_load_dwordx4 ... nt)
__device__ __forceinline__ w8_v4u ld16_nt(const uint8_t* p) { return __builtin_nontemporal_load(reinterpret_cast<const w8_v4u*>(p)); }

// the float4 of one dword: code m sits in byte m (v_cvt_pk_f32_fp8 widens bytes 0, 1 or, with the word select, bytes 2, 3)
__device__ __forceinline__ float4 w8_wide(const unsigned d) {
  const w8_v2f lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)d, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)d, true);
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}

// one unit against the lane's x: gemv_seg_kernel's `acc[b][i & 1] = dot4(w[i], xr[b][i], acc[b][i & 1])` for i = 0..3
template <int B>
__device__ __forceinline__ void w8_unit(const w8_v4u u, const float4 (&xr)[B][4], float (&acc)[B][2]) {
  const float4 w0 = w8_wide(u.x), w1 = w8_wide(u.y), w2 = w8_wide(u.z), w3 = w8_wide(u.w);
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b][0] = dot4(w0, xr[b][0], acc[b][0]);
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b][1] = dot4(w1, xr[b][1], acc[b][1]);
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b][0] = dot4(w2, xr[b][2], acc[b][0]);
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b][1] = dot4(w3, xr[b][3], acc[b][1]);
}

// one unit done: seg_park with the row's scale applied to the partial sum that is parked (u = local_row * S + seg)
template <int B>
__device__ __forceinline__ void w8_park(const float (&acc)[B][2], float sc, float* part, int u, int lane) {
  float mine = 0.f;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const float sum = wave_sum(acc[b][0] + acc[b][1]);
    if (lane == b) mine = sum;
  }
  if (lane < B) part[lane + u * B] = mine * sc;
}

// one unit done, seg_park (gemv_shared.h) with the index written part[u * B + lane]: the form of w16_segu_kernel's written-out park and
// of the fp32 merge pair kernel's (gemv_shared.h notes that hipcc tells the two forms apart by a VGPR)
template <int B>
__device__ __forceinline__ void seg_park_ub(const float (&acc)[B][2], float* part, int u, int lane) {
  float mine = 0.f;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const float sum = wave_sum(acc[b][0] + acc[b][1]);
    if (lane == b) mine = sum;
  }
  if (lane < B) part[u * B + lane] = mine;
}

// ---- the stream policies. A unit is one (row, 1024-element segment of K): 4 KiB of fp32, 2 KiB of bf16, 1 KiB of e4m3. Each policy says
//   Elem / LANE    the stored element and how many of them a lane's share of one load holds (the lane's offset into a unit is lane * LANE);
//   Slot           the ring slot of one unit in flight;
//   request        the unit's non-temporal loads into a slot, `row` = the lane's pointer into the unit;
//   dot<B>         the unit against the lane's x; with `refill` (a constant once the unit loop is unrolled) each piece is re-requested in
//                  place from next(), the lane's pointer into the successor unit, right behind its use, between sched_barriers (use, THEN overwrite);
//   load_scales    the scales-at-entry hook: e4m3 requests the row scales of a wave's N units into a float[N] and `fence` keeps them in
//                  front of the first codes; the other two pass a NoScales (sc[j] reads 1 and park ignores it) and both are empty;
//   park<B>        the wave's partial sums of the unit into part[u][b], times the row's scale where there is one.
struct NoScales {
  __device__ __forceinline__ float operator[](int) const { return 1.f; }
};

struct WsF32 {
  typedef float Elem;
  typedef float4 Slot[4];
  static constexpr int LANE = 4;
  static __device__ __forceinline__ void request(Slot& s, const float* row) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = ld_nt(row + i * 256);
  }
  template <int B, class Next>
  static __device__ __forceinline__ void dot(Slot& s, const float4 (&xr)[B][4], float (&acc)[B][2], bool refill, const Next& next) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int b = 0; b < B; ++b) acc[b][i & 1] = dot4(s[i], xr[b][i], acc[b][i & 1]);
      if (refill) {
        __builtin_amdgcn_sched_barrier(0);
        s[i] = ld_nt(next() + i * 256);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  template <int N, int SH> static __device__ __forceinline__ void load_scales(NoScales&, const float*, int, int) {}
  static __device__ __forceinline__ void fence() {}
  template <int B>
  static __device__ __forceinline__ void park(const float (&acc)[B][2], float, float* part, int u, int lane) { seg_park<B>(acc, part, u, lane); }
};

struct WsB16 {
  typedef uint16_t Elem;
  typedef w16_v4u Slot[2];
  static constexpr int LANE = 8;
  static __device__ __forceinline__ void request(Slot& s, const uint16_t* row) {
#pragma unroll
    for (int i = 0; i < 2; ++i) s[i] = ld16_nt(row + i * 512);
  }
  template <int B, class Next>
  static __device__ __forceinline__ void dot(Slot& s, const float4 (&xr)[B][4], float (&acc)[B][2], bool refill, const Next& next) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      w16_piece<B>(s[i], i, xr, acc);
      if (refill) {
        __builtin_amdgcn_sched_barrier(0);
        s[i] = ld16_nt(next() + i * 512);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  template <int N, int SH> static __device__ __forceinline__ void load_scales(NoScales&, const float*, int, int) {}
  static __device__ __forceinline__ void fence() {}
  template <int B>
  static __device__ __forceinline__ void park(const float (&acc)[B][2], float, float* part, int u, int lane) { seg_park_ub<B>(acc, part, u, lane); }
};

struct WsE4 {
  typedef uint8_t Elem;
  typedef w8_v4u Slot;
  static constexpr int LANE = 16;
  static __device__ __forceinline__ void request(Slot& s, const uint8_t* row) { s = ld16_nt(row); }
  template <int B, class Next>
  static __device__ __forceinline__ void dot(Slot& s, const float4 (&xr)[B][4], float (&acc)[B][2], bool refill, const Next& next) {
    w8_unit<B>(s, xr, acc);
    if (refill) {
      __builtin_amdgcn_sched_barrier(0);                            // use, THEN overwrite in place
      s = ld16_nt(next());
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // the scales of a wave's N units, unit j on row r0 + ((wave + 8 j) >> SH) of `rows`: requested at kernel ENTRY, ahead of the first
  // codes, so that a row's scale is always an older load than the row's codes
  template <int N, int SH> static __device__ __forceinline__ void load_scales(float (&sc)[N], const float* rows, int r0, int wave) {
#pragma unroll
    for (int j = 0; j < N; ++j) sc[j] = rows[r0 + ((wave + SEG_NW * j) >> SH)];
  }
  static __device__ __forceinline__ void fence() { __builtin_amdgcn_sched_barrier(0); }   // the scheduler must not move a code in front of the scales (it did)
  template <int B>
  static __device__ __forceinline__ void park(const float (&acc)[B][2], float sc, float* part, int u, int lane) { w8_park<B>(acc, sc, part, u, lane); }
};

}  // namespace
