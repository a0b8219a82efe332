// codec.hip — the watermarked-Encodec kernels that are not plain GEMMs (gfx950).
//
// Activations are time-major fp32 ([rows][C], C contiguous): convolutions and transposed convolutions run on
// ssrhip_gemm over strided views (see include/ssrhip.h), so what is left here is
//   * the first SEANet conv (C_in = 1, K = 7: too thin for a GEMM; pure HBM streaming, coalesced over C_out),
//   * reflect padding of a padded buffer's halo rows,
//   * the LSTM recurrence: per time step ONE kernel = recurrent GEMV (the 4 gate rows of a hidden unit per
//     wave, h_{t-1} in registers) fused with the gate non-linearities and the optional skip add; W_hh
//     (16.8 MB at C=1024) is re-read every step from L2/Infinity Cache,
//   * residual vector quantisation: nearest codebook row per frame (block per frame, scores in the
//     reference's arithmetic form, first-max tie rule) and the gather-sum dequantiser,
#include <string.h>
#include <stdlib.h>
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void conv_cin1_kernel(const float* x, const float* w, const float* bias, float* out, int T_out,
                                                        int k, int stride, int Cout, long x_bstride, long out_bstride) {
  // generic fallback (C_out not a multiple of 4 or k > 8): thread -> (t, co) with co fastest
  const long total = (long)T_out * Cout;
  const float* xb = x + (size_t)blockIdx.y * x_bstride;
  float* ob = out + (size_t)blockIdx.y * out_bstride;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int t = (int)(i / Cout), co = (int)(i % Cout);
    float acc = 0.f;
    for (int kk = 0; kk < k; ++kk) acc = fmaf(w[co * k + kk], xb[(size_t)t * stride + kk], acc);
    ob[i] = acc + bias[co];
  }
}

// The same convolution as a store-bound streaming kernel (SEANet's first layer writes B x T x 64 floats: 3.9 GB at 32 clips x
// 30 s; the generic kernel above spent 5.8 ms there in 64-bit index arithmetic and scalar stores). A 256-thread workgroup
// owns TT consecutive output times: the input window goes to LDS once, a thread keeps the K taps of its 4 output channels
// in registers and writes one float4 per time step (C_out/4 threads cover a row: 256 contiguous bytes at C_out = 64).
template <int KT>
__global__ __launch_bounds__(256) void conv_cin1_vec_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ out, int T_out,
                                                            int stride, int Cout, long x_bstride, long out_bstride, int TT) {
  extern __shared__ float xs[];                       // (TT - 1) * stride + KT input samples
  const float* xb = x + (size_t)blockIdx.y * x_bstride;
  float* ob = out + (size_t)blockIdx.y * out_bstride;
  const int t0 = blockIdx.x * TT;
  const int nt = min(TT, T_out - t0);
  const int nin = (nt - 1) * stride + KT;
  for (int i = threadIdx.x; i < nin; i += 256) xs[i] = xb[(size_t)t0 * stride + i];
  const int tpr = Cout >> 2;                           // threads per output row
  const int co = (threadIdx.x % tpr) * 4, tl = threadIdx.x / tpr, tstep = 256 / tpr;
  float wr[4][KT];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) wr[j][kk] = w[(co + j) * KT + kk];
  const float4 b4 = make_float4(bias[co], bias[co + 1], bias[co + 2], bias[co + 3]);
  __syncthreads();
  for (int t = tl; t < nt; t += tstep) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
      const float xv = xs[t * stride + kk];
      a0 = fmaf(wr[0][kk], xv, a0);
      a1 = fmaf(wr[1][kk], xv, a1);
      a2 = fmaf(wr[2][kk], xv, a2);
      a3 = fmaf(wr[3][kk], xv, a3);
    }
    *reinterpret_cast<float4*>(ob + (size_t)(t0 + t) * Cout + co) = make_float4(a0 + b4.x, a1 + b4.y, a2 + b4.z, a3 + b4.w);
  }
}

// Convolution with very few OUTPUT channels (SEANet's last layer: 64 -> 1, k = 7, at the full sample rate) on a time-major input:
// the im2col row of output t is the CONTIGUOUS window x[t*C_in .. (t+k)*C_in) — a dot product of K = k*C_in floats per output.
// A GEMM tile wastes 31/32 of its columns on it (7.4 ms per call at 32 x 30 s); this is the read-bound form: a workgroup stages
// TT + k - 1 input rows in LDS with the ELU applied once per element (rows padded to C_in + 1 floats: lane t reads row t, so
// consecutive lanes hit consecutive banks), a lane owns one output time and walks the window against the weights (uniform
// addresses: scalar loads).
__global__ __launch_bounds__(256) void conv_few_out_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ out, int T_out,
                                                           int k, int Cin, int Cout, int act_in, long x_bstride, long out_bstride, int TT) {
  extern __shared__ __attribute__((aligned(16))) float xs[];   // (TT + k - 1) rows of C_in + 4, then C_out * k * C_in weights
  const float* xb = x + (size_t)blockIdx.y * x_bstride;
  float* ob = out + (size_t)blockIdx.y * out_bstride;
  const int t0 = blockIdx.x * TT;
  const int nt = min(TT, T_out - t0);
  // rows padded to C_in + 4 floats: 16-byte aligned, and the 16 lanes a ds_read_b128 services together (rows t, t+1, ..)
  // start 4 banks apart -> conflict-free float4 reads of a lane's own row
  const int rows = nt + k - 1, ldr = Cin + 4;
  const int c4n = Cin >> 2, K = k * Cin;
  float* ws = xs + (size_t)(TT + k - 1) * ldr;
  for (int i = threadIdx.x; i < Cout * K / 4; i += 256) *reinterpret_cast<float4*>(ws + 4 * i) = ld4(w + 4 * i);
  for (int i = threadIdx.x; i < rows * c4n; i += 256) {
    const int r = i / c4n, c = (i % c4n) * 4;
    float4 v = ld4(xb + ((size_t)(t0 + r)) * Cin + c);
    if (act_in == SSRHIP_ACT_ELU) { v.x = elu1(v.x); v.y = elu1(v.y); v.z = elu1(v.z); v.w = elu1(v.w); }   // the GEMM's operand-load ELU (common.h)
    *reinterpret_cast<float4*>(xs + r * ldr + c) = v;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nt; t += 256) {
    for (int co = 0; co < Cout; ++co) {
      const float* wr = ws + co * K;                  // [k][C_in] (the GEMM layout of the same layer); uniform address: LDS broadcast
      float a0 = 0.f, a1 = 0.f;
      for (int kk = 0; kk < k; ++kk) {
        const float* xr = xs + (t + kk) * ldr;
        const float* wk = wr + kk * Cin;
#pragma unroll 4
        for (int c = 0; c < Cin; c += 8) {
          const float4 x0 = *reinterpret_cast<const float4*>(xr + c), x1 = *reinterpret_cast<const float4*>(xr + c + 4);
          const float4 w0 = *reinterpret_cast<const float4*>(wk + c), w1 = *reinterpret_cast<const float4*>(wk + c + 4);
          a0 = dot4(w0, x0, a0);
          a1 = dot4(w1, x1, a1);
        }
      }
      ob[(size_t)(t0 + t) * Cout + co] = (a0 + a1) + bias[co];
    }
  }
}

// The same layer on the matrix core (round 5; VERDICT r4: "conv_few_out <= 8 ms"): the kernel above spends 224 LDS reads per output (its
// 448-float window and the 448 weights, both through LDS) — 13.3 ms per config-5 decode pass against 6.3 ms of HBM time for the 31.5 GB it
// reads. Here a lane never re-reads an input element: for C_out == 1 the layer is P[r][kk] = x[r][:] . w[kk][:] (a [rows x C_in] x
// [C_in x k] GEMM, k <= 16 columns of a 16 x 16 tile) followed by the diagonal sum out[t] = sum_kk P[t + kk][kk]. A wave takes 16 input
// rows at a time straight from global memory into v_mfma_f32_16x16x4_f32's A operand — lane (c = l & 15, g = l >> 4) loads the four
// float4 x[row c][16 q + 4 g ..] (64 contiguous bytes per row and instruction; ELU on load) — against the weights held as the B operand in
// C_in / 4 registers (column c = tap c, zero beyond k; the k index of MFMA (q, comp) is 16 q + 4 g + comp on both sides), parks the k
// useful columns of the tile in LDS (rows padded to 17 floats: the diagonal reads are conflict-free) and, behind one barrier, thread t adds
// its diagonal in tap order. fp32 MFMA = an fmaf chain (MI355X_MICROARCH.md); the summation ORDER differs from the kernel above (channels
// in MFMA order, then taps), so results agree with it to rounding, not bit for bit.
template <int CQ, bool ELU>
__global__ __launch_bounds__(256) void conv_one_out_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                float* __restrict__ out, int T_out, int k, long x_bstride, long out_bstride) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  constexpr int Cin = 16 * CQ, TT = 256, LDP = 17, MAXT = 5;       // 256 outputs + k - 1 <= 271 rows = 17 tiles of 16 over 4 waves
  __shared__ float P[(TT + 16) * LDP];
  const float* xb = x + (size_t)blockIdx.y * x_bstride;
  float* ob = out + (size_t)blockIdx.y * out_bstride;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), c = lane & 15, g = lane >> 4;
  const int t0 = blockIdx.x * TT, nt = min(TT, T_out - t0);
  const int rows = nt + k - 1, ntiles = (rows + 15) >> 4, last_row = T_out + k - 2;        // the input has T_out + k - 1 rows
  float4 wq[CQ];                                                   // the weights first (L2 hits): the waits in front of the tiles then count down through the x loads
#pragma unroll
  for (int q = 0; q < CQ; ++q) {                                   // unconditional (clamped) loads, zeroed by selects: no branch, no drain
    const float4 v = ld4(w + (size_t)min(c, k - 1) * Cin + 16 * q + 4 * g);
    wq[q] = make_float4(c < k ? v.x : 0.f, c < k ? v.y : 0.f, c < k ? v.z : 0.f, c < k ? v.w : 0.f);
  }
  float4 xa[MAXT][CQ];
#pragma unroll
  for (int i = 0; i < MAXT; ++i) {
    const int tile = wave + 4 * i;
    if (tile < ntiles) {
      const float* xr = xb + (size_t)min(t0 + tile * 16 + c, last_row) * Cin + 4 * g;
#pragma unroll
      for (int q = 0; q < CQ; ++q) xa[i][q] = ld4(xr + 16 * q);
    }
  }
#pragma unroll
  for (int i = 0; i < MAXT; ++i) {
    const int tile = wave + 4 * i;
    if (tile < ntiles) {
      f4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < CQ; ++q) {
        float4 v = xa[i][q];
        if (ELU) { v.x = elu1(v.x); v.y = elu1(v.y); v.z = elu1(v.z); v.w = elu1(v.w); }
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v.x, wq[q].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v.y, wq[q].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v.z, wq[q].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v.w, wq[q].w, acc, 0, 0, 0);
      }
      if (c < k) {                                                 // D[row 4 g + r][tap c]
#pragma unroll
        for (int r = 0; r < 4; ++r) P[(tile * 16 + 4 * g + r) * LDP + c] = acc[r];
      }
    }
  }
  __syncthreads();
  if (t < nt) {
    float s = P[t * LDP];
    for (int kk = 1; kk < k; ++kk) s += P[(t + kk) * LDP + kk];
    ob[(size_t)(t0 + t)] = s + bias[0];
  }
}

// Reflect padding with the reference's small-input rule (audiocraft/modules/conv.py:71-88): an input no longer than the larger
// pad is first zero-extended on the right by `extra = max_pad - T + 1` samples, reflected, and the last `extra` samples of
// the result are dropped again. x' = [x, 0 * extra], T' = T + extra; a halo row takes x'[i] (zero when i >= T).
__global__ __launch_bounds__(256) void pad_reflect_kernel(float* buf, int T, int padL, int padR, int C, long bstride, int extra) {
  float* b = buf + (size_t)blockIdx.y * bstride;
  const long total = (long)(padL + padR) * C;
  const int Tx = T + extra;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int p = (int)(i / C), c = (int)(i % C);
    int dst, src;                                                             // src: index into x'
    if (p < padL) { dst = p; src = padL - p; }                                // edge excluded
    else {
      const int r = p - padL;
      dst = padL + T + r;
      src = (T + r < Tx) ? T + r : Tx - 2 - (T + r - Tx);                     // still inside the zero extension, else mirrored
    }
    b[(size_t)dst * C + c] = (src < T) ? b[(size_t)(padL + src) * C + c] : 0.f;
  }
}

// Halo rows of a RAGGED batch: item b holds lens[b] <= T valid rows; the padR rows right behind ITS last valid row (partly inside
// the interior of the dense buffer, whose producer wrote T rows for every item) and the padL rows in front get the value the
// convolution's padding has for an item of that length alone: zeros, or the reflection about its own ends (conv.py:71-88, incl.
// the zero extension of inputs shorter than the pad). Rows further right stay whatever the producer wrote: no valid output reads them.
__global__ __launch_bounds__(256) void pad_ragged_kernel(float* buf, const int* __restrict__ lens, int T, int padL, int padR, int C,
                                                         long bstride, int reflect) {
  float* b = buf + (size_t)blockIdx.y * bstride;
  const int Ti = min(max(lens[blockIdx.y], 0), T);
  const int max_pad = padL > padR ? padL : padR;
  const int Tx = Ti + ((reflect && Ti <= max_pad) ? max_pad - Ti + 1 : 0);
  const long total = (long)((reflect ? padL : 0) + padR) * C;
  const int nl = reflect ? padL : 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int p = (int)(i / C), c = (int)(i % C);
    int dst, src;
    if (p < nl) { dst = p; src = padL - p; }
    else {
      const int r = p - nl;
      dst = padL + Ti + r;
      src = (Ti + r < Tx) ? Ti + r : Tx - 2 - (Ti + r - Tx);
    }
    b[(size_t)dst * C + c] = (reflect && src >= 0 && src < Ti) ? b[(size_t)(padL + src) * C + c] : 0.f;
  }
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// One LSTM time step for B <= 4 items. Wave -> hidden unit j (4 gate rows j, C+j, 2C+j, 3C+j of W_hh).
// NCH = C / 256 float4 chunks per lane (C a multiple of 256): every load is unconditional, so all 4*NCH weight loads and the
// B*NCH h loads of a wave are in flight together (predicated loads make hipcc drain the queue between groups).
template <int B, int NCH>
__global__ __launch_bounds__(256) void lstm_step_kernel(const ssrhip_lstm_args a, int t, const float* hprev, float* hnext) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = a.C;
  const int j = min(blockIdx.x * 4 + wave, C - 1);          // C % 4 == 0: never clamps; keeps the loads unconditional
  float4 h[B][NCH];
#pragma unroll
  for (int b = 0; b < B; ++b)
#pragma unroll
    for (int i = 0; i < NCH; ++i) h[b][i] = ld4(hprev + (size_t)b * C + (i * 64 + lane) * 4);
  float4 w[4][NCH];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int i = 0; i < NCH; ++i) w[q][i] = ld4(a.w_hh + ((size_t)q * C + j) * C + (i * 64 + lane) * 4);
  float g[4][B];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int b = 0; b < B; ++b) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i) s = dot4(w[q][i], h[b][i], s);
      g[q][b] = wave_sum(s);
    }
  }
  if (lane < B) {
    float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f;
#pragma unroll
    for (int b = 0; b < B; ++b)
      if (lane == b) { gi = g[0][b]; gf = g[1][b]; gg = g[2][b]; go = g[3][b]; }
    const int b = lane;
    const float* gin = a.gin + (size_t)b * a.gin_bstride + (size_t)t * 4 * C;
    gi += gin[j]; gf += gin[C + j]; gg += gin[2 * C + j]; go += gin[3 * C + j];
    float* cc = a.cbuf + (size_t)b * C + j;
    const float cprev = (t == 0) ? 0.f : *cc;
    const float cn = sigmoidf_(gf) * cprev + sigmoidf_(gi) * tanhf(gg);
    const float hn = sigmoidf_(go) * tanhf(cn);
    *cc = cn;
    hnext[(size_t)b * C + j] = hn;
    float o = hn;
    if (a.skip) o += a.skip[(size_t)b * a.skip_bstride + (size_t)t * C + j];
    if (a.out_act == SSRHIP_ACT_ELU) o = elu1(o);
    a.out[(size_t)b * a.out_bstride + (size_t)t * C + j] = o;
  }
}

template <int B>
void launch_lstm_step(const ssrhip_lstm_args& a, int t, const float* hp, float* hn, hipStream_t s) {
  dim3 grid((a.C + 3) / 4);
  switch (a.C / 256) {
    case 1: hipLaunchKernelGGL((lstm_step_kernel<B, 1>), grid, dim3(256), 0, s, a, t, hp, hn); break;
    case 2: hipLaunchKernelGGL((lstm_step_kernel<B, 2>), grid, dim3(256), 0, s, a, t, hp, hn); break;
    case 4: hipLaunchKernelGGL((lstm_step_kernel<B, 4>), grid, dim3(256), 0, s, a, t, hp, hn); break;
    default: hipLaunchKernelGGL((lstm_step_kernel<B, 8>), grid, dim3(256), 0, s, a, t, hp, hn); break;
  }
}

// One LSTM time step for B > 4 items on the matrix core (same tile scheme as gemv_mfma.hip): a workgroup owns 4 hidden units
// j0..j0+3 = 16 rows of W_hh (row 4u+q of the tile is gate q of unit j0+u, i.e. W_hh row q*C + j0+u — only address math, the
// weights stay in torch's [4C][C] layout) and one tile of 16 batch columns (blockIdx.y). v_mfma_f32_16x16x4_f32 leaves lane
// (column n, k-slot u) with rows 4u..4u+3 of column n = the i,f,g,o pre-activations of unit j0+u of item n, so the gate
// math, the cell update and the h/out stores are lane-local: one launch per step, no [B][4C] round trip.
// h_{t-1} is kept in the 16-column tiled layout per batch tile (include/ssrhip.h SSRHIP_TILED): contiguous operand loads.
// W_hh (16.8 MB at C=1024) is re-read every step: workgroup->XCD placement is the same for every launch, so each XCD's
// L2 keeps its 1/8 of W_hh (plain loads, not nt).
typedef float f4v_ __attribute__((ext_vector_type(4)));

// NT = 16-item batch tiles per workgroup (blockIdx.y covers NT consecutive tiles): the wave's W_hh slice (16 k-steps = 256
// columns, 16 float4) is loaded ONCE into registers and multiplied with NT h tiles, so W_hh's L2 traffic per step halves for
// B > 16. Waves: C/256 per workgroup (<= 4: C <= 1024, which leaves 512 VGPRs per wave for the two operand sets).
template <int NT>
__global__ __launch_bounds__(256) void lstm_step_mfma_kernel(const ssrhip_lstm_args a, int t, const float* hprev, float* hnext, int nw, int steps,
                                                              int nbt) {
  constexpr int SPW = 16;
  __shared__ f4v_ tile[NT][4][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, ks = lane >> 4;
  const int C = a.C, j0 = blockIdx.x * 4, bt0 = blockIdx.y * NT;
  const int last = steps - 1;
  // W_hh operand: torch's [4C][C] (lane -> row (gate c&3, unit j0 + c>>2): 64 sixteen-byte pieces of 16 rows per wave-level load) or,
  // a.w_packed, the same 16 x 16 blocks stored in the order the lanes read them (one contiguous KiB per load; codec/wmencodec.py packs it)
  const unsigned wvoff = a.w_packed ? (unsigned)(ks * 16 + c) * 4 : ((unsigned)(c & 3) * C + min(j0 + (c >> 2), C - 1)) * (unsigned)C + ks * 4;
  const float* wbase = a.w_packed ? a.w_hh + (size_t)blockIdx.x * steps * 256 : a.w_hh;
  const int wstep = a.w_packed ? 256 : 16;
  const unsigned xvoff = (unsigned)(ks * 16 + c) * 4;
  const int tbase = wave * SPW;

  // operands are requested in the order the MFMA chain consumes them (k-step by k-step: W_hh block, then that k-step's h blocks of every
  // batch tile): loads return in order, so the chain starts after the first three KiB instead of after all 48 (the h tiles used to be
  // requested first, all W_hh blocks last: the whole 1.7 us matrix-core chain sat behind the complete load phase)
  float4 xr[NT][SPW];
  float4 w[SPW];
#pragma unroll
  for (int i = 0; i < SPW; ++i) {
    w[i] = ld4(wbase + min(tbase + i, last) * wstep + wvoff);
#pragma unroll
    for (int q = 0; q < NT; ++q) xr[q][i] = ld4(hprev + (size_t)min(bt0 + q, nbt - 1) * 16 * C + min(tbase + i, last) * 256 + xvoff);
  }
  // the finishing waves (wave q finishes batch tile q) request their gate inputs and cell state NOW: they do not depend on
  // the recurrent product, so their L2/HBM latency hides under the MFMA chain instead of following it
  float pg[4] = {0.f, 0.f, 0.f, 0.f}, pc = 0.f;
  const bool fin = (nw > 1) && (wave < NT);
  if (fin) {
    const int bt = bt0 + wave, bb = min(bt * 16 + c, a.B - 1), jj = min(j0 + ks, C - 1);
    const float* gin = a.gin + (size_t)bb * a.gin_bstride + (size_t)t * 4 * C;
    pg[0] = gin[jj]; pg[1] = gin[C + jj]; pg[2] = gin[2 * C + jj]; pg[3] = gin[3 * C + jj];
    pc = (t == 0) ? 0.f : a.cbuf[(size_t)bb * C + jj];
  }
#pragma unroll
  for (int q = 0; q < NT; ++q)
#pragma unroll
    for (int i = 0; i < SPW; ++i)
      if (tbase + i > last) xr[q][i] = make_float4(0.f, 0.f, 0.f, 0.f);
  f4v_ acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = f4v_{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < SPW; ++i) {
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i].x, xr[q][i].x, acc[q], 0, 0, 0);
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i].y, xr[q][i].y, acc[q], 0, 0, 0);
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i].z, xr[q][i].z, acc[q], 0, 0, 0);
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i].w, xr[q][i].w, acc[q], 0, 0, 0);
  }
  if (nw > 1) {
#pragma unroll
    for (int q = 0; q < NT; ++q) tile[q][wave][lane] = acc[q];
    __syncthreads();
    if (wave >= NT) return;                       // wave q finishes batch tile q
  }
  const int q = (nw > 1) ? wave : 0;
  f4v_ sum = acc[0];
  if (nw > 1) {
    sum = tile[q][0][lane];
    for (int w2 = 1; w2 < nw; ++w2) sum += tile[q][w2][lane];
  }
#pragma unroll
  for (int qq = 0; qq < NT; ++qq) {               // nw == 1: the single wave walks its NT tiles; nw > 1: only qq == q
    if (nw > 1 && qq != q) continue;
    if (nw == 1) sum = acc[qq];
    const int bt = bt0 + qq;
    const int b = bt * 16 + c, j = j0 + ks;
    if (bt >= nbt || b >= a.B || j >= C) continue;
    float* cc = a.cbuf + (size_t)b * C + j;
    if (!fin) {                                   // single-wave workgroups (narrow C): no early request was made
      const float* gin = a.gin + (size_t)b * a.gin_bstride + (size_t)t * 4 * C;
      pg[0] = gin[j]; pg[1] = gin[C + j]; pg[2] = gin[2 * C + j]; pg[3] = gin[3 * C + j];
      pc = (t == 0) ? 0.f : *cc;
    }
    const float gi = sum[0] + pg[0], gf = sum[1] + pg[1], gg = sum[2] + pg[2], go = sum[3] + pg[3];
    const float cn = sigmoidf_(gf) * pc + sigmoidf_(gi) * tanhf(gg);
    const float hn = sigmoidf_(go) * tanhf(cn);
    *cc = cn;
    hnext[(size_t)bt * 16 * C + SSRHIP_TILED(c, j)] = hn;
    float o = hn;
    if (a.skip) o += a.skip[(size_t)b * a.skip_bstride + (size_t)t * C + j];
    if (a.out_act == SSRHIP_ACT_ELU) o = elu1(o);
    a.out[(size_t)b * a.out_bstride + (size_t)t * C + j] = o;
  }
}

// The same step for LARGE batches (>= 8 batch tiles, i.e. more than 112 items). With 4 hidden units per workgroup every one of the
// C/4 = 256 workgroup columns re-reads the whole h_{t-1} (1 MB at 256 items) and every pair of batch tiles re-reads all of W_hh:
// 393 MB of L2 traffic per step at 256 items, 64 us per step against a matrix-core floor of 13.7 us (rocprofv3, 256 clips x 30 s).
// Here a workgroup owns RT = 4 row tiles (16 hidden units: 64 gate rows) — its W_hh slice, 256 KB, lives in the registers of its 4
// waves (each wave a quarter of K) for the whole launch — and walks NQ batch tiles one after the other: h traffic drops 4x (64
// workgroup columns), W traffic 2x (nbt/NQ batch groups), and the matrix core sees 256 back-to-back MFMAs per batch tile per wave.
// The K-slices of a batch tile are added through LDS (double-buffered: one barrier per batch tile); wave r then finishes row tile
// r of that batch tile (gates, cell update, h / out stores) while the others already multiply the next one. Needs the packed
// W_hh (w_packed) and C % 16 == 0.
template <int RT>
__global__ __launch_bounds__(256) void lstm_step_wide_kernel(const ssrhip_lstm_args a, int t, const float* hprev, float* hnext, int nw, int steps,
                                                              int nbt, int NQ) {
  constexpr int SPW = 16;
  __shared__ f4v_ tile[2][RT][4][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, ks = lane >> 4;
  const int C = a.C, j0 = blockIdx.x * 4 * RT, bt0 = blockIdx.y * NQ;
  const int last = steps - 1;
  const int tbase = wave * SPW;
  const unsigned lvoff = (unsigned)(ks * 16 + c) * 4;          // this lane's float4 inside a 1-KiB block (weights and h alike)

  const int nq = min(NQ, nbt - bt0);
  float4 w[RT][SPW];
  float4 xr[SPW];
  auto load_x = [&](int q) {
    const float* xbase = hprev + (size_t)min(bt0 + q, nbt - 1) * 16 * C;
#pragma unroll
    for (int i = 0; i < SPW; ++i) xr[i] = ld4(xbase + min(tbase + i, last) * 256 + lvoff);
  };
  // the first batch tile's h slice, then W in the order the MFMA loop consumes it (k-step major): loads return in order, so the
  // chain starts after the first RT weight loads and the rest of the 256 KB slice streams in underneath it
  load_x(0);
  const float* wb[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) wb[r] = a.w_hh + (size_t)min(blockIdx.x * RT + r, C / 4 - 1) * steps * 256 + lvoff;
#pragma unroll
  for (int i = 0; i < SPW; ++i)
#pragma unroll
    for (int r = 0; r < RT; ++r) w[r][i] = ld4(wb[r] + min(tbase + i, last) * 256);
  for (int q = 0; q < nq; ++q) {
    // what the finishing wave (wave r finishes row tile r) needs for this batch tile: requested before the MFMA chain
    float pg[4] = {0.f, 0.f, 0.f, 0.f}, pc = 0.f;
    const bool fin = wave < RT;
    const int bt = bt0 + q;
    const int bb = min(bt * 16 + c, a.B - 1), jj = min(j0 + 4 * wave + ks, C - 1);
    if (fin) {
      const float* gin = a.gin + (size_t)bb * a.gin_bstride + (size_t)t * 4 * C;
      pg[0] = gin[jj]; pg[1] = gin[C + jj]; pg[2] = gin[2 * C + jj]; pg[3] = gin[3 * C + jj];
      pc = (t == 0) ? 0.f : a.cbuf[(size_t)bb * C + jj];
    }
    f4v_ acc[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = f4v_{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < SPW; ++i) {
      float4 xv = xr[i];
      if (tbase + i > last) xv = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[r][i].x, xv.x, acc[r], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[r][i].y, xv.y, acc[r], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[r][i].z, xv.z, acc[r], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[r][i].w, xv.w, acc[r], 0, 0, 0);
    }
    if (q + 1 < nq) load_x(q + 1);                            // next batch tile's h slice: in flight during the merge / gate phase
#pragma unroll
    for (int r = 0; r < RT; ++r) tile[q & 1][r][wave][lane] = acc[r];
    __syncthreads();
    if (fin) {
      f4v_ sum = tile[q & 1][wave][0][lane];
      for (int w2 = 1; w2 < nw; ++w2) sum += tile[q & 1][wave][w2][lane];
      const int b = bt * 16 + c, j = j0 + 4 * wave + ks;
      if (b < a.B && j < C) {
        const float gi = sum[0] + pg[0], gf = sum[1] + pg[1], gg = sum[2] + pg[2], go = sum[3] + pg[3];
        const float cn = sigmoidf_(gf) * pc + sigmoidf_(gi) * tanhf(gg);
        const float hn = sigmoidf_(go) * tanhf(cn);
        a.cbuf[(size_t)b * C + j] = cn;
        hnext[(size_t)bt * 16 * C + SSRHIP_TILED(c, j)] = hn;
        float o = hn;
        if (a.skip) o += a.skip[(size_t)b * a.skip_bstride + (size_t)t * C + j];
        if (a.out_act == SSRHIP_ACT_ELU) o = elu1(o);
        a.out[(size_t)b * a.out_bstride + (size_t)t * C + j] = o;
      }
    }
  }
}

__global__ __launch_bounds__(256) void zero_kernel(float* p, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] = 0.f;
}

// RVQ encode: one workgroup per frame. score_j = -(|x|^2 - (2x).e_j + |e_j|^2) exactly as
// EuclideanCodebook.quantize writes it (core_vq.py:164-172); argmax with the first-index tie rule of torch.max.
__global__ __launch_bounds__(256) void rvq_encode_kernel(const float* emb, const float* cb, const float* e2, int* codes, int T, int D,
                                                         int n_q, int bins, long emb_bstride) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* x = sm;                 // [D]
  float* red = sm + D;           // [8]
  int* redi = reinterpret_cast<int*>(red + 8);
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* src = emb + (size_t)b * emb_bstride + (size_t)t * D;
  for (int d = tid; d < D; d += 256) x[d] = src[d];
  __syncthreads();
  for (int q = 0; q < n_q; ++q) {
    float p = 0.f;
    for (int d = tid; d < D; d += 256) p += x[d] * x[d];
    p = wave_sum(p);
    if (lane == 0) red[wave] = p;
    __syncthreads();
    const float x2 = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    const float* E = cb + (size_t)q * bins * D;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int j = tid; j < bins; j += 256) {
      const float* e = E + (size_t)j * D;
      float dot = 0.f;
      for (int d = 0; d < D; d += 4) {
        const float4 ev = ld4(e + d);
        const float4 xv = *reinterpret_cast<const float4*>(x + d);
        dot = fmaf(2.0f * xv.x, ev.x, dot);
        dot = fmaf(2.0f * xv.y, ev.y, dot);
        dot = fmaf(2.0f * xv.z, ev.z, dot);
        dot = fmaf(2.0f * xv.w, ev.w, dot);
      }
      const float sc = -((x2 - dot) + e2[(size_t)q * bins + j]);
      if (sc > best) { best = sc; bi = j; }       // j ascending per thread: first max kept
    }
    const float wb = wave_max(best);
    int wi = (best == wb) ? bi : 0x7fffffff;
    wi = wave_min_i(wi);
    if (lane == 0) { red[wave] = wb; redi[wave] = wi; }
    __syncthreads();
    float bb = red[0];
    int ii = redi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (red[w] > bb || (red[w] == bb && redi[w] < ii)) { bb = red[w]; ii = redi[w]; }
    if (tid == 0) codes[((size_t)b * n_q + q) * T + t] = ii;
    const float* e = E + (size_t)ii * D;
    __syncthreads();
    for (int d = tid; d < D; d += 256) x[d] -= e[d];      // residual = residual - quantized (core_vq.py:389-390)
    __syncthreads();
  }
}

// RVQ encode on the matrix core: a workgroup owns 16 consecutive frames of one item; per stage the score matrix
// [bins x 16 frames] = -(|x|^2 - (2x).e + |e|^2) is built 16 codes x 16 frames at a time with v_mfma_f32_16x16x4_f32
// (A = codebook rows straight from L2, B = the doubled residual, register-resident in operand layout); the 4 waves take
// every 4th code tile, keep a running first-max per (lane = frame, 4 codes) and merge through LDS. The codebook is read
// once per 16 frames instead of once per frame (the per-frame kernel above is L2-bound: 4 MB of codebook per frame).
template <int NS>   // D / 16 k-steps
__global__ __launch_bounds__(256) void rvq_encode_mfma_kernel(const float* emb, const float* cb, const float* e2, int* codes, int T, int n_q,
                                                              int bins, long emb_bstride) {
  constexpr int D = NS * 16;
  __shared__ float redv[4][16];
  __shared__ int redi[4][16];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, ks = lane >> 4;
  const int t0 = blockIdx.x * 16, b = blockIdx.y;
  const float* src = emb + (size_t)b * emb_bstride + (size_t)min(t0 + c, T - 1) * D + ks * 4;
  float4 xr[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) xr[s] = ld4(src + s * 16);
  const int ntile = bins / 16;
  for (int q = 0; q < n_q; ++q) {
    float p = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) p += (xr[s].x * xr[s].x + xr[s].y * xr[s].y) + (xr[s].z * xr[s].z + xr[s].w * xr[s].w);
    p += xor16_f(p);
    p += xor32_f(p);
    const float x2 = p;                                   // |x|^2 of frame c
    const float* E = cb + (size_t)q * bins * D;
    const float* e2q = e2 + (size_t)q * bins;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    float4 ec[NS], en[NS];
    {
      const float* er = E + (size_t)(wave * 16 + c) * D + ks * 4;
#pragma unroll
      for (int s = 0; s < NS; ++s) ec[s] = ld4(er + s * 16);
    }
    for (int ct = wave; ct < ntile; ct += 4) {
      {
        const float* er = E + (size_t)(min(ct + 4, ntile - 1) * 16 + c) * D + ks * 4;      // clamped, never predicated
#pragma unroll
        for (int s = 0; s < NS; ++s) en[s] = ld4(er + s * 16);
      }
      const float4 ee = ld4(e2q + ct * 16 + ks * 4);
      f4v_ acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ec[s].x, 2.0f * xr[s].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ec[s].y, 2.0f * xr[s].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ec[s].z, 2.0f * xr[s].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ec[s].w, 2.0f * xr[s].w, acc, 0, 0, 0);
      }
      const int j0 = ct * 16 + ks * 4;                    // this lane: codes j0..j0+3 of frame c, ascending
      const float s0 = -((x2 - acc[0]) + ee.x), s1 = -((x2 - acc[1]) + ee.y), s2 = -((x2 - acc[2]) + ee.z), s3 = -((x2 - acc[3]) + ee.w);
      if (s0 > best) { best = s0; bi = j0; }
      if (s1 > best) { best = s1; bi = j0 + 1; }
      if (s2 > best) { best = s2; bi = j0 + 2; }
      if (s3 > best) { best = s3; bi = j0 + 3; }
#pragma unroll
      for (int s = 0; s < NS; ++s) ec[s] = en[s];
    }
    // merge the 4 k-slot lanes of a frame, then the 4 waves: larger score wins, ties -> smaller index (torch.max: first)
    {
      float ov = xor16_f(best);
      int oi = __builtin_bit_cast(int, xor16_f(__builtin_bit_cast(float, bi)));
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
      ov = xor32_f(best);
      oi = __builtin_bit_cast(int, xor32_f(__builtin_bit_cast(float, bi)));
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (ks == 0) { redv[wave][c] = best; redi[wave][c] = bi; }
    __syncthreads();
    float bb = redv[0][c];
    int ii = redi[0][c];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float v = redv[w][c];
      const int i2 = redi[w][c];
      if (v > bb || (v == bb && i2 < ii)) { bb = v; ii = i2; }
    }
    __syncthreads();
    if (wave == 0 && ks == 0 && t0 + c < T) codes[((size_t)b * n_q + q) * T + t0 + c] = ii;
    const float* eb = E + (size_t)ii * D + ks * 4;        // residual = residual - quantized (core_vq.py:389-390)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float4 ev = ld4(eb + s * 16);
      xr[s].x -= ev.x; xr[s].y -= ev.y; xr[s].z -= ev.z; xr[s].w -= ev.w;
    }
  }
}

__global__ __launch_bounds__(128) void rvq_decode_kernel(const int* codes, const float* cb, float* out, int T, int D, int n_q, int bins,
                                                         long out_bstride) {
  const int t = blockIdx.x, b = blockIdx.y;
  for (int d = threadIdx.x; d < D; d += 128) {
    float acc = 0.0f;                              // quantized_out = 0.0 + q0 + q1 + ... (core_vq.py:395-399)
    for (int q = 0; q < n_q; ++q) {
      const int c = codes[((size_t)b * n_q + q) * T + t];
      acc += cb[((size_t)q * bins + c) * D + d];
    }
    out[(size_t)b * out_bstride + (size_t)t * D + d] = acc;
  }
}


inline int nblocks(long total, int cap = 4096) {
  long n = (total + 255) / 256;
  return (int)(n < 1 ? 1 : (n > cap ? cap : n));
}

// ssrhip_lstm_layer's matrix-core step (16-item batch tiles; any C % 16 == 0, any B), planned once per call. Wide: 16 hidden units per
// workgroup, W_hh slice in registers, `wide_nq` batch tiles walked in sequence (from 8 tiles on: at 4 it measured slower);
// otherwise two / one batch tile per workgroup.
enum lstm_mfma_form { LSTM_WIDE, LSTM_MFMA2, LSTM_MFMA1 };
struct lstm_mfma_plan { lstm_mfma_form form; dim3 grid, block; int wide_nq; };
lstm_mfma_plan plan_lstm_mfma(const ssrhip_lstm_args* a, int nbt, int nw, const codec_knobs& k) {
  if (a->w_packed && nbt >= 8 && a->C % 16 == 0 && a->C >= 64 && !k.lstm_nowide) return {LSTM_WIDE, dim3(a->C / 16, (nbt + 3) / 4), dim3(256), 4};
  if (nbt >= 2 && nw >= 2) return {LSTM_MFMA2, dim3((a->C + 3) / 4, (nbt + 1) / 2), dim3(nw * 64), 0};
  return {LSTM_MFMA1, dim3((a->C + 3) / 4, nbt), dim3(nw * 64), 0};
}

}  // namespace

extern "C" int ssrhip_conv_cin1(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t T_out, int32_t k,
                                int32_t stride, int32_t Cout, int64_t x_bstride, int64_t out_bstride, ssrhip_stream_t stream) {
  SSR_REQUIRE(x && w && bias && out && B > 0 && T_out > 0 && k > 0 && stride > 0 && Cout > 0, "ssrhip_conv_cin1: bad argument");
  SSR_REQUIRE(B <= 65535, "ssrhip_conv_cin1: batch too large");
  hipStream_t s = (hipStream_t)stream;
  if (Cout % 4 == 0 && Cout <= 1024 && (256 % (Cout / 4)) == 0 && (k == 7 || k == 3 || k == 5) && stride <= 4) {
    const int TT = 512;
    dim3 grid((T_out + TT - 1) / TT, B);
    const size_t smem = ((size_t)(TT - 1) * stride + k) * sizeof(float);
    if (k == 7) hipLaunchKernelGGL(conv_cin1_vec_kernel<7>, grid, dim3(256), smem, s, x, w, bias, out, T_out, stride, Cout, (long)x_bstride, (long)out_bstride, TT);
    else if (k == 5) hipLaunchKernelGGL(conv_cin1_vec_kernel<5>, grid, dim3(256), smem, s, x, w, bias, out, T_out, stride, Cout, (long)x_bstride, (long)out_bstride, TT);
    else hipLaunchKernelGGL(conv_cin1_vec_kernel<3>, grid, dim3(256), smem, s, x, w, bias, out, T_out, stride, Cout, (long)x_bstride, (long)out_bstride, TT);
  } else {
    dim3 grid(nblocks((long)T_out * Cout, 16384), B);
    hipLaunchKernelGGL(conv_cin1_kernel, grid, dim3(256), 0, s, x, w, bias, out, T_out, k, stride, Cout, (long)x_bstride, (long)out_bstride);
  }
  SSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssrhip_conv_few_out(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t T_out, int32_t k,
                                   int32_t Cin, int32_t Cout, int32_t act_in, int64_t x_bstride, int64_t out_bstride, ssrhip_stream_t stream) {
  SSR_REQUIRE(x && w && bias && out && B > 0 && T_out > 0 && k > 0 && Cin > 0 && Cout > 0, "ssrhip_conv_few_out: bad argument");
  SSR_REQUIRE(Cin % 8 == 0 && Cout <= 4 && B <= 65535, "ssrhip_conv_few_out: needs C_in %% 8 == 0 and C_out <= 4");
  SSR_REQUIRE(act_in == SSRHIP_ACT_NONE || act_in == SSRHIP_ACT_ELU, "ssrhip_conv_few_out: act_in must be NONE or ELU");
  // one output channel, 64 input channels, at most 16 taps (SEANet's last layer): the matrix-core form (SSRHIP_CONV_FEW_MFMA=0: the LDS form)
  if (ssr_codec_knobs().conv_few_mfma && Cout == 1 && Cin == 64 && k <= 16) {
    dim3 grid((T_out + 255) / 256, B);
    if (act_in == SSRHIP_ACT_ELU) hipLaunchKernelGGL((conv_one_out_mfma_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)stream, x, w, bias, out, T_out, k, (long)x_bstride, (long)out_bstride);
    else hipLaunchKernelGGL((conv_one_out_mfma_kernel<4, false>), grid, dim3(256), 0, (hipStream_t)stream, x, w, bias, out, T_out, k, (long)x_bstride, (long)out_bstride);
    SSR_LAUNCH_CHECK();
    return 0;
  }
  const size_t wbytes = (size_t)Cout * k * Cin * sizeof(float);
  int TT = 256;
  while (TT > 32 && (size_t)(TT + k - 1) * (Cin + 4) * sizeof(float) + wbytes > 78 * 1024) TT >>= 1;     // two workgroups per CU
  const size_t smem = (size_t)(TT + k - 1) * (Cin + 4) * sizeof(float) + wbytes;
  SSR_REQUIRE(smem <= 160 * 1024, "ssrhip_conv_few_out: C_in * k too large");
  // up to 160 KB of dynamic LDS (71 KB at the product's own shape): above the 64 KB a kernel gets unasked
  SSR_RAISE_LDS(160 * 1024, conv_few_out_kernel);
  dim3 grid((T_out + TT - 1) / TT, B);
  hipLaunchKernelGGL(conv_few_out_kernel, grid, dim3(256), smem, (hipStream_t)stream, x, w, bias, out, T_out, k, Cin, Cout, act_in,
                     (long)x_bstride, (long)out_bstride, TT);
  SSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssrhip_pad_reflect(float* buf, int32_t B, int32_t T, int32_t padL, int32_t padR, int32_t C, int64_t bstride, ssrhip_stream_t stream) {
  SSR_REQUIRE(buf && B > 0 && T > 0 && C > 0 && padL >= 0 && padR >= 0, "ssrhip_pad_reflect: bad argument");
  if (padL + padR == 0) return 0;
  const int max_pad = padL > padR ? padL : padR;
  const int extra = T <= max_pad ? max_pad - T + 1 : 0;                       // conv.py:79-83
  dim3 grid(nblocks((long)(padL + padR) * C), B);
  hipLaunchKernelGGL(pad_reflect_kernel, grid, dim3(256), 0, (hipStream_t)stream, buf, T, padL, padR, C, (long)bstride, extra);
  SSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssrhip_pad_ragged(float* buf, const int32_t* lens, int32_t B, int32_t T, int32_t padL, int32_t padR, int32_t C, int64_t bstride,
                                 int32_t reflect, ssrhip_stream_t stream) {
  SSR_REQUIRE(buf && lens && B > 0 && T > 0 && C > 0 && padL >= 0 && padR >= 0, "ssrhip_pad_ragged: bad argument");
  SSR_REQUIRE(B <= 65535, "ssrhip_pad_ragged: batch too large (%d)", B);
  const long n = (long)((reflect ? padL : 0) + padR) * C;
  if (n == 0) return 0;
  dim3 grid(nblocks(n), B);
  hipLaunchKernelGGL(pad_ragged_kernel, grid, dim3(256), 0, (hipStream_t)stream, buf, lens, T, padL, padR, C, (long)bstride, reflect);
  SSR_LAUNCH_CHECK();
  return 0;
}

bool ssrhip_lstm_split_eligible(const ssrhip_lstm_args* a);                             // lstm_split.hip
int ssrhip_lstm_split_steps(const ssrhip_lstm_args* a, int t_lo, int t_hi, hipStream_t s);

extern "C" int ssrhip_lstm_layer(const ssrhip_lstm_args* a, ssrhip_stream_t stream) {
  SSR_REQUIRE(a && a->gin && a->w_hh && a->out && a->hbuf && a->cbuf, "ssrhip_lstm_layer: null argument");
  SSR_REQUIRE(a->B > 0 && a->T > 0 && a->C > 0 && a->C % 16 == 0 && a->C <= 4096, "ssrhip_lstm_layer: need C %% 16 == 0, C <= 4096");
  hipStream_t s = (hipStream_t)stream;
  const int nbt = (a->B + 15) / 16;                                          // 16-item batch tiles (matrix-core path)
  const bool small_b = a->B <= 4 && (a->C == 256 || a->C == 512 || a->C == 1024 || a->C == 2048);
  const size_t hc = small_b ? (size_t)a->B * a->C : (size_t)nbt * 16 * a->C;
  const int t_lo = a->t_begin, t_hi = a->t_end > 0 ? a->t_end : a->T;
  SSR_REQUIRE(t_lo >= 0 && t_lo < t_hi && t_hi <= a->T, "ssrhip_lstm_layer: bad time window [%d, %d) of %d", t_lo, t_hi, a->T);
  SSR_REQUIRE(!a->w_split == !a->hsplit, "ssrhip_lstm_layer: w_split and hsplit go together");
  if (!small_b && ssrhip_lstm_split_eligible(a)) return ssrhip_lstm_split_steps(a, t_lo, t_hi, s);   // bf16 matrix cores, split operands
  if (t_lo == 0) hipLaunchKernelGGL(zero_kernel, dim3(nblocks(2 * hc)), dim3(256), 0, s, a->hbuf, (long)(2 * hc));   // h_0 = 0
  // small-batch kernel: C in {256, 512, 1024, 2048}; anything else (e.g. the narrow test configs) takes the matrix-core path
  if (small_b) {
    SSR_REQUIRE(!a->w_packed, "ssrhip_lstm_layer: the small-batch path reads W_hh in torch's [4C][C] layout");
    for (int t = t_lo; t < t_hi; ++t) {
      const float* hp = a->hbuf + (size_t)(t & 1) * hc;
      float* hn = a->hbuf + (size_t)((t + 1) & 1) * hc;
      switch (a->B) {
        case 1: launch_lstm_step<1>(*a, t, hp, hn, s); break;
        case 2: launch_lstm_step<2>(*a, t, hp, hn, s); break;
        case 3: launch_lstm_step<3>(*a, t, hp, hn, s); break;
        default: launch_lstm_step<4>(*a, t, hp, hn, s); break;
      }
    }
  } else {
    // hbuf holds [2][ceil(B/16)][C/4][16][4] (tiled per 16-item batch tile) on this path
    const int steps = a->C / 16;
    SSR_REQUIRE(!a->w_packed || a->C % 16 == 0, "ssrhip_lstm_layer: packed W_hh needs C %% 16 == 0");
    SSR_REQUIRE(a->C <= 1024, "ssrhip_lstm_layer: the matrix-core path (B > 4, or C not in {256,512,1024,2048}) needs C <= 1024");
    const int nw = (steps + 15) / 16;                        // 256 columns of W_hh per wave -> <= 4 waves
    const lstm_mfma_plan p = plan_lstm_mfma(a, nbt, nw, ssr_codec_knobs());   // outside the loop, which issues thousands of launches per pass
    for (int t = t_lo; t < t_hi; ++t) {
      const float* hp = a->hbuf + (size_t)(t & 1) * hc;
      float* hn = a->hbuf + (size_t)((t + 1) & 1) * hc;
      switch (p.form) {
        case LSTM_WIDE: hipLaunchKernelGGL((lstm_step_wide_kernel<4>), p.grid, p.block, 0, s, *a, t, hp, hn, nw, steps, nbt, p.wide_nq); break;
        case LSTM_MFMA2: hipLaunchKernelGGL((lstm_step_mfma_kernel<2>), p.grid, p.block, 0, s, *a, t, hp, hn, nw, steps, nbt); break;
        case LSTM_MFMA1: hipLaunchKernelGGL((lstm_step_mfma_kernel<1>), p.grid, p.block, 0, s, *a, t, hp, hn, nw, steps, nbt); break;
      }
    }
  }
  SSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssrhip_rvq_encode(const float* emb, const float* codebooks, const float* e2, int32_t* codes, int32_t B, int32_t T,
                                 int32_t D, int32_t n_q, int32_t bins, int64_t emb_bstride, ssrhip_stream_t stream) {
  SSR_REQUIRE(emb && codebooks && e2 && codes && B > 0 && T > 0 && D > 0 && D % 4 == 0 && n_q > 0 && bins > 0, "ssrhip_rvq_encode: bad argument");
  SSR_REQUIRE(B <= 65535, "ssrhip_rvq_encode: B too large");
  const bool mfma = bins % 16 == 0 && bins >= 64 && (D == 32 || D == 64 || D == 128 || D == 256) && !getenv_set("SSRHIP_RVQ_SCALAR");   // read at every call
  if (mfma) {
    dim3 grid((T + 15) / 16, B);
    hipStream_t s = (hipStream_t)stream;
    switch (D) {
      case 32: hipLaunchKernelGGL(rvq_encode_mfma_kernel<2>, grid, dim3(256), 0, s, emb, codebooks, e2, codes, T, n_q, bins, (long)emb_bstride); break;
      case 64: hipLaunchKernelGGL(rvq_encode_mfma_kernel<4>, grid, dim3(256), 0, s, emb, codebooks, e2, codes, T, n_q, bins, (long)emb_bstride); break;
      case 128: hipLaunchKernelGGL(rvq_encode_mfma_kernel<8>, grid, dim3(256), 0, s, emb, codebooks, e2, codes, T, n_q, bins, (long)emb_bstride); break;
      default: hipLaunchKernelGGL(rvq_encode_mfma_kernel<16>, grid, dim3(256), 0, s, emb, codebooks, e2, codes, T, n_q, bins, (long)emb_bstride); break;
    }
    SSR_LAUNCH_CHECK();
    return 0;
  }
  const size_t smem = ((size_t)D + 16) * sizeof(float);
  hipLaunchKernelGGL(rvq_encode_kernel, dim3(T, B), dim3(256), smem, (hipStream_t)stream, emb, codebooks, e2, codes, T, D, n_q, bins, (long)emb_bstride);
  SSR_LAUNCH_CHECK();
  return 0;
}

extern "C" int ssrhip_rvq_decode(const int32_t* codes, const float* codebooks, float* out, int32_t B, int32_t T, int32_t D, int32_t n_q,
                                 int32_t bins, int64_t out_bstride, ssrhip_stream_t stream) {
  SSR_REQUIRE(codes && codebooks && out && B > 0 && T > 0 && D > 0 && n_q > 0 && bins > 0 && B <= 65535, "ssrhip_rvq_decode: bad argument");
  hipLaunchKernelGGL(rvq_decode_kernel, dim3(T, B), dim3(128), 0, (hipStream_t)stream, codes, codebooks, out, T, D, n_q, bins, (long)out_bstride);
  SSR_LAUNCH_CHECK();
  return 0;
}

