/* ssrhip.h — C-ABI of libssrhip.so: the MI355X (gfx950) kernels and decode engine behind the
 * `ssr_speech_amd` Python classes that mirror SSR-Speech's inference surface.
 *
 * The reference (WangHelin1997/SSR-Speech) has NO native/FFI layer on this path — it is plain
 * PyTorch modules — so every entry point below names the reference *Python*
 * function(s) whose arithmetic it replaces (paths relative to the reference root).  A maintainer's
 * binding is a ctypes stub.
 *
 * Conventions
 *   - plain C types only; all `*_dev` / `float*` / `int*` arguments are DEVICE pointers into buffers
 *     the caller owns (torch-allocated); the library never allocates or frees device memory.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); no internal device sync.
 *   - return 0 on success, negative on error; `ssrhip_last_error()` returns a thread-local message.
 *   - fp32 everywhere (the reference's CPU path is fp32); integer tokens are int32 on the device.
 *   - "rows": B = utterances x (2 if classifier-free guidance else 1); row 2u is the conditional row
 *     of utterance u and row 2u+1 its unconditional row (models/ssr.py:571-577, 690-696).
 */
#ifndef SSRHIP_H
#define SSRHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSRHIP_VERSION 107
#define SSRHIP_PAGE 128          /* KV-cache page = 128 positions */
#define SSRHIP_MAX_CODEBOOKS 4
#define SSRHIP_MAX_SILENCE 8

typedef void* ssrhip_stream_t;

int ssrhip_version(void);
/* sizeof() of the ABI structs, for binding self-checks: 0 kv, 1 gemv_args, 2 attn_args, 3 embed_args,
 * 4 sampler_cfg, 5 sampler_state, 6 sample_args, 7 gemm_args, 8 lm_weights, 9 lm_dims, 10 lm_buffers, 11 prefill_args,
 * 12 lstm_args, 13 resblock_args, 14 score_args, 15 lm_w16 */
int ssrhip_sizeof(int which);
const char* ssrhip_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Paged KV cache (replaces the dense, re-concatenated `past` tensor: models/ssr.py:685-686,
 * models/modules/activation.py:626-631).
 *   pool  [n_pages][n_layer][2][n_head][SSRHIP_PAGE][head_dim] fp32 (the *16 / *_kv16 entry points: the same layout in 2-byte bf16 entries)
 *   table [n_seq][max_pages] int32 : logical page -> physical page of that sequence (row)
 * ---------------------------------------------------------------------------------------------- */
typedef struct ssrhip_kv {
  float* pool;
  const int32_t* table;
  int32_t max_pages;   /* table row stride */
  int32_t n_layer, n_head, head_dim;
} ssrhip_kv;

/* ------------------------------------------------------------------------------------------------
 * Fused weight-streaming GEMV for B<=4 rows:  y[b][n] = epi( sum_k pro(x)[b][k] * W[n][k] + bias[n] )
 * replaces F.linear at: activation.py:86 (packed in-proj), :637 (out-proj), transformer.py:386-388
 * (linear1/ReLU/linear2), models/ssr.py:175-179 (prediction heads), fused with
 * transformer.py:58-75 (LayerNorm, eps 1e-5) as prologue and the residual add (transformer.py:328-329).
 * ---------------------------------------------------------------------------------------------- */
enum { SSRHIP_PRO_NONE = 0, SSRHIP_PRO_LAYERNORM = 1, SSRHIP_PRO_ATTN_COMBINE = 2 };
enum { SSRHIP_ACT_NONE = 0, SSRHIP_ACT_RELU = 1, SSRHIP_ACT_GELU_ERF = 2, SSRHIP_ACT_ELU = 3 };
/* SSRHIP_EPI_QKV_APPEND16 (5..32 rows only; <= 4 rows answer a contract error): QKV_APPEND into a cache of 2-byte entries — kv.pool
 * points at bf16 storage of the same layout and element offsets, a K / V value is stored as the upper half of its fp32 bits rounded to
 * nearest even (torch's .to(bfloat16): overflow to inf, NaN stays NaN); q goes to y as fp32, unchanged. */
enum { SSRHIP_EPI_STORE = 0, SSRHIP_EPI_RESIDUAL = 1, SSRHIP_EPI_QKV_APPEND = 2, SSRHIP_EPI_QKV_APPEND16 = 3 };

typedef struct ssrhip_gemv_args {
  const float* W;        /* [groups][N][K] row-major (PyTorch Linear.weight layout) */
  const float* bias;     /* [groups][N] or NULL */
  const float* x;        /* PRO_NONE/LAYERNORM: [B][x_stride] (+ g*K);  ATTN_COMBINE: unused */
  float* y;              /* STORE: [B][y_stride] (+ g*N); RESIDUAL: y += ...; QKV_APPEND: q out [B][K] */
  int32_t B, N, K, groups;
  int32_t x_stride, y_stride;
  int32_t pro, act, epi;
  const float* ln_w; const float* ln_b; float ln_eps;           /* PRO_LAYERNORM */
  /* PRO_ATTN_COMBINE: split-KV partials written by ssrhip_attn_decode */
  const float* part_o; const float* part_ml; int32_t max_splits; /* [R][H][max_splits][hd], [R][H][max_splits][2] */
  const int32_t* row_len;                                        /* [B] keys visible to each row */
  /* EPI_QKV_APPEND: N == 3K; q -> y, k/v -> cache at position kv_pos[b] of sequence b */
  ssrhip_kv kv; int32_t layer; const int32_t* kv_pos;
  /* 5..32 rows only (matrix-core path): activations in the 16-column tiled layout SSRHIP_TILED_P(b,k,K) below instead of
   * row-major [B][stride] (K = the operand's full width: groups*K for x, groups*N for y); x_stride / y_stride are ignored for a
   * tiled operand. QKV_APPEND's q output is always row-major. */
  int32_t x_tiled, y_tiled;
  /* 5..32 rows only: W is stored in the matrix core's streaming order instead of [N][K] (see SSRHIP_WTILED_INDEX): one
   * wave-level load then reads 8 full 128-byte lines instead of 64 sixteen-byte pieces of 16 different rows. */
  int32_t w_tiled;
} ssrhip_gemv_args;

/* Streaming-order weight layout for the 5..32-row GEMV (`w_tiled`): rows are grouped in 8-row units (the last unit zero-padded),
 * K in 16-float steps; the 512-byte block of (unit u, k-step t) holds, at float4 index ks*8 + c, the four weights
 * W[8u + c][16t + 4ks .. 16t + 4ks + 3]   (c = 0..7 row inside the unit, ks = 0..3 k-slot of the 16x16x4 MFMA).
 * Blocks of one unit are contiguous along t, units follow each other: float index of W[n][k] is
 *   ((n/8) * (K/16) + k/16) * 128 + (((k%16)/4) * 8 + n%8) * 4 + k%4 ;  a group's matrix takes ceil(N/8)*8*K floats. */
#define SSRHIP_WTILED_INDEX(n, k, K) ((((size_t)(n) / 8) * ((size_t)(K) / 16) + (size_t)(k) / 16) * 128 + ((((k) % 16) / 4) * 8 + (n) % 8) * 4 + (k) % 4)

/* 16-column tiled activation layout used between the kernels of the 5..32-row decode step: element (row b, feature k) of a
 * [<=16][K] activation lives at float index ((k/4)*16 + b)*4 + k%4, i.e. 4 consecutive features of the 16 rows are 256
 * contiguous bytes — exactly what one 64-lane MFMA B-operand load wants (a whole KiB per wave instruction). */
#define SSRHIP_TILED(b, k) ((((size_t)(k) >> 2) * 16 + (size_t)(b)) * 4 + ((k) & 3))
/* Paneled form for up to 32 rows: row b of a [B][K] tiled activation lives in panel b/16, panel p starts at float offset p*16*K,
 * and inside a panel the layout is SSRHIP_TILED(b % 16, k). For b < 16 this is SSRHIP_TILED(b, k). A buffer holds
 * ceil(B/16)*16*K floats (16*K for 5..16 rows). */
#define SSRHIP_TILED_P(b, k, K) (((size_t)(b) >> 4) * 16 * (size_t)(K) + SSRHIP_TILED((b) & 15, k))

int ssrhip_gemv(const ssrhip_gemv_args* a, ssrhip_stream_t stream);

/* Packed bf16 weight layout of the opt-in bf16 weight stream (<= 4 rows, csrc/gemv_w16.hip; K % 1024 == 0). The unit is the fp32 segment
 * kernels' (row, 1024-element segment of K) = 2 KiB; inside it lane l's 16-byte load j (j = 0, 1) sits at byte j*1024 + l*16 and holds the
 * 8 weights of that kernel's float4 #2j followed by #2j+1 of the same lane (float4 #i of lane l = elements i*256 + 4l .. 4l+3 of the
 * segment): a wave-level load is one contiguous KiB and, widened, meets the same pieces of x as in the fp32 kernel. uint16 index of W[n][k]:
 *   r = k % 1024, i = r / 256, lane = (r % 256) / 4:   (n*(K/1024) + k/1024)*1024 + (i/2)*512 + lane*8 + (i%2)*4 + k%4
 * A group's matrix takes N*K uint16; groups follow each other. Each uint16 is the upper half of the fp32 weight rounded to nearest even. */
#define SSRHIP_W16_INDEX(n, k, K) \
  (((size_t)(n) * ((size_t)(K) / 1024) + (size_t)(k) / 1024) * 1024 + ((((k) % 1024) / 256) / 2) * 512 + ((((k) % 1024) % 256) / 4) * 8 + ((((k) % 1024) / 256) % 2) * 4 + (k) % 4)

/* ssrhip_gemv(a) streaming the PACKED bf16 copy `W16` (SSRHIP_W16_INDEX) of a->W instead of a->W itself. a->W must hold exactly the
 * bf16-representable values of W16 (the fp32 "master": what a->W rounds to is what W16 stores); the result is then BIT-IDENTICAL to
 * ssrhip_gemv(a): the weights are widened in registers (a 16-bit shift, exact) and every sum runs in the order of the fp32 kernel.
 *   returns 0 = launched, 1 = `a` does not qualify and NOTHING was launched (call ssrhip_gemv(a)), < 0 = contract error.
 *   Qualifies exactly when ssrhip_gemv takes its segment kernels: B in {1, 2, 4}; K % 1024 == 0 and K / 1024 in {1, 2, 4, 8}; a LayerNorm
 *   prologue only with folded gamma / beta (ln_w == NULL); a split-KV merge prologue only with K == 2048, one group; SSRHIP_GEMV_SEG != 0. */
int ssrhip_gemv_w16(const ssrhip_gemv_args* a, const uint16_t* W16, ssrhip_stream_t stream);
int ssrhip_gemv_w16_applicable(const ssrhip_gemv_args* a);

/* Packed OCP e4m3 weight layout of the opt-in e4m3 weight stream (<= 4 rows, csrc/gemv_w8.hip; K % 1024 == 0). The unit is the fp32
 * segment kernels' (row, 1024-element segment of K) = 1 KiB = one wave-level load; lane l's 16 bytes sit at byte l*16 of the unit and hold
 * that lane's four float4 of the fp32 kernel in order: dword i holds elements i*256 + 4l .. 4l+3 of the segment. Byte index of W[n][k]:
 *   r = k % 1024:   (n*(K/1024) + k/1024)*1024 + ((r % 256)/4)*16 + (r/256)*4 + k%4
 * A group's matrix takes N*K bytes; groups follow each other. Each byte is a finite OCP e4m3 code (torch.float8_e4m3fn; 0x7f / 0xff never
 * occur); the weight is code * scale[n], scale[n] = 2^e one fp32 per output row (per group: scale[g*N + n]). */
#define SSRHIP_W8_INDEX(n, k, K) \
  (((size_t)(n) * ((size_t)(K) / 1024) + (size_t)(k) / 1024) * 1024 + ((((k) % 1024) % 256) / 4) * 16 + (((k) % 1024) / 256) * 4 + (k) % 4)

/* ssrhip_gemv(a) streaming the PACKED e4m3 codes `W8` (SSRHIP_W8_INDEX) and the per-row power-of-two scales `scale` [groups][N] instead of
 * a->W. a->W must hold exactly code * scale (the fp32 "master" q * 2^e); the result is then BIT-IDENTICAL to ssrhip_gemv(a): the codes are
 * widened in registers (v_cvt_pk_f32_fp8, exact), every sum runs in the order of the fp32 kernel, and each (row, segment) partial sum is
 * multiplied by scale[n] where it is parked — a power of two commutes with every fp32 rounding as long as no intermediate value is
 * subnormal or overflows (the caveat: operands of that size round differently on the two sides).
 *   returns 0 = launched, 1 = `a` does not qualify and NOTHING was launched (call ssrhip_gemv(a)), < 0 = contract error.
 *   Qualifies exactly when ssrhip_gemv_w16 does. SSRHIP_GEMV_W8_DEPTH (read at every call): units in flight per wave of the straight-line
 *   form, 2 | 4 | 8 (= every unit at entry); 0 = never that form. */
int ssrhip_gemv_w8(const ssrhip_gemv_args* a, const uint8_t* W8, const float* scale, ssrhip_stream_t stream);
int ssrhip_gemv_w8_applicable(const ssrhip_gemv_args* a);

/* Packed bf16 weight layout of the bf16 weight stream at 5..16 rows (csrc/gemv_mfma_w16.hip; K % 64 == 0): the streaming order
 * SSRHIP_WTILED_INDEX in 2-byte weights. Rows in 8-row units (the last unit zero-padded), K in QUADS of four 16-float k-steps. With
 *   n = 8u + c,  k = 64q + 16j + 4ks + e,  h = j % 2,  g = j / 2
 * the uint16 index of W[n][k] is ((u*(K/64) + q)*2 + h)*256 + (ks*8 + c)*8 + g*4 + e: the 512-byte block (u, q, h) holds, at 16-byte piece
 * ks*8 + c, the four weights of k-step 4q + h followed by the four of k-step 4q + h + 2. The layout does not depend on the kernel form the
 * launch plan picks: the plain form (lanes c >= 8 = the next unit) reads blocks h = 0 and h = 1 of a quad as two wave-level loads of two
 * 512-byte runs each, the k-step-pair form (lanes c >= 8 = the other k-step of a pair) reads both blocks of (u, q) as ONE contiguous KiB.
 * A group's matrix takes ceil(N/8)*8*K uint16; groups follow each other. Each uint16 is the upper half of the (rounded) fp32 master. */
#define SSRHIP_WT16_INDEX(n, k, K) \
  (((((size_t)(n) / 8) * ((size_t)(K) / 64) + (size_t)(k) / 64) * 2 + (((k) % 64) / 16) % 2) * 256 + ((((k) % 16) / 4) * 8 + (n) % 8) * 8 + ((((k) % 64) / 16) / 2) * 4 + (k) % 4)

/* ssrhip_gemv(a) for 5..16 rows streaming the PACKED bf16 copy `Wt16` (SSRHIP_WT16_INDEX) of the weights instead of a->W. `a` is the call as
 * ssrhip_gemv takes it, with a->w_tiled = 1 and a->W = the fp32 streaming-order copy, which must hold exactly the bf16-representable values
 * of Wt16 (the rounded master); the result is then BIT-IDENTICAL to ssrhip_gemv(a): the same launch plan, the weights widened in registers
 * (a 16-bit shift, exact), every MFMA and every sum in the order of the fp32 kernel.
 *   returns 0 = launched, 1 = `a` does not qualify and NOTHING was launched (call ssrhip_gemv(a)), < 0 = contract error (decided before
 *   any HIP call). Qualifies: 5 <= B <= 16, w_tiled == 1, K % 64 == 0, the arguments ssrhip_gemv accepts at these rows, and the
 *   rows-per-workgroup kernels selected (SSRHIP_GEMVM_V != 1). SSRHIP_GEMVM_WPC / _NOPAIR act as on ssrhip_gemv; the fp32 unit's opt-in
 *   experiments (SSRHIP_GEMVM_EDGE, _WFIRST, _DEP8) are ignored — they are bit-identical to the default. */
int ssrhip_gemv_wt16(const ssrhip_gemv_args* a, const uint16_t* Wt16, ssrhip_stream_t stream);
int ssrhip_gemv_wt16_applicable(const ssrhip_gemv_args* a);

/* The same for 17..32 rows (csrc/gemv_mfma32_w16.hip: the two-panel kernels over the SAME packed copy `Wt16`, SSRHIP_WT16_INDEX): the
 * result is BIT-IDENTICAL to ssrhip_gemv(a) at that row count on the fp32 streaming-order copy of the rounded master.
 *   returns 0 = launched, 1 = `a` does not qualify and NOTHING was launched (call ssrhip_gemv(a)): B outside 17..32, w_tiled != 1 or
 *   K % 64 != 0; < 0 = contract error, decided before any HIP call: what ssrhip_gemv refuses at these rows, e.g. a LayerNorm prologue with
 *   K > 2048. SSRHIP_GEMVM_WPC / _NOPAIR act as on ssrhip_gemv. ssrhip_gemv_wt16 keeps answering 1 for these rows. */
int ssrhip_gemv_wt32(const ssrhip_gemv_args* a, const uint16_t* Wt16, ssrhip_stream_t stream);
int ssrhip_gemv_wt32_applicable(const ssrhip_gemv_args* a);

/* Packed OCP e4m3 weight layout of the e4m3 weight stream at 5..16 rows (csrc/gemv_mfma_w8.hip; K % 128 == 0): SSRHIP_WT16_INDEX in 1-byte
 * codes. Rows in 8-row units (the last unit zero-padded: code 0x00), K in OCTETS of eight 16-float k-steps. With
 *   n = 8u + c,  k = 128o + 16j + 4ks + e,  h = j % 2,  g = j / 2
 * the byte index of the code of W[n][k] is ((u*(K/128) + o)*2 + h)*512 + (ks*8 + c)*16 + g*4 + e: the 512-byte block (u, o, h) holds, at
 * 16-byte piece ks*8 + c, as dword g the four codes of k-step 8o + 2g + h. The layout does not depend on the kernel form the launch plan
 * picks: the plain form (lanes c >= 8 = the next unit) reads blocks h = 0 and h = 1 of an octet as two wave-level loads of two 512-byte runs
 * each, the k-step-pair form (lanes c >= 8 = the other k-step of a pair) reads both blocks of (u, o) as ONE contiguous KiB. A group's matrix
 * takes ceil(N/8)*8*K bytes; groups follow each other. Each byte is a finite OCP e4m3 code (torch.float8_e4m3fn; 0x7f / 0xff never occur);
 * the weight is code * scale[n], scale[n] = 2^e one fp32 per output row (per group: scale[g*N + n]; the scales of ssrhip_gemv_w8). */
#define SSRHIP_WT8_INDEX(n, k, K) \
  (((((size_t)(n) / 8) * ((size_t)(K) / 128) + (size_t)(k) / 128) * 2 + (((k) % 128) / 16) % 2) * 512 + ((((k) % 16) / 4) * 8 + (n) % 8) * 16 + ((((k) % 128) / 16) / 2) * 4 + (k) % 4)

/* ssrhip_gemv(a) for 5..16 rows streaming the PACKED e4m3 codes `Wt8` (SSRHIP_WT8_INDEX) and the per-row power-of-two scales `scale`
 * [groups][N] instead of a->W. `a` is the call as ssrhip_gemv takes it, with a->w_tiled = 1 and a->W = the fp32 streaming-order copy of
 * code * scale (the fp32 "master"); the result is then BIT-IDENTICAL to ssrhip_gemv(a): the same launch plan, the codes widened in registers
 * (v_cvt_pk_f32_fp8, exact) and multiplied by their row's scale BEFORE the MFMA (exact: that product is the master), every MFMA and every
 * sum in the order of the fp32 kernel. No caveat about subnormal partial sums applies (ssrhip_gemv_w8 scales sums; this one scales weights).
 *   returns 0 = launched, 1 = `a` does not qualify and NOTHING was launched (call ssrhip_gemv(a)), < 0 = contract error (decided before
 *   any HIP call). Qualifies: 5 <= B <= 16, w_tiled == 1, K % 128 == 0, the arguments ssrhip_gemv accepts at these rows, and the
 *   rows-per-workgroup kernels selected (SSRHIP_GEMVM_V != 1). SSRHIP_GEMVM_WPC / _NOPAIR act as on ssrhip_gemv. */
int ssrhip_gemv_wt8(const ssrhip_gemv_args* a, const uint8_t* Wt8, const float* scale, ssrhip_stream_t stream);
int ssrhip_gemv_wt8_applicable(const ssrhip_gemv_args* a);

/* Two consecutive launches of the 2-row decode step as ONE: `a` = a GEMV with the residual epilogue and `b` = the LayerNorm + Linear that
 * reads a's output, with the all-to-all edge between them inside the launch (csrc/gemv.hip gemv_pair_kernel / gemv_pair_merge_kernel:
 * tagged 8-byte granules, write-through stores, one gather round trip). Two forms:
 *   a = FFN2 (models/modules/transformer.py:386-388 linear2 + the residual add at :328-329), b = the next layer's packed QKV projection
 *       (activation.py:86, with the KV append) or the first Linear of the prediction heads (models/ssr.py:175-179);
 *   a = split-KV merge + out-projection (activation.py:637) + residual, b = LayerNorm + linear1 + ReLU (transformer.py:386-388).
 * Results are bit-identical to ssrhip_gemv(a) followed by ssrhip_gemv(b).
 *   returns 0 = launched, 1 = this (a, b) does not qualify (nothing launched: call ssrhip_gemv twice), < 0 = error.
 *   Qualifies: B == 2 rows; a: ACT_NONE / EPI_RESIDUAL, N == 2048, and either PRO_NONE with K == 8192 or PRO_ATTN_COMBINE with K == 2048;
 *   b: PRO_LAYERNORM with folded gamma / beta, K == 2048, x == a->y, EPI_STORE or EPI_QKV_APPEND, N in {4096, 6144, 8192} (8192 only
 *   behind the merge form); >= 256 CUs; SSRHIP_GEMV_PAIR (0 = never, 1 = only the FFN2 form).
 *   ws: SSRHIP_PAIR_WS_BYTES of device memory, zeroed once by the caller and then owned by the chain of pair launches: three granule
 *   buffers + the give-up flag. `buf` is the buffer this launch uses, `buf_next` (!= buf) the one the NEXT pair launch on this workspace
 *   will use — this launch resets it. Consecutive pair launches must therefore follow each other's buf_next, cyclically.
 *   The launch needs its 256 workgroups resident together (ssrhip_gemv_pair_applicable also asks the occupancy calculator that each pair
 *   kernel fits a CU and refuses when a CU mask is set in the environment); a workgroup that waits longer than ~1 s for the others
 *   gives up, sets the flag and the outputs are garbage: ssrhip_gemv_pair_status (synchronises `stream`) returns 1 ONCE and re-zeroes the
 *   workspace (tags and flag), so the chain can be started again from its first launch. Who may pair at all on a device is decided one
 *   level up, per decode engine: ssrhip_lm_create below. */
#define SSRHIP_PAIR_WS_BYTES (3 * 4096 * 8 + 64)
int ssrhip_pair_buffer(int32_t i, int32_t n);   /* granule buffer (0..2) of the i-th of n cyclically consecutive pair launches; -1: bad i / n < 2 */
int ssrhip_gemv_pair_applicable(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b);
int ssrhip_gemv_pair(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, void* ws, int32_t buf, int32_t buf_next, ssrhip_stream_t stream);
int ssrhip_gemv_pair_status(const void* ws, ssrhip_stream_t stream);

/* ssrhip_gemv_pair(a, b, ...) streaming the PACKED bf16 copies `Wa16` / `Wb16` (SSRHIP_W16_INDEX) of a->W / b->W instead of the masters
 * (csrc/gemv_pair_w16.hip w16_pair_kernel / w16_pair_merge_kernel; DESIGN.md Part I.19). The hand-off is ssrhip_gemv_pair's own: the same
 * barriers, edge role, granules, workspace (SSRHIP_PAIR_WS_BYTES), buffer cycle (ssrhip_pair_buffer) and give-up flag
 * (ssrhip_gemv_pair_status); only the bytes the streaming waves read change. a->W / b->W must hold exactly the values the copies store
 * (ssrhip_gemv_w16); the result is then BIT-IDENTICAL to ssrhip_gemv_w16(a, Wa16) followed by ssrhip_gemv_w16(b, Wb16), and to
 * ssrhip_gemv_pair(a, b) on the masters.
 *   returns 0 = launched, 1 = does not qualify and NOTHING was launched, < 0 = contract error (a null pointer, granule buffers outside
 *   0..2 or equal, EPI_QKV_APPEND16); the answer comes before any HIP call.
 *   Qualifies iff ssrhip_gemv_pair_applicable(a, b) (shapes, >= 256 CUs, no CU mask, SSRHIP_GEMV_PAIR = 0 / 1 / 2 as there) AND
 *   ssrhip_gemv_w16_applicable(a) and (b) (SSRHIP_GEMV_SEG=0 turns it off) AND the occupancy calculator places at least one workgroup of
 *   every bf16 pair kernel on a CU (asked once per process). SSRHIP_GEMV_PAIR_EARLY acts as on ssrhip_gemv_pair. */
int ssrhip_gemv_pair_w16(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, const uint16_t* Wa16, const uint16_t* Wb16, void* ws,
                         int32_t buf, int32_t buf_next, ssrhip_stream_t stream);
int ssrhip_gemv_pair_w16_applicable(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b);

/* ssrhip_gemv_pair(a, b, ...) streaming the PACKED e4m3 codes `Wa8` / `Wb8` (SSRHIP_W8_INDEX) with the per-row scales `scale_a` [a->N] /
 * `scale_b` [b->N] (powers of two) instead of the masters (csrc/gemv_pair_w8.hip w8_pair_kernel / w8_pair_merge_kernel; DESIGN.md Part
 * I.20). The hand-off is ssrhip_gemv_pair's own: the same barriers, edge role, granules, workspace (SSRHIP_PAIR_WS_BYTES), buffer cycle
 * (ssrhip_pair_buffer) and give-up flag (ssrhip_gemv_pair_status); only the bytes the streaming waves read change, and every partial sum
 * is multiplied by its row's scale where it is parked. a->W / b->W must hold exactly code * scale (ssrhip_gemv_w8); the result is then
 * BIT-IDENTICAL to ssrhip_gemv_w8(a, Wa8, scale_a) followed by ssrhip_gemv_w8(b, Wb8, scale_b), and to ssrhip_gemv_pair(a, b) on the
 * masters (the caveat of ssrhip_gemv_w8 about subnormal partial sums applies).
 *   returns 0 = launched, 1 = does not qualify and NOTHING was launched, < 0 = contract error (a null pointer, granule buffers outside
 *   0..2 or equal, EPI_QKV_APPEND16); the answer comes before any HIP call.
 *   Qualifies iff ssrhip_gemv_pair_applicable(a, b) (shapes, >= 256 CUs, no CU mask, SSRHIP_GEMV_PAIR = 0 / 1 / 2 as there) AND
 *   ssrhip_gemv_w8_applicable(a) and (b) (SSRHIP_GEMV_SEG=0 turns it off) AND the occupancy calculator places at least one workgroup of
 *   every e4m3 pair kernel on a CU (asked once per process). SSRHIP_GEMV_PAIR_EARLY acts as on ssrhip_gemv_pair. */
int ssrhip_gemv_pair_w8(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, const uint8_t* Wa8, const float* scale_a, const uint8_t* Wb8,
                        const float* scale_b, void* ws, int32_t buf, int32_t buf_next, ssrhip_stream_t stream);
int ssrhip_gemv_pair_w8_applicable(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b);

/* ssrhip_gemv_pair(a, b, ...) for the 4-ROW decode step (two utterances x CFG, four without), fp32 weights (csrc/gemv_pair4.hip
 * pair4_kernel / pair4_merge_kernel; DESIGN.md Part I.24). The hand-off is ssrhip_gemv_pair's in kind — tagged 8-byte granules, three
 * buffers cycled by ssrhip_pair_buffer, every launch resets the next one's, a time-bounded spin with a give-up flag — at granule index
 * n * 4 + row, 8192 granules per buffer: the workspace is SSRHIP_PAIR4_WS_BYTES, zeroed once by the caller, and is NOT interchangeable with
 * a 2-row workspace. Results are BIT-IDENTICAL to ssrhip_gemv(a) followed by ssrhip_gemv(b) at B = 4.
 *   returns 0 = launched, 1 = does not qualify and NOTHING was launched, < 0 = contract error (a null pointer, granule buffers outside
 *   0..2 or equal, EPI_QKV_APPEND16); the answer comes before any HIP call.
 *   Qualifies iff a->B == b->B == 4 AND ssrhip_gemv_pair_applicable's rules hold for the same two descriptors at 2 rows (shapes, >= 256
 *   CUs, no CU mask, SSRHIP_GEMV_PAIR = 0 / 1 / 2 as there) AND, for the merge form, 4 * n_head * max_splits floats fit 16 KB of LDS AND the
 *   occupancy calculator places at least one workgroup of every 4-row pair kernel on a CU (asked once per process).
 *   ssrhip_gemv_pair4_status is ssrhip_gemv_pair_status for a workspace of this size: 1 ONCE after a give-up, the workspace re-zeroed.
 * ssrhip_gemv_pair, ssrhip_gemv_pair_w16 and ssrhip_gemv_pair_w8 keep answering 1 for B = 4. */
#define SSRHIP_PAIR4_WS_BYTES (3 * 8192 * 8 + 64)
int ssrhip_gemv_pair4_applicable(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b);
int ssrhip_gemv_pair4(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, void* ws, int32_t buf, int32_t buf_next, ssrhip_stream_t stream);
int ssrhip_gemv_pair4_status(const void* ws, ssrhip_stream_t stream);

/* ssrhip_gemv_pair4(a, b, ...) streaming the PACKED copies of a->W / b->W instead of the masters (csrc/gemv_pair4_pk.hip; DESIGN.md Part
 * I.26): the bf16 copies `Wa16` / `Wb16` (SSRHIP_W16_INDEX), or the e4m3 codes `Wa8` / `Wb8` (SSRHIP_W8_INDEX) with the per-row scales
 * `scale_a` [a->N] / `scale_b` [b->N]. The hand-off is ssrhip_gemv_pair4's own — granule index n * 4 + row, the workspace
 * (SSRHIP_PAIR4_WS_BYTES), the buffer cycle (ssrhip_pair_buffer) and the give-up poll (ssrhip_gemv_pair4_status) — only the bytes the
 * streaming waves read change; with e4m3 every partial sum is multiplied by its row's scale where it is parked. The masters must hold
 * exactly the values the copies store (ssrhip_gemv_w16), or code * scale (ssrhip_gemv_w8); the result is then BIT-IDENTICAL to two
 * ssrhip_gemv_w16 (ssrhip_gemv_w8) launches at B = 4 and to ssrhip_gemv_pair4(a, b) on the masters (the caveat of ssrhip_gemv_w8 about
 * subnormal partial sums applies).
 *   returns 0 = launched, 1 = does not qualify and NOTHING was launched, < 0 = contract error (a null pointer, granule buffers outside
 *   0..2 or equal, EPI_QKV_APPEND16); the answer comes before any HIP call.
 *   Qualifies iff the shape rules of ssrhip_gemv_pair4_applicable hold (B == 4; the 2-row question on the same descriptors: shapes, >= 256
 *   CUs, no CU mask, SSRHIP_GEMV_PAIR = 0 / 1 / 2; <= 512 (row, head) pairs and merge weights within 16 KB of LDS) AND the stream's own
 *   ssrhip_gemv_w16_applicable / ssrhip_gemv_w8_applicable takes (a) and (b) (SSRHIP_GEMV_SEG=0 turns it off) AND the occupancy calculator
 *   places at least one workgroup of every kernel of the form on a CU (asked once per process). SSRHIP_GEMV_PAIR_EARLY=0 selects the merge
 *   form without early units, as on ssrhip_gemv_pair_w16. */
int ssrhip_gemv_pair4_w16_applicable(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b);
int ssrhip_gemv_pair4_w16(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, const uint16_t* Wa16, const uint16_t* Wb16, void* ws,
                          int32_t buf, int32_t buf_next, ssrhip_stream_t stream);
int ssrhip_gemv_pair4_w8_applicable(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b);
int ssrhip_gemv_pair4_w8(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, const uint8_t* Wa8, const float* scale_a, const uint8_t* Wb8,
                         const float* scale_b, void* ws, int32_t buf, int32_t buf_next, ssrhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Single-query attention over the paged cache, split over pages (one workgroup per page):
 * replaces F.scaled_dot_product_attention at activation.py:634 for tgt_len==1 (and, row by row,
 * the causal prefill).  Row r attends to positions [0, row_len[r]) of sequence row_seq[r]
 * (row_seq==NULL -> r).  Writes per-page partials (o, m, l); combine via ssrhip_gemv PRO_ATTN_COMBINE
 * or ssrhip_attn_combine.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ssrhip_attn_args {
  const float* q;          /* [R][q_stride] (first n_head*head_dim floats of each row) */
  int32_t q_stride;        /* 0 -> n_head*head_dim */
  ssrhip_kv kv; int32_t layer;
  const int32_t* row_seq;  /* [R] or NULL */
  const int32_t* row_len;  /* [R] */
  int32_t R, max_splits;   /* max_splits >= ceil(max(row_len)/SSRHIP_PAGE) */
  float scale;             /* 1/sqrt(head_dim) */
  float* part_o; float* part_ml;
  int32_t out_tiled;       /* ssrhip_attn_combine / ssrhip_attn_rows: write `out` in the SSRHIP_TILED_P layout (R <= 32) */
  /* ssrhip_attn_decode only, optional (NULL = off; an experiment that did not pay, DESIGN.md Part I.5): while this latency-bound launch runs, workgroup i (linear launch index, the first 256)
   * touches floats [i * prefetch_floats, (i + 1) * prefetch_floats) of `prefetch` with plain loads whose results nobody reads — the weights
   * the NEXT launch's workgroup i will stream (workgroup i of both launches runs on XCD i % 8, so they land in the right L2). */
  const float* prefetch; int32_t prefetch_floats;
} ssrhip_attn_args;

int ssrhip_attn_decode(const ssrhip_attn_args* a, ssrhip_stream_t stream);
int ssrhip_attn_combine(const ssrhip_attn_args* a, float* out /* [R][n_head*head_dim] */, ssrhip_stream_t stream);
/* The same attention (activation.py:634, tgt_len == 1) WITHOUT splitting over pages: one workgroup per (row, head) walks the
 * row's pages with an online softmax and writes the normalised output row directly (part_o / part_ml unused, may be NULL;
 * `out` must not alias q; out_tiled as for ssrhip_attn_combine). Meant for many rows (rows x heads >= the number of CUs): the
 * 5..32-row decode step. */
int ssrhip_attn_rows(const ssrhip_attn_args* a, float* out /* [R][n_head*head_dim] */, ssrhip_stream_t stream);
/* Causal attention of whole PROMPTS (activation.py:634 with the mask of ssr.py:227-255, tgt_len = prompt length): the rows of
 * sequence s are rows seq_start[s] .. seq_start[s+1]-1 of q / out (positions 0 .. len-1, in order); K/V are read from the paged
 * cache (already scattered there), a query at position i sees keys 0..i. K/V tiles are staged in LDS once per 128 queries and
 * both products run on the matrix core (fp32). Uses a->q, q_stride, kv, layer, scale; `seq_start` is a DEVICE array of n_seq+1
 * ints, `max_len` an upper bound of the sequence lengths (grid size). out is row-major [R][n_head*head_dim]. Segment s reads the cache
 * of sequence a->row_seq[seq_start[s]] (row_seq == NULL: sequence s), so a SUBSET of an engine's rows can be prefilled. */
int ssrhip_attn_prefill(const ssrhip_attn_args* a, const int32_t* seq_start, int32_t n_seq, int32_t max_len, float* out,
                        ssrhip_stream_t stream);
/* The bf16 KV cache (opt-in, 5..32-row engines: ssrhip_lm_set_kv16): the two entries above with a->kv.pool read as 2-byte entries (same
 * layout and element offsets; an entry is the upper half of an fp32 value) and widened with a 16-bit shift, which is exact. The
 * arithmetic behind the widening is the fp32 kernels', in their order and with their lane map (a lane's 8-byte load holds the 4 features
 * its 16-byte load held): the result equals the fp32 entry's on the widened pool bit for bit. q, scores, softmax, accumulation and out
 * stay fp32. ssrhip_attn_rows_kv16 keeps 2 or 4 pages in flight per workgroup: SSRHIP_ATTN_KV16_DEPTH = 2 | 4, read at every launch
 * (unset or anything else: 2). */
int ssrhip_attn_rows_kv16(const ssrhip_attn_args* a, float* out /* [R][n_head*head_dim] */, ssrhip_stream_t stream);
int ssrhip_attn_prefill_kv16(const ssrhip_attn_args* a, const int32_t* seq_start, int32_t n_seq, int32_t max_len, float* out,
                             ssrhip_stream_t stream);
/* ssrhip_attn_decode over a 2-byte pool, for the <= 4-row decode step (opt-in: ssrhip_lm_set_kv16_small). The position row_len[r] - 1 of
 * every row — the one this step's QKV launch appended — is NOT in the pool yet: the launch wrote it, fp32, into the landing cache `land`
 * [R][1][2][n_head][SSRHIP_PAGE][head_dim], a->layer's K / V at position a->layer of row r's page. Every workgroup reads its (row, head)'s
 * landing entry, rounds it to bf16 (nearest even) and uses the ROUNDED values for that position, whatever the pool holds there; the
 * workgroup of the page that owns the position stores the rounded entries into the pool (8 bytes per lane) for later steps. `land` is
 * not written. part_o / part_ml equal ssrhip_attn_decode's on the widened pool with the rounded landing entry at row_len[r] - 1, bit for
 * bit. Same grid, SSRHIP_ATTN_VAT and SSRHIP_ATTN_HEAD_FASTEST as ssrhip_attn_decode, a->prefetch honoured. a->row_seq must be NULL
 * (row r is sequence r), a->layer < SSRHIP_PAGE, R <= 65535; every contract error is answered before any HIP call. */
int ssrhip_attn_decode_kv16(const ssrhip_attn_args* a, const float* land, ssrhip_stream_t stream);
/* ssrhip_attn_rows for rows that SHARE their first pages (the samples of one utterance, opt-in: ssrhip_lm_set_prompt_groups; fp32 entries
 * only). chunk_head / n_shared are DEVICE arrays of R ints: chunk_head[r] = the lowest row of r's chunk, a chunk being at most
 * ssrhip_attn_group_members() rows whose first n_shared[head] table entries name the same physical pages (any rows, in any mix of lengths;
 * the caller's contract: rows past that many naming one head are not computed). One workgroup per (head, chunk) loads K/V of a shared page
 * once and folds it into every member's own softmax state with that member's q, then walks each member's own pages. The grid is
 * (n_head, R) whatever the arrays hold — a captured launch keeps working when the arrays are rewritten — and workgroups of non-head rows
 * exit at once. Identity arrays (chunk_head[r] = r, n_shared[r] = 0) are ssrhip_attn_rows. Every row's result equals ssrhip_attn_rows'
 * on the same (aliased) table bit for bit: sharing changes which workgroup computes a row, never the order of its arithmetic.
 * SSRHIP_ATTN_GROUP_MEMBERS = 2 | 4 | 8 (read at every launch; unset or anything else: 2) is the chunk size the kernel is built for. */
int ssrhip_attn_rows_group(const ssrhip_attn_args* a, const int32_t* chunk_head, const int32_t* n_shared,
                           float* out /* [R][n_head*head_dim] */, ssrhip_stream_t stream);
int ssrhip_attn_group_members(void);
/* the same launch with the chunk size as an argument (2, 4 or 8; anything else is a contract error): for a caller that cut its chunks
 * once and must not depend on what the environment says at a later launch (the decode engine) */
int ssrhip_attn_rows_group_m(const ssrhip_attn_args* a, const int32_t* chunk_head, const int32_t* n_shared, int32_t members,
                             float* out /* [R][n_head*head_dim] */, ssrhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Token embedding + sinusoidal position: replaces embed_y (models/ssr.py:191-198, :655-660, :757-761),
 * TokenEmbedding / SinePositionalEmbedding.forward (models/modules/embedding.py:44-48, 94-97).
 *   kind[r]==0: text row   x = text_emb[tok[r][0]] + alpha_text * pe[pos[r]]
 *   kind[r]==1: audio row  x = sum_k audio_emb[k][tok[r][k]] + alpha_audio * pe[pos[r]]
 * ---------------------------------------------------------------------------------------------- */
typedef struct ssrhip_embed_args {
  const float* text_emb;   /* [n_text][D] */
  const float* audio_emb;  /* [K][card][D] */
  const float* pe;         /* [max_pos][D] */
  float alpha_text, alpha_audio;
  const int32_t* tok;      /* [R][SSRHIP_MAX_CODEBOOKS] */
  const int32_t* pos;      /* [R] */
  const int32_t* kind;     /* [R] or NULL (all audio) */
  int32_t R, D, K, card;
  float* out;              /* [R][D] */
  int32_t out_tiled;       /* write `out` in the SSRHIP_TILED_P layout (R <= 32) */
} ssrhip_embed_args;

int ssrhip_embed(const ssrhip_embed_args* a, ssrhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Per-step sampler + logit state machine, one workgroup per utterance, no host sync:
 * replaces models/ssr.py:689-754 (CFG combine, special-token edits, eog cascade, silence penalty,
 * topk_sampling/top_k_top_p_filtering :26-86, stop rules, span hand-over :646-660).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ssrhip_sampler_cfg {     /* per utterance, device memory, read-only during decode */
  int32_t top_k; float top_p; float temperature; int32_t stop_repetition;
  float cfg_coef; float cfg_one_minus; /* fp32(1 - cfg_coef) computed in double like the reference :692 */
  int32_t cfg_stride; int32_t use_cfg;
  int32_t n_silence; int32_t silence[SSRHIP_MAX_SILENCE];
  int32_t text_len;        /* L of the (doubled) text batch, for the 10*L cap :739 */
  int32_t n_spans;         /* num_task */
  int32_t empty_token, eog, eos, sos, mts, max_n_spans;
  int32_t max_steps;       /* capacity of `generated` per utterance */
  uint32_t seed_lo, seed_hi; /* on-device RNG stream when noise==NULL or use_noise==0 */
  int32_t use_noise;       /* 1: take the multinomial's Exp(1) draws from `noise` (host-drawn, reproduces torch's CPU stream);
                              0: on-device hash RNG. Lets one engine keep ONE persistent noise buffer (stable pointer, no graph
                              re-capture) whether or not a given generation uses it. */
} ssrhip_sampler_cfg;

typedef struct ssrhip_sampler_state {   /* per utterance, device memory, mutated every step */
  int32_t span;            /* current span index */
  int32_t num_gen, num_eog, num_cfg_tag, prev_token, consec_silence;
  int32_t audio_pos;       /* position of the token being fed this step (y_input.shape[1]-1) */
  int32_t n_steps;         /* samples written so far (all spans) */
  int32_t done;            /* 1 when all spans finished (or max_steps hit: 2) */
  int32_t span_end[3];     /* n_steps at the end of each finished span */
  int32_t pad[3];
} ssrhip_sampler_state;

typedef struct ssrhip_sample_args {
  const float* logits;     /* [B][K][card]; rows 2u,2u+1 when use_cfg else row u */
  int32_t n_utt, K, card;
  const ssrhip_sampler_cfg* cfg;
  ssrhip_sampler_state* state;
  const float* noise;      /* [n_utt][max_steps][K][card] Exp(1) draws, or NULL */
  int32_t* generated;      /* [n_utt][max_steps][K] */
  int32_t* next_tok;       /* [B][SSRHIP_MAX_CODEBOOKS] token ids fed to ssrhip_embed next step */
  int32_t* next_pos;       /* [B] audio position of the next input */
  int32_t* kv_pos;         /* [B] incremented for live utterances */
  int32_t* row_len;        /* [B] = kv_pos+1 */
  float* dbg_logits;       /* optional [n_utt][K][card] post-edit logits (tests) or NULL */
  ssrhip_embed_args embed; /* embed.out != NULL: also write the next input rows x[b] = embed(next_tok) (fused, saves a launch) */
} ssrhip_sample_args;

int ssrhip_sample(const ssrhip_sample_args* a, ssrhip_stream_t stream);
/* ssrhip_sample, and the log-probability of every token it generates (DESIGN.md Part I.27): for utterance u, its step s and codebook k,
 *     logp[(u * max_steps + s) * K + k] = z[t] - logsumexp(z over all card entries)          (natural log, fp32)
 * where z = the logits handed to the reference's topk_sampling (after the CFG combine, the special-token edits and the silence penalty,
 * before top-k / top-p) divided by the temperature, and t = generated[u][s][k]. NaN where the state machine, not the draw, decided t:
 * the start-of-span delay (num_gen < K-1 and k > num_gen), the eog cascade (num_eog > 0 and k <= num_eog) and the stop rule
 * (num_eog == 0, k == 0 and argmax == eog or audio_pos + 1 > 10 * text_len), by the state at kernel entry; NaN also where t is no index of
 * the card (nothing to draw from: every logit NaN). An utterance that is done writes nothing; a live one writes all K values of its step. Same tokens, state and next-step inputs as ssrhip_sample; one more workgroup-wide sum and, without the fused embed,
 * one more barrier. `logp` is a DEVICE buffer [n_utt][max_steps][K] of the caller's; NULL is an argument error. */
int ssrhip_sample_logp(const ssrhip_sample_args* a, float* logp, ssrhip_stream_t stream);

/* The batched stream's hand-off from the sampler to the codec (DESIGN.md Part I.16): for utterance u < n_utt, generated frame f in
 * [f0[u], f1[u]) and codebook k < K,
 *     codes_out[u][k][col0[u] + f] = generated[u][step0[u] + f + k][k]
 * — the delay pattern undone (revert_pattern_sequence, models/ssr.py:438-464) — as the [B][K][cap] int32 block ssrhip_rvq_decode
 * reads. An id outside [0, bins) is stored clamped and sets *flag = 1 (never cleared here: the caller zeroes it once and reads it after
 * every launch). The ranges are one int32 table [4][n_utt] = step0 | f0 | f1 | col0, given twice: `ranges_host` is checked here before
 * any HIP call (f0 <= f1, every step < max_steps, every column < cap), `ranges_dev` is the copy the kernel reads (pushed by the caller
 * ahead of this call on the same stream, as the page table is) and checks again. One launch whatever n_utt is; none when every range
 * is empty. generated = [n_utt][max_steps][K], the sampler's buffer. */
int ssrhip_stream_gather(const int32_t* generated, int32_t n_utt, int32_t max_steps, int32_t K, const int32_t* ranges_host,
                         const int32_t* ranges_dev, int32_t* codes_out, int32_t B, int32_t cap, int32_t bins, int32_t* flag,
                         ssrhip_stream_t stream);

/* The batched watermarked stream's row mover (DESIGN.md Part I.29; csrc/stream_rows.hip): ONE launch executes a table of up to
 * SSRHIP_STREAM_ROWS_MAX_OPS operations on fp32 buffers. Op i, for r < rows and c < width:
 *     mode 0:  dst[r * dst_ld + c] = 0                                  (src is never read)
 *     mode 1:  dst[r * dst_ld + c] = src[r * src_ld + c]
 * dst_ld / src_ld are floats per row step; src_ld may be negative or 0 (a reflected edge is a copy that walks its source backwards).
 * Copies and zeros only: the result is exact. An op whose rows all start on 16-byte boundaries and hold a multiple of 4 floats
 * (both pointers, both steps, the width) moves 16 bytes per lane, any other op 4 bytes per lane. The table is given twice, as
 * ssrhip_stream_gather's: `ops_host` is checked here before any HIP call — 0 <= n_ops <= SSRHIP_STREAM_ROWS_MAX_OPS, counts >= 0,
 * mode 0 or 1, |dst_ld| >= width where rows > 1, and no op's dst range may overlap another op's dst range or any op's src range
 * (its own included; ranges are compared as bounding address intervals) — and sizes the grid; `ops_dev` is the copy the kernel reads,
 * pushed by the caller ahead of this call on the same stream. Returns 0 on launch, 0 without a launch when every op is empty, < 0 with
 * ssrhip_last_error on a contract error. The record has no index in ssrhip_sizeof: its size comes back through
 * ssrhip_stream_rows_sizeof. */
#define SSRHIP_STREAM_ROWS_MAX_OPS 64
typedef struct ssrhip_rows_op {
  float* dst;
  const float* src;        /* mode 1 only */
  int64_t dst_ld, src_ld;  /* floats per row step */
  int32_t rows, width;
  int32_t mode, reserved_;
} ssrhip_rows_op;
int ssrhip_stream_rows_sizeof(void);
int ssrhip_stream_rows(const ssrhip_rows_op* ops_host, const ssrhip_rows_op* ops_dev, int32_t n_ops, ssrhip_stream_t stream);

/* The opt-in device-side source of the sampler's noise (DESIGN.md Part I.21; csrc/noise.hip): one launch writes the Exp(1) draws of up to
 * SSRHIP_NOISE_MAX_SEGMENTS segments — steps [first_step, first_step + n_steps) of utterance slot `slot`, drawn from the utterance's
 * 64-bit seed (seed_lo, seed_hi) — into noise[n_utt][max_steps][K][card], the buffer ssrhip_sampler_cfg.use_noise = 1 makes the
 * sampler read. The stream: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85), key = (seed_lo,
 * seed_hi), counter = (b, t, 0x6e6f6973, 0) for block b of step t; word j of the block is element e = 4b + j of the step's flattened
 * [K][card] tensor (the last block is used partly when K * card % 4 != 0). A word w gives n = w >> 9, u = (n + 0.5) * 2^-23 (exact in
 * fp32) and the value -logf(u), in [5.96e-8, 16.64]. A value depends on (seed, t, e) only. `words` (optional, tests): a buffer of the
 * same shape that receives the raw word of every element written. The whole record travels by value in the kernel's arguments: no device
 * table, no copy. Contract errors (a null pointer, more than SSRHIP_NOISE_MAX_SEGMENTS segments, a negative range, a segment that ends
 * past max_steps, a slot >= n_utt) return < 0 before any HIP call. The record has no index in ssrhip_sizeof: its size comes back
 * through ssrhip_noise_sizeof. */
#define SSRHIP_NOISE_MAX_SEGMENTS 32
typedef struct ssrhip_noise_segment {
  int32_t slot, first_step, n_steps;
  uint32_t seed_lo, seed_hi;
} ssrhip_noise_segment;
typedef struct ssrhip_noise_args {
  float* noise;            /* [n_utt][max_steps][K][card] */
  uint32_t* words;         /* optional, same shape: the raw Philox word of each element written */
  int32_t n_utt, max_steps, K, card;
  int32_t n_seg;
  ssrhip_noise_segment seg[SSRHIP_NOISE_MAX_SEGMENTS];
} ssrhip_noise_args;
int ssrhip_noise_sizeof(void);
int ssrhip_noise_philox(const ssrhip_noise_args* a, ssrhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Dense fp32 GEMM on the matrix cores (v_mfma_f32_32x32x2_f32, exact fp32 FMA chain) for the
 * prefill rows and the codec:  C[M][N] = epi( A[M][K] . W[N][K]^T + bias[N] ), act/residual as GEMV.
 * replaces the same F.linear call sites as ssrhip_gemv when tgt_len > 4.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ssrhip_gemm_args {
  const float* A; const float* W; const float* bias; float* C;
  int32_t M, N, K, lda, ldc;
  int32_t act, residual;   /* residual: C += ... (in place) */
  /* --- extensions used by the codec (all zero = plain GEMM) --- */
  int32_t act_in;          /* SSRHIP_ACT_ELU: apply ELU(alpha=1) to A while staging it (conv input activation) */
  const float* R; int32_t ldr;      /* R != NULL: C = epi(...) + R[m*ldr+n]  (SEANet residual block skip) */
  int32_t batch;           /* grid.z; 0/1 = single problem */
  int64_t strideA, strideC, strideR; /* per-batch element strides */
  int32_t tm_c, tm_lo, tm_hi;       /* tm_c > 0: element (m,n) belongs to time row u = (m*N+n)/tm_c and is stored only
                                       if tm_lo <= u < tm_hi (transposed-conv trimming, modules/conv.py:236-243) */
  /* per-row CLASS bias (all NULL/0 = off): C[m][n] += rbias[rclass[z * rclass_stride + m / rrep] * N + n]  (z = batch index).
   * The watermark decoder's label conditioning (modules/seanet.py:577-591): the 1x1 convolution over cat(skip, embed(label))
   * splits into W_a . ELU(skip) + (W_b . ELU(embed(label))), and the second term takes only as many values as there are labels —
   * so the concatenated tensor is never built and the GEMM's K shrinks by the embedding width. */
  const float* rbias; const int32_t* rclass; int32_t rrep, rclass_stride;
  /* optional (NULL = always the fp32 FMA chain): W as three bf16 planes [3][N][K] made by ssrhip_split_weights. When given — and the
   * problem is large enough, N > 64, K % 8 == 0 — the GEMM runs on the bf16 matrix cores with every fp32 operand split EXACTLY into
   * three bf16 pieces and the six largest cross products accumulated in fp32 (csrc/gemm_split.hip): fp32 accuracy (error against an
   * fp64 reference no larger than the fp32 chain's), ~1.3-1.5x the speed, NOT bit-identical to the k-ordered fp32 chain. The codec
   * passes it, and so do the LM prefill and ssrhip_lm_score when their weights record carries planes (ssrhip_lm_weights *_ws).
   * For ssrhip_gemm_w1 (below) the same field holds ONE bf16 plane [N][K]. */
  const uint16_t* W_split;
  /* SSRHIP_ACT_ELU: apply ELU(alpha = 1) LAST — after act, residual, R and the class bias — i.e. store what the consumer would compute
   * on load. For tensors that are only ever read through ELU (SEANet: a residual block's output feeds `ELU -> conv`, seanet.py:137-141,
   * 236-247) the activation then runs once per element in the producer instead of once per (tap, column block) in every consumer. */
  int32_t act_out;
} ssrhip_gemm_args;
int ssrhip_gemm(const ssrhip_gemm_args* a, ssrhip_stream_t stream);
/* W fp32 [n_elems] -> out bf16 [3][n_elems]: piece p of element i at out[p * n_elems + i], w = w0 + w1 + w2 exactly
 * (w0 = bf16_rne(w), w1 = bf16_rne(w - w0), w2 = bf16_rne(w - w0 - w1)). One-time preparation of a weight matrix for W_split. */
int ssrhip_split_weights(const float* W, uint16_t* out, int64_t n_elems, ssrhip_stream_t stream);
/* The split GEMM for a weight matrix whose every value IS a bf16 value (a weight_dtype="bf16" arena's masters): `a->W_split` is ONE bf16
 * plane [N][K] (the values themselves, 2 bytes per weight), `a->W` is not read. The exact split of such a matrix has two planes of
 * zeros; this entry runs the three products that remain (a2w0, a1w0, a0w0, in ssrhip_gemm's order) with one W plane in flight, in the
 * tile shapes ssrhip_gemm would choose, and returns ssrhip_gemm's result on the three planes of the same matrix BIT FOR BIT for finite
 * activations (a non-finite activation times a zero plane is NaN in the six-product form only). Returns 0 when it launched; 1 when the
 * call does not qualify and NOTHING was launched — ssrhip_gemm's rule for W_split (N > 64, K % 8 == 0, grid limits, SSRHIP_GEMM_SPLIT
 * not "0..."), and act_in == SSRHIP_ACT_ELU, which has no one-plane kernel; the caller then calls ssrhip_gemm with W_split = NULL, the
 * chain a three-plane call that does not qualify takes too; < 0 for a contract error (ssrhip_last_error; e.g. W_split == NULL), before
 * any HIP call. NEVER hand a one-plane buffer to ssrhip_gemm: it reads three planes, twice the buffer's size past its end. */
int ssrhip_gemm_w1(const ssrhip_gemm_args* a, ssrhip_stream_t stream);
/* how many calls of ssrhip_gemm_w1 launched a one-plane kernel (answered 0) in this process so far, through whichever entry (direct,
 * ssrhip_lm_prefill, ssrhip_lm_score_w1): a caller that expects the one-plane path can tell it from the silent fp32-chain fallback. */
int64_t ssrhip_gemm_w1_launches(void);
/* ssrhip_gemm_w1 for the codec's bf16-rounded weights (WMEncodecModel weight_dtype="bf16"): the same contract — W_split is ONE bf16 plane
 * [N][K]; 0 launched, 1 does not qualify and nothing was launched, < 0 contract error before any HIP call — and the same bits as
 * ssrhip_gemm on the three planes of the same matrix, but it also launches a one-plane kernel for act_in == SSRHIP_ACT_ELU and takes the
 * time-mask-folded 16-byte epilogue under exactly the conditions a three-plane call takes it. It answers 1 only where ssrhip_gemm's rule
 * for W_split fails. Plan, tile order, k-block order and product order (a2w0, a1w0, a0w0) are those of the three-plane call. */
int ssrhip_codec_gemm_w1(const ssrhip_gemm_args* a, ssrhip_stream_t stream);
/* how many calls of ssrhip_codec_gemm_w1 and ssrhip_resblock_w1 launched a one-plane kernel (answered 0) in this process so far;
 * ssrhip_gemm_w1_launches does not count them. */
int64_t ssrhip_codec_w1_launches(void);
/* ssrhip_codec_gemm_w1 with the activation operand ROUNDED to bf16 (nearest even) where that entry splits it in three — behind ELU on
 * load where act_in == SSRHIP_ACT_ELU (WMEncodecModel weight_dtype="bf16", act_dtype="bf16"): one product a0w0 per k block, one A plane
 * in LDS. Its twin's contract — W_split is ONE bf16 plane [N][K]; 0 launched, 1 does not qualify and nothing was launched, under exactly
 * the twin's conditions, < 0 contract error before any HIP call — and its plan, tile order, k-block order and epilogues: accumulation,
 * bias, residual, ELU on store, time mask and class bias in fp32. On activations that already are bf16 values (and act_in NONE) the twin's
 * result BIT FOR BIT. */
int ssrhip_codec_gemm_a1(const ssrhip_gemm_args* a, ssrhip_stream_t stream);
/* how many calls of ssrhip_codec_gemm_a1 and ssrhip_resblock_a1 launched a kernel (answered 0) in this process so far; the other
 * counters do not count them. */
int64_t ssrhip_codec_a1_launches(void);


/* ------------------------------------------------------------------------------------------------
 * Codec (watermarked Encodec) kernels. Activations are TIME-MAJOR fp32: one item = [rows][C] with C contiguous,
 * so a Conv1d (kernel k, stride s) over a zero/reflect-padded buffer is a plain GEMM on a strided view:
 * A row t = k consecutive time rows = k*C contiguous floats starting at padded row t*s (lda = s*C), W repacked to
 * [Cout][k][Cin]; a ConvTranspose1d (k = 2s) is ONE GEMM with N = s*Cout (the s output phases side by side) and
 * K = 2*Cin, trimmed by the time mask. replaces StreamableConv1d / StreamableConvTranspose1d
 * (audiocraft/modules/conv.py:185-243) and SEANetResnetBlock (modules/seanet.py:16-60) via ssrhip_gemm.
 * ---------------------------------------------------------------------------------------------- */
/* first conv of SEANet (Cin == 1): out[b][t][co] = bias[co] + sum_kk w[co][kk] * x[b][t*stride + kk]  (x pre-padded) */
int ssrhip_conv_cin1(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t T_out, int32_t k,
                     int32_t stride, int32_t Cout, int64_t x_bstride, int64_t out_bstride, ssrhip_stream_t stream);
/* convolution with at most 4 OUTPUT channels on a time-major, pre-padded input (SEANet's last layer, 64 -> 1, k = 7; conv.py:185-201):
 * out[b][t][co] = bias[co] + sum_{kk, ci} w[co][kk][ci] * act_in(x[b][t + kk][ci]);  w is [Cout][k][Cin]; act_in NONE or ELU */
int ssrhip_conv_few_out(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t T_out, int32_t k,
                        int32_t Cin, int32_t Cout, int32_t act_in, int64_t x_bstride, int64_t out_bstride, ssrhip_stream_t stream);
/* reflect padding of a time-major buffer (conv.py:71-88): rows [0,padL) and [padL+T, padL+T+padR) mirror the interior */
int ssrhip_pad_reflect(float* buf, int32_t B, int32_t T, int32_t padL, int32_t padR, int32_t C, int64_t bstride,
                       ssrhip_stream_t stream);
/* halo rows of a RAGGED batch in a time-major buffer [B][padL + T + padR][C] whose producer wrote T rows for every item although
 * item b holds only lens[b] <= T valid ones (device array): the padR rows right behind item b's last valid row (rows padL + lens[b] ..,
 * partly inside the dense interior) and, for reflect, its padL leading rows get the padding an item of that length ALONE would have —
 * zeros (reflect == 0) or the mirror image about its own ends (conv.py:71-88, incl. the zero extension of inputs shorter than the
 * pad). Every layer of the batch then computes, for t < its own length, exactly what a batch-1 call computes (the SEANet
 * convolutions are not causal, so dense zero padding of a short item would change its tail; wmencodec.py:341-375 per item). */
int ssrhip_pad_ragged(float* buf, const int32_t* lens, int32_t B, int32_t T, int32_t padL, int32_t padR, int32_t C, int64_t bstride,
                      int32_t reflect, ssrhip_stream_t stream);
/* one LSTM layer over T steps (torch.nn.LSTM semantics, gates i,f,g,o; modules/lstm.py:10-25):
 * gin[b][t][4C] = x_t W_ih^T + b_ih + b_hh (precomputed by ssrhip_gemm); h,c start at 0.
 * One call runs the steps [t_begin, t_end) (t_end <= 0: up to T). A call with t_begin == 0 starts from h = c = 0 whatever hbuf / cbuf
 * hold; a call with t_begin > 0 CONTINUES from the hbuf / cbuf (and hsplit) the call that ended at t_begin left there — h_t lives in
 * half (t & 1) of hbuf by the ABSOLUTE step, so the buffers, B, C and the path must be the same from call to call and nothing else may
 * write them in between. Any split of [0, n) into consecutive calls writes the bits of the one call over [0, n). T is the CAPACITY of
 * gin and out in steps (their row count per item), not the number of steps run: a caller that does not know the final length yet
 * (codec/wmencodec.py DecodeStream) sizes them for the longest case and advances as inputs arrive.
 * out[b][t][C] = h_t (+ skip[b][t][C] when skip != NULL).  cbuf: [B][C]; hbuf: [2][ceil(B/16)*16][C] floats (row-major
 * [B][C] on the small-batch path B <= 4 && C in {256,512,1024,2048}; otherwise kept in the SSRHIP_TILED layout per 16-item
 * tile, which needs C <= 1024); gates: unused (may be NULL). C % 16 == 0. */
typedef struct ssrhip_lstm_args {
  const float* gin; const float* w_hh; float* out; const float* skip;
  float* hbuf; float* cbuf; float* gates;
  int32_t B, T, C;
  int64_t gin_bstride, out_bstride, skip_bstride;   /* element strides between items */
  /* time window of this call: steps [t_begin, t_end) of the T-step sequence (t_end == 0 means T). t_begin == 0 starts from
   * h = c = 0; a later window continues from the state the previous call left in hbuf / cbuf. Lets a caller run two stacked
   * layers as a software pipeline over chunks of steps on two streams (layer 2 chunk i beside layer 1 chunk i+1). */
  int32_t t_begin, t_end;
  /* matrix-core path only (B > 4, or C not in {256,512,1024,2048}): w_hh is given as 16 x 16 blocks in lane order,
   * packed[C/4 tiles][C/16 k-steps][4 k-slots][16 rows][4 floats] with row r of tile j = W_hh[(r % 4) * C + 4j + r / 4] (gate r % 4 of
   * hidden unit 4j + r / 4), so that one wave-level load is one contiguous KiB instead of 64 pieces of 16 rows */
  int32_t w_packed;
  int32_t out_act;   /* SSRHIP_ACT_ELU: out = ELU(h_t (+ skip)) (the layer's only consumer is `ELU -> conv`: seanet.py:147-150, 226-236) */
  /* optional (both or none; used when C % 128 == 0 and B >= 32): the recurrent product on the bf16 matrix cores with exactly split fp32
   * operands (csrc/lstm_split.hip), both operands in MFMA fragment order — KS = C/64 k-steps of 16 per wave, a block = 64 lanes x 8 bf16:
   *   w_split [C/16][4][KS][2][3][64][8]: lane l (li = l % 32, lh = l / 32), element e of block (ub, w, s, mb, q) = piece q
   *            (ssrhip_split_weights) of w_hh[g C + 16 ub + u][w C/4 + 16 s + 8 lh + e] with 32 mb + li = 16 g + u;
   *   hsplit  workspace, 2 x ceil(B/64) x 64 x C x 3 bf16 (two buffers by step parity): h_t in the same order, written and zeroed by
   *            the library. `hbuf` is not used on this path (it still has to be a valid pointer). */
  const uint16_t* w_split; uint16_t* hsplit;
} ssrhip_lstm_args;
int ssrhip_lstm_layer(const ssrhip_lstm_args* a, ssrhip_stream_t stream);
/* The split-operand step of ssrhip_lstm_layer for a recurrent matrix whose every value IS a bf16 value (WMEncodecModel
 * weight_dtype="bf16"): `a->w_split` is ONE bf16 plane in fragment order, [C/16][4][KS][2][64][8] — the slice q = 0 of the three-plane
 * layout above, a third of its bytes — and `a->hsplit` is the three-plane path's workspace, byte for byte (h is an fp32 activation and keeps
 * its three pieces). Three products per accumulator and k-step instead of six (csrc/lstm_w1.hip). ssrhip_lstm_layer's contract and time
 * windows: a call with t_begin == 0 zeroes both hsplit buffers, a later window continues from them; out / cbuf / hsplit are those of
 * ssrhip_lstm_layer on the three planes of the same matrix BIT FOR BIT, so windows of one sequence may alternate between the two entries.
 * Returns 0 when it launched; 1, launching nothing, where ssrhip_lstm_layer would not take the split step (C % 128 != 0, C > 4096,
 * B < 32, or the small-batch shapes B <= 4 with C in {256,512,1024,2048}): the caller then calls ssrhip_lstm_layer with
 * w_split = hsplit = NULL; < 0 for a contract error (a null argument, w_split and hsplit not both set, a bad window), before any HIP
 * call. SSRHIP_LSTM_W1_DEPTH=8 (read at every call) keeps eight k-steps in flight instead of four where C % 512 == 0. NEVER hand a
 * one-plane buffer to ssrhip_lstm_layer: it reads three planes, twice the buffer's size past its end. */
int ssrhip_lstm_layer_w1(const ssrhip_lstm_args* a, ssrhip_stream_t stream);
/* how many one-plane STEP kernels ssrhip_lstm_layer_w1 has launched in this process so far (one per time step of every call that
 * answered 0); ssrhip_codec_w1_launches does not count them. */
int64_t ssrhip_lstm_w1_launches(void);
/* residual vector quantisation (quantization/core_vq.py:164-179, 382-400): emb [B][T][D] time-major;
 * codebooks [n_q][bins][D]; e2 [n_q][bins] = |e|^2; codes int32 [B][n_q][T] */
int ssrhip_rvq_encode(const float* emb, const float* codebooks, const float* e2, int32_t* codes, int32_t B, int32_t T,
                      int32_t D, int32_t n_q, int32_t bins, int64_t emb_bstride, ssrhip_stream_t stream);
int ssrhip_rvq_decode(const int32_t* codes, const float* codebooks, float* out, int32_t B, int32_t T, int32_t D,
                      int32_t n_q, int32_t bins, int64_t out_bstride, ssrhip_stream_t stream);
/* Fused SEANetResnetBlock (modules/seanet.py:16-60; true_skip, dilation 1, kernel sizes 3 and 1) for C in {64, 128, 256, 512}
 * channels (64: one persistent kernel with W3 resident in LDS; wider: two chained GEMMs with the C/2 intermediate kept in LDS):
 *   y[b][t][:] = x[b][t][:] + b1 + W1 . ELU(b3 + W3 . ELU(x[b][t-1 : t+2][:]))
 * x points at the row BEFORE t = 0 of item 0 of a time-major buffer [B][1 + T + 1][C] (halo rows hold the zero / reflect
 * padding); w3 is [C/2][3][C] (output channel, tap, input channel), w1 is [C][C/2]; y points at row t = 0. */
typedef struct ssrhip_resblock_args {
  const float* x; float* y;
  const float* w3; const float* b3; const float* w1; const float* b1;
  int32_t B, T, C;
  int64_t x_bstride, y_bstride;   /* elements between items */
  int32_t out_act;                /* SSRHIP_ACT_ELU: y = ELU(block(x)): the block's only consumer is `ELU -> conv` */
  /* optional (both or none; C in {64, 128}): the two weight matrices as three bf16 planes each (ssrhip_split_weights) — the block then runs
   * on the bf16 matrix cores with exactly split fp32 operands, weights streamed global -> LDS by DMA (csrc/resblock_split.hip).
   *   w3_split: planes of w3 as it is, [3][C/2][3*C];
   *   w1_split: planes of w1 with its COLUMNS permuted into the order the kernel's stage-1 accumulator hands the hidden channels on:
   *             column k' = 16 j + 8 g + i (j = k'/16, g = (k'/8) % 2, i = k' % 8) holds hidden channel h = 16 j + (i % 4) + 8 (i / 4) + 4 g. */
  const uint16_t* w3_split; const uint16_t* w1_split;
} ssrhip_resblock_args;
int ssrhip_resblock(const ssrhip_resblock_args* a, ssrhip_stream_t stream);
/* The DMA kernel of ssrhip_resblock for matrices whose every value IS a bf16 value: w3_split and w1_split (both required) hold ONE bf16
 * plane each — [C/2][3*C], and [C][C/2] in the permuted column order above — and w3 / w1 are not read. Three products per k block
 * instead of six, a third of the weight bytes through LDS; ssrhip_resblock's result on the three planes of the same matrices BIT FOR BIT
 * for finite activations. Returns 0 when it launched; 1, launching nothing, where ssrhip_resblock would not take the DMA kernel (C not
 * in {64, 128}, SSRHIP_GEMM_SPLIT=0, SSRHIP_RESBLOCK_DMA=0): the caller then calls ssrhip_resblock WITHOUT planes; < 0 for a contract
 * error (a NULL plane), before any HIP call. NEVER hand a one-plane buffer to ssrhip_resblock. Counted by ssrhip_codec_w1_launches. */
int ssrhip_resblock_w1(const ssrhip_resblock_args* a, ssrhip_stream_t stream);
/* ssrhip_resblock_w1 with both activation operands ROUNDED to bf16 (nearest even) where that entry splits them in three: ELU(x), and
 * ELU(H + b3) between the two stages. One product per k block in both stages; the residual x is added back in fp32. Its twin's arguments,
 * answers (0 / 1 under exactly its conditions / < 0 before any HIP call) and ring default. Counted by ssrhip_codec_a1_launches. */
int ssrhip_resblock_a1(const ssrhip_resblock_args* a, ssrhip_stream_t stream);

/* LayerNorm over rows (transformer.py:58-75) */
int ssrhip_layernorm(const float* x, const float* w, const float* b, float eps, float* y, int32_t R, int32_t D,
                     ssrhip_stream_t stream);

/* Scatter the k/v thirds of a packed qkv buffer [R][3D] into the paged cache; row r -> sequence
 * row_seq[r], position row_pos[r].  (activation.py:626-631 for the prefill rows) */
int ssrhip_kv_scatter(const float* qkv, const ssrhip_kv* kv, int32_t layer, const int32_t* row_seq,
                      const int32_t* row_pos, int32_t R, ssrhip_stream_t stream);
/* The same into a cache of 2-byte entries (kv->pool points at bf16 storage, same layout): every value rounded to nearest even like
 * SSRHIP_EPI_QKV_APPEND16. */
int ssrhip_kv_scatter16(const float* qkv, const ssrhip_kv* kv, int32_t layer, const int32_t* row_seq,
                        const int32_t* row_pos, int32_t R, ssrhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Decode engine: one LM, B rows; prefill + N decode steps replayed from a captured hipGraph.
 * replaces the body of SSR_Speech.inference (models/ssr.py:597-754) on the device.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ssrhip_lm_weights {      /* device pointers; per-layer arrays have n_layer entries (host arrays) */
  const float* text_emb; const float* audio_emb; const float* pe; float alpha_text, alpha_audio;
  const float* const* ln1_w; const float* const* ln1_b;
  const float* const* in_proj_w; const float* const* in_proj_b;
  const float* const* out_proj_w; const float* const* out_proj_b;
  const float* const* ln2_w; const float* const* ln2_b;
  const float* const* ffn1_w; const float* const* ffn1_b;
  const float* const* ffn2_w; const float* const* ffn2_b;
  const float* lnf_w; const float* lnf_b;
  const float* head1_w; const float* head1_b;   /* [K*Hh][D], [K*Hh]   (predict_layer.k.0 stacked) */
  const float* head2_w; const float* head2_b;   /* [K][card][Hh], [K][card] (predict_layer.k.2 stacked) */
  /* optional second copy of the six matrices in the streaming order of the 5..32-row GEMV (SSRHIP_WTILED_INDEX; all NULL = absent).
   * Used by the decode steps of engines with more than 4 rows; the prefill GEMMs and the <= 4-row GEMV read the [N][K] copies. */
  const float* const* in_proj_wt; const float* const* out_proj_wt; const float* const* ffn1_wt; const float* const* ffn2_wt;
  const float* head1_wt; const float* head2_wt;
  /* optional (all four or none; NULL = the fp32 FMA chain): the four matrices of every layer as three bf16 planes each (ssrhip_split_weights)
   * for the PREFILL GEMMs (ssrhip_lm_prefill: tgt_len = prompt length): fp32 operands split exactly, six cross products on the bf16 matrix
   * cores (ssrhip_gemm_args.W_split: error against fp64 no larger than the chain's, not bit-identical to it). The decode step never reads them. */
  const uint16_t* const* in_proj_ws; const uint16_t* const* out_proj_ws; const uint16_t* const* ffn1_ws; const uint16_t* const* ffn2_ws;
} ssrhip_lm_weights;

typedef struct ssrhip_lm_dims {
  int32_t d_model, n_head, n_layer, d_ffn, n_codebooks, card, head_hidden, n_text, max_pos;
  int32_t ln_folded;   /* 1: the LayerNorm affine (gamma, beta) of norm1/norm2/decoder.norm is already folded into in_proj/ffn1/head1
                          (W' = W diag(gamma), b' = b + W beta); ln*_w / ln*_b then hold ones / zeros (used by the prefill LayerNorm) */
} ssrhip_lm_dims;

typedef struct ssrhip_lm_buffers {      /* caller-allocated device workspaces */
  int32_t B, n_utt, max_splits;   /* B in {1, 2, 4} or 5..32 rows; with B > 4, x / q / h hold ceil(B/16)*16 rows (SSRHIP_TILED_P) */
  int32_t pair_mode;   /* 2-row engines: 0 = pair launches if this engine may hold the device's pairing slot (ssrhip_lm_create), 1 = never,
                          2 = always (tests of the give-up path: no slot taken, no guard) */
  float* x;        /* [B][D] residual stream */
  float* q;        /* [B][D] */
  float* h;        /* [B][max(d_ffn, K*Hh)] */
  float* logits;   /* [B][K][card] */
  float* part_o;   /* [B][H][max_splits][hd] */
  float* part_ml;  /* [B][H][max_splits][2] */
  int32_t* next_tok; int32_t* next_pos; int32_t* kv_pos; int32_t* row_len;
  ssrhip_kv kv;
  ssrhip_sampler_cfg* cfg; ssrhip_sampler_state* state;
  const float* noise; int32_t* generated; float* dbg_logits;
} ssrhip_lm_buffers;

typedef struct ssrhip_lm ssrhip_lm;     /* opaque host-side object (graph + launch descriptors) */

/* A 2-row engine (one utterance x CFG) runs its step with pair launches (ssrhip_gemv_pair) only while it holds the PAIRING SLOT of its
 * device: two pair chains on one GPU can starve each other of CUs (each launch spins until all 256 of its workgroups are resident).
 * The slot is taken here and given back by ssrhip_lm_destroy: at most one live engine per process and device (a table in the library)
 * and at most one process per device (an exclusive flock on /dev/shm/ssrhip_pair_<pci bus id>.lock, released by the kernel when the
 * process dies). An engine that does not get the slot — or finds a CU mask in the environment, fewer than 256 CUs, a pair kernel that
 * does not fit a CU, SSRHIP_GEMV_PAIR=0, pair_mode 1 — steps with the ordinary launches (same tokens, bit for bit) and says why once
 * on stderr; ssrhip_lm_pairing reports it. */
int ssrhip_lm_create(const ssrhip_lm_dims* d, const ssrhip_lm_weights* w, const ssrhip_lm_buffers* b, ssrhip_lm** out);
/* 1 = this engine's decode step uses pair launches, 0 = it does not; `why` (may be NULL) receives the reason as text */
int ssrhip_lm_pairing(const ssrhip_lm* lm, char* why, int32_t why_len);
void ssrhip_lm_destroy(ssrhip_lm* lm);
/* The opt-in bf16 weight stream of the <= 4-row decode step: packed bf16 copies (SSRHIP_W16_INDEX) of the six matrix families, device
 * pointers; the per-layer fields are HOST arrays of n_layer entries (copied by ssrhip_lm_set_w16). A NULL field (or a NULL entry of a
 * per-layer array) means that matrix streams its fp32 master. The masters in ssrhip_lm_weights must hold the rounded values (ssrhip_gemv_w16). */
typedef struct ssrhip_lm_w16 {
  const uint16_t* const* in_proj_w16; const uint16_t* const* out_proj_w16; const uint16_t* const* ffn1_w16; const uint16_t* const* ffn2_w16;
  const uint16_t* head1_w16; const uint16_t* head2_w16;
} ssrhip_lm_w16;
/* Hand the engine the packed copies: from now on every GEMV launch of its decode step whose family has one and whose shape qualifies
 * (ssrhip_gemv_w16) streams 2-byte weights; the others run ssrhip_gemv on the masters. Same tokens, bit for bit, as the same engine without
 * this call. To be called before the first decode step is enqueued or captured; refused (< 0) afterwards and for engines of more than 4
 * rows. The default pair launches read fp32 weights: an engine that holds its device's pairing slot gives it back and steps unpaired
 * (ssrhip_lm_pairing then reports 0 and names the bf16 stream) unless ssrhip_lm_set_w16_pair, below, opts in to the pair launches over the
 * packed copies. Prefill and scoring read the masters and are not affected. */
int ssrhip_lm_set_w16(ssrhip_lm* lm, const ssrhip_lm_w16* w16);
/* how many GEMV launches of the last enqueued (or captured) decode step ran a bf16-stream kernel (4 * n_layer + 2 when every family qualifies) */
int ssrhip_lm_w16_launches(const ssrhip_lm* lm);

/* Opt-in: pair launches over the bf16 weight stream (ssrhip_gemv_pair_w16). Accepted only on a 2-row engine that has ssrhip_lm_set_w16
 * set, before the step is captured (< 0 otherwise). on = 1 repeats ssrhip_lm_create's pairing decision for this engine: pair_mode 1
 * refuses, the step's own descriptors are put to ssrhip_gemv_pair_w16_applicable, the device's pairing slot is taken unless pair_mode is 2,
 * the workspace is allocated and zeroed. An engine that cannot pair returns 0 all the same and steps unpaired (ssrhip_lm_pairing says why);
 * one that can reports ssrhip_lm_pairing = 1 with a text that names the bf16 pair launches. A pair whose two matrices do not both have
 * packed copies runs as two single launches. on = 0 gives slot and workspace back. Same tokens, bit for bit, either way. */
int ssrhip_lm_set_w16_pair(ssrhip_lm* lm, int on);
/* pair launches of the last enqueued step that ran a w16_pair* kernel (2 * n_layer when every family has a packed copy; ssrhip_lm_w16_launches
 * keeps counting the SINGLE bf16 launches: then 2, layer 0's QKV and the second head Linear where it has a copy); 0 for other engines */
int ssrhip_lm_w16_pair_launches(const ssrhip_lm* lm);

/* The opt-in e4m3 weight stream of the <= 4-row decode step: packed codes (SSRHIP_W8_INDEX) and per-row scales of the six matrix
 * families, device pointers; the per-layer fields are HOST arrays of n_layer entries (copied by ssrhip_lm_set_w8). Codes and scales of a
 * family come together; a NULL pair means that family streams its fp32 master. The masters in ssrhip_lm_weights must hold code * scale
 * (ssrhip_gemv_w8). Twelve pointers; the record has no index in ssrhip_sizeof, its size comes back through ssrhip_lm_w8_sizeof. */
typedef struct ssrhip_lm_w8 {
  const uint8_t* const* in_proj_w8; const uint8_t* const* out_proj_w8; const uint8_t* const* ffn1_w8; const uint8_t* const* ffn2_w8;
  const float* const* in_proj_s; const float* const* out_proj_s; const float* const* ffn1_s; const float* const* ffn2_s;
  const uint8_t* head1_w8; const uint8_t* head2_w8;
  const float* head1_s; const float* head2_s;
} ssrhip_lm_w8;
int ssrhip_lm_w8_sizeof(void);
/* Hand the engine the packed codes and scales: from now on every GEMV launch of its decode step whose family has them and whose shape
 * qualifies (ssrhip_gemv_w8) streams 1-byte weights; the others run ssrhip_gemv on the masters. Same tokens, bit for bit, as the same engine
 * without this call. To be called before the first decode step is enqueued or captured; refused (< 0) afterwards, for engines of more than
 * 4 rows (5..16 rows have ssrhip_lm_set_wt8), where another packed stream is already set (ssrhip_lm_set_w16 and its kin, and the reverse), and for a family with codes but no
 * scales. The default pair launches read fp32 weights: the engine gives its device's pairing slot back and steps unpaired (ssrhip_lm_pairing
 * then reports 0 and names the e4m3 stream) unless ssrhip_lm_set_w8_pair, below, opts in to the pair launches over the codes. Prefill and
 * scoring read the masters and are not affected. */
int ssrhip_lm_set_w8(ssrhip_lm* lm, const ssrhip_lm_w8* w8);
/* how many GEMV launches of the last enqueued (or captured) decode step ran a kernel of csrc/gemv_w8.hip (4 * n_layer + 2 when every family
 * qualifies); a counter of its own: the bf16 streams' counters stay 0 for these engines */
int ssrhip_lm_w8_launches(const ssrhip_lm* lm);
/* Opt-in: pair launches over the e4m3 weight stream (ssrhip_gemv_pair_w8); ssrhip_lm_set_w16_pair's twin. Accepted only on a 2-row engine
 * that has ssrhip_lm_set_w8 set, before the step is captured (< 0 otherwise). on = 1 repeats ssrhip_lm_create's pairing decision for this
 * engine: pair_mode 1 refuses, the step's own descriptors are put to ssrhip_gemv_pair_w8_applicable, the device's pairing slot is taken
 * unless pair_mode is 2, the workspace is allocated and zeroed. An engine that cannot pair returns 0 all the same and steps unpaired
 * (ssrhip_lm_pairing says why); one that can reports ssrhip_lm_pairing = 1 with a text that names the e4m3 pair launches. A pair whose two
 * matrices do not both have codes and scales runs as two single launches. on = 0 gives slot and workspace back (the state
 * ssrhip_lm_set_w8 left). Same tokens, bit for bit, either way. */
int ssrhip_lm_set_w8_pair(ssrhip_lm* lm, int on);
/* pair launches of the last enqueued step that ran a w8_pair* kernel (2 * n_layer when every family has codes; ssrhip_lm_w8_launches keeps
 * counting the SINGLE e4m3 launches: then 2, layer 0's QKV and the second head Linear); 0 for other engines */
int ssrhip_lm_w8_pair_launches(const ssrhip_lm* lm);
/* Opt-in: pair launches for the 4-ROW step over the fp32 weights (ssrhip_gemv_pair4). Accepted only on a 4-row engine that streams no
 * packed weights, before the step is captured (< 0 otherwise). on = 1 repeats ssrhip_lm_create's pairing decision for this engine: pair_mode
 * 1 refuses, the step's own descriptors are put to ssrhip_gemv_pair4_applicable, the device's pairing slot is taken unless pair_mode is 2,
 * the workspace (SSRHIP_PAIR4_WS_BYTES) is allocated and zeroed. An engine that cannot pair returns 0 all the same and steps unpaired
 * (ssrhip_lm_pairing says why); one that can reports ssrhip_lm_pairing = 1 with a text that names the 4-row pair launches. on = 0 gives
 * slot and workspace back. Same tokens, bit for bit, either way. ssrhip_lm_pair_status covers this workspace too. */
int ssrhip_lm_set_pair4(ssrhip_lm* lm, int on);
/* pair launches of the last enqueued step that ran a pair4* kernel (2 * n_layer when both forms apply); 0 for other engines */
int ssrhip_lm_pair4_launches(const ssrhip_lm* lm);
/* Opt-in: pair launches for the 4-ROW step over the engine's PACKED stream (ssrhip_gemv_pair4_w16 / ssrhip_gemv_pair4_w8). Accepted only on
 * a 4-row engine that has ssrhip_lm_set_w16 or ssrhip_lm_set_w8 set, before the step is captured (< 0 otherwise). on = 1 repeats
 * ssrhip_lm_create's pairing decision for this engine: pair_mode 1 refuses, the step's own descriptors are put to the kind's _applicable,
 * the device's pairing slot is taken unless pair_mode is 2, the workspace (SSRHIP_PAIR4_WS_BYTES) is allocated and zeroed. An engine that
 * cannot pair returns 0 all the same and steps unpaired (ssrhip_lm_pairing says why); one that can reports ssrhip_lm_pairing = 1 with a
 * text that names the form. A pair whose two matrices do not both have packed copies runs as two single launches. on = 0 gives slot and
 * workspace back (the state the stream's setter left). Same tokens, bit for bit, either way. ssrhip_lm_pair_status covers this workspace too. */
int ssrhip_lm_set_pair4_pk(ssrhip_lm* lm, int on);
/* pair launches of the last enqueued step that ran a kernel of csrc/gemv_pair4_pk.hip (2 * n_layer when every family has packed copies;
 * the stream's own counter keeps counting the SINGLE packed launches: then 2); 0 for other engines */
int ssrhip_lm_pair4_pk_launches(const ssrhip_lm* lm);
/* The same for the 5..16-row decode step: the record's pointers are SSRHIP_WT16_INDEX copies of the six families (NULL field / NULL entry:
 * that family streams the fp32 streaming-order copy of its master). From now on every GEMV launch of the step tries ssrhip_gemv_wt16 first
 * and falls back to ssrhip_gemv; same tokens, bit for bit; the step stays one captured graph. Refused (< 0) for engines of <= 4 rows (they
 * have ssrhip_lm_set_w16), of more than 16 rows, engines already captured and engines created without the fp32 streaming-order copies. */
int ssrhip_lm_set_wt16(ssrhip_lm* lm, const ssrhip_lm_w16* wt16);
/* how many GEMV launches of the last enqueued (or captured) decode step ran a kernel of csrc/gemv_mfma_w16.hip (4 * n_layer + 2 when every
 * family qualifies); a counter of its own: ssrhip_lm_w16_launches stays 0 for these engines */
int ssrhip_lm_wt16_launches(const ssrhip_lm* lm);
/* The same for the 17..32-row decode step: the record is the one ssrhip_lm_set_wt16 takes (SSRHIP_WT16_INDEX copies; NULL = that family
 * streams its fp32 streaming-order copy). Every GEMV launch of the step tries ssrhip_gemv_wt32 first and falls back to ssrhip_gemv; same
 * tokens, bit for bit; the step stays one captured graph. Refused (< 0) for engines of <= 16 rows (the error names their setter), engines
 * already captured and engines created without the fp32 streaming-order copies. */
int ssrhip_lm_set_wt32(ssrhip_lm* lm, const ssrhip_lm_w16* wt16);
/* how many GEMV launches of the last enqueued (or captured) decode step ran a kernel of csrc/gemv_mfma32_w16.hip (4 * n_layer + 2 when
 * every family qualifies); the other two counters stay 0 for these engines */
int ssrhip_lm_wt32_launches(const ssrhip_lm* lm);
/* The e4m3 weight stream of the 5..16-row decode step: the record is the one ssrhip_lm_set_w8 takes, with the codes in SSRHIP_WT8_INDEX
 * order (scales unchanged; a NULL pair = that family streams the fp32 streaming-order copy of its master). Every GEMV launch of the step
 * tries ssrhip_gemv_wt8 first and falls back to ssrhip_gemv; same tokens, bit for bit; the step stays one captured graph. Refused (< 0) for
 * engines of <= 4 rows (the error names ssrhip_lm_set_w8) and of more than 16 rows, engines already captured, engines created without the
 * fp32 streaming-order copies, engines that already have another packed stream, and for a family with codes but no scales. */
int ssrhip_lm_set_wt8(ssrhip_lm* lm, const ssrhip_lm_w8* wt8);
/* how many GEMV launches of the last enqueued (or captured) decode step ran a kernel of csrc/gemv_mfma_w8.hip (4 * n_layer + 2 when every
 * family qualifies); a counter of its own: every other stream's counter stays 0 for these engines */
int ssrhip_lm_wt8_launches(const ssrhip_lm* lm);
/* on != 0: the *_ws buffers of this engine's ssrhip_lm_weights hold ONE bf16 plane [N][K] each (a bf16 arena: the weight itself) instead
 * of three; ssrhip_lm_prefill then multiplies through ssrhip_gemm_w1 (and, where that answers 1, through the fp32 chain on the masters).
 * Same KV cache and x as with the three planes of the same weights, bit for bit. The count is the CALLER's statement about its buffers
 * and comes from nowhere else (no environment variable is read). Refused (< 0) for an engine created without planes and for one whose
 * decode step is already captured. */
int ssrhip_lm_set_prefill_w1(ssrhip_lm* lm, int32_t on);
/* on != 0: the pool of this engine's ssrhip_lm_buffers.kv holds 2-byte (bf16) entries, same layout and element count — the CALLER's
 * statement about its buffer. The decode step then appends with SSRHIP_EPI_QKV_APPEND16 and always takes the fused walk
 * (ssrhip_attn_rows_kv16, also at 5..11 rows x 16 heads; SSRHIP_ATTN_SPLIT is ignored); ssrhip_lm_prefill scatters with
 * ssrhip_kv_scatter16 and attends with ssrhip_attn_prefill_kv16, and a prefill that cannot take the tiled attention (no seq_start,
 * SSRHIP_PREFILL_ATTN_ROWWISE) is an error. So every attention of the engine sees bf16-valued K/V, whichever path wrote them.
 * Refused (< 0) for engines of <= 4 rows, of more than 256 pages per row, and engines whose decode step is already captured. */
int ssrhip_lm_set_kv16(ssrhip_lm* lm, int32_t on);
/* how many attention launches of the last enqueued (or captured) decode step ran ssrhip_attn_rows_kv16 — or, at <= 4 rows,
 * ssrhip_attn_decode_kv16 (n_layer for an engine with a 2-byte cache, else 0) */
int ssrhip_lm_kv16_launches(const ssrhip_lm* lm);
/* logp != NULL: the decode step of this engine ends in ssrhip_sample_logp with this DEVICE buffer [n_utt][max_steps][K] of the caller's
 * (n_utt and max_steps as its sampler reads them), at every row count; NULL: back to ssrhip_sample. Opt-in: an engine that never calls
 * this runs the step it ran before. Refused (< 0) once the decode step is captured. */
int ssrhip_lm_set_logprobs(ssrhip_lm* lm, float* logp);
/* 1: the step of this engine writes per-token log-probabilities (ssrhip_lm_set_logprobs), 0: it does not */
int ssrhip_lm_logprobs(const ssrhip_lm* lm);
/* The same statement for engines of 1, 2 or 4 rows (opt-in, DESIGN.md Part I.23): the pool of ssrhip_lm_buffers.kv holds 2-byte entries,
 * and the caller hands over three DEVICE buffers it owns and has filled ONCE:
 *   land        [B][1][2][n_head][SSRHIP_PAGE][head_dim] fp32 — a one-layer cache of B pages in the pool's layout (contents: anything);
 *   land_table  [B] int32, land_table[b] = b;
 *   land_pos    [n_layer][B] int32, land_pos[l * B + b] = l.
 * The QKV launch of layer l keeps SSRHIP_EPI_QKV_APPEND — no GEMV or pair kernel knows of this — with a descriptor that names the landing
 * cache: kv = {land, land_table, max_pages 1, n_layer 1, n_head, head_dim}, layer 0, kv_pos = land_pos + l * B, so layer l's K / V of row b
 * land at position l of page b. The attention launch is ssrhip_attn_decode_kv16, which rounds them once and promotes them into the pool.
 * ssrhip_lm_prefill scatters with ssrhip_kv_scatter16 and attends with ssrhip_attn_prefill_kv16 (tiled only, as for ssrhip_lm_set_kv16).
 * Nothing changes between steps, so the captured step replays. NULL, NULL, NULL: off. Refused (< 0) for engines of more than 4 rows
 * (they take ssrhip_lm_set_kv16), of more than SSRHIP_PAGE layers, with SSRHIP_PREFILL_ATTN_ROWWISE set, after the step is captured, and
 * for one pointer without the others. */
int ssrhip_lm_set_kv16_small(ssrhip_lm* lm, float* land, const int32_t* land_table, const int32_t* land_pos);
/* Prompt sharing (opt-in, 5..32-row fp32-cache engines, at most 256 pages per row): two DEVICE arrays of B ints the caller owns and
 * rewrites between steps (see ssrhip_attn_rows_group), or NULL, NULL for off. Call it before the first ssrhip_lm_decode (the captured step
 * keeps the pointers). With it set every layer's attention of the decode step is ssrhip_attn_rows_group (also at 5..11 rows x 16 heads,
 * where the unshared step takes the split kernels; SSRHIP_ATTN_SPLIT is ignored) — the rule ssrhip_lm_set_kv16 uses. The prefill is
 * untouched: the caller prefills the rows it wants and aliases the others' table entries. */
int ssrhip_lm_set_prompt_groups(ssrhip_lm* lm, const int32_t* chunk_head, const int32_t* n_shared);
/* The chunk size the caller cuts its chunks for (2, 4 or 8): every grouped attention launch of this engine's step is built for it, whatever
 * SSRHIP_ATTN_GROUP_MEMBERS says when a step is enqueued or captured. Without this call it is ssrhip_attn_group_members() at the time of
 * ssrhip_lm_set_prompt_groups. Refused after capture. ssrhip_lm_group_members reads it back (0 = the engine does not share). */
int ssrhip_lm_set_group_members(ssrhip_lm* lm, int32_t members);
int ssrhip_lm_group_members(const ssrhip_lm* lm);
/* how many attention launches of the last enqueued (or captured) decode step ran ssrhip_attn_rows_group (n_layer with groups set, else 0) */
int ssrhip_lm_group_launches(const ssrhip_lm* lm);
/* enqueue `n_steps` decode steps (graph replays when use_graph!=0) */
int ssrhip_lm_decode(ssrhip_lm* lm, int32_t n_steps, int32_t use_graph, ssrhip_stream_t stream);
/* prefill R rows ([text || audio] of every sequence, flattened): fills the cache for all layers.
 * ws: workspace floats: x[R][D], xn[R][D], qkv[R][3D], o[R][D], h[R][d_ffn], part_o, part_ml sized for R. */
typedef struct ssrhip_prefill_args {
  const int32_t* tok; const int32_t* pos; const int32_t* kind;   /* embed inputs, [R].. */
  const int32_t* row_seq; const int32_t* row_pos; const int32_t* row_len; /* cache coordinates, [R] */
  int32_t R, max_splits;
  float* x; float* xn; float* qkv; float* o; float* h; float* part_o; float* part_ml;
  /* optional (NULL/0 = per-row attention through part_o / part_ml): the rows of sequence s are seq_start[s] .. seq_start[s+1]-1,
   * in position order -> the tiled prefill attention (ssrhip_attn_prefill); part_o / part_ml may then be NULL */
  const int32_t* seq_start; int32_t n_seq, max_len;
  /* two-phase admission (continuous batching: a new utterance is prefilled on a SIDE stream while the graph keeps stepping the live rows):
   * `table` != NULL replaces the engine's page table for THIS prefill (same layout) — the rows being filled are still parked on the
   * scratch page in the table the decode step reads; `no_embed` != 0 skips the closing embedding of the rows' pending tokens into the
   * residual stream (it is live decode state): the caller issues ssrhip_lm_embed_pending on the decode stream when it activates the rows. */
  const int32_t* table; int32_t no_embed, reserved_;
} ssrhip_prefill_args;
int ssrhip_lm_prefill(ssrhip_lm* lm, const ssrhip_prefill_args* p, ssrhip_stream_t stream);
/* x[b] = embedding of row b's pending input token (next_tok / next_pos) for EVERY row of the engine — the closing step of ssrhip_lm_prefill
 * on its own (rows in mid-decode get exactly what the sampler's fused embedding left there: same function, same inputs). */
int ssrhip_lm_embed_pending(ssrhip_lm* lm, ssrhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Teacher-forced scoring (the numbers of the reference's training forward, models/ssr.py:280-379, without autograd):
 * the same flattened [text || audio] rows as a prefill, the same layer loop (one internal function serves both entries), then the
 * final LayerNorm of the SCORED rows only, the prediction heads and cross entropy / rank per codebook. Needs no decode engine.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ssrhip_score_args {
  /* prefill rows, exactly as in ssrhip_prefill_args: device arrays [R]; seq_start [n_seq + 1] (device), rows of a sequence contiguous and in
   * position order (the tiled prefill attention) */
  const int32_t* tok; const int32_t* pos; const int32_t* kind;
  const int32_t* row_seq; const int32_t* row_pos; const int32_t* row_len;
  const int32_t* seq_start;
  int32_t R, n_seq, max_len;
  float* x; float* xn; float* qkv; float* o; float* h;   /* workspaces [R][D], [R][D], [R][3D], [R][D], [R][d_ffn] */
  /* scratch KV pool: kv.n_layer must be 1 (every layer writes and reads layer 0 of the pool: stream order makes the reuse safe);
   * kv.table [n_seq][kv.max_pages] */
  ssrhip_kv kv;
  /* scored rows, HOST arrays [n_seq]: sequence s scores its rows score_first[s] .. score_first[s] + score_count[s] - 1 (absolute row
   * indices into the R rows); M = sum of score_count. Scored row m (in that order) predicts target[k * M + m] of codebook k. */
  const int32_t* score_first; const int32_t* score_count;
  int32_t M;
  const int32_t* target;   /* device [K][M], 0 <= target < card */
  float* nll;              /* device [K][M]: -log softmax(logits)[target] */
  int32_t* rank;           /* device [K][M]: classes whose logit is STRICTLY greater than the target's (ssrhip_xent_rank) */
  float* hs;               /* workspace [M][D]: final-LayerNorm output of the scored rows (may alias xn) */
  float* head_h;           /* workspace [head_chunk][K * head_hidden] */
  float* logits;           /* workspace [head_chunk][ldc], ldc = card rounded up to a multiple of 4 */
  int32_t head_chunk;      /* rows per head pass (bounds the logits buffer) */
  /* optional (both or none; NULL = the fp32 chain): three bf16 planes (ssrhip_split_weights) of head1_w as one [3][K*Hh][D] and of each
   * codebook's head2_w[k] separately, [K][3][card][Hh]. Used under the prefill's rule (not with SSRHIP_PREFILL_SPLIT=0). */
  const uint16_t* head1_ws; const uint16_t* head2_ws;
} ssrhip_score_args;
/* Writes nll / rank of every scored row and codebook. Layer GEMMs use the ssrhip_lm_weights split planes when present (same rule as
 * ssrhip_lm_prefill). The workspaces, the scratch pool and the output belong to the caller. */
int ssrhip_lm_score(const ssrhip_lm_dims* d, const ssrhip_lm_weights* w, const ssrhip_score_args* a, ssrhip_stream_t stream);
/* ssrhip_lm_score for ONE-plane buffers (ssrhip_gemm_w1): every *_ws of `w` is one bf16 plane [N][K], head1_ws one [K*Hh][D], head2_ws
 * [K][card][Hh]. Same nll / rank as ssrhip_lm_score on the three planes of the same bf16-valued weights, bit for bit. */
int ssrhip_lm_score_w1(const ssrhip_lm_dims* d, const ssrhip_lm_weights* w, const ssrhip_score_args* a, ssrhip_stream_t stream);
/* Cross entropy and rank of M rows of logits [M][ld] (one codebook) against target [M]: one wave64 per row, one pass with an online max and
 * rescaled fp32 exp-sum. nll[m] = logsumexp(row) - row[target]; rank[m] = #{c != target : row[c] > row[target]} (top-10 hit = rank < 10;
 * exact ties at the 10th place count as hits, where torch.topk's order is arbitrary). ld % 4 == 0, card <= ld. */
int ssrhip_xent_rank(const float* logits, int32_t ld, int32_t card, const int32_t* target, int32_t M, float* nll, int32_t* rank,
                     ssrhip_stream_t stream);
/* 0 = fine, 1 = a paired GEMV launch of this engine's decode step gave up waiting (ssrhip_gemv_pair): every token since the last call
 * that returned 0 is invalid and so are the KV cache and the residual stream of the rows in flight; reported ONCE (the workspace is
 * re-zeroed: after a new prefill the engine decodes correctly again). Synchronises `stream`. Engines that do not pair always return 0
 * without touching the stream. */
int ssrhip_lm_pair_status(ssrhip_lm* lm, ssrhip_stream_t stream);

/* Test hook (tests/test_gpu_lm.py: the pair launches' give-up path): `n_wg` workgroups that each hold `lds_bytes` of LDS (<= 160 KB) and
 * spin for `ms` milliseconds of the constant 100 MHz clock — a foreign kernel that keeps CUs away from everybody else. `started` (may be
 * NULL): an int32 the device can reach (pinned host memory), incremented once by every workgroup when it has become resident, so that the
 * caller can wait for all of them before it starts what the squatters are meant to starve. */
int ssrhip_debug_occupy(int32_t n_wg, int32_t lds_bytes, float ms, int32_t* started, ssrhip_stream_t stream);

/* run `n_steps` eager decode steps with a hipEvent pair around EVERY kernel launch (bench.py roofline).
 * out_us[i] = average microseconds of launch slot i of a step, out_kind[i] = 0 gemv | 1 attention | 2 sampler;
 * returns the number of slots (<= n_out) or a negative error. */
int ssrhip_lm_time_steps(ssrhip_lm* lm, int32_t n_steps, ssrhip_stream_t stream, float* out_us, int32_t* out_kind, int32_t n_out);

/* Launch duration of ONE kernel category inside a decode step, measured the way the product runs it: the launches of
 * `category` (0 gemv | 1 attention | 2 sampler) of one step are captured into a hipGraph (the others are left out), the
 * graph is replayed `n_replays` times between one hipEvent pair on `stream`, and the elapsed time is divided by the number
 * of launches. No per-launch event overhead, so the figure agrees with rocprofv3's kernel durations (+ the ~0.1 us
 * in-graph gap). The decode state is NOT advanced and the hidden-state buffers are left with garbage: call
 * ssrhip_lm_prefill (DecodeEngine.start) again before decoding. */
int ssrhip_lm_time_category(ssrhip_lm* lm, int32_t category, int32_t n_replays, ssrhip_stream_t stream, float* out_us_per_launch,
                            int32_t* out_launches_per_step);

#ifdef __cplusplus
}
#endif
#endif /* SSRHIP_H */
