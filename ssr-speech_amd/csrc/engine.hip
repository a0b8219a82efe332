// engine.hip — host side of the decode engine: launch descriptors for one decode step, hipGraph
// capture/replay, prefill orchestration, per-kernel event timing. No device allocation here: all
// buffers belong to the caller (torch tensors), the engine owns only the graph objects and a private
// capture stream.
//
// One decode step = embed -> n_layer x [LN1+QKV GEMV(+KV append) -> paged attention (split-KV partials)
// -> combine+out-proj GEMV(+residual) -> LN2+FFN1 GEMV(+ReLU) -> FFN2 GEMV(+residual)]
// -> final-LN + 4 head MLP-1 GEMV(+GELU) -> grouped head MLP-2 GEMV -> sampler/state machine.
// The step touches no host state, so the captured graph replays unchanged for every step
// (positions, tokens, stop flags all live in device memory).
// Replaces the per-iteration body of SSR_Speech.inference (models/ssr.py:671-770).
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <errno.h>
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>
#include <mutex>
#include <vector>
#include "common.h"

static thread_local char g_err[512] = "";
void ssrhip_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* ssrhip_last_error(void) { return g_err; }
extern "C" int ssrhip_version(void) { return SSRHIP_VERSION; }
extern "C" int ssrhip_sizeof(int which) {
  switch (which) {
    case 0: return sizeof(ssrhip_kv);
    case 1: return sizeof(ssrhip_gemv_args);
    case 2: return sizeof(ssrhip_attn_args);
    case 3: return sizeof(ssrhip_embed_args);
    case 4: return sizeof(ssrhip_sampler_cfg);
    case 5: return sizeof(ssrhip_sampler_state);
    case 6: return sizeof(ssrhip_sample_args);
    case 7: return sizeof(ssrhip_gemm_args);
    case 8: return sizeof(ssrhip_lm_weights);
    case 9: return sizeof(ssrhip_lm_dims);
    case 10: return sizeof(ssrhip_lm_buffers);
    case 11: return sizeof(ssrhip_prefill_args);
    case 12: return sizeof(ssrhip_lstm_args);
    case 13: return sizeof(ssrhip_resblock_args);
    case 14: return sizeof(ssrhip_score_args);
    case 15: return sizeof(ssrhip_lm_w16);
    default: return -1;
  }
}

struct ssrhip_lm {
  ssrhip_lm_dims d;
  ssrhip_lm_weights w;
  ssrhip_lm_buffers b;
  std::vector<const float*> ptrs[16];
  std::vector<const uint16_t*> sptrs[4];
  bool prefill_split = false;   // bf16 planes present and SSRHIP_PREFILL_SPLIT != 0
  bool prefill_w1 = false;      // ... and they hold ONE plane each (ssrhip_lm_set_prefill_w1: the caller's statement about its buffers)
  hipStream_t cap_stream = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  void* pair_ws = nullptr;      // granules of the paired GEMV launches (2-row step; SSRHIP_PAIR_WS_BYTES, owned)
  int pair_dev = -1;            // >= 0: this engine holds the pairing slot of that device (released in ssrhip_lm_destroy)
  char pair_why[200] = "";      // why the step pairs / does not pair (ssrhip_lm_pairing)
  bool pk_pair = false;         // the pair launches of this engine stream its packed weights: the bf16 copies (ssrhip_lm_set_w16_pair; pk_kind ==
                                // PK_W16) or the e4m3 codes and scales (ssrhip_lm_set_w8_pair; PK_W8)
  bool pair4 = false;           // 4-row engine: the step runs the 4-row pair launches (ssrhip_lm_set_pair4; pair_ws then has SSRHIP_PAIR4_WS_BYTES)
  int pair4_launches = 0;       // pair launches of the last enqueued step that ran a pair4* kernel (ssrhip_lm_pair4_launches)
  bool pair4_pk = false;        // 4-row engine with a packed stream (pk_kind PK_W16 / PK_W8): the step runs the 4-row pair launches over it
                                // (ssrhip_lm_set_pair4_pk; pair_ws then has SSRHIP_PAIR4_WS_BYTES)
  int pair4_pk_launches = 0;    // pair launches of the last enqueued step that ran a kernel of gemv_pair4_pk.hip (ssrhip_lm_pair4_pk_launches)
  int pk_pair_launches = 0;     // pair launches of the last enqueued step that ran a w16_pair* / w8_pair* kernel (ssrhip_lm_{w16,w8}_pair_launches)
  // the bf16 weight stream: an engine has one row count, so one kind (index into PACKED_STREAMS, -1: none) and one record of packed copies
  // of the six families, in that kind's order (SSRHIP_W16_INDEX at <= 4 rows, SSRHIP_WT16_INDEX at 5..32); NULL = that matrix streams fp32
  int pk_kind = -1;
  std::vector<const uint16_t*> pk[4];       // in_proj, out_proj, ffn1, ffn2 per layer (empty: none)
  const uint16_t* pk_head1 = nullptr;
  const uint16_t* pk_head2 = nullptr;
  int pk_launches = 0;          // launches of the last enqueued step that ran a kernel of pk_kind (ssrhip_lm_{w16,wt16,wt32,w8,wt8}_launches)
  // the e4m3 weight streams (pk_kind == PK_W8, <= 4 rows: codes in SSRHIP_W8_INDEX order; PK_WT8, 5..16 rows: SSRHIP_WT8_INDEX order) and,
  // travelling next to the codes, the per-row scales
  std::vector<const uint8_t*> pk8[4];
  std::vector<const float*> pk8s[4];
  const uint8_t* pk8_head1 = nullptr; const uint8_t* pk8_head2 = nullptr;
  const float* pk8s_head1 = nullptr; const float* pk8s_head2 = nullptr;
  bool kv16 = false;            // b.kv.pool holds 2-byte entries (ssrhip_lm_set_kv16: the caller's statement about its buffer)
  int kv16_launches = 0;        // attention launches of the last enqueued step that read 2-byte entries: ssrhip_attn_rows_kv16, or
                                // ssrhip_attn_decode_kv16 at <= 4 rows (ssrhip_lm_kv16_launches)
  // the bf16 cache of the <= 4-row step (ssrhip_lm_set_kv16_small: the caller's statement about its buffers; all null = off): b.kv.pool holds
  // 2-byte entries, the QKV launch appends fp32 into the landing cache and the attention launch promotes from there
  float* land = nullptr;                 // [B][1][2][n_head][SSRHIP_PAGE][head_dim] fp32: layer l at position l of row b's page
  const int32_t* land_table = nullptr;   // [B]: land_table[b] = b
  const int32_t* land_pos = nullptr;     // [n_layer][B]: land_pos[l * B + b] = l
  const int32_t* chunk_head = nullptr;   // prompt sharing (ssrhip_lm_set_prompt_groups): the caller's two device arrays [B], or null = off
  const int32_t* n_shared = nullptr;
  int group_members = 0;        // rows per chunk the caller's chunks are cut for (ssrhip_lm_set_group_members; set with the arrays)
  int group_launches = 0;       // attention launches of the last enqueued step that ran ssrhip_attn_rows_group (ssrhip_lm_group_launches)
  float* logp = nullptr;        // the step ends in ssrhip_sample_logp with this buffer of the caller's (ssrhip_lm_set_logprobs; null = off)
};

namespace {

// The three bf16 weight streams, one per row range: the setter's name, its rows (as numbers and as its messages spell them), what its
// refusal of more rows says, the packed GEMV entry point, whether the engine needs the fp32 streaming-order copies (ssrhip_lm_weights
// *_wt) and whether taking the record gives the pairing slot back (the pair launches stream fp32 weights).
struct PackedStream {
  const char* setter; int lo, hi; const char* rows; const char* only;
  int (*gemv)(const ssrhip_gemv_args*, const uint16_t*, ssrhip_stream_t);
  bool needs_wt, unpairs;
};
const PackedStream PACKED_STREAMS[3] = {
    {"ssrhip_lm_set_w16", 1, 4, "<= 4", "the bf16 weight stream exists for the <= 4-row decode step only", ssrhip_gemv_w16, false, true},
    {"ssrhip_lm_set_wt16", 5, 16, "5..16", "the bf16 weight stream of the matrix-core step exists for 5..16 rows only", ssrhip_gemv_wt16, true, false},
    {"ssrhip_lm_set_wt32", 17, 32, "17..32", "the bf16 weight stream of the two-panel step exists for 17..32 rows only", ssrhip_gemv_wt32, true, false},
};
enum { PK_PAIR4 = -2 };   // not a packed stream: StepShapes::pair_plan's name for the 4-row pair launches over fp32 weights
enum { PK_PAIR4_W16 = -3, PK_PAIR4_W8 = -4 };   // ... and for the 4-row pair launches over the packed bf16 copies / the e4m3 codes
enum { PK_W16 = 0, PK_WT16 = 1, PK_WT32 = 2, PK_W8 = 3, PK_WT8 = 4 };   // PK_W8 / PK_WT8: the e4m3 streams of <= 4 rows (ssrhip_lm_set_w8) and of
                                                            // 5..16 rows (ssrhip_lm_set_wt8): codes AND scales, so their entry points have
                                                            // another signature and they have no row in PACKED_STREAMS
inline bool pk_codes(int kind) { return kind == PK_W8 || kind == PK_WT8; }
// what a launch of one family streams instead of its fp32 master: a 2-byte copy (the bf16 kinds) or codes + scales (PK_W8); all NULL = nothing
struct PackedRef { const uint16_t* w16; const uint8_t* w8; const float* sc; };

enum { CAT_GEMV = 0, CAT_ATTN = 1, CAT_SAMPLE = 2 };

// ---- the pairing slot: ONE chain of pair launches per device (include/ssrhip.h ssrhip_lm_create). A pair launch spins until its 256
// workgroups are resident together; two such chains at once (two engines on two streams, two processes) can each hold half the CUs and
// wait for the other half — bounded (~1 s), flagged, but garbage. So the right to pair is a resource: a per-process table (one live
// engine per device) plus an exclusive flock on a file named after the GPU's PCI address (one process per device; the kernel drops the
// lock when the process dies, however it dies).
constexpr int PAIR_MAX_DEV = 64;
std::mutex g_pair_mu;
struct PairSlot { int live = 0; int fd = -1; };
PairSlot g_pair_slot[PAIR_MAX_DEV];

// true: slot taken (give it back with pair_slot_release); false: `why` says who has it / what went wrong
bool pair_slot_acquire(int dev, char* why, size_t why_len) {
  std::lock_guard<std::mutex> lk(g_pair_mu);
  if (dev < 0 || dev >= PAIR_MAX_DEV) { snprintf(why, why_len, "device index %d outside the pairing table", dev); return false; }
  PairSlot& sl = g_pair_slot[dev];
  if (sl.live > 0) { snprintf(why, why_len, "another decode engine of this process already runs pair launches on device %d", dev); return false; }
  char bus[64] = "";
  if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), dev) != hipSuccess || !bus[0]) snprintf(bus, sizeof(bus), "dev%d", dev);
  for (char* c = bus; *c; ++c) if (*c == ':' || *c == '/' || *c == '.') *c = '_';
  const char* dirs[2] = {"/dev/shm", "/tmp"};
  int fd = -1;
  char path[160] = "";
  for (int i = 0; i < 2 && fd < 0; ++i) {
    snprintf(path, sizeof(path), "%s/ssrhip_pair_%s.lock", dirs[i], bus);
    fd = open(path, O_RDWR | O_CREAT | O_CLOEXEC, 0666);
    if (fd >= 0) fchmod(fd, 0666);                                  // the next user's process must be able to open it too (umask)
    else fd = open(path, O_RDONLY | O_CLOEXEC);                     // someone else's file: a shared descriptor is enough for flock
  }
  if (fd < 0) { snprintf(why, why_len, "cannot create the pair-launch lock file (%s: %s)", path, strerror(errno)); return false; }
  if (flock(fd, LOCK_EX | LOCK_NB) != 0) {
    snprintf(why, why_len, "another process holds the pair-launch lock of this GPU (%s)", path);
    close(fd);
    return false;
  }
  sl.fd = fd;
  sl.live = 1;
  return true;
}

void pair_slot_release(int dev) {
  std::lock_guard<std::mutex> lk(g_pair_mu);
  if (dev < 0 || dev >= PAIR_MAX_DEV) return;
  PairSlot& sl = g_pair_slot[dev];
  if (sl.live > 0) sl.live = 0;
  if (sl.fd >= 0) { flock(sl.fd, LOCK_UN); close(sl.fd); sl.fd = -1; }
}

// give pairing back: the workspace, the device's slot and both "this engine's step pairs its ..." flags (a caller that pairs again sets its own)
void lm_unpair(ssrhip_lm* lm) {
  if (lm->pair_ws) { hipFree(lm->pair_ws); lm->pair_ws = nullptr; }
  if (lm->pair_dev >= 0) { pair_slot_release(lm->pair_dev); lm->pair_dev = -1; }
  lm->pk_pair = lm->pair4 = lm->pair4_pk = false;
}

// What differs between the pairing decisions of ssrhip_lm_create (fp32, 2 rows), ssrhip_lm_set_w16_pair / ssrhip_lm_set_w8_pair,
// ssrhip_lm_set_pair4 and ssrhip_lm_set_pair4_pk: whom StepShapes::pair_plan asks, the workspace, where the refusal is read and the texts.
struct PairSpec {
  int kind; size_t ws_bytes;      // pair_plan's packed_kind (-1: the fp32 forms of 2 rows); SSRHIP_PAIR_WS_BYTES or SSRHIP_PAIR4_WS_BYTES
  const char* (*why)();           // the refusal of the kind's _applicable ...
  const char* no_reason;          // ... and what is said when it left none (null: the empty text stands)
  const char* who;                // the entry point an allocation failure names
  const char* slot_taken;         // the stderr line when another chain holds the device's slot (%s: who holds it)
  const char* forced; const char* holds;   // pair_why of an engine that pairs: pair_mode 2 / with the slot
};
const PairSpec PAIRSPEC_FP32 = {-1, SSRHIP_PAIR_WS_BYTES, ssrhip_gemv_pair_why, nullptr, "ssrhip_lm_create",
                                "ssrhip: this 2-row decode engine steps WITHOUT pair launches (same tokens, ~5 %% slower): %s\n",
                                "forced on by the caller (pair_mode 2: no slot, no guard)", "this engine holds the pairing slot of its device"};
const PairSpec PAIRSPEC_W16 = {PK_W16, SSRHIP_PAIR_WS_BYTES, ssrhip_gemv_pair_w16_why, nullptr, "ssrhip_lm_set_w16_pair",
                               "ssrhip: this 2-row decode engine steps WITHOUT bf16 pair launches (same tokens): %s\n",
                               "bf16 pair launches (ssrhip_gemv_pair_w16), forced on by the caller (pair_mode 2: no slot, no guard)",
                               "bf16 pair launches (ssrhip_gemv_pair_w16): this engine holds the pairing slot of its device"};
const PairSpec PAIRSPEC_W8 = {PK_W8, SSRHIP_PAIR_WS_BYTES, ssrhip_gemv_pair_w8_why, nullptr, "ssrhip_lm_set_w8_pair",
                              "ssrhip: this 2-row decode engine steps WITHOUT e4m3 pair launches (same tokens): %s\n",
                              "e4m3 pair launches (ssrhip_gemv_pair_w8), forced on by the caller (pair_mode 2: no slot, no guard)",
                              "e4m3 pair launches (ssrhip_gemv_pair_w8): this engine holds the pairing slot of its device"};
const PairSpec PAIRSPEC_PAIR4 = {PK_PAIR4, SSRHIP_PAIR4_WS_BYTES, ssrhip_gemv_pair4_why, "fewer than two launches of the step qualify for the 4-row pair forms",
                                 "ssrhip_lm_set_pair4", "ssrhip: this 4-row decode engine steps WITHOUT its 4-row pair launches (same tokens): %s\n",
                                 "4-row pair launches (ssrhip_gemv_pair4), forced on by the caller (pair_mode 2: no slot, no guard)",
                                 "4-row pair launches (ssrhip_gemv_pair4): this engine holds the pairing slot of its device"};
const PairSpec PAIRSPEC_PAIR4_W16 = {PK_PAIR4_W16, SSRHIP_PAIR4_WS_BYTES, ssrhip_gemv_pair4_w16_why, "fewer than two launches of the step qualify for the 4-row bf16 pair forms",
                                     "ssrhip_lm_set_pair4_pk", "ssrhip: this 4-row decode engine steps WITHOUT its 4-row bf16 pair launches (same tokens): %s\n",
                                     "4-row bf16 pair launches (ssrhip_gemv_pair4_w16), forced on by the caller (pair_mode 2: no slot, no guard)",
                                     "4-row bf16 pair launches (ssrhip_gemv_pair4_w16): this engine holds the pairing slot of its device"};
const PairSpec PAIRSPEC_PAIR4_W8 = {PK_PAIR4_W8, SSRHIP_PAIR4_WS_BYTES, ssrhip_gemv_pair4_w8_why, "fewer than two launches of the step qualify for the 4-row e4m3 pair forms",
                                    "ssrhip_lm_set_pair4_pk", "ssrhip: this 4-row decode engine steps WITHOUT its 4-row e4m3 pair launches (same tokens): %s\n",
                                    "4-row e4m3 pair launches (ssrhip_gemv_pair4_w8), forced on by the caller (pair_mode 2: no slot, no guard)",
                                    "4-row e4m3 pair launches (ssrhip_gemv_pair4_w8): this engine holds the pairing slot of its device"};

__global__ void occupy_kernel(long long ticks, int lds_floats, int* started) {
  extern __shared__ float occ[];
  for (int i = threadIdx.x; i < lds_floats; i += blockDim.x) occ[i] = (float)i;
  __syncthreads();
  if (started && threadIdx.x == 0) __hip_atomic_fetch_add(started, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // "this workgroup is resident"
  const long long t0 = wall_clock64();
  float acc = 0.f;
  while (wall_clock64() - t0 < ticks) { acc += occ[(threadIdx.x * 7) % (lds_floats > 0 ? lds_floats : 1)]; __builtin_amdgcn_s_sleep(32); }
  if (acc == -1.f) occ[0] = acc;
}

bool getenv_flag(const char* name) {      // tuning / A-B knobs, read once per process
  const char* e = getenv(name);
  return e && e[0] && e[0] != '0';
}

struct Timer {   // optional per-launch event timing: one accumulator per launch slot of a step
  bool on = false;
  hipStream_t s = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int slot = 0;
  int only = -1;          // >= 0: enqueue only launches of this category (graph-chained category timing)
  int n_enq = 0;
  std::vector<float> ms;
  std::vector<int> kind;
};

#define STEP_CALL(cat, call)                                    \
  do {                                                          \
    if (tm && tm->only >= 0 && tm->only != (cat)) break;        \
    if (tm) tm->n_enq += 1;                                     \
    if (tm && tm->on) hipEventRecord(tm->e0, tm->s);            \
    int _rc = (call);                                           \
    if (_rc) return _rc;                                        \
    if (tm && tm->on) {                                         \
      hipEventRecord(tm->e1, tm->s);                            \
      hipEventSynchronize(tm->e1);                              \
      float _ms = 0.f;                                          \
      hipEventElapsedTime(&_ms, tm->e0, tm->e1);                \
      if ((int)tm->ms.size() <= tm->slot) { tm->ms.push_back(0.f); tm->kind.push_back(cat); } \
      tm->ms[tm->slot] += _ms;                                  \
      tm->slot += 1;                                            \
    }                                                           \
  } while (0)

// The embedding launch of R rows into `out`: tables and sizes. The caller adds where the tokens come from (tok / pos / kind).
ssrhip_embed_args embed_args(const ssrhip_lm_dims& d, const ssrhip_lm_weights& w, int R, float* out, int out_tiled) {
  ssrhip_embed_args ea;
  memset(&ea, 0, sizeof(ea));
  ea.text_emb = w.text_emb; ea.audio_emb = w.audio_emb; ea.pe = w.pe;
  ea.alpha_text = w.alpha_text; ea.alpha_audio = w.alpha_audio;
  ea.R = R; ea.D = d.d_model; ea.K = d.n_codebooks; ea.card = d.card; ea.out = out; ea.out_tiled = out_tiled;
  return ea;
}

// Launch descriptors of a decode step: every launch enqueue_step makes is built here, and ssrhip_lm_create's "would this engine pair?"
// asks with the same descriptors the step later hands to ssrhip_gemv_pair
struct StepShapes {
  const ssrhip_lm_dims& d;
  const ssrhip_lm_weights& w;
  const ssrhip_lm_buffers& b;
  const int D, B, K, Hh;
  // 5..32 rows: the residual stream x, the combined attention output and the hidden h live in the 16-column tiled layout
  // (include/ssrhip.h SSRHIP_TILED_P: one 16-row panel per 16 rows) so that the matrix-core GEMV's operand loads are contiguous KiBs
  const int tiled;
  const bool wt;       // streaming-order weight copies for the matrix-core GEMV (include/ssrhip.h w_tiled)
  const bool kv16;     // the cache holds 2-byte entries and the QKV launch appends them (ssrhip_lm_set_kv16, 5..32 rows)
  float* const land;   // <= 4 rows with a 2-byte cache (ssrhip_lm_set_kv16_small): the QKV launch appends fp32 into this landing cache
  const int32_t* const land_table;
  const int32_t* const land_pos;
  explicit StepShapes(const ssrhip_lm* lm)
      : d(lm->d), w(lm->w), b(lm->b), D(lm->d.d_model), B(lm->b.B), K(lm->d.n_codebooks), Hh(lm->d.head_hidden), tiled(lm->b.B > 4 ? 1 : 0),
        wt(lm->b.B > 4 && lm->w.in_proj_wt), kv16(lm->kv16), land(lm->land), land_table(lm->land_table), land_pos(lm->land_pos) {}
  ssrhip_gemv_args qkv_args(int l) const {
    ssrhip_gemv_args g;
    // LN1 + packed QKV projection, q -> b.q, k/v appended in place into the paged cache
    memset(&g, 0, sizeof(g));
    g.W = w.in_proj_w[l]; g.bias = w.in_proj_b[l]; g.x = b.x; g.y = b.q;
    g.B = B; g.N = 3 * D; g.K = D; g.groups = 1; g.x_stride = D; g.y_stride = D;
    g.pro = SSRHIP_PRO_LAYERNORM; g.act = SSRHIP_ACT_NONE; g.epi = kv16 ? SSRHIP_EPI_QKV_APPEND16 : SSRHIP_EPI_QKV_APPEND;
    if (!d.ln_folded) { g.ln_w = w.ln1_w[l]; g.ln_b = w.ln1_b[l]; }
    g.ln_eps = 1e-5f;
    g.kv = b.kv; g.layer = l; g.kv_pos = b.kv_pos;
    if (land) {
      // the landing cache is a one-layer cache of B pages in the pool's layout whose row b owns page b; layer l appends at position l of it.
      // Every append form computes its address from (kv, layer, kv_pos) alone, so the launch — single, segment or pair, any weight
      // stream — is the fp32 engine's with another destination
      g.kv.pool = land; g.kv.table = land_table; g.kv.max_pages = 1; g.kv.n_layer = 1;
      g.layer = 0; g.kv_pos = land_pos + (size_t)l * B;
    }
    g.x_tiled = tiled;                         // q stays row-major for the attention kernel
    if (wt) { g.W = w.in_proj_wt[l]; g.w_tiled = 1; }
    return g;
  }
  ssrhip_gemv_args head1_args() const {
    ssrhip_gemv_args g;
    // final LayerNorm + first Linear of the K prediction heads (stacked) + GELU
    memset(&g, 0, sizeof(g));
    g.W = w.head1_w; g.bias = w.head1_b; g.x = b.x; g.y = b.h;
    g.B = B; g.N = K * Hh; g.K = D; g.groups = 1; g.x_stride = D; g.y_stride = K * Hh;
    g.pro = SSRHIP_PRO_LAYERNORM; g.act = SSRHIP_ACT_GELU_ERF; g.epi = SSRHIP_EPI_STORE;
    if (!d.ln_folded) { g.ln_w = w.lnf_w; g.ln_b = w.lnf_b; }
    g.ln_eps = 1e-5f;
    g.x_tiled = tiled; g.y_tiled = tiled;
    if (wt) { g.W = w.head1_wt; g.w_tiled = 1; }
    return g;
  }
  ssrhip_gemv_args outproj_args(int l) const {               // the <= 4-row form: split-KV merge prologue + out-proj + residual
    ssrhip_gemv_args g;
    memset(&g, 0, sizeof(g));
    g.W = w.out_proj_w[l]; g.bias = w.out_proj_b[l]; g.x = nullptr; g.y = b.x;
    g.B = B; g.N = D; g.K = D; g.groups = 1; g.x_stride = D; g.y_stride = D;
    g.pro = SSRHIP_PRO_ATTN_COMBINE; g.act = SSRHIP_ACT_NONE; g.epi = SSRHIP_EPI_RESIDUAL;
    g.part_o = b.part_o; g.part_ml = b.part_ml; g.max_splits = b.max_splits; g.row_len = b.row_len;
    g.kv = b.kv;
    return g;
  }
  // 5..32 rows: the attention output is already combined (in `attn_out`, tiled), so the out-projection is a plain GEMV + residual
  ssrhip_gemv_args outproj_rows_args(int l, const float* attn_out) const {
    ssrhip_gemv_args g = outproj_args(l);
    g.x = attn_out;
    g.pro = SSRHIP_PRO_NONE; g.x_tiled = 1; g.y_tiled = 1;
    if (wt) { g.W = w.out_proj_wt[l]; g.w_tiled = 1; }
    return g;
  }
  ssrhip_gemv_args ffn1_args(int l) const {
    ssrhip_gemv_args g;
    // LN2 + FFN1 + ReLU
    memset(&g, 0, sizeof(g));
    g.W = w.ffn1_w[l]; g.bias = w.ffn1_b[l]; g.x = b.x; g.y = b.h;
    g.B = B; g.N = d.d_ffn; g.K = D; g.groups = 1; g.x_stride = D; g.y_stride = d.d_ffn;
    g.pro = SSRHIP_PRO_LAYERNORM; g.act = SSRHIP_ACT_RELU; g.epi = SSRHIP_EPI_STORE;
    if (!d.ln_folded) { g.ln_w = w.ln2_w[l]; g.ln_b = w.ln2_b[l]; }
    g.ln_eps = 1e-5f;
    g.x_tiled = tiled; g.y_tiled = tiled;
    if (wt) { g.W = w.ffn1_wt[l]; g.w_tiled = 1; }
    return g;
  }
  ssrhip_gemv_args ffn2_args(int l) const {
    ssrhip_gemv_args g;
    memset(&g, 0, sizeof(g));
    g.W = w.ffn2_w[l]; g.bias = w.ffn2_b[l]; g.x = b.h; g.y = b.x;
    g.B = B; g.N = D; g.K = d.d_ffn; g.groups = 1; g.x_stride = d.d_ffn; g.y_stride = D;
    g.pro = SSRHIP_PRO_NONE; g.act = SSRHIP_ACT_NONE; g.epi = SSRHIP_EPI_RESIDUAL;
    g.x_tiled = tiled; g.y_tiled = tiled;
    if (wt) { g.W = w.ffn2_wt[l]; g.w_tiled = 1; }
    return g;
  }
  ssrhip_gemv_args head2_args() const {
    ssrhip_gemv_args g;
    // second Linear of each head: K groups
    memset(&g, 0, sizeof(g));
    g.W = w.head2_w; g.bias = w.head2_b; g.x = b.h; g.y = b.logits;
    g.B = B; g.N = d.card; g.K = Hh; g.groups = K; g.x_stride = K * Hh; g.y_stride = K * d.card;
    g.pro = SSRHIP_PRO_NONE; g.act = SSRHIP_ACT_NONE; g.epi = SSRHIP_EPI_STORE;
    g.x_tiled = tiled;                         // logits stay row-major for the sampler
    if (wt) { g.W = w.head2_wt; g.w_tiled = 1; }
    return g;
  }
  ssrhip_attn_args attn_args(int l) const {
    ssrhip_attn_args at;
    memset(&at, 0, sizeof(at));
    at.q = b.q; at.kv = b.kv; at.layer = l; at.row_seq = nullptr; at.row_len = b.row_len;
    at.R = B; at.max_splits = b.max_splits; at.scale = 1.0f / sqrtf((float)(D / d.n_head));
    at.part_o = b.part_o; at.part_ml = b.part_ml;
    return at;
  }
  ssrhip_sample_args sample_args() const {
    ssrhip_sample_args sa;
    memset(&sa, 0, sizeof(sa));
    sa.logits = b.logits; sa.n_utt = b.n_utt; sa.K = K; sa.card = d.card;
    sa.cfg = b.cfg; sa.state = b.state; sa.noise = b.noise; sa.generated = b.generated;
    sa.next_tok = b.next_tok; sa.next_pos = b.next_pos; sa.kv_pos = b.kv_pos; sa.row_len = b.row_len;
    sa.dbg_logits = b.dbg_logits;
    // the sampler also embeds the tokens it chose: x of the next step (no separate embed launch)
    sa.embed = embed_args(d, w, B, b.x, tiled);
    return sa;
  }
  // which launches of the 2-row step qualify for the pair forms, and how many pair launches a step then has (0: fewer than 2 -> none)
  // packed_kind PK_W16 / PK_W8: the question goes to the pair launches over packed bf16 weights / e4m3 codes (ssrhip_gemv_pair_w16_applicable,
  // ssrhip_gemv_pair_w8_applicable), -1: to the fp32 forms; which of a step's pairs then have packed copies of both matrices is
  // enqueue_step's part. PK_PAIR4: the 4-row step, the question goes to ssrhip_gemv_pair4_applicable (fp32 weights); PK_PAIR4_W16 /
  // PK_PAIR4_W8: the 4-row step over a packed stream (ssrhip_gemv_pair4_w16_applicable, ssrhip_gemv_pair4_w8_applicable)
  int pair_plan(bool* qkv, bool* head, bool* ffn1, int packed_kind = -1) const {
    *qkv = *head = *ffn1 = false;
    const bool four = packed_kind == PK_PAIR4 || packed_kind == PK_PAIR4_W16 || packed_kind == PK_PAIR4_W8;
    if (B != (four ? 4 : 2)) return 0;
    int (*const applicable)(const ssrhip_gemv_args*, const ssrhip_gemv_args*) =
        packed_kind == PK_PAIR4 ? ssrhip_gemv_pair4_applicable : packed_kind == PK_PAIR4_W16 ? ssrhip_gemv_pair4_w16_applicable : packed_kind == PK_PAIR4_W8 ? ssrhip_gemv_pair4_w8_applicable
        : packed_kind == PK_W16 ? ssrhip_gemv_pair_w16_applicable : packed_kind == PK_W8 ? ssrhip_gemv_pair_w8_applicable : ssrhip_gemv_pair_applicable;
    const ssrhip_gemv_args fa = ffn2_args(0);
    if (d.n_layer > 1) { const ssrhip_gemv_args qa = qkv_args(1); *qkv = applicable(&fa, &qa) != 0; }
    { const ssrhip_gemv_args ha = head1_args(); *head = applicable(&fa, &ha) != 0; }
    { const ssrhip_gemv_args oa = outproj_args(0), f1 = ffn1_args(0); *ffn1 = applicable(&oa, &f1) != 0; }
    const int n = (*qkv ? d.n_layer - 1 : 0) + (*head ? 1 : 0) + (*ffn1 ? d.n_layer : 0);
    if (n < 2) { *qkv = *head = *ffn1 = false; return 0; }
    return n;
  }
};

int enqueue_step(ssrhip_lm* lm, hipStream_t s, Timer* tm) {
  const StepShapes sh(lm);
  const ssrhip_lm_dims& d = lm->d;
  const ssrhip_lm_buffers& b = lm->b;
  // 2-row step: FFN2 of layer l and the launch that consumes its output (QKV of layer l + 1; the head MLP after the last layer) run as ONE
  // launch with the all-to-all edge inside it (csrc/gemv.hip gemv_pair_kernel), and so do the out-projection (with its split-KV merge
  // prologue) and FFN1 (gemv_pair_merge_kernel): attention, pair, pair per layer. The pairs of a step use the three granule buffers of
  // lm->pair_ws cyclically: pair i uses buffer i % 3 and resets the buffer of pair (i + 1) % n — closed over the step, so that graph
  // replays (and eager steps) always find their buffer reset by the launch before them; with n % 3 == 1 the last pair takes buffer 1.
  // An engine that pairs its packed stream (ssrhip_lm_set_w16_pair, ssrhip_lm_set_w8_pair) hands the same pairs to the packed entry of its
  // kind, ssrhip_gemv_pair_w16 or ssrhip_gemv_pair_w8 — those whose TWO matrices have packed copies; a pair that lacks one runs as two
  // single launches. n_pairs is the count actually launched: the buffer cycle closes over exactly these. A 4-row engine that pairs its
  // packed stream (ssrhip_lm_set_pair4_pk) does the same with ssrhip_gemv_pair4_w16 / ssrhip_gemv_pair4_w8.
  enum { W16_IN = 0, W16_OUT = 1, W16_FFN1 = 2, W16_FFN2 = 3 };
  const bool wp = (lm->pk_pair || lm->pair4_pk) && lm->pair_ws && (lm->pk_kind == PK_W16 || lm->pk_kind == PK_W8);
  const bool wp8 = wp && lm->pk_kind == PK_W8;
  const bool wp4 = wp && lm->pair4_pk;          // ... at 4 rows (ssrhip_lm_set_pair4_pk): the same rule for a pair that lacks a packed copy
  bool pair_qkv = false, pair_head = false, pair_ffn1 = false;
  const bool p4 = lm->pair4 && lm->pair_ws;     // the 4-row step's pair launches (ssrhip_lm_set_pair4): same plan, same cycle, ssrhip_gemv_pair4
  int n_pairs = lm->pair_ws ? sh.pair_plan(&pair_qkv, &pair_head, &pair_ffn1, p4 ? PK_PAIR4 : wp4 ? (wp8 ? PK_PAIR4_W8 : PK_PAIR4_W16) : wp ? lm->pk_kind : -1) : 0;
  // what a launch of (family, layer) streams instead of its fp32 master, in the engine's kind
  auto w16_of = [&](int family, int l) -> PackedRef {
    if (pk_codes(lm->pk_kind)) return lm->pk8[family].empty() ? PackedRef{nullptr, nullptr, nullptr} : PackedRef{nullptr, lm->pk8[family][l], lm->pk8s[family][l]};
    return PackedRef{lm->pk[family].empty() ? nullptr : lm->pk[family][l], nullptr, nullptr};
  };
  const PackedRef pk_h1 = {lm->pk_head1, lm->pk8_head1, lm->pk8s_head1}, pk_h2 = {lm->pk_head2, lm->pk8_head2, lm->pk8s_head2};
  auto packed = [&](const PackedRef r) { return r.w16 || r.w8; };
  auto ffn1_pairs = [&](int l) { return pair_ffn1 && (!wp || (packed(w16_of(W16_OUT, l)) && packed(w16_of(W16_FFN1, l)))); };
  auto ffn2_pairs = [&](int l) {
    const bool last = l == d.n_layer - 1;
    if (!(last ? pair_head : pair_qkv)) return false;
    return !wp || (packed(w16_of(W16_FFN2, l)) && packed(last ? pk_h1 : w16_of(W16_IN, l + 1)));
  };
  if (wp) {
    n_pairs = 0;
    for (int l = 0; l < d.n_layer; ++l) n_pairs += (ffn1_pairs(l) ? 1 : 0) + (ffn2_pairs(l) ? 1 : 0);
    if (n_pairs < 2) { pair_qkv = pair_head = pair_ffn1 = false; n_pairs = 0; }
  }
  int pair_i = 0, n_wp = 0, n_p4 = 0, n_p4pk = 0;
  // the launch (a, b) that pair_plan found applicable, on this pair's granule buffer; pa / pb: the packed copies (wp only)
  auto pair_call = [&](const ssrhip_gemv_args& ga, const ssrhip_gemv_args& gb, const PackedRef pa, const PackedRef pb) {
    const int bufi = ssrhip_pair_buffer(pair_i, n_pairs), bufn = ssrhip_pair_buffer((pair_i + 1) % n_pairs, n_pairs);
    pair_i += 1;
    if (wp4) {
      const int rc = wp8 ? ssrhip_gemv_pair4_w8(&ga, &gb, pa.w8, pa.sc, pb.w8, pb.sc, lm->pair_ws, bufi, bufn, (ssrhip_stream_t)s)
                         : ssrhip_gemv_pair4_w16(&ga, &gb, pa.w16, pb.w16, lm->pair_ws, bufi, bufn, (ssrhip_stream_t)s);
      n_p4pk += rc == 0;
      if (rc == 1) ssrhip_set_error("ssrhip_lm_decode: a pair the plan accepted was refused by %s (%s)", wp8 ? "ssrhip_gemv_pair4_w8" : "ssrhip_gemv_pair4_w16",
                                    wp8 ? ssrhip_gemv_pair4_w8_why() : ssrhip_gemv_pair4_w16_why());
      return rc == 1 ? -1 : rc;
    }
    if (wp) {
      const int rc = wp8 ? ssrhip_gemv_pair_w8(&ga, &gb, pa.w8, pa.sc, pb.w8, pb.sc, lm->pair_ws, bufi, bufn, (ssrhip_stream_t)s)
                         : ssrhip_gemv_pair_w16(&ga, &gb, pa.w16, pb.w16, lm->pair_ws, bufi, bufn, (ssrhip_stream_t)s);
      n_wp += rc == 0;
      if (rc == 1) ssrhip_set_error("ssrhip_lm_decode: a pair the plan accepted was refused by %s (%s)", wp8 ? "ssrhip_gemv_pair_w8" : "ssrhip_gemv_pair_w16",
                                    wp8 ? ssrhip_gemv_pair_w8_why() : ssrhip_gemv_pair_w16_why());
      return rc == 1 ? -1 : rc;
    }
    if (p4) {
      const int rc = ssrhip_gemv_pair4(&ga, &gb, lm->pair_ws, bufi, bufn, (ssrhip_stream_t)s);
      n_p4 += rc == 0;
      if (rc == 1) ssrhip_set_error("ssrhip_lm_decode: a pair the plan accepted was refused by ssrhip_gemv_pair4 (%s)", ssrhip_gemv_pair4_why());
      return rc == 1 ? -1 : rc;
    }
    return ssrhip_gemv_pair(&ga, &gb, lm->pair_ws, bufi, bufn, (ssrhip_stream_t)s);
  };
  // Every single GEMV launch of the step goes through here: the packed bf16 copy of the matrix when the engine has one and the shape
  // qualifies (the packed entry point of the engine's kind answers 1 without launching when it does not), the fp32 weights otherwise.
  // Same bits either way.
  int n_pk = 0;
  auto gemv_call = [&](const ssrhip_gemv_args& ga, const PackedRef pk) -> int {
    if (pk.w16 || pk.w8) {
      const int rc = !pk.w8                   ? PACKED_STREAMS[lm->pk_kind].gemv(&ga, pk.w16, (ssrhip_stream_t)s)
                     : lm->pk_kind == PK_WT8 ? ssrhip_gemv_wt8(&ga, pk.w8, pk.sc, (ssrhip_stream_t)s)      // 5..16 rows (B > 4: it answers 1 otherwise)
                                             : ssrhip_gemv_w8(&ga, pk.w8, pk.sc, (ssrhip_stream_t)s);
      if (rc <= 0) { n_pk += rc == 0; return rc; }
    }
    return ssrhip_gemv(&ga, s);
  };
  bool qkv_done = false;                        // this layer's QKV already ran inside the previous layer's pair launch
  // 5..32 rows with enough (row, head) pairs to give every CU one: the fused walk over the pages (no partials, no merge
  // launch); its output goes to b.h (free until FFN1 of this layer) because q is still being read by other workgroups
  // a bf16 KV cache (ssrhip_lm_set_kv16 checked the rows and the pages) always takes the fused walk: the split kernels read fp32 entries
  // prompt groups (ssrhip_lm_set_prompt_groups checked the same things) take the grouped form of the fused walk, by the same rule
  const bool grouped = lm->chunk_head != nullptr;
  const bool fused_attn = lm->kv16 || grouped || (sh.B > 4 && sh.B * d.n_head >= 192 && b.kv.max_pages <= 256 && !getenv_flag("SSRHIP_ATTN_SPLIT"));   // 256 pages: the kernel's page-id registers
  int n_kv16 = 0, n_group = 0;

  if (tm) tm->slot = 0;

  for (int l = 0; l < d.n_layer; ++l) {
    if (!qkv_done) {
      const ssrhip_gemv_args g = sh.qkv_args(l);
      STEP_CALL(CAT_GEMV, gemv_call(g, w16_of(W16_IN, l)));
    }
    qkv_done = false;

    ssrhip_attn_args at = sh.attn_args(l);
    // 2-row paired step, OPT-IN experiment (SSRHIP_ATTN_PREFETCH=1, read when the step is enqueued): the attention launch pre-touches the
    // out-projection slice the merge pair launch behind it starts with (include/ssrhip.h ssrhip_attn_args.prefetch). Measured: the attention
    // launch pays for the 16.8 MB (6.55 -> 8.80 us) and the pair launch gains nothing (18.33 vs 18.35 us): 0.7477 -> 0.7707 ms/step
    // (profiles/r06_microbench/decode_ab_attn_prefetch.log). Like every cross-launch prefetch tried since round 1, it loses.
    if (pair_ffn1 && !p4 && sh.D % 256 == 0 && getenv("SSRHIP_ATTN_PREFETCH") && getenv("SSRHIP_ATTN_PREFETCH")[0] == '1') {
      at.prefetch = lm->w.out_proj_w[l];
      at.prefetch_floats = (sh.D / 256) * sh.D;              // workgroup i of the pair launch owns rows [8 i, 8 i + 8) of W_o [D][D]
    }
    // attention, then split-KV combine + out-proj + residual: <= 4 rows fuse the combine into the out-projection's prologue
    ssrhip_gemv_args op;
    if (fused_attn) {
      at.out_tiled = 1;
      if (lm->kv16) { STEP_CALL(CAT_ATTN, ssrhip_attn_rows_kv16(&at, b.h, s)); n_kv16 += 1; }
      else if (grouped) { STEP_CALL(CAT_ATTN, ssrhip_attn_rows_group_m(&at, lm->chunk_head, lm->n_shared, lm->group_members, b.h, s)); n_group += 1; }
      else STEP_CALL(CAT_ATTN, ssrhip_attn_rows(&at, b.h, s));
      op = sh.outproj_rows_args(l, b.h);
    } else {
      if (lm->land) { STEP_CALL(CAT_ATTN, ssrhip_attn_decode_kv16(&at, lm->land, s)); n_kv16 += 1; }   // <= 4 rows (the setter checked)
      else STEP_CALL(CAT_ATTN, ssrhip_attn_decode(&at, s));
      if (sh.B > 4) {
        // the combine is its own small launch; q is dead after the attention, reuse it
        at.out_tiled = 1;
        STEP_CALL(CAT_ATTN, ssrhip_attn_combine(&at, b.q, s));
        op = sh.outproj_rows_args(l, b.q);
      } else {
        op = sh.outproj_args(l);
      }
    }
    const ssrhip_gemv_args f1 = sh.ffn1_args(l);
    if (ffn1_pairs(l)) {                          // out-projection + FFN1 as one launch (2 rows)
      STEP_CALL(CAT_GEMV, pair_call(op, f1, w16_of(W16_OUT, l), w16_of(W16_FFN1, l)));
    } else {
      STEP_CALL(CAT_GEMV, gemv_call(op, w16_of(W16_OUT, l)));
      STEP_CALL(CAT_GEMV, gemv_call(f1, w16_of(W16_FFN1, l)));
    }

    // FFN2 + residual — paired with the next launch where that applies
    const ssrhip_gemv_args f2 = sh.ffn2_args(l);
    const bool last = l == d.n_layer - 1;
    if (ffn2_pairs(l)) {
      STEP_CALL(CAT_GEMV, pair_call(f2, last ? sh.head1_args() : sh.qkv_args(l + 1), w16_of(W16_FFN2, l), last ? pk_h1 : w16_of(W16_IN, l + 1)));
      qkv_done = true;                          // (after the last layer: the head MLP's first launch)
    } else {
      STEP_CALL(CAT_GEMV, gemv_call(f2, w16_of(W16_FFN2, l)));
    }
  }
  if (!qkv_done) {
    const ssrhip_gemv_args g = sh.head1_args();
    STEP_CALL(CAT_GEMV, gemv_call(g, pk_h1));
  }
  const ssrhip_gemv_args h2 = sh.head2_args();
  STEP_CALL(CAT_GEMV, gemv_call(h2, pk_h2));
  const ssrhip_sample_args sa = sh.sample_args();
  STEP_CALL(CAT_SAMPLE, lm->logp ? ssrhip_sample_logp(&sa, lm->logp, s) : ssrhip_sample(&sa, s));
  if (!tm || tm->only < 0) { lm->pk_launches = n_pk; lm->pk_pair_launches = n_wp; lm->pair4_launches = n_p4; lm->pair4_pk_launches = n_p4pk; lm->kv16_launches = n_kv16; lm->group_launches = n_group; }   // (a category-timing pass enqueues only part of a step)
  return 0;
}

// The pairing decision, once: may the step of this engine run pair launches of the spec's kind? Everything was given back before
// (lm_unpair, or a new engine). 1: it pairs — workspace allocated and zeroed (every tag invalid), the device's slot held unless pair_mode
// is 2 — and the caller sets the flag of its kind; 0: it does not, lm->pair_why says why; -1: the allocation failed (nothing is held).
int lm_take_pairing(ssrhip_lm* lm, const PairSpec& sp) {
  const int pair_mode = lm->b.pair_mode;
  if (pair_mode == 1) { snprintf(lm->pair_why, sizeof(lm->pair_why), "switched off by the caller (pair_mode 1)"); return 0; }
  // does the step pair at all (shapes, CU count, occupancy, CU mask, SSRHIP_GEMV_PAIR) ...
  bool pq, ph, pf;
  if (StepShapes(lm).pair_plan(&pq, &ph, &pf, sp.kind) == 0) {
    const char* why = sp.why();
    snprintf(lm->pair_why, sizeof(lm->pair_why), "%s", (why[0] || !sp.no_reason) ? why : sp.no_reason);
    return 0;
  }
  if (pair_mode != 2) {   // ... and may THIS engine do it? A refusal the user did not ask for: say it once on stderr
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    if (!pair_slot_acquire(dev, lm->pair_why, sizeof(lm->pair_why))) {
      fprintf(stderr, sp.slot_taken, lm->pair_why);
      return 0;
    }
    lm->pair_dev = dev;
  }
  if (hipMalloc(&lm->pair_ws, sp.ws_bytes) != hipSuccess || hipMemset(lm->pair_ws, 0, sp.ws_bytes) != hipSuccess) {
    lm_unpair(lm);
    ssrhip_set_error("%s: allocating the pair workspace failed", sp.who);
    return -1;
  }
  snprintf(lm->pair_why, sizeof(lm->pair_why), "%s", pair_mode == 2 ? sp.forced : sp.holds);
  return 1;
}

}  // namespace

extern "C" int ssrhip_lm_create(const ssrhip_lm_dims* d, const ssrhip_lm_weights* w, const ssrhip_lm_buffers* b, ssrhip_lm** out) {
  SSR_REQUIRE(d && w && b && out, "ssrhip_lm_create: null argument");
  SSR_REQUIRE(d->d_model % d->n_head == 0, "ssrhip_lm_create: d_model %% n_head != 0");
  const int hd = d->d_model / d->n_head;
  SSR_REQUIRE(hd == 64 || hd == 128, "ssrhip_lm_create: head_dim %d not in {64,128}", hd);
  SSR_REQUIRE(b->B == 1 || b->B == 2 || b->B == 4 || (b->B >= 5 && b->B <= 32), "ssrhip_lm_create: B=%d rows not in {1,2,4,5..32}", b->B);
  SSR_REQUIRE(b->B <= 4 || d->ln_folded, "ssrhip_lm_create: B > 4 rows needs LayerNorm gamma/beta folded into the weights (ln_folded)");
  SSR_REQUIRE(d->n_codebooks <= SSRHIP_MAX_CODEBOOKS, "ssrhip_lm_create: too many codebooks");
  // a row's text and audio positions are both below its sequence capacity: the sinusoidal table must cover it (embed reads pe[pos])
  SSR_REQUIRE((int64_t)b->kv.max_pages * SSRHIP_PAGE <= d->max_pos, "ssrhip_lm_create: sequence capacity %lld exceeds the position table (%d rows)",
              (long long)b->kv.max_pages * SSRHIP_PAGE, d->max_pos);
  ssrhip_lm* lm = new ssrhip_lm();
  lm->d = *d; lm->w = *w; lm->b = *b;
  // deep-copy the per-layer pointer arrays (the caller's ctypes arrays may be temporaries)
  const float* const** fields[12] = {&lm->w.ln1_w, &lm->w.ln1_b, &lm->w.in_proj_w, &lm->w.in_proj_b, &lm->w.out_proj_w, &lm->w.out_proj_b,
                                     &lm->w.ln2_w, &lm->w.ln2_b, &lm->w.ffn1_w, &lm->w.ffn1_b, &lm->w.ffn2_w, &lm->w.ffn2_b};
  for (int f = 0; f < 12; ++f) {
    const float* const* src = *fields[f];
    if (!src) { delete lm; ssrhip_set_error("ssrhip_lm_create: null per-layer pointer array %d", f); return -1; }
    lm->ptrs[f].assign(src, src + d->n_layer);
    *fields[f] = lm->ptrs[f].data();
  }
  // optional streaming-order copies (all or none)
  const float* const** opt[4] = {&lm->w.in_proj_wt, &lm->w.out_proj_wt, &lm->w.ffn1_wt, &lm->w.ffn2_wt};
  const bool has_wt = lm->w.in_proj_wt && lm->w.out_proj_wt && lm->w.ffn1_wt && lm->w.ffn2_wt && lm->w.head1_wt && lm->w.head2_wt;
  for (int f = 0; f < 4; ++f) {
    if (has_wt) {
      const float* const* src = *opt[f];
      lm->ptrs[12 + f].assign(src, src + d->n_layer);
      *opt[f] = lm->ptrs[12 + f].data();
    } else {
      *opt[f] = nullptr;
    }
  }
  if (!has_wt) lm->w.head1_wt = lm->w.head2_wt = nullptr;
  // optional bf16 planes for the prefill GEMMs (all four or none)
  const uint16_t* const** sp[4] = {&lm->w.in_proj_ws, &lm->w.out_proj_ws, &lm->w.ffn1_ws, &lm->w.ffn2_ws};
  const bool has_ws = lm->w.in_proj_ws && lm->w.out_proj_ws && lm->w.ffn1_ws && lm->w.ffn2_ws;
  for (int f = 0; f < 4; ++f) {
    if (has_ws) {
      const uint16_t* const* src = *sp[f];
      lm->sptrs[f].assign(src, src + d->n_layer);
      *sp[f] = lm->sptrs[f].data();
    } else {
      *sp[f] = nullptr;
    }
  }
  { const char* e = getenv("SSRHIP_PREFILL_SPLIT"); lm->prefill_split = has_ws && !(e && e[0] == '0'); }
  if (b->B != 2) {
    snprintf(lm->pair_why, sizeof(lm->pair_why), "pair launches exist for the 2-row step only (this engine has %d rows)", b->B);
  } else if (lm_take_pairing(lm, PAIRSPEC_FP32) < 0) {
    delete lm;
    return -1;
  }
  *out = lm;
  return 0;
}

extern "C" int ssrhip_lm_pairing(const ssrhip_lm* lm, char* why, int32_t why_len) {
  if (!lm) return 0;
  if (why && why_len > 0) snprintf(why, (size_t)why_len, "%s", lm->pair_why);
  return lm->pair_ws ? 1 : 0;
}

// The one body of the three setters: `kind`'s checks, then the record. Rows below the kind's range belong to another kind's setter.
static int lm_set_packed(ssrhip_lm* lm, const ssrhip_lm_w16* rec, int kind) {
  const PackedStream& ps = PACKED_STREAMS[kind];
  SSR_REQUIRE(lm && rec, "%s: null argument", ps.setter);
  const int B = lm->b.B;
  for (const PackedStream& o : PACKED_STREAMS)   // the kind that owns these rows
    SSR_REQUIRE(B >= ps.lo || B > o.hi, "%s: engines of %s rows stream bf16 weights through %s (this engine has %d rows)", ps.setter, o.rows, o.setter, B);
  SSR_REQUIRE(B <= ps.hi, "%s: %s (this engine has %d rows)", ps.setter, ps.only, B);
  SSR_REQUIRE(!lm->exec, "%s: the decode step of this engine is already captured (call it before the first ssrhip_lm_decode)", ps.setter);
  SSR_REQUIRE(!lm->pair4, "%s: this engine runs the 4-row pair launches over fp32 weights (ssrhip_lm_set_pair4); switch them off first", ps.setter);
  SSR_REQUIRE(!pk_codes(lm->pk_kind), "%s: this engine already streams e4m3 weights (%s); an engine has one packed stream", ps.setter,
              lm->pk_kind == PK_WT8 ? "ssrhip_lm_set_wt8" : "ssrhip_lm_set_w8");
  SSR_REQUIRE(!ps.needs_wt || lm->w.in_proj_wt, "%s: this engine was created without the fp32 streaming-order copies (ssrhip_lm_weights *_wt)", ps.setter);
  const uint16_t* const* src[4] = {rec->in_proj_w16, rec->out_proj_w16, rec->ffn1_w16, rec->ffn2_w16};
  for (int f = 0; f < 4; ++f) {
    if (src[f]) lm->pk[f].assign(src[f], src[f] + lm->d.n_layer);
    else lm->pk[f].clear();
  }
  lm->pk_head1 = rec->head1_w16;
  lm->pk_head2 = rec->head2_w16;
  lm->pk_kind = kind;
  if (ps.unpairs) {   // the default pair launches stream fp32 weights: this engine steps unpaired and gives the device's pairing slot back
                      // (ssrhip_lm_set_w16_pair may take it again for the pair launches over the packed copies)
    lm_unpair(lm);
    snprintf(lm->pair_why, sizeof(lm->pair_why), "this engine streams bf16 weights (%s): its pair launches are an opt-in (ssrhip_lm_set_w16_pair, 2 rows)", ps.setter);
  }
  return 0;
}
static int lm_packed_launches(const ssrhip_lm* lm, int kind) { return lm && lm->pk_kind == kind ? lm->pk_launches : 0; }

extern "C" int ssrhip_lm_w8_sizeof(void) { return (int)sizeof(ssrhip_lm_w8); }
// The e4m3 kinds: the checks of lm_set_packed for the kind's rows (PK_W8: <= 4, PK_WT8: 5..16), then codes and scales side by side.
static int lm_set_codes(ssrhip_lm* lm, const ssrhip_lm_w8* rec, int kind) {
  const char* who = kind == PK_WT8 ? "ssrhip_lm_set_wt8" : "ssrhip_lm_set_w8";
  SSR_REQUIRE(lm && rec, "%s: null argument", who);
  const int B = lm->b.B;
  if (kind == PK_W8) {
    SSR_REQUIRE(B <= 4, "ssrhip_lm_set_w8: the e4m3 weight stream exists for the <= 4-row decode step only (this engine has %d rows; engines of 5..16 rows take ssrhip_lm_set_wt8)", B);
  } else {
    SSR_REQUIRE(B > 4, "ssrhip_lm_set_wt8: engines of <= 4 rows stream e4m3 weights through ssrhip_lm_set_w8 (this engine has %d rows)", B);
    SSR_REQUIRE(B <= 16, "ssrhip_lm_set_wt8: the e4m3 weight stream of the matrix-core step exists for 5..16 rows only (this engine has %d rows; engines of 17..32 rows stream 2-byte copies through ssrhip_lm_set_wt32)", B);
  }
  SSR_REQUIRE(!lm->exec, "%s: the decode step of this engine is already captured (call it before the first ssrhip_lm_decode)", who);
  SSR_REQUIRE(!lm->pair4, "%s: this engine runs the 4-row pair launches over fp32 weights (ssrhip_lm_set_pair4); switch them off first", who);
  SSR_REQUIRE(lm->pk_kind < 0 || lm->pk_kind == kind, "%s: this engine already streams bf16 weights (%s); an engine has one packed stream", who,
              lm->pk_kind >= 0 && lm->pk_kind < PK_W8 ? PACKED_STREAMS[lm->pk_kind].setter : "");
  SSR_REQUIRE(kind != PK_WT8 || lm->w.in_proj_wt, "%s: this engine was created without the fp32 streaming-order copies (ssrhip_lm_weights *_wt)", who);
  const uint8_t* const* src[4] = {rec->in_proj_w8, rec->out_proj_w8, rec->ffn1_w8, rec->ffn2_w8};
  const float* const* scl[4] = {rec->in_proj_s, rec->out_proj_s, rec->ffn1_s, rec->ffn2_s};
  for (int f = 0; f < 4; ++f) SSR_REQUIRE(!src[f] == !scl[f], "%s: codes and scales of a family come together (family %d)", who, f);
  SSR_REQUIRE(!rec->head1_w8 == !rec->head1_s && !rec->head2_w8 == !rec->head2_s, "%s: codes and scales of a head matrix come together", who);
  for (int f = 0; f < 4; ++f) {
    if (src[f]) {
      for (int l = 0; l < lm->d.n_layer; ++l)
        SSR_REQUIRE(src[f][l] && scl[f][l], "%s: null codes or scales (family %d, layer %d)", who, f, l);
    }
  }
  for (int f = 0; f < 4; ++f) {
    if (src[f]) { lm->pk8[f].assign(src[f], src[f] + lm->d.n_layer); lm->pk8s[f].assign(scl[f], scl[f] + lm->d.n_layer); }
    else { lm->pk8[f].clear(); lm->pk8s[f].clear(); }
  }
  lm->pk8_head1 = rec->head1_w8; lm->pk8s_head1 = rec->head1_s;
  lm->pk8_head2 = rec->head2_w8; lm->pk8s_head2 = rec->head2_s;
  lm->pk_kind = kind;
  if (kind == PK_WT8) return 0;   // engines of more than 4 rows never pair
  // the default pair launches stream fp32 weights: this engine steps unpaired and gives the device's pairing slot back
  // (ssrhip_lm_set_w8_pair may take it again for the pair launches over the codes)
  lm_unpair(lm);
  snprintf(lm->pair_why, sizeof(lm->pair_why), "this engine streams e4m3 weights (ssrhip_lm_set_w8): its pair launches are an opt-in (ssrhip_lm_set_w8_pair, 2 rows)");
  return 0;
}
extern "C" int ssrhip_lm_set_w8(ssrhip_lm* lm, const ssrhip_lm_w8* rec) { return lm_set_codes(lm, rec, PK_W8); }
extern "C" int ssrhip_lm_set_wt8(ssrhip_lm* lm, const ssrhip_lm_w8* rec) { return lm_set_codes(lm, rec, PK_WT8); }
extern "C" int ssrhip_lm_wt8_launches(const ssrhip_lm* lm) { return lm_packed_launches(lm, PK_WT8); }
extern "C" int ssrhip_lm_w8_launches(const ssrhip_lm* lm) { return lm_packed_launches(lm, PK_W8); }

extern "C" int ssrhip_lm_set_w16(ssrhip_lm* lm, const ssrhip_lm_w16* w16) { return lm_set_packed(lm, w16, PK_W16); }
extern "C" int ssrhip_lm_set_wt16(ssrhip_lm* lm, const ssrhip_lm_w16* wt16) { return lm_set_packed(lm, wt16, PK_WT16); }
extern "C" int ssrhip_lm_set_wt32(ssrhip_lm* lm, const ssrhip_lm_w16* wt16) { return lm_set_packed(lm, wt16, PK_WT32); }
extern "C" int ssrhip_lm_set_prefill_w1(ssrhip_lm* lm, int32_t on) {
  SSR_REQUIRE(lm, "ssrhip_lm_set_prefill_w1: null engine");
  SSR_REQUIRE(!lm->exec, "ssrhip_lm_set_prefill_w1: the decode step of this engine is already captured (call it before the first ssrhip_lm_decode)");
  SSR_REQUIRE(!on || lm->w.in_proj_ws, "ssrhip_lm_set_prefill_w1: this engine was created without planes (ssrhip_lm_weights *_ws)");
  lm->prefill_w1 = on != 0;
  return 0;
}
extern "C" int ssrhip_lm_set_kv16(ssrhip_lm* lm, int32_t on) {
  SSR_REQUIRE(lm, "ssrhip_lm_set_kv16: null engine");
  SSR_REQUIRE(!lm->exec, "ssrhip_lm_set_kv16: the decode step of this engine is already captured (call it before the first ssrhip_lm_decode)");
  SSR_REQUIRE(!on || lm->b.B > 4, "ssrhip_lm_set_kv16: the bf16 KV cache exists for 5..32 rows only (this engine has %d rows)", lm->b.B);
  SSR_REQUIRE(!on || lm->b.kv.max_pages <= 256, "ssrhip_lm_set_kv16: the fused attention walk takes at most 256 pages per row (this engine has %d)", lm->b.kv.max_pages);
  SSR_REQUIRE(!on || !getenv_flag("SSRHIP_PREFILL_ATTN_ROWWISE"), "ssrhip_lm_set_kv16: SSRHIP_PREFILL_ATTN_ROWWISE is set, and the rowwise prefill attention reads fp32 entries");
  SSR_REQUIRE(!on || !lm->chunk_head, "ssrhip_lm_set_kv16: this engine shares prompts (ssrhip_lm_set_prompt_groups), and the grouped walk reads fp32 entries");
  lm->kv16 = on != 0;
  return 0;
}
extern "C" int ssrhip_lm_kv16_launches(const ssrhip_lm* lm) { return lm && (lm->kv16 || lm->land) ? lm->kv16_launches : 0; }
// The bf16 cache of the <= 4-row step: b.kv.pool holds 2-byte entries, and the three buffers are the landing cache of the QKV launch's
// append (StepShapes::qkv_args) that ssrhip_attn_decode_kv16 promotes from. All three null: off.
extern "C" int ssrhip_lm_set_kv16_small(ssrhip_lm* lm, float* land, const int32_t* land_table, const int32_t* land_pos) {
  SSR_REQUIRE(lm, "ssrhip_lm_set_kv16_small: null engine");
  SSR_REQUIRE(!lm->exec, "ssrhip_lm_set_kv16_small: the decode step of this engine is already captured (call it before the first ssrhip_lm_decode)");
  SSR_REQUIRE(!land == !land_table && !land == !land_pos, "ssrhip_lm_set_kv16_small: land, land_table and land_pos come together (all null = off)");
  const bool on = land != nullptr;
  SSR_REQUIRE(!on || lm->b.B <= 4, "ssrhip_lm_set_kv16_small: the landing cache exists for the <= 4-row decode step only (this engine has %d rows; engines of "
              "5..32 rows take ssrhip_lm_set_kv16)", lm->b.B);
  SSR_REQUIRE(!on || lm->d.n_layer <= SSRHIP_PAGE, "ssrhip_lm_set_kv16_small: layer l lands at position l of a row's landing page, which holds %d (this engine has %d layers)",
              SSRHIP_PAGE, lm->d.n_layer);
  SSR_REQUIRE(!on || !getenv_flag("SSRHIP_PREFILL_ATTN_ROWWISE"), "ssrhip_lm_set_kv16_small: SSRHIP_PREFILL_ATTN_ROWWISE is set, and the rowwise prefill attention reads fp32 entries");
  lm->land = land;
  lm->land_table = land_table;
  lm->land_pos = land_pos;
  return 0;
}

// Per-token log-probabilities (DESIGN.md Part I.27): with a buffer set, enqueue_step ends in ssrhip_sample_logp. Null: off.
extern "C" int ssrhip_lm_set_logprobs(ssrhip_lm* lm, float* logp) {
  SSR_REQUIRE(lm, "ssrhip_lm_set_logprobs: null engine");
  SSR_REQUIRE(!lm->exec, "ssrhip_lm_set_logprobs: the decode step of this engine is already captured (call it before the first ssrhip_lm_decode)");
  lm->logp = logp;
  return 0;
}
extern "C" int ssrhip_lm_logprobs(const ssrhip_lm* lm) { return (lm && lm->logp) ? 1 : 0; }

extern "C" int ssrhip_lm_set_prompt_groups(ssrhip_lm* lm, const int32_t* chunk_head, const int32_t* n_shared) {
  SSR_REQUIRE(lm, "ssrhip_lm_set_prompt_groups: null engine");
  SSR_REQUIRE(!lm->exec, "ssrhip_lm_set_prompt_groups: the decode step of this engine is already captured (call it before the first ssrhip_lm_decode)");
  SSR_REQUIRE(!chunk_head == !n_shared, "ssrhip_lm_set_prompt_groups: chunk_head and n_shared come together (both null = off)");
  const bool on = chunk_head != nullptr;
  SSR_REQUIRE(!on || lm->b.B > 4, "ssrhip_lm_set_prompt_groups: prompt sharing exists for 5..32 rows only (this engine has %d rows)", lm->b.B);
  SSR_REQUIRE(!on || lm->b.kv.max_pages <= 256, "ssrhip_lm_set_prompt_groups: the fused attention walk takes at most 256 pages per row (this engine has %d)", lm->b.kv.max_pages);
  SSR_REQUIRE(!on || !lm->kv16, "ssrhip_lm_set_prompt_groups: an engine with a bf16 KV cache does not share prompts (the grouped walk reads fp32 entries)");
  lm->chunk_head = chunk_head;
  lm->n_shared = n_shared;
  lm->group_members = on ? ssrhip_attn_group_members() : 0;
  return 0;
}
extern "C" int ssrhip_lm_set_group_members(ssrhip_lm* lm, int32_t members) {
  SSR_REQUIRE(lm, "ssrhip_lm_set_group_members: null engine");
  SSR_REQUIRE(!lm->exec, "ssrhip_lm_set_group_members: the decode step of this engine is already captured (call it before the first ssrhip_lm_decode)");
  SSR_REQUIRE(lm->chunk_head, "ssrhip_lm_set_group_members: this engine does not share prompts (ssrhip_lm_set_prompt_groups comes first)");
  SSR_REQUIRE(members == 2 || members == 4 || members == 8, "ssrhip_lm_set_group_members: %d members per chunk not in {2,4,8}", members);
  lm->group_members = members;
  return 0;
}
extern "C" int ssrhip_lm_group_members(const ssrhip_lm* lm) { return lm && lm->chunk_head ? lm->group_members : 0; }
extern "C" int ssrhip_lm_group_launches(const ssrhip_lm* lm) { return lm && lm->chunk_head ? lm->group_launches : 0; }
extern "C" int ssrhip_lm_w16_launches(const ssrhip_lm* lm) { return lm_packed_launches(lm, PK_W16); }

// Pair launches over the packed weights of the engine's kind: the bf16 copies (csrc/gemv_pair_w16.hip) or the e4m3 codes and scales
// (csrc/gemv_pair_w8.hip). on = 1 repeats ssrhip_lm_create's pairing decision for this engine, with the question put to the kind's
// _applicable; on = 0 gives everything back (the state the stream's setter left). One body, the names of the kind in a record.
struct PackedPair { int kind; const char* setter; const char* stream_setter; const char* fmt; const PairSpec& spec; };
const PackedPair PAIR_W16 = {PK_W16, "ssrhip_lm_set_w16_pair", "ssrhip_lm_set_w16", "bf16", PAIRSPEC_W16};
const PackedPair PAIR_W8 = {PK_W8, "ssrhip_lm_set_w8_pair", "ssrhip_lm_set_w8", "e4m3", PAIRSPEC_W8};
static int lm_set_packed_pair(ssrhip_lm* lm, int on, const PackedPair& pp) {
  SSR_REQUIRE(lm, "%s: null engine", pp.setter);
  SSR_REQUIRE(!lm->exec, "%s: the decode step of this engine is already captured (call it before the first ssrhip_lm_decode)", pp.setter);
  SSR_REQUIRE(lm->b.B == 2, "%s: pair launches exist for the 2-row step only (this engine has %d rows)", pp.setter, lm->b.B);
  SSR_REQUIRE(lm->pk_kind == pp.kind, "%s: this engine does not stream %s weights (%s comes first)", pp.setter, pp.fmt, pp.stream_setter);
  lm_unpair(lm);
  if (!on) {
    snprintf(lm->pair_why, sizeof(lm->pair_why), "this engine streams %s weights (%s) and its %s pair launches are switched off (%s)", pp.fmt, pp.stream_setter, pp.fmt, pp.setter);
    return 0;
  }
  const int rc = lm_take_pairing(lm, pp.spec);
  lm->pk_pair = rc == 1;
  return rc < 0 ? -1 : 0;
}
static int lm_packed_pair_launches(const ssrhip_lm* lm, int kind) { return lm && lm->pk_pair && lm->pk_kind == kind ? lm->pk_pair_launches : 0; }
extern "C" int ssrhip_lm_set_w16_pair(ssrhip_lm* lm, int on) { return lm_set_packed_pair(lm, on, PAIR_W16); }
extern "C" int ssrhip_lm_w16_pair_launches(const ssrhip_lm* lm) { return lm_packed_pair_launches(lm, PK_W16); }
extern "C" int ssrhip_lm_set_w8_pair(ssrhip_lm* lm, int on) { return lm_set_packed_pair(lm, on, PAIR_W8); }
extern "C" int ssrhip_lm_w8_pair_launches(const ssrhip_lm* lm) { return lm_packed_pair_launches(lm, PK_W8); }

// Pair launches of the 4-row step over the fp32 weights (csrc/gemv_pair4.hip). on = 1 repeats ssrhip_lm_create's pairing decision for this
// engine with the question put to ssrhip_gemv_pair4_applicable; on = 0 gives slot and workspace back.
extern "C" int ssrhip_lm_set_pair4(ssrhip_lm* lm, int on) {
  SSR_REQUIRE(lm, "ssrhip_lm_set_pair4: null engine");
  SSR_REQUIRE(!lm->exec, "ssrhip_lm_set_pair4: the decode step of this engine is already captured (call it before the first ssrhip_lm_decode)");
  SSR_REQUIRE(lm->b.B == 4, "ssrhip_lm_set_pair4: the 4-row pair launches exist for the 4-row step only (this engine has %d rows)", lm->b.B);
  SSR_REQUIRE(lm->pk_kind < 0, "ssrhip_lm_set_pair4: this engine streams packed weights; the 4-row pair launches read the fp32 masters");
  lm_unpair(lm);
  if (!on) {
    snprintf(lm->pair_why, sizeof(lm->pair_why), "the 4-row pair launches of this engine are switched off (ssrhip_lm_set_pair4)");
    return 0;
  }
  const int rc = lm_take_pairing(lm, PAIRSPEC_PAIR4);
  lm->pair4 = rc == 1;
  return rc < 0 ? -1 : 0;
}
extern "C" int ssrhip_lm_pair4_launches(const ssrhip_lm* lm) { return lm && lm->pair4 ? lm->pair4_launches : 0; }

// Pair launches of the 4-row step over the engine's packed stream (csrc/gemv_pair4_pk.hip): the bf16 copies or the e4m3 codes and scales.
// on = 1 repeats ssrhip_lm_create's pairing decision for this engine with the question put to the kind's _applicable; on = 0 gives slot
// and workspace back (the state the stream's setter left).
extern "C" int ssrhip_lm_set_pair4_pk(ssrhip_lm* lm, int on) {
  SSR_REQUIRE(lm, "ssrhip_lm_set_pair4_pk: null engine");
  SSR_REQUIRE(!lm->exec, "ssrhip_lm_set_pair4_pk: the decode step of this engine is already captured (call it before the first ssrhip_lm_decode)");
  SSR_REQUIRE(lm->b.B == 4, "ssrhip_lm_set_pair4_pk: the 4-row pair launches exist for the 4-row step only (this engine has %d rows)", lm->b.B);
  SSR_REQUIRE(lm->pk_kind == PK_W16 || lm->pk_kind == PK_W8, "ssrhip_lm_set_pair4_pk: this engine streams no packed weights (ssrhip_lm_set_w16 or ssrhip_lm_set_w8 comes first; "
              "ssrhip_lm_set_pair4 pairs the fp32 masters)");
  const bool w8 = lm->pk_kind == PK_W8;
  lm_unpair(lm);
  if (!on) {
    snprintf(lm->pair_why, sizeof(lm->pair_why), "this engine streams %s weights and its 4-row %s pair launches are switched off (ssrhip_lm_set_pair4_pk)", w8 ? "e4m3" : "bf16",
             w8 ? "e4m3" : "bf16");
    return 0;
  }
  const int rc = lm_take_pairing(lm, w8 ? PAIRSPEC_PAIR4_W8 : PAIRSPEC_PAIR4_W16);
  lm->pair4_pk = rc == 1;
  return rc < 0 ? -1 : 0;
}
extern "C" int ssrhip_lm_pair4_pk_launches(const ssrhip_lm* lm) { return lm && lm->pair4_pk ? lm->pair4_pk_launches : 0; }
extern "C" int ssrhip_lm_wt16_launches(const ssrhip_lm* lm) { return lm_packed_launches(lm, PK_WT16); }
extern "C" int ssrhip_lm_wt32_launches(const ssrhip_lm* lm) { return lm_packed_launches(lm, PK_WT32); }

extern "C" int ssrhip_lm_pair_status(ssrhip_lm* lm, ssrhip_stream_t stream) {
  SSR_REQUIRE(lm, "ssrhip_lm_pair_status: null engine");
  if (!lm->pair_ws) return 0;
  if (lm->pair4 || lm->pair4_pk) return ssrhip_gemv_pair4_status(lm->pair_ws, stream);   // the 4-row workspace is twice the size
  return ssrhip_gemv_pair_status(lm->pair_ws, stream);
}

extern "C" int ssrhip_debug_occupy(int32_t n_wg, int32_t lds_bytes, float ms, int32_t* started, ssrhip_stream_t stream) {
  SSR_REQUIRE(n_wg > 0 && n_wg <= 65535 && lds_bytes >= 0 && lds_bytes <= 160 * 1024 && ms >= 0.f && ms <= 20000.f, "ssrhip_debug_occupy: bad argument");
  if (lds_bytes > 64 * 1024)
    SSR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(occupy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
  hipLaunchKernelGGL(occupy_kernel, dim3(n_wg), dim3(256), (size_t)lds_bytes, (hipStream_t)stream, (long long)(ms * 100000.0f), lds_bytes / 4, started);
  SSR_LAUNCH_CHECK();
  return 0;
}

extern "C" void ssrhip_lm_destroy(ssrhip_lm* lm) {
  if (!lm) return;
  if (lm->exec) hipGraphExecDestroy(lm->exec);
  if (lm->graph) hipGraphDestroy(lm->graph);
  if (lm->cap_stream) hipStreamDestroy(lm->cap_stream);
  lm_unpair(lm);
  delete lm;
}

extern "C" int ssrhip_lm_decode(ssrhip_lm* lm, int32_t n_steps, int32_t use_graph, ssrhip_stream_t stream) {
  SSR_REQUIRE(lm && n_steps >= 0, "ssrhip_lm_decode: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (!use_graph) {
    for (int i = 0; i < n_steps; ++i)
      if (int rc = enqueue_step(lm, s, nullptr)) return rc;
    return 0;
  }
  if (!lm->exec) {
    if (!lm->cap_stream) SSR_HIP(hipStreamCreateWithFlags(&lm->cap_stream, hipStreamNonBlocking));
    SSR_HIP(hipStreamBeginCapture(lm->cap_stream, hipStreamCaptureModeThreadLocal));
    int rc = enqueue_step(lm, lm->cap_stream, nullptr);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(lm->cap_stream, &g);
    if (rc) { if (g) hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) { ssrhip_set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return -2; }
    lm->graph = g;
    SSR_HIP(hipGraphInstantiate(&lm->exec, lm->graph, nullptr, nullptr, 0));
  }
  for (int i = 0; i < n_steps; ++i) SSR_HIP(hipGraphLaunch(lm->exec, s));
  return 0;
}

extern "C" int ssrhip_lm_time_steps(ssrhip_lm* lm, int32_t n_steps, ssrhip_stream_t stream, float* out_us, int32_t* out_kind, int32_t n_out) {
  SSR_REQUIRE(lm && n_steps > 0 && out_us && out_kind, "ssrhip_lm_time_steps: bad argument");
  Timer tm;
  tm.on = true;
  tm.s = (hipStream_t)stream;
  SSR_HIP(hipEventCreate(&tm.e0));
  SSR_HIP(hipEventCreate(&tm.e1));
  int rc = 0;
  for (int i = 0; i < n_steps && !rc; ++i) rc = enqueue_step(lm, tm.s, &tm);
  hipEventDestroy(tm.e0);
  hipEventDestroy(tm.e1);
  if (rc) return rc;
  const int n = (int)tm.ms.size();
  SSR_REQUIRE(n <= n_out, "ssrhip_lm_time_steps: %d slots > n_out=%d", n, n_out);
  for (int i = 0; i < n; ++i) { out_us[i] = 1000.f * tm.ms[i] / n_steps; out_kind[i] = tm.kind[i]; }
  return n;
}

extern "C" int ssrhip_lm_time_category(ssrhip_lm* lm, int32_t category, int32_t n_replays, ssrhip_stream_t stream, float* out_us_per_launch,
                                       int32_t* out_launches_per_step) {
  SSR_REQUIRE(lm && category >= 0 && category <= CAT_SAMPLE && n_replays > 0 && out_us_per_launch && out_launches_per_step,
              "ssrhip_lm_time_category: bad argument");
  hipStream_t s = (hipStream_t)stream;
  Timer tm;
  tm.only = category;
  hipStream_t cap = nullptr;
  SSR_HIP(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
  SSR_HIP(hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
  int rc = enqueue_step(lm, cap, &tm);
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(cap, &g);
  hipGraphExec_t ex = nullptr;
  if (!rc && e == hipSuccess) e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  float ms = 0.f;
  if (!rc && e == hipSuccess) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int i = 0; i < 3; ++i) hipGraphLaunch(ex, s);
    hipEventRecord(e0, s);
    for (int i = 0; i < n_replays; ++i) hipGraphLaunch(ex, s);
    hipEventRecord(e1, s);
    e = hipEventSynchronize(e1);
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  if (ex) hipGraphExecDestroy(ex);
  if (g) hipGraphDestroy(g);
  hipStreamDestroy(cap);
  if (rc) return rc;
  if (e != hipSuccess) { ssrhip_set_error("ssrhip_lm_time_category: %s", hipGetErrorString(e)); return -2; }
  SSR_REQUIRE(tm.n_enq > 0, "ssrhip_lm_time_category: no launches in category %d", category);
  *out_launches_per_step = tm.n_enq;
  *out_us_per_launch = 1000.f * ms / ((float)n_replays * (float)tm.n_enq);
  return 0;
}

// The layer loop over R flattened rows (embedding, then n_layer x [LN1 -> QKV GEMM -> KV scatter -> attention -> out-proj + residual
// -> LN2 -> FFN1 + ReLU -> FFN2 + residual]), shared by the prefill and the scoring entry. `kv` is the cache the rows write and read;
// with kv.n_layer == 1 (a scoring scratch pool) every layer uses layer 0 of it. `planes`: how many bf16 planes each `*_ws` of `w` holds —
// 0 = GEMMs on the fp32 chain, 3 = ssrhip_gemm on the exact split, 1 = ssrhip_gemm_w1.
//
// One GEMM of the LM on `planes` planes at `ws`. One plane: ssrhip_gemm_w1, and where it does not qualify (answer 1) the fp32 chain on the
// masters — what a three-plane call that does not qualify takes too (ssrhip_gemm never reads a one-plane buffer as three).
static int lm_gemm(ssrhip_gemm_args& g, int planes, const uint16_t* ws, hipStream_t s) {
  g.W_split = planes ? ws : nullptr;
  if (planes == 1) {
    const int rc = ssrhip_gemm_w1(&g, s);
    if (rc != 1) return rc;
    g.W_split = nullptr;
  }
  return ssrhip_gemm(&g, s);
}

// `kv16`: the cache holds 2-byte entries — the rounding scatter and the widening tiled attention (the caller has refused a rowwise prefill).
static int lm_layer_loop(const ssrhip_lm_dims& d, const ssrhip_lm_weights& w, int planes, const ssrhip_kv& kv, const ssrhip_prefill_args* p,
                         bool tiled_attn, bool kv16, hipStream_t s) {
  const int D = d.d_model, R = p->R;
  const bool one_layer_kv = kv.n_layer == 1;

  ssrhip_embed_args ea = embed_args(d, w, R, p->x, 0);
  ea.tok = p->tok; ea.pos = p->pos; ea.kind = p->kind;
  if (int rc = ssrhip_embed(&ea, s)) return rc;

  for (int l = 0; l < d.n_layer; ++l) {
    const int kl = one_layer_kv ? 0 : l;
    if (int rc = ssrhip_layernorm(p->x, w.ln1_w[l], w.ln1_b[l], 1e-5f, p->xn, R, D, s)) return rc;
    ssrhip_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.A = p->xn; g.W = w.in_proj_w[l]; g.bias = w.in_proj_b[l]; g.C = p->qkv;
    g.M = R; g.N = 3 * D; g.K = D; g.lda = D; g.ldc = 3 * D;
    if (int rc = lm_gemm(g, planes, planes ? w.in_proj_ws[l] : nullptr, s)) return rc;
    if (int rc = (kv16 ? ssrhip_kv_scatter16 : ssrhip_kv_scatter)(p->qkv, &kv, kl, p->row_seq, p->row_pos, R, s)) return rc;

    ssrhip_attn_args at;
    memset(&at, 0, sizeof(at));
    at.kv = kv; at.layer = kl; at.row_seq = p->row_seq; at.row_len = p->row_len;
    at.R = R; at.max_splits = p->max_splits; at.scale = 1.0f / sqrtf((float)(D / d.n_head));
    at.part_o = p->part_o; at.part_ml = p->part_ml;
    at.q = p->qkv; at.q_stride = 3 * D;   // q is the first third of each packed qkv row
    if (tiled_attn) {
      // whole prompts: K/V tiles staged in LDS once per 128 queries, both products on the matrix core, no partials
      if (int rc = (kv16 ? ssrhip_attn_prefill_kv16 : ssrhip_attn_prefill)(&at, p->seq_start, p->n_seq, p->max_len, p->o, s)) return rc;
    } else {
      if (int rc = ssrhip_attn_decode(&at, s)) return rc;
      if (int rc = ssrhip_attn_combine(&at, p->o, s)) return rc;
    }

    memset(&g, 0, sizeof(g));
    g.A = p->o; g.W = w.out_proj_w[l]; g.bias = w.out_proj_b[l]; g.C = p->x;
    g.M = R; g.N = D; g.K = D; g.lda = D; g.ldc = D; g.residual = 1;
    if (int rc = lm_gemm(g, planes, planes ? w.out_proj_ws[l] : nullptr, s)) return rc;

    if (int rc = ssrhip_layernorm(p->x, w.ln2_w[l], w.ln2_b[l], 1e-5f, p->xn, R, D, s)) return rc;
    memset(&g, 0, sizeof(g));
    g.A = p->xn; g.W = w.ffn1_w[l]; g.bias = w.ffn1_b[l]; g.C = p->h;
    g.M = R; g.N = d.d_ffn; g.K = D; g.lda = D; g.ldc = d.d_ffn; g.act = SSRHIP_ACT_RELU;
    if (int rc = lm_gemm(g, planes, planes ? w.ffn1_ws[l] : nullptr, s)) return rc;
    memset(&g, 0, sizeof(g));
    g.A = p->h; g.W = w.ffn2_w[l]; g.bias = w.ffn2_b[l]; g.C = p->x;
    g.M = R; g.N = D; g.K = d.d_ffn; g.lda = d.d_ffn; g.ldc = D; g.residual = 1;
    if (int rc = lm_gemm(g, planes, planes ? w.ffn2_ws[l] : nullptr, s)) return rc;
  }
  return 0;
}

extern "C" int ssrhip_lm_prefill(ssrhip_lm* lm, const ssrhip_prefill_args* p, ssrhip_stream_t stream) {
  SSR_REQUIRE(lm && p && p->tok && p->pos && p->kind && p->row_seq && p->row_pos && p->row_len, "ssrhip_lm_prefill: null argument");
  const bool tiled_attn = p->seq_start && p->n_seq > 0 && p->max_len > 0 && !getenv_flag("SSRHIP_PREFILL_ATTN_ROWWISE");
  const bool kv16 = lm->kv16 || lm->land;         // the pool holds 2-byte entries, whichever step fills it later
  SSR_REQUIRE(tiled_attn || !kv16, "ssrhip_lm_prefill: an engine with a bf16 KV cache prefills through the tiled attention only (seq_start is missing or "
              "SSRHIP_PREFILL_ATTN_ROWWISE is set): the rowwise kernels read fp32 entries");
  SSR_REQUIRE(p->x && p->xn && p->qkv && p->o && p->h && (tiled_attn || (p->part_o && p->part_ml)), "ssrhip_lm_prefill: null workspace");
  ssrhip_kv kv = lm->b.kv;
  if (p->table) kv.table = p->table;              // two-phase admission: the rows being filled are not in the decode step's table yet
  if (int rc = lm_layer_loop(lm->d, lm->w, lm->prefill_split ? (lm->prefill_w1 ? 1 : 3) : 0, kv, p, tiled_attn, kv16, (hipStream_t)stream)) return rc;
  if (p->no_embed) return 0;
  return ssrhip_lm_embed_pending(lm, stream);
}

// the one body of ssrhip_lm_score (np = 3) and ssrhip_lm_score_w1 (np = 1): `np` = planes in every *_ws buffer of `w` and `a`
static int lm_score(const ssrhip_lm_dims* d, const ssrhip_lm_weights* w, const ssrhip_score_args* a, int np, ssrhip_stream_t stream) {
  SSR_REQUIRE(d && w && a, "ssrhip_lm_score: null argument");
  SSR_REQUIRE(a->tok && a->pos && a->kind && a->row_seq && a->row_pos && a->row_len && a->seq_start && a->score_first && a->score_count &&
              a->target && a->nll && a->rank, "ssrhip_lm_score: null row / target / output array");
  SSR_REQUIRE(a->x && a->xn && a->qkv && a->o && a->h && a->hs && a->head_h && a->logits && a->kv.pool && a->kv.table,
              "ssrhip_lm_score: null workspace");
  SSR_REQUIRE(a->kv.n_layer == 1, "ssrhip_lm_score: the scratch pool holds one layer (kv.n_layer = %d)", a->kv.n_layer);
  SSR_REQUIRE(a->kv.n_head == d->n_head && a->kv.head_dim * d->n_head == d->d_model, "ssrhip_lm_score: kv heads do not match the dims");
  SSR_REQUIRE(a->R > 0 && a->n_seq > 0 && a->max_len > 0 && a->M > 0 && a->head_chunk > 0, "ssrhip_lm_score: empty problem");
  SSR_REQUIRE(d->n_codebooks >= 1 && d->n_codebooks <= SSRHIP_MAX_CODEBOOKS, "ssrhip_lm_score: n_codebooks %d", d->n_codebooks);
  SSR_REQUIRE(w->lnf_w && w->lnf_b && w->head1_w && w->head1_b && w->head2_w && w->head2_b, "ssrhip_lm_score: null head weights");
  SSR_REQUIRE(!a->head1_ws == !a->head2_ws, "ssrhip_lm_score: head split planes come both or none");
  // the scored rows: inside the R rows, M in total (host arrays; checked before anything is launched)
  long m_sum = 0;
  for (int sq = 0; sq < a->n_seq; ++sq) {
    const int f = a->score_first[sq], c = a->score_count[sq];
    SSR_REQUIRE(f >= 0 && c >= 0 && (long)f + c <= a->R, "ssrhip_lm_score: scored rows of sequence %d outside the %d rows", sq, a->R);
    m_sum += c;
  }
  SSR_REQUIRE(m_sum == a->M, "ssrhip_lm_score: score_count sums to %ld, M = %d", m_sum, a->M);
  const int D = d->d_model, K = d->n_codebooks, Hh = d->head_hidden, card = d->card, ldc = (card + 3) / 4 * 4;
  hipStream_t s = (hipStream_t)stream;
  const char* e = getenv("SSRHIP_PREFILL_SPLIT");
  const bool split_ok = !(e && e[0] == '0');
  const bool layer_split = split_ok && w->in_proj_ws && w->out_proj_ws && w->ffn1_ws && w->ffn2_ws;
  const bool head_split = split_ok && a->head1_ws;

  ssrhip_prefill_args p;
  memset(&p, 0, sizeof(p));
  p.tok = a->tok; p.pos = a->pos; p.kind = a->kind;
  p.row_seq = a->row_seq; p.row_pos = a->row_pos; p.row_len = a->row_len;
  p.R = a->R; p.max_splits = (a->max_len + SSRHIP_PAGE - 1) / SSRHIP_PAGE;
  p.x = a->x; p.xn = a->xn; p.qkv = a->qkv; p.o = a->o; p.h = a->h;
  p.seq_start = a->seq_start; p.n_seq = a->n_seq; p.max_len = a->max_len;
  if (int rc = lm_layer_loop(*d, *w, layer_split ? np : 0, a->kv, &p, true, false, s)) return rc;

  // final LayerNorm of the scored rows only, gathered by the launch itself: one launch per sequence (its scored rows are contiguous)
  long off = 0;
  for (int sq = 0; sq < a->n_seq; ++sq) {
    const int c = a->score_count[sq];
    if (c == 0) continue;
    if (int rc = ssrhip_layernorm(a->x + (size_t)a->score_first[sq] * D, w->lnf_w, w->lnf_b, 1e-5f, a->hs + (size_t)off * D, c, D, s)) return rc;
    off += c;
  }
  // prediction heads in chunks of rows: head 1 of all codebooks in one GEMM (+GELU), then per codebook head 2 -> logits -> CE / rank
  for (int m0 = 0; m0 < a->M; m0 += a->head_chunk) {
    const int mc = a->M - m0 < a->head_chunk ? a->M - m0 : a->head_chunk;
    ssrhip_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.A = a->hs + (size_t)m0 * D; g.W = w->head1_w; g.bias = w->head1_b; g.C = a->head_h;
    g.M = mc; g.N = K * Hh; g.K = D; g.lda = D; g.ldc = K * Hh; g.act = SSRHIP_ACT_GELU_ERF;
    if (int rc = lm_gemm(g, head_split ? np : 0, a->head1_ws, s)) return rc;
    for (int k = 0; k < K; ++k) {
      memset(&g, 0, sizeof(g));
      g.A = a->head_h + (size_t)k * Hh; g.W = w->head2_w + (size_t)k * card * Hh; g.bias = w->head2_b + (size_t)k * card; g.C = a->logits;
      g.M = mc; g.N = card; g.K = Hh; g.lda = K * Hh; g.ldc = ldc;
      if (int rc = lm_gemm(g, head_split ? np : 0, head_split ? a->head2_ws + (size_t)k * np * card * Hh : nullptr, s)) return rc;
      const size_t o = (size_t)k * a->M + m0;
      if (int rc = ssrhip_xent_rank(a->logits, ldc, card, a->target + o, mc, a->nll + o, a->rank + o, stream)) return rc;
    }
  }
  return 0;
}

extern "C" int ssrhip_lm_score(const ssrhip_lm_dims* d, const ssrhip_lm_weights* w, const ssrhip_score_args* a, ssrhip_stream_t stream) {
  return lm_score(d, w, a, 3, stream);
}
extern "C" int ssrhip_lm_score_w1(const ssrhip_lm_dims* d, const ssrhip_lm_weights* w, const ssrhip_score_args* a, ssrhip_stream_t stream) {
  return lm_score(d, w, a, 1, stream);
}

extern "C" int ssrhip_lm_embed_pending(ssrhip_lm* lm, ssrhip_stream_t stream) {
  SSR_REQUIRE(lm, "ssrhip_lm_embed_pending: null argument");
  // x of the first decode step: the rows' pending input tokens (the span-0 mask token, ssr.py:655-662)
  const ssrhip_lm_buffers& b = lm->b;
  ssrhip_embed_args ea = embed_args(lm->d, lm->w, b.B, b.x, b.B > 4 ? 1 : 0);
  ea.tok = b.next_tok; ea.pos = b.next_pos; ea.kind = nullptr;
  return ssrhip_embed(&ea, (hipStream_t)stream);
}
