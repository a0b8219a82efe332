// gemv_pair_host.h — the host side of the pair launches, once for every form (fp32 at 2 rows: gemv.hip; packed bf16: gemv_pair_w16.hip;
// e4m3 codes: gemv_pair_w8.hip; fp32 at 4 rows: gemv_pair4.hip; packed at 4 rows: gemv_pair4_pk.hip): the argument checks of an entry
// point, the launch descriptor, the table of a form's kernels with the launch through it, the occupancy question, the packed forms'
// applicability question, the 4-row forms' shape rules and the give-up poll.
// What a form keeps to itself: its kernels, its table, its thread-local "why" text and what its question adds to the 2-row one.
#pragma once
#include <stdlib.h>
#include "common.h"
#include "gemv_shared.h"
#include "gemv_pair.h"

// gemv.hip's pair_nuwb on the current device, the ONE shape qualifier: units per wave of B (4, 6 or 8) if the 2-row launches (a, b) can
// run as one pair launch, 0 otherwise (the reason is then ssrhip_gemv_pair_why()); *merge = A is the out-projection behind the split-KV merge
int ssrhip_gemv_pair_plan(const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, bool* merge);

namespace {

// a form's kernels (Q = its kernel argument: PairK, or PairK with the packed pointers beside it) and what its occupancy question says
template <class Q>
struct PairForm {
  void (*ffn2[3])(Q);        // A = FFN2, B with 4 / 6 / 8 units per wave
  void (*merge_early)(Q);    // A = merge + out-projection, B = FFN1; with B's first two units requested at entry where the form has them
  void (*merge_plain)(Q);    // the same without early units (SSRHIP_GEMV_PAIR_EARLY=0), or null: the 4-row form has no such split
  bool ask_plain;            // the occupancy question covers merge_plain too (the packed forms ask all five, the fp32 form four)
  const char* what;          // "pair", "bf16 pair", ... in the refusal
  size_t wtab_bytes;         // most dynamic LDS a merge launch takes (its merge weights)
  bool asked;                // the occupancy verdict, asked once per process
  const char* verdict;
  char buf[200];
};

// the argument checks every pair entry point makes; others_ok = the form's further pointers (workspace, packed weights, scales) are set
inline int pair_entry_check(const char* who, const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, bool others_ok, int buf, int buf_next) {
  SSR_REQUIRE(a && b && others_ok, "%s: null argument", who);
  SSR_REQUIRE(buf >= 0 && buf < 3 && buf_next >= 0 && buf_next < 3 && buf != buf_next, "%s: granule buffers %d -> %d (0..2, different)", who, buf, buf_next);
  SSR_REQUIRE(a->epi != SSRHIP_EPI_QKV_APPEND16 && b->epi != SSRHIP_EPI_QKV_APPEND16, "%s: the 2-byte KV append (EPI_QKV_APPEND16) exists for 5..32 rows only", who);
  return 0;
}

// the descriptor of a pair launch: one workgroup per CU (8 rows of A, N / 256 rows of B), this launch's granule buffer and the next one's
// of the three in ws (gran_per_buffer = PAIR_GRAN or PAIR4_GRAN granules each), the give-up flag behind them
inline void pair_fill(PairK& p, const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, bool merge, void* ws, int buf, int buf_next, int gran_per_buffer) {
  seg_fill(&p.a, a, merge ? 2 : 8, 256);
  seg_fill(&p.b, b, 2, 256);
  unsigned long long* gran = (unsigned long long*)ws;
  p.gran = gran + (size_t)buf * gran_per_buffer;
  p.gran_next = gran + (size_t)buf_next * gran_per_buffer;
  p.gave_up = (int*)(gran + 3 * (size_t)gran_per_buffer);
}

// launch the form's kernel for (merge, nuwb) as the plan derived them; B = batch rows (the merge weights in dynamic LDS are [B * H][max_splits])
template <class Q>
int pair_launch(const PairForm<Q>& f, const Q& q, bool merge, int nuwb, int B, const ssrhip_gemv_args* a, hipStream_t s) {
  if (merge) {
    const size_t sm = ((size_t)B * (a->K / a->kv.head_dim) * a->max_splits * sizeof(float) + 15) / 16 * 16;
    // SSRHIP_GEMV_PAIR_EARLY is read at every call (graph capture): A/B inside one process. 0 = round 5's order. (With the early units in
    // place, FOUR units in flight behind (1b) measured 0.759 ms/step and TWO — nothing between the publish and the gather — 0.767 against
    // 0.745-0.748 for three: PFX stays PAIR_PF; profiles/r06_microbench/decode_ab_pair_early_pf*.log.)
    const char* ee = f.merge_plain ? getenv("SSRHIP_GEMV_PAIR_EARLY") : nullptr;
    hipLaunchKernelGGL((ee && ee[0] == '0') ? f.merge_plain : f.merge_early, dim3(256), dim3(PAIR_TH), sm, s, q);
  } else {
    hipLaunchKernelGGL(f.ffn2[nuwb == 4 ? 0 : nuwb == 6 ? 1 : 2], dim3(256), dim3(PAIR_TH), 0, s, q);
  }
  SSR_LAUNCH_CHECK();
  return 0;
}

// Can a CU take a workgroup of every instantiation of the form (12 waves, their registers and LDS)? Asked once per process; CU count
// and CU masks are gemv.hip's pair_device_refusal's part, which every form's question reaches first.
template <class Q>
const char* pair_occupancy_refusal(PairForm<Q>& f) {
  if (f.asked) return f.verdict;
  f.asked = true;
  void (*const k[5])(Q) = {f.ffn2[0], f.ffn2[1], f.ffn2[2], f.merge_early, f.merge_plain};
  const int n = f.ask_plain ? 5 : 4;
  int nb[5] = {0, 0, 0, 0, 0};
  bool ok = true;
  for (int i = 0; i < n; ++i) {                                      // every one is asked, also behind a failure: the text shows all counts
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb[i], k[i], PAIR_TH, i < 3 ? 0 : f.wtab_bytes);
    ok = ok && e == hipSuccess && nb[i] >= 1;
  }
  if (ok) return f.verdict = nullptr;
  if (n == 5) snprintf(f.buf, sizeof(f.buf), "the occupancy calculator places %d / %d / %d / %d / %d workgroups of the %s kernels on a CU (need >= 1 each)", nb[0], nb[1], nb[2], nb[3], nb[4], f.what);
  else snprintf(f.buf, sizeof(f.buf), "the occupancy calculator places %d / %d / %d / %d workgroups of the %s kernels on a CU (need >= 1 each)", nb[0], nb[1], nb[2], nb[3], f.what);
  return f.verdict = f.buf;
}

inline int pair_refuse(char (&why)[200], const char* text) { snprintf(why, sizeof(why), "%s", text); return 0; }

// The packed forms' question, answered like pair_nuwb: the 2-row question (shapes, >= 256 CUs, no CU mask, SSRHIP_GEMV_PAIR) AND the
// stream's own applicability for both launches (SSRHIP_GEMV_SEG=0 turns it off) AND a CU takes every instantiation. `why` is the form's
// thread-local text: the last question on this thread.
template <class Q>
int pair_packed_plan(PairForm<Q>& f, char (&why)[200], const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, int (*stream_applicable)(const ssrhip_gemv_args*),
                     const char* stream_refusal, bool* merge) {
  const int nuwb = ssrhip_gemv_pair_plan(a, b, merge);
  if (!nuwb) return pair_refuse(why, ssrhip_gemv_pair_why());
  if (!stream_applicable(a) || !stream_applicable(b)) return pair_refuse(why, stream_refusal);
  if (const char* w = pair_occupancy_refusal(f)) return pair_refuse(why, w);
  why[0] = 0;
  return nuwb;
}

constexpr size_t PAIR4_WTAB_MAX = 16 * 1024;   // 4 rows: merge weights in dynamic LDS, next to ~34 KB of static buffers

// The shape part of every 4-row question (fp32: gemv_pair4.hip; packed: gemv_pair4_pk.hip): B == 4, then the 2-row question put with the
// row count set to 2 (shapes, >= 256 CUs, no CU mask, SSRHIP_GEMV_PAIR = 0 / 1 / 2), then what four rows change — the merge's (row,
// head) table and its LDS. Units per wave of B (`why` untouched), or 0 with the reason in `why`.
inline int pair4_shape_plan(char (&why)[200], const ssrhip_gemv_args* a, const ssrhip_gemv_args* b, bool* merge) {
  if (a->B != PAIR4_B || b->B != PAIR4_B) return pair_refuse(why, "not a 4-row launch (the 4-row pair kernels take B = 4 only)");
  ssrhip_gemv_args a2 = *a, b2 = *b;
  a2.B = b2.B = 2;
  const int nuwb = ssrhip_gemv_pair_plan(&a2, &b2, merge);
  if (!nuwb) return pair_refuse(why, ssrhip_gemv_pair_why());
  if (*merge) {
    const int H = a->K / a->kv.head_dim;
    if (PAIR4_B * H > SEG_TH) return pair_refuse(why, "merge form: more than 512 (row, head) pairs");
    if ((size_t)PAIR4_B * H * a->max_splits * sizeof(float) > PAIR4_WTAB_MAX) return pair_refuse(why, "merge weights exceed 16 KB of LDS (context too long for the 4-row merge form)");
  }
  return nuwb;
}

// Did a workgroup of a launch on this workspace give up (1) or not (0)? Reported once: tags and flag go back to "nothing published" so
// that a chain restarted from its first launch (after a new prefill) is valid again (the stream is idle: it is synchronised here).
// The flag sits behind the three granule buffers, at byte flag_offset of the ws_bytes.
inline int pair_status(const void* ws, size_t ws_bytes, size_t flag_offset, const char* who, ssrhip_stream_t stream) {
  SSR_REQUIRE(ws, "%s: null workspace", who);
  int flag = 0;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) { ssrhip_set_error("%s: stream synchronize failed", who); return -1; }
  if (hipMemcpy(&flag, (const char*)ws + flag_offset, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
    ssrhip_set_error("%s: copy failed", who);
    return -1;
  }
  if (flag) {
    if (hipMemset(const_cast<void*>(ws), 0, ws_bytes) != hipSuccess) { ssrhip_set_error("%s: re-zeroing the workspace failed", who); return -1; }
  }
  return flag ? 1 : 0;
}

}  // namespace
