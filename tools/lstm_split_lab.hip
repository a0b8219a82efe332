// lstm_split_lab.hip — the LSTM recurrence through the C-ABI on ONE bf16-rounded W_hh, four arms in one process: the fp32 matrix pipe
// (ssrhip_lstm_layer without planes: lstm_step_wide_kernel), the three-plane split step (csrc/lstm_split.hip), and the one-plane step
// (ssrhip_lstm_layer_w1, csrc/lstm_w1.hip) with four and — where C % 512 == 0 — eight k-steps in flight (SSRHIP_LSTM_W1_DEPTH=8).
// Microseconds per step alone and with two layers' chains on two streams (the codec's pipeline): one untimed pass, then `rounds` rounds
// in alternating arm order, median and spread (max - min). The one-plane outputs are compared with the three-plane ones bit for bit, the
// split ones with the fp32 pipe's by their largest difference. No torch: a GPU call of a few seconds.
// Usage: lstm_split_lab [B = 256] [C = 512] [T = 200] [rounds = 4]; a last line `JSON {...}` repeats the table for scripts.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include tools/lstm_split_lab.hip -Lssr-speech_amd/csrc -lssrhip \
//        -Wl,-rpath,'$ORIGIN/../../ssr-speech_amd/csrc' -o tools/bin/lstm_split_lab
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "ssrhip.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
#define SK(x) do { if ((x) != 0) { fprintf(stderr, "%s: %s\n", #x, ssrhip_last_error()); exit(1); } } while (0)

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s; }
static float rnd(unsigned& s) { return ((int)(lcg(s) >> 8) - (1 << 23)) * (1.0f / (1 << 23)); }      // (-1, 1)

static float bf16_rne(float v) {                                     // the value WMEncodecModel(weight_dtype="bf16") keeps: nearest even
  unsigned u; memcpy(&u, &v, 4);
  u = (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
  memcpy(&v, &u, 4);
  return v;
}

struct Layer {
  float *gin, *whh_packed, *out, *hbuf, *cbuf;
  uint16_t *wsplit, *wone, *hsplit;
};

enum Arm { WIDE = 0, X3 = 1, X1_D4 = 2, X1_D8 = 3, NARMS = 4 };
static const char* ARM_NAME[NARMS] = {"fp32 matrix pipe (lstm_step_wide_kernel)", "three planes, six products (lstm_split.hip)",
                                      "one plane, three products (lstm_w1.hip)", "one plane, SSRHIP_LSTM_W1_DEPTH=8"};
static const char* ARM_KEY[NARMS] = {"wide", "x3", "x1", "x1_depth8"};

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 256, C = argc > 2 ? atoi(argv[2]) : 512, T = argc > 3 ? atoi(argv[3]) : 200;
  const int rounds = argc > 4 ? atoi(argv[4]) : 4;
  if (C % 128 || C > 1024 || B < 32 || T < 1 || rounds < 1) { fprintf(stderr, "need C %% 128 == 0, C <= 1024 (the fp32 pipe's limit), B >= 32\n"); return 1; }
  const int KS = C / 64, rows = (B + 15) / 16 * 16, nbg = (B + 63) / 64;
  unsigned seed = 99;
  std::vector<float> whh((size_t)4 * C * C), gin((size_t)B * T * 4 * C);
  for (auto& v : whh) v = bf16_rne(rnd(seed) / sqrtf((float)C) * 1.7f);
  for (auto& v : gin) v = rnd(seed) * 1.5f;
  // the fp32 kernels' packed order (include/ssrhip.h w_packed): [C/4 tiles][C/16 k-steps][4 k-slots][16 rows][4 floats], row r of tile j =
  // W_hh[(r % 4) C + 4 j + r / 4]  ==  whh.view(4, C/4, 4, C/16, 4, 4).permute(1, 3, 4, 2, 0, 5) of wmencodec._Lstm
  std::vector<float> packed((size_t)4 * C * C);
  {
    size_t o = 0;
    for (int j = 0; j < C / 4; ++j)
      for (int s = 0; s < C / 16; ++s)
        for (int ks = 0; ks < 4; ++ks)
          for (int u = 0; u < 4; ++u)
            for (int g = 0; g < 4; ++g)
              for (int e = 0; e < 4; ++e) packed[o++] = whh[((size_t)g * C + 4 * j + u) * C + 16 * s + 4 * ks + e];
  }
  float *d_whh;
  uint16_t* d_planes;
  CK(hipMalloc(&d_whh, whh.size() * 4)); CK(hipMalloc(&d_planes, whh.size() * 6));
  CK(hipMemcpy(d_whh, whh.data(), whh.size() * 4, hipMemcpyHostToDevice));
  SK(ssrhip_split_weights(d_whh, d_planes, (int64_t)whh.size(), nullptr));
  std::vector<uint16_t> planes(whh.size() * 3), wsplit(whh.size() * 3);
  CK(hipMemcpy(planes.data(), d_planes, planes.size() * 2, hipMemcpyDeviceToHost));
  // wmencodec.pack_lstm_whh_planes: out[ub][w][s][mb][q][lh][li][e] = planes[q][g C + 16 ub + u][w C/4 + 16 s + 8 lh + e], 32 mb + li = 16 g + u
  {
    size_t o = 0;
    for (int ub = 0; ub < C / 16; ++ub)
      for (int w = 0; w < 4; ++w)
        for (int s = 0; s < KS; ++s)
          for (int mb = 0; mb < 2; ++mb)
            for (int q = 0; q < 3; ++q)
              for (int lh = 0; lh < 2; ++lh)
                for (int li = 0; li < 32; ++li) {
                  const int m = 32 * mb + li, g = m / 16, u = m % 16;
                  for (int e = 0; e < 8; ++e)
                    wsplit[o++] = planes[((size_t)q * 4 * C + (size_t)g * C + 16 * ub + u) * C + w * (C / 4) + 16 * s + 8 * lh + e];
                }
  }
  // planes 1 and 2 of a rounded matrix are zeros; wmencodec.pack_lstm_whh_plane = the slice q = 0 of the order above
  for (size_t i = whh.size(); i < planes.size(); ++i)
    if (planes[i]) { fprintf(stderr, "plane %zu of the rounded matrix is not zero\n", i / whh.size()); return 1; }
  std::vector<uint16_t> wone(whh.size());
  for (size_t blk = 0; blk < whh.size() / 512; ++blk) memcpy(&wone[blk * 512], &wsplit[blk * 3 * 512], 1024);
  Layer L[2];
  for (int l = 0; l < 2; ++l) {
    CK(hipMalloc(&L[l].gin, gin.size() * 4)); CK(hipMalloc(&L[l].whh_packed, packed.size() * 4)); CK(hipMalloc(&L[l].out, (size_t)B * T * C * 4));
    CK(hipMalloc(&L[l].hbuf, (size_t)2 * rows * C * 4)); CK(hipMalloc(&L[l].cbuf, (size_t)B * C * 4));
    CK(hipMalloc(&L[l].wsplit, wsplit.size() * 2)); CK(hipMalloc(&L[l].wone, wone.size() * 2)); CK(hipMalloc(&L[l].hsplit, (size_t)2 * nbg * 64 * C * 3 * 2));
    CK(hipMemcpy(L[l].gin, gin.data(), gin.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(L[l].whh_packed, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(L[l].wsplit, wsplit.data(), wsplit.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(L[l].wone, wone.data(), wone.size() * 2, hipMemcpyHostToDevice));
  }
  auto args = [&](int l, int arm) {
    ssrhip_lstm_args a = {};
    a.gin = L[l].gin; a.w_hh = L[l].whh_packed; a.out = L[l].out; a.hbuf = L[l].hbuf; a.cbuf = L[l].cbuf;
    a.B = B; a.T = T; a.C = C; a.gin_bstride = (int64_t)T * 4 * C; a.out_bstride = (int64_t)T * C; a.w_packed = 1;
    if (arm != WIDE) { a.w_split = arm == X3 ? L[l].wsplit : L[l].wone; a.hsplit = L[l].hsplit; }
    return a;
  };
  auto layer = [&](int l, int arm, hipStream_t s) {
    const ssrhip_lstm_args a = args(l, arm);
    if (arm == WIDE || arm == X3) { SK(ssrhip_lstm_layer(&a, s)); return; }
    if (arm == X1_D8) setenv("SSRHIP_LSTM_W1_DEPTH", "8", 1); else unsetenv("SSRHIP_LSTM_W1_DEPTH");       // read at every call
    const int rc = ssrhip_lstm_layer_w1(&a, s);
    unsetenv("SSRHIP_LSTM_W1_DEPTH");
    if (rc != 0) { fprintf(stderr, "ssrhip_lstm_layer_w1 answered %d: %s\n", rc, rc < 0 ? ssrhip_last_error() : "does not qualify"); exit(1); }
  };
  hipStream_t s0, s1;
  CK(hipStreamCreate(&s0)); CK(hipStreamCreate(&s1));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const bool have[NARMS] = {true, true, true, KS % 8 == 0};
  std::vector<float> res[NARMS];
  printf("B = %d, C = %d, T = %d steps (%d workgroups per step), W_hh rounded to bf16, %d rounds behind one untimed pass\n", B, C, T, (C / 16) * nbg, rounds);
  const int64_t n0 = ssrhip_lstm_w1_launches();
  for (int arm = 0; arm < NARMS; ++arm) {                                // untimed: warm, and the results that are compared
    if (!have[arm]) continue;
    layer(0, arm, s0); layer(1, arm, s1);
    CK(hipDeviceSynchronize());
    res[arm].resize((size_t)B * T * C);
    CK(hipMemcpy(res[arm].data(), L[0].out, res[arm].size() * 4, hipMemcpyDeviceToHost));
  }
  const int64_t counted = ssrhip_lstm_w1_launches() - n0;
  std::vector<float> alone[NARMS], both[NARMS];
  for (int r = 0; r < rounds; ++r)
    for (int i = 0; i < NARMS; ++i) {
      const int arm = r % 2 == 0 ? i : NARMS - 1 - i;
      if (!have[arm]) continue;
      float ms = 0;
      CK(hipDeviceSynchronize());
      CK(hipEventRecord(e0, s0));
      layer(0, arm, s0);
      CK(hipEventRecord(e1, s0));
      CK(hipEventSynchronize(e1));
      CK(hipEventElapsedTime(&ms, e0, e1));
      alone[arm].push_back(ms * 1e3f / T);
      CK(hipDeviceSynchronize());
      CK(hipEventRecord(e0, s0));
      CK(hipStreamWaitEvent(s1, e0, 0));
      layer(0, arm, s0);
      layer(1, arm, s1);                                                 // a second chain beside it, as the codec's two-layer pipeline has
      CK(hipEventRecord(e1, s1));
      CK(hipStreamWaitEvent(s0, e1, 0));
      CK(hipEventRecord(e1, s0));
      CK(hipEventSynchronize(e1));
      CK(hipEventElapsedTime(&ms, e0, e1));
      both[arm].push_back(ms * 1e3f / T);
    }
  auto median = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return v.size() % 2 ? v[v.size() / 2] : 0.5f * (v[v.size() / 2 - 1] + v[v.size() / 2]); };
  auto spread = [](const std::vector<float>& v) { return *std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end()); };
  std::string json = "JSON {\"B\": " + std::to_string(B) + ", \"C\": " + std::to_string(C) + ", \"T\": " + std::to_string(T) + ", \"rounds\": " + std::to_string(rounds);
  printf("| arm | us per step alone (spread) | with a second chain on another stream (spread) |\n|---|---|---|\n");
  for (int arm = 0; arm < NARMS; ++arm) {
    if (!have[arm]) continue;
    printf("| %s | %.2f (%.2f) | %.2f (%.2f) |\n", ARM_NAME[arm], median(alone[arm]), spread(alone[arm]), median(both[arm]), spread(both[arm]));
    char buf[256];
    snprintf(buf, sizeof buf, ", \"%s\": {\"alone_us\": %.3f, \"alone_spread\": %.3f, \"both_us\": %.3f, \"both_spread\": %.3f}", ARM_KEY[arm], median(alone[arm]),
             spread(alone[arm]), median(both[arm]), spread(both[arm]));
    json += buf;
  }
  bool same = memcmp(res[X1_D4].data(), res[X3].data(), res[X3].size() * 4) == 0;
  if (have[X1_D8]) same = same && memcmp(res[X1_D8].data(), res[X3].data(), res[X3].size() * 4) == 0;
  double worst = 0, mean = 0;
  for (size_t i = 0; i < res[WIDE].size(); ++i) { const double d = fabs((double)res[WIDE][i] - res[X3][i]); worst = d > worst ? d : worst; mean += d; }
  printf("one-plane outputs == three-plane outputs bit for bit over %d steps: %s; one-plane step launches counted in the untimed pass: %lld (%d expected)\n", T,
         same ? "yes" : "NO", (long long)counted, (have[X1_D8] ? 4 : 2) * T);
  printf("three planes against the fp32 pipe: max |diff| %.3g, mean %.3g (both carry fp32-level rounding; a layout bug shows as O(0.1))\n", worst, mean / res[WIDE].size());
  printf("%s, \"x1_equals_x3\": %s}\n", json.c_str(), same ? "true" : "false");
  return same ? 0 : 2;
}
