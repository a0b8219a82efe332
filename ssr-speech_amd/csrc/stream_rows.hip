// stream_rows.hip — the batched watermarked stream's row mover (DESIGN.md Part I.29): ONE launch executes a table of up to
// SSRHIP_STREAM_ROWS_MAX_OPS row operations on fp32 buffers — zero `rows` rows of `width` floats, or copy them from a source whose row
// step may be negative (a reflected edge is a copy that walks its source backwards). Per poll the stream has a handful of such pieces per
// item (the zero rows in front of a short prompt, an ended item's right edge, the tap cores, the output cores); as torch calls they are
// B small kernels each, here they are one launch per stage whatever B is. A translation unit of its own: no other kernel's code moves.
//
// Exact by construction: the kernel loads and stores, nothing else. Every store is a per-lane global store (a 16-byte one on the vector
// path, 4-byte ones on the scalar path).
#include "common.h"

namespace {

constexpr int ROWS_THREADS = 256;

// One unit = up to four consecutive floats of one row; a row has (width + 3) / 4 of them. The vector path moves a unit as ONE float4:
// every row of the op starts on a 16-byte boundary and is a whole number of units. The same rule on the host (the grid) and on the
// device (the path), from the same fields.
__host__ __device__ inline bool rows_op_vec(const ssrhip_rows_op& o) {
  bool v = o.width % 4 == 0 && ((uintptr_t)o.dst & 15) == 0 && o.dst_ld % 4 == 0;
  if (o.mode != 0) v = v && ((uintptr_t)o.src & 15) == 0 && o.src_ld % 4 == 0;
  return v;
}

struct rows_prefix {
  int first[SSRHIP_STREAM_ROWS_MAX_OPS + 1];           // first[i] = the first workgroup of op i; first[n_ops] = the grid
};

// grid = sum over the ops of ceil(rows * units per row / ROWS_THREADS): a flat index over (op, row, unit). The workgroup finds its op
// in the prefix table (a uniform scan of at most 64 kernel-argument words), the lane its row and unit. The launcher sized the grid
// from the host copy of the table; the lane reads the device copy and returns where that copy has fewer rows than the grid assumed.
__global__ __launch_bounds__(ROWS_THREADS) void stream_rows_kernel(const ssrhip_rows_op* __restrict__ ops, int n_ops, const rows_prefix pre) {
  const int wg = blockIdx.x;
  int i = 0;
  while (i + 1 < n_ops && pre.first[i + 1] <= wg) ++i;
  const ssrhip_rows_op o = ops[i];
  if (o.rows <= 0 || o.width <= 0) return;
  const long upr = (o.width + 3) / 4;
  const long unit = (long)(wg - pre.first[i]) * ROWS_THREADS + threadIdx.x;
  if (unit >= (long)o.rows * upr) return;
  const long r = unit / upr;
  const int c = (int)(unit % upr) * 4;
  float* d = o.dst + r * o.dst_ld + c;
  const float* s = o.mode != 0 ? o.src + r * o.src_ld + c : nullptr;
  if (rows_op_vec(o)) {
    *reinterpret_cast<float4*>(d) = s ? *reinterpret_cast<const float4*>(s) : make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    const int n = min(4, o.width - c);
    for (int j = 0; j < n; ++j) d[j] = s ? s[j] : 0.f;
  }
}

// the bounding byte interval [lo, hi) of the addresses an op touches through one of its pointers
inline void rows_span(const float* p, long ld, int rows, int width, uintptr_t* lo, uintptr_t* hi) {
  const long last = (long)(rows - 1) * ld;
  const float* a = p + (last < 0 ? last : 0);
  const float* b = p + (last > 0 ? last : 0) + width;
  *lo = (uintptr_t)a;
  *hi = (uintptr_t)b;
}

}  // namespace

extern "C" int ssrhip_stream_rows_sizeof(void) { return (int)sizeof(ssrhip_rows_op); }

extern "C" int ssrhip_stream_rows(const ssrhip_rows_op* ops_host, const ssrhip_rows_op* ops_dev, int32_t n_ops, ssrhip_stream_t stream) {
  SSR_REQUIRE(n_ops >= 0 && n_ops <= SSRHIP_STREAM_ROWS_MAX_OPS, "ssrhip_stream_rows: %d ops (at most %d per launch)", n_ops,
              SSRHIP_STREAM_ROWS_MAX_OPS);
  SSR_REQUIRE(n_ops == 0 || (ops_host && ops_dev), "ssrhip_stream_rows: null argument");
  rows_prefix pre;
  uintptr_t dlo[SSRHIP_STREAM_ROWS_MAX_OPS], dhi[SSRHIP_STREAM_ROWS_MAX_OPS], slo[SSRHIP_STREAM_ROWS_MAX_OPS], shi[SSRHIP_STREAM_ROWS_MAX_OPS];
  long total = 0;
  for (int i = 0; i < n_ops; ++i) {
    const ssrhip_rows_op& o = ops_host[i];
    SSR_REQUIRE(o.rows >= 0 && o.width >= 0, "ssrhip_stream_rows: op %d has the negative count rows=%d / width=%d", i, o.rows, o.width);
    SSR_REQUIRE(o.mode == 0 || o.mode == 1, "ssrhip_stream_rows: op %d has mode %d (0 = zero, 1 = copy)", i, o.mode);
    pre.first[i] = (int)total;
    dlo[i] = dhi[i] = slo[i] = shi[i] = 0;
    if (o.rows == 0 || o.width == 0) continue;
    SSR_REQUIRE(o.dst && (o.mode == 0 || o.src), "ssrhip_stream_rows: op %d has a null pointer", i);
    const long step = o.dst_ld < 0 ? -o.dst_ld : o.dst_ld;
    SSR_REQUIRE(o.rows == 1 || step >= o.width, "ssrhip_stream_rows: op %d writes rows of %d floats %ld apart", i, o.width, (long)o.dst_ld);
    rows_span(o.dst, o.dst_ld, o.rows, o.width, &dlo[i], &dhi[i]);
    if (o.mode != 0) rows_span(o.src, o.src_ld, o.rows, o.width, &slo[i], &shi[i]);
    const long units = (long)o.rows * ((o.width + 3) / 4);
    total += (units + ROWS_THREADS - 1) / ROWS_THREADS;
    SSR_REQUIRE(total <= 0x7fffffffL, "ssrhip_stream_rows: op %d brings the launch to %ld workgroups", i, total);
  }
  pre.first[n_ops] = (int)total;
  for (int i = 0; i < n_ops; ++i) {                    // (bounding intervals: two ops that interleave their rows count as overlapping)
    if (dhi[i] == dlo[i]) continue;
    for (int j = 0; j < n_ops; ++j) {
      SSR_REQUIRE(j <= i || dhi[j] == dlo[j] || dhi[i] <= dlo[j] || dhi[j] <= dlo[i], "ssrhip_stream_rows: ops %d and %d overlap in dst", i, j);
      SSR_REQUIRE(shi[j] == slo[j] || dhi[i] <= slo[j] || shi[j] <= dlo[i], "ssrhip_stream_rows: op %d writes what op %d reads", i, j);
    }
  }
  if (total == 0) return 0;                            // every op is empty
  hipLaunchKernelGGL(stream_rows_kernel, dim3((unsigned)total), dim3(ROWS_THREADS), 0, (hipStream_t)stream, ops_dev, n_ops, pre);
  SSR_LAUNCH_CHECK();
  return 0;
}
