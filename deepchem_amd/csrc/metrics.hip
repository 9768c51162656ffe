// Validation metrics on the predictions where they sit in HBM (deepchem/metrics/metric.py:568-727).
//   gcmi_metric_rank: per-task ROC-AUC / area under the precision-recall curve.  Nothing is filtered, so every task is
//     a fixed segment of exactly n elements:
//       rank_keys_kernel     task-major (key, row) pairs; key = bitwise complement of the order-preserving 32-bit image
//                            of the fp32 score (-0.0 mapped to +0.0), so an ascending sort walks scores downwards
//       4 x { radix_hist_kernel, radix_offsets_kernel, radix_scatter_kernel }
//                            stable LSD radix sort, 8-bit digits, ping-pong buffers, grid = (tiles per segment, tasks)
//       rank_scan_kernel     one workgroup per task walks its sorted segment in chunks with a carried state: inclusive
//                            scans of positives and negatives (int64 counts unweighted, fp64 sums weighted), tie-group
//                            tails where the key changes, the sums at the previous tail carried by a max-scan (the
//                            cumulative sums are monotone), one contribution per tie group
//   gcmi_metric_moments: per-task shifted first and second moments, absolute and squared error, accuracy count, in one
//     pass over (n, T).
// No allocation inside: the sort's buffers are the caller's workspace.
#include <math.h>

#include "common.h"

namespace gcmi {

constexpr int kRadixBits = 8;
constexpr int kRadix = 1 << kRadixBits;
constexpr int kSortBlock = 256;
constexpr int kSortTile = 2048;  // elements of one segment that one workgroup histograms and scatters
constexpr int kScanBlock = 1024;
constexpr int kScanWaves = kScanBlock / 64;

struct RankWorkspace {
  uint32_t* keys[2];
  uint32_t* rows[2];
  uint32_t* hist;  // [task][digit][tile]
  int64_t tiles;
};

inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

inline int64_t rank_tiles(int64_t n) { return (n + kSortTile - 1) / kSortTile; }

inline RankWorkspace carve(void* ws, int64_t n, int32_t n_tasks) {
  RankWorkspace r;
  char* p = (char*)ws;
  const int64_t seg = align16(n * n_tasks * (int64_t)sizeof(uint32_t));
  r.keys[0] = (uint32_t*)p;
  r.keys[1] = (uint32_t*)(p + seg);
  r.rows[0] = (uint32_t*)(p + 2 * seg);
  r.rows[1] = (uint32_t*)(p + 3 * seg);
  r.hist = (uint32_t*)(p + 4 * seg);
  r.tiles = rank_tiles(n);
  return r;
}

// ---------------------------------------------------------------------------------------------- keys
__global__ void __launch_bounds__(kSortBlock)
rank_keys_kernel(const float* __restrict__ scores, int64_t row_stride, int64_t elem_stride, int64_t n, int n_tasks,
                 uint32_t* __restrict__ keys, uint32_t* __restrict__ rows, int32_t* __restrict__ status) {
  const int t = blockIdx.y;
  for (int64_t r = (int64_t)blockIdx.x * kSortBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kSortBlock) {
    const float s = scores[r * row_stride + t * elem_stride];
    uint32_t u = __float_as_uint(s);
    if (s != s) atomicOr(&status[t], 2);
    if (isinf(s)) atomicOr(&status[t], 4);
    if (u == 0x80000000u) u = 0u;                              // -0.0 ranks with +0.0
    const uint32_t up = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending image of the score
    keys[(int64_t)t * n + r] = ~up;                            // descending
    rows[(int64_t)t * n + r] = (uint32_t)r;
  }
}

// ---------------------------------------------------------------------------------------------- radix sort
__global__ void __launch_bounds__(kSortBlock)
radix_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int shift, int64_t tiles, uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[kRadix];
  const int t = blockIdx.y;
  const int64_t tile = blockIdx.x;
  bins[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t* seg = keys + (int64_t)t * n;
  const int64_t lo = tile * kSortTile;
  const int64_t hi = lo + kSortTile < n ? lo + kSortTile : n;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kSortBlock) atomicAdd(&bins[(seg[i] >> shift) & (kRadix - 1)], 1u);
  __syncthreads();
  hist[((int64_t)t * kRadix + threadIdx.x) * tiles + tile] = bins[threadIdx.x];
}

// counts [digit][tile] of one task -> where each (digit, tile) run starts in the sorted segment
__global__ void __launch_bounds__(kRadix)
radix_offsets_kernel(uint32_t* __restrict__ hist, int64_t tiles) {
  __shared__ uint32_t total[kRadix];
  uint32_t* mine = hist + ((int64_t)blockIdx.x * kRadix + threadIdx.x) * tiles;
  uint32_t sum = 0;
  for (int64_t b = 0; b < tiles; ++b) sum += mine[b];
  total[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int d = 0; d < kRadix; ++d) {
      const uint32_t c = total[d];
      total[d] = run;
      run += c;
    }
  }
  __syncthreads();
  uint32_t run = total[threadIdx.x];
  for (int64_t b = 0; b < tiles; ++b) {
    const uint32_t c = mine[b];
    mine[b] = run;
    run += c;
  }
}

__global__ void __launch_bounds__(kSortBlock)
radix_scatter_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ rows_in, int64_t n, int shift,
                     int64_t tiles, const uint32_t* __restrict__ hist, uint32_t* __restrict__ keys_out,
                     uint32_t* __restrict__ rows_out) {
  constexpr int kWaves = kSortBlock / 64;
  __shared__ uint32_t next[kRadix];            // where the next element with this digit goes
  __shared__ uint32_t wave_count[kWaves][kRadix];
  const int t = blockIdx.y;
  const int64_t tile = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  next[threadIdx.x] = hist[((int64_t)t * kRadix + threadIdx.x) * tiles + tile];
#pragma unroll
  for (int w = 0; w < kWaves; ++w) wave_count[w][threadIdx.x] = 0;
  __syncthreads();
  const int64_t seg0 = (int64_t)t * n;
  const int64_t lo = tile * kSortTile;
  const int64_t hi = lo + kSortTile < n ? lo + kSortTile : n;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int64_t base = lo; base < hi; base += kSortBlock) {  // rounds in order keep the sort stable
    const int64_t i = base + threadIdx.x;
    const bool live = i < hi;
    uint32_t key = 0, row = 0, digit = 0;
    if (live) {
      key = keys_in[seg0 + i];
      row = rows_in[seg0 + i];
      digit = (key >> shift) & (kRadix - 1);
    }
    // the lanes of this wave that hold the same digit
    unsigned long long peers = __ballot(live);
#pragma unroll
    for (int b = 0; b < kRadixBits; ++b) {
      const unsigned long long has = __ballot(live && ((digit >> b) & 1u));
      peers &= ((digit >> b) & 1u) ? has : ~has;
    }
    const uint32_t rank_in_wave = __popcll(peers & below);
    if (live && rank_in_wave == 0) wave_count[wave][digit] = __popcll(peers);
    __syncthreads();
    if (live) {
      uint32_t pos = next[digit] + rank_in_wave;
      for (int w = 0; w < wave; ++w) pos += wave_count[w][digit];
      if (pos < n) {  // always, for consistent counts; a guard against writing outside the segment
        keys_out[seg0 + pos] = key;
        rows_out[seg0 + pos] = row;
      }
    }
    __syncthreads();
    {
      uint32_t add = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        add += wave_count[w][threadIdx.x];
        wave_count[w][threadIdx.x] = 0;
      }
      next[threadIdx.x] += add;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------- scan
template <typename S>
__device__ __forceinline__ S shfl_up_t(S v, int o) {
  return __shfl_up(v, o);
}
template <typename S>
__device__ __forceinline__ S shfl_down_t(S v, int o) {
  return __shfl_down(v, o);
}

struct AddOp {
  template <typename S>
  __device__ __forceinline__ S operator()(S a, S b) const { return a + b; }
};
struct MaxOp {
  template <typename S>
  __device__ __forceinline__ S operator()(S a, S b) const { return a > b ? a : b; }
};

// inclusive scan over the workgroup's threads, values >= 0 (identity 0 for both operations); *total = the last thread's
template <typename S, typename Op>
__device__ __forceinline__ S block_scan(S v, Op op, S* wave_tot, S* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const S u = shfl_up_t(v, o);
    if (lane >= o) v = op(v, u);
  }
  __syncthreads();  // wave_tot free again
  if (lane == 63) wave_tot[wave] = v;
  __syncthreads();
  S pre = 0;
  for (int w = 0; w < wave; ++w) pre = op(pre, wave_tot[w]);
  S all = pre;
  for (int w = wave; w < kScanWaves; ++w) all = op(all, wave_tot[w]);
  *total = all;
  return op(pre, v);
}

template <typename S>
__device__ __forceinline__ S block_sum_t(S v, S* wave_tot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += shfl_down_t(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = v;
  __syncthreads();
  S t = 0;
  for (int w = 0; w < kScanWaves; ++w) t += wave_tot[w];
  return t;
}

// S = long long: unweighted (counts); S = double: weighted (sums of weights)
template <typename S, bool kWeighted>
__global__ void __launch_bounds__(kScanBlock)
rank_scan_kernel(int which, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ rows, int64_t n, int n_tasks,
                 const double* __restrict__ labels, double positive, const float* __restrict__ weights,
                 double* __restrict__ out, int32_t* __restrict__ status) {
  __shared__ S wave_tot[kScanWaves];
  __shared__ S seen_p[kScanBlock], seen_n[kScanBlock];
  const int t = blockIdx.x;
  const uint32_t* kseg = keys + (int64_t)t * n;
  const uint32_t* rseg = rows + (int64_t)t * n;
  S carry_p = 0, carry_n = 0;  // sums over everything before this chunk
  S tail_p = 0, tail_n = 0;    // sums at the last tie-group tail before this chunk
  S roc_acc = 0;               // this thread's share of  sum over groups  neg_g * (P_before + P_through)
  double prc_acc = 0.0;        //                         sum over groups  dTP_g * (prec_g + prec_before) / 2
  for (int64_t base = 0; base < n; base += kScanBlock) {
    const int64_t i = base + threadIdx.x;
    const bool live = i < n;
    S p = 0, q = 0;
    bool tail = false;
    if (live) {
      const uint32_t key = kseg[i];
      const int64_t at = (int64_t)rseg[i] * n_tasks + t;
      const S w = kWeighted ? (S)weights[at] : (S)1;
      const bool is_pos = labels[at] == positive;
      p = is_pos ? w : (S)0;
      q = is_pos ? (S)0 : w;
      tail = (i + 1 == n) || kseg[i + 1] != key;
    }
    S tot_p, tot_n, chunk_tail_p, chunk_tail_n;
    const S cum_p = carry_p + block_scan(p, AddOp(), wave_tot, &tot_p);
    const S cum_n = carry_n + block_scan(q, AddOp(), wave_tot, &tot_n);
    // the sums at the nearest tail at or before each element, then the one strictly before it
    const S at_tail_p = block_scan(tail ? cum_p : (S)0, MaxOp(), wave_tot, &chunk_tail_p);
    const S at_tail_n = block_scan(tail ? cum_n : (S)0, MaxOp(), wave_tot, &chunk_tail_n);
    // (a tail sees its own sums there: the tail before an element is what the thread before it sees)
    __syncthreads();
    seen_p[threadIdx.x] = at_tail_p;
    seen_n[threadIdx.x] = at_tail_n;
    __syncthreads();
    const S before_p = threadIdx.x == 0 ? (S)0 : seen_p[threadIdx.x - 1];
    const S before_n = threadIdx.x == 0 ? (S)0 : seen_n[threadIdx.x - 1];
    const S prev_p = before_p > tail_p ? before_p : tail_p;
    const S prev_n = before_n > tail_n ? before_n : tail_n;
    if (tail) {
      if (which == GCMI_METRIC_ROC_AUC) {
        roc_acc += (cum_n - prev_n) * (prev_p + cum_p);
      } else {
        const double tp = (double)cum_p, ps = (double)cum_p + (double)cum_n;
        const double tp0 = (double)prev_p, ps0 = (double)prev_p + (double)prev_n;
        const double prec = ps > 0.0 ? tp / ps : 0.0;
        const double prec0 = ps0 > 0.0 ? tp0 / ps0 : 1.0;  // the curve starts at (recall 0, precision 1)
        prc_acc += (tp - tp0) * (prec + prec0) * 0.5;
      }
    }
    carry_p += tot_p;
    carry_n += tot_n;
    tail_p = chunk_tail_p > tail_p ? chunk_tail_p : tail_p;
    tail_n = chunk_tail_n > tail_n ? chunk_tail_n : tail_n;
  }
  const S roc = block_sum_t(roc_acc, wave_tot);
  __shared__ double wave_tot_d[kScanWaves];
  const double prc = block_sum_t(prc_acc, wave_tot_d);
  if (threadIdx.x == 0) {
    const double P = (double)carry_p, N = (double)carry_n;
    if (!(P > 0.0) || !(N > 0.0)) {
      atomicOr(&status[t], 1);
      out[t] = 0.0;
    } else if (which == GCMI_METRIC_ROC_AUC) {
      out[t] = (double)roc / (2.0 * P * N);
    } else {
      out[t] = prc / P;
    }
  }
}

// ---------------------------------------------------------------------------------------------- moments
constexpr int kMomBlock = 256;
constexpr int kMomSums = 9;  // [0..7] of the header's layout and the accuracy sum

// x * scale + shift in two roundings, as the host's z * std + mean.  (__dmul_rn / __dadd_rn are a plain `*` and `+` in
// HIP's headers and contract into one fma under hipcc's default -ffp-contract=fast: one rounding, an ulp off the host.)
__device__ __forceinline__ double affine_two_roundings(double x, double scale, double shift) {
#pragma clang fp contract(off)
  const double m = x * scale;
  return m + shift;
}

__global__ void __launch_bounds__(kMomBlock)
moments_kernel(int which, const float* __restrict__ pred, int64_t row_stride, int64_t elem_stride, int n_classes,
               const double* __restrict__ labels, const float* __restrict__ weights, const double* __restrict__ scale,
               const double* __restrict__ shift, int64_t n, int n_tasks, int lanes_t, double* __restrict__ out) {
  __shared__ double red[kMomBlock];
  const int tx = threadIdx.x % lanes_t, ty = threadIdx.x / lanes_t, rows_per_pass = kMomBlock / lanes_t;
  const int t = blockIdx.x * lanes_t + tx;
  const bool live_t = t < n_tasks;
  double acc[kMomSums];
#pragma unroll
  for (int k = 0; k < kMomSums; ++k) acc[k] = 0.0;
  double y0 = 0.0, p0 = 0.0;
  if (live_t) {
    const double sc = scale ? scale[t] : 1.0, sh = shift ? shift[t] : 0.0;
    y0 = labels[t];
    if (which == GCMI_METRIC_MOMENTS) p0 = affine_two_roundings((double)pred[t * elem_stride], sc, sh);
    for (int64_t r = (int64_t)blockIdx.y * rows_per_pass + ty; r < n; r += (int64_t)gridDim.y * rows_per_pass) {
      const double y = labels[r * n_tasks + t];
      const double w = weights ? (double)weights[r * n_tasks + t] : 1.0;
      const float* x = pred + r * row_stride + t * elem_stride;
      acc[0] += w;
      if (which == GCMI_METRIC_MOMENTS) {
        const double p = affine_two_roundings((double)x[0], sc, sh);
        const double dy = y - y0, dp = p - p0, e = y - p;
        acc[1] += w * dy;
        acc[2] += w * dp;
        acc[3] += w * dy * dy;
        acc[4] += w * dp * dp;
        acc[5] += w * dy * dp;
        acc[6] += w * fabs(e);
        acc[7] += w * e * e;
      } else {
        int best = 0;
        float top = x[0];
        for (int c = 1; c < n_classes; ++c)
          if (x[c] > top) {  // the first maximum on ties (np.argmax)
            top = x[c];
            best = c;
          }
        if ((double)best == y) acc[8] += w;
      }
    }
  }
  // rows of the workgroup -> one value per task -> one atomic per (workgroup, task, sum)
  for (int k = 0; k < kMomSums; ++k) {
    __syncthreads();
    red[threadIdx.x] = acc[k];
    __syncthreads();
    if (ty == 0 && live_t) {
      double s = 0.0;
      for (int j = 0; j < rows_per_pass; ++j) s += red[j * lanes_t + tx];
      double* o = out + (int64_t)t * GCMI_METRIC_MOMENT_DOUBLES;
      atomicAdd(&o[k == 8 ? 10 : k], s);
      if (k == 0 && blockIdx.y == 0) {
        o[8] = y0;
        o[9] = p0;
      }
    }
  }
}

}  // namespace gcmi

using namespace gcmi;

extern "C" {

int64_t gcmi_metrics_workspace_bytes(int64_t n, int32_t n_tasks) {
  if (n <= 0 || n_tasks <= 0) return 0;
  const int64_t seg = align16(n * n_tasks * (int64_t)sizeof(uint32_t));
  return 4 * seg + align16((int64_t)n_tasks * kRadix * rank_tiles(n) * (int64_t)sizeof(uint32_t));
}

int gcmi_metric_rank(int32_t which, const float* d_scores, int64_t row_stride, int64_t elem_stride,
                     const double* d_labels, int32_t positive, const float* d_weights, int64_t n, int32_t n_tasks,
                     double* d_out, int32_t* d_status, void* d_workspace, void* stream) {
  GCMI_CHECK_ARG(which == GCMI_METRIC_ROC_AUC || which == GCMI_METRIC_PRC_AUC, "metric_rank: which must be 0 (ROC) or 1 (PRC)");
  GCMI_CHECK_ARG(n > 0 && n < ((int64_t)1 << 31) && n_tasks > 0 && n_tasks <= 65535, "metric_rank: bad shape");
  GCMI_CHECK_ARG(row_stride >= 0 && elem_stride >= 0, "metric_rank: negative stride");
  GCMI_CHECK_ARG(d_scores && d_labels && d_out && d_status && d_workspace, "metric_rank: NULL buffer");
  GCMI_CHECK_ARG(aligned16(d_workspace), "metric_rank: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  RankWorkspace ws = carve(d_workspace, n, n_tasks);
  if (hipMemsetAsync(d_status, 0, sizeof(int32_t) * n_tasks, st) != hipSuccess) {
    set_error("metric_rank: memset failed");
    return GCMI_ERR_LAUNCH;
  }
  const int64_t tiles = ws.tiles;
  GCMI_CHECK_ARG(tiles < ((int64_t)1 << 31), "metric_rank: too many rows");
  const int key_blocks = (int)std::min<int64_t>((n + kSortBlock - 1) / kSortBlock, 1024);
  hipLaunchKernelGGL(rank_keys_kernel, dim3(key_blocks, n_tasks), dim3(kSortBlock), 0, st, d_scores, row_stride,
                     elem_stride, n, n_tasks, ws.keys[0], ws.rows[0], d_status);
  GCMI_CHECK_LAUNCH("rank_keys");
  int cur = 0;
  for (int pass = 0; pass < 32 / kRadixBits; ++pass) {
    const int shift = pass * kRadixBits;
    hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)tiles, n_tasks), dim3(kSortBlock), 0, st, ws.keys[cur], n, shift,
                       tiles, ws.hist);
    GCMI_CHECK_LAUNCH("radix_hist");
    hipLaunchKernelGGL(radix_offsets_kernel, dim3(n_tasks), dim3(kRadix), 0, st, ws.hist, tiles);
    GCMI_CHECK_LAUNCH("radix_offsets");
    hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)tiles, n_tasks), dim3(kSortBlock), 0, st, ws.keys[cur],
                       ws.rows[cur], n, shift, tiles, ws.hist, ws.keys[cur ^ 1], ws.rows[cur ^ 1]);
    GCMI_CHECK_LAUNCH("radix_scatter");
    cur ^= 1;
  }
  if (d_weights)
    hipLaunchKernelGGL((rank_scan_kernel<double, true>), dim3(n_tasks), dim3(kScanBlock), 0, st, which, ws.keys[cur],
                       ws.rows[cur], n, n_tasks, d_labels, (double)positive, d_weights, d_out, d_status);
  else
    hipLaunchKernelGGL((rank_scan_kernel<long long, false>), dim3(n_tasks), dim3(kScanBlock), 0, st, which, ws.keys[cur],
                       ws.rows[cur], n, n_tasks, d_labels, (double)positive, d_weights, d_out, d_status);
  GCMI_CHECK_LAUNCH("rank_scan");
  return GCMI_OK;
}

int gcmi_metric_moments(int32_t which, const float* d_pred, int64_t row_stride, int64_t elem_stride, int32_t n_classes,
                        const double* d_labels, const float* d_weights, const double* d_scale, const double* d_shift,
                        int64_t n, int32_t n_tasks, double* d_out, void* stream) {
  GCMI_CHECK_ARG(which == GCMI_METRIC_MOMENTS || which == GCMI_METRIC_ACCURACY,
                 "metric_moments: which must be 0 (moments) or 1 (accuracy)");
  GCMI_CHECK_ARG(n > 0 && n_tasks > 0, "metric_moments: bad shape");
  GCMI_CHECK_ARG(which == GCMI_METRIC_MOMENTS || n_classes >= 1, "metric_moments: accuracy needs n_classes >= 1");
  GCMI_CHECK_ARG(row_stride >= 0 && elem_stride >= 0, "metric_moments: negative stride");
  GCMI_CHECK_ARG(d_pred && d_labels && d_out, "metric_moments: NULL buffer");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_out, 0, sizeof(double) * GCMI_METRIC_MOMENT_DOUBLES * n_tasks, st) != hipSuccess) {
    set_error("metric_moments: memset failed");
    return GCMI_ERR_LAUNCH;
  }
  int lanes_t = 1;  // threads of a workgroup along the tasks: the power of two at or above n_tasks, at most 64
  while (lanes_t < n_tasks && lanes_t < 64) lanes_t <<= 1;
  const int rows_per_pass = kMomBlock / lanes_t;
  const int task_blocks = (n_tasks + lanes_t - 1) / lanes_t;
  const int row_blocks = (int)std::min<int64_t>((n + rows_per_pass - 1) / rows_per_pass, 64);
  hipLaunchKernelGGL(moments_kernel, dim3(task_blocks, row_blocks), dim3(kMomBlock), 0, st, which, d_pred, row_stride,
                     elem_stride, n_classes, d_labels, d_weights, d_scale, d_shift, n, n_tasks, lanes_t, d_out);
  GCMI_CHECK_LAUNCH("metric_moments");
  return GCMI_OK;
}

}  // extern "C"
