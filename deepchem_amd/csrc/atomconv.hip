// Atomic convolution (Gomes et al. 2017): the whole AtomicConvolution layer of the reference, fp32, 3-D coordinates.
//
// For sample b and atom slot n with the neighbour list nbrs[b, n, 0 .. M) and the neighbours' types z[b, n, 0 .. M):
//     D[m] = x[b, nbrs[m]] - x[b, n],   with a box  D -= rint(D / box) * box  (half to even),   R[m] = |D[m]|,
//     rsf(R, l) = exp(-re_l (R - rs_l)^2) * (R <= rc_l ? 0.5 (cos(pi R / rc_l) + 1) : 0),
//     row[a L + l] = sum over the m with z[m] == types[a] of rsf(R[m], l)        (without types: a = 0, the m with z[m] != 0),
//     y[b, n, c] = (row[c] - mean[n]) * invstd[n],  mean / unbiased variance of slot n over its B * C values.
// The reference materialises the (L, B, N, M) tensor of rsf, masks and reduces it once per type and normalises a
// (B, N, C) copy.  Here a row is rebuilt from its 3 M + 3 coordinates words, M indices and M types wherever it is needed,
// and the only (B, N, C) array is the output.
//
//   ac_stats_kernel    builds each row in LDS and leaves, per row, its mean and centred second moment in double, taken
//                      about the row's first value (so a row far from zero does not cancel).  The row is not written.
//   ac_finish_kernel   one thread per slot n: combines its B rows in index order in double about the first row's mean.
//   ac_fwd_kernel      rebuilds the row and writes it normalised, 64 consecutive floats per wave and instruction.
//   ac_bwd_kernel      recomputes R (in double), reads dy and accumulates, per lane and filter, the three sums of
//                      dy * invstd[n] * d rsf / d{rc, rs, re} in double over the rows of its workgroup in row order;
//   ac_bwd_finish      combines the workgroups, one wave per value, by a fixed tree.
//
// Layout: one wave per row (b, n), 4 rows per workgroup.  Lanes m < M compute R[m] and the type slot t[m] once per row
// (LDS, 8 bytes per neighbour); then the lanes run along the filters l, and lane l owns the columns a L + l of the
// row for every a: it zeroes them, adds into them neighbour by neighbour in list order and nobody else touches them, so
// the sums need no atomics and their order is the list's.  The row lives in (dynamic) LDS, C floats per wave: C <=
// GCMI_AC_MAX_CHANNELS = 2048 keeps a workgroup at 34 KiB (4 workgroups = 16 waves per CU) and below the 64 KiB a
// kernel may take without a raised limit.  The backward keeps two filters per lane in registers and takes the filters
// in chunks of 128 along gridDim.y.  A neighbour index outside [0, N) is compared with N before it is used and
// contributes nothing, like a neighbour whose type is in no slot; a neighbour whose distance is NaN (a zero box, NaN
// coordinates) makes its whole row NaN, as the reference's mask products do.  No float atomics; two runs agree bit for bit.
#include "common.h"

namespace gcmi {
namespace {

constexpr int kAcThreads = 256;
constexpr int kAcWaves = kAcThreads / 64;  // rows per workgroup
constexpr int kAcChunk = 128;              // filters per backward workgroup: two per lane
constexpr int kAcMaxParts = 1024;          // workgroups along the rows that leave a partial sum
constexpr double kPiD = 3.14159265358979323846;

template <typename T>
struct AcPairsT {  // per wave: what lanes m < M leave for the lanes along l (T: float forward, double backward)
  T R[kAcWaves][GCMI_AC_MAX_NEIGHBORS];
  int t[kAcWaves][GCMI_AC_MAX_NEIGHBORS];
  float types[GCMI_AC_MAX_TYPES];  // the table, where a dynamic index costs a read (load_types)
};
using AcPairs = AcPairsT<float>;

__device__ __forceinline__ bool inside(int i, int n) { return (unsigned)i < (unsigned)n; }

// The type table from the kernarg segment to LDS, once per workgroup (static indices there: a dynamic one would go
// through scratch); valid after the caller's next barrier
template <typename T>
__device__ __forceinline__ void load_types(const gcmi_ac_input& a, AcPairsT<T>& p) {
  if (threadIdx.x < GCMI_AC_MAX_TYPES) p.types[threadIdx.x] = pick_n(a.types, (int)threadIdx.x);
}

// The channel block of a neighbour of type z: the a with types[a] == z (the host refuses duplicates), -1 for none
template <typename T>
__device__ __forceinline__ int type_slot(int n_types, const AcPairsT<T>& p, float z) {
  if (n_types == 0) return z != 0.f ? 0 : -1;
  int t = -1;
#pragma unroll 1
  for (int k = 0; k < n_types; ++k) t = (z == p.types[k]) ? k : t;
  return t;
}

// R and the type slot of neighbour `lane` of row (b, n) = `row`; every lane of the wave calls it
template <typename T>
__device__ __forceinline__ void ac_pairs(const gcmi_ac_input& a, int row, bool valid, int wave, int lane, AcPairsT<T>& p) {
  if (lane >= a.M) return;
  T R = 0;
  int t = -1;
  if (valid) {
    const int b = row / a.N;  // (rows fit 32 bits: check_ac)
    const int j = a.nbrs[(int64_t)row * a.M + lane];
    if (inside(j, a.N)) {
      const float* xi = a.x + (int64_t)row * 3;
      const float* xj = a.x + ((int64_t)b * a.N + j) * 3;
      T d[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        d[k] = (T)xj[k] - (T)xi[k];
        if (a.has_box) d[k] -= rint(d[k] / (T)a.box[k]) * (T)a.box[k];
      }
      R = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      t = type_slot(a.n_types, p, a.z[(int64_t)row * a.M + lane]);
    }
  }
  p.R[wave][lane] = R;
  p.t[wave][lane] = t;
}

struct Filter {
  float rc, rs, re;
};
__device__ __forceinline__ Filter load_filter(const gcmi_ac_input& a, int l) { return {a.rc[l], a.rs[l], a.re[l]}; }

// (cos(pi R / rc) as cospif(R / rc): the argument is in [0, 1] wherever it is used, and cosf's large-argument reduction
// cost the forward kernel SGPR spills)
__device__ __forceinline__ float rsf(float R, const Filter& f) {
  if (!(R <= f.rc)) return 0.f;
  const float dr = R - f.rs;
  return expf(-f.re * (dr * dr)) * (0.5f * (cospif(R / f.rc) + 1.f));
}

// Builds the row of wave `wave` in LDS.  The caller has put a barrier after ac_pairs and puts one before the row is read
// across lanes.
__device__ __forceinline__ void ac_row(const gcmi_ac_input& a, int n_blocks, int wave, int lane, const AcPairs& p,
                                       float* __restrict__ row) {
  for (int l = lane; l < a.L; l += 64) {
    const Filter f = load_filter(a, l);
#pragma unroll 1
    for (int k = 0; k < n_blocks; ++k) row[k * a.L + l] = 0.f;
    for (int m = 0; m < a.M; ++m) {
      const int t = p.t[wave][m];  // (the same for every lane)
      const float R = p.R[wave][m];
      if (R != R) {  // the reference multiplies NaN by the masks: every block of the row is NaN
#pragma unroll 1
        for (int k = 0; k < n_blocks; ++k) row[k * a.L + l] += R;
        continue;
      }
      if (t < 0) continue;
      row[t * a.L + l] += rsf(R, f);
    }
  }
}

// The sum of v over the lanes of a wave by a fixed tree, valid in every lane
__device__ __forceinline__ double wave_sum_all(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- statistics
__global__ __launch_bounds__(kAcThreads) void ac_stats_kernel(gcmi_ac_input a, double* __restrict__ part) {
  extern __shared__ __align__(16) float ac_rows[];
  __shared__ AcPairs pairs;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_blocks = a.n_types > 0 ? a.n_types : 1, C = n_blocks * a.L;
  float* row = ac_rows + (int64_t)wave * C;
  const int rows = a.B * a.N;
  load_types(a, pairs);
  __syncthreads();
  for (int base = (int)blockIdx.x * kAcWaves; base < rows; base += (int)gridDim.x * kAcWaves) {
    const int r = base + wave;
    const bool valid = r < rows;
    ac_pairs(a, r, valid, wave, lane, pairs);
    __syncthreads();
    ac_row(a, n_blocks, wave, lane, pairs, row);
    __syncthreads();
    const float pivot = row[0];
    double s1 = 0.0, s2 = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double d = (double)(row[c] - pivot);
      s1 += d;
      s2 += d * d;
    }
    s1 = wave_sum_all(s1);
    s2 = wave_sum_all(s2);
    if (valid && lane == 0) {
      part[2 * (int64_t)r] = (double)pivot + s1 / (double)C;
      part[2 * (int64_t)r + 1] = fmax(s2 - s1 * s1 / (double)C, 0.0);
    }
    __syncthreads();
  }
}

// One thread per slot: the B rows in index order, moments about the first row's mean; every row counts C values
__global__ __launch_bounds__(kAcThreads) void ac_finish_kernel(const double* __restrict__ part, int B, int N, int C, float eps,
                                                               float2* __restrict__ stats) {
  const int n = (int)blockIdx.x * kAcThreads + (int)threadIdx.x;
  if (n >= N) return;
  const double ref = part[2 * (int64_t)n];
  double s1 = 0.0, s2 = 0.0;
  for (int b = 0; b < B; ++b) {
    const int64_t r = (int64_t)b * N + n;
    const double dm = part[2 * r] - ref;
    s1 += (double)C * dm;
    s2 += part[2 * r + 1] + (double)C * dm * dm;
  }
  const double count = (double)B * (double)C;  // >= 2: the host checked
  const double m2 = fmax(s2 - s1 * s1 / count, 0.0);
  stats[n] = make_float2((float)(ref + s1 / count), (float)(1.0 / sqrt(m2 / (count - 1.0) + (double)eps)));
}

// ---- forward
__global__ __launch_bounds__(kAcThreads) void ac_fwd_kernel(gcmi_ac_input a, const float2* __restrict__ stats,
                                                            float* __restrict__ out) {
  extern __shared__ __align__(16) float ac_rows[];
  __shared__ AcPairs pairs;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_blocks = a.n_types > 0 ? a.n_types : 1, C = n_blocks * a.L;
  float* row = ac_rows + (int64_t)wave * C;
  const int rows = a.B * a.N;
  load_types(a, pairs);
  __syncthreads();
  for (int base = (int)blockIdx.x * kAcWaves; base < rows; base += (int)gridDim.x * kAcWaves) {
    const int r = base + wave;
    const bool valid = r < rows;
    ac_pairs(a, r, valid, wave, lane, pairs);
    __syncthreads();
    ac_row(a, n_blocks, wave, lane, pairs, row);
    __syncthreads();
    if (valid) {
      const int n = r % a.N;
      const float2 st = stats[n];
      const float mu = st.x, is = st.y;
      float* dst = out + (int64_t)r * C;
#pragma unroll 1
      for (int c = lane; c < C; c += 64) dst[c] = (row[c] - mu) * is;
    }
    __syncthreads();
  }
}

// ---- backward: the gradients of rc, rs, re.  In double from the coordinates on: a gradient is one number summed over
// every pair of the batch, and float32 terms would leave it a few ulp off however they are added.
__global__ __launch_bounds__(kAcThreads) void ac_bwd_kernel(gcmi_ac_input a, const float2* __restrict__ stats,
                                                            const float* __restrict__ dy, double* __restrict__ part) {
  __shared__ AcPairsT<double> pairs;
  __shared__ double red[kAcWaves][6][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_blocks = a.n_types > 0 ? a.n_types : 1, C = n_blocks * a.L;
  const int l0 = (int)blockIdx.y * kAcChunk;
  double g[6];  // [filter of the lane][rc, rs, re]
#pragma unroll
  for (int i = 0; i < 6; ++i) g[i] = 0.0;
  double rc[2], rs[2], re[2];
  bool have[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int l = l0 + 64 * k + lane;
    have[k] = l < a.L;
    rc[k] = have[k] ? (double)a.rc[l] : 1.0;
    rs[k] = have[k] ? (double)a.rs[l] : 0.0;
    re[k] = have[k] ? (double)a.re[l] : 0.0;
  }
  const int rows = a.B * a.N;
  load_types(a, pairs);
  __syncthreads();
  for (int base = (int)blockIdx.x * kAcWaves; base < rows; base += (int)gridDim.x * kAcWaves) {
    const int r = base + wave;
    const bool valid = r < rows;
    ac_pairs(a, r, valid, wave, lane, pairs);
    __syncthreads();
    if (valid) {
      const double is = (double)stats[r % a.N].y;
      const float* src = dy + (int64_t)r * C;
      for (int m = 0; m < a.M; ++m) {
        const int t = pairs.t[wave][m];
        const double R = pairs.R[wave][m];
        if (R != R) {  // as the forward: NaN everywhere
#pragma unroll
          for (int i = 0; i < 6; ++i) g[i] += R;
          continue;
        }
        if (t < 0) continue;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (!have[k] || !(R <= rc[k])) continue;
          const double d = (double)src[t * a.L + l0 + 64 * k + lane] * is;
          const double dr = R - rs[k];
          const double K = exp(-re[k] * (dr * dr));
          const double q = R / rc[k];
          double sn, cs;
          sincospi(q, &sn, &cs);
          const double v = K * (0.5 * (cs + 1.0));
          g[3 * k + 0] += d * (K * (0.5 * sn) * (kPiD * q) / rc[k]);
          g[3 * k + 1] += d * (v * (2.0 * re[k] * dr));
          g[3 * k + 2] -= d * (v * (dr * dr));
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) red[wave][i][lane] = g[i];
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int l = l0 + 64 * k + lane;
    if (l >= a.L) continue;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      double s = red[0][3 * k + q][lane];
      for (int w = 1; w < kAcWaves; ++w) s += red[w][3 * k + q][lane];
      part[((int64_t)blockIdx.x * 3 + q) * a.L + l] = s;
    }
  }
}

// grad[j], j in [0, 3 L): the sum over the workgroups; lane i takes the workgroups i, i + 64, ... in order
__global__ __launch_bounds__(kAcThreads) void ac_bwd_finish_kernel(const double* __restrict__ part, int n_part, int L,
                                                                   float* __restrict__ grad) {
  const int j = (int)blockIdx.x * kAcWaves + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= 3 * L) return;  // (the whole wave)
  double s = 0.0;
  for (int b = lane; b < n_part; b += 64) s += part[(int64_t)b * 3 * L + j];
  s = wave_sum_all(s);
  if (lane == 0) grad[j] = (float)s;
}

// ---- host side
int row_grid(int64_t rows) { return grid_for(rows, kAcWaves); }
int part_grid(int64_t rows) { return std::min(row_grid(rows), kAcMaxParts); }
int channels(const gcmi_ac_input* a) { return (a->n_types > 0 ? a->n_types : 1) * a->L; }
size_t row_bytes(const gcmi_ac_input* a) { return (size_t)kAcWaves * channels(a) * sizeof(float); }

int64_t workspace_floats(int64_t B, int64_t N, int64_t L) {
  const int64_t doubles = std::max(2 * B * N, (int64_t)part_grid(B * N) * 3 * L);
  return 2 * doubles;
}

int check_ac(const char* what, const gcmi_ac_input* a) {
  GCMI_CHECK_ARG(a != nullptr, "%s: NULL input description", what);
  GCMI_CHECK_ARG(a->B > 0 && a->N > 0 && (int64_t)a->B * a->N < ((int64_t)1 << 31) / GCMI_AC_MAX_NEIGHBORS,
                 "%s: B %d, N %d (both positive, B * N * %d below 2^31)", what, a->B, a->N, GCMI_AC_MAX_NEIGHBORS);
  GCMI_CHECK_ARG(a->M >= 1 && a->M <= GCMI_AC_MAX_NEIGHBORS, "%s: M %d is not in [1, %d]", what, a->M, GCMI_AC_MAX_NEIGHBORS);
  GCMI_CHECK_ARG(a->d == 3, "%s: d %d, the kernels take 3 coordinates", what, a->d);
  GCMI_CHECK_ARG(a->n_types >= 0 && a->n_types <= GCMI_AC_MAX_TYPES, "%s: %d atom types, at most %d", what, a->n_types,
                 GCMI_AC_MAX_TYPES);
  GCMI_CHECK_ARG(a->L >= 1 && channels(a) <= GCMI_AC_MAX_CHANNELS && a->L <= GCMI_AC_MAX_CHANNELS,
                 "%s: L %d with %d type blocks: the row must hold 1 .. %d channels", what, a->L, a->n_types > 0 ? a->n_types : 1,
                 GCMI_AC_MAX_CHANNELS);
  for (int i = 0; i < a->n_types; ++i)
    for (int j = 0; j < i; ++j)
      GCMI_CHECK_ARG(!(a->types[i] == a->types[j]), "%s: atom type %g stands twice in the list", what, (double)a->types[i]);
  GCMI_CHECK_ARG(a->x && a->nbrs && a->z && a->rc && a->rs && a->re, "%s: NULL x / nbrs / z / rc / rs / re", what);
  GCMI_CHECK_ARG(aligned4(a->x) && aligned4(a->nbrs) && aligned4(a->z) && aligned4(a->rc) && aligned4(a->rs) && aligned4(a->re),
                 "%s: x / nbrs / z / rc / rs / re must be 4-byte aligned", what);
  GCMI_CHECK_ARG(a->has_box == 0 || a->has_box == 1, "%s: has_box %d is not 0 or 1", what, a->has_box);
  return GCMI_OK;
}

int check_ac_workspace(const char* what, const gcmi_ac_input* a, const float* ws, int64_t ws_floats) {
  const int64_t need = workspace_floats(a->B, a->N, a->L);
  GCMI_CHECK_ARG(ws && aligned16(ws) && ws_floats >= need,
                 "%s: the workspace is NULL, not 16-byte aligned, or holds %lld floats of the %lld needed", what,
                 (long long)ws_floats, (long long)need);
  return GCMI_OK;
}

}  // namespace
}  // namespace gcmi

using namespace gcmi;

#define AC_TRY(expr)                  \
  do {                                \
    const int rc__ = (expr);          \
    if (rc__ != GCMI_OK) return rc__; \
  } while (0)

extern "C" {

int64_t gcmi_ac_workspace_floats(int32_t B, int32_t N, int32_t L) {
  if (B <= 0 || N <= 0 || L <= 0 || L > GCMI_AC_MAX_CHANNELS) return -1;
  return workspace_floats(B, N, L);
}

int gcmi_ac_stats(const gcmi_ac_input* in, float eps, float* d_stats, float* d_workspace, int64_t workspace_floats_,
                  void* stream) {
  const char* what = "ac_stats";
  AC_TRY(check_ac(what, in));
  GCMI_CHECK_ARG((int64_t)in->B * channels(in) >= 2, "%s: a slot needs at least 2 values, B * C = %lld", what,
                 (long long)in->B * channels(in));
  GCMI_CHECK_ARG(d_stats && aligned8(d_stats), "%s: NULL or misaligned statistics", what);
  GCMI_CHECK_ARG(eps >= 0.f, "%s: eps %g is negative", what, (double)eps);
  AC_TRY(check_ac_workspace(what, in, d_workspace, workspace_floats_));
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(d_workspace);
  const int64_t rows = (int64_t)in->B * in->N;
  hipLaunchKernelGGL(ac_stats_kernel, dim3(row_grid(rows)), dim3(kAcThreads), row_bytes(in), st, *in, part);
  hipLaunchKernelGGL(ac_finish_kernel, dim3(grid_for(in->N, kAcThreads)), dim3(kAcThreads), 0, st, part, in->B, in->N,
                     channels(in), eps, reinterpret_cast<float2*>(d_stats));
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

int gcmi_ac_fwd(const gcmi_ac_input* in, const float* d_stats, float* d_out, void* stream) {
  const char* what = "ac_fwd";
  AC_TRY(check_ac(what, in));
  GCMI_CHECK_ARG(d_stats && aligned8(d_stats), "%s: NULL or misaligned statistics", what);
  GCMI_CHECK_ARG(d_out && aligned4(d_out), "%s: NULL or misaligned output", what);
  const int64_t rows = (int64_t)in->B * in->N;
  hipLaunchKernelGGL(ac_fwd_kernel, dim3(row_grid(rows)), dim3(kAcThreads), row_bytes(in), static_cast<hipStream_t>(stream),
                     *in, reinterpret_cast<const float2*>(d_stats), d_out);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

int gcmi_ac_bwd(const gcmi_ac_input* in, const float* d_stats, const float* d_dy, float* d_grad, float* d_workspace,
                int64_t workspace_floats_, void* stream) {
  const char* what = "ac_bwd";
  AC_TRY(check_ac(what, in));
  GCMI_CHECK_ARG(d_stats && aligned8(d_stats), "%s: NULL or misaligned statistics", what);
  GCMI_CHECK_ARG(d_dy && aligned4(d_dy), "%s: NULL or misaligned dy", what);
  GCMI_CHECK_ARG(d_grad && aligned4(d_grad), "%s: NULL or misaligned gradient", what);
  AC_TRY(check_ac_workspace(what, in, d_workspace, workspace_floats_));
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(d_workspace);
  const int parts = part_grid((int64_t)in->B * in->N);
  hipLaunchKernelGGL(ac_bwd_kernel, dim3(parts, (in->L + kAcChunk - 1) / kAcChunk), dim3(kAcThreads), 0, st, *in,
                     reinterpret_cast<const float2*>(d_stats), d_dy, part);
  hipLaunchKernelGGL(ac_bwd_finish_kernel, dim3((3 * in->L + kAcWaves - 1) / kAcWaves), dim3(kAcThreads), 0, st, part, parts,
                     in->L, d_grad);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

}  // extern "C"
