// Lattice convolution (LCNN, Lym et al. 2019): everything of one LCNNBlock behind its one product, fp32.
//
// The reference's block gathers, per site v and permutation p, the K neighbour rows x[nbr[v, p, j]] into one row of
// K * F floats, applies Linear(K * F, O), a BatchNorm1d(O) PER SITE over the P permutation rows, a dropout mask of P
// values per site and the sum over p.  With conv_weights.weight split by neighbour slot into K blocks W_j (O, F) and
//     Y = x [W_0; ...; W_{K-1}]^T            (N rows of K * O floats: one product),
//     X[v, p, :] = b + sum_j Y[nbr[v, p, j], j, :]
// the (N, P, K * F) tensor never exists and the product is P times smaller.
//
//   lc_site_fwd   one site per row group: gathers the P * K pieces of Y, keeps the P rows of X in registers, takes the
//                 mean and the biased variance over p in-lane (training) or the given statistics (eval), applies gamma,
//                 beta and the mask, sums over p; optionally writes X (N, P, O) for the backward and lc_running.
//   lc_site_bwd   from X, dOut, the mask and gamma: the BatchNorm backward over p in-lane (training) or the scale alone
//                 (eval), dX (N, P, O), and per-workgroup column sums of dgamma, dbeta and db in double;
//                 lc_sums_finish adds the workgroups in double in a fixed order (one wave per value, a fixed tree).
//   lc_rev_sum    dY[u, j, :] = the sum of dX[v, p, :] over the list of (v, p) with nbr[v, p, j] = u, in list order:
//                 one owner per output row, a zero row for an empty list.  Lists are NOT chunked.
//   lc_running    the running statistics after the N per-site updates of the reference, in closed form:
//                 r_N = (1 - m)^N r_0 + m sum_v (1 - m)^(N - 1 - v) s_v, weights and sums in double, fixed order.
//
// Layout: one channel per lane, so a row of O floats takes O consecutive lanes (any O in [1, 64], no padding, no
// alignment beyond 4 bytes) and a workgroup of 256 threads floor(256 / O) rows.  A lane owns its channel for all P rows
// of a site: the statistics over p need no cross-lane step and no LDS.  No atomics, one owner per output element, every
// sum in an order the sizes alone fix: two runs agree bit for bit.  Every index read from the device is compared with
// the sizes the host passed before it is used.
#include "common.h"

namespace gcmi {
namespace {

constexpr int kLcThreads = 256;
constexpr int kLcMaxP = GCMI_LC_MAX_PERM;
constexpr int kLcSums = 3;         // dgamma, dbeta, db
constexpr int kLcMaxParts = 1024;  // workgroups of lc_site_bwd: few enough for a short finish, enough to fill the device
// lc_running: sites further back than this from the last one are skipped.  Their weight is m (1 - m)^k with
// (1 - m) <= 0.9 (checked by the entry): 0.9^k < 2^-311 for k >= 2048, so even a statistic at the top of the float32
// range (2^128), summed over the geometric tail (a factor 10 < 2^4), stays below 2^-179: under a quarter of the
// smallest float32 denormal (2^-149), whatever the result is.
constexpr int kLcRunWindow = 2048;

__device__ __forceinline__ bool inside(int i, int n) { return (unsigned)i < (unsigned)n; }

// Which row and channel of a launch over rows of O floats this thread takes: channel c of row r of the floor(256 / O)
// rows its workgroup takes per turn (threads past them idle).
struct Lanes {
  int rpb, r, c;
  bool active;
  __device__ __forceinline__ explicit Lanes(int O) {
    rpb = kLcThreads / O;
    r = (int)threadIdx.x / O;
    c = (int)threadIdx.x - r * O;
    active = r < rpb;
  }
};

struct LcNorm {  // vectors of O floats.  mean == nullptr: the statistics of each site over its P rows (training)
  const float *gamma, *beta, *mean, *var;
  float eps;
};

// Eval mode: 1 / sqrt(var + eps) in double and xhat through it.  An error of a float32 invstd is the same in every term
// of a column and does not average out of the column sums; one double rsqrt per lane and two double operations per
// element cost nothing beside the gather.
__device__ __forceinline__ double eval_invstd(const LcNorm& n, int c) { return 1.0 / sqrt((double)n.var[c] + (double)n.eps); }
__device__ __forceinline__ float eval_xhat(float x, float mean, double invstd) {
  return (float)(((double)x - (double)mean) * invstd);
}

// mean and 1 / sqrt(biased variance + eps) of x[0 .. P)
__device__ __forceinline__ void site_stats(const float (&x)[kLcMaxP], int P, float eps, float& mean, float& invstd) {
  float s = 0.f;
#pragma unroll
  for (int p = 0; p < kLcMaxP; ++p)
    if (p < P) s += x[p];
  mean = s / (float)P;
  float m2 = 0.f;
#pragma unroll
  for (int p = 0; p < kLcMaxP; ++p)
    if (p < P) m2 += (x[p] - mean) * (x[p] - mean);
  invstd = 1.f / sqrtf(m2 / (float)P + eps);
}

// ---- forward
__global__ __launch_bounds__(kLcThreads) void lc_site_fwd_kernel(gcmi_lc_batch b, const float* __restrict__ y, int64_t ldy,
                                                                const float* __restrict__ bias, LcNorm nrm,
                                                                const float* __restrict__ mask, float* __restrict__ out,
                                                                int64_t ldo, float* __restrict__ xs) {
  const int O = b.O, P = b.P, K = b.K;
  const Lanes w(O);
  if (!w.active) return;
  const float bc = bias ? bias[w.c] : 0.f, gamma = nrm.gamma[w.c], beta = nrm.beta[w.c];
  const bool train = nrm.mean == nullptr;
  float mean = train ? 0.f : nrm.mean[w.c], invstd = 1.f;
  const double invstd_d = train ? 1.0 : eval_invstd(nrm, w.c);
  for (int64_t base = (int64_t)blockIdx.x * w.rpb; base < b.n_sites; base += (int64_t)gridDim.x * w.rpb) {
    const int64_t v = base + w.r;
    if (v >= b.n_sites) continue;
    const int32_t* nb = b.nbr + v * (int64_t)(P * K);
    float x[kLcMaxP];
#pragma unroll
    for (int p = 0; p < kLcMaxP; ++p) {
      x[p] = bc;
      if (p < P) {
        for (int j = 0; j < K; ++j) {
          const int u = nb[p * K + j];  // (the same address in every lane of the row: one transaction)
          if (inside(u, b.n_sites)) x[p] += y[(int64_t)u * ldy + j * O + w.c];
        }
      }
    }
    if (train) site_stats(x, P, nrm.eps, mean, invstd);
    float acc = 0.f;
#pragma unroll
    for (int p = 0; p < kLcMaxP; ++p) {
      if (p < P) {
        const float m = mask ? mask[v * P + p] : 1.f;
        const float xh = train ? (x[p] - mean) * invstd : eval_xhat(x[p], mean, invstd_d);
        acc += m * (xh * gamma + beta);
        if (xs) xs[(v * P + p) * O + w.c] = x[p];
      }
    }
    out[v * ldo + w.c] = acc;
  }
}

// ---- backward
// The sum of v over the lanes of a wave by a fixed tree; valid in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__global__ __launch_bounds__(kLcThreads) void lc_site_bwd_kernel(gcmi_lc_batch b, const float* __restrict__ xs,
                                                                const float* __restrict__ dout, int64_t lddo,
                                                                const float* __restrict__ mask, LcNorm nrm,
                                                                float* __restrict__ dxs, double* __restrict__ part) {
  const int O = b.O, P = b.P;
  const Lanes w(O);
  // every term is formed and added in double: the column sums then carry the rounding of xhat and dX alone, not of a
  // float32 product per term and a float32 partial sum per site as well
  double sums[kLcSums] = {0.0, 0.0, 0.0};
  if (w.active) {
    const float gamma = nrm.gamma[w.c];
    const bool train = nrm.mean == nullptr;
    float mean = train ? 0.f : nrm.mean[w.c], invstd = 1.f;
    const double invstd_d = train ? 1.0 : eval_invstd(nrm, w.c);
    const float a_eval = (float)((double)gamma * invstd_d);
    for (int64_t base = (int64_t)blockIdx.x * w.rpb; base < b.n_sites; base += (int64_t)gridDim.x * w.rpb) {
      const int64_t v = base + w.r;
      if (v >= b.n_sites) continue;
      float x[kLcMaxP];
#pragma unroll
      for (int p = 0; p < kLcMaxP; ++p) x[p] = p < P ? xs[(v * P + p) * O + w.c] : 0.f;
      if (train) site_stats(x, P, nrm.eps, mean, invstd);
      const float go = dout[v * lddo + w.c];
      // dy[p] = mask[p] * dOut; dxhat[p] = dy[p] * gamma
      float dy[kLcMaxP], s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int p = 0; p < kLcMaxP; ++p) {
        dy[p] = 0.f;
        if (p < P) {
          x[p] = train ? (x[p] - mean) * invstd : eval_xhat(x[p], mean, invstd_d);  // xhat
          const float m = mask ? mask[v * P + p] : 1.f;
          dy[p] = m * go;
          s1 += dy[p];
          s2 += dy[p] * x[p];
          const double dyd = (double)m * (double)go;  // (exact)
          sums[0] += dyd * (double)x[p];  // dgamma
          sums[1] += dyd;                 // dbeta
        }
      }
      const float c1 = train ? s1 / (float)P : 0.f, c2 = train ? s2 / (float)P : 0.f, a = train ? gamma * invstd : a_eval;
#pragma unroll
      for (int p = 0; p < kLcMaxP; ++p) {
        if (p < P) {
          const float dx = a * ((dy[p] - c1) - x[p] * c2);
          dxs[(v * P + p) * O + w.c] = dx;
          if (train) sums[2] += (double)dx;  // db
        }
      }
    }
    // eval: dX = (gamma * invstd) dy exactly, so db is that factor times dbeta, in double; the sum of the float32 dX
    // would carry one rounding per term and the rounding of the factor, the same in every term, on top
    if (!train) sums[2] = (double)gamma * invstd_d * sums[1];
  }
  // over the rows of the workgroup, rows in order; valid in the threads of row 0
  __shared__ double red[kLcSums][kLcThreads];
#pragma unroll
  for (int i = 0; i < kLcSums; ++i) red[i][threadIdx.x] = sums[i];
  __syncthreads();
  if ((int)threadIdx.x < O) {
    for (int rr = 1; rr < w.rpb; ++rr) {
#pragma unroll
      for (int i = 0; i < kLcSums; ++i) sums[i] += red[i][rr * O + threadIdx.x];
    }
    double* row = part + (int64_t)blockIdx.x * (kLcSums * O);
#pragma unroll
    for (int i = 0; i < kLcSums; ++i) row[i * O + threadIdx.x] = sums[i];
  }
}

// sums[j] = the sum over the workgroups of their value j, in double: one wave per value, lane l takes the workgroups
// l, l + 64, ... in order, the lanes are combined by a fixed tree
__global__ __launch_bounds__(kLcThreads) void lc_sums_finish_kernel(const double* __restrict__ part, int n_part, int n_values,
                                                                   float* __restrict__ sums) {
  const int j = (int)blockIdx.x * (kLcThreads / 64) + (int)threadIdx.x / 64, lane = threadIdx.x & 63;
  if (j >= n_values) return;  // (the whole wave)
  double sum = 0.0;
  for (int p = lane; p < n_part; p += 64) sum += part[(int64_t)p * n_values + j];
  sum = wave_sum(sum);
  if (lane == 0) sums[j] = (float)sum;
}

// dY[u, j, :] = the sum of dX over the list of (u, j); rows of the launch are the N * K pairs (u, j)
__global__ __launch_bounds__(kLcThreads) void lc_rev_sum_kernel(gcmi_lc_batch b, const float* __restrict__ dxs,
                                                               float* __restrict__ dy, int64_t lddy) {
  const int O = b.O, K = b.K;
  const Lanes w(O);
  if (!w.active) return;
  const int64_t n_rows = (int64_t)b.n_sites * K, n_list = (int64_t)b.n_sites * b.P * K, n_src = (int64_t)b.n_sites * b.P;
  for (int64_t base = (int64_t)blockIdx.x * w.rpb; base < n_rows; base += (int64_t)gridDim.x * w.rpb) {
    const int64_t row = base + w.r;
    if (row >= n_rows) continue;
    int64_t lo = b.rev_ptr[row], hi = b.rev_ptr[row + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_list ? n_list : hi;
    float acc = 0.f;
    for (int64_t k = lo; k < hi; ++k) {
      const int64_t s = b.rev_row[k];
      if (s >= 0 && s < n_src) acc += dxs[s * O + w.c];
    }
    const int64_t u = row / K;
    const int j = (int)(row - u * K);
    dy[u * lddy + j * O + w.c] = acc;
  }
}

// One workgroup per channel.  Thread t takes the sites N - 1 - k for k = t, t + 256, ... < min(N, kLcRunWindow) in that
// order, the threads are combined by a fixed tree in LDS.
__global__ __launch_bounds__(kLcThreads) void lc_running_kernel(gcmi_lc_batch b, const float* __restrict__ xs, double momentum,
                                                               float* __restrict__ running_mean,
                                                               float* __restrict__ running_var,
                                                               int64_t* __restrict__ batches_tracked) {
  const int O = b.O, P = b.P, c = blockIdx.x, tid = threadIdx.x;
  if (c == 0 && tid == 0 && batches_tracked) *batches_tracked += b.n_sites;
  const int n = b.n_sites < kLcRunWindow ? b.n_sites : kLcRunWindow;
  const double keep = 1.0 - momentum;
  double sm = 0.0, sv = 0.0;
  for (int k = tid; k < n; k += kLcThreads) {
    const int64_t v = (int64_t)b.n_sites - 1 - k;
    float x[kLcMaxP], s = 0.f, m2 = 0.f;
#pragma unroll
    for (int p = 0; p < kLcMaxP; ++p) {
      x[p] = p < P ? xs[(v * P + p) * O + c] : 0.f;
      s += x[p];
    }
    const float mean = s / (float)P;
#pragma unroll
    for (int p = 0; p < kLcMaxP; ++p)
      if (p < P) m2 += (x[p] - mean) * (x[p] - mean);
    const double wk = momentum * pow(keep, (double)k);
    sm += wk * (double)mean;
    sv += wk * (double)(m2 / (float)(P - 1));
  }
  __shared__ double red[2][kLcThreads];
  red[0][tid] = sm;
  red[1][tid] = sv;
  __syncthreads();
  for (int off = kLcThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      red[0][tid] += red[0][tid + off];
      red[1][tid] += red[1][tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double k0 = pow(keep, (double)b.n_sites);
    running_mean[c] = (float)(k0 * (double)running_mean[c] + red[0][0]);
    running_var[c] = (float)(k0 * (double)running_var[c] + red[1][0]);
  }
}

// ---- host side
int rows_per_wg(int O) { return kLcThreads / O; }
int grid_rows(int64_t n_rows, int O) { return grid_for(n_rows, rows_per_wg(O)); }
int grid_parts(int64_t n_rows, int O) { return std::min(grid_rows(n_rows, O), kLcMaxParts); }
int64_t workspace_floats(int32_t n_sites, int32_t O) { return 2 * (int64_t)grid_parts(n_sites, O) * kLcSums * O; }

bool rows_ok(const void* p, int64_t ld, int width) { return p && aligned4(p) && ld >= width; }
bool vec_ok(const void* p) { return p && aligned4(p); }

int check_lc(const char* what, const gcmi_lc_batch* b, bool need_rev) {
  GCMI_CHECK_ARG(b != nullptr, "%s: NULL batch", what);
  GCMI_CHECK_ARG(b->O >= 1 && b->O <= GCMI_LC_MAX_WIDTH, "%s: O %d is outside [1, %d]", what, b->O, GCMI_LC_MAX_WIDTH);
  GCMI_CHECK_ARG(b->P >= GCMI_LC_MIN_PERM && b->P <= GCMI_LC_MAX_PERM, "%s: P %d is outside [%d, %d]", what, b->P,
                 GCMI_LC_MIN_PERM, GCMI_LC_MAX_PERM);
  GCMI_CHECK_ARG(b->K >= 1 && b->K <= GCMI_LC_MAX_SLOTS, "%s: K %d is outside [1, %d]", what, b->K, GCMI_LC_MAX_SLOTS);
  GCMI_CHECK_ARG(b->n_sites > 0 && (int64_t)b->n_sites * b->P * b->K * GCMI_LC_MAX_WIDTH < INT32_MAX,
                 "%s: n_sites %d must be positive with n_sites * P * K * %d below 2^31", what, b->n_sites, GCMI_LC_MAX_WIDTH);
  GCMI_CHECK_ARG(b->nbr != nullptr && aligned4(b->nbr), "%s: NULL or misaligned neighbour table", what);
  GCMI_CHECK_ARG(!need_rev || (b->rev_ptr && b->rev_row && aligned4(b->rev_ptr) && aligned4(b->rev_row)),
                 "%s: NULL or misaligned reverse lists", what);
  return GCMI_OK;
}

int check_norm(const char* what, const float* gamma, const float* beta, const float* mean, const float* var, float eps) {
  GCMI_CHECK_ARG(vec_ok(gamma) && (beta == nullptr || aligned4(beta)), "%s: NULL or misaligned gamma / beta", what);
  GCMI_CHECK_ARG((mean == nullptr) == (var == nullptr), "%s: mean and var go together", what);
  GCMI_CHECK_ARG(mean == nullptr || (aligned4(mean) && aligned4(var)), "%s: misaligned mean / var", what);
  GCMI_CHECK_ARG(eps > 0.f, "%s: eps %g must be positive", what, (double)eps);
  return GCMI_OK;
}

}  // namespace
}  // namespace gcmi

using namespace gcmi;

#define LC_TRY(expr)                  \
  do {                                \
    const int rc__ = (expr);          \
    if (rc__ != GCMI_OK) return rc__; \
  } while (0)

extern "C" {

int64_t gcmi_lc_workspace_floats(int32_t n_sites, int32_t O) {
  if (n_sites < 0 || O < 1 || O > GCMI_LC_MAX_WIDTH) return -1;
  return workspace_floats(n_sites, O);
}

int gcmi_lc_site_fwd(const gcmi_lc_batch* b, const float* d_y, int64_t ldy, const float* d_bias, const float* d_gamma,
                     const float* d_beta, const float* d_mean, const float* d_var, float eps, const float* d_mask,
                     float* d_out, int64_t ldo, float* d_x, void* stream) {
  const char* what = "lc_site_fwd";
  LC_TRY(check_lc(what, b, false));
  GCMI_CHECK_ARG(rows_ok(d_y, ldy, b->K * b->O) && (int64_t)b->n_sites * ldy < INT32_MAX,
                 "%s: bad Y (NULL, misaligned, ldy < K * O = %d, or n_sites * ldy past 2^31)", what, b->K * b->O);
  GCMI_CHECK_ARG(d_bias == nullptr || aligned4(d_bias), "%s: misaligned bias", what);
  LC_TRY(check_norm(what, d_gamma, d_beta, d_mean, d_var, eps));
  GCMI_CHECK_ARG(d_beta != nullptr, "%s: NULL beta", what);
  GCMI_CHECK_ARG(d_mask == nullptr || aligned4(d_mask), "%s: misaligned mask", what);
  GCMI_CHECK_ARG(rows_ok(d_out, ldo, b->O) && d_out != d_y, "%s: bad output (NULL, Y itself, misaligned, or ldo < %d)", what,
                 b->O);
  GCMI_CHECK_ARG(d_x == nullptr || (aligned4(d_x) && d_x != d_y && d_x != d_out), "%s: bad X (misaligned, or Y or the output itself)",
                 what);
  const LcNorm n = {d_gamma, d_beta, d_mean, d_var, eps};
  hipLaunchKernelGGL(lc_site_fwd_kernel, dim3(grid_rows(b->n_sites, b->O)), dim3(kLcThreads), 0,
                     static_cast<hipStream_t>(stream), *b, d_y, ldy, d_bias, n, d_mask, d_out, ldo, d_x);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

int gcmi_lc_site_bwd(const gcmi_lc_batch* b, const float* d_x, const float* d_dout, int64_t lddo, const float* d_mask,
                     const float* d_gamma, const float* d_mean, const float* d_var, float eps, float* d_dx, float* d_sums,
                     float* d_workspace, int64_t workspace_floats_, void* stream) {
  const char* what = "lc_site_bwd";
  LC_TRY(check_lc(what, b, false));
  GCMI_CHECK_ARG(d_x && aligned4(d_x), "%s: NULL or misaligned X", what);
  GCMI_CHECK_ARG(rows_ok(d_dout, lddo, b->O), "%s: bad dOut (NULL, misaligned, or lddo < %d)", what, b->O);
  GCMI_CHECK_ARG(d_mask == nullptr || aligned4(d_mask), "%s: misaligned mask", what);
  LC_TRY(check_norm(what, d_gamma, nullptr, d_mean, d_var, eps));
  GCMI_CHECK_ARG(d_dx && aligned4(d_dx) && d_dx != d_x && d_dx != d_dout, "%s: bad dX (NULL, misaligned, or one of the inputs)",
                 what);
  GCMI_CHECK_ARG(d_sums && aligned4(d_sums), "%s: NULL or misaligned sums", what);
  GCMI_CHECK_ARG(d_workspace && aligned16(d_workspace) && workspace_floats_ >= workspace_floats(b->n_sites, b->O),
                 "%s: the workspace is NULL, not 16-byte aligned, or holds %lld floats of the %lld needed", what,
                 (long long)workspace_floats_, (long long)workspace_floats(b->n_sites, b->O));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LcNorm n = {d_gamma, nullptr, d_mean, d_var, eps};
  const int parts = grid_parts(b->n_sites, b->O);
  double* part = reinterpret_cast<double*>(d_workspace);
  hipLaunchKernelGGL(lc_site_bwd_kernel, dim3(parts), dim3(kLcThreads), 0, st, *b, d_x, d_dout, lddo, d_mask, n, d_dx, part);
  GCMI_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(lc_sums_finish_kernel, dim3((kLcSums * b->O + 3) / 4), dim3(kLcThreads), 0, st, part, parts, kLcSums * b->O,
                     d_sums);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

int gcmi_lc_rev_sum(const gcmi_lc_batch* b, const float* d_dx, float* d_dy, int64_t lddy, void* stream) {
  const char* what = "lc_rev_sum";
  LC_TRY(check_lc(what, b, true));
  GCMI_CHECK_ARG(d_dx && aligned4(d_dx), "%s: NULL or misaligned dX", what);
  GCMI_CHECK_ARG(rows_ok(d_dy, lddy, b->K * b->O) && d_dy != d_dx && (int64_t)b->n_sites * lddy < INT32_MAX,
                 "%s: bad dY (NULL, dX itself, misaligned, lddy < K * O = %d, or n_sites * lddy past 2^31)", what, b->K * b->O);
  hipLaunchKernelGGL(lc_rev_sum_kernel, dim3(grid_rows((int64_t)b->n_sites * b->K, b->O)), dim3(kLcThreads), 0,
                     static_cast<hipStream_t>(stream), *b, d_dx, d_dy, lddy);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

int gcmi_lc_running(const gcmi_lc_batch* b, const float* d_x, float momentum, float* d_running_mean, float* d_running_var,
                    int64_t* d_batches_tracked, void* stream) {
  const char* what = "lc_running";
  LC_TRY(check_lc(what, b, false));
  GCMI_CHECK_ARG(d_x && aligned4(d_x), "%s: NULL or misaligned X", what);
  GCMI_CHECK_ARG(momentum >= 0.1f && momentum <= 1.f, "%s: momentum %g is outside [0.1, 1] (the window of sites is derived for it)",
                 what, (double)momentum);
  GCMI_CHECK_ARG(vec_ok(d_running_mean) && vec_ok(d_running_var), "%s: NULL or misaligned running_mean / running_var", what);
  GCMI_CHECK_ARG(d_batches_tracked == nullptr || aligned8(d_batches_tracked), "%s: misaligned batches_tracked", what);
  hipLaunchKernelGGL(lc_running_kernel, dim3(b->O), dim3(kLcThreads), 0, static_cast<hipStream_t>(stream), *b, d_x,
                     (double)momentum, d_running_mean, d_running_var, d_batches_tracked);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

}  // extern "C"
