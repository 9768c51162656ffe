// Molecule Attention Transformer: the per-batch bias and the pad-free attention of one (molecule, head), both directions.
//
// A batch is the concatenation of its molecules' atoms (atom_off [n_mols + 1]); pair data is stored per molecule as
// row-major n x n blocks (pair_off [n_mols + 1] = the exclusive sums of n^2).  No pad atom exists, so no mask does.
//
//     B[i][j] = lambda_distance * g(D)[i][j] + lambda_adjacency * A[i][j] / (sum_j A[i][j] + eps)     (gcmi_mat_bias)
//     O       = (lambda_attention * softmax(Q K^T / sqrt(d_k)) + B) V                                  per (molecule, head)
//
// g is the row softmax of -D (row minimum subtracted) or the elementwise exp(-D).  B depends on neither head nor layer:
// once per batch.  Q, K, V are row-major (atoms, ld) with head h in columns [h d_k, (h + 1) d_k); O and the gradients
// are written in that layout too, so nothing is transposed or made contiguous afterwards.
//
// Layout of the attention kernels.  fp32 VALU: molecules have tens of atoms, a 32 x 32 matrix-core tile would be mostly
// padding and fp32 accuracy would need the six-product split on top.  One workgroup of ceil(n_max / 64) waves per
// (molecule, head), n_max = the largest molecule of the batch; lane i owns query row i (and, in the backward's second
// half, key column i).  LDS (dynamic, sized by n_max): two row tiles X, Y of n_max x (d_k + 4) floats, filled with
// coalesced 16-byte reads (the pitch keeps a wave's own-row ds_read_b128 on 64 distinct banks; the inner loops read ONE
// row in all lanes, which broadcasts), the n x n tile T with an odd pitch (row walks and column walks both
// conflict-free) and n row sums.  Forward: X = K, Y = V (one tile when the pointers alias).  Backward: the attention
// matrix is recomputed into T; the row-owned half (dP = dO V^T, delta, dS, dQ = dS K) runs against X = K, Y = V, then
// X and Y are refilled with Q and dO (nothing to refill when Q = K = V: X holds the one tensor, Y holds dO from the
// start) for the column-owned half (dK = dS^T Q, dV = W^T dO), which walks T down its columns.  dP is recomputed
// where it is needed a second time instead of being kept in a second n x n tile: 2 row tiles + T fit the 160 KiB of a
// CU at 128 atoms and d_k = 64 (136 192 bytes), three would not.  No atomics: every output element has one owner.
// Sums over atoms run in atom order; the two scalar ones per row (softmax denominator, delta) are compensated (comp_add).
#include <math.h>

#include "common.h"

namespace gcmi {
namespace {

constexpr int kMatMaxAtoms = GCMI_MAT_MAX_ATOMS;
constexpr int kMatBiasThreads = 256;

struct MatArgs {
  const float *q, *k, *v;  // rows of ld floats (every leading dimension here: rows x ld < 2^31, checked by the host)
  int32_t ld;
  const float* bias;
  const int32_t *atom_off, *pair_off;
  int32_t n_mols, n_heads, dk, n_max;
  int32_t n_atoms;  // = atom_off[n_mols] as the host validated it: what the kernels bound their indices by
  int64_t n_pairs;
  float lambda_att, inv_sqrt_dk;
  float* o;  // forward
  int32_t ldo;
  const float* dO;  // backward
  int32_t lddo;
  float *dq, *dkk, *dv;
  int32_t ldg;
  int32_t shared;
};

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void axpy4(float4& y, float a, const float4& x) {
  y.x = fmaf(a, x.x, y.x); y.y = fmaf(a, x.y, y.y); y.z = fmaf(a, x.z, y.z); y.w = fmaf(a, x.w, y.w);
}

// What a workgroup knows about its (molecule, head); ok = false (uniform): nothing to do, or offsets that would leave
// the buffers (the host validated ITS copy of the offsets; the device copy is only trusted inside these bounds)
struct MatBlock {
  int a0, n, col0, nv;
  int64_t p0;
  bool ok;
};
__device__ __forceinline__ MatBlock mat_block(const MatArgs& a) {
  MatBlock b;
  const int mol = blockIdx.x / a.n_heads, head = blockIdx.x - mol * a.n_heads;
  b.a0 = a.atom_off[mol];
  b.n = a.atom_off[mol + 1] - b.a0;
  b.p0 = a.pair_off[mol];
  b.col0 = head * a.dk;
  b.nv = a.dk >> 2;
  b.ok = b.n > 0 && b.n <= a.n_max && b.a0 >= 0 && b.a0 + b.n <= a.n_atoms && b.p0 >= 0 &&
         b.p0 + (int64_t)b.n * b.n <= a.n_pairs;
  return b;
}

// rows [0, n) x 4 NV columns of src (its columns past 4 nv read as zero) -> tile, pitch 4 NV + 4
template <int NV>
__device__ __forceinline__ void stage_rows(float* tile, const float* src, int ld, int n, int nv) {
  constexpr int RP = 4 * NV + 4;
  for (int f = threadIdx.x; f < n * NV; f += blockDim.x) {
    const int r = f / NV, c = f - r * NV;
    const float4 x = c < nv ? *reinterpret_cast<const float4*>(src + r * ld + 4 * c) : f4zero();
    *reinterpret_cast<float4*>(tile + r * RP + 4 * c) = x;
  }
}
template <int NV>
__device__ __forceinline__ void load_row(float4 (&x)[NV], const float* row, int nv) {
#pragma unroll
  for (int c = 0; c < NV; ++c) x[c] = c < nv ? *reinterpret_cast<const float4*>(row + 4 * c) : f4zero();
}
template <int NV>
__device__ __forceinline__ float dot_row(const float4 (&x)[NV], const float* lds_row) {
  // four running sums, as a vectorised dot product has them
  float4 s = f4zero();
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const float4 y = *reinterpret_cast<const float4*>(lds_row + 4 * c);
    s.x = fmaf(x[c].x, y.x, s.x); s.y = fmaf(x[c].y, y.y, s.y); s.z = fmaf(x[c].z, y.z, s.z); s.w = fmaf(x[c].w, y.w, s.w);
  }
  return (s.x + s.y) + (s.z + s.w);
}
template <int NV>
__device__ __forceinline__ void axpy_row(float4 (&y)[NV], float a, const float* lds_row) {
#pragma unroll
  for (int c = 0; c < NV; ++c) axpy4(y[c], a, *reinterpret_cast<const float4*>(lds_row + 4 * c));
}
template <int NV, bool ADD>
__device__ __forceinline__ void store_row(float* row, const float4 (&x)[NV], int nv) {
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    if (c < nv) {
      float4* p = reinterpret_cast<float4*>(row + 4 * c);
      if constexpr (ADD) {
        const float4 w = *p;
        *p = make_float4(w.x + x[c].x, w.y + x[c].y, w.z + x[c].z, w.w + x[c].w);
      } else {
        *p = x[c];
      }
    }
  }
}

// sum += x with the rounding error of every addition carried along in comp (Kahan): the sum of n terms is good to an
// ulp or two for any n.  For the two SCALAR row sums below only (softmax denominator, delta): on a row whose softmax
// is close to one-hot, dS_ii = p_ii (dP_ii - delta_i) cancels, and what a plain running sum over 100 atoms loses in
// l (so in p_ii) and in delta comes back multiplied by |dP_ii| in a whole row of dQ and dK.
__device__ __forceinline__ void comp_add(float& sum, float& comp, float x) {
  const float y = x - comp;
  const float t = sum + y;
  comp = (t - sum) - y;
  sum = t;
}

// Row i of T: exp(s_ij - max_j s_ij) with s_ij = q_i . K_j / sqrt(d_k); returns the row sum
template <int NV>
__device__ __forceinline__ float softmax_row(const float4 (&q)[NV], const float* Kt, float* Trow, int n, float scale) {
  constexpr int RP = 4 * NV + 4;
  float m = -INFINITY;
  for (int j = 0; j < n; ++j) {
    const float s = dot_row<NV>(q, Kt + j * RP) * scale;
    Trow[j] = s;
    m = fmaxf(m, s);
  }
  float l = 0.f, comp = 0.f;
  for (int j = 0; j < n; ++j) {
    const float e = expf(Trow[j] - m);
    Trow[j] = e;
    comp_add(l, comp, e);
  }
  return l;
}

__device__ __forceinline__ int mat_tile_pitch(int n_max) { return n_max | 1; }

// ---------------------------------------------------------------------------------------------------- forward
template <int NV>
__global__ __launch_bounds__(kMatMaxAtoms) void mat_attn_fwd_kernel(const MatArgs a) {
  extern __shared__ float4 mat_smem[];
  constexpr int RP = 4 * NV + 4;
  const MatBlock b = mat_block(a);
  if (!b.ok) return;
  const int TP = mat_tile_pitch(a.n_max);
  float* X = reinterpret_cast<float*>(mat_smem);
  float* Y = X + a.n_max * RP;
  float* T = Y + a.n_max * RP;
  const bool kv_same = a.k == a.v;
  stage_rows<NV>(X, a.k + b.a0 * a.ld + b.col0, a.ld, b.n, b.nv);
  if (!kv_same) stage_rows<NV>(Y, a.v + b.a0 * a.ld + b.col0, a.ld, b.n, b.nv);
  __syncthreads();
  const float* Vt = kv_same ? X : Y;
  const int i = threadIdx.x;
  if (i >= b.n) return;  // (no barrier below)
  float4 r[NV];
  load_row<NV>(r, a.q + (b.a0 + i) * a.ld + b.col0, b.nv);
  float* Trow = T + i * TP;
  const float l = softmax_row<NV>(r, X, Trow, b.n, a.inv_sqrt_dk);
  const float* brow = a.bias + b.p0 + (int64_t)i * b.n;
#pragma unroll
  for (int c = 0; c < NV; ++c) r[c] = f4zero();
  for (int j = 0; j < b.n; ++j) {
    const float w = fmaf(a.lambda_att, Trow[j] / l, brow[j]);
    axpy_row<NV>(r, w, Vt + j * RP);
  }
  store_row<NV, false>(a.o + (b.a0 + i) * a.ldo + b.col0, r, b.nv);
}

// ---------------------------------------------------------------------------------------------------- backward
template <int NV>
__global__ __launch_bounds__(kMatMaxAtoms) void mat_attn_bwd_kernel(const MatArgs a) {
  extern __shared__ float4 mat_smem[];
  constexpr int RP = 4 * NV + 4;
  const MatBlock b = mat_block(a);
  if (!b.ok) return;  // uniform: before every barrier
  const int TP = mat_tile_pitch(a.n_max);
  float* X = reinterpret_cast<float*>(mat_smem);
  float* Y = X + a.n_max * RP;
  float* T = Y + a.n_max * RP;
  float* Dl = T + a.n_max * TP;
  const int t = threadIdx.x;
  const bool active = t < b.n;
  const bool shared = a.shared != 0;
  const int row0 = b.a0;
  const float* gO = a.dO + row0 * a.lddo + b.col0;
  stage_rows<NV>(X, a.k + row0 * a.ld + b.col0, a.ld, b.n, b.nv);
  if (shared) {
    stage_rows<NV>(Y, gO, a.lddo, b.n, b.nv);
  } else {
    stage_rows<NV>(Y, a.v + row0 * a.ld + b.col0, a.ld, b.n, b.nv);
  }
  __syncthreads();
  const float c_ds = a.lambda_att * a.inv_sqrt_dk;
  // ---- row-owned: lane t = query row i
  {
    const float* Kt = X;
    const float* Vt = shared ? X : Y;
    if (active) {
      float4 r[NV], acc[NV];
      load_row<NV>(r, a.q + (row0 + t) * a.ld + b.col0, b.nv);
      float* Trow = T + t * TP;
      const float l = softmax_row<NV>(r, Kt, Trow, b.n, a.inv_sqrt_dk);
      load_row<NV>(r, gO + t * a.lddo, b.nv);  // dO_i
      float delta = 0.f, comp = 0.f;
      for (int j = 0; j < b.n; ++j) {
        const float p = Trow[j] / l;
        Trow[j] = p;
        comp_add(delta, comp, p * dot_row<NV>(r, Vt + j * RP));
      }
      Dl[t] = delta;
#pragma unroll
      for (int c = 0; c < NV; ++c) acc[c] = f4zero();
      for (int j = 0; j < b.n; ++j) {
        const float ds = c_ds * Trow[j] * (dot_row<NV>(r, Vt + j * RP) - delta);
        axpy_row<NV>(acc, ds, Kt + j * RP);
      }
      store_row<NV, false>(a.dq + (row0 + t) * a.ldg + b.col0, acc, b.nv);
    }
  }
  __syncthreads();
  // ---- column-owned: lane t = key column j.  v_j before its tile is refilled
  float4 vj[NV];
  if (active) load_row<NV>(vj, (shared ? X : Y) + t * RP, NV);
  if (!shared) {
    __syncthreads();
    stage_rows<NV>(X, a.q + row0 * a.ld + b.col0, a.ld, b.n, b.nv);
    stage_rows<NV>(Y, gO, a.lddo, b.n, b.nv);
    __syncthreads();
  }
  if (!active) return;  // (no barrier below)
  const float* Qt = X;
  const float* Gt = Y;
  float4 acc[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) acc[c] = f4zero();
  for (int i = 0; i < b.n; ++i) {
    const float ds = c_ds * T[i * TP + t] * (dot_row<NV>(vj, Gt + i * RP) - Dl[i]);
    axpy_row<NV>(acc, ds, Qt + i * RP);
  }
  if (shared) {
    store_row<NV, true>(a.dq + (row0 + t) * a.ldg + b.col0, acc, b.nv);
  } else {
    store_row<NV, false>(a.dkk + (row0 + t) * a.ldg + b.col0, acc, b.nv);
  }
#pragma unroll
  for (int c = 0; c < NV; ++c) acc[c] = f4zero();
  const float* bcol = a.bias + b.p0 + t;
  for (int i = 0; i < b.n; ++i) {
    const float w = fmaf(a.lambda_att, T[i * TP + t], bcol[(int64_t)i * b.n]);
    axpy_row<NV>(acc, w, Gt + i * RP);
  }
  if (shared) {
    store_row<NV, true>(a.dq + (row0 + t) * a.ldg + b.col0, acc, b.nv);
  } else {
    store_row<NV, false>(a.dv + (row0 + t) * a.ldg + b.col0, acc, b.nv);
  }
}

size_t mat_lds_bytes(int nv_cap, int n_max, bool bwd) {
  const size_t rp = 4 * nv_cap + 4, tp = n_max | 1;
  return (2 * (size_t)n_max * rp + (size_t)n_max * tp + (bwd ? n_max : 0)) * sizeof(float);
}

template <bool BWD, int NV>
int launch_mat(const MatArgs& a, hipStream_t st) {
  const size_t lds = mat_lds_bytes(NV, a.n_max, BWD);
  void (*kern)(const MatArgs);
  if constexpr (BWD) {
    kern = mat_attn_bwd_kernel<NV>;
  } else {
    kern = mat_attn_fwd_kernel<NV>;
  }
  static LdsLimit lim;  // per instantiation, keyed by device inside
  if (lds > 64 * 1024 && !raise_lds_limit(lim, reinterpret_cast<const void*>(kern), mat_lds_bytes(NV, kMatMaxAtoms, BWD))) {
    set_error("mat_attention: hipFuncSetAttribute(max dynamic LDS = %zu) failed", mat_lds_bytes(NV, kMatMaxAtoms, BWD));
    return GCMI_ERR_LAUNCH;
  }
  const int threads = (a.n_max + 63) / 64 * 64;
  hipLaunchKernelGGL(kern, dim3((unsigned)(a.n_mols * a.n_heads)), dim3(threads), lds, st, a);
  GCMI_CHECK_LAUNCH(BWD ? "mat_attention_bwd" : "mat_attention_fwd");
  return GCMI_OK;
}

template <bool BWD>
int dispatch_mat(const MatArgs& a, hipStream_t st) {
  const int nv = a.dk / 4;
  if (nv <= 1) return launch_mat<BWD, 1>(a, st);
  if (nv <= 2) return launch_mat<BWD, 2>(a, st);
  if (nv <= 4) return launch_mat<BWD, 4>(a, st);
  if (nv <= 8) return launch_mat<BWD, 8>(a, st);
  return launch_mat<BWD, 16>(a, st);
}

// The host's copy of the offsets: n_mols + 1 entries each, atom_off strictly increasing from 0, pair_off the exclusive
// sums of n^2.  *n_max: the largest molecule.
int check_mat_offsets(const char* what, const int32_t* h_atom_off, const int32_t* h_pair_off, const int32_t* d_atom_off,
                      const int32_t* d_pair_off, int32_t n_mols, int32_t* n_max) {
  GCMI_CHECK_ARG(n_mols > 0, "%s: n_mols %d must be positive", what, n_mols);
  GCMI_CHECK_ARG(h_atom_off && h_pair_off && d_atom_off && d_pair_off, "%s: NULL offsets", what);
  GCMI_CHECK_ARG(h_atom_off[0] == 0 && h_pair_off[0] == 0, "%s: offsets must start at 0", what);
  int32_t mx = 0;
  for (int32_t m = 0; m < n_mols; ++m) {
    const int64_t n = (int64_t)h_atom_off[m + 1] - h_atom_off[m];
    GCMI_CHECK_ARG(n > 0, "%s: atom offsets do not increase at molecule %d", what, m);
    GCMI_CHECK_ARG((int64_t)h_pair_off[m + 1] - h_pair_off[m] == n * n && n * n < ((int64_t)1 << 30),
                   "%s: pair offsets do not increase by n^2 at molecule %d", what, m);
    mx = std::max<int32_t>(mx, (int32_t)n);
  }
  *n_max = mx;
  return GCMI_OK;
}

// the kernels index rows with 32-bit element offsets
bool mat_rows_fit(int32_t n_atoms, int64_t ld) { return ld < ((int64_t)1 << 31) && (int64_t)n_atoms * ld < ((int64_t)1 << 31); }

int check_mat_attention(const char* what, const float* d_q, const float* d_k, const float* d_v, int64_t ld,
                        const float* d_bias, const int32_t* h_atom_off, const int32_t* h_pair_off,
                        const int32_t* d_atom_off, const int32_t* d_pair_off, int32_t n_mols, int32_t n_heads, int32_t dk,
                        int32_t* n_max) {
  GCMI_CHECK_ARG(d_q && d_k && d_v && d_bias, "%s: NULL buffer", what);
  GCMI_CHECK_ARG(n_heads > 0 && dk > 0 && (int64_t)n_heads * dk <= ((int64_t)1 << 24), "%s: bad n_heads %d / d_k %d", what,
                 n_heads, dk);
  GCMI_CHECK_ARG(ld >= (int64_t)n_heads * dk, "%s: ld %lld < n_heads * d_k = %lld", what, (long long)ld,
                 (long long)n_heads * dk);
  const int rc = check_mat_offsets(what, h_atom_off, h_pair_off, d_atom_off, d_pair_off, n_mols, n_max);
  if (rc != GCMI_OK) return rc;
  GCMI_CHECK_ARG((int64_t)n_mols * n_heads < ((int64_t)1 << 31), "%s: n_mols * n_heads does not fit a grid", what);
  GCMI_CHECK_ARG(mat_rows_fit(h_atom_off[n_mols], ld), "%s: atoms x ld does not fit 31 bits", what);
  if (dk % 4 != 0 || dk > 64) {
    set_error("%s: d_k %d is not a multiple of 4 up to 64: no kernel for it", what, dk);
    return GCMI_ERR_UNSUPPORTED;
  }
  if (*n_max > kMatMaxAtoms) {
    set_error("%s: a molecule of %d atoms is above the cap of %d", what, *n_max, kMatMaxAtoms);
    return GCMI_ERR_UNSUPPORTED;
  }
  GCMI_CHECK_ARG(ld % 4 == 0 && aligned16(d_q) && aligned16(d_k) && aligned16(d_v),
                 "%s: rows must be 16-byte aligned with ld %% 4 == 0", what);
  return GCMI_OK;
}

// ---------------------------------------------------------------------------------------------------- bias
// One wave per atom row
__global__ __launch_bounds__(kMatBiasThreads) void mat_bias_kernel(const float* __restrict__ adj,
                                                                   const float* __restrict__ dist,
                                                                   const int32_t* __restrict__ atom_off,
                                                                   const int32_t* __restrict__ pair_off, int32_t n_mols,
                                                                   int32_t n_atoms, int64_t n_pairs, int32_t use_exp,
                                                                   float l_dist, float l_adj, float eps,
                                                                   float* __restrict__ bias) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (kMatBiasThreads / 64) + (threadIdx.x >> 6);
  if (row >= n_atoms) return;
  int lo = 0, hi = n_mols - 1;  // the last molecule whose first atom is <= row
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (atom_off[mid] <= row) lo = mid; else hi = mid - 1;
  }
  const int a0 = atom_off[lo], n = atom_off[lo + 1] - a0, i = row - a0;
  const int64_t p0 = pair_off[lo];
  if (n <= 0 || i < 0 || i >= n || p0 < 0 || p0 + (int64_t)n * n > n_pairs) return;
  const int64_t base = p0 + (int64_t)i * n;
  float sa = 0.f, dmin = INFINITY;
  for (int j = lane; j < n; j += 64) {
    sa += adj[base + j];
    dmin = fminf(dmin, dist[base + j]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sa += __shfl_xor(sa, o);
    dmin = fminf(dmin, __shfl_xor(dmin, o));
  }
  const float inv_a = 1.f / (sa + eps);
  if (use_exp) {
    for (int j = lane; j < n; j += 64) bias[base + j] = fmaf(l_dist, expf(-dist[base + j]), l_adj * (adj[base + j] * inv_a));
    return;
  }
  float se = 0.f;
  for (int j = lane; j < n; j += 64) se += expf(dmin - dist[base + j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
  for (int j = lane; j < n; j += 64)
    bias[base + j] = fmaf(l_dist, expf(dmin - dist[base + j]) / se, l_adj * (adj[base + j] * inv_a));
}

}  // namespace
}  // namespace gcmi

using namespace gcmi;

extern "C" {

int gcmi_mat_bias(const float* d_adj, const float* d_dist, const int32_t* h_atom_off, const int32_t* h_pair_off,
                  const int32_t* d_atom_off, const int32_t* d_pair_off, int32_t n_mols, int32_t dist_kernel,
                  float lambda_distance, float lambda_adjacency, float eps, float* d_bias, void* stream) {
  GCMI_CHECK_ARG(d_adj && d_dist && d_bias, "mat_bias: NULL buffer");
  GCMI_CHECK_ARG(dist_kernel == GCMI_MAT_DIST_SOFTMAX || dist_kernel == GCMI_MAT_DIST_EXP, "mat_bias: dist_kernel %d",
                 dist_kernel);
  int32_t n_max = 0;
  const int rc = check_mat_offsets("mat_bias", h_atom_off, h_pair_off, d_atom_off, d_pair_off, n_mols, &n_max);
  if (rc != GCMI_OK) return rc;
  const int32_t n_atoms = h_atom_off[n_mols];
  const int rows_per_wg = kMatBiasThreads / 64;
  hipLaunchKernelGGL(mat_bias_kernel, dim3((n_atoms + rows_per_wg - 1) / rows_per_wg), dim3(kMatBiasThreads), 0,
                     static_cast<hipStream_t>(stream), d_adj, d_dist, d_atom_off, d_pair_off, n_mols, n_atoms,
                     (int64_t)h_pair_off[n_mols], dist_kernel == GCMI_MAT_DIST_EXP ? 1 : 0, lambda_distance,
                     lambda_adjacency, eps, d_bias);
  GCMI_CHECK_LAUNCH("mat_bias");
  return GCMI_OK;
}

int gcmi_mat_attention_fwd(const float* d_q, const float* d_k, const float* d_v, int64_t ld, const float* d_bias,
                           const int32_t* h_atom_off, const int32_t* h_pair_off, const int32_t* d_atom_off,
                           const int32_t* d_pair_off, int32_t n_mols, int32_t n_heads, int32_t head_dim,
                           float lambda_attention, float* d_o, int64_t ldo, void* stream) {
  int32_t n_max = 0;
  const int rc = check_mat_attention("mat_attention_fwd", d_q, d_k, d_v, ld, d_bias, h_atom_off, h_pair_off, d_atom_off,
                                     d_pair_off, n_mols, n_heads, head_dim, &n_max);
  if (rc != GCMI_OK) return rc;
  GCMI_CHECK_ARG(d_o && ldo >= (int64_t)n_heads * head_dim && ldo % 4 == 0 && aligned16(d_o) &&
                     mat_rows_fit(h_atom_off[n_mols], ldo),
                 "mat_attention_fwd: bad output (NULL, ldo < n_heads * d_k, rows not 16-byte aligned, or atoms x ldo >= 2^31)");
  MatArgs a = {};
  a.q = d_q; a.k = d_k; a.v = d_v; a.ld = (int32_t)ld; a.bias = d_bias; a.atom_off = d_atom_off; a.pair_off = d_pair_off;
  a.n_mols = n_mols; a.n_heads = n_heads; a.dk = head_dim; a.n_max = n_max; a.n_atoms = h_atom_off[n_mols];
  a.n_pairs = h_pair_off[n_mols]; a.lambda_att = lambda_attention; a.inv_sqrt_dk = 1.f / sqrtf((float)head_dim);
  a.o = d_o; a.ldo = (int32_t)ldo;
  return dispatch_mat<false>(a, static_cast<hipStream_t>(stream));
}

int gcmi_mat_attention_bwd(const float* d_q, const float* d_k, const float* d_v, int64_t ld, const float* d_bias,
                           const int32_t* h_atom_off, const int32_t* h_pair_off, const int32_t* d_atom_off,
                           const int32_t* d_pair_off, int32_t n_mols, int32_t n_heads, int32_t head_dim,
                           float lambda_attention, const float* d_do, int64_t lddo, float* d_dq, float* d_dk, float* d_dv,
                           int64_t ldg, int32_t shared, void* stream) {
  int32_t n_max = 0;
  const int rc = check_mat_attention("mat_attention_bwd", d_q, d_k, d_v, ld, d_bias, h_atom_off, h_pair_off, d_atom_off,
                                     d_pair_off, n_mols, n_heads, head_dim, &n_max);
  if (rc != GCMI_OK) return rc;
  const int64_t width = (int64_t)n_heads * head_dim;
  GCMI_CHECK_ARG(d_do && lddo >= width && lddo % 4 == 0 && aligned16(d_do) && mat_rows_fit(h_atom_off[n_mols], lddo),
                 "mat_attention_bwd: bad dO (NULL, lddo < n_heads * d_k, rows not 16-byte aligned, or atoms x lddo >= 2^31)");
  GCMI_CHECK_ARG(d_dq && (shared || (d_dk && d_dv)), "mat_attention_bwd: NULL gradient buffer");
  GCMI_CHECK_ARG(ldg >= width && ldg % 4 == 0 && aligned16(d_dq) && (shared || (aligned16(d_dk) && aligned16(d_dv))) &&
                     mat_rows_fit(h_atom_off[n_mols], ldg),
                 "mat_attention_bwd: bad gradient rows (ldg < n_heads * d_k, not 16-byte aligned, or atoms x ldg >= 2^31)");
  GCMI_CHECK_ARG(!shared || (d_q == d_k && d_k == d_v), "mat_attention_bwd: shared needs Q, K and V to be one tensor");
  GCMI_CHECK_ARG(shared || (d_dq != d_dk && d_dk != d_dv && d_dq != d_dv),
                 "mat_attention_bwd: the three gradient buffers must be distinct (one buffer: shared)");
  MatArgs a = {};
  a.q = d_q; a.k = d_k; a.v = d_v; a.ld = (int32_t)ld; a.bias = d_bias; a.atom_off = d_atom_off; a.pair_off = d_pair_off;
  a.n_mols = n_mols; a.n_heads = n_heads; a.dk = head_dim; a.n_max = n_max; a.n_atoms = h_atom_off[n_mols];
  a.n_pairs = h_pair_off[n_mols]; a.lambda_att = lambda_attention; a.inv_sqrt_dk = 1.f / sqrtf((float)head_dim);
  a.dO = d_do; a.lddo = (int32_t)lddo; a.dq = d_dq; a.dkk = d_dk; a.dv = d_dv; a.ldg = (int32_t)ldg; a.shared = shared ? 1 : 0;
  return dispatch_mat<true>(a, static_cast<hipStream_t>(stream));
}

}  // extern "C"
