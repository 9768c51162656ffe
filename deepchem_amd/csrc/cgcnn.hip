// Crystal-graph convolution (CGCNN, Xie & Grossman 2018): everything between the two products of one CGCNNLayer, fp32.
//
// The reference's layer builds per edge k = (s -> d) the row [h[s] | h[d] | e[k]], applies Linear(2H + Fe, 2H) and
// BatchNorm1d(2H) over the E rows, gates one half with the other and sums the messages at the destination:
//     z[k] = W [h[s] | h[d] | e[k]] + b,  zh = BN(z),  m[k] = sigmoid(zh[k, :H]) * softplus(zh[k, H:]),
//     h'[v] = softplus(h[v] + sum over the edges arriving at v of m[k]),      h'[v] = 0 where no edge arrives.
// With W split by columns into A_s | A_d | C and
//     Ps = h A_s^T, Pd = h A_d^T (N rows of 2H), Q = e C^T + b (E rows of 2H)
// z[k] = (Ps[s] + Pd[d]) + Q[k] is recomputed wherever it is needed: Q is the only E-row tensor the forward reads and
// dQ = dz the only one the backward writes.  Neither z, zh, the two activations nor m ever exist in memory.
//
//   cg_stats      per-column mean and biased variance of z over the E rows.  Every workgroup accumulates, per column,
//                 sum (z - K) and sum (z - K)^2 about a pivot row K of its own (a sample of the column, so the sums
//                 stay at the scale of the spread however far the mean is from zero), sums them over its rows in double,
//                 turns them into its own mean and centred second moment (doubles), and cg_stats_finish combines the
//                 workgroups in double in a fixed order (one wave per column, a lane per 64th workgroup, a fixed tree).
//   cg_conv_fwd   one node per row group: walks the arriving list in list order, forms z, normalises, gates, adds.
//   cg_bwd_stats  the same walk with dpre[v] = dh'[v] * sigmoid(h[v] + S[v]); sigmoid(pre) = 1 - exp(-softplus(pre)), so
//                 it is recovered from h' itself and no (N, H) row is kept for it.  Per-column sums of dzh and
//                 dzh * xhat (= dbeta, dgamma), per workgroup in double, then cg_sums_finish the same way.
//   cg_bwd_edges  the walk a third time: BatchNorm backward of dzh with those sums, dQ[k] = dz[k] (an edge stands in
//                 exactly one arriving list: one owner), dPd[v] = the sum over the list, and dpre[v].
//   cg_bwd_src    dPs[v] = the sum of dQ over the LEAVING list of v.
//
// Layout: 4 consecutive hidden channels per lane, held as one float4 of the gate half and one of the message half,
// so a row takes L = H / 4 lanes (1 .. 32) and a workgroup of 256 threads floor(256 / L) rows; a lane keeps its
// channels through the whole launch, which is what lets the column sums be reduced per lane.  No atomics, one owner per
// output element, every sum in list order or in an order the sizes alone fix: two runs agree bit for bit.  Every index read from the
// device is compared with the sizes the host passed before it is used.
#include "common.h"

namespace gcmi {
namespace {

constexpr int kCgThreads = 256;
constexpr int kCgSums = 16;  // floats a lane reduces across the rows of its workgroup (two sums of 8 columns)

__device__ __forceinline__ float4 ld4(const float* p, int64_t row, int64_t ld, int c) {
  return *reinterpret_cast<const float4*>(p + row * ld + c);
}
__device__ __forceinline__ void st4(float* p, int64_t row, int64_t ld, int c, const float4& v) {
  *reinterpret_cast<float4*>(p + row * ld + c) = v;
}
__device__ __forceinline__ float4 splat4(float v) { return make_float4(v, v, v, v); }
template <typename F>
__device__ __forceinline__ float4 map4(F f, const float4& a) {
  return make_float4(f(a.x), f(a.y), f(a.z), f(a.w));
}
template <typename F>
__device__ __forceinline__ float4 map4(F f, const float4& a, const float4& b) {
  return make_float4(f(a.x, b.x), f(a.y, b.y), f(a.z, b.z), f(a.w, b.w));
}
template <typename F>
__device__ __forceinline__ float4 map4(F f, const float4& a, const float4& b, const float4& c) {
  return make_float4(f(a.x, b.x, c.x), f(a.y, b.y, c.y), f(a.z, b.z, c.z), f(a.w, b.w, c.w));
}
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) {
  return map4([](float x, float y) { return x + y; }, a, b);
}
__device__ __forceinline__ float4 sub4(const float4& a, const float4& b) {
  return map4([](float x, float y) { return x - y; }, a, b);
}
__device__ __forceinline__ float4 mul4(const float4& a, const float4& b) {
  return map4([](float x, float y) { return x * y; }, a, b);
}
__device__ __forceinline__ bool inside(int i, int n) { return (unsigned)i < (unsigned)n; }

// F.softplus(beta = 1, threshold = 20), its derivative, and the logistic function
__device__ __forceinline__ float softplus1(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoid1(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float dsoftplus1(float x) { return x > 20.f ? 1.f : sigmoid1(x); }
// sigmoid(pre) from y = softplus(pre): 1 - exp(-y); above the threshold, where y = pre, it rounds to 1
__device__ __forceinline__ float sigmoid_of_softplus(float y) { return -expm1f(-y); }

// [lo, hi) of entry v of a CSR pointer, cut to [0, n_items]; an inverted pair is an empty range
__device__ __forceinline__ void csr_range(const int32_t* ptr, int v, int n_items, int& lo, int& hi) {
  lo = ptr[v];
  hi = ptr[v + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > n_items ? n_items : hi;
  hi = hi < lo ? lo : hi;
}

struct CgRows {  // the projections; rows of 2H floats: [gate half | message half]
  const float *ps, *pd, *q;
  int64_t ldp, ldq;
  int32_t H;
};
struct CgNorm {  // vectors of 2H floats; nullptr: 0, 1, 1, 0
  const float *mean, *invstd, *gamma, *beta;
};
struct Norm4 {  // ... the 4 columns of one half that a lane holds
  float4 mean, invstd, gamma, beta;
};
__device__ __forceinline__ float4 vec4(const float* p, int col, float otherwise) {
  return p ? *reinterpret_cast<const float4*>(p + col) : splat4(otherwise);
}
__device__ __forceinline__ Norm4 load_norm(const CgNorm& n, int col) {
  return {vec4(n.mean, col, 0.f), vec4(n.invstd, col, 1.f), vec4(n.gamma, col, 1.f), vec4(n.beta, col, 0.f)};
}
__device__ __forceinline__ float4 xhat4(const float4& z, const Norm4& n) { return mul4(sub4(z, n.mean), n.invstd); }
__device__ __forceinline__ float4 affine4(const float4& xhat, const Norm4& n) {
  return map4([](float x, float g, float b) { return x * g + b; }, xhat, n.gamma, n.beta);
}

// Which rows and columns of a launch over rows of `width` floats this thread takes: 4 columns from c, row r of the
// floor(256 / L) rows its workgroup takes per turn (threads past them idle).
struct Lanes {
  int L, rpb, r, c;
  bool active;
  __device__ __forceinline__ explicit Lanes(int width) {
    L = width / 4;
    rpb = kCgThreads / L;
    r = (int)threadIdx.x / L;
    c = 4 * ((int)threadIdx.x - r * L);
    active = r < rpb;
  }
};

// Sums v[0 .. kCgSums) and cnt over the rows of the workgroup, lane by lane, rows in order, in double (a row's partial
// is a handful of terms; the sum over up to 256 rows is where float32 would lose bits of the mean); the result is valid
// in the threads of row 0 (threadIdx.x < L).  Every thread of the workgroup calls it.
template <typename T>
__device__ __forceinline__ void reduce_rows(const Lanes& w, const T (&v)[kCgSums], int& cnt, double (&d)[kCgSums]) {
  __shared__ T red[kCgSums][kCgThreads];
  __shared__ int redn[kCgThreads];
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < kCgSums; ++i) red[i][tid] = v[i];
  redn[tid] = cnt;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kCgSums; ++i) d[i] = (double)v[i];
  if (tid < w.L) {
    for (int rr = 1; rr < w.rpb; ++rr) {
#pragma unroll
      for (int i = 0; i < kCgSums; ++i) d[i] += (double)red[i][rr * w.L + tid];
      cnt += redn[rr * w.L + tid];
    }
  }
}

// What one workgroup leaves for the finishing kernels: a row of 8H + 4 floats, [count (int32) | pad to 16 bytes | 4H
// doubles]
__host__ __device__ __forceinline__ int64_t part_stride(int H) { return 8 * (int64_t)H + 4; }
__device__ __forceinline__ const double* part_values(const float* row) { return reinterpret_cast<const double*>(row + 4); }
__device__ __forceinline__ double* part_values(float* row) { return reinterpret_cast<double*>(row + 4); }

__device__ __forceinline__ void put8(double* dst, int H, int c, const double* v) {  // v[0..4) to c, v[4..8) to H + c
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dst[c + i] = v[i];
    dst[H + c + i] = v[4 + i];
  }
}

__device__ __forceinline__ void z_of_edge(const CgRows& a, int s, int d, int e, int c, float4& zg, float4& zm) {
  zg = add4(add4(ld4(a.ps, s, a.ldp, c), ld4(a.pd, d, a.ldp, c)), ld4(a.q, e, a.ldq, c));
  zm = add4(add4(ld4(a.ps, s, a.ldp, a.H + c), ld4(a.pd, d, a.ldp, a.H + c)), ld4(a.q, e, a.ldq, a.H + c));
}

// ---- statistics of z over the edges
__global__ __launch_bounds__(kCgThreads) void cg_stats_kernel(gcmi_gn_graph g, CgRows a, float* __restrict__ part) {
  const Lanes w(a.H);
  double v[kCgSums];  // (in double: with few workgroups a lane adds many rows)
#pragma unroll
  for (int i = 0; i < kCgSums; ++i) v[i] = 0.0;
  int cnt = 0;
  // the pivot: z of the first row of this workgroup (the grid never has more workgroups than row groups)
  float4 kg = splat4(0.f), km = splat4(0.f);
  {
    const int64_t e0 = (int64_t)blockIdx.x * w.rpb;
    if (w.active && e0 < g.n_edges) {
      const int s = g.src[e0], d = g.dst[e0];
      if (inside(s, g.n_nodes) && inside(d, g.n_nodes)) z_of_edge(a, s, d, (int)e0, w.c, kg, km);
    }
  }
  for (int64_t base = (int64_t)blockIdx.x * w.rpb; base < g.n_edges; base += (int64_t)gridDim.x * w.rpb) {
    const int64_t e = base + w.r;
    if (!w.active || e >= g.n_edges) continue;
    const int s = g.src[e], d = g.dst[e];
    if (!inside(s, g.n_nodes) || !inside(d, g.n_nodes)) continue;
    float4 zg, zm;
    z_of_edge(a, s, d, (int)e, w.c, zg, zm);
    const float4 dg = sub4(zg, kg), dm = sub4(zm, km);
    const float dl[8] = {dg.x, dg.y, dg.z, dg.w, dm.x, dm.y, dm.z, dm.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] += (double)dl[i];
      v[8 + i] += (double)(dl[i] * dl[i]);
    }
    ++cnt;
  }
  double d[kCgSums];
  reduce_rows(w, v, cnt, d);
  if ((int)threadIdx.x < w.L) {
    float* row = part + (int64_t)blockIdx.x * part_stride(a.H);
    if (threadIdx.x == 0) reinterpret_cast<int32_t*>(row)[0] = cnt;
    const float k8[8] = {kg.x, kg.y, kg.z, kg.w, km.x, km.y, km.z, km.w};
    double mean[8], m2[8];
    const double inv = cnt > 0 ? 1.0 / (double)cnt : 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      mean[i] = cnt > 0 ? (double)k8[i] + d[i] * inv : 0.0;
      m2[i] = fmax(d[8 + i] - d[i] * d[i] * inv, 0.0);
    }
    put8(part_values(row), a.H, w.c, mean);           // values [0, 2H): the workgroup's mean
    put8(part_values(row) + 2 * a.H, a.H, w.c, m2);   // values [2H, 4H): its centred second moment
  }
}

// The sum of v over the lanes of a wave by a fixed tree; valid in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One wave per column: lane l takes the workgroups l, l + 64, ... in order, the lanes are combined by a fixed tree.  The
// moments are combined in double about the first workgroup's mean.
__global__ __launch_bounds__(kCgThreads) void cg_stats_finish_kernel(const float* __restrict__ part, int n_part, int H, float eps,
                                                                     float momentum, float* __restrict__ mean,
                                                                     float* __restrict__ invstd, float* __restrict__ running_mean,
                                                                     float* __restrict__ running_var,
                                                                     int64_t* __restrict__ batches_tracked) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && batches_tracked) *batches_tracked += 1;
  const int j = (int)blockIdx.x * (kCgThreads / 64) + (int)threadIdx.x / 64, lane = threadIdx.x & 63;
  if (j >= 2 * H) return;  // (the whole wave)
  const int64_t stride = part_stride(H);
  const double ref = part_values(part)[j];
  double s1 = 0.0, s2 = 0.0, total = 0.0;
  for (int b = lane; b < n_part; b += 64) {
    const float* row = part + b * stride;
    const double n = (double)reinterpret_cast<const int32_t*>(row)[0];
    const double dm = part_values(row)[j] - ref;
    s1 += n * dm;
    s2 += part_values(row)[2 * H + j] + n * dm * dm;
    total += n;
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  total = wave_sum(total);
  if (lane != 0) return;
  const double count = total > 0.0 ? total : 1.0;
  const double mu = ref + s1 / count;
  double m2 = s2 - s1 * s1 / count;
  m2 = m2 > 0.0 ? m2 : 0.0;
  mean[j] = (float)mu;
  invstd[j] = (float)(1.0 / sqrt(m2 / count + (double)eps));
  if (running_mean) {
    running_mean[j] = (1.f - momentum) * running_mean[j] + momentum * (float)mu;
    running_var[j] = (1.f - momentum) * running_var[j] + momentum * (float)(m2 / (total > 1.0 ? total - 1.0 : 1.0));
  }
}

// ---- forward
__global__ __launch_bounds__(kCgThreads) void cg_conv_fwd_kernel(gcmi_gn_graph g, CgRows a, CgNorm nrm,
                                                                const float* __restrict__ h, int64_t ldh,
                                                                float* __restrict__ out, int64_t ldo) {
  const Lanes w(a.H);
  if (!w.active) return;
  const Norm4 ng = load_norm(nrm, w.c), nm = load_norm(nrm, a.H + w.c);
  for (int64_t base = (int64_t)blockIdx.x * w.rpb; base < g.n_nodes; base += (int64_t)gridDim.x * w.rpb) {
    const int64_t v = base + w.r;
    if (v >= g.n_nodes) continue;
    int lo, hi;
    csr_range(g.inc_ptr, (int)v, g.n_inc, lo, hi);
    float4 res = splat4(0.f);
    if (hi > lo) {
      float4 acc = splat4(0.f);
      for (int k = lo; k < hi; ++k) {
        const int e = g.inc_edge[k], o = g.inc_other[k];
        if (!inside(e, g.n_edges) || !inside(o, g.n_nodes)) continue;
        float4 zg, zm;
        z_of_edge(a, o, (int)v, e, w.c, zg, zm);
        const float4 gate = map4(sigmoid1, affine4(xhat4(zg, ng), ng));
        const float4 msg = map4(softplus1, affine4(xhat4(zm, nm), nm));
        acc = add4(acc, mul4(gate, msg));
      }
      res = map4(softplus1, add4(ld4(h, v, ldh, w.c), acc));
    }
    st4(out, v, ldo, w.c, res);
  }
}

// ---- backward
struct CgGrad {  // h' and the gradient that arrives for it
  const float *hnew, *dhnew;
  int64_t ldhn, lddh;
};

// dpre of node v for the lane's 4 channels; 0 where the arriving list is empty
__device__ __forceinline__ float4 dpre_of(const CgGrad& b, int64_t v, int c, bool has_edges) {
  if (!has_edges) return splat4(0.f);
  return mul4(ld4(b.dhnew, v, b.lddh, c), map4(sigmoid_of_softplus, ld4(b.hnew, v, b.ldhn, c)));
}

// (dzh of the gate half, dzh of the message half) of one edge from dpre and the two xhat
__device__ __forceinline__ void dzh_of(const float4& dpre, const float4& xg, const float4& xm, const Norm4& ng, const Norm4& nm,
                                       float4& dg, float4& dm) {
  const float4 zhg = affine4(xg, ng), zhm = affine4(xm, nm);
  const float4 sg = map4(sigmoid1, zhg);
  dg = map4([](float d, float sp, float s) { return d * sp * (s * (1.f - s)); }, dpre, map4(softplus1, zhm), sg);
  dm = map4([](float d, float s, float ds) { return d * s * ds; }, dpre, sg, map4(dsoftplus1, zhm));
}

__global__ __launch_bounds__(kCgThreads) void cg_bwd_stats_kernel(gcmi_gn_graph g, CgRows a, CgNorm nrm, CgGrad b,
                                                                 float* __restrict__ part) {
  const Lanes w(a.H);
  // in double: a lane adds one term per entry of its nodes' lists, hundreds in a row for a crowded node, all of one
  // scale; in float32 that sequential sum alone costs more than the terms' own rounding
  double v8[kCgSums];
#pragma unroll
  for (int i = 0; i < kCgSums; ++i) v8[i] = 0.0;
  int cnt = 0;
  if (w.active) {
    const Norm4 ng = load_norm(nrm, w.c), nm = load_norm(nrm, a.H + w.c);
    for (int64_t base = (int64_t)blockIdx.x * w.rpb; base < g.n_nodes; base += (int64_t)gridDim.x * w.rpb) {
      const int64_t v = base + w.r;
      if (v >= g.n_nodes) continue;
      int lo, hi;
      csr_range(g.inc_ptr, (int)v, g.n_inc, lo, hi);
      if (hi <= lo) continue;
      const float4 dpre = dpre_of(b, v, w.c, true);
      for (int k = lo; k < hi; ++k) {
        const int e = g.inc_edge[k], o = g.inc_other[k];
        if (!inside(e, g.n_edges) || !inside(o, g.n_nodes)) continue;
        float4 zg, zm, dg, dm;
        z_of_edge(a, o, (int)v, e, w.c, zg, zm);
        const float4 xg = xhat4(zg, ng), xm = xhat4(zm, nm);
        dzh_of(dpre, xg, xm, ng, nm, dg, dm);
        const float d8[8] = {dg.x, dg.y, dg.z, dg.w, dm.x, dm.y, dm.z, dm.w};
        const float x8[8] = {xg.x, xg.y, xg.z, xg.w, xm.x, xm.y, xm.z, xm.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          v8[i] += (double)d8[i];
          v8[8 + i] += (double)(d8[i] * x8[i]);
        }
        ++cnt;
      }
    }
  }
  double d[kCgSums];
  reduce_rows(w, v8, cnt, d);
  if ((int)threadIdx.x < w.L) {
    float* row = part + (int64_t)blockIdx.x * part_stride(a.H);
    if (threadIdx.x == 0) reinterpret_cast<int32_t*>(row)[0] = cnt;
    put8(part_values(row), a.H, w.c, d);               // sum of dzh
    put8(part_values(row) + 2 * a.H, a.H, w.c, d + 8);  // sum of dzh * xhat
  }
}

// sums[j] = the sum over the workgroups of their value j in double: one wave per value, as cg_stats_finish_kernel
__global__ __launch_bounds__(kCgThreads) void cg_sums_finish_kernel(const float* __restrict__ part, int n_part, int H,
                                                                    float* __restrict__ sums) {
  const int j = (int)blockIdx.x * (kCgThreads / 64) + (int)threadIdx.x / 64, lane = threadIdx.x & 63;
  if (j >= 4 * H) return;
  const int64_t stride = part_stride(H);
  double sum = 0.0;
  for (int b = lane; b < n_part; b += 64) sum += part_values(part + b * stride)[j];
  sum = wave_sum(sum);
  if (lane == 0) sums[j] = (float)sum;
}

__global__ __launch_bounds__(kCgThreads) void cg_bwd_edges_kernel(gcmi_gn_graph g, CgRows a, CgNorm nrm, CgGrad b,
                                                                 const float* __restrict__ sums, float inv_e,
                                                                 float* __restrict__ dq, int64_t lddq, float* __restrict__ dpd,
                                                                 int64_t lddp, float* __restrict__ dpre_out, int64_t lddpre) {
  const Lanes w(a.H);
  if (!w.active) return;
  const Norm4 ng = load_norm(nrm, w.c), nm = load_norm(nrm, a.H + w.c);
  const float4 ag = mul4(ng.gamma, ng.invstd), am = mul4(nm.gamma, nm.invstd);  // dz per dxhat-term
  const bool train = sums != nullptr;
  // training: dz = a (dzh - c1 - xhat c2), c1 = sum dzh / E, c2 = sum dzh xhat / E
  const float4 c1g = train ? mul4(vec4(sums, w.c, 0.f), splat4(inv_e)) : splat4(0.f);
  const float4 c1m = train ? mul4(vec4(sums, a.H + w.c, 0.f), splat4(inv_e)) : splat4(0.f);
  const float4 c2g = train ? mul4(vec4(sums, 2 * a.H + w.c, 0.f), splat4(inv_e)) : splat4(0.f);
  const float4 c2m = train ? mul4(vec4(sums, 3 * a.H + w.c, 0.f), splat4(inv_e)) : splat4(0.f);
  auto bn_bwd = [](float d, float x, float c2) { return d - x * c2; };
  for (int64_t base = (int64_t)blockIdx.x * w.rpb; base < g.n_nodes; base += (int64_t)gridDim.x * w.rpb) {
    const int64_t v = base + w.r;
    if (v >= g.n_nodes) continue;
    int lo, hi;
    csr_range(g.inc_ptr, (int)v, g.n_inc, lo, hi);
    const float4 dpre = dpre_of(b, v, w.c, hi > lo);
    float4 accg = splat4(0.f), accm = splat4(0.f);
    for (int k = lo; k < hi; ++k) {
      const int e = g.inc_edge[k], o = g.inc_other[k];
      if (!inside(e, g.n_edges) || !inside(o, g.n_nodes)) continue;
      float4 zg, zm, dg, dm;
      z_of_edge(a, o, (int)v, e, w.c, zg, zm);
      const float4 xg = xhat4(zg, ng), xm = xhat4(zm, nm);
      dzh_of(dpre, xg, xm, ng, nm, dg, dm);
      const float4 dzg = mul4(ag, map4(bn_bwd, sub4(dg, c1g), xg, c2g));
      const float4 dzm = mul4(am, map4(bn_bwd, sub4(dm, c1m), xm, c2m));
      st4(dq, e, lddq, w.c, dzg);
      st4(dq, e, lddq, a.H + w.c, dzm);
      accg = add4(accg, dzg);
      accm = add4(accm, dzm);
    }
    st4(dpd, v, lddp, w.c, accg);
    st4(dpd, v, lddp, a.H + w.c, accm);
    st4(dpre_out, v, lddpre, w.c, dpre);
  }
}

// out[v] = the sum over list(v) of rows[edge], rows of `width` floats
__global__ __launch_bounds__(kCgThreads) void cg_list_sum_kernel(int32_t n_nodes, int32_t n_edges, int32_t n_list,
                                                                const int32_t* __restrict__ ptr,
                                                                const int32_t* __restrict__ list_edge, int32_t width,
                                                                const float* __restrict__ rows, int64_t ldr,
                                                                float* __restrict__ out, int64_t ldo) {
  const Lanes w(width);
  if (!w.active) return;
  for (int64_t base = (int64_t)blockIdx.x * w.rpb; base < n_nodes; base += (int64_t)gridDim.x * w.rpb) {
    const int64_t v = base + w.r;
    if (v >= n_nodes) continue;
    int lo, hi;
    csr_range(ptr, (int)v, n_list, lo, hi);
    float4 acc = splat4(0.f);
    for (int k = lo; k < hi; ++k) {
      const int e = list_edge[k];
      if (inside(e, n_edges)) acc = add4(acc, ld4(rows, e, ldr, w.c));
    }
    st4(out, v, ldo, w.c, acc);
  }
}

// ---- host side
int rows_per_wg(int width) { return kCgThreads / (width / 4); }
int grid_rows(int64_t n_rows, int width) { return grid_for(n_rows, rows_per_wg(width)); }  // one "item" = one row group slot
// ... of the two launches that leave one partial row per workgroup: few enough for the finishing kernels to stay short,
// enough for 4 waves on every SIMD
constexpr int kCgMaxParts = 1024;
int grid_parts(int64_t n_rows, int width) { return std::min(grid_rows(n_rows, width), kCgMaxParts); }

bool rows_ok(const void* p, int64_t ld, int width) { return p && aligned16(p) && ld >= width && ld % 4 == 0; }
bool vec_ok(const void* p) { return p == nullptr || aligned16(p); }

int check_cg(const char* what, const gcmi_gn_graph* g, int32_t H) {
  GCMI_CHECK_ARG(g != nullptr, "%s: NULL graph", what);
  GCMI_CHECK_ARG(H >= GCMI_CG_MIN_WIDTH && H <= GCMI_CG_MAX_WIDTH && H % 4 == 0,
                 "%s: H %d is not a multiple of 4 in [%d, %d]", what, H, GCMI_CG_MIN_WIDTH, GCMI_CG_MAX_WIDTH);
  GCMI_CHECK_ARG(g->n_nodes > 0 && g->n_graphs > 0 && g->n_edges >= 0 && g->n_graphs <= g->n_nodes,
                 "%s: n_nodes %d, n_edges %d, n_graphs %d (nodes and graphs must be positive, every graph holds a node)",
                 what, g->n_nodes, g->n_edges, g->n_graphs);
  GCMI_CHECK_ARG(g->undirected == 0, "%s: the graph description must be directed (undirected = %d)", what, g->undirected);
  GCMI_CHECK_ARG(g->n_inc == g->n_edges && (int64_t)g->n_edges * 2 < INT32_MAX, "%s: n_inc %d is not n_edges %d", what,
                 g->n_inc, g->n_edges);
  GCMI_CHECK_ARG(g->inc_ptr && g->out_ptr, "%s: NULL inc_ptr / out_ptr", what);
  GCMI_CHECK_ARG(g->n_edges == 0 || (g->src && g->dst && g->inc_edge && g->inc_other && g->out_edge && g->out_other),
                 "%s: NULL edge, arriving or leaving list", what);
  return GCMI_OK;
}

int check_cg_rows(const char* what, const gcmi_gn_graph* g, int32_t H, const float* ps, const float* pd, int64_t ldp,
                  const float* q, int64_t ldq) {
  GCMI_CHECK_ARG(rows_ok(ps, ldp, 2 * H) && rows_ok(pd, ldp, 2 * H),
                 "%s: bad Ps / Pd (NULL, not 16-byte aligned, or ldp < %d or ldp %% 4)", what, 2 * H);
  GCMI_CHECK_ARG(g->n_edges == 0 || rows_ok(q, ldq, 2 * H), "%s: bad Q (NULL, not 16-byte aligned, or ldq < %d or ldq %% 4)",
                 what, 2 * H);
  return GCMI_OK;
}

int check_cg_norm(const char* what, const float* mean, const float* invstd, const float* gamma, const float* beta) {
  GCMI_CHECK_ARG(vec_ok(mean) && vec_ok(invstd) && vec_ok(gamma) && vec_ok(beta),
                 "%s: mean / invstd / gamma / beta must be 16-byte aligned", what);
  GCMI_CHECK_ARG((mean == nullptr) == (invstd == nullptr), "%s: mean and invstd go together", what);
  return GCMI_OK;
}

int check_cg_grad(const char* what, int32_t H, const float* hnew, int64_t ldhn, const float* dhnew, int64_t lddh) {
  GCMI_CHECK_ARG(rows_ok(hnew, ldhn, H), "%s: bad h' (NULL, not 16-byte aligned, or ldhn < %d or ldhn %% 4)", what, H);
  GCMI_CHECK_ARG(rows_ok(dhnew, lddh, H), "%s: bad dh' (NULL, not 16-byte aligned, or lddh < %d or lddh %% 4)", what, H);
  return GCMI_OK;
}

int64_t workspace_floats(int32_t n_nodes, int32_t n_edges, int32_t H) {
  const int64_t parts = std::max(grid_parts(n_nodes, H), grid_parts(n_edges, H));
  return parts * part_stride(H);
}

int check_workspace(const char* what, const gcmi_gn_graph* g, int32_t H, const float* ws, int64_t ws_floats) {
  GCMI_CHECK_ARG(ws && aligned16(ws) && ws_floats >= workspace_floats(g->n_nodes, g->n_edges, H),
                 "%s: the workspace is NULL, not 16-byte aligned, or holds %lld floats of the %lld needed", what,
                 (long long)ws_floats, (long long)workspace_floats(g->n_nodes, g->n_edges, H));
  return GCMI_OK;
}

}  // namespace
}  // namespace gcmi

using namespace gcmi;

#define CG_TRY(expr)                \
  do {                              \
    const int rc__ = (expr);        \
    if (rc__ != GCMI_OK) return rc__; \
  } while (0)

extern "C" {

int64_t gcmi_cg_workspace_floats(int32_t n_nodes, int32_t n_edges, int32_t H) {
  if (n_nodes < 0 || n_edges < 0 || H < GCMI_CG_MIN_WIDTH || H > GCMI_CG_MAX_WIDTH || H % 4) return -1;
  return workspace_floats(n_nodes, n_edges, H);
}

int gcmi_cg_stats(const gcmi_gn_graph* g, const float* d_ps, const float* d_pd, int64_t ldp, const float* d_q, int64_t ldq,
                  int32_t H, float eps, float momentum, float* d_mean, float* d_invstd, float* d_running_mean,
                  float* d_running_var, int64_t* d_batches_tracked, float* d_workspace, int64_t workspace_floats_,
                  void* stream) {
  const char* what = "cg_stats";
  CG_TRY(check_cg(what, g, H));
  GCMI_CHECK_ARG(g->n_edges >= 2, "%s: the statistics need at least 2 edges, got %d", what, g->n_edges);
  CG_TRY(check_cg_rows(what, g, H, d_ps, d_pd, ldp, d_q, ldq));
  GCMI_CHECK_ARG(d_mean && d_invstd && aligned16(d_mean) && aligned16(d_invstd), "%s: NULL or misaligned mean / invstd", what);
  GCMI_CHECK_ARG((d_running_mean == nullptr) == (d_running_var == nullptr), "%s: running_mean and running_var go together", what);
  GCMI_CHECK_ARG(eps > 0.f && momentum >= 0.f && momentum <= 1.f, "%s: eps %g must be positive, momentum %g in [0, 1]", what,
                 (double)eps, (double)momentum);
  CG_TRY(check_workspace(what, g, H, d_workspace, workspace_floats_));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const CgRows a = {d_ps, d_pd, d_q, ldp, ldq, H};
  const int parts = grid_parts(g->n_edges, H);
  hipLaunchKernelGGL(cg_stats_kernel, dim3(parts), dim3(kCgThreads), 0, st, *g, a, d_workspace);
  hipLaunchKernelGGL(cg_stats_finish_kernel, dim3((2 * H + 3) / 4), dim3(kCgThreads), 0, st, d_workspace, parts, H, eps, momentum, d_mean,
                     d_invstd, d_running_mean, d_running_var, d_batches_tracked);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

int gcmi_cg_conv_fwd(const gcmi_gn_graph* g, const float* d_ps, const float* d_pd, int64_t ldp, const float* d_q,
                     int64_t ldq, int32_t H, const float* d_mean, const float* d_invstd, const float* d_gamma,
                     const float* d_beta, const float* d_h, int64_t ldh, float* d_out, int64_t ldo, void* stream) {
  const char* what = "cg_conv_fwd";
  CG_TRY(check_cg(what, g, H));
  CG_TRY(check_cg_rows(what, g, H, d_ps, d_pd, ldp, d_q, ldq));
  CG_TRY(check_cg_norm(what, d_mean, d_invstd, d_gamma, d_beta));
  GCMI_CHECK_ARG(rows_ok(d_h, ldh, H), "%s: bad h (NULL, not 16-byte aligned, or ldh < %d or ldh %% 4)", what, H);
  GCMI_CHECK_ARG(rows_ok(d_out, ldo, H) && d_out != d_h, "%s: bad output (NULL, h itself, not 16-byte aligned, or ldo < %d or ldo %% 4)",
                 what, H);
  const CgRows a = {d_ps, d_pd, d_q, ldp, ldq, H};
  const CgNorm n = {d_mean, d_invstd, d_gamma, d_beta};
  hipLaunchKernelGGL(cg_conv_fwd_kernel, dim3(grid_rows(g->n_nodes, H)), dim3(kCgThreads), 0, static_cast<hipStream_t>(stream),
                     *g, a, n, d_h, ldh, d_out, ldo);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

int gcmi_cg_bwd_stats(const gcmi_gn_graph* g, const float* d_ps, const float* d_pd, int64_t ldp, const float* d_q,
                      int64_t ldq, int32_t H, const float* d_mean, const float* d_invstd, const float* d_gamma,
                      const float* d_beta, const float* d_hnew, int64_t ldhn, const float* d_dhnew, int64_t lddh,
                      float* d_sums, float* d_workspace, int64_t workspace_floats_, void* stream) {
  const char* what = "cg_bwd_stats";
  CG_TRY(check_cg(what, g, H));
  GCMI_CHECK_ARG(g->n_edges >= 1, "%s: no edges, nothing to sum", what);
  CG_TRY(check_cg_rows(what, g, H, d_ps, d_pd, ldp, d_q, ldq));
  CG_TRY(check_cg_norm(what, d_mean, d_invstd, d_gamma, d_beta));
  CG_TRY(check_cg_grad(what, H, d_hnew, ldhn, d_dhnew, lddh));
  GCMI_CHECK_ARG(d_sums && aligned16(d_sums), "%s: NULL or misaligned sums", what);
  CG_TRY(check_workspace(what, g, H, d_workspace, workspace_floats_));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const CgRows a = {d_ps, d_pd, d_q, ldp, ldq, H};
  const CgNorm n = {d_mean, d_invstd, d_gamma, d_beta};
  const CgGrad b = {d_hnew, d_dhnew, ldhn, lddh};
  const int parts = grid_parts(g->n_nodes, H);
  hipLaunchKernelGGL(cg_bwd_stats_kernel, dim3(parts), dim3(kCgThreads), 0, st, *g, a, n, b, d_workspace);
  hipLaunchKernelGGL(cg_sums_finish_kernel, dim3(H), dim3(kCgThreads), 0, st, d_workspace, parts, H, d_sums);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

int gcmi_cg_bwd_edges(const gcmi_gn_graph* g, const float* d_ps, const float* d_pd, int64_t ldp, const float* d_q,
                      int64_t ldq, int32_t H, const float* d_mean, const float* d_invstd, const float* d_gamma,
                      const float* d_beta, const float* d_hnew, int64_t ldhn, const float* d_dhnew, int64_t lddh,
                      const float* d_sums, float* d_dq, int64_t lddq, float* d_dpd, int64_t lddp, float* d_dpre,
                      int64_t lddpre, void* stream) {
  const char* what = "cg_bwd_edges";
  CG_TRY(check_cg(what, g, H));
  CG_TRY(check_cg_rows(what, g, H, d_ps, d_pd, ldp, d_q, ldq));
  CG_TRY(check_cg_norm(what, d_mean, d_invstd, d_gamma, d_beta));
  CG_TRY(check_cg_grad(what, H, d_hnew, ldhn, d_dhnew, lddh));
  GCMI_CHECK_ARG(d_sums == nullptr || (aligned16(d_sums) && g->n_edges > 0), "%s: misaligned sums, or sums without edges", what);
  GCMI_CHECK_ARG(g->n_edges == 0 || (rows_ok(d_dq, lddq, 2 * H) && d_dq != d_q),
                 "%s: bad dQ (NULL, Q itself, not 16-byte aligned, or lddq < %d or lddq %% 4)", what, 2 * H);
  GCMI_CHECK_ARG(rows_ok(d_dpd, lddp, 2 * H), "%s: bad dPd (NULL, not 16-byte aligned, or lddp < %d or lddp %% 4)", what, 2 * H);
  GCMI_CHECK_ARG(rows_ok(d_dpre, lddpre, H) && d_dpre != d_dhnew && d_dpre != d_hnew,
                 "%s: bad dpre (NULL, one of the inputs, not 16-byte aligned, or lddpre < %d or lddpre %% 4)", what, H);
  const CgRows a = {d_ps, d_pd, d_q, ldp, ldq, H};
  const CgNorm n = {d_mean, d_invstd, d_gamma, d_beta};
  const CgGrad b = {d_hnew, d_dhnew, ldhn, lddh};
  const float inv_e = g->n_edges > 0 ? 1.f / (float)g->n_edges : 0.f;
  hipLaunchKernelGGL(cg_bwd_edges_kernel, dim3(grid_rows(g->n_nodes, H)), dim3(kCgThreads), 0, static_cast<hipStream_t>(stream),
                     *g, a, n, b, d_sums, inv_e, d_dq, lddq, d_dpd, lddp, d_dpre, lddpre);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

int gcmi_cg_bwd_src(const gcmi_gn_graph* g, const float* d_dq, int64_t lddq, int32_t H, float* d_dps, int64_t lddp,
                    void* stream) {
  const char* what = "cg_bwd_src";
  CG_TRY(check_cg(what, g, H));
  GCMI_CHECK_ARG(g->n_edges == 0 || rows_ok(d_dq, lddq, 2 * H), "%s: bad dQ (NULL, not 16-byte aligned, or lddq < %d or lddq %% 4)",
                 what, 2 * H);
  GCMI_CHECK_ARG(rows_ok(d_dps, lddp, 2 * H), "%s: bad dPs (NULL, not 16-byte aligned, or lddp < %d or lddp %% 4)", what, 2 * H);
  hipLaunchKernelGGL(cg_list_sum_kernel, dim3(grid_rows(g->n_nodes, 2 * H)), dim3(kCgThreads), 0,
                     static_cast<hipStream_t>(stream), g->n_nodes, g->n_edges, g->n_edges, g->out_ptr, g->out_edge, 2 * H, d_dq,
                     lddq, d_dps, lddp);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

}  // extern "C"
