// Graph-network block (MEGNet): everything between the products of one block, on rows of the hidden width 32, fp32.
//
// The reference's block is Linear -> Linear three times without a nonlinearity, over concatenations it builds per
// DIRECTED edge (2E rows for an undirected graph).  With edge_models[0].weight split by columns into A_s | A_d | C | D
// and
//     Ps = x A_s^T, Pd = x A_d^T (N rows), Q = e C^T (E rows), R = u D^T + b1 (G rows)
// the hidden row of the directed edge s -> d of graph g is Ps[s] + Pd[d] + Q[e] + R[g].  What the block needs of them:
//
//     Hs[e] = Q[e] + R[g] + 1/2 ((Ps[s] + Pd[d]) + (Ps[d] + Pd[s]))     undirected: the mean of both directions
//     Hs[e] = Q[e] + R[g] + (Ps[s] + Pd[d])                             directed                       (gn_edge_fwd)
//     Mh[v] = Pd[v] + R[g] + (sum over inc(v) of (Ps[other] + Q[edge])) / |inc(v)|,  0 where inc(v) is empty
//                                                                                                       (gn_node_fwd)
// inc(v) lists (edge, other end) for every directed edge that ARRIVES at v: in undirected mode both ends of every edge
// (a self-loop twice in one list), in directed mode the destination only.  Every later step is linear, so edge_dense
// is applied to Hs and Mh by the caller (one product each), and the per-graph means commute with it (gn_seg: means and
// sums over contiguous row ranges, and their transposes).
//
// Backward, over the same lists (out(v): the edges that LEAVE v, directed mode only):
//     edge pass  dQ = dHs;  undirected dPs[v] = dPd[v] = 1/2 sum over inc(v) of dHs[edge];
//                directed dPd[v] = sum over inc(v), dPs[v] = sum over out(v);  dR[g] = sum over the edges of g
//     node pass  dPd[v] = dMh[v] where inc(v) is non-empty, else 0;  dR[g] = the sum of those rows over the nodes of g;
//                dQ[e] = dMh[d] / |inc(d)| (+ dMh[s] / |inc(s)| undirected);
//                dPs[o] = sum over the entries (edge, v) of inc(o) (undirected) / out(o) (directed) of dMh[v] / |inc(v)|
//
// Layout: a row is 128 bytes; 8 lanes hold it as one float4 each, so a wave moves 8 rows per instruction and a
// workgroup of 256 threads 32 rows.  A node's list is walked by its 8 lanes in list order: no atomics, one owner per
// output element, the same sums in the same order on every run.  No LDS.  Every index read from the device is
// compared with the sizes the host passed before it is used: gcmi_gn_graph_check validates the HOST copy of the lists
// once per batch, the device copy is trusted only inside those bounds.
#include "common.h"

namespace gcmi {
namespace {

constexpr int kGnWidth = GCMI_GN_WIDTH;  // floats per row
constexpr int kGnLanes = kGnWidth / 4;   // lanes per row
constexpr int kGnThreads = 256;          // = GCMI_GN_ROWS_PER_WG rows
static_assert(kGnThreads / kGnLanes == GCMI_GN_ROWS_PER_WG, "rows per workgroup");

__device__ __forceinline__ float4 ld4(const float* p, int64_t row, int64_t ld, int c) {
  return *reinterpret_cast<const float4*>(p + row * ld + c);
}
__device__ __forceinline__ void st4(float* p, int64_t row, int64_t ld, int c, const float4& v) {
  *reinterpret_cast<float4*>(p + row * ld + c) = v;
}
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 scale4(const float4& a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float4 div4(const float4& a, float s) { return make_float4(a.x / s, a.y / s, a.z / s, a.w / s); }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ bool inside(int i, int n) { return (unsigned)i < (unsigned)n; }

// [lo, hi) of entry v of a CSR pointer, cut to [0, n_items]; an inverted pair is an empty range
__device__ __forceinline__ void csr_range(const int32_t* ptr, int v, int n_items, int& lo, int& hi) {
  lo = ptr[v];
  hi = ptr[v + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > n_items ? n_items : hi;
  hi = hi < lo ? lo : hi;
}

struct GnRows {  // the four projections
  const float *ps, *pd, *q, *r;
  int64_t ldp, ldq, ldr;
};

__global__ __launch_bounds__(kGnThreads) void gn_edge_fwd_kernel(gcmi_gn_graph g, GnRows a, float* __restrict__ hs,
                                                                 int64_t ldh) {
  const int64_t total = (int64_t)g.n_edges * kGnLanes, stride = (int64_t)gridDim.x * kGnThreads;
  for (int64_t t = (int64_t)blockIdx.x * kGnThreads + threadIdx.x; t < total; t += stride) {
    const int e = (int)(t / kGnLanes), c = 4 * (int)(t % kGnLanes);
    const int s = g.src[e], d = g.dst[e];
    if (!inside(s, g.n_nodes) || !inside(d, g.n_nodes)) continue;
    const int gi = g.node_graph[s];
    if (!inside(gi, g.n_graphs)) continue;
    float4 p = add4(ld4(a.ps, s, a.ldp, c), ld4(a.pd, d, a.ldp, c));
    if (g.undirected) p = scale4(add4(p, add4(ld4(a.ps, d, a.ldp, c), ld4(a.pd, s, a.ldp, c))), 0.5f);
    st4(hs, e, ldh, c, add4(add4(ld4(a.q, e, a.ldq, c), ld4(a.r, gi, a.ldr, c)), p));
  }
}

__global__ __launch_bounds__(kGnThreads) void gn_node_fwd_kernel(gcmi_gn_graph g, GnRows a, float* __restrict__ mh,
                                                                 int64_t ldm) {
  const int64_t total = (int64_t)g.n_nodes * kGnLanes, stride = (int64_t)gridDim.x * kGnThreads;
  for (int64_t t = (int64_t)blockIdx.x * kGnThreads + threadIdx.x; t < total; t += stride) {
    const int v = (int)(t / kGnLanes), c = 4 * (int)(t % kGnLanes);
    int lo, hi;
    csr_range(g.inc_ptr, v, g.n_inc, lo, hi);
    const int gi = g.node_graph[v];
    float4 out = zero4();
    if (hi > lo && inside(gi, g.n_graphs)) {
      float4 acc = zero4();
      for (int k = lo; k < hi; ++k) {
        const int e = g.inc_edge[k], o = g.inc_other[k];
        if (!inside(e, g.n_edges) || !inside(o, g.n_nodes)) continue;
        acc = add4(acc, add4(ld4(a.ps, o, a.ldp, c), ld4(a.q, e, a.ldq, c)));
      }
      out = add4(add4(ld4(a.pd, v, a.ldp, c), ld4(a.r, gi, a.ldr, c)), div4(acc, (float)(hi - lo)));
    }
    st4(mh, v, ldm, c, out);
  }
}

// out[v] = scale * sum over list(v) of rows[edge]; out2 (optional) gets the same rows.  The edge pass's dPs / dPd.
__global__ __launch_bounds__(kGnThreads) void gn_edge_sum_kernel(int32_t n_nodes, int32_t n_edges, int32_t n_list,
                                                                 const int32_t* __restrict__ ptr,
                                                                 const int32_t* __restrict__ list_edge,
                                                                 const float* __restrict__ rows, int64_t ldr, float scale,
                                                                 float* __restrict__ out, float* __restrict__ out2,
                                                                 int64_t ldo) {
  const int64_t total = (int64_t)n_nodes * kGnLanes, stride = (int64_t)gridDim.x * kGnThreads;
  for (int64_t t = (int64_t)blockIdx.x * kGnThreads + threadIdx.x; t < total; t += stride) {
    const int v = (int)(t / kGnLanes), c = 4 * (int)(t % kGnLanes);
    int lo, hi;
    csr_range(ptr, v, n_list, lo, hi);
    float4 acc = zero4();
    for (int k = lo; k < hi; ++k) {
      const int e = list_edge[k];
      if (inside(e, n_edges)) acc = add4(acc, ld4(rows, e, ldr, c));
    }
    acc = scale4(acc, scale);
    st4(out, v, ldo, c, acc);
    if (out2) st4(out2, v, ldo, c, acc);
  }
}

__device__ __forceinline__ int inc_count(const gcmi_gn_graph& g, int v) {
  int lo, hi;
  csr_range(g.inc_ptr, v, g.n_inc, lo, hi);
  return hi - lo;
}

// The node pass's dQ: one row per edge
__global__ __launch_bounds__(kGnThreads) void gn_node_bwd_edges_kernel(gcmi_gn_graph g, const float* __restrict__ dmh,
                                                                       int64_t ldm, float* __restrict__ dq, int64_t ldq) {
  const int64_t total = (int64_t)g.n_edges * kGnLanes, stride = (int64_t)gridDim.x * kGnThreads;
  for (int64_t t = (int64_t)blockIdx.x * kGnThreads + threadIdx.x; t < total; t += stride) {
    const int e = (int)(t / kGnLanes), c = 4 * (int)(t % kGnLanes);
    const int s = g.src[e], d = g.dst[e];
    float4 out = zero4();
    if (inside(s, g.n_nodes) && inside(d, g.n_nodes)) {
      const int cd = inc_count(g, d);
      if (cd > 0) out = div4(ld4(dmh, d, ldm, c), (float)cd);
      if (g.undirected) {
        const int cs = inc_count(g, s);
        if (cs > 0) out = add4(out, div4(ld4(dmh, s, ldm, c), (float)cs));
      }
    }
    st4(dq, e, ldq, c, out);
  }
}

// The node pass's dPs and dPd: one row of each per node; list = inc (undirected) or out (directed)
__global__ __launch_bounds__(kGnThreads) void gn_node_bwd_nodes_kernel(gcmi_gn_graph g, const int32_t* __restrict__ ptr,
                                                                       const int32_t* __restrict__ list_other,
                                                                       int32_t n_list, const float* __restrict__ dmh,
                                                                       int64_t ldm, float* __restrict__ dps,
                                                                       float* __restrict__ dpd, int64_t ldp) {
  const int64_t total = (int64_t)g.n_nodes * kGnLanes, stride = (int64_t)gridDim.x * kGnThreads;
  for (int64_t t = (int64_t)blockIdx.x * kGnThreads + threadIdx.x; t < total; t += stride) {
    const int o = (int)(t / kGnLanes), c = 4 * (int)(t % kGnLanes);
    int lo, hi;
    csr_range(ptr, o, n_list, lo, hi);
    float4 acc = zero4();
    for (int k = lo; k < hi; ++k) {
      const int v = list_other[k];
      if (!inside(v, g.n_nodes)) continue;
      const int cv = inc_count(g, v);
      if (cv > 0) acc = add4(acc, div4(ld4(dmh, v, ldm, c), (float)cv));
    }
    st4(dps, o, ldp, c, acc);
    st4(dpd, o, ldp, c, inc_count(g, o) > 0 ? ld4(dmh, o, ldm, c) : zero4());
  }
}

// Contiguous row ranges [ptr[s], ptr[s + 1]): one thread per (range, column), rows in order.
//   kSegMean: out[s] = mean of the rows (0 for an empty range); kSegSum: their sum;
//   kSegSpread / kSegSpreadMean (their transposes): rows[r] = x[s] (/ count) for the rows of range s.
enum SegMode { kSegMean = 0, kSegSum = 1, kSegSpread = 2, kSegSpreadMean = 3 };
template <int MODE>
__global__ __launch_bounds__(kGnThreads) void gn_seg_kernel(const int32_t* __restrict__ ptr, int32_t n_seg, int32_t n_rows,
                                                            int32_t width, const float* __restrict__ x, int64_t ldx,
                                                            float* __restrict__ out, int64_t ldo) {
  const int64_t total = (int64_t)n_seg * width, stride = (int64_t)gridDim.x * kGnThreads;
  for (int64_t t = (int64_t)blockIdx.x * kGnThreads + threadIdx.x; t < total; t += stride) {
    const int s = (int)(t / width), c = (int)(t % width);
    int lo, hi;
    csr_range(ptr, s, n_rows, lo, hi);
    if constexpr (MODE == kSegSpread || MODE == kSegSpreadMean) {
      if (hi > lo) {
        const float v = MODE == kSegSpreadMean ? x[s * ldx + c] / (float)(hi - lo) : x[s * ldx + c];
        for (int r = lo; r < hi; ++r) out[r * ldo + c] = v;
      }
    } else {
      float acc = 0.f;
      for (int r = lo; r < hi; ++r) acc += x[r * ldx + c];
      if (MODE == kSegMean && hi > lo) acc /= (float)(hi - lo);
      out[s * ldo + c] = acc;
    }
  }
}

bool rows_ok(const void* p, int64_t ld) { return p && aligned16(p) && ld >= kGnWidth && ld % 4 == 0; }

// The sizes and pointers of a description whose lists live on the DEVICE (they are not followed here)
int check_gn_desc(const char* what, const gcmi_gn_graph* g) {
  GCMI_CHECK_ARG(g != nullptr, "%s: NULL graph", what);
  GCMI_CHECK_ARG(g->n_nodes > 0 && g->n_graphs > 0 && g->n_edges >= 0 && g->n_graphs <= g->n_nodes,
                 "%s: n_nodes %d, n_edges %d, n_graphs %d (nodes and graphs must be positive, every graph holds a node)",
                 what, g->n_nodes, g->n_edges, g->n_graphs);
  GCMI_CHECK_ARG(g->undirected == 0 || g->undirected == 1, "%s: undirected must be 0 or 1", what);
  GCMI_CHECK_ARG((int64_t)g->n_inc == (int64_t)g->n_edges * (g->undirected ? 2 : 1) && (int64_t)g->n_edges * 2 < INT32_MAX,
                 "%s: n_inc %d is not %s n_edges", what, g->n_inc, g->undirected ? "2 x" : "");
  GCMI_CHECK_ARG(g->node_graph && g->node_ptr && g->edge_ptr && g->inc_ptr, "%s: NULL node_graph / node_ptr / edge_ptr / inc_ptr",
                 what);
  GCMI_CHECK_ARG(g->n_edges == 0 || (g->src && g->dst && g->inc_edge && g->inc_other), "%s: NULL edge or incidence list",
                 what);
  GCMI_CHECK_ARG(g->undirected || (g->out_ptr && (g->n_edges == 0 || (g->out_edge && g->out_other))),
                 "%s: a directed graph needs the lists sorted by source (out_ptr, out_edge, out_other)", what);
  return GCMI_OK;
}

int check_gn_rows(const char* what, const gcmi_gn_graph* g, const float* ps, const float* pd, int64_t ldp, const float* q,
                  int64_t ldq, const float* r, int64_t ldr) {
  GCMI_CHECK_ARG(rows_ok(ps, ldp) && rows_ok(pd, ldp), "%s: bad Ps / Pd (NULL, not 16-byte aligned, or ldp < %d or ldp %% 4)", what,
                 kGnWidth);
  GCMI_CHECK_ARG(g->n_edges == 0 || rows_ok(q, ldq), "%s: bad Q (NULL, not 16-byte aligned, or ldq < %d or ldq %% 4)", what,
                 kGnWidth);
  GCMI_CHECK_ARG(rows_ok(r, ldr), "%s: bad R (NULL, not 16-byte aligned, or ldr < %d or ldr %% 4)", what, kGnWidth);
  return GCMI_OK;
}

template <int MODE>
int launch_seg(const char* what, const int32_t* d_ptr, int32_t n_seg, int32_t n_rows, int32_t width, const float* d_x,
               int64_t ldx, float* d_out, int64_t ldo, hipStream_t st) {
  GCMI_CHECK_ARG(d_ptr && n_seg > 0 && n_rows >= 0 && width > 0, "%s: NULL ptr, or n_seg %d / n_rows %d / width %d", what, n_seg,
                 n_rows, width);
  GCMI_CHECK_ARG(d_x && d_out && ldx >= width && ldo >= width, "%s: NULL rows, or a leading dimension below the width %d", what,
                 width);
  hipLaunchKernelGGL(gn_seg_kernel<MODE>, dim3(grid_for((int64_t)n_seg * width, kGnThreads)), dim3(kGnThreads), 0, st, d_ptr,
                     n_seg, n_rows, width, d_x, ldx, d_out, ldo);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

}  // namespace
}  // namespace gcmi

using namespace gcmi;

extern "C" {

int gcmi_gn_graph_check(const gcmi_gn_graph* h) {
  const char* what = "gn_graph_check";
  const int rc = check_gn_desc(what, h);
  if (rc != GCMI_OK) return rc;
  const int N = h->n_nodes, E = h->n_edges, G = h->n_graphs;
  GCMI_CHECK_ARG(h->node_ptr[0] == 0 && h->node_ptr[G] == N && h->edge_ptr[0] == 0 && h->edge_ptr[G] == E,
                 "%s: node_ptr / edge_ptr must run from 0 to n_nodes / n_edges", what);
  for (int gi = 0; gi < G; ++gi) {
    GCMI_CHECK_ARG(h->node_ptr[gi + 1] > h->node_ptr[gi], "%s: graph %d has no node (node_ptr must increase)", what, gi);
    GCMI_CHECK_ARG(h->edge_ptr[gi + 1] >= h->edge_ptr[gi], "%s: edge_ptr decreases at graph %d", what, gi);
    GCMI_CHECK_ARG(h->node_ptr[gi + 1] <= N && h->edge_ptr[gi + 1] <= E, "%s: node_ptr / edge_ptr of graph %d past the end", what, gi);
    for (int v = h->node_ptr[gi]; v < h->node_ptr[gi + 1]; ++v)
      GCMI_CHECK_ARG(h->node_graph[v] == gi, "%s: node_graph[%d] = %d, node_ptr says %d", what, v, h->node_graph[v], gi);
    for (int e = h->edge_ptr[gi]; e < h->edge_ptr[gi + 1]; ++e) {
      const int s = h->src[e], d = h->dst[e];
      GCMI_CHECK_ARG(s >= 0 && s < N && d >= 0 && d < N, "%s: edge %d (%d -> %d) leaves the %d nodes", what, e, s, d, N);
      GCMI_CHECK_ARG(h->node_graph[s] == gi && h->node_graph[d] == gi, "%s: edge %d (%d -> %d) is not inside graph %d", what, e, s,
                     d, gi);
    }
  }
  auto check_list = [&](const char* name, const int32_t* ptr, const int32_t* le, const int32_t* lo, int n_list,
                        bool arriving) -> int {
    GCMI_CHECK_ARG(ptr[0] == 0 && ptr[N] == n_list, "%s: %s_ptr must run from 0 to %d", what, name, n_list);
    for (int v = 0; v < N; ++v) {
      GCMI_CHECK_ARG(ptr[v + 1] >= ptr[v], "%s: %s_ptr decreases at node %d", what, name, v);
      GCMI_CHECK_ARG(ptr[v + 1] <= n_list, "%s: %s_ptr of node %d past the end", what, name, v);
      for (int k = ptr[v]; k < ptr[v + 1]; ++k) {
        const int e = le[k], o = lo[k];
        GCMI_CHECK_ARG(e >= 0 && e < E && o >= 0 && o < N, "%s: %s entry %d (edge %d, node %d) out of range", what, name, k, e, o);
        const int s = h->src[e], d = h->dst[e];
        const bool fwd = arriving ? (d == v && s == o) : (s == v && d == o);
        const bool flipped = h->undirected && s == v && d == o;
        GCMI_CHECK_ARG(fwd || flipped, "%s: %s entry %d (edge %d, node %d) in the list of node %d is not edge %d -> %d", what, name,
                       k, e, o, v, s, d);
      }
    }
    return GCMI_OK;
  };
  int rc2 = check_list("inc", h->inc_ptr, h->inc_edge, h->inc_other, h->n_inc, true);
  if (rc2 != GCMI_OK) return rc2;
  if (!h->undirected) {
    rc2 = check_list("out", h->out_ptr, h->out_edge, h->out_other, E, false);
    if (rc2 != GCMI_OK) return rc2;
  }
  // every edge the right number of times: with the membership test above that makes each list a permutation
  const int per_edge = h->undirected ? 2 : 1;
  for (int pass = 0; pass < (h->undirected ? 1 : 2); ++pass) {
    const int32_t* le = pass == 0 ? h->inc_edge : h->out_edge;
    const int n_list = pass == 0 ? h->n_inc : E;
    int32_t* seen = static_cast<int32_t*>(calloc(E > 0 ? E : 1, sizeof(int32_t)));
    GCMI_CHECK_ARG(seen != nullptr, "%s: out of memory", what);
    for (int k = 0; k < n_list; ++k) ++seen[le[k]];
    int bad = -1;
    for (int e = 0; e < E && bad < 0; ++e) bad = seen[e] != per_edge ? e : -1;
    free(seen);
    GCMI_CHECK_ARG(bad < 0, "%s: edge %d is not listed %d time(s)", what, bad, per_edge);
  }
  return GCMI_OK;
}

int gcmi_gn_edge_fwd(const gcmi_gn_graph* g, const float* d_ps, const float* d_pd, int64_t ldp, const float* d_q, int64_t ldq,
                     const float* d_r, int64_t ldr, float* d_hs, int64_t ldh, void* stream) {
  int rc = check_gn_desc("gn_edge_fwd", g);
  if (rc != GCMI_OK) return rc;
  rc = check_gn_rows("gn_edge_fwd", g, d_ps, d_pd, ldp, d_q, ldq, d_r, ldr);
  if (rc != GCMI_OK) return rc;
  if (g->n_edges == 0) return GCMI_OK;
  GCMI_CHECK_ARG(rows_ok(d_hs, ldh), "gn_edge_fwd: bad output (NULL, not 16-byte aligned, or ldh < %d or ldh %% 4)", kGnWidth);
  const GnRows a = {d_ps, d_pd, d_q, d_r, ldp, ldq, ldr};
  hipLaunchKernelGGL(gn_edge_fwd_kernel, dim3(grid_for((int64_t)g->n_edges * kGnLanes, kGnThreads)), dim3(kGnThreads), 0,
                     static_cast<hipStream_t>(stream), *g, a, d_hs, ldh);
  GCMI_CHECK_LAUNCH("gn_edge_fwd");
  return GCMI_OK;
}

int gcmi_gn_node_fwd(const gcmi_gn_graph* g, const float* d_ps, const float* d_pd, int64_t ldp, const float* d_q, int64_t ldq,
                     const float* d_r, int64_t ldr, float* d_mh, int64_t ldm, void* stream) {
  int rc = check_gn_desc("gn_node_fwd", g);
  if (rc != GCMI_OK) return rc;
  rc = check_gn_rows("gn_node_fwd", g, d_ps, d_pd, ldp, d_q, ldq, d_r, ldr);
  if (rc != GCMI_OK) return rc;
  GCMI_CHECK_ARG(rows_ok(d_mh, ldm), "gn_node_fwd: bad output (NULL, not 16-byte aligned, or ldm < %d or ldm %% 4)", kGnWidth);
  const GnRows a = {d_ps, d_pd, d_q, d_r, ldp, ldq, ldr};
  hipLaunchKernelGGL(gn_node_fwd_kernel, dim3(grid_for((int64_t)g->n_nodes * kGnLanes, kGnThreads)), dim3(kGnThreads), 0,
                     static_cast<hipStream_t>(stream), *g, a, d_mh, ldm);
  GCMI_CHECK_LAUNCH("gn_node_fwd");
  return GCMI_OK;
}

int gcmi_gn_edge_bwd(const gcmi_gn_graph* g, const float* d_dhs, int64_t ldh, float* d_dps, float* d_dpd, int64_t ldp,
                     float* d_dr, int64_t ldr, void* stream) {
  const int rc = check_gn_desc("gn_edge_bwd", g);
  if (rc != GCMI_OK) return rc;
  GCMI_CHECK_ARG(g->n_edges == 0 || rows_ok(d_dhs, ldh), "gn_edge_bwd: bad dHs (NULL, not 16-byte aligned, or ldh < %d or ldh %% 4)",
                 kGnWidth);
  GCMI_CHECK_ARG(rows_ok(d_dps, ldp) && rows_ok(d_dpd, ldp) && d_dps != d_dpd,
                 "gn_edge_bwd: bad dPs / dPd (NULL, one buffer, not 16-byte aligned, or ldp < %d or ldp %% 4)", kGnWidth);
  GCMI_CHECK_ARG(rows_ok(d_dr, ldr), "gn_edge_bwd: bad dR (NULL, not 16-byte aligned, or ldr < %d or ldr %% 4)", kGnWidth);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(grid_for((int64_t)g->n_nodes * kGnLanes, kGnThreads)), block(kGnThreads);
  if (g->undirected) {
    hipLaunchKernelGGL(gn_edge_sum_kernel, grid, block, 0, st, g->n_nodes, g->n_edges, g->n_inc, g->inc_ptr, g->inc_edge, d_dhs,
                       ldh, 0.5f, d_dps, d_dpd, ldp);
  } else {
    hipLaunchKernelGGL(gn_edge_sum_kernel, grid, block, 0, st, g->n_nodes, g->n_edges, g->n_inc, g->inc_ptr, g->inc_edge, d_dhs,
                       ldh, 1.f, d_dpd, static_cast<float*>(nullptr), ldp);
    hipLaunchKernelGGL(gn_edge_sum_kernel, grid, block, 0, st, g->n_nodes, g->n_edges, g->n_edges, g->out_ptr, g->out_edge,
                       d_dhs, ldh, 1.f, d_dps, static_cast<float*>(nullptr), ldp);
  }
  GCMI_CHECK_LAUNCH("gn_edge_bwd");
  // (without edges every range is empty and no row of the first operand is read)
  const bool none = g->n_edges == 0;
  return launch_seg<kSegSum>("gn_edge_bwd", g->edge_ptr, g->n_graphs, g->n_edges, kGnWidth, none ? d_dr : d_dhs, none ? ldr : ldh,
                             d_dr, ldr, st);
}

int gcmi_gn_node_bwd(const gcmi_gn_graph* g, const float* d_dmh, int64_t ldm, float* d_dq, int64_t ldq, float* d_dps,
                     float* d_dpd, int64_t ldp, float* d_dr, int64_t ldr, void* stream) {
  const int rc = check_gn_desc("gn_node_bwd", g);
  if (rc != GCMI_OK) return rc;
  GCMI_CHECK_ARG(rows_ok(d_dmh, ldm), "gn_node_bwd: bad dMh (NULL, not 16-byte aligned, or ldm < %d or ldm %% 4)", kGnWidth);
  GCMI_CHECK_ARG(g->n_edges == 0 || rows_ok(d_dq, ldq), "gn_node_bwd: bad dQ (NULL, not 16-byte aligned, or ldq < %d or ldq %% 4)",
                 kGnWidth);
  GCMI_CHECK_ARG(rows_ok(d_dps, ldp) && rows_ok(d_dpd, ldp) && d_dps != d_dpd,
                 "gn_node_bwd: bad dPs / dPd (NULL, one buffer, not 16-byte aligned, or ldp < %d or ldp %% 4)", kGnWidth);
  GCMI_CHECK_ARG(rows_ok(d_dr, ldr), "gn_node_bwd: bad dR (NULL, not 16-byte aligned, or ldr < %d or ldr %% 4)", kGnWidth);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (g->n_edges > 0)
    hipLaunchKernelGGL(gn_node_bwd_edges_kernel, dim3(grid_for((int64_t)g->n_edges * kGnLanes, kGnThreads)), dim3(kGnThreads), 0,
                       st, *g, d_dmh, ldm, d_dq, ldq);
  const bool und = g->undirected != 0;
  hipLaunchKernelGGL(gn_node_bwd_nodes_kernel, dim3(grid_for((int64_t)g->n_nodes * kGnLanes, kGnThreads)), dim3(kGnThreads), 0,
                     st, *g, und ? g->inc_ptr : g->out_ptr, und ? g->inc_other : g->out_other, und ? g->n_inc : g->n_edges, d_dmh,
                     ldm, d_dps, d_dpd, ldp);
  GCMI_CHECK_LAUNCH("gn_node_bwd");
  return launch_seg<kSegSum>("gn_node_bwd", g->node_ptr, g->n_graphs, g->n_nodes, kGnWidth, d_dpd, ldp, d_dr, ldr, st);
}

int gcmi_gn_seg_reduce(const int32_t* d_ptr, int32_t n_seg, int32_t n_rows, int32_t width, int32_t mean, const float* d_x,
                       int64_t ldx, float* d_out, int64_t ldo, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCMI_CHECK_ARG(mean == 0 || mean == 1, "gn_seg_reduce: mean must be 0 or 1");
  return mean ? launch_seg<kSegMean>("gn_seg_reduce", d_ptr, n_seg, n_rows, width, d_x, ldx, d_out, ldo, st)
              : launch_seg<kSegSum>("gn_seg_reduce", d_ptr, n_seg, n_rows, width, d_x, ldx, d_out, ldo, st);
}

int gcmi_gn_seg_spread(const int32_t* d_ptr, int32_t n_seg, int32_t n_rows, int32_t width, int32_t mean, const float* d_x,
                       int64_t ldx, float* d_out, int64_t ldo, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCMI_CHECK_ARG(mean == 0 || mean == 1, "gn_seg_spread: mean must be 0 or 1");
  return mean ? launch_seg<kSegSpreadMean>("gn_seg_spread", d_ptr, n_seg, n_rows, width, d_x, ldx, d_out, ldo, st)
              : launch_seg<kSegSpread>("gn_seg_spread", d_ptr, n_seg, n_rows, width, d_x, ldx, d_out, ldo, st);
}

}  // extern "C"
