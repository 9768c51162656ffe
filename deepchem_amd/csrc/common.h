// Shared host/device helpers for libgcmi.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <stdlib.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/gcmi.h"

namespace gcmi {

void set_error(const char* fmt, ...);
// 0 / 1 alternately: whether the next row-streaming launch walks its rows backwards (core.cpp)
int next_sweep_direction();

// Dynamic-LDS limit of one kernel, raised once per device: hipFuncSetAttribute acts on the current device only, so the
// cache is keyed by hipGetDevice (one static LdsLimit per kernel instantiation).  raise_lds_limit returns 0 when HIP
// refuses the limit (its error cleared, nothing cached); otherwise, with threads > 0, how many workgroups of `threads`
// threads with `shmem` bytes of dynamic LDS one CU of this device holds (2 where HIP cannot say), else 1.
constexpr int kMaxDev = 64;
struct LdsLimit {
  std::atomic<int> per_cu[kMaxDev];
};
int raise_lds_limit(LdsLimit& a, const void* kern, size_t lds_bytes, int threads = 0, size_t shmem = 0);

#define GCMI_CHECK_ARG(cond, ...)          \
  do {                                     \
    if (!(cond)) {                         \
      ::gcmi::set_error(__VA_ARGS__);      \
      return GCMI_ERR_ARG;                 \
    }                                      \
  } while (0)

#define GCMI_CHECK_LAUNCH(what)                                                        \
  do {                                                                                 \
    hipError_t e__ = hipGetLastError();                                                \
    if (e__ != hipSuccess) {                                                           \
      ::gcmi::set_error("%s: %s", what, hipGetErrorString(e__));                       \
      return GCMI_ERR_LAUNCH;                                                          \
    }                                                                                  \
  } while (0)

// Per-kernel-family timing (bench.py roofline): events recorded on the launch stream.
void timing_begin(int kernel_id, hipStream_t s);
void timing_end(int kernel_id, hipStream_t s);

struct TimedScope {
  int id;
  hipStream_t s;
  TimedScope(int id_, hipStream_t s_) : id(id_), s(s_) { timing_begin(id, s); }
  ~TimedScope() { timing_end(id, s); }
};

// The degree blocks of a collated batch, passed BY VALUE to kernels (lives in
// SGPRs / the kernarg segment: no memory traffic for row -> degree lookups).
struct DegTable {
  int32_t max_deg;
  int32_t deg_start[GCMI_MAX_DEG + 2];
  int32_t edge_start[GCMI_MAX_DEG + 2];
};

inline DegTable make_deg_table(const gcmi_graph* g) {
  DegTable t;
  t.max_deg = g->max_deg;
  for (int d = 0; d < GCMI_MAX_DEG + 2; ++d) {
    t.deg_start[d] = g->deg_start[d < g->max_deg + 1 ? d : g->max_deg + 1];
    t.edge_start[d] = g->edge_start[d < g->max_deg + 1 ? d : g->max_deg + 1];
  }
  return t;
}

int check_graph(const gcmi_graph* g, bool need_cols);

// LDS-window forms of the gather kernels (gather_lds.hip)
bool win_usable(const gcmi_graph* g, int n_feat, bool aux);
bool win_has_width(int n_feat);
int win_gather_sum(const gcmi_graph* g, const float* d_x, int64_t ldx, int n_feat, float* d_s,
                   int64_t lds, hipStream_t st, bool accumulate = false);
int win_gather_max(const gcmi_graph* g, const float* d_x, int64_t ldx, int n_feat, const float* d_scale,
                   const float* d_shift, float* d_out, int64_t ldo, uint8_t* d_arg, hipStream_t st);
int win_gather_max_bwd(const gcmi_graph* g, const float* d_dout, int64_t lddo, int n_feat,
                       const uint8_t* d_arg, float* d_dx, int64_t lddx, hipStream_t st);
// SumOp<true> followed by the GraphPool backward of the block below in one window pass, dX in LDS only
bool win_two_stage_usable(const gcmi_graph* g, int n_feat);
int win_gather_sumacc_max_bwd(const gcmi_graph* g, const float* d_ds, int64_t ldds, int n_feat, float* d_dxs,
                              int64_t lddxs, const uint8_t* d_arg, float* d_dy, int64_t lddy, hipStream_t st);
// GraphPool followed by the neighbour sum of the block above in one window pass (n_feat 64 / 128): the pooled rows are
// written but not read back
bool win_max_sum_usable(const gcmi_graph* g, int n_feat);
int win_gather_max_sum(const gcmi_graph* g, const float* d_y, int64_t ldy, int n_feat, const float* d_scale,
                       const float* d_shift, float* d_pool, int64_t ldp, uint8_t* d_arg, float* d_s, int64_t lds,
                       hipStream_t st);
int max_sum_launches();  // launches of that pass so far (tests)
// the GraphPool backward that returns at once unless the pooled BatchNorm sums are ill-conditioned (BnBackward::psums)
int win_gather_max_bwd_if_ill(const gcmi_graph* g, const float* d_dout, int64_t lddo, int n_feat, const uint8_t* d_arg,
                              float* d_dx, int64_t lddx, const float* d_gamma, const float* d_beta, hipStream_t st);
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline int64_t up4(int64_t n) { return (n + 3) / 4 * 4; }  // floats of a 16-byte aligned block
inline int64_t up8(int64_t n) { return (n + 7) / 8 * 8; }  // bf16 elements of one

// ---- One segmented forward product,
//     out[rows of s] = act(a1[rows of s] . w1[s] + a2[rows of s] . w2[s] + bias[s])      for the row segments s,
// as its kernels are handed it (gemm.hip, gemm_split.hip, fwd_fused.hip, fwd_bf16.hip).  TA / TO = element type of the
// operand / output rows: float, or unsigned short for rows stored as raw bf16 patterns (leading dimensions in elements).
template <typename TA>
struct SegOperand {
  const TA* a = nullptr;           // rows; nullptr: term absent
  int64_t ld = 0;
  int32_t k = 0;                   // columns contracted
  const float* w = nullptr;        // weights, k x n_out per segment (trans_w: n_out x k, nn.Linear)
  const int64_t* w_off = nullptr;  // per segment: where its block starts in w; < 0: term absent in that segment
};
template <typename TA, typename TO = TA>
struct SegProduct {
  int32_t n_seg = 0;
  const int32_t* seg_begin = nullptr;  // rows [seg_begin[s], seg_end[s])
  const int32_t* seg_end = nullptr;
  SegOperand<TA> op[2];
  const float* bias = nullptr;
  const int64_t* bias_off = nullptr;  // per segment, into bias; < 0: none
  int32_t n_out = 0;
  int32_t trans_w = 0;
  int32_t act = 0;  // 0 none, 1 ReLU, 2 out += result
  TO* out = nullptr;
  int64_t ldo = 0;
};

// One segment, rows [0, *n_rows) of one operand against one weight block and bias row (the dense layer, the task head
// and their input gradients; callers set trans_w and act by name).  The description holds pointers: *n_rows must
// outlive it.
inline constexpr int32_t kZero32 = 0;
inline constexpr int64_t kZero64 = 0;
template <typename TA, typename TO>
inline SegProduct<TA, TO> one_segment(const int32_t* n_rows, const TA* a, int64_t lda, int32_t k, const float* w,
                                      const float* bias, int32_t n_out, TO* out, int64_t ldo) {
  SegProduct<TA, TO> p;
  p.n_seg = 1;
  p.seg_begin = &kZero32;
  p.seg_end = n_rows;
  p.op[0] = {a, lda, k, w, &kZero64};
  p.bias = bias;
  p.bias_off = bias ? &kZero64 : nullptr;
  p.n_out = n_out;
  p.out = out;
  p.ldo = ldo;
  return p;
}

// The shapes of the default model that the persistent forward kernels cover (fwd_fused.hip in split-bf16 mode,
// fwd_bf16.hip over bf16 rows):
//   kFwdConv80  two operands of 65..80 columns -> 64 columns (the first GraphConv)
//   kFwdConv    two operands of 33..64 columns -> 64 columns (GraphConv over pooled rows)
//   kFwdDense   one operand of 33..64 columns -> 128 columns in nn.Linear layout (the atom-level dense layer)
// with no activation or ReLU, 16-byte addressable rows (ld a multiple of 4 floats / 8 bf16 elements) and 32-bit
// element offsets (rows * ld < 2^30).  Anything else: kFwdNone, and the caller answers GCMI_ERR_UNSUPPORTED.
constexpr int kMaxProductSeg = 16;  // segments of a product: the size of SegTable below, which every product kernel takes
enum FwdShape { kFwdNone = 0, kFwdConv80, kFwdConv, kFwdDense };
template <typename TA, typename TO>
inline FwdShape fwd_shape(const SegProduct<TA, TO>& p) {
  const SegOperand<TA>&a1 = p.op[0], &a2 = p.op[1];
  if (p.n_seg > kMaxProductSeg || (p.act != 0 && p.act != 1) || a1.a == nullptr) return kFwdNone;
  const bool two = a2.a != nullptr;
  const bool conv_like = two && !p.trans_w && p.n_out == 64 && a1.k == a2.k;
  const FwdShape shape = (conv_like && a1.k > 64 && a1.k <= 80)                            ? kFwdConv80
                         : (conv_like && a1.k > 32 && a1.k <= 64)                          ? kFwdConv
                         : (!two && p.trans_w && p.n_out == 128 && a1.k > 32 && a1.k <= 64) ? kFwdDense
                                                                                           : kFwdNone;
  if (shape == kFwdNone) return kFwdNone;
  constexpr int64_t kPiece = 16 / sizeof(TA);  // elements of a 16-byte piece of an operand row
  if (!aligned16(a1.a) || a1.ld % kPiece || (two && (!aligned16(a2.a) || a2.ld % kPiece)) || !aligned16(p.out) ||
      p.ldo % kPiece || p.ldo < p.n_out || (p.bias && !aligned16(p.bias)))
    return kFwdNone;
  int64_t rows = 0;
  for (int s = 0; s < p.n_seg; ++s) rows = std::max<int64_t>(rows, p.seg_end[s]);
  if (rows * std::max(std::max(a1.ld, two ? a2.ld : 0), p.ldo) >= (int64_t)1 << 30) return kFwdNone;
  return shape;
}
// ---- The per-segment table every segmented kernel takes BY VALUE (kernarg segment / SGPRs): the forward products of
// gemm.hip, gemm_split.hip, fwd_fused.hip and fwd_bf16.hip and the one-pass backward of bwd_fused.hip.  For tiles of
// tile_rows rows: the segments, the first tile of each (tile_start[kMaxProductSeg] = the total), and per segment the
// offsets into the weight array of either operand and into the bias (-1 = absent; slots past n_seg are zeroed).
struct SegTable {
  int32_t n_seg;
  int32_t seg_begin[kMaxProductSeg];
  int32_t seg_end[kMaxProductSeg];
  int32_t tile_start[kMaxProductSeg + 1];
  int64_t w_off[2][kMaxProductSeg];  // weight block of operand o (backward: the same block of the gradient); < 0: term absent
  int64_t b_off[kMaxProductSeg];     // bias row (backward: the bias-GRADIENT row); < 0: none
};
// Fills it from raw per-segment arrays (a nullptr offset array = that term absent everywhere; no bounds = no rows, for a
// kernel that reads the offsets only); returns the number of tiles.
inline int64_t fill_seg_table(SegTable& st, int32_t n_seg, const int32_t* seg_begin, const int32_t* seg_end,
                              const int64_t* w0_off, const int64_t* w1_off, const int64_t* b_off, int tile_rows) {
  memset(&st, 0, sizeof(st));
  st.n_seg = n_seg;
  int64_t tiles = 0;
  for (int s = 0; s < kMaxProductSeg; ++s) {
    const bool in = s < n_seg;
    st.tile_start[s] = (int32_t)tiles;
    const bool rows = in && seg_begin && seg_end;
    st.seg_begin[s] = rows ? seg_begin[s] : 0;
    st.seg_end[s] = rows ? seg_end[s] : 0;
    st.w_off[0][s] = (in && w0_off) ? w0_off[s] : -1;
    st.w_off[1][s] = (in && w1_off) ? w1_off[s] : -1;
    st.b_off[s] = (in && b_off) ? b_off[s] : -1;
    if (rows) tiles += (seg_end[s] - seg_begin[s] + tile_rows - 1) / tile_rows;
  }
  st.tile_start[kMaxProductSeg] = (int32_t)tiles;
  return tiles;
}
template <typename TA, typename TO>
inline int64_t fill_seg_table(SegTable& st, const SegProduct<TA, TO>& p, int tile_rows) {
  return fill_seg_table(st, p.n_seg, p.seg_begin, p.seg_end, p.op[0].a ? p.op[0].w_off : nullptr,
                        p.op[1].a ? p.op[1].w_off : nullptr, p.bias ? p.bias_off : nullptr, tile_rows);
}

// ---- The backward half of the step and every BatchNorm entry point, as their launchers are handed them (bn.hip,
// bwd_fused.hip, head_bwd.hip).  Host side only: what a kernel takes by value, its launcher builds from these.

// Synchronised BatchNorm (gcmi_model_*_dp): with a BnSync the backward entries below, after their sums, write THIS
// rank's dgamma / dbeta, exchange [sum dy | sum dy xhat | rows] through the callback and make the coefficient vectors
// of the global batch; the forward exchanges [sum x | sum x^2 | rows] the same way.  A rank without rows
// (n_rows == 0) takes part in every exchange with zero sums.  buf: 2F + 1 doubles.
struct BnSync {
  gcmi_stat_sync_fn fn;
  void* ctx;
  double* buf;
};

// One BatchNorm point: nn.BatchNorm1d(n_feat) and where its vectors live
struct BnPoint {
  int32_t n_feat = 0;
  const float *gamma = nullptr, *beta = nullptr;  // nullptr: 1 and 0
  float *dgamma = nullptr, *dbeta = nullptr;      // gradients (optional); synchronised: THIS rank's sums
  float *mean = nullptr, *invstd = nullptr;  // this batch's statistics: written by the forward (optional there), read by the backward
  float *scale = nullptr, *shift = nullptr;  // the folded map y = scale * x + shift, for the kernel that reads the rows next
  float *running_mean = nullptr, *running_var = nullptr;  // optional
  int64_t* batches_tracked = nullptr;  // optional: num_batches_tracked, bumped by the finalising launch
  float eps = 0.f, momentum = 0.f;
};

// The gradient w.r.t. the readout input, recomputed instead of read (GraphGather backward fused into its consumer):
// with g2[m] = [dsum | dmax] of molecule m (tanh derivative already applied) and arg[m,f] = row of the first maximum,
//   dy[r, f] = g2[mol(r)][f] + (arg[mol(r)][f] == r) * g2[mol(r)][F + f].
// Built once per backward; passed BY VALUE to col_sums_kernel and bn_bwd_dx_kernel (bn.hip): the layout is theirs.
struct ReadoutGrad {
  const int32_t* membership;  // N
  const float* g2;            // n_mols x ldg2 (>= 2F)
  int64_t ldg2;
  const int32_t* arg;         // n_mols x F
  // optional: what the column sums need to come from per-molecule data (readout_bn_sums_kernel)
  const float* rawsum = nullptr;  // n_mols x 2F: [row sums | arg-max row's value] of the BatchNorm input
  const int32_t* runs = nullptr;  // n_mols x n_deg x 2 row runs
  int32_t n_mols = 0, n_deg = 0;
};

// The training forward of a point: the column sums of the rows (or the sums a product's epilogue left in acc),
// finalised into mean / invstd / scale / shift and the running statistics.  Three routes, each with the argument checks
// it always had: a pass over the rows; sums_ready (n_rows > 0 either way); sync, where n_rows == 0 is a rank that
// only takes part in the exchange.
struct BnForward {
  const float* x = nullptr;  // rows, n_rows x ldx; not read when sums_ready
  int64_t ldx = 0;
  bool sums_ready = false;   // acc already holds sum x, sum x^2 (seg_gemm_stats, fwd_h_gemm)
  int64_t n_rows = 0;
  double* acc = nullptr;     // GCMI_BN_ACC_DOUBLES(n_feat) doubles
  bool acc_clean = false;    // the caller guarantees zeroed accumulators (the whole-model path zeroes its scratch once
                             // per pass instead of once per call); they are left clean either way
  const BnSync* sync = nullptr;
};
int bn_train_forward(const BnPoint& p, const BnForward& f, void* stream);

// One call's worth of BatchNorm backward over a point: dgamma, dbeta, the coefficient vectors [A | B | C] at the head
// of acc (bn.hip: dx = A dy + B x + C) and, with dx, the input gradient.
struct BnBackward {
  const float* dy = nullptr;  // the incoming gradient rows (bn_bwd_pool_impl: nullptr when the caller never produces
  int64_t lddy = 0;           // them), or
  const ReadoutGrad* rg = nullptr;  // the readout gradient they are recomputed from (then dy is not read)
  const float* x = nullptr;   // the BatchNorm input
  int64_t ldx = 0;
  int32_t x_bf16 = 0;         // bn_bwd_pool_impl only: x (1) or x and dy (2) are bf16 rows, leading dimensions in elements
  int64_t n_rows = 0;
  float* dx = nullptr;        // optional (bn_bwd_impl only)
  int64_t lddx = 0;
  int32_t relu_mask = 0;      // x is a ReLU output and dx is wanted w.r.t. the ReLU input
  double* acc = nullptr;      // as BnForward's
  bool acc_clean = false;
  // bn_bwd_pool_impl: the sums sum dP, sum dP * P over the rows of the block ABOVE (bwd_fused.hip: psums), with
  // P = max over neighbours of the BatchNorm output y = gamma * xhat + beta: sum dy = sum dP and
  // sum dy * xhat = (sum dP * P - beta * sum dP) / gamma, no pass over dy.  Where that division is ill-conditioned
  // (|beta| > 64 |gamma| in some column) the direct column sums are taken instead: the kernels that are only needed
  // for them (column sums; in reference mode also the GraphPool backward) are launched every time and return at once
  // unless that test says so.  Without dy the direct sums are missing too.
  double* psums = nullptr;
  const BnSync* sync = nullptr;
  // bn_bwd_params_impl: also *out = inv_count * sum of the rep accumulator replicas, cleared (loss_finalize_impl
  // folded into the launch that follows the head kernel anyway; synchronised: this rank's own, in the collapse launch)
  struct Loss { double* acc = nullptr; int rep = 0; float inv_count = 0.f; float* out = nullptr; } loss;
};
// sums from a pass over dy (or the readout gradient: from per-molecule data where rg has rawsum and runs), then dx
int bn_bwd_impl(const BnPoint& p, const BnBackward& b, void* stream);
// sums from psums (see there); no dx
int bn_bwd_pool_impl(const BnPoint& p, const BnBackward& b, void* stream);
// the part after the column sums, which are in acc already (head_bwd.hip left them); no dx
int bn_bwd_params_impl(const BnPoint& p, const BnBackward& b, void* stream);
// the backward of a rank without rows: the exchange alone (zero sums, count 0) -- the other ranks wait for it
int bn_bwd_sync_empty(int32_t n_feat, const BnSync& sy, void* stream);

// One block's backward in one pass over its rows (bwd_fused.hip): the host-side counterpart of FusedArgs, leading
// dimensions 64-bit (the launchers narrow them and refuse rows x ld >= 2^30).  G = the gradient w.r.t. the block's
// pre-activation, formed per tile from the gradient source, gc and coef.
struct BlockBackward {
  // row segments; w_off / b_off: per segment into w / dw and into db (a nullptr array or an entry < 0: absent).  The
  // dense layer: one segment of [0, *seg_end) as one_segment makes it for products -- *seg_end must outlive this
  int32_t n_seg = 0;
  const int32_t *seg_begin = nullptr, *seg_end = nullptr;
  const int64_t* w_off[2] = {nullptr, nullptr};  // GraphConv: W_rel[d] against in[0], W_self[d] against in[1]
  const int64_t* b_off = nullptr;
  const float* dy = nullptr;        // the gradient source: rows (GraphConv), or
  int64_t lddy = 0;
  const ReadoutGrad* rg = nullptr;  // the readout gradient (the dense layer behind the GraphGather)
  const float* gc = nullptr;    // the block's ReLU output = its BatchNorm's input
  int64_t ldgc = 0;
  const float* coef = nullptr;  // [A | B | C] of that BatchNorm's backward; nullptr (GraphConv only): G = relu'(gc) * dy
  int32_t width = 0;            // columns of G
  struct In { const float* rows = nullptr; int64_t ld = 0; } in[2];  // GraphConv: S and X; dense: the pooled rows
  int32_t k_in = 0;
  const float* w = nullptr;
  float* dw = nullptr;          // += In^T G (dense: G^T In, nn.Linear layout)
  float* db = nullptr;          // += colsum G per segment
  struct Out { float* rows = nullptr; int64_t ld = 0; } dout[2];  // G W^T: dS, the self part of dX; dense: dP.  nullptr: not wanted
  double* psums = nullptr;      // optional, with dout: sum dP, sum dP * P for the BatchNorm of the block below
  int32_t act_bf16 = 0;         // gc and in are bf16 rows, leading dimensions in elements (2: dy and dout too)
  int32_t in_bf16 = 0;          // without act_bf16: in[] alone are bf16 rows that hold their values exactly -- the
                                // first GraphConv, which needs no input gradient
};

// head_bwd.hip: loss + d logits + task-head gradients + tanh' of the readout + the dense BatchNorm's backward sums in
// one kernel over the molecules (<= 32 outputs), or two on the matrix cores (33..256 outputs)
struct HeadBackward {
  int32_t kind = 0;  // 0 softmax cross-entropy, 1 L2
  const float *logits = nullptr, *labels = nullptr, *weights = nullptr;
  int64_t n_rows = 0;  // molecules that carry a loss
  int32_t n_tasks = 0, n_classes = 0;
  const float* fp = nullptr;  // the fingerprint, rg->n_mols x ldfp
  int64_t ldfp = 0;
  const float* w = nullptr;   // head weights (nn.Linear), and their gradients:
  float *dw = nullptr, *db = nullptr;
  const ReadoutGrad* rg = nullptr;    // n_mols, ldg2, and for the sums runs, n_deg, arg, rawsum
  float* g2 = nullptr;                // written: the rows rg->g2 names
  double* loss_acc = nullptr;         // kLossRep replicas, added into
  const BnPoint* dense_bn = nullptr;  // the dense layer's: its width, and mean / invstd for the sums
  double* sums = nullptr;             // optional: that BatchNorm's backward sums, added into this accumulator
  float* dl_scratch = nullptr;        // more than 32 outputs: n_mols x outputs floats, and
  float* img = nullptr;               // kHeadImgFloats floats, filled with head_prep's images of w first
  int32_t* route = nullptr;           // optional, on the host (gcmi_head_backward): 0 head_bwd_kernel, 1 the wide pair
};

// row slabs of the weight-gradient kernels (gemm.hip, gemm_split.hip): slabs instead of tiles, other offsets
constexpr int kMaxSegW = 16;
struct SlabTable {
  int32_t n_seg;
  int32_t slab_rows;
  int32_t seg_begin[kMaxSegW];
  int32_t seg_end[kMaxSegW];
  int32_t slab_start[kMaxSegW + 1];
  int64_t dw_off[kMaxSegW];
  int64_t db_off[kMaxSegW];
};

// ---- device side of the two tables
// Entry s of a by-value table array, picked with selects (a dynamic index into a kernarg struct would go through
// scratch).  The pointer form looks at the first N entries only.
template <int N, typename T>
__device__ __forceinline__ T pick_n(const T* a, int s) {
  T v = a[0];
#pragma unroll
  for (int k = 1; k < N; ++k) v = (s == k) ? a[k] : v;
  return v;
}
template <typename T, int N>
__device__ __forceinline__ T pick_n(const T (&a)[N], int s) {
  return pick_n<N>(&a[0], s);
}
// The first tile / slab of segment s.  Over the first 16 entries on purpose: s < 16, the 17th entry is the total, and the
// array form of pick_n would add a select per use to every one-tile kernel.
__device__ __forceinline__ int first_tile(const SegTable& st, int s) { return pick_n<kMaxProductSeg>(st.tile_start, s); }
__device__ __forceinline__ int first_slab(const SlabTable& st, int s) { return pick_n<kMaxSegW>(st.slab_start, s); }
// the segment of tile b / of slab b: the number of segment starts (s >= 1) that are <= b
__device__ __forceinline__ int seg_of_tile(const SegTable& st, int b) {
  int s = 0;
#pragma unroll
  for (int k = 1; k < kMaxProductSeg; ++k) s += (k < st.n_seg && b >= st.tile_start[k]) ? 1 : 0;
  return s;
}
__device__ __forceinline__ int seg_of_slab(const SlabTable& st, int b) {
  int s = 0;
#pragma unroll
  for (int q = 1; q < kMaxSegW; ++q) s += (q < st.n_seg && b >= st.slab_start[q]) ? 1 : 0;
  return s;
}

// ---- The tile walk of the persistent kernels (fwd_fused_kernel, fwd_reg_kernel, fwd_hd_kernel, fused_bwd_kernel): a
// workgroup copies the table to LDS once, takes a contiguous range of the tiles and walks it, forwards or (rev)
// backwards, with a cursor.
// The table in LDS, where a dynamic index costs a read: filled by the first kMaxProductSeg + 1 threads, valid after
// the caller's next barrier.
struct SegTableLds {
  int begin[kMaxProductSeg], end[kMaxProductSeg], tile[kMaxProductSeg + 1];
  long long w[2][kMaxProductSeg], b[kMaxProductSeg];
  __device__ __forceinline__ void fill(const SegTable& st) {
    const int tid = threadIdx.x;
    if (tid <= kMaxProductSeg) {
      tile[tid] = pick_n(st.tile_start, tid);
      if (tid < kMaxProductSeg) {
        begin[tid] = pick_n(st.seg_begin, tid);
        end[tid] = pick_n(st.seg_end, tid);
        w[0][tid] = pick_n(st.w_off[0], tid);
        w[1][tid] = pick_n(st.w_off[1], tid);
        b[tid] = pick_n(st.b_off, tid);
      }
    }
  }
};
// Tiles [t_begin, t_end) of this workgroup, an even share of n_tiles (>= 1 tile: the grids are never larger than the
// tile count); at(i) = the i-th tile it visits.  rev: last-written rows first on alternate launches, and the
// workgroups in reverse order too.  UNIFORM says that the bounds are wave-uniform (their 64-bit division runs on the
// vector unit): fwd_reg_kernel and fwd_hd_kernel do, fwd_fused_kernel and fused_bwd_kernel leave them as computed.
struct TileRange {
  int t_begin, t_end, rev;
  __device__ __forceinline__ int count() const { return t_end - t_begin; }
  __device__ __forceinline__ int at(int i) const { return rev ? t_end - 1 - i : t_begin + i; }
};
template <bool UNIFORM>
__device__ __forceinline__ TileRange tile_range(int n_tiles, int rev) {
  const int b = rev ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
  int t_begin = (int)((int64_t)b * n_tiles / gridDim.x);
  int t_end = (int)((int64_t)(b + 1) * n_tiles / gridDim.x);
  if constexpr (UNIFORM) {
    t_begin = __builtin_amdgcn_readfirstlane(t_begin);
    t_end = __builtin_amdgcn_readfirstlane(t_end);
  }
  return {t_begin, t_end, rev};
}
// Tile -> (segment, first row, rows) by a cursor that moves with the walk: a workgroup's tiles are consecutive, so the
// segment changes now and then and a look-up is otherwise two scalar operations.  (The per-tile search it replaces --
// a loop of LDS reads over the segment starts, each landing in a vector register -- measured ~1 200 cycles per
// look-up in fwd_hd_kernel's phase clocks, two look-ups per tile: a third of its tile loop.)  A kernel may keep several
// (fwd_hd_kernel: one for the tiles it requests, one for the tile it multiplies).
struct SegCursor {
  int seg, t0, t1, r0, r1;  // the segment, its tiles [t0, t1) and rows [r0, r1): all wave-uniform
  __device__ __forceinline__ void load(const SegTableLds& tl) {
    t0 = __builtin_amdgcn_readfirstlane(tl.tile[seg]);
    t1 = __builtin_amdgcn_readfirstlane(tl.tile[seg + 1]);
    r0 = __builtin_amdgcn_readfirstlane(tl.begin[seg]);
    r1 = __builtin_amdgcn_readfirstlane(tl.end[seg]);
  }
  // the one search, for the first tile of the walk
  __device__ __forceinline__ void init(const SegTableLds& tl, int n_seg, int tile) {
    int sg = 0;
    for (int k = 1; k < n_seg; ++k) sg += tile >= tl.tile[k] ? 1 : 0;
    seg = __builtin_amdgcn_readfirstlane(sg);
    load(tl);
  }
  // moves to `tile` (either direction); returns its segment, and its first row and row count (<= ROWS) in row0, valid
  template <int ROWS>
  __device__ __forceinline__ int seek(const SegTableLds& tl, int tile, int& row0, int& valid) {
    while (tile >= t1) { ++seg; load(tl); }  // (uniform; empty segments are stepped over)
    while (tile < t0) { --seg; load(tl); }
    row0 = r0 + (tile - t0) * ROWS;
    const int left = r1 - row0;
    valid = left < ROWS ? left : ROWS;
    return seg;
  }
};

// ---- bf16 activation storage (gcmi_model_desc.storage == 1): raw 16-bit patterns, leading dimensions in elements
bool win_usable_h(const gcmi_graph* g, int n_feat);
int win_gather_sum_fh(const gcmi_graph* g, const float* d_x, int64_t ldx, int n_feat, unsigned short* d_s,
                      unsigned short* d_xcopy, int64_t ldo, hipStream_t st);
int win_gather_sum_h(const gcmi_graph* g, const unsigned short* d_x, int64_t ldx, int n_feat, unsigned short* d_s,
                     int64_t lds, hipStream_t st, bool accumulate = false);
int win_gather_max_h(const gcmi_graph* g, const unsigned short* d_x, int64_t ldx, int n_feat, const float* d_scale,
                     const float* d_shift, unsigned short* d_out, int64_t ldo, uint8_t* d_arg, hipStream_t st);
// gradient streams in bf16 (storage == 2)
bool win_usable_gh(const gcmi_graph* g, int n_feat);
int win_gather_max_bwd_h(const gcmi_graph* g, const unsigned short* d_dout, int64_t lddo, int n_feat, const uint8_t* d_arg,
                         unsigned short* d_dx, int64_t lddx, const float* only_if_gamma, const float* only_if_beta,
                         hipStream_t st);
bool win_two_stage_usable_h(const gcmi_graph* g, int n_feat);
// ... at every bf16 width with a kernel (64 / 80 / 128), for the operation-level entry points
bool win_usable_bwd_h(const gcmi_graph* g, int n_feat);
bool win_two_stage_usable_bwd_h(const gcmi_graph* g, int n_feat);
int win_gather_sumacc_max_bwd_h(const gcmi_graph* g, const unsigned short* d_ds, int64_t ldds, int n_feat,
                                unsigned short* d_dxs, int64_t lddxs, const uint8_t* d_arg, unsigned short* d_dy,
                                int64_t lddy, hipStream_t st);
// fwd_bf16.hip: forward product over bf16 operands (shapes: fwd_shape above), BatchNorm sums of the rounded output.
// TO = unsigned short: bf16 output rows; TO = float: fp32 output rows and sums of the unrounded values -- the
// two-operand 65..80-column shape only
template <typename TO>
int fwd_h_gemm(const SegProduct<unsigned short, TO>& p, double* d_stats, float* d_wimg_scratch, hipStream_t sm);
int fwd_weight_images(int32_t n_seg, const int64_t* w1_off, const int64_t* w2_off, const float* d_w1, const float* d_w2,
                      int32_t k_in, int32_t ko, int32_t n_ops, int32_t n_out, int32_t trans_w, float* d_scratch,
                      hipStream_t sm);
constexpr int64_t kFwdHWimgFloats = 16 * 20 * 3 * 256;  // scratch of fwd_h_gemm: split weight fragments of <= 16 segments

bool gemm_exact_mode();  // gcmi_set_option(GCMI_OPT_GEMM_EXACT)

int launch_wgrad3(const SlabTable& st, int slabs, const float* d_a, int64_t lda, int k, const float* d_g, int64_t ldg,
                  int n, float* d_dw, float* d_dbias, int trans_w, hipStream_t sm);

// gemm_split.hip: the segmented GEMM on the bf16 matrix cores with exactly split fp32 operands;
// GCMI_ERR_UNSUPPORTED = shape not covered (fall back to gemm.hip)
int launch_seg_gemm4(const SegProduct<float>& p, hipStream_t sm, double* d_stats = nullptr);

// bwd_fused.hip: BatchNorm-backward + weight gradients + input gradients of one block in one pass over the rows;
// GCMI_ERR_UNSUPPORTED = switched off / exact mode / shape not covered (the caller runs the separate kernels)
void set_readout_pipelined(int on);
int get_readout_pipelined();
void set_fused_bwd(int on);
int get_fused_bwd();
bool fused_bwd_enabled();
int fused_bwd_launches();  // launches of the one-pass kernel so far (tests)
int one_piece_launches();  // model.hip: launches of the first block's one-piece forward product and backward so far
// (GraphConv block: dW_rel += S^T G, dW_self += X^T G, dbsum += colsum G, and with dout dS = G W_rel^T, dXs = G W_self^T;
// dense layer behind the GraphGather: dW += G^T P, db += colsum G, dP = G W)
int fused_conv_bwd(const BlockBackward& b, hipStream_t sm);
int fused_dense_bwd(const BlockBackward& b, hipStream_t sm);

// fwd_fused.hip: the forward product of a block as persistent workgroups with resident weight images (split-bf16 mode,
// shapes: fwd_shape above); GCMI_ERR_UNSUPPORTED = shape not covered
int fwd_fused_gemm(const SegProduct<float>& p, double* d_stats, hipStream_t sm, float* d_wimg_scratch = nullptr);

// head_bwd.hip (HeadBackward above); GCMI_ERR_UNSUPPORTED = shape not covered (256-column fingerprint)
int head_bwd_fused(const HeadBackward& h, hipStream_t st);
// ... and the forward head with 33..256 outputs (one segment, 256-column rows, nn.Linear weight, no activation); d_img:
// the fragment images head_prep made of d_w (kHeadImgFloats floats: forward order, then backward order), or nullptr
constexpr int kHeadImgFloats = 2 * 8 * 16 * 3 * 64 * 4;
int head_prep(const float* d_w, int32_t n_out, float* d_img, hipStream_t st);
int head_fwd_wide(const float* d_in, int64_t ldin, int64_t n_rows, int32_t k, const float* d_w, const float* d_bias,
                  int32_t n_out, int32_t act, float* d_out, int64_t ldo, hipStream_t st, const float* d_img = nullptr);
// replicas of the loss accumulator (doubles) that head_bwd_fused adds into; loss_finalize_impl sums and clears them
constexpr int kLossRep = 16;
int loss_finalize_impl(double* d_acc, float inv_count, float* d_loss, void* stream, int n_rep = 1);

// accumulator replicas of the BatchNorm column sums (same-address fp64 atomics serialise); scratch layout in
// doubles: [0, 2F) backward coefficient vectors, then kBnReplicas blocks of [sum(F) | sum of squares(F)]
constexpr int kBnReplicas = 32;
// gcmi_seg_gemm on a description (gemm.hip): the same argument checks, the same kernels
int seg_gemm(const SegProduct<float>& p, hipStream_t sm);
// ... with the column sums of the output (after bias and activation) added into d_stats in that layout
// by the product's own epilogue; *fused = false (and nothing added) when the kernel in charge cannot do it
int seg_gemm_stats(const SegProduct<float>& p, double* d_stats, bool* fused, hipStream_t sm,
                   float* d_wimg_scratch = nullptr);
// gcmi_readout_fwd that also leaves the per-molecule sums of the rows before the folded BatchNorm in d_rawsum
int readout_fwd_impl(const gcmi_graph* g, const float* d_x, int64_t ldx, int32_t n_feat, const float* d_scale,
                     const float* d_shift, int32_t act, float* d_out, int64_t ldo, int32_t* d_arg, float* d_rawsum,
                     void* stream, int32_t x_bf16 = 0);
int readout_grad_prep(float* d_g, int64_t ldg, const float* d_out, int64_t ldo, int64_t n_mols, int n_feat,
                      hipStream_t st);
// (acc_clean: as BnForward's)
int loss_impl(int32_t kind, const float* d_logits, const float* d_labels, const float* d_weights,
              int64_t n_rows, int32_t n_tasks, int32_t n_classes, float* d_loss, float* d_dlogits,
              float* d_probs, double* d_acc, bool acc_clean, void* stream);

// degree of batch row i: the number of block starts (d >= 1) that are <= i.
__device__ __forceinline__ int degree_of_row(const DegTable& t, int i) {
  int d = 0;
#pragma unroll
  for (int k = 1; k <= GCMI_MAX_DEG; ++k) d += (k <= t.max_deg && i >= t.deg_start[k]) ? 1 : 0;
  return d;
}

// wave-uniform: some column has |beta| > 64 |gamma| (or a NaN): (y - beta) / gamma does not recover xhat well there
__device__ __forceinline__ bool bn_pool_ill_conditioned(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int n_feat) {
  bool bad = false;
  for (int c = threadIdx.x & 63; c < n_feat; c += 64) {
    const float gm = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
    bad = bad || !(fabsf(bt) <= 64.f * fabsf(gm));
  }
  return __ballot(bad) != 0ull;
}

// vector width usable for a row-major matrix access
inline int vec_width(const void* p, int64_t ld, int n_feat) {
  return (aligned16(p) && (ld % 4 == 0) && (n_feat % 4 == 0)) ? 4 : 1;
}

constexpr int kMaxBlocks = 256 * 8 * 4;  // grid cap for grid-stride kernels: 256 CUs x 8 x 4

inline int grid_for(int64_t work_items, int block) {
  int64_t b = (work_items + block - 1) / block;
  if (b < 1) b = 1;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return static_cast<int>(b);
}

template <int V>
struct Vec;
template <>
struct Vec<1> {
  using T = float;
};
template <>
struct Vec<4> {
  using T = float4;
};

__device__ __forceinline__ float vzero(float) { return 0.f; }
__device__ __forceinline__ float4 vzero(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float4 vadd(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

}  // namespace gcmi
