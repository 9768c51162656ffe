// Whole-model sequencing: _GraphConvTorchModel.forward
// (models/torch_models/graphconvmodel.py:188-249) and the loss + backward of one
// fit_generator step (models/torch_models/torch_model.py:436-442) as one C call each.
// Host code only enqueues the kernels of this library on the caller's stream; the few
// device functions here are parameter-layout helpers (bias packing, counters).
#include <map>
#include <mutex>

#include "common.h"
#include "split_bf16.h"

namespace gcmi {

constexpr int kMaxL = GCMI_MAX_CONV_LAYERS;

struct BiasLayers {  // the GraphConv layers' bias blocks: one launch packs (or unpacks) all of them (blockIdx.y = layer)
  const float* src[kMaxL];
  float* dst[kMaxL];
  int width[kMaxL];
};

__global__ void bias_pack_kernel(BiasLayers bl, int max_deg) {
  // b_list: (2*max_deg+1, width) in reference order; bsum[d] = b_rel_d + b_self_d, bsum[0] = b_self_0
  const int l = blockIdx.y;
  const float* __restrict__ b_list = pick_n(bl.src, l);
  float* __restrict__ bsum = pick_n(bl.dst, l);
  const int width = pick_n(bl.width, l);
  if (b_list == nullptr) return;
  const int n = (max_deg + 1) * width;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int d = i / width, c = i - d * width;
    bsum[i] = d == 0 ? b_list[(2 * max_deg) * width + c]
                     : b_list[(2 * (d - 1)) * width + c] + b_list[(2 * (d - 1) + 1) * width + c];
  }
}

__global__ void bias_unpack_kernel(BiasLayers bl, int max_deg) {
  const int l = blockIdx.y;
  const float* __restrict__ dbsum = pick_n(bl.src, l);
  float* __restrict__ db_list = pick_n(bl.dst, l);
  const int width = pick_n(bl.width, l);
  if (dbsum == nullptr) return;
  const int n = (2 * max_deg + 1) * width;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int k = i / width, c = i - k * width;
    const int d = k == 2 * max_deg ? 0 : k / 2 + 1;
    db_list[i] = dbsum[d * width + c];
  }
}

// elements of an n_rows x n_cols matrix that are NOT integers of magnitude <= limit (NaN and infinities count)
__global__ void small_int_count_kernel(const float* __restrict__ x, int64_t ld, int64_t n_rows, int n_cols, float limit,
                                       unsigned long long* __restrict__ count) {
  const int64_t total = n_rows * n_cols;
  unsigned bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / n_cols;
    const float v = x[r * ld + (i - r * n_cols)];
    bad += (fabsf(v) <= limit && v == truncf(v)) ? 0u : 1u;
  }
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(count, (unsigned long long)bad);
}

struct CounterPtrs {
  int64_t* p[kMaxL + 1];
  int n;
};
__global__ void bump_counters_kernel(CounterPtrs c) {
  const int i = threadIdx.x;
  if (i < c.n && c.p[i] != nullptr) *c.p[i] += 1;
}

// Workspace carve-up (floats).  Everything the backward needs from the forward, plus the
// backward's temporaries.  All blocks start 16-byte aligned.
struct Ws {
  int64_t S[kMaxL], gc[kMaxL], pool[kMaxL], arg[kMaxL], bsum[kMaxL], bnv[kMaxL + 1];
  int64_t ldS[kMaxL], ngather[kMaxL];
  int64_t dense, arg_r, rsum, dfp, tA, tB, tC, tD, tE, total;
  int64_t xb;    // bf16 copy of the atom features: storage == 1 (ld = ldS[0]); storage == 0 over 73..76 features
                 // (ld = kOnePieceLd), used by the first block's one-piece form
  int64_t wimg;  // scratch of the forward products (split weight fragments in lane order, rebuilt by every launch)
  int64_t himg;  // more than 32 task outputs: the head matrix's two fragment images (head_bwd.hip: head_prep; the
                 // forward and the backward each make them of the weights they are given)
  // one region the backward zeroes with a single memset: [dlogits | dbsum per layer | lacc | acc]
  int64_t dlogits, dbsum[kMaxL], lacc, acc, acc2, z_end;
  int64_t xch;   // synchronised BatchNorm: the exchange buffer of one BatchNorm point, 2 wmax + 1 doubles (bn.hip)
};

constexpr int64_t kOnePieceLd = 80;  // elements of a bf16 row of S0 / Xb in the first block's one-piece form

static Ws carve(const gcmi_model_desc* m, int64_t N, int64_t B, int64_t ld_features) {
  Ws w;
  memset(&w, 0, sizeof(w));
  int64_t off = 0;
  auto take = [&](int64_t n) {
    int64_t o = off;
    off += up4(n);
    return o;
  };
  // storage == 1: the matrices the step writes and reads back (S, gc, pool, dense, and a copy of the atom features)
  // are bf16: rows of ld ELEMENTS with ld a multiple of 8, half the floats of the workspace per element
  const bool h = m->storage >= 1;
  auto take_act = [&](int64_t rows, int64_t ld) { return take(h ? (rows * ld + 1) / 2 : rows * ld); };
  const int L = m->n_layers;
  int64_t wmax = m->dense_width, kmax = up4(m->n_feat_in);
  for (int l = 0; l < L; ++l) {
    const int64_t k = l == 0 ? m->n_feat_in : m->conv_width[l - 1];
    const int64_t ldx = l == 0 ? ld_features : m->conv_width[l - 1];
    // gather over the padded width when the rows are 16-byte addressable (pad columns are 0)
    w.ngather[l] = (l == 0 && ldx % 4 == 0 && ldx < k + 4) ? ldx : k;
    if (h && l == 0) w.ngather[l] = up4(k);
    w.ldS[l] = h ? up8(w.ngather[l]) : up4(w.ngather[l]);
    const int64_t wd = m->conv_width[l];
    w.S[l] = take_act(N, w.ldS[l]);
    if (h && l == 0) w.xb = take_act(N, w.ldS[0]);
    // (fp32 storage: S[0]'s own block, N x 76 floats, is large enough for the bf16 sums of the one-piece form)
    if (!h && l == 0 && up4(m->n_feat_in) == 76) w.xb = take((N * kOnePieceLd + 1) / 2);
    if (l == 0) w.wimg = take(kFwdHWimgFloats);
    w.gc[l] = take_act(N, wd);
    w.pool[l] = take_act(N, wd);
    w.arg[l] = take((N * wd + 3) / 4);
    w.bsum[l] = take((int64_t)(m->max_deg + 1) * wd);
    w.bnv[l] = take(4 * wd);
    if (wd > wmax) wmax = wd;
    if (w.ldS[l] > kmax) kmax = w.ldS[l];
  }
  const int64_t D = m->dense_width;
  const int64_t TC = (int64_t)m->n_tasks * m->n_classes;
  w.bnv[L] = take(4 * D);
  w.himg = (TC <= 256 && 2 * D == 256) ? take(kHeadImgFloats) : -1;  // (786 KB; used from head_wide_min() outputs on)
  w.dense = take_act(N, D);
  w.arg_r = take(B * D);
  w.rsum = take(2 * B * D);  // per-molecule [row sums | arg-max row value] of the dense output (BatchNorm backward)
  w.dfp = take(B * 2 * D);
  w.tA = take(N * wmax);
  w.tB = take(N * wmax);
  w.tC = take(N * wmax);
  w.tD = take(N * wmax);
  w.tE = take(N * kmax);
  w.dlogits = take(B * TC);
  for (int l = 0; l < L; ++l) w.dbsum[l] = take((int64_t)(m->max_deg + 1) * m->conv_width[l]);
  w.lacc = take(2 * kLossRep);
  w.acc = take(2 * GCMI_BN_ACC_DOUBLES(wmax));
  w.acc2 = take(2 * GCMI_BN_ACC_DOUBLES(wmax));  // pooled BatchNorm-backward sums of the block below (bwd_fused.hip)
  w.z_end = off;
  w.xch = take(2 * (2 * wmax + 2));
  w.total = off;
  return w;
}

// b_rel_d + b_self_d of every GraphConv layer (the products add ONE bias row per degree): one launch for all layers
static int pack_biases(const gcmi_model_desc* m, const Ws& w, float* ws, const float* d_params, hipStream_t st) {
  BiasLayers bl;
  memset(&bl, 0, sizeof(bl));
  for (int l = 0; l < m->n_layers; ++l) {
    bl.src[l] = d_params + m->off_conv_b[l];
    bl.dst[l] = ws + w.bsum[l];
    bl.width[l] = m->conv_width[l];
  }
  hipLaunchKernelGGL(bias_pack_kernel, dim3(4, m->n_layers), dim3(256), 0, st, bl, m->max_deg);
  GCMI_CHECK_LAUNCH("bias_pack");
  return GCMI_OK;
}

// ... and the per-degree bias gradients back into the reference's (2 max_deg + 1) rows, for the layers whose block ran
static int unpack_bias_grads(const gcmi_model_desc* m, const BiasLayers& bl, int n_layers, hipStream_t st) {
  bool any = false;
  for (int l = 0; l < n_layers; ++l) any = any || bl.src[l] != nullptr;
  if (!any) return GCMI_OK;
  hipLaunchKernelGGL(bias_unpack_kernel, dim3(4, n_layers), dim3(256), 0, st, bl, m->max_deg);
  GCMI_CHECK_LAUNCH("bias_unpack");
  return GCMI_OK;
}

// The task head's forward product: with more than 32 outputs on the prepared images (head_bwd.hip; the backward makes
// its own of the weights it is given); otherwise (and in the exact product mode) the segmented product.
static int head_forward(const gcmi_model_desc* m, const Ws& w, float* ws, const float* d_params, const gcmi_model_io* io,
                        int64_t B, void* stream) {
  const int D = m->dense_width;
  const int TC = m->n_tasks * m->n_classes;
  const int32_t nB = (int32_t)B;
  hipStream_t st = (hipStream_t)stream;
  if (w.himg >= 0 && B > 0) {
    int rc = head_prep(d_params + m->off_head_w, TC, ws + w.himg, st);
    if (rc == GCMI_OK)
      rc = head_fwd_wide(io->d_fingerprint, 2 * D, B, 2 * D, d_params + m->off_head_w, d_params + m->off_head_b, TC, 0,
                         io->d_logits, TC, st, ws + w.himg);
    if (rc != GCMI_ERR_UNSUPPORTED) return rc;
  }
  SegProduct<float> p = one_segment(&nB, io->d_fingerprint, 2 * D, 2 * D, d_params + m->off_head_w,
                                    d_params + m->off_head_b, TC, io->d_logits, TC);
  p.trans_w = 1;
  return seg_gemm(p, st);
}

static int check_desc(const gcmi_model_desc* m) {
  GCMI_CHECK_ARG(m != nullptr, "model desc is NULL");
  GCMI_CHECK_ARG(m->n_layers >= 1 && m->n_layers <= kMaxL, "n_layers %d outside [1,%d]", m->n_layers, kMaxL);
  GCMI_CHECK_ARG(m->max_deg >= 0 && m->max_deg <= GCMI_MAX_DEG, "bad max_deg");
  GCMI_CHECK_ARG(m->n_feat_in > 0 && m->dense_width > 0 && m->n_tasks > 0 && m->n_classes > 0, "bad widths");
  GCMI_CHECK_ARG(m->mode == 0 || m->mode == 1, "mode must be 0 (classification) or 1 (regression)");
  GCMI_CHECK_ARG(m->mode == 0 || m->n_classes == 1, "regression needs n_classes == 1");
  for (int l = 0; l < m->n_layers; ++l) GCMI_CHECK_ARG(m->conv_width[l] > 0, "bad conv width");
  if (m->storage != 0) {
    // bf16 activation storage in the streaming kernels (fwd_bf16.hip, bwd_fused.hip HB, gather_lds.hip *OpH): the
    // default shapes -- GraphConv widths 64 over 73..76 input columns (the fp32 -> bf16 window gather of the atom
    // features has the 76-column instantiation only), dense width 128, BatchNorm on
    // (2 = the gradient streams between the kernels are bf16 as well)
    bool ok = (m->storage == 1 || m->storage == 2) && m->batch_norm && m->dense_width == 128 && up4(m->n_feat_in) == 76;
    for (int l = 0; l < m->n_layers; ++l) ok = ok && m->conv_width[l] == 64;
    if (!ok) {
      set_error("gcmi_model_*: bf16 activation storage covers graph_conv_layers of width 64 over 73..76 atom features, "
                "dense_layer_size 128 and batch_normalize=True (other shapes: gcmi_small_* or storage 0)");
      return GCMI_ERR_UNSUPPORTED;
    }
  }
  return GCMI_OK;
}

struct Segs {
  int32_t begin[GCMI_MAX_DEG + 1], end[GCMI_MAX_DEG + 1];
  int64_t w_rel[GCMI_MAX_DEG + 1], w_self[GCMI_MAX_DEG + 1], b_off[GCMI_MAX_DEG + 1];
  int n;
};

static Segs make_segs(const gcmi_graph* g, int64_t k, int64_t width) {
  Segs s;
  s.n = g->max_deg + 1;
  const int64_t blk = k * width;
  for (int d = 0; d <= g->max_deg; ++d) {
    s.begin[d] = g->deg_start[d];
    s.end[d] = g->deg_start[d + 1];
    s.w_rel[d] = d == 0 ? -1 : (int64_t)(2 * (d - 1)) * blk;
    s.w_self[d] = d == 0 ? (int64_t)(2 * g->max_deg) * blk : (int64_t)(2 * (d - 1) + 1) * blk;
    s.b_off[d] = (int64_t)d * width;
  }
  return s;
}

// ------------------------------------------------------------------------------------------------------------------
// storage == 0, the first GraphConv block over SMALL-INTEGER atom features (gcmi_model_io.features_small_int: every
// element an integer with |x| <= 256 / max_deg).  Such an element is exactly one bf16 value, and so is every neighbour
// sum (at most max_deg terms: an integer below 256).  The window pass then writes S0 and a copy Xb of the rows as bf16
// (gather_lds.hip SumOpFH), the forward product reads them as they are (fwd_bf16.hip, fp32 output rows: 3 MFMAs per
// k-step instead of 6 and no operand split) and the backward takes In = [S0 | Xb] in one piece against G in three
// (bwd_fused.hip IB).  Every term the split-fp32 kernels compute is still computed: the two operand pieces that are
// dropped are zero.  Conditions = what the bf16 kernels need (require_h below): fast product mode, BatchNorm on, the
// default widths, window plans, reverse slots, the one-pass backward enabled.  Anything else runs the fp32 sequence.
static bool one_piece_block0(const gcmi_model_desc* m, const gcmi_graph* g, const gcmi_model_io* io) {
  if (!io->features_small_int || m->storage != 0 || !m->batch_norm || g->n_atoms <= 0) return false;
  if (gemm_exact_mode() || !fused_bwd_enabled()) return false;
  if (m->conv_width[0] != 64 || up4(m->n_feat_in) != 76 || m->max_deg < 1 || m->max_deg > 10) return false;
  if (io->ld_features % 4 != 0 || io->ld_features < 76 || !aligned16(io->d_atom_features) || !aligned16(io->d_workspace))
    return false;
  if (!win_usable(g, 76, false) || !win_has_width(76)) return false;
  return g->d_rev_pos != nullptr || g->n_edges == 0;
}
// What the last training forward on a workspace decided: the backward reads S0 / Xb in the form they were written,
// whatever the options say by then.
static std::mutex g_one_piece_mu;
static std::map<const void*, bool> g_one_piece_ws;
static void note_one_piece(const void* ws, bool on) {
  std::lock_guard<std::mutex> lk(g_one_piece_mu);
  if (on) g_one_piece_ws[ws] = true;
  else g_one_piece_ws.erase(ws);
}
static bool noted_one_piece(const void* ws) {
  std::lock_guard<std::mutex> lk(g_one_piece_mu);
  return g_one_piece_ws.count(ws) != 0;
}
static std::atomic<int> g_one_piece_launches{0};
int one_piece_launches() { return g_one_piece_launches.load(std::memory_order_relaxed); }

#define RUN(call)            \
  do {                       \
    int rc__ = (call);       \
    if (rc__) return rc__;   \
  } while (0)

// Block l of the step (l < n_layers: GraphConv + BatchNorm + GraphPool; l == n_layers: the atom-level dense layer and
// its BatchNorm): its widths and where its parameters, their gradients and its BatchNorm vectors live.
struct Block {
  int K, W;                       // input / output columns
  const float *w, *bias;          // bias: the rows the product adds (GraphConv: the per-degree sums pack_biases left)
  float *dw, *dbias;              // gradients; nullptr in the forward.  dbias of a GraphConv: per-degree sums in the
  float* dbias_rows;              // workspace, unpacked into the reference's bias rows (dbias_rows) after the loop
  BnPoint bn;                     // its BatchNorm, W wide: gamma, beta and their gradients nullptr without BatchNorm;
};                                // this batch's statistics and the folded affine map in the workspace

static void make_blocks(const gcmi_model_desc* m, const Ws& w, float* ws, const float* d_params, float* d_grads,
                        const gcmi_model_io* io, Block* blk) {
  const int L = m->n_layers;
  auto grad = [&](int64_t off) { return d_grads ? d_grads + off : nullptr; };
  for (int l = 0; l <= L; ++l) {
    Block& b = blk[l];
    b.K = l == 0 ? m->n_feat_in : m->conv_width[l - 1];
    b.W = l == L ? m->dense_width : m->conv_width[l];
    b.w = d_params + (l == L ? m->off_dense_w : m->off_conv_w[l]);
    b.bias = l == L ? d_params + m->off_dense_b : ws + w.bsum[l];
    b.dw = grad(l == L ? m->off_dense_w : m->off_conv_w[l]);
    b.dbias = l == L ? grad(m->off_dense_b) : ws + w.dbsum[l];
    b.dbias_rows = l == L ? nullptr : grad(m->off_conv_b[l]);
    BnPoint& p = b.bn;
    p = BnPoint();
    p.n_feat = b.W;
    if (m->batch_norm) {
      p.gamma = d_params + m->off_bn_gamma[l]; p.beta = d_params + m->off_bn_beta[l];
      p.dgamma = grad(m->off_bn_gamma[l]); p.dbeta = grad(m->off_bn_beta[l]);
    }
    float* bnv = ws + w.bnv[l];
    p.mean = bnv; p.invstd = bnv + b.W; p.scale = bnv + 2 * b.W; p.shift = bnv + 3 * b.W;
    p.running_mean = io->d_bn_running_mean[l]; p.running_var = io->d_bn_running_var[l];
    p.batches_tracked = io->d_bn_batches_tracked[l];
    p.eps = m->bn_eps; p.momentum = m->bn_momentum;
  }
}

// A product over the degree segments with the first operand's weight blocks at w_off (sg.w_rel / sg.w_self)
template <typename TA, typename TO>
static SegProduct<TA, TO> seg_product(const Segs& sg, const TA* a, int64_t lda, int32_t k, const float* w,
                                      const int64_t* w_off, int32_t n_out, TO* out) {
  SegProduct<TA, TO> p;
  p.n_seg = sg.n;
  p.seg_begin = sg.begin;
  p.seg_end = sg.end;
  p.op[0] = {a, lda, k, w, w_off};
  p.n_out = n_out;
  p.out = out;
  p.ldo = n_out;
  return p;
}

// The product of GraphConv block b: relu([S | X] . [W_rel[d]; W_self[d]] + bsum[d])
template <typename TA, typename TO>
static SegProduct<TA, TO> conv_product(const Segs& sg, const TA* s, int64_t lds, const TA* x, int64_t ldx, const Block& b,
                                       TO* out) {
  SegProduct<TA, TO> p = seg_product(sg, s, lds, b.K, b.w, sg.w_rel, b.W, out);
  p.op[1] = {x, ldx, b.K, b.w, sg.w_self};
  p.bias = b.bias;
  p.bias_off = sg.b_off;
  p.act = 1;
  return p;
}

// BatchNorm of block b in the forward, folded into b.bn.scale / shift for the kernel that reads the rows next: training
// = this batch's statistics, from the sums the product left in acc (stats_fused) or from a pass over the rows; eval =
// the running statistics
// (sy: synchronised BatchNorm, training only -- the statistics of the global batch, also for a rank with N == 0)
static int bn_forward(const Block& b, int64_t N, int32_t training, bool stats_fused, const float* rows, int64_t ld,
                      double* acc, void* stream, const BnSync* sy = nullptr) {
  const BnPoint& p = b.bn;
  if (!training)
    return gcmi_bn_fold_eval(p.gamma, p.beta, p.running_mean, p.running_var, p.eps, p.n_feat, p.scale, p.shift, stream);
  BnForward f;
  f.x = rows; f.ldx = ld; f.sums_ready = stats_fused; f.n_rows = N; f.acc = acc; f.sync = sy;
  f.acc_clean = true;  // zeroed once per pass by the caller
  return bn_train_forward(p, f, stream);
}

// A training batch without atoms launches no statistics kernel, and those are what bump the counters otherwise
static int bump_counters(const gcmi_model_desc* m, const gcmi_model_io* io, hipStream_t st) {
  CounterPtrs c;
  c.n = m->n_layers + 1;
  bool any = false;
  for (int i = 0; i <= kMaxL; ++i) {
    c.p[i] = i <= m->n_layers ? io->d_bn_batches_tracked[i] : nullptr;
    any = any || c.p[i] != nullptr;
  }
  if (any) {
    hipLaunchKernelGGL(bump_counters_kernel, dim3(1), dim3(64), 0, st, c);
    GCMI_CHECK_LAUNCH("bump_counters");
  }
  return GCMI_OK;
}

// Synchronised BatchNorm: the caller's exchange callback and the exchange buffer in the workspace
static BnSync make_sync(gcmi_stat_sync_fn sync, void* sync_ctx, const Ws& w, float* ws) {
  return BnSync{sync, sync_ctx, reinterpret_cast<double*>(ws + w.xch)};
}

// ... and the backward of a rank whose batch has no atoms: no BatchNorm kernel runs, but the other ranks wait in the
// exchange of every BatchNorm point their backward computes (the dense block's, then the GraphConv blocks' last to
// first; reference gradient mode stops behind the last GraphConv block)
static int empty_backward_syncs(const gcmi_model_desc* m, const Block* blk, const BnSync& sy, void* stream) {
  for (int l = m->n_layers; l >= 0; --l) {
    RUN(bn_bwd_sync_empty(blk[l].W, sy, stream));
    if (m->grad_mode != 1 && l < m->n_layers) break;
  }
  return GCMI_OK;
}

// Synchronised BatchNorm: what makes a one-pass block kernel refuse its buffers after dispatch is known before the
// first launch -- a workspace that is not 16-byte aligned (every block of it then is not), or rows x leading dimension
// beyond the kernels' 32-bit element offsets.  Refused at the entry of both calls, before this rank makes any exchange
// of the step.
static int check_sync_buffers(const gcmi_model_desc* m, const gcmi_graph* g, const gcmi_model_io* io) {
  if (!aligned16(io->d_workspace)) {
    set_error("synchronised BatchNorm: the workspace must be 16-byte aligned");
    return GCMI_ERR_UNSUPPORTED;
  }
  const int64_t ldmax = std::max<int64_t>(2 * (int64_t)m->dense_width, std::max<int64_t>(io->ld_features, kOnePieceLd));
  if (fused_bwd_enabled() && (int64_t)g->n_atoms * ldmax >= (int64_t)1 << 30) {
    set_error("synchronised BatchNorm: %lld atoms per rank are beyond the one-pass block kernels (rows x row length "
              "below 2^30); use smaller shards", (long long)g->n_atoms);
    return GCMI_ERR_UNSUPPORTED;
  }
  return GCMI_OK;
}

// The backstop of check_sync_buffers (a kernel that cannot get its LDS).  One more pass of a BatchNorm backward's sums
// (a one-pass block kernel refused its buffers after all) would be one
// more exchange than the other ranks make
static int refuse_second_sync(const char* what) {
  set_error("synchronised BatchNorm: %s refused its buffers, and the separate pass would exchange this BatchNorm's sums "
            "twice (16-byte aligned workspace and feature rows needed)", what);
  return GCMI_ERR_UNSUPPORTED;
}

// The first block's forward in its one-piece form (one_piece_block0 above): the window pass writes S0 and Xb as bf16
// rows, the product reads them as they are and leaves fp32 rows (and, training, the BatchNorm sums in acc)
static int one_piece_forward(const gcmi_graph* g, const Ws& w, float* ws, const Block& b, const Segs& sg,
                             const gcmi_model_io* io, double* stats, hipStream_t st) {
  bf16_t* s0 = reinterpret_cast<bf16_t*>(ws + w.S[0]);
  bf16_t* xb = reinterpret_cast<bf16_t*>(ws + w.xb);
  {
    TimedScope ts(GCMI_K_GATHER_SUM, st);
    RUN(win_gather_sum_fh(g, io->d_atom_features, io->ld_features, 76, s0, xb, kOnePieceLd, st));
  }
  {
    TimedScope ts(GCMI_K_SEG_GEMM, st);
    const int rc = fwd_h_gemm(conv_product(sg, s0, kOnePieceLd, xb, kOnePieceLd, b, ws + w.gc[0]), stats, ws + w.wimg, st);
    if (rc == GCMI_ERR_UNSUPPORTED) set_error("model_forward: the one-piece product of GraphConv 0 refused its shape");
    RUN(rc);
  }
  g_one_piece_launches.fetch_add(1, std::memory_order_relaxed);
  return GCMI_OK;
}

// The per-molecule part of the backward as separate launches (what head_bwd_fused does in one, for the shapes it does
// not cover): loss and d logits of the first n_rows molecules, the head's gradients, the gradient w.r.t. the
// fingerprint in dfp; prep: the tanh derivative applied to it in place, for a BatchNorm backward that recomputes the
// GraphGather backward from it
static int head_backward_separate(const gcmi_model_desc* m, const Ws& w, float* ws, const float* d_params, float* d_grads,
                                  const gcmi_model_io* io, const float* d_labels, const float* d_weights, int64_t n_rows,
                                  int64_t B, bool prep, void* stream) {
  const int D = m->dense_width;
  const int TC = m->n_tasks * m->n_classes;
  const int32_t nB = (int32_t)B;
  RUN(loss_impl(m->mode == 0 ? 0 : 1, io->d_logits, d_labels, d_weights, n_rows, m->n_tasks, m->n_classes, io->d_loss,
                ws + w.dlogits, nullptr, reinterpret_cast<double*>(ws + w.lacc), true, stream));
  RUN(gcmi_seg_gemm_wgrad(1, &kZero32, &nB, io->d_fingerprint, 2 * D, 2 * D, ws + w.dlogits, TC, TC,
                          d_grads + m->off_head_w, &kZero64, d_grads + m->off_head_b, &kZero64, 1, stream));
  hipStream_t st = (hipStream_t)stream;
  RUN(seg_gemm(one_segment(&nB, ws + w.dlogits, TC, TC, d_params + m->off_head_w, nullptr, 2 * D, ws + w.dfp, 2 * D), st));
  if (prep) RUN(readout_grad_prep(ws + w.dfp, 2 * D, io->d_fingerprint, 2 * D, B, D, st));
  return GCMI_OK;
}

// the dense block's backward takes the one-pass kernel (bwd_fused.hip: fused_dense_bwd) -- asked once per call: the
// head kernel in front of it leaves the BatchNorm sums only for that kernel
static bool dense_block_one_pass(const gcmi_model_desc* m, int64_t N) {
  const int Wl = m->conv_width[m->n_layers - 1];
  return m->batch_norm && N > 0 && fused_bwd_enabled() && m->dense_width == 128 && Wl > 32 && Wl <= 64;
}

// ---- What both backward sequences hand the backward entries (common.h)
// The per-molecule gradient the head part leaves in dfp (tanh derivative applied), as the dense block's consumers read
// it: built once per backward
static ReadoutGrad readout_grad(const gcmi_graph* g, const Ws& w, float* ws, int D) {
  ReadoutGrad rg{g->d_membership, ws + w.dfp, 2 * (int64_t)D, reinterpret_cast<const int32_t*>(ws + w.arg_r)};
  rg.rawsum = ws + w.rsum; rg.runs = g->d_mol_runs; rg.n_mols = g->n_mols; rg.n_deg = g->max_deg + 1;
  return rg;
}

// A BatchNorm backward over N rows of x on the step's accumulator (zeroed once per call, self-cleaning afterwards);
// the caller names the gradient source and what else it wants
static BnBackward bn_backward(const float* x, int64_t ldx, int64_t N, double* acc, const BnSync* sy) {
  BnBackward q;
  q.x = x; q.ldx = ldx; q.n_rows = N; q.acc = acc; q.acc_clean = true; q.sync = sy;
  return q;
}

// GraphConv block b's BatchNorm backward from a pass over dy, and (dx given) the gradient w.r.t. the ReLU input
static int bn_bwd_rows(const Block& b, const float* dy, const float* gc, int64_t N, float* dx, double* acc,
                       const BnSync* sy, void* stream) {
  BnBackward q = bn_backward(gc, b.W, N, acc, sy);
  q.dy = dy; q.lddy = b.W; q.dx = dx; q.lddx = b.W; q.relu_mask = 1;
  return bn_bwd_impl(b.bn, q, stream);
}

// The per-molecule part of the backward in one kernel where the shapes allow (head_bwd.hip): loss, d logits, head
// gradients, the gradient w.r.t. GraphGather's pre-activation in rg.g2, and -- sums given: the one-pass dense block
// follows -- the backward sums of the dense layer's BatchNorm.  *done = false: shape not covered, nothing launched.
// *with_sums: the sums are in place, and the loss is finalised by the BatchNorm parameter launch that follows.
static int head_backward_fused(const gcmi_model_desc* m, const Ws& w, float* ws, const float* d_params, float* d_grads,
                               const gcmi_model_io* io, const float* d_labels, const float* d_weights, int64_t n_rows,
                               const ReadoutGrad& rg, const BnPoint& dense_bn, double* sums, void* stream, bool* done,
                               bool* with_sums) {
  double* lacc = reinterpret_cast<double*>(ws + w.lacc);
  HeadBackward h;
  h.kind = m->mode == 0 ? 0 : 1; h.logits = io->d_logits; h.labels = d_labels; h.weights = d_weights;
  h.n_rows = n_rows; h.n_tasks = m->n_tasks; h.n_classes = m->n_classes;
  h.fp = io->d_fingerprint; h.ldfp = 2 * dense_bn.n_feat;
  h.w = d_params + m->off_head_w; h.dw = d_grads + m->off_head_w; h.db = d_grads + m->off_head_b;
  h.rg = &rg; h.g2 = ws + w.dfp; h.loss_acc = lacc; h.dense_bn = &dense_bn; h.sums = sums;
  h.dl_scratch = ws + w.dlogits; h.img = w.himg >= 0 ? ws + w.himg : nullptr;
  *done = *with_sums = false;
  const int rc = head_bwd_fused(h, (hipStream_t)stream);
  if (rc == GCMI_ERR_UNSUPPORTED) return GCMI_OK;
  RUN(rc);
  *done = true;
  *with_sums = sums != nullptr;
  if (!*with_sums) RUN(loss_finalize_impl(lacc, 1.f / (float)(n_rows * m->n_tasks), io->d_loss, stream, kLossRep));
  return GCMI_OK;
}

// The dense block in one pass (fused_dense_bwd): G from the readout gradient, the block's output `dense` and coef;
// dW, db; dpool = G W, and in psums the pooled sums for the BatchNorm below.  *n_rows must outlive the description.
static BlockBackward dense_backward(const int32_t* n_rows, const ReadoutGrad& rg, const float* dense, const float* coef,
                                    const float* pool, const Block& dn, float* dpool, double* psums) {
  BlockBackward q;
  q.n_seg = 1; q.seg_begin = &kZero32; q.seg_end = n_rows; q.w_off[0] = &kZero64; q.b_off = &kZero64;
  q.rg = &rg; q.gc = dense; q.ldgc = dn.W; q.coef = coef; q.width = dn.W;
  q.in[0] = {pool, dn.K}; q.k_in = dn.K; q.w = dn.w; q.dw = dn.dw; q.db = dn.dbias;
  q.dout[0] = {dpool, dn.K}; q.psums = psums;
  return q;
}

// GraphConv block b in one pass (fused_conv_bwd): G from dy, the block's output gc and coef; dW_rel, dW_self, dbsum
// over [S | X].  The caller adds the input gradients (dout[].rows, psums) where the block below needs them.
static BlockBackward conv_backward(const Segs& sg, const float* dy, const float* gc, const float* coef, const Block& b,
                                   const float* s, int64_t lds, const float* x, int64_t ldx) {
  BlockBackward q;
  q.n_seg = sg.n; q.seg_begin = sg.begin; q.seg_end = sg.end; q.w_off[0] = sg.w_rel; q.w_off[1] = sg.w_self; q.b_off = sg.b_off;
  q.dy = dy; q.lddy = b.W; q.gc = gc; q.ldgc = b.W; q.coef = coef; q.width = b.W;
  q.in[0] = {s, lds}; q.in[1] = {x, ldx}; q.k_in = b.K; q.w = b.w; q.dw = b.dw; q.db = b.dbias;
  q.dout[0].ld = q.dout[1].ld = b.K;
  return q;
}

// block l's bias gradient sums are in place: unpacked into the reference's bias rows in one launch after the loop
static void note_bias_grads(BiasLayers& ub, int l, const Block& b) {
  ub.src[l] = b.dbias; ub.dst[l] = b.dbias_rows; ub.width[l] = b.W;
}

// ------------------------------------------------------------------------------------------------------------------
// storage == 1: the same step with every matrix it writes and reads back kept as bf16 (fp32 arithmetic, fp64
// statistics, fp32 parameters / gradients / gradient streams).  One linear sequence of the kernels that have a bf16
// form; what they do not cover (other widths, no BatchNorm, graphs without window plans or reverse slots, the
// exact-fp32 product mode) is refused, never computed some other way.
static int require_h(const gcmi_model_desc* m, const gcmi_graph* g, const gcmi_model_io* io, bool backward) {
  if (gemm_exact_mode()) {
    set_error("bf16 activation storage: not available in the exact-fp32 product mode (set_gemm_mode('fast'))");
    return GCMI_ERR_UNSUPPORTED;
  }
  if (g->n_atoms > 0 && (!win_usable_h(g, 64) || !win_usable_h(g, 80) || !win_usable(g, (int)up4(m->n_feat_in), false) ||
                         !win_has_width((int)up4(m->n_feat_in)))) {
    set_error("bf16 activation storage: the graph carries no usable molecule-window plan (collate with gcmi_collate_plans)");
    return GCMI_ERR_UNSUPPORTED;
  }
  if (g->n_atoms > 0 && (io->ld_features % 4 != 0 || io->ld_features < up4(m->n_feat_in) || !aligned16(io->d_atom_features))) {
    set_error("bf16 activation storage: atom feature rows must be 16-byte addressable and padded to %d columns",
              (int)up4(m->n_feat_in));
    return GCMI_ERR_UNSUPPORTED;
  }
  if (backward && g->n_atoms > 0) {
    if (!(g->d_rev_pos != nullptr || g->n_edges == 0)) {
      set_error("bf16 activation storage: the backward needs reverse slots (every bond listed from both ends)");
      return GCMI_ERR_UNSUPPORTED;
    }
    if (!fused_bwd_enabled()) {
      set_error("bf16 activation storage: the one-pass block kernels are switched off (GCMI_OPT_FUSED_BWD)");
      return GCMI_ERR_UNSUPPORTED;
    }
    if (m->storage == 2 && !win_usable_gh(g, 64)) {
      set_error("bf16 gradient streams: the graph carries no usable molecule-window plan");
      return GCMI_ERR_UNSUPPORTED;
    }
  }
  return GCMI_OK;
}

static int model_forward_h(const gcmi_model_desc* m, const gcmi_graph* g, const float* d_params, const gcmi_model_io* io,
                           int32_t training, gcmi_stat_sync_fn sync, void* sync_ctx, void* stream) {
  RUN(require_h(m, g, io, false));
  hipStream_t st = (hipStream_t)stream;
  const int L = m->n_layers;
  const int64_t N = g->n_atoms, B = g->n_mols;
  const Ws w = carve(m, N, B, io->ld_features);
  float* ws = io->d_workspace;
  Block blk[kMaxL + 1];
  make_blocks(m, w, ws, d_params, nullptr, io, blk);
  auto H = [&](int64_t off) { return reinterpret_cast<bf16_t*>(ws + off); };
  double* acc = reinterpret_cast<double*>(ws + w.acc);
  const BnSync sync_s = make_sync(sync, sync_ctx, w, ws);
  const BnSync* sy = (sync && training) ? &sync_s : nullptr;
  if (training && N > 0 && hipMemsetAsync(ws + w.acc, 0, sizeof(float) * (size_t)(w.z_end - w.acc), st) != hipSuccess) {
    set_error("model_forward: memset failed");
    return GCMI_ERR_LAUNCH;
  }
  const bf16_t* xin = nullptr;
  int64_t ldin = 0;
  RUN(pack_biases(m, w, ws, d_params, st));
  for (int l = 0; l < L; ++l) {
    const Block& b = blk[l];
    const Segs sg = make_segs(g, b.K, b.W);
    if (N > 0) {
      {
        TimedScope ts(GCMI_K_GATHER_SUM, st);
        if (l == 0) {  // fp32 atom features -> bf16 neighbour sums + a bf16 copy of the rows themselves
          RUN(win_gather_sum_fh(g, io->d_atom_features, io->ld_features, (int)w.ngather[0], H(w.S[0]), H(w.xb), w.ldS[0], st));
          xin = H(w.xb);
          ldin = w.ldS[0];
        } else {
          RUN(win_gather_sum_h(g, xin, ldin, b.K, H(w.S[l]), w.ldS[l], st));
        }
      }
      {
        TimedScope ts(GCMI_K_SEG_GEMM, st);
        const int rc = fwd_h_gemm(conv_product(sg, H(w.S[l]), w.ldS[l], xin, ldin, b, H(w.gc[l])),
                                  training ? acc : nullptr, ws + w.wimg, st);
        if (rc == GCMI_ERR_UNSUPPORTED) set_error("bf16 activation storage: GraphConv %d has no bf16 product kernel", l);
        RUN(rc);
      }
      RUN(bn_forward(b, N, training, true, nullptr, 0, acc, stream, sy));
      {
        TimedScope ts(GCMI_K_GATHER_MAX, st);
        RUN(win_gather_max_h(g, H(w.gc[l]), b.W, b.W, b.bn.scale, b.bn.shift, H(w.pool[l]), b.W,
                             training ? reinterpret_cast<uint8_t*>(ws + w.arg[l]) : nullptr, st));
      }
    } else if (sy) {
      RUN(bn_forward(b, 0, training, true, nullptr, 0, acc, stream, sy));
    }
    xin = H(w.pool[l]);
    ldin = b.W;
  }
  const Block& dn = blk[L];
  const int D = dn.W;
  if (N > 0) {
    const int32_t nN = (int32_t)N;
    {
      TimedScope ts(GCMI_K_SEG_GEMM, st);
      SegProduct<bf16_t> p = one_segment(&nN, xin, ldin, dn.K, dn.w, dn.bias, D, H(w.dense), D);
      p.trans_w = 1;
      p.act = 1;
      const int rc = fwd_h_gemm(p, training ? acc : nullptr, ws + w.wimg, st);
      if (rc == GCMI_ERR_UNSUPPORTED) set_error("bf16 activation storage: the dense layer has no bf16 product kernel");
      RUN(rc);
    }
    RUN(bn_forward(dn, N, training, true, nullptr, 0, acc, stream, sy));
  } else if (sy) {
    RUN(bn_forward(dn, 0, training, true, nullptr, 0, acc, stream, sy));
  }
  RUN(readout_fwd_impl(g, reinterpret_cast<const float*>(H(w.dense)), D, D, N > 0 ? dn.bn.scale : nullptr,
                       N > 0 ? dn.bn.shift : nullptr, 1, io->d_fingerprint, 2 * D, reinterpret_cast<int32_t*>(ws + w.arg_r),
                       training ? ws + w.rsum : nullptr, stream, 1));
  RUN(head_forward(m, w, ws, d_params, io, B, stream));
  if (m->mode == 0 && io->d_probs) RUN(gcmi_softmax(io->d_logits, B * m->n_tasks, m->n_classes, io->d_probs, stream));
  if (training && N == 0 && !sy) RUN(bump_counters(m, io, st));  // (sy: the finalisation of every exchange did)
  return GCMI_OK;
}

static int model_loss_backward_h(const gcmi_model_desc* m, const gcmi_graph* g, const float* d_params, float* d_grads,
                                 const gcmi_model_io* io, const float* d_labels, const float* d_weights, int64_t n_rows,
                                 int64_t* grad_lo, int64_t* grad_hi, gcmi_stat_sync_fn sync, void* sync_ctx,
                                 void* stream) {
  RUN(require_h(m, g, io, true));
  hipStream_t st = (hipStream_t)stream;
  const int L = m->n_layers;
  const int64_t N = g->n_atoms, B = g->n_mols;
  const Ws w = carve(m, N, B, io->ld_features);
  float* ws = io->d_workspace;
  Block blk[kMaxL + 1];
  make_blocks(m, w, ws, d_params, d_grads, io, blk);
  auto H = [&](int64_t off) { return reinterpret_cast<bf16_t*>(ws + off); };
  auto HF = [&](int64_t off) { return reinterpret_cast<const float*>(ws + off); };  // a bf16 matrix behind a float* parameter
  const bool full = m->grad_mode == 1;
  const int64_t lo = full ? 0 : m->off_bn_gamma[L - 1];
  const int64_t hi = m->n_params;
  if (grad_lo) *grad_lo = lo;
  if (grad_hi) *grad_hi = hi;
  if (hipMemsetAsync(d_grads + lo, 0, sizeof(float) * (size_t)(hi - lo), st) != hipSuccess ||
      hipMemsetAsync(ws + w.dlogits, 0, sizeof(float) * (size_t)(w.z_end - w.dlogits), st) != hipSuccess) {
    set_error("model_loss_backward: memset failed");
    return GCMI_ERR_LAUNCH;
  }
  double* acc = reinterpret_cast<double*>(ws + w.acc);
  double* acc2 = reinterpret_cast<double*>(ws + w.acc2);
  double* lacc = reinterpret_cast<double*>(ws + w.lacc);
  const float loss_inv_count = 1.f / (float)(n_rows * m->n_tasks);
  const BnSync sync_s = make_sync(sync, sync_ctx, w, ws);
  const BnSync* sy = sync ? &sync_s : nullptr;
  // ---- per-molecule part (fp32 throughout: the fingerprint and everything behind it are per-molecule rows)
  const Block& dn = blk[L];
  const int D = dn.W;
  const ReadoutGrad rg = readout_grad(g, w, ws, D);
  bool head_done = false, head_sums = false;
  RUN(head_backward_fused(m, w, ws, d_params, d_grads, io, d_labels, d_weights, n_rows, rg, dn.bn,
                          (N > 0 && g->d_mol_runs) ? acc : nullptr, stream, &head_done, &head_sums));
  if (!head_done) RUN(head_backward_separate(m, w, ws, d_params, d_grads, io, d_labels, d_weights, n_rows, B, true, stream));
  if (N == 0) return sy ? empty_backward_syncs(m, blk, *sy, stream) : GCMI_OK;
  float* dpool = ws + w.tC;
  const float* coef = ws + w.acc;
  // storage == 2: dpool, dy, dS and dXs are bf16 rows (in the same fp32-sized workspace blocks, ld in elements)
  const bool gb = m->storage == 2;
  auto HG = [](float* p) { return reinterpret_cast<bf16_t*>(p); };
  // ---- dense block: BatchNorm sums from per-molecule data, then one pass (dense and pool rows arrive as bf16)
  {
    // (the per-molecule sums kernel reads rawsum, never the atom rows: the bf16 matrix is only passed through)
    BnBackward q = bn_backward(HF(w.dense), D, N, acc, sy);
    if (head_sums) {
      q.loss = {lacc, kLossRep, loss_inv_count, io->d_loss};
      RUN(bn_bwd_params_impl(dn.bn, q, stream));
    } else {
      q.rg = &rg;
      RUN(bn_bwd_impl(dn.bn, q, stream));
    }
  }
  {
    TimedScope ts(GCMI_K_FUSED_BWD, st);
    const int32_t nN = (int32_t)N;
    BlockBackward q = dense_backward(&nN, rg, HF(w.dense), coef, HF(w.pool[L - 1]), dn, dpool, acc2);
    q.act_bf16 = gb ? 2 : 1;
    const int rc = fused_dense_bwd(q, st);
    if (rc == GCMI_ERR_UNSUPPORTED) set_error("bf16 activation storage: the dense block has no one-pass backward");
    RUN(rc);
  }
  // ---- GraphConv / BatchNorm / GraphPool blocks, last to first (gradient streams fp32: the window kernels as they are)
  bool dy_ready = false;
  BiasLayers ub;
  memset(&ub, 0, sizeof(ub));
  for (int l = L - 1; l >= 0; --l) {
    const Block& b = blk[l];
    const int W = b.W, K = b.K;
    float* dy = ws + w.tD;
    const Segs sg = make_segs(g, K, W);
    const bf16_t* xin = l == 0 ? H(w.xb) : H(w.pool[l - 1]);
    const int64_t ldx = l == 0 ? w.ldS[0] : m->conv_width[l - 1];
    float* dS = ws + w.tE;
    float* dX = ws + w.tC;
    const uint8_t* arg = reinterpret_cast<const uint8_t*>(ws + w.arg[l]);
    // the block above left sum dP and sum dP * P: this BatchNorm's backward needs no pass over dy (bn_bwd_pool_impl);
    // dy itself only when the GraphConv below trains, or where the pooled sums are ill-conditioned
    if (dy_ready) {
      // (left by win_gather_sumacc_max_bwd below, one iteration ago)
    } else if (gb) {
      TimedScope ts(GCMI_K_GATHER_MAX_BWD, st);
      RUN(win_gather_max_bwd_h(g, HG(dpool), W, W, arg, HG(dy), W, full ? nullptr : b.bn.gamma, full ? nullptr : b.bn.beta, st));
    } else if (full) {
      RUN(gcmi_gather_max_bwd(g, dpool, W, W, arg, dy, W, stream));
    } else {
      TimedScope ts(GCMI_K_GATHER_MAX_BWD, st);
      RUN(win_gather_max_bwd_if_ill(g, dpool, W, W, arg, dy, W, b.bn.gamma, b.bn.beta, st));
    }
    {
      BnBackward q = bn_backward(HF(w.gc[l]), W, N, acc, sy);
      q.dy = dy; q.lddy = W; q.x_bf16 = gb ? 2 : 1; q.psums = acc2;
      RUN(bn_bwd_pool_impl(b.bn, q, stream));
    }
    dy_ready = false;
    if (!full) break;  // reference semantics: nothing in front of a GraphConv output trains
    {
      TimedScope ts(GCMI_K_FUSED_BWD, st);
      BlockBackward q = conv_backward(sg, dy, HF(w.gc[l]), coef, b, HF(w.S[l]), w.ldS[l], reinterpret_cast<const float*>(xin), ldx);
      q.act_bf16 = gb ? 2 : 1;
      if (l > 0) { q.dout[0].rows = dS; q.dout[1].rows = dX; q.psums = acc2; }
      const int rc = fused_conv_bwd(q, st);
      if (rc == GCMI_ERR_UNSUPPORTED) set_error("bf16 activation storage: GraphConv %d has no one-pass backward", l);
      RUN(rc);
    }
    note_bias_grads(ub, l, b);
    if (l == 0) break;  // the atom features need no gradient
    // dX holds the self part; the neighbour part is added onto it, and where the window kernels can hold a third tile
    // the GraphPool backward of the block below runs in the same pass
    const uint8_t* arg_below = reinterpret_cast<const uint8_t*>(ws + w.arg[l - 1]);
    if (gb) {
      if (!win_two_stage_usable_h(g, K)) {
        set_error("bf16 gradient streams: no LDS for the two-stage window pass");
        return GCMI_ERR_UNSUPPORTED;
      }
      TimedScope ts(GCMI_K_GATHER_MAX_BWD, st);
      RUN(win_gather_sumacc_max_bwd_h(g, HG(dS), K, K, HG(dX), K, arg_below, HG(ws + w.tD), K, st));
      dy_ready = true;
    } else if (win_two_stage_usable(g, K) && aligned16(dS) && aligned16(dX) && aligned16(ws + w.tD)) {
      TimedScope ts(GCMI_K_GATHER_MAX_BWD, st);
      RUN(win_gather_sumacc_max_bwd(g, dS, K, K, dX, K, arg_below, ws + w.tD, K, st));
      dy_ready = true;
    } else {
      RUN(gcmi_gather_sum_fwd(g, dS, K, K, dX, K, 1, stream));
    }
    dpool = dX;
  }
  RUN(unpack_bias_grads(m, ub, L, st));
  return GCMI_OK;
}

}  // namespace gcmi

using namespace gcmi;

extern "C" {

int gcmi_count_not_small_int(const float* d_x, int64_t ld, int64_t n_rows, int32_t n_cols, int32_t max_deg,
                             int64_t* d_count, void* stream) {
  GCMI_CHECK_ARG(d_count != nullptr && n_rows >= 0 && n_cols >= 0 && ld >= n_cols, "count_not_small_int: bad shape");
  GCMI_CHECK_ARG(n_rows * (int64_t)n_cols == 0 || d_x != nullptr, "count_not_small_int: NULL matrix");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_count, 0, sizeof(int64_t), st) != hipSuccess) {
    set_error("count_not_small_int: memset failed");
    return GCMI_ERR_LAUNCH;
  }
  if (n_rows * (int64_t)n_cols == 0) return GCMI_OK;
  const float limit = (float)(256 / std::max(1, max_deg));
  hipLaunchKernelGGL(small_int_count_kernel, dim3(grid_for(n_rows * (int64_t)n_cols, 256)), dim3(256), 0, st, d_x, ld, n_rows,
                     n_cols, limit, reinterpret_cast<unsigned long long*>(d_count));
  GCMI_CHECK_LAUNCH("count_not_small_int");
  return GCMI_OK;
}

int64_t gcmi_model_workspace_floats(const gcmi_model_desc* m, int64_t n_atoms, int64_t n_mols) {
  if (check_desc(m) != GCMI_OK || n_atoms < 0 || n_mols < 0) return -1;
  // ld of the features is not known here: assume the padded width (worst case)
  return carve(m, n_atoms, n_mols, up4(m->n_feat_in)).total;
}

int gcmi_model_forward(const gcmi_model_desc* m, const gcmi_graph* g, const float* d_params,
                       const gcmi_model_io* io, int32_t training, void* stream) {
  return gcmi_model_forward_dp(m, g, d_params, io, training, nullptr, nullptr, stream);
}

int gcmi_model_forward_dp(const gcmi_model_desc* m, const gcmi_graph* g, const float* d_params,
                          const gcmi_model_io* io, int32_t training, gcmi_stat_sync_fn sync, void* sync_ctx,
                          void* stream) {
  RUN(check_desc(m));
  GCMI_CHECK_ARG(sync == nullptr || m->batch_norm, "model_forward_dp: a statistics exchange for a model without BatchNorm");
  RUN(check_graph(g, true));
  GCMI_CHECK_ARG(io && d_params && io->d_workspace && io->d_logits && io->d_fingerprint,
                 "model_forward: NULL buffer");
  GCMI_CHECK_ARG(g->max_deg == m->max_deg, "graph max_deg %d != model max_deg %d", g->max_deg, m->max_deg);
  GCMI_CHECK_ARG(g->n_mols > 1, "graph_gather requires batches larger than 1");
  GCMI_CHECK_ARG(g->n_atoms == 0 || io->d_atom_features, "model_forward: NULL atom features");
  GCMI_CHECK_ARG(io->ld_features >= m->n_feat_in, "ld_features < n_feat_in");
  if (sync && training) RUN(check_sync_buffers(m, g, io));
  if (m->storage >= 1) return model_forward_h(m, g, d_params, io, training, sync, sync_ctx, stream);
  hipStream_t st = (hipStream_t)stream;
  const int L = m->n_layers;
  const int64_t N = g->n_atoms, B = g->n_mols;
  const Ws w = carve(m, N, B, io->ld_features);
  float* ws = io->d_workspace;
  Block blk[kMaxL + 1];
  make_blocks(m, w, ws, d_params, nullptr, io, blk);
  const float* x = io->d_atom_features;
  int64_t ldx = io->ld_features;
  if (training && m->batch_norm && N > 0 &&
      hipMemsetAsync(ws + w.acc, 0, sizeof(float) * (size_t)(w.z_end - w.acc), st) != hipSuccess) {
    set_error("model_forward: memset failed");
    return GCMI_ERR_LAUNCH;
  }
  // training with BatchNorm: a product's epilogue also adds the column sums of its output into the BatchNorm
  // accumulators (clean: zeroed above, self-cleaning afterwards), so the layer output is not read again
  double* acc = reinterpret_cast<double*>(ws + w.acc);
  double* stats = (m->batch_norm && training) ? acc : nullptr;
  const BnSync sync_s = make_sync(sync, sync_ctx, w, ws);
  const BnSync* sy = (sync && training) ? &sync_s : nullptr;
  bool stats_fused = false;
  const bool one_piece = one_piece_block0(m, g, io);
  note_one_piece(ws, one_piece);
  RUN(pack_biases(m, w, ws, d_params, st));
  for (int l = 0; l < L; ++l) {
    const Block& b = blk[l];
    const int W = b.W;
    const Segs sg = make_segs(g, b.K, W);
    stats_fused = false;
    if (l == 0 && one_piece) {
      RUN(one_piece_forward(g, w, ws, b, sg, io, stats, st));
      stats_fused = training != 0;
    } else if (N > 0) {
      // (l > 0: the GraphPool of the block below left the neighbour sums of its output with it)
      if (l == 0) RUN(gcmi_gather_sum_fwd(g, x, ldx, (int32_t)w.ngather[l], ws + w.S[l], w.ldS[l], 0, stream));
      RUN(seg_gemm_stats(conv_product(sg, ws + w.S[l], w.ldS[l], x, ldx, b, ws + w.gc[l]), stats, &stats_fused, st,
                         ws + w.wimg));
    }
    const bool bn = m->batch_norm && N > 0;
    if (bn || sy) RUN(bn_forward(b, N, training, stats_fused, ws + w.gc[l], W, acc, stream, sy));
    if (N > 0) {
      uint8_t* arg = training ? reinterpret_cast<uint8_t*>(ws + w.arg[l]) : nullptr;
      const float* sc = bn ? b.bn.scale : nullptr;
      const float* sh = bn ? b.bn.shift : nullptr;
      if (l + 1 < L)  // GraphPool and the neighbour sums of the block above in one window pass
        RUN(gcmi_gather_max_sum_fwd(g, ws + w.gc[l], W, W, sc, sh, ws + w.pool[l], W, arg, ws + w.S[l + 1], w.ldS[l + 1], stream));
      else
        RUN(gcmi_gather_max_fwd(g, ws + w.gc[l], W, W, sc, sh, ws + w.pool[l], W, arg, stream));
    }
    x = ws + w.pool[l];
    ldx = W;
  }
  const Block& dn = blk[L];
  const int D = dn.W;
  if (N > 0) {
    const int32_t nN = (int32_t)N;
    SegProduct<float> p = one_segment(&nN, x, ldx, dn.K, dn.w, dn.bias, D, ws + w.dense, D);
    p.trans_w = 1;
    p.act = 1;
    RUN(seg_gemm_stats(p, stats, &stats_fused, st));
  }
  const bool bn = m->batch_norm && N > 0;
  if (bn || sy) RUN(bn_forward(dn, N, training, stats_fused, ws + w.dense, D, acc, stream, sy));
  RUN(readout_fwd_impl(g, ws + w.dense, D, D, bn ? dn.bn.scale : nullptr, bn ? dn.bn.shift : nullptr, 1, io->d_fingerprint,
                       2 * D, reinterpret_cast<int32_t*>(ws + w.arg_r),
                       (training && m->batch_norm) ? ws + w.rsum : nullptr, stream));
  RUN(head_forward(m, w, ws, d_params, io, B, stream));
  if (m->mode == 0 && io->d_probs)
    RUN(gcmi_softmax(io->d_logits, B * m->n_tasks, m->n_classes, io->d_probs, stream));
  if (training && m->batch_norm && N == 0 && !sy) RUN(bump_counters(m, io, st));  // (sy: every exchange's finalisation did)
  return GCMI_OK;
}

int gcmi_model_loss_backward(const gcmi_model_desc* m, const gcmi_graph* g, const float* d_params,
                             float* d_grads, const gcmi_model_io* io, const float* d_labels,
                             const float* d_weights, int64_t n_rows, int64_t* grad_lo,
                             int64_t* grad_hi, void* stream) {
  return gcmi_model_loss_backward_dp(m, g, d_params, d_grads, io, d_labels, d_weights, n_rows, grad_lo, grad_hi, nullptr,
                                     nullptr, stream);
}

int gcmi_model_loss_backward_dp(const gcmi_model_desc* m, const gcmi_graph* g, const float* d_params,
                                float* d_grads, const gcmi_model_io* io, const float* d_labels,
                                const float* d_weights, int64_t n_rows, int64_t* grad_lo, int64_t* grad_hi,
                                gcmi_stat_sync_fn sync, void* sync_ctx, void* stream) {
  RUN(check_desc(m));
  GCMI_CHECK_ARG(sync == nullptr || m->batch_norm,
                 "model_loss_backward_dp: a statistics exchange for a model without BatchNorm");
  RUN(check_graph(g, true));
  GCMI_CHECK_ARG(io && d_params && d_grads && io->d_workspace && io->d_logits && io->d_fingerprint &&
                     io->d_loss && d_labels,
                 "model_loss_backward: NULL buffer");
  GCMI_CHECK_ARG(n_rows > 0 && n_rows <= g->n_mols, "n_rows %lld outside (0, n_mols=%d]", (long long)n_rows,
                 g->n_mols);
  if (sync) RUN(check_sync_buffers(m, g, io));
  if (m->storage >= 1)
    return model_loss_backward_h(m, g, d_params, d_grads, io, d_labels, d_weights, n_rows, grad_lo, grad_hi, sync,
                                 sync_ctx, stream);
  hipStream_t st = (hipStream_t)stream;
  const int L = m->n_layers;
  const int64_t N = g->n_atoms, B = g->n_mols;
  const Ws w = carve(m, N, B, io->ld_features);
  float* ws = io->d_workspace;
  Block blk[kMaxL + 1];
  make_blocks(m, w, ws, d_params, d_grads, io, blk);
  const bool full = m->grad_mode == 1;
  const bool sym = g->d_rev_pos != nullptr || g->n_edges == 0;
  const int64_t lo = full ? 0 : (m->batch_norm ? m->off_bn_gamma[L - 1] : m->off_dense_w);
  const int64_t hi = m->n_params;
  if (grad_lo) *grad_lo = lo;
  if (grad_hi) *grad_hi = hi;
  auto zero = [&](void* p, size_t bytes) -> int {
    if (bytes && hipMemsetAsync(p, 0, bytes, st) != hipSuccess) {
      set_error("model_loss_backward: memset failed");
      return GCMI_ERR_LAUNCH;
    }
    return GCMI_OK;
  };
  RUN(zero(d_grads + lo, sizeof(float) * (size_t)(hi - lo)));
  // dlogits (rows beyond n_rows carry no gradient), the bias-gradient sums and every accumulator
  RUN(zero(ws + w.dlogits, sizeof(float) * (size_t)(w.z_end - w.dlogits)));
  double* acc = reinterpret_cast<double*>(ws + w.acc);
  double* acc2 = reinterpret_cast<double*>(ws + w.acc2);
  double* lacc = reinterpret_cast<double*>(ws + w.lacc);
  const float loss_inv_count = 1.f / (float)(n_rows * m->n_tasks);
  const BnSync sync_s = make_sync(sync, sync_ctx, w, ws);
  const BnSync* sy = sync ? &sync_s : nullptr;
  const Block& dn = blk[L];
  const int D = dn.W, Wl = dn.K;
  const int32_t nN = (int32_t)N;
  // ---- per-molecule part in one kernel where the shapes allow (head_bwd.hip): loss, d logits, head gradients, the
  // gradient w.r.t. GraphGather's pre-activation (tanh derivative applied), and -- when the one-pass dense block
  // follows -- the BatchNorm backward sums of the dense layer
  const bool dense_one_pass = dense_block_one_pass(m, N);
  const ReadoutGrad rg = readout_grad(g, w, ws, D);
  bool head_done = false, head_sums = false;
  if (m->batch_norm)  // (without BatchNorm the readout backward applies the tanh derivative itself)
    RUN(head_backward_fused(m, w, ws, d_params, d_grads, io, d_labels, d_weights, n_rows, rg, dn.bn,
                            (dense_one_pass && g->d_mol_runs) ? acc : nullptr, stream, &head_done, &head_sums));
  // (the tanh derivative applied in place only for the BatchNorm backward below)
  if (!head_done)
    RUN(head_backward_separate(m, w, ws, d_params, d_grads, io, d_labels, d_weights, n_rows, B, m->batch_norm && N > 0,
                               stream));
  if (N == 0) return sy ? empty_backward_syncs(m, blk, *sy, stream) : GCMI_OK;
  // ---- readout (+ folded BatchNorm of the dense layer, + its ReLU mask)
  float* dyD = ws + w.tA;   // grad w.r.t. the (normalised) readout input
  float* dxD = ws + w.tB;   // grad w.r.t. the dense pre-activation
  float* dpool = ws + w.tC;  // grad w.r.t. the output of the last GraphPool
  const float* coef = ws + w.acc;  // [A | B | C] of the BatchNorm backward just computed (bn.hip: head of its scratch)
  const int32_t* arg_r = reinterpret_cast<const int32_t*>(ws + w.arg_r);
  bool dense_done = false;
  bool have_psums = false;  // acc2 holds sum dP, sum dP * P for the BatchNorm below the block just processed
  bool dy_ready = false;  // the gather of the block above already left this block's dy (two-stage window pass)
  if (m->batch_norm) {
    // GraphGather backward is recomputed inside the BatchNorm backward from the per-molecule
    // gradient (tanh derivative applied in place): the N x D gradient is never written or re-read
    auto readout_bn_bwd = [&](float* dx, const BnSync* s) {
      BnBackward q = bn_backward(ws + w.dense, D, N, acc, s);
      q.rg = &rg; q.dx = dx; q.lddx = D; q.relu_mask = 1;
      return bn_bwd_impl(dn.bn, q, stream);
    };
    if (head_sums) {
      // the sums are in place (head_bwd.hip): dgamma, dbeta and the coefficient vectors
      BnBackward q = bn_backward(ws + w.dense, D, N, acc, sy);
      q.loss = {lacc, kLossRep, loss_inv_count, io->d_loss};
      RUN(bn_bwd_params_impl(dn.bn, q, stream));
    } else {
      RUN(readout_bn_bwd(dense_one_pass ? nullptr : dxD, sy));
    }
    if (dense_one_pass) {
      // one pass: dxD formed per 64-row tile in LDS, dW_dense += dxD^T pool, db += colsum, dpool = dxD W_dense
      TimedScope ts(GCMI_K_FUSED_BWD, st);
      const int rc = fused_dense_bwd(dense_backward(&nN, rg, ws + w.dense, coef, ws + w.pool[L - 1], dn, dpool, acc2), st);
      if (rc == GCMI_OK) {
        dense_done = true;
        have_psums = true;
      }
      else if (rc != GCMI_ERR_UNSUPPORTED) return rc;
      else if (sy) return refuse_second_sync("the one-pass dense block");
      else  // not covered after all (misaligned buffers): the separate pass, with its sums once more
        RUN(readout_bn_bwd(dxD, nullptr));
    }
  } else {
    RUN(gcmi_readout_bwd(g, ws + w.dfp, 2 * D, io->d_fingerprint, 2 * D, D, 1, arg_r, dyD, D, stream));
    RUN(gcmi_relu_bwd(dyD, D, ws + w.dense, D, N, D, stream));
    dxD = dyD;
  }
  // ---- dense layer
  if (!dense_done) {
    RUN(gcmi_seg_gemm_wgrad(1, &kZero32, &nN, ws + w.pool[L - 1], Wl, Wl, dxD, D, D, dn.dw, &kZero64, dn.dbias, &kZero64,
                            1, stream));
    RUN(seg_gemm(one_segment(&nN, dxD, D, D, dn.w, nullptr, Wl, dpool, Wl), st));
  }
  // ---- GraphConv / BatchNorm / GraphPool blocks, last to first
  BiasLayers ub;
  memset(&ub, 0, sizeof(ub));
  for (int l = L - 1; l >= 0; --l) {
    if (!full && !m->batch_norm) break;  // nothing trainable in front of the dense layer
    const Block& b = blk[l];
    const int W = b.W, K = b.K;
    float* dy = ws + w.tD;  // grad w.r.t. the (normalised) pool input
    float* dgc = ws + w.tA;  // grad w.r.t. the GraphConv pre-activation
    const Segs sg = make_segs(g, K, W);
    // (one-piece form of the first block: S0 and the copy Xb of the atom features are bf16 rows, as the forward left them)
    const bool one_piece = l == 0 && noted_one_piece(ws);
    const float* xin = one_piece ? ws + w.xb : l == 0 ? io->d_atom_features : ws + w.pool[l - 1];
    const int64_t ldx = one_piece ? kOnePieceLd : l == 0 ? io->ld_features : m->conv_width[l - 1];
    const int64_t ldS = one_piece ? kOnePieceLd : w.ldS[l];
    float* dS = ws + w.tE;
    float* dX = ws + w.tC;
    const uint8_t* arg = reinterpret_cast<const uint8_t*>(ws + w.arg[l]);
    // the fused pass covers the default widths in split-bf16 mode; it wants 16-byte rows of every operand
    const bool try_fused = full && fused_bwd_enabled() && W == 64 && ldx % 4 == 0 && aligned16(xin) &&
                           ((l == 0 && K > 32 && K <= 96) || (l > 0 && K > 32 && K <= 64));
    // GraphPool backward
    if (!sym) RUN(zero(dy, sizeof(float) * (size_t)(N * W)));
    const bool pool_sums = have_psums && m->batch_norm && sym && (try_fused || !full) && win_usable(g, W, true) &&
                           win_has_width(W);
    have_psums = false;
    if (pool_sums) {
      // The block above left sum dP and sum dP * P: this BatchNorm's backward needs no pass over dy (bn.hip,
      // bn_bwd_pool_impl).  dy itself is needed when the GraphConv below trains; otherwise only by the
      // ill-conditioned fallback, and the kernel returns at once unless that applies.
      if (dy_ready) {
        // (left by win_gather_sumacc_max_bwd below, one iteration ago)
      } else if (full) {
        RUN(gcmi_gather_max_bwd(g, dpool, W, W, arg, dy, W, stream));
      } else {
        TimedScope ts(GCMI_K_GATHER_MAX_BWD, st);
        RUN(win_gather_max_bwd_if_ill(g, dpool, W, W, arg, dy, W, b.bn.gamma, b.bn.beta, st));
      }
      BnBackward q = bn_backward(ws + w.gc[l], W, N, acc, sy);
      q.dy = dy; q.lddy = W; q.psums = acc2;
      RUN(bn_bwd_pool_impl(b.bn, q, stream));
    } else {
      if (!dy_ready) RUN(gcmi_gather_max_bwd(g, dpool, W, W, arg, dy, W, stream));
      if (m->batch_norm) {
        RUN(bn_bwd_rows(b, dy, ws + w.gc[l], N, (full && !try_fused) ? dgc : nullptr, acc, sy, stream));
      } else if (full && !try_fused) {
        RUN(gcmi_relu_bwd(dy, W, ws + w.gc[l], W, N, W, stream));
        dgc = dy;
      }
    }
    dy_ready = false;
    if (!full) break;  // reference semantics: nothing in front of a GraphConv output trains
    bool fused_done = false;
    if (try_fused) {
      // one pass over the rows: dgc formed per tile in LDS; dW_rel, dW_self, dbsum; and for l > 0 dS = dgc W_rel^T
      // and the self part of dX
      TimedScope ts(GCMI_K_FUSED_BWD, st);
      BlockBackward q = conv_backward(sg, dy, ws + w.gc[l], m->batch_norm ? coef : nullptr, b, ws + w.S[l], ldS, xin, ldx);
      q.in_bf16 = one_piece ? 1 : 0;
      if (l > 0) { q.dout[0].rows = dS; q.dout[1].rows = dX; q.psums = (sym && m->batch_norm) ? acc2 : nullptr; }
      const int rc = fused_conv_bwd(q, st);
      if (rc == GCMI_OK) {
        fused_done = true;
        have_psums = l > 0 && sym && m->batch_norm;
        if (one_piece) g_one_piece_launches.fetch_add(1, std::memory_order_relaxed);
      }
      else if (rc != GCMI_ERR_UNSUPPORTED) return rc;
      else if (sy) return refuse_second_sync("the one-pass GraphConv block");
      else if (m->batch_norm) {  // not covered after all (misaligned buffers): the separate pass, sums once more
        RUN(bn_bwd_rows(b, dy, ws + w.gc[l], N, dgc, acc, nullptr, stream));
      } else {
        RUN(gcmi_relu_bwd(dy, W, ws + w.gc[l], W, N, W, stream));
        dgc = dy;
      }
    }
    if (!fused_done && one_piece) {  // (the one-pass backward was switched off between the forward and this call)
      set_error("model_loss_backward: the forward left the first block's operands as bf16 rows, and the one-pass "
                "backward that reads them is not available now (GCMI_OPT_FUSED_BWD / GCMI_OPT_GEMM_EXACT changed?)");
      return GCMI_ERR_UNSUPPORTED;
    }
    if (!fused_done) {
      RUN(gcmi_seg_gemm_wgrad(sg.n, sg.begin, sg.end, ws + w.S[l], w.ldS[l], K, dgc, W, W, b.dw, sg.w_rel, nullptr,
                              nullptr, 0, stream));
      RUN(gcmi_seg_gemm_wgrad(sg.n, sg.begin, sg.end, xin, ldx, K, dgc, W, W, b.dw, sg.w_self, b.dbias, sg.b_off, 0,
                              stream));
    }
    note_bias_grads(ub, l, b);
    if (l == 0) break;  // the atom features need no gradient
    // dS = dgc . W_rel^T ; dX = dgc . W_self^T + (transposed gather of dS)
    if (fused_done) {
      // dX holds the self part: the neighbour part is added onto it (bonds listed from both ends: the scatter
      // of dS is a gather)
      // ... and when the window kernels can hold a third tile, the GraphPool backward of the block below in the
      // same pass: dX = dXs + gather(dS) is consumed in LDS and never exists in HBM
      const bool two_stage = sym && fused_bwd_enabled() && win_two_stage_usable(g, K) &&
                             aligned16(dS) && aligned16(dX) && aligned16(ws + w.tD);
      if (two_stage) {
        TimedScope ts(GCMI_K_GATHER_MAX_BWD, st);
        RUN(win_gather_sumacc_max_bwd(g, dS, K, K, dX, K, reinterpret_cast<const uint8_t*>(ws + w.arg[l - 1]),
                                      ws + w.tD, K, st));
        dy_ready = true;
      } else if (sym) RUN(gcmi_gather_sum_fwd(g, dS, K, K, dX, K, 1, stream));
      else RUN(gcmi_scatter_add(g, dS, K, K, dX, K, stream));
    } else {
      // dS = dgc . W_rel[d]^T
      SegProduct<float> dg = seg_product(sg, dgc, W, W, b.w, sg.w_rel, K, dS);
      dg.trans_w = 1;
      RUN(seg_gemm(dg, st));
      // bonds listed from both ends: the scatter of dS is a gather (LDS-window kernel), and the
      // self term accumulates onto it in the GEMM epilogue
      if (sym) RUN(gcmi_gather_sum_fwd(g, dS, K, K, dX, K, 0, stream));
      dg.op[0].w_off = sg.w_self;  // dX (+)= dgc . W_self[d]^T
      dg.act = sym ? 2 : 0;
      dg.out = dX;
      RUN(seg_gemm(dg, st));
      if (!sym) RUN(gcmi_scatter_add(g, dS, K, K, dX, K, stream));
    }
    dpool = dX;
  }
  RUN(unpack_bias_grads(m, ub, L, st));
  return GCMI_OK;
}

}  // extern "C"
