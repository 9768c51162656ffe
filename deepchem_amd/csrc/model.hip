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

// One call of the step, forward or backward: what the caller handed over, the workspace carved up, the blocks, the
// accumulators and the statistics exchange.  Built once per call (make_step; begin_forward / begin_backward add what
// only their direction has) and handed to every helper below.  storage: 0 = fp32 rows, 1 = the matrices the step
// writes and reads back are bf16, 2 = the gradient streams between the backward's kernels too.
struct Step {
  const gcmi_model_desc* m;
  const gcmi_graph* g;
  const gcmi_model_io* io;
  const float* d_params;
  float* d_grads;  // nullptr in the forward
  hipStream_t st;
  int L, storage;
  int64_t N, B;
  int32_t nN;      // N as the one segment of the dense products (outlives their descriptions)
  Ws w;
  float* ws;
  Block blk[kMaxL + 1];
  double *acc, *acc2, *lacc;
  BnSync sync_s;
  const BnSync* sy;  // synchronised BatchNorm: &sync_s where this call exchanges statistics, else nullptr
  // forward
  int32_t training;
  double* stats;   // training with BatchNorm: a product's epilogue also adds the column sums of its output into the
                   // BatchNorm accumulators (clean: zeroed once per pass, self-cleaning afterwards)
  // backward
  const float *d_labels, *d_weights;
  int64_t n_rows;
  int64_t *grad_lo, *grad_hi;  // optional: where the caller learns the range of d_grads this call writes
  float loss_inv_count;
  bool full;       // grad_mode 1: everything trains (else the reference's: nothing in front of a GraphConv output)
  bool sym;        // reverse slots: the scatter over the bonds is a gather
  bool one_piece;  // what the last training forward on this workspace left of the first block (g_one_piece_ws)
  ReadoutGrad rg;  // the per-molecule gradient the head part leaves in dfp, as the dense block's consumers read it
  BiasLayers ub;   // the blocks whose bias gradient sums are in place: unpacked in one launch after the loop

  Step() = default;
  Step(const Step&) = delete;
  bool bn() const { return m->batch_norm != 0; }
  bf16_t* H(int64_t off) const { return reinterpret_cast<bf16_t*>(ws + off); }  // a bf16 matrix of the workspace
  const float* HF(int64_t off) const { return ws + off; }  // a matrix of the step's storage behind a float* parameter
  static bf16_t* HG(float* p) { return reinterpret_cast<bf16_t*>(p); }  // storage 2: a gradient stream as bf16 rows
  // the backward's temporaries (storage 2: bf16 rows in the same fp32-sized blocks, ld in elements)
  float* dpool() const { return ws + w.tC; }  // grad w.r.t. a GraphPool's output; the block below finds its own here
  float* dX() const { return ws + w.tC; }     // grad w.r.t. a GraphConv's input rows (= dpool of the block below)
  float* dS() const { return ws + w.tE; }     // grad w.r.t. its neighbour sums
  float* dy() const { return ws + w.tD; }     // grad w.r.t. the (normalised) GraphPool input
  float* dgc() const { return bn() ? ws + w.tA : dy(); }  // grad w.r.t. the GraphConv pre-activation, where it is
                                                          // written out (no BatchNorm: the ReLU mask on dy in place)
  const float* coef() const { return ws + w.acc; }  // [A | B | C] of the BatchNorm backward just computed (bn.hip)
  const uint8_t* arg(int l) const { return reinterpret_cast<const uint8_t*>(ws + w.arg[l]); }
  int zero(void* p, size_t bytes, const char* who) const {
    if (bytes && hipMemsetAsync(p, 0, bytes, st) != hipSuccess) {
      set_error("%s: memset failed", who);
      return GCMI_ERR_LAUNCH;
    }
    return GCMI_OK;
  }
};

static void make_blocks(Step& s) {
  const gcmi_model_desc* m = s.m;
  const int L = m->n_layers;
  auto grad = [&](int64_t off) { return s.d_grads ? s.d_grads + off : nullptr; };
  for (int l = 0; l <= L; ++l) {
    Block& b = s.blk[l];
    b.K = l == 0 ? m->n_feat_in : m->conv_width[l - 1];
    b.W = l == L ? m->dense_width : m->conv_width[l];
    b.w = s.d_params + (l == L ? m->off_dense_w : m->off_conv_w[l]);
    b.bias = l == L ? s.d_params + m->off_dense_b : s.ws + s.w.bsum[l];
    b.dw = grad(l == L ? m->off_dense_w : m->off_conv_w[l]);
    b.dbias = l == L ? grad(m->off_dense_b) : s.ws + s.w.dbsum[l];
    b.dbias_rows = l == L ? nullptr : grad(m->off_conv_b[l]);
    BnPoint& p = b.bn;
    p = BnPoint();
    p.n_feat = b.W;
    if (m->batch_norm) {
      p.gamma = s.d_params + m->off_bn_gamma[l]; p.beta = s.d_params + m->off_bn_beta[l];
      p.dgamma = grad(m->off_bn_gamma[l]); p.dbeta = grad(m->off_bn_beta[l]);
    }
    float* bnv = s.ws + s.w.bnv[l];
    p.mean = bnv; p.invstd = bnv + b.W; p.scale = bnv + 2 * b.W; p.shift = bnv + 3 * b.W;
    p.running_mean = s.io->d_bn_running_mean[l]; p.running_var = s.io->d_bn_running_var[l];
    p.batches_tracked = s.io->d_bn_batches_tracked[l];
    p.eps = m->bn_eps; p.momentum = m->bn_momentum;
  }
}

// exchange: this call takes part in the statistics exchange of synchronised BatchNorm (sync given; the forward: training)
static void make_step(Step& s, const gcmi_model_desc* m, const gcmi_graph* g, const float* d_params, float* d_grads,
                      const gcmi_model_io* io, gcmi_stat_sync_fn sync, void* sync_ctx, bool exchange, void* stream) {
  s.m = m; s.g = g; s.io = io; s.d_params = d_params; s.d_grads = d_grads;
  s.st = (hipStream_t)stream;
  s.L = m->n_layers; s.storage = m->storage;
  s.N = g->n_atoms; s.B = g->n_mols; s.nN = (int32_t)s.N;
  s.w = carve(m, s.N, s.B, io->ld_features);
  s.ws = io->d_workspace;
  make_blocks(s);
  s.acc = reinterpret_cast<double*>(s.ws + s.w.acc);
  s.acc2 = reinterpret_cast<double*>(s.ws + s.w.acc2);
  s.lacc = reinterpret_cast<double*>(s.ws + s.w.lacc);
  s.sync_s = BnSync{sync, sync_ctx, reinterpret_cast<double*>(s.ws + s.w.xch)};  // (the exchange buffer of one point)
  s.sy = exchange ? &s.sync_s : nullptr;
  s.training = 0; s.stats = nullptr;
  s.d_labels = s.d_weights = nullptr; s.n_rows = 0; s.grad_lo = s.grad_hi = nullptr; s.loss_inv_count = 0.f;
  s.full = m->grad_mode == 1;
  s.sym = g->d_rev_pos != nullptr || g->n_edges == 0;
  s.one_piece = false;
  memset(&s.ub, 0, sizeof(s.ub));
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


// b_rel_d + b_self_d of every GraphConv layer (the products add ONE bias row per degree): one launch for all layers
static int pack_biases(const Step& s) {
  BiasLayers bl;
  memset(&bl, 0, sizeof(bl));
  for (int l = 0; l < s.L; ++l) {
    bl.src[l] = s.d_params + s.m->off_conv_b[l];
    bl.dst[l] = s.ws + s.w.bsum[l];
    bl.width[l] = s.m->conv_width[l];
  }
  hipLaunchKernelGGL(bias_pack_kernel, dim3(4, s.L), dim3(256), 0, s.st, bl, s.m->max_deg);
  GCMI_CHECK_LAUNCH("bias_pack");
  return GCMI_OK;
}

// ... and the per-degree bias gradients back into the reference's (2 max_deg + 1) rows, for the layers whose block ran
static int unpack_bias_grads(const Step& s) {
  bool any = false;
  for (int l = 0; l < s.L; ++l) any = any || s.ub.src[l] != nullptr;
  if (!any) return GCMI_OK;
  hipLaunchKernelGGL(bias_unpack_kernel, dim3(4, s.L), dim3(256), 0, s.st, s.ub, s.m->max_deg);
  GCMI_CHECK_LAUNCH("bias_unpack");
  return GCMI_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Forward

// BatchNorm of block b, folded into b.bn.scale / shift for the kernel that reads the rows next: training = this
// batch's statistics, from the sums the product left in acc (stats_fused) or from a pass over the rows; eval = the
// running statistics
// (s.sy: synchronised BatchNorm, training only -- the statistics of the global batch, also for a rank with N == 0)
static int bn_forward(const Step& s, const Block& b, bool stats_fused, const float* rows, int64_t ld) {
  const BnPoint& p = b.bn;
  if (!s.training)
    return gcmi_bn_fold_eval(p.gamma, p.beta, p.running_mean, p.running_var, p.eps, p.n_feat, p.scale, p.shift, s.st);
  BnForward f;
  f.x = rows; f.ldx = ld; f.sums_ready = stats_fused; f.n_rows = s.N; f.acc = s.acc; f.sync = s.sy;
  f.acc_clean = true;  // zeroed once per pass (begin_forward)
  return bn_train_forward(p, f, s.st);
}

// A training batch without atoms launches no statistics kernel, and those are what bump the counters otherwise
static int bump_counters(const Step& s) {
  CounterPtrs c;
  c.n = s.L + 1;
  bool any = false;
  for (int i = 0; i <= kMaxL; ++i) {
    c.p[i] = i <= s.L ? s.io->d_bn_batches_tracked[i] : nullptr;
    any = any || c.p[i] != nullptr;
  }
  if (any) {
    hipLaunchKernelGGL(bump_counters_kernel, dim3(1), dim3(64), 0, s.st, c);
    GCMI_CHECK_LAUNCH("bump_counters");
  }
  return GCMI_OK;
}

// What both forward sequences start with: the accumulators zeroed once, the bias rows packed
static int begin_forward(Step& s, int32_t training) {
  s.training = training;
  s.stats = (s.bn() && training) ? s.acc : nullptr;
  if (training && s.bn() && s.N > 0)
    RUN(s.zero(s.ws + s.w.acc, sizeof(float) * (size_t)(s.w.z_end - s.w.acc), "model_forward"));
  return pack_biases(s);
}

// The task head's forward product: with more than 32 outputs on the prepared images (head_bwd.hip; the backward makes
// its own of the weights it is given); otherwise (and in the exact product mode) the segmented product.
static int head_forward(const Step& s) {
  const gcmi_model_desc* m = s.m;
  const int D = m->dense_width;
  const int TC = m->n_tasks * m->n_classes;
  const int32_t nB = (int32_t)s.B;
  const float* hw = s.d_params + m->off_head_w;
  const float* hb = s.d_params + m->off_head_b;
  if (s.w.himg >= 0 && s.B > 0) {
    int rc = head_prep(hw, TC, s.ws + s.w.himg, s.st);
    if (rc == GCMI_OK)
      rc = head_fwd_wide(s.io->d_fingerprint, 2 * D, s.B, 2 * D, hw, hb, TC, 0, s.io->d_logits, TC, s.st, s.ws + s.w.himg);
    if (rc != GCMI_ERR_UNSUPPORTED) return rc;
  }
  SegProduct<float> p = one_segment(&nB, s.io->d_fingerprint, 2 * D, 2 * D, hw, hb, TC, s.io->d_logits, TC);
  p.trans_w = 1;
  return seg_gemm(p, s.st);
}

// Everything behind the last GraphPool, for both storages: the dense product over its rows, BatchNorm, the readout,
// the task head, softmax and -- a training batch without atoms -- the counters
static int forward_tail(const Step& s) {
  const gcmi_model_desc* m = s.m;
  const Ws& w = s.w;
  const Block& dn = s.blk[s.L];
  const int D = dn.W;
  const bool h = s.storage != 0;
  bool stats_fused = h;  // (the bf16 product always leaves the sums; it has no rows for a pass over them)
  if (s.N > 0 && h) {
    TimedScope ts(GCMI_K_SEG_GEMM, s.st);
    SegProduct<bf16_t> p = one_segment(&s.nN, (const bf16_t*)s.H(w.pool[s.L - 1]), (int64_t)dn.K, dn.K, dn.w, dn.bias, D,
                                       s.H(w.dense), D);
    p.trans_w = 1;
    p.act = 1;
    const int rc = fwd_h_gemm(p, s.stats, s.ws + w.wimg, s.st);
    if (rc == GCMI_ERR_UNSUPPORTED) set_error("bf16 activation storage: the dense layer has no bf16 product kernel");
    RUN(rc);
  } else if (s.N > 0) {
    SegProduct<float> p = one_segment(&s.nN, s.HF(w.pool[s.L - 1]), (int64_t)dn.K, dn.K, dn.w, dn.bias, D, s.ws + w.dense, D);
    p.trans_w = 1;
    p.act = 1;
    RUN(seg_gemm_stats(p, s.stats, &stats_fused, s.st));
  }
  const bool bn = s.bn() && s.N > 0;
  if (bn || s.sy) RUN(bn_forward(s, dn, stats_fused, h ? nullptr : s.ws + w.dense, h ? 0 : D));
  RUN(readout_fwd_impl(s.g, s.HF(w.dense), D, D, bn ? dn.bn.scale : nullptr, bn ? dn.bn.shift : nullptr, 1,
                       s.io->d_fingerprint, 2 * D, reinterpret_cast<int32_t*>(s.ws + w.arg_r),
                       (s.training && s.bn()) ? s.ws + w.rsum : nullptr, s.st, h ? 1 : 0));
  RUN(head_forward(s));
  if (m->mode == 0 && s.io->d_probs) RUN(gcmi_softmax(s.io->d_logits, s.B * m->n_tasks, m->n_classes, s.io->d_probs, s.st));
  if (s.training && s.bn() && s.N == 0 && !s.sy) RUN(bump_counters(s));  // (sy: every exchange's finalisation did)
  return GCMI_OK;
}

// The first block's forward in its one-piece form (one_piece_block0 above): the window pass writes S0 and Xb as bf16
// rows, the product reads them as they are and leaves fp32 rows (and, training, the BatchNorm sums in acc)
static int one_piece_forward(const Step& s, const Segs& sg) {
  bf16_t* s0 = s.H(s.w.S[0]);
  bf16_t* xb = s.H(s.w.xb);
  {
    TimedScope ts(GCMI_K_GATHER_SUM, s.st);
    RUN(win_gather_sum_fh(s.g, s.io->d_atom_features, s.io->ld_features, 76, s0, xb, kOnePieceLd, s.st));
  }
  {
    TimedScope ts(GCMI_K_SEG_GEMM, s.st);
    const int rc = fwd_h_gemm(conv_product(sg, (const bf16_t*)s0, kOnePieceLd, (const bf16_t*)xb, kOnePieceLd, s.blk[0],
                                           s.ws + s.w.gc[0]),
                              s.stats, s.ws + s.w.wimg, s.st);
    if (rc == GCMI_ERR_UNSUPPORTED) set_error("model_forward: the one-piece product of GraphConv 0 refused its shape");
    RUN(rc);
  }
  g_one_piece_launches.fetch_add(1, std::memory_order_relaxed);
  return GCMI_OK;
}

// storage == 0: split-fp32 products (seg_gemm_stats picks the kernel), GraphPool and the next block's neighbour sums in
// one window pass; what a kernel does not cover falls back to the general one
static int model_forward_f(Step& s, int32_t training) {
  const gcmi_model_desc* m = s.m;
  const gcmi_graph* g = s.g;
  const Ws& w = s.w;
  float* ws = s.ws;
  const int64_t N = s.N;
  const bool one_piece = one_piece_block0(m, g, s.io);
  note_one_piece(ws, one_piece);
  RUN(begin_forward(s, training));
  const float* x = s.io->d_atom_features;
  int64_t ldx = s.io->ld_features;
  for (int l = 0; l < s.L; ++l) {
    const Block& b = s.blk[l];
    const int W = b.W;
    const Segs sg = make_segs(g, b.K, W);
    bool stats_fused = false;
    if (l == 0 && one_piece) {
      RUN(one_piece_forward(s, sg));
      stats_fused = training != 0;
    } else if (N > 0) {
      // (l > 0: the GraphPool of the block below left the neighbour sums of its output with it)
      if (l == 0) RUN(gcmi_gather_sum_fwd(g, x, ldx, (int32_t)w.ngather[l], ws + w.S[l], w.ldS[l], 0, s.st));
      RUN(seg_gemm_stats(conv_product(sg, s.HF(w.S[l]), w.ldS[l], x, ldx, b, ws + w.gc[l]), s.stats, &stats_fused, s.st,
                         ws + w.wimg));
    }
    const bool bn = s.bn() && N > 0;
    if (bn || s.sy) RUN(bn_forward(s, b, stats_fused, ws + w.gc[l], W));
    if (N > 0) {
      uint8_t* arg = training ? reinterpret_cast<uint8_t*>(ws + w.arg[l]) : nullptr;
      const float* sc = bn ? b.bn.scale : nullptr;
      const float* sh = bn ? b.bn.shift : nullptr;
      if (l + 1 < s.L)  // GraphPool and the neighbour sums of the block above in one window pass
        RUN(gcmi_gather_max_sum_fwd(g, ws + w.gc[l], W, W, sc, sh, ws + w.pool[l], W, arg, ws + w.S[l + 1], w.ldS[l + 1], s.st));
      else
        RUN(gcmi_gather_max_fwd(g, ws + w.gc[l], W, W, sc, sh, ws + w.pool[l], W, arg, s.st));
    }
    x = ws + w.pool[l];
    ldx = W;
  }
  return forward_tail(s);
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


static int model_forward_h(Step& s, int32_t training) {
  RUN(require_h(s.m, s.g, s.io, false));
  const gcmi_graph* g = s.g;
  const Ws& w = s.w;
  RUN(begin_forward(s, training));
  const bf16_t* xin = nullptr;
  int64_t ldin = 0;
  for (int l = 0; l < s.L; ++l) {
    const Block& b = s.blk[l];
    const Segs sg = make_segs(g, b.K, b.W);
    if (s.N > 0) {
      {
        TimedScope ts(GCMI_K_GATHER_SUM, s.st);
        if (l == 0) {  // fp32 atom features -> bf16 neighbour sums + a bf16 copy of the rows themselves
          RUN(win_gather_sum_fh(g, s.io->d_atom_features, s.io->ld_features, (int)w.ngather[0], s.H(w.S[0]), s.H(w.xb),
                                w.ldS[0], s.st));
          xin = s.H(w.xb);
          ldin = w.ldS[0];
        } else {
          RUN(win_gather_sum_h(g, xin, ldin, b.K, s.H(w.S[l]), w.ldS[l], s.st));
        }
      }
      {
        TimedScope ts(GCMI_K_SEG_GEMM, s.st);
        const int rc = fwd_h_gemm(conv_product(sg, (const bf16_t*)s.H(w.S[l]), w.ldS[l], xin, ldin, b, s.H(w.gc[l])),
                                  s.stats, s.ws + w.wimg, s.st);
        if (rc == GCMI_ERR_UNSUPPORTED) set_error("bf16 activation storage: GraphConv %d has no bf16 product kernel", l);
        RUN(rc);
      }
      RUN(bn_forward(s, b, true, nullptr, 0));
      {
        TimedScope ts(GCMI_K_GATHER_MAX, s.st);
        RUN(win_gather_max_h(g, s.H(w.gc[l]), b.W, b.W, b.bn.scale, b.bn.shift, s.H(w.pool[l]), b.W,
                             training ? reinterpret_cast<uint8_t*>(s.ws + w.arg[l]) : nullptr, s.st));
      }
    } else if (s.sy) {
      RUN(bn_forward(s, b, true, nullptr, 0));
    }
    xin = s.H(w.pool[l]);
    ldin = b.W;
  }
  return forward_tail(s);
}

// ------------------------------------------------------------------------------------------------------------------
// Loss + backward.  One walk over the blocks for both storages: the per-molecule head part, the dense block, then
// GraphConv / BatchNorm / GraphPool last to first.  Each block takes the route block_route picks for it; bf16 storage
// has one route, and a kernel of it that refuses is an error where fp32 storage falls back.

// What the backward starts with: the range of the gradient arena it writes, zeroed; [dlogits (rows beyond n_rows carry
// no gradient) | the bias-gradient sums | every accumulator] zeroed; the readout gradient's description
static int begin_backward(Step& s) {
  const gcmi_model_desc* m = s.m;
  s.loss_inv_count = 1.f / (float)(s.n_rows * m->n_tasks);
  s.one_piece = s.storage == 0 && noted_one_piece(s.ws);
  const int64_t lo = s.full ? 0 : (s.bn() ? m->off_bn_gamma[s.L - 1] : m->off_dense_w);
  const int64_t hi = m->n_params;
  if (s.grad_lo) *s.grad_lo = lo;
  if (s.grad_hi) *s.grad_hi = hi;
  RUN(s.zero(s.d_grads + lo, sizeof(float) * (size_t)(hi - lo), "model_loss_backward"));
  RUN(s.zero(s.ws + s.w.dlogits, sizeof(float) * (size_t)(s.w.z_end - s.w.dlogits), "model_loss_backward"));
  const int D = m->dense_width;
  s.rg = ReadoutGrad{s.g->d_membership, s.ws + s.w.dfp, 2 * (int64_t)D, reinterpret_cast<const int32_t*>(s.ws + s.w.arg_r)};
  s.rg.rawsum = s.ws + s.w.rsum; s.rg.runs = s.g->d_mol_runs; s.rg.n_mols = s.g->n_mols; s.rg.n_deg = s.g->max_deg + 1;
  return GCMI_OK;
}

// The backward of a rank whose batch has no atoms: no BatchNorm kernel runs, but the other ranks wait in the exchange
// of every BatchNorm point their backward computes (the dense block's, then the GraphConv blocks' last to first;
// reference gradient mode stops behind the last GraphConv block)
static int empty_backward_syncs(const Step& s) {
  for (int l = s.L; l >= 0; --l) {
    RUN(bn_bwd_sync_empty(s.blk[l].W, *s.sy, s.st));
    if (!s.full && l < s.L) break;
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


// A BatchNorm backward over the N rows of x on the step's accumulator (zeroed once per call, self-cleaning afterwards);
// the caller names the gradient source and what else it wants
static BnBackward bn_backward(const Step& s, const float* x, int64_t ldx, const BnSync* sy) {
  BnBackward q;
  q.x = x; q.ldx = ldx; q.n_rows = s.N; q.acc = s.acc; q.acc_clean = true; q.sync = sy;
  return q;
}

// ---- the per-molecule part (fp32 in every storage: the fingerprint and everything behind it are per-molecule rows)
// In one kernel where the shapes allow (head_bwd.hip): loss, d logits, head gradients, the gradient w.r.t.
// GraphGather's pre-activation in rg.g2, and -- sums given: the one-pass dense block follows -- the backward sums of
// the dense layer's BatchNorm.  *done = false: shape not covered, nothing launched.  *with_sums: the sums are in
// place, and the loss is finalised by the BatchNorm parameter launch that follows.
static int head_backward_fused(const Step& s, double* sums, bool* done, bool* with_sums) {
  const gcmi_model_desc* m = s.m;
  const BnPoint& dense_bn = s.blk[s.L].bn;
  HeadBackward h;
  h.kind = m->mode == 0 ? 0 : 1; h.logits = s.io->d_logits; h.labels = s.d_labels; h.weights = s.d_weights;
  h.n_rows = s.n_rows; h.n_tasks = m->n_tasks; h.n_classes = m->n_classes;
  h.fp = s.io->d_fingerprint; h.ldfp = 2 * dense_bn.n_feat;
  h.w = s.d_params + m->off_head_w; h.dw = s.d_grads + m->off_head_w; h.db = s.d_grads + m->off_head_b;
  h.rg = &s.rg; h.g2 = s.ws + s.w.dfp; h.loss_acc = s.lacc; h.dense_bn = &dense_bn; h.sums = sums;
  h.dl_scratch = s.ws + s.w.dlogits; h.img = s.w.himg >= 0 ? s.ws + s.w.himg : nullptr;
  *done = *with_sums = false;
  const int rc = head_bwd_fused(h, s.st);
  if (rc == GCMI_ERR_UNSUPPORTED) return GCMI_OK;
  RUN(rc);
  *done = true;
  *with_sums = sums != nullptr;
  if (!*with_sums) RUN(loss_finalize_impl(s.lacc, s.loss_inv_count, s.io->d_loss, s.st, kLossRep));
  return GCMI_OK;
}

// ... as separate launches (the shapes head_bwd_fused does not cover): loss and d logits of the first n_rows
// molecules, the head's gradients, the gradient w.r.t. the fingerprint in dfp; prep: the tanh derivative applied to it
// in place, for a BatchNorm backward that recomputes the GraphGather backward from it
static int head_backward_separate(const Step& s, bool prep) {
  const gcmi_model_desc* m = s.m;
  const Ws& w = s.w;
  float* ws = s.ws;
  const int D = m->dense_width;
  const int TC = m->n_tasks * m->n_classes;
  const int32_t nB = (int32_t)s.B;
  RUN(loss_impl(m->mode == 0 ? 0 : 1, s.io->d_logits, s.d_labels, s.d_weights, s.n_rows, m->n_tasks, m->n_classes,
                s.io->d_loss, ws + w.dlogits, nullptr, s.lacc, true, s.st));
  RUN(gcmi_seg_gemm_wgrad(1, &kZero32, &nB, s.io->d_fingerprint, 2 * D, 2 * D, ws + w.dlogits, TC, TC,
                          s.d_grads + m->off_head_w, &kZero64, s.d_grads + m->off_head_b, &kZero64, 1, s.st));
  RUN(seg_gemm(one_segment(&nB, s.HF(w.dlogits), TC, TC, s.d_params + m->off_head_w, nullptr, 2 * D, ws + w.dfp, 2 * D), s.st));
  if (prep) RUN(readout_grad_prep(ws + w.dfp, 2 * D, s.io->d_fingerprint, 2 * D, s.B, D, s.st));
  return GCMI_OK;
}

// the dense block's backward takes the one-pass kernel (bwd_fused.hip: fused_dense_bwd) -- asked once per call: the
// head kernel in front of it leaves the BatchNorm sums only for that kernel
// (bf16 storage: true whenever there are atoms -- check_desc and require_h leave no other shape)
static bool dense_block_one_pass(const gcmi_model_desc* m, int64_t N) {
  const int Wl = m->conv_width[m->n_layers - 1];
  return m->batch_norm && N > 0 && fused_bwd_enabled() && m->dense_width == 128 && Wl > 32 && Wl <= 64;
}

// *head_sums: the dense BatchNorm's backward sums are in acc
static int head_backward(const Step& s, bool dense_one_pass, bool* head_sums) {
  bool done = false;
  *head_sums = false;
  if (s.bn())  // (without BatchNorm the readout backward applies the tanh derivative itself)
    RUN(head_backward_fused(s, (dense_one_pass && s.g->d_mol_runs) ? s.acc : nullptr, &done, head_sums));
  // (the tanh derivative applied in place only for the BatchNorm backward that follows; bf16 storage: always)
  if (!done) RUN(head_backward_separate(s, s.storage != 0 || (s.bn() && s.N > 0)));
  return GCMI_OK;
}

// ---- the dense block
// Its BatchNorm's parameters (dgamma, dbeta, the coefficient vectors): from the sums the head kernel left in place
// (which also finalises the loss), else with the GraphGather backward recomputed from the per-molecule gradient -- the
// N x D gradient is never written or re-read.  dx: also the gradient w.r.t. the dense pre-activation (separate route).
static int dense_bn_backward(const Step& s, bool head_sums, float* dx, const BnSync* sy) {
  const Block& dn = s.blk[s.L];
  // (per-molecule sums read rawsum, never the atom rows: a bf16 matrix is only passed through)
  BnBackward q = bn_backward(s, s.HF(s.w.dense), dn.W, sy);
  if (head_sums) {
    q.loss = {s.lacc, kLossRep, s.loss_inv_count, s.io->d_loss};
    return bn_bwd_params_impl(dn.bn, q, s.st);
  }
  q.rg = &s.rg; q.dx = dx; q.lddx = dn.W; q.relu_mask = 1;
  return bn_bwd_impl(dn.bn, q, s.st);
}

// The dense block in one pass (fused_dense_bwd): G from the readout gradient, the block's output `dense` and coef;
// dW, db; dpool = G W, and in acc2 the pooled sums for the BatchNorm below.
static BlockBackward dense_backward(const Step& s) {
  const Block& dn = s.blk[s.L];
  BlockBackward q;
  q.n_seg = 1; q.seg_begin = &kZero32; q.seg_end = &s.nN; q.w_off[0] = &kZero64; q.b_off = &kZero64;
  q.rg = &s.rg; q.gc = s.HF(s.w.dense); q.ldgc = dn.W; q.coef = s.coef(); q.width = dn.W;
  q.in[0] = {s.HF(s.w.pool[s.L - 1]), dn.K}; q.k_in = dn.K; q.w = dn.w; q.dw = dn.dw; q.db = dn.dbias;
  q.dout[0] = {s.dpool(), dn.K}; q.psums = s.acc2;
  q.act_bf16 = s.storage;
  return q;
}

// BatchNorm parameters, then dW, db and dpool: in one pass over the rows (dxD formed per 64-row tile in LDS) where
// dense_one_pass says so, else as separate launches.  *have_psums: acc2 holds sum dP, sum dP * P for the BatchNorm of
// the last GraphConv block.
static int dense_block_backward(const Step& s, bool dense_one_pass, bool head_sums, bool* have_psums) {
  const Ws& w = s.w;
  float* ws = s.ws;
  const Block& dn = s.blk[s.L];
  const int D = dn.W, Wl = dn.K;
  float* dxD = ws + w.tB;  // grad w.r.t. the dense pre-activation
  *have_psums = false;
  if (s.bn()) {
    RUN(dense_bn_backward(s, head_sums, dense_one_pass ? nullptr : dxD, s.sy));
    if (dense_one_pass) {
      int rc;
      {
        TimedScope ts(GCMI_K_FUSED_BWD, s.st);
        rc = fused_dense_bwd(dense_backward(s), s.st);
      }
      *have_psums = rc == GCMI_OK;
      if (rc != GCMI_ERR_UNSUPPORTED) return rc;
      if (s.storage != 0) {
        set_error("bf16 activation storage: the dense block has no one-pass backward");
        return rc;
      }
      if (s.sy) return refuse_second_sync("the one-pass dense block");
      // not covered after all (misaligned buffers): the separate pass, with its sums once more
      RUN(dense_bn_backward(s, false, dxD, nullptr));
    }
  } else {
    dxD = ws + w.tA;  // grad w.r.t. the readout input, then the ReLU mask in place
    RUN(gcmi_readout_bwd(s.g, ws + w.dfp, 2 * D, s.io->d_fingerprint, 2 * D, D, 1, s.rg.arg, dxD, D, s.st));
    RUN(gcmi_relu_bwd(dxD, D, ws + w.dense, D, s.N, D, s.st));
  }
  RUN(gcmi_seg_gemm_wgrad(1, &kZero32, &s.nN, ws + w.pool[s.L - 1], Wl, Wl, dxD, D, D, dn.dw, &kZero64, dn.dbias, &kZero64,
                          1, s.st));
  return seg_gemm(one_segment(&s.nN, (const float*)dxD, D, D, dn.w, nullptr, Wl, s.dpool(), Wl), s.st);
}

// ---- a GraphConv / BatchNorm / GraphPool block
// The rows block l's GraphConv read: S and X with their leading dimensions, in the form the forward left them
// (one-piece form of the first block: S0 and the copy Xb of the atom features are bf16 rows)
struct BlockIn {
  const float* x;
  int64_t ldx, ldS;
};
static BlockIn block_in(const Step& s, int l) {
  if (l > 0) return {s.HF(s.w.pool[l - 1]), s.m->conv_width[l - 1], s.w.ldS[l]};
  if (s.storage != 0) return {s.HF(s.w.xb), s.w.ldS[0], s.w.ldS[0]};
  if (s.one_piece) return {s.HF(s.w.xb), kOnePieceLd, kOnePieceLd};
  return {s.io->d_atom_features, s.io->ld_features, s.w.ldS[0]};
}

// The route block l's backward takes, decided once, before its first launch.
struct BlockRoute {
  bool one_pass;     // dW_rel, dW_self, dbsum (and for l > 0 dS and the self part of dX) in one pass over the rows
                     // (bwd_fused.hip); else the separate launches
  bool pooled_sums;  // its BatchNorm's backward sums from the pooled sums the block above left in acc2; else from a
                     // pass over dy
  bool two_stage;    // after the one pass: the neighbour part and the GraphPool backward of the block below in one
                     // window pass (dX in LDS only); else the accumulating gather, without reverse slots the scatter
  bool one_piece;    // the first block on the bf16 rows its one-piece forward left
};
// have_psums: the block above ran in one pass and left the pooled sums
static BlockRoute block_route(const Step& s, int l, const BlockIn& in, bool have_psums) {
  const gcmi_graph* g = s.g;
  const int W = s.blk[l].W, K = s.blk[l].K;
  BlockRoute r;
  r.one_piece = l == 0 && s.one_piece;
  if (s.storage != 0) {  // the one route of bf16 storage (require_h); a kernel that refuses ends the call
    r.one_pass = s.full;
    r.pooled_sums = true;
  } else {
    // the one pass covers the default widths in split-bf16 mode; it wants 16-byte rows of every operand
    r.one_pass = s.full && fused_bwd_enabled() && W == 64 && in.ldx % 4 == 0 && aligned16(in.x) &&
                 ((l == 0 && K > 32 && K <= 96) || (l > 0 && K > 32 && K <= 64));
    r.pooled_sums = have_psums && s.bn() && s.sym && (r.one_pass || !s.full) && win_usable(g, W, true) && win_has_width(W);
  }
  // ... when the window kernels can hold a third tile
  r.two_stage = r.one_pass && l > 0 &&
                (s.storage == 2 ? win_two_stage_usable_h(g, K)
                                : s.sym && fused_bwd_enabled() && win_two_stage_usable(g, K) && aligned16(s.dS()) &&
                                      aligned16(s.dX()) && aligned16(s.dy()));
  return r;
}

// dgc, the gradient w.r.t. block l's pre-activation, written out in rows (what the one pass forms per tile): with
// BatchNorm by its backward over dy, which also leaves dgamma, dbeta and coef and runs for those alone when dgc is not
// wanted; without, the ReLU mask on dy in place
static int bn_relu_backward_rows(const Step& s, int l, bool want_dgc, const BnSync* sy) {
  const Block& b = s.blk[l];
  if (s.bn()) {
    BnBackward q = bn_backward(s, s.ws + s.w.gc[l], b.W, sy);
    q.dy = s.dy(); q.lddy = b.W; q.dx = want_dgc ? s.dgc() : nullptr; q.lddx = b.W; q.relu_mask = 1;
    return bn_bwd_impl(b.bn, q, s.st);
  }
  return want_dgc ? gcmi_relu_bwd(s.dy(), b.W, s.ws + s.w.gc[l], b.W, s.N, b.W, s.st) : GCMI_OK;
}

// GraphPool backward of block l (dpool -> dy) and its BatchNorm backward.  Pooled sums: the block above left sum dP
// and sum dP * P, so this BatchNorm's backward needs no pass over dy (bn.hip, bn_bwd_pool_impl); dy itself is needed
// when the GraphConv below trains, otherwise only by the ill-conditioned fallback, and those kernels return at once
// unless that applies.  dy_ready: the two-stage pass of the block above already left dy.
static int pool_bn_backward(const Step& s, int l, const BlockRoute& r, bool dy_ready) {
  const gcmi_graph* g = s.g;
  const Block& b = s.blk[l];
  const int W = b.W;
  float* dy = s.dy();
  if (!s.sym) RUN(s.zero(dy, sizeof(float) * (size_t)(s.N * W), "model_loss_backward"));  // (the atomic form adds)
  if (!r.pooled_sums) {
    if (!dy_ready) RUN(gcmi_gather_max_bwd(g, s.dpool(), W, W, s.arg(l), dy, W, s.st));
    return bn_relu_backward_rows(s, l, s.full && !r.one_pass, s.sy);
  }
  if (dy_ready) {
  } else if (s.storage == 2) {
    TimedScope ts(GCMI_K_GATHER_MAX_BWD, s.st);
    RUN(win_gather_max_bwd_h(g, s.HG(s.dpool()), W, W, s.arg(l), s.HG(dy), W, s.full ? nullptr : b.bn.gamma,
                             s.full ? nullptr : b.bn.beta, s.st));
  } else if (s.full) {
    RUN(gcmi_gather_max_bwd(g, s.dpool(), W, W, s.arg(l), dy, W, s.st));
  } else {
    TimedScope ts(GCMI_K_GATHER_MAX_BWD, s.st);
    RUN(win_gather_max_bwd_if_ill(g, s.dpool(), W, W, s.arg(l), dy, W, b.bn.gamma, b.bn.beta, s.st));
  }
  BnBackward q = bn_backward(s, s.HF(s.w.gc[l]), W, s.sy);
  q.dy = dy; q.lddy = W; q.x_bf16 = s.storage; q.psums = s.acc2;
  return bn_bwd_pool_impl(b.bn, q, s.st);
}

// Block l in one pass (fused_conv_bwd): G from dy, the block's output gc and coef, formed per tile in LDS; dW_rel,
// dW_self, dbsum over [S | X]; for l > 0 dS = G W_rel^T, the self part of dX and the pooled sums for the BatchNorm
// below.  *done = false: the kernel refused its buffers after all (misaligned ones) and the separate pass has left dgc
// in rows, its sums taken once more -- which bf16 storage and synchronised BatchNorm refuse.
static int conv_one_pass(const Step& s, int l, const Segs& sg, const BlockIn& in, const BlockRoute& r, bool* done) {
  const Block& b = s.blk[l];
  int rc;
  {
    TimedScope ts(GCMI_K_FUSED_BWD, s.st);
    BlockBackward q;
    q.n_seg = sg.n; q.seg_begin = sg.begin; q.seg_end = sg.end; q.w_off[0] = sg.w_rel; q.w_off[1] = sg.w_self; q.b_off = sg.b_off;
    q.dy = s.dy(); q.lddy = b.W; q.gc = s.HF(s.w.gc[l]); q.ldgc = b.W; q.coef = s.bn() ? s.coef() : nullptr; q.width = b.W;
    q.in[0] = {s.HF(s.w.S[l]), in.ldS}; q.in[1] = {in.x, in.ldx}; q.k_in = b.K; q.w = b.w; q.dw = b.dw; q.db = b.dbias;
    q.dout[0].ld = q.dout[1].ld = b.K;
    q.act_bf16 = s.storage;
    q.in_bf16 = r.one_piece ? 1 : 0;
    if (l > 0) { q.dout[0].rows = s.dS(); q.dout[1].rows = s.dX(); q.psums = (s.sym && s.bn()) ? s.acc2 : nullptr; }
    rc = fused_conv_bwd(q, s.st);
  }
  *done = rc == GCMI_OK;
  if (*done && r.one_piece) g_one_piece_launches.fetch_add(1, std::memory_order_relaxed);
  if (rc != GCMI_ERR_UNSUPPORTED) return rc;
  if (s.storage != 0) {
    set_error("bf16 activation storage: GraphConv %d has no one-pass backward", l);
    return rc;
  }
  if (s.sy) return refuse_second_sync("the one-pass GraphConv block");
  return bn_relu_backward_rows(s, l, true, nullptr);
}

// After the one pass dX holds the self part: the neighbour part is added onto it (bonds listed from both ends: the
// scatter of dS is a gather), and on the two-stage route the GraphPool backward of the block below runs in the same
// pass -- dX = dXs + gather(dS) is consumed in LDS and never exists in HBM (*dy_ready: that block's dy is in place)
static int neighbour_part(const Step& s, int l, const BlockRoute& r, bool* dy_ready) {
  const gcmi_graph* g = s.g;
  const int K = s.blk[l].K;
  float *dS = s.dS(), *dX = s.dX();
  *dy_ready = r.two_stage;
  if (r.two_stage) {
    TimedScope ts(GCMI_K_GATHER_MAX_BWD, s.st);
    if (s.storage == 2) return win_gather_sumacc_max_bwd_h(g, s.HG(dS), K, K, s.HG(dX), K, s.arg(l - 1), s.HG(s.dy()), K, s.st);
    return win_gather_sumacc_max_bwd(g, dS, K, K, dX, K, s.arg(l - 1), s.dy(), K, s.st);
  }
  if (s.storage == 2) {
    set_error("bf16 gradient streams: no LDS for the two-stage window pass");
    return GCMI_ERR_UNSUPPORTED;
  }
  if (s.sym) return gcmi_gather_sum_fwd(g, dS, K, K, dX, K, 1, s.st);
  return gcmi_scatter_add(g, dS, K, K, dX, K, s.st);
}

// Block l as separate launches over dgc in rows: dW_rel += S^T dgc; dW_self += X^T dgc and dbsum; for l > 0
// dS = dgc . W_rel[d]^T and dX = dgc . W_self[d]^T + (transposed gather of dS)
static int conv_separate(const Step& s, int l, const Segs& sg, const BlockIn& in) {
  const gcmi_graph* g = s.g;
  const Block& b = s.blk[l];
  const int W = b.W, K = b.K;
  float *dgc = s.dgc(), *dS = s.dS(), *dX = s.dX();
  RUN(gcmi_seg_gemm_wgrad(sg.n, sg.begin, sg.end, s.ws + s.w.S[l], s.w.ldS[l], K, dgc, W, W, b.dw, sg.w_rel, nullptr, nullptr,
                          0, s.st));
  RUN(gcmi_seg_gemm_wgrad(sg.n, sg.begin, sg.end, in.x, in.ldx, K, dgc, W, W, b.dw, sg.w_self, b.dbias, sg.b_off, 0, s.st));
  if (l == 0) return GCMI_OK;  // the atom features need no gradient
  SegProduct<float> dg = seg_product(sg, (const float*)dgc, W, W, b.w, sg.w_rel, K, dS);
  dg.trans_w = 1;
  RUN(seg_gemm(dg, s.st));
  // bonds listed from both ends: the scatter of dS is a gather (LDS-window kernel), and the self term accumulates
  // onto it in the GEMM epilogue
  if (s.sym) RUN(gcmi_gather_sum_fwd(g, dS, K, K, dX, K, 0, s.st));
  dg.op[0].w_off = sg.w_self;  // dX (+)= dgc . W_self[d]^T
  dg.act = s.sym ? 2 : 0;
  dg.out = dX;
  RUN(seg_gemm(dg, s.st));
  if (!s.sym) RUN(gcmi_scatter_add(g, dS, K, K, dX, K, s.st));
  return GCMI_OK;
}

static int model_loss_backward_f(Step& s) {
  RUN(begin_backward(s));
  const bool dense_one_pass = dense_block_one_pass(s.m, s.N);
  bool head_sums = false;
  RUN(head_backward(s, dense_one_pass, &head_sums));
  if (s.N == 0) return s.sy ? empty_backward_syncs(s) : GCMI_OK;
  bool have_psums = false;  // acc2 holds sum dP, sum dP * P for the BatchNorm below the block just processed
  bool dy_ready = false;    // the two-stage pass of the block above already left this block's dy
  RUN(dense_block_backward(s, dense_one_pass, head_sums, &have_psums));
  for (int l = s.L - 1; l >= 0; --l) {
    if (!s.full && !s.bn()) break;  // nothing trainable in front of the dense layer
    const Block& b = s.blk[l];
    const Segs sg = make_segs(s.g, b.K, b.W);
    const BlockIn in = block_in(s, l);
    const BlockRoute r = block_route(s, l, in, have_psums);
    RUN(pool_bn_backward(s, l, r, dy_ready));
    have_psums = dy_ready = false;
    if (!s.full) break;  // reference semantics: nothing in front of a GraphConv output trains
    bool one_pass_done = false;
    if (r.one_pass) RUN(conv_one_pass(s, l, sg, in, r, &one_pass_done));
    if (!one_pass_done && r.one_piece) {  // (the one-pass backward was switched off between the forward and this call)
      set_error("model_loss_backward: the forward left the first block's operands as bf16 rows, and the one-pass "
                "backward that reads them is not available now (GCMI_OPT_FUSED_BWD / GCMI_OPT_GEMM_EXACT changed?)");
      return GCMI_ERR_UNSUPPORTED;
    }
    if (!one_pass_done) RUN(conv_separate(s, l, sg, in));
    else if (l > 0) RUN(neighbour_part(s, l, r, &dy_ready));
    have_psums = one_pass_done && l > 0 && s.sym && s.bn();
    s.ub.src[l] = b.dbias; s.ub.dst[l] = b.dbias_rows; s.ub.width[l] = b.W;  // unpacked in one launch below
  }
  return unpack_bias_grads(s);
}

// bf16 storage: the same walk; what its kernels do not cover is refused up front
static int model_loss_backward_h(Step& s) {
  RUN(require_h(s.m, s.g, s.io, true));
  return model_loss_backward_f(s);
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
  Step s;
  make_step(s, m, g, d_params, nullptr, io, sync, sync_ctx, sync && training, stream);
  return m->storage >= 1 ? model_forward_h(s, training) : model_forward_f(s, training);
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
  Step s;
  make_step(s, m, g, d_params, d_grads, io, sync, sync_ctx, sync != nullptr, stream);
  s.d_labels = d_labels; s.d_weights = d_weights; s.n_rows = n_rows; s.grad_lo = grad_lo; s.grad_hi = grad_hi;
  return m->storage >= 1 ? model_loss_backward_h(s) : model_loss_backward_f(s);
}

}  // extern "C"
