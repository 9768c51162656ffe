// Optimizer steps on flat arenas.
//   gcmi_opt_step: the elementwise rules (SGD, Adagrad, RMSprop, Adam with L2, AdamW) of optim_rules.h, one launch
//     over a flat float range: 16-byte loads and stores, a scalar tail, grid-stride, no atomics.
//   gcmi_lamb_step: LambOptimizer (utils/optimizer_utils.py:91-163; debias=False, adam=False, clamp 10) over a
//     segment table, two launches.  Pass 1 updates the moments, leaves the update u = m / (sqrt(v) + eps) + wd p in
//     a scratch arena and one fp64 pair (sum p^2, sum u^2) per fixed chunk of a segment; pass 2 sums the pairs of its
//     segment in index order, forms the trust ratio and applies p -= lr * trust * u.  No floating-point atomics: the
//     reduction tree is fixed by the table alone, so equal inputs give equal bits on every run and every rank.
// All launch-bound at the sizes trained here (15 k - 204 k floats): few launches, plain tiling.
#include <math.h>

#include <type_traits>

#include "optim_rules.h"

namespace gcmi {

constexpr int kOBlock = 256;
constexpr int kOMaxBlocks = 1024;  // beyond 1 Mi floats the elementwise kernel strides
constexpr int kLambChunk = 1024;   // floats of a segment per workgroup: 4 per thread

template <int R>
__global__ void __launch_bounds__(kOBlock)
opt_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1, float* __restrict__ s2,
                int64_t n4, int64_t n, OptConsts k) {
  constexpr int kStates = R == kRuleSGD ? 0 : (R == kRuleAdagrad || R == kRuleRMSprop) ? 1 : 2;
  const int64_t stride = (int64_t)gridDim.x * kOBlock;
  const int64_t t0 = (int64_t)blockIdx.x * kOBlock + threadIdx.x;
  for (int64_t i = t0; i < n4; i += stride) {
    const int64_t o = 4 * i;
    float4 pv = *reinterpret_cast<const float4*>(p + o);
    const float4 gv = *reinterpret_cast<const float4*>(g + o);
    float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
    if constexpr (kStates >= 1) av = *reinterpret_cast<const float4*>(s1 + o);
    if constexpr (kStates >= 2) bv = *reinterpret_cast<const float4*>(s2 + o);
    float* pf = reinterpret_cast<float*>(&pv);
    const float* gf = reinterpret_cast<const float*>(&gv);
    float* af = reinterpret_cast<float*>(&av);
    float* bf = reinterpret_cast<float*>(&bv);
#pragma unroll
    for (int c = 0; c < 4; ++c) opt_update<R>(pf[c], gf[c], af[c], bf[c], k);
    if constexpr (kStates >= 1) *reinterpret_cast<float4*>(s1 + o) = av;
    if constexpr (kStates >= 2) *reinterpret_cast<float4*>(s2 + o) = bv;
    *reinterpret_cast<float4*>(p + o) = pv;
  }
  // the floats behind the last whole vector (all of them when a pointer is not 16-byte aligned: n4 == 0)
  for (int64_t i = 4 * n4 + t0; i < n; i += stride) {
    float pi = p[i], a = 0.f, b = 0.f;
    if constexpr (kStates >= 1) a = s1[i];
    if constexpr (kStates >= 2) b = s2[i];
    opt_update<R>(pi, g[i], a, b, k);
    if constexpr (kStates >= 1) s1[i] = a;
    if constexpr (kStates >= 2) s2[i] = b;
    p[i] = pi;
  }
}

// ---------------------------------------------------------------------------------------------------------- Lamb
// sum over the workgroup of (a, b), fixed tree: 64-lane shuffle halving, then the waves in order.  Valid on every thread.
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_down(a, o);
    b += __shfl_down(b, o);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();  // (red may still be read from an earlier call)
  if (lane == 0) {
    red[2 * wave] = a;
    red[2 * wave + 1] = b;
  }
  __syncthreads();
  a = 0.0;
  b = 0.0;
  for (int w = 0; w < kOBlock / 64; ++w) {
    a += red[2 * w];
    b += red[2 * w + 1];
  }
}

// Which (segment, chunk of it) workgroup `blk` owns: the chunks of the segments in table order.  A segment that does
// not lie inside [0, n) counts as empty (nothing outside the arenas is ever touched).  False: no chunk for this workgroup.
struct LambWork {
  int seg;
  int64_t off, cnt;     // the segment
  int64_t chunk;        // this workgroup's chunk of it
  int64_t first_chunk;  // global index of the segment's first chunk
  int64_t n_chunks;     // chunks of the segment
};
__device__ __forceinline__ bool lamb_find(const int64_t* __restrict__ segs, int n_seg, int64_t n, int64_t blk, LambWork* w) {
  int64_t cum = 0;
  for (int s = 0; s < n_seg; ++s) {
    const int64_t off = segs[2 * s];
    int64_t cnt = segs[2 * s + 1];
    if (off < 0 || cnt < 0 || off > n || cnt > n - off) cnt = 0;
    const int64_t nch = (cnt + kLambChunk - 1) / kLambChunk;
    if (blk < cum + nch) {
      w->seg = s;
      w->off = off;
      w->cnt = cnt;
      w->chunk = blk - cum;
      w->first_chunk = cum;
      w->n_chunks = nch;
      return true;
    }
    cum += nch;
  }
  return false;
}

__global__ void __launch_bounds__(kOBlock)
lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                    float* __restrict__ u, double* __restrict__ partial, const int64_t* __restrict__ segs, int n_seg,
                    int64_t n, float b1, float one_minus_b1, float b2, float one_minus_b2, float eps, float wd) {
  __shared__ double red[2 * kOBlock / 64];
  LambWork w;
  if (!lamb_find(segs, n_seg, n, blockIdx.x, &w)) return;  // uniform over the workgroup
  const int64_t end = w.off + w.cnt;
  double sp = 0.0, su = 0.0;
#pragma unroll
  for (int j = 0; j < kLambChunk / kOBlock; ++j) {
    const int64_t i = w.off + w.chunk * kLambChunk + j * kOBlock + threadIdx.x;
    if (i < end) {
      const float gi = g[i], pi = p[i];
      const float mi = m[i] * b1 + gi * one_minus_b1;       // exp_avg.mul_(beta1).add_(grad, alpha=1-beta1)
      const float vi = v[i] * b2 + gi * gi * one_minus_b2;  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
      m[i] = mi;
      v[i] = vi;
      float ui = mi / (sqrtf(vi) + eps);  // exp_avg / exp_avg_sq.sqrt().add(eps)
      if (wd != 0.f) ui = ui + wd * pi;   // adam_step.add_(p, alpha=weight_decay)
      u[i] = ui;
      sp += (double)pi * (double)pi;
      su += (double)ui * (double)ui;
    }
  }
  block_sum2(sp, su, red);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = sp;
    partial[2 * blockIdx.x + 1] = su;
  }
}

__global__ void __launch_bounds__(kOBlock)
lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ u, const double* __restrict__ partial,
                  const int64_t* __restrict__ segs, int n_seg, int64_t n, float lr, float clamp,
                  float* __restrict__ norms) {
  __shared__ double red[2 * kOBlock / 64];
  LambWork w;
  if (!lamb_find(segs, n_seg, n, blockIdx.x, &w)) return;
  // every workgroup of a segment sums that segment's pairs the same way: strided by thread in index order, then the tree
  double sp = 0.0, su = 0.0;
  for (int64_t j = threadIdx.x; j < w.n_chunks; j += kOBlock) {
    sp += partial[2 * (w.first_chunk + j)];
    su += partial[2 * (w.first_chunk + j) + 1];
  }
  block_sum2(sp, su, red);
  // weight_norm = torch.norm(p).clamp(0, clamp_value); trust_ratio = 1 where either norm is 0
  const float wn = fminf(fmaxf((float)sqrt(sp), 0.f), clamp);
  const float an = (float)sqrt(su);
  const float trust = (wn == 0.f || an == 0.f) ? 1.f : wn / an;
  if (w.chunk == 0 && threadIdx.x == 0 && norms) {
    norms[3 * w.seg] = wn;
    norms[3 * w.seg + 1] = an;
    norms[3 * w.seg + 2] = trust;
  }
  const float scale = lr * trust;
  const int64_t end = w.off + w.cnt;
#pragma unroll
  for (int j = 0; j < kLambChunk / kOBlock; ++j) {
    const int64_t i = w.off + w.chunk * kLambChunk + j * kOBlock + threadIdx.x;
    if (i < end) p[i] -= scale * u[i];  // p.add_(adam_step, alpha=-step_size * trust_ratio)
  }
}

static inline int64_t lamb_max_chunks(int64_t n, int64_t n_seg) { return (n + kLambChunk - 1) / kLambChunk + n_seg; }

int opt_consts(const gcmi_opt_desc* d, float lr, int64_t step, OptConsts* out, int* rule) {
  GCMI_CHECK_ARG(d != nullptr, "opt: NULL description");
  GCMI_CHECK_ARG(d->rule >= GCMI_RULE_SGD && d->rule <= GCMI_RULE_ADAMW, "opt: rule %d is not an elementwise rule", d->rule);
  GCMI_CHECK_ARG(step >= 1, "opt: step must be >= 1 (the count after this update)");
  memset(out, 0, sizeof(*out));
  out->lr = lr;
  out->eps = d->eps;
  int r = d->rule;
  if (r == GCMI_RULE_RMSPROP) {
    out->alpha = d->alpha;
    out->one_minus_alpha = 1.f - d->alpha;
    out->momentum = d->momentum;
    if (d->momentum != 0.f) r = kRuleRMSpropMom;
  } else if (r == GCMI_RULE_ADAM_L2 || r == GCMI_RULE_ADAMW) {
    GCMI_CHECK_ARG(d->beta1 >= 0.f && d->beta1 < 1.f && d->beta2 >= 0.f && d->beta2 < 1.f, "opt: betas must lie in [0, 1)");
    const double bc1 = 1.0 - pow((double)d->beta1, (double)step);
    const double bc2 = 1.0 - pow((double)d->beta2, (double)step);
    out->one_minus_b1 = 1.f - d->beta1;
    out->b2 = d->beta2;
    out->one_minus_b2 = 1.f - d->beta2;
    out->step_size = (float)((double)lr / bc1);
    out->inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    if (r == GCMI_RULE_ADAMW)
      out->wd = (float)(1.0 - (double)lr * (double)d->weight_decay);
    else if (d->weight_decay != 0.f)
      out->wd = d->weight_decay;
    else
      r = kRuleAdam;
  }
  *rule = r;
  return GCMI_OK;
}

}  // namespace gcmi

using namespace gcmi;

extern "C" {

int gcmi_opt_step(const gcmi_opt_desc* desc, float* d_param, const float* d_grad, float* d_state1, float* d_state2,
                  int64_t n, float lr, int64_t step, void* stream) {
  OptConsts k;
  int rule = 0;
  const int rc = opt_consts(desc, lr, step, &k, &rule);
  if (rc != GCMI_OK) return rc;
  GCMI_CHECK_ARG(n >= 0, "opt: bad n");
  if (n == 0) return GCMI_OK;
  const int n_states = opt_rule_states(rule);
  GCMI_CHECK_ARG(d_param && d_grad && (n_states < 1 || d_state1) && (n_states < 2 || d_state2), "opt: NULL buffer");
  // Adam without weight decay is gcmi_adam_step's kernel itself: one arithmetic, whichever entry point is used
  if (rule == kRuleAdam)
    return gcmi_adam_step(d_param, d_grad, d_state1, d_state2, n, lr, desc->beta1, desc->beta2, desc->eps, step, stream);
  const bool vec = aligned16(d_param) && aligned16(d_grad) && (n_states < 1 || aligned16(d_state1)) &&
                   (n_states < 2 || aligned16(d_state2));
  const int64_t n4 = vec ? n / 4 : 0;
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>((std::max(n4, n - 4 * n4) + kOBlock - 1) / kOBlock, 1),
                                            kOMaxBlocks);
  opt_dispatch(rule, [&](auto r) {
    hipLaunchKernelGGL((opt_step_kernel<decltype(r)::value>), dim3(blocks), dim3(kOBlock), 0, (hipStream_t)stream,
                       d_param, d_grad, d_state1, d_state2, n4, n, k);
  });
  GCMI_CHECK_LAUNCH("opt_step");
  return GCMI_OK;
}

int64_t gcmi_lamb_scratch_floats(int64_t n, int64_t n_segments) {
  if (n < 0 || n_segments < 0) return -1;
  // [2 doubles per chunk | the update arena]
  return 4 * lamb_max_chunks(n, n_segments) + (n + 3) / 4 * 4;
}

int gcmi_lamb_step(const gcmi_opt_desc* desc, float* d_param, const float* d_grad, float* d_m, float* d_v,
                   float* d_scratch, const int64_t* d_segments, int32_t n_segments, int64_t n, float* d_norms, float lr,
                   void* stream) {
  GCMI_CHECK_ARG(desc != nullptr, "lamb: NULL description");
  GCMI_CHECK_ARG(desc->rule == GCMI_RULE_LAMB, "lamb: rule %d is not GCMI_RULE_LAMB", desc->rule);
  GCMI_CHECK_ARG(n >= 0 && n_segments >= 0, "lamb: bad n / n_segments");
  GCMI_CHECK_ARG(desc->beta1 >= 0.f && desc->beta1 < 1.f && desc->beta2 >= 0.f && desc->beta2 < 1.f,
                 "lamb: betas must lie in [0, 1)");
  if (n == 0 || n_segments == 0) return GCMI_OK;
  GCMI_CHECK_ARG(d_param && d_grad && d_m && d_v && d_scratch && d_segments, "lamb: NULL buffer");
  GCMI_CHECK_ARG(aligned16(d_scratch), "lamb: the scratch must be 16-byte aligned");
  const int64_t chunks = lamb_max_chunks(n, n_segments);
  GCMI_CHECK_ARG(chunks < ((int64_t)1 << 31), "lamb: too many chunks");
  double* partial = reinterpret_cast<double*>(d_scratch);
  float* u = d_scratch + 4 * chunks;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3((unsigned)chunks), dim3(kOBlock), 0, st, d_param, d_grad, d_m, d_v, u,
                     partial, d_segments, n_segments, n, desc->beta1, 1.f - desc->beta1, desc->beta2, 1.f - desc->beta2,
                     desc->eps, desc->weight_decay);
  GCMI_CHECK_LAUNCH("lamb_moments");
  hipLaunchKernelGGL(lamb_apply_kernel, dim3((unsigned)chunks), dim3(kOBlock), 0, st, d_param, u, partial, d_segments,
                     n_segments, n, lr, 10.f, d_norms);
  GCMI_CHECK_LAUNCH("lamb_apply");
  return GCMI_OK;
}

}  // extern "C"
