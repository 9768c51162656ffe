// The elementwise optimizer rules, shared by gcmi_opt_step (optim.hip) and the small-batch engine's step-end kernel
// (smallstep.hip).  Each rule follows the operation order of torch's single-tensor implementation
// (torch/optim/{sgd,adagrad,rmsprop,adam,adamw}.py), the way adam_kernel (loss.hip) follows torch.optim.Adam.
#pragma once
#include <type_traits>

#include "common.h"

namespace gcmi {

// Kernel-side rules: gcmi_opt_desc.rule, with the two cases split out that change the arithmetic at compile time.
enum OptRule {
  kRuleSGD = GCMI_RULE_SGD,
  kRuleAdagrad = GCMI_RULE_ADAGRAD,
  kRuleRMSprop = GCMI_RULE_RMSPROP,  // momentum == 0
  kRuleAdamL2 = GCMI_RULE_ADAM_L2,   // weight_decay != 0
  kRuleAdamW = GCMI_RULE_ADAMW,
  kRuleAdam = 16,                    // ADAM_L2 with weight_decay == 0: the arithmetic of adam_kernel, bit for bit
  kRuleRMSpropMom = 17,              // momentum != 0
};

struct OptConsts {
  float lr, eps;
  float one_minus_b1, b2, one_minus_b2, step_size, inv_bc2_sqrt;  // Adam family
  float wd;                                                        // ADAM_L2: weight_decay; ADAMW: 1 - lr * weight_decay
  float alpha, one_minus_alpha, momentum;                          // RMSprop
};

// Checks the description and fills the constants of one step; *rule = the kernel-side rule.  optim.hip.
int opt_consts(const gcmi_opt_desc* d, float lr, int64_t step, OptConsts* out, int* rule);
// how many state arenas the (kernel-side) rule reads and writes
inline int opt_rule_states(int rule) {
  return rule == kRuleSGD ? 0 : (rule == kRuleAdagrad || rule == kRuleRMSprop) ? 1 : 2;
}

template <int R>
__device__ __forceinline__ void opt_update(float& p, float g, float& s1, float& s2, const OptConsts& k) {
  if constexpr (R == kRuleSGD) {
    p -= k.lr * g;  // param.add_(grad, alpha=-lr)
  } else if constexpr (R == kRuleAdagrad) {
    s1 = s1 + g * g;                    // state_sum.addcmul_(grad, grad, value=1)
    const float sd = sqrtf(s1) + k.eps;  // std = state_sum.sqrt().add_(eps)
    p -= k.lr * (g / sd);               // param.addcdiv_(grad, std, value=-clr)
  } else if constexpr (R == kRuleRMSprop || R == kRuleRMSpropMom) {
    s1 = s1 * k.alpha + g * g * k.one_minus_alpha;  // square_avg.mul_(alpha).addcmul_(grad, grad, value=1-alpha)
    const float avg = sqrtf(s1) + k.eps;            // avg = square_avg.sqrt().add_(eps)
    if constexpr (R == kRuleRMSpropMom) {
      s2 = s2 * k.momentum + g / avg;  // buf.mul_(momentum).addcdiv_(grad, avg)
      p -= k.lr * s2;                  // param.add_(buf, alpha=-lr)
    } else {
      p -= k.lr * (g / avg);  // param.addcdiv_(grad, avg, value=-lr)
    }
  } else {
    if constexpr (R == kRuleAdamL2) g = g + k.wd * p;  // grad = grad.add(param, alpha=weight_decay)
    if constexpr (R == kRuleAdamW) p = p * k.wd;       // param.mul_(1 - lr * weight_decay)
    // torch.optim.Adam (optimizers.py:231-241): exp_avg.lerp_, exp_avg_sq.mul_.addcmul_, addcdiv_
    s1 = s1 + (g - s1) * k.one_minus_b1;
    s2 = s2 * k.b2 + g * g * k.one_minus_b2;
    const float denom = sqrtf(s2) * k.inv_bc2_sqrt + k.eps;
    p -= k.step_size * (s1 / denom);
  }
}

// Calls f(std::integral_constant<int, rule>) for the kernel-side rule; false for a value that is none.
template <typename F>
inline bool opt_dispatch(int rule, F&& f) {
  switch (rule) {
    case kRuleSGD: f(std::integral_constant<int, kRuleSGD>()); return true;
    case kRuleAdagrad: f(std::integral_constant<int, kRuleAdagrad>()); return true;
    case kRuleRMSprop: f(std::integral_constant<int, kRuleRMSprop>()); return true;
    case kRuleRMSpropMom: f(std::integral_constant<int, kRuleRMSpropMom>()); return true;
    case kRuleAdamL2: f(std::integral_constant<int, kRuleAdamL2>()); return true;
    case kRuleAdamW: f(std::integral_constant<int, kRuleAdamW>()); return true;
    case kRuleAdam: f(std::integral_constant<int, kRuleAdam>()); return true;
    default: return false;
  }
}

}  // namespace gcmi
