// The regularised variants of the fused policy head (policy_head_kernel<..., REG = true>,
// policy_head.h): per-board entropy / KL(q || p) / max |logit| diagnostics and the entropy-bonus and
// KL-anchor terms of the gradient.  launch_policy_head (head.hip) comes here only when stats,
// ref_probs or a coefficient is set.  The kernel, its blocks and the launch rule (policy_head_go,
// head_rows_mapping) are all in policy_head.h; this file only instantiates.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "policy_head.h"

namespace agk {

void launch_policy_head_reg(const PolicyHeadArgs& a, bool train, hipStream_t st) {
  if (train) policy_head_go<true, true>(a, st);
  else policy_head_go<false, true>(a, st);
}

}  // namespace agk
