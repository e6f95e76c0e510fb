// The two head kernels of the dual (policy + value) network, one trunk with two 1x1 heads.
//
// policy_value_head: the inference head, policy_value_head_body (policy_head.h) without the ownership
// row: masked-softmax probabilities at temperature 1 and the value head's fp32 logits from one read
// of the board.
//
// head_backward_add: head_backward_accumulate (policy_head.h) for one head.  It adds the value head's
// ReLU'-masked dY into the dZ the policy head wrote, so the dual trainer runs every policy-head kernel
// unchanged and the trunk backward sees the sum of both heads' gradients.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "policy_head.h"

namespace agk {

template <int NT, class Board>
__global__ __launch_bounds__(NT) void policy_value_head_kernel(PolicyValueHeadArgs a) {
  policy_value_head_body<NT, Board, false>(a, nullptr, nullptr, nullptr);
}

void launch_policy_value_head(const PolicyValueHeadArgs& a, hipStream_t st) {
  if (head_rows_mapping(a.B, a.S, a.C))
    hipLaunchKernelGGL((policy_value_head_kernel<512, BoardRows<512>>), dim3(a.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((policy_value_head_kernel<1024, BoardRegs<1024>>), dim3(a.B), dim3(1024), 0, st, a);
}

template <int NT>
__global__ __launch_bounds__(NT) void head_backward_add_kernel(PolicyHeadArgs a, const float* dlogits) {
  const float* const w[1] = {a.w};
  const float* const g[1] = {dlogits};
  float* const dhead[1] = {a.dhead};
  head_backward_accumulate<NT, 1>(a.y, a.dz, w, g, dhead, a.S, a.C, a.C_real);
}

void launch_head_backward_add(const PolicyHeadArgs& a, const float* dlogits, hipStream_t st) {
  if (head_wide_block(a.B)) hipLaunchKernelGGL(head_backward_add_kernel<1024>, dim3(a.B), dim3(1024), 0, st, a, dlogits);
  else hipLaunchKernelGGL(head_backward_add_kernel<256>, dim3(a.B), dim3(256), 0, st, a, dlogits);
}

}  // namespace agk
