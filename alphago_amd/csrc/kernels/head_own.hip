// The ownership head of the dual network: a third 1x1 head on the trunk, tanh per board point, whose
// target is the final territory map in the mover's frame.
//
// value_own_head: the training / evaluation forward of both non-policy heads.  One workgroup per
// board reads the board once into registers (head_stage_weights, BoardRows / BoardRegs with
// board_launder between the two dots, policy_head.h) and takes the value row (head_logits' quantity,
// BoardRegs: its bits) and the ownership row from that copy.  With
// a target it also writes the per-board MSE, the sign-agreement count and the gradient with respect
// to the ownership logits.  The target is gathered through the board's symmetry as policy_head_soft
// gathers tdist (sym_inv), so no host work moves it with the augmented planes.
//
// head_backward_add2: head_backward_accumulate (policy_head.h) for two heads, one read of y and one
// read-modify-write of dz instead of two each.  dhead1 has head_backward_add's bits, and with g2 == 0
// so has dz (fma(0, w2, x) == x; a -0 sum becomes +0).
//
// policy_value_own_head: policy_value_head_body (policy_head.h) with the ownership row, for inference;
// probs and zv carry policy_value_head's bits.
//
// policy_value_pass_head: the same body with the pass entry (PASS) in the softmax, with the ownership row
// (head.wo given) or without; probs rows have S * S + 1 entries, zv (and own) carry policy_value_head's
// (policy_value_own_head's) bits.  It lives here because its arguments are policy_value_own_head's plus
// the pass operands.
//
// No atomics: every sum has a fixed order.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "policy_head.h"
#include "symmetry.h"

namespace agk {

template <int NT, class Board>
__global__ __launch_bounds__(NT) void value_own_head_kernel(ValueOwnHeadArgs a) {
  static_assert(NT >= 368, "one board point per thread");
  __shared__ float wv_s[256];
  __shared__ float wo_s[256];
  __shared__ float zv_s[368];
  __shared__ float zo_s[368];
  __shared__ float red[16];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int HP = a.S + 2;
  // this thread's target entry (S * S <= 361 < NT), requested ahead of the board's loads
  float t = 0.f;
  if (a.target && tid < SS) {
    const int s = a.sym ? a.sym[b] : 0;
    const int i = tid / a.S, j = tid - i * a.S;
    int x, y;
    sym_inv(s, a.S, i, j, x, y);
    t = (float)a.target[(size_t)b * SS + x * a.S + y];
  }
  head_stage_weights<NT>({wv_s, wo_s}, {a.wv, a.wo}, a.C, a.C_real);
  Board board;
  board.load(a.y + (size_t)b * HP * HP * a.C, a.S, a.C);
  __syncthreads();
  const float vbias = a.bv[0];
  const float obias = a.bo[0];

  board.dots(wv_s, zv_s, a.S, a.C);
  board_launder(board);
  board.dots(wo_s, zo_s, a.S, a.C);

  float own = 0.f;
  if (tid < SS) {
    const size_t q = (size_t)b * SS + tid;
    a.zv[q] = zv_s[tid] + vbias;
    const float o = zo_s[tid] + obias;
    own = tanhf(o);
    if (a.olog) a.olog[q] = o;
    if (a.own) a.own[q] = own;
  }
  if (!a.target) return;
  const float e = own - t;
  float se = tid < SS ? e * e : 0.f;
  float ag = 0.f;
  if (tid < SS && t != 0.f) ag = ((own > 0.f ? 1.f : (own < 0.f ? -1.f : 0.f)) == t) ? 1.f : 0.f;
  se = block_reduce_sum(se, red);
  ag = block_reduce_sum(ag, red);
  if (tid == 0) {
    a.oloss[b] = se / (float)SS;
    a.oagree[b] = ag;
  }
  const float k = (a.valid ? a.valid[b] : 1.f) * (a.weight ? a.weight[b] : 1.f);
  // the board's coefficient first, so that a doubled weight doubles every entry exactly
  const float coef = a.grad_scale * k * (2.f / (float)SS);
  if (tid < SS) a.dlo[(size_t)b * SS + tid] = k == 0.f ? 0.f : coef * (e * (1.f - own * own));
}

void launch_value_own_head(const ValueOwnHeadArgs& a, hipStream_t st) {
  if (head_rows_mapping(a.B, a.S, a.C))
    hipLaunchKernelGGL((value_own_head_kernel<512, BoardRows<512>>), dim3(a.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((value_own_head_kernel<1024, BoardRegs<1024>>), dim3(a.B), dim3(1024), 0, st, a);
}

template <int NT>
__global__ __launch_bounds__(NT) void head_backward_add2_kernel(HeadBackwardAdd2Args a) {
  const float* const w[2] = {a.w1, a.w2};
  const float* const g[2] = {a.g1, a.g2};
  float* const dhead[2] = {a.dhead1, a.dhead2};
  head_backward_accumulate<NT, 2>(a.y, a.dz, w, g, dhead, a.S, a.C, a.C_real);
}

void launch_head_backward_add2(const HeadBackwardAdd2Args& a, hipStream_t st) {
  if (head_wide_block(a.B)) hipLaunchKernelGGL(head_backward_add2_kernel<1024>, dim3(a.B), dim3(1024), 0, st, a);
  else hipLaunchKernelGGL(head_backward_add2_kernel<256>, dim3(a.B), dim3(256), 0, st, a);
}

template <int NT, class Board>
__global__ __launch_bounds__(NT) void policy_value_own_head_kernel(PolicyValueOwnHeadArgs a) {
  policy_value_head_body<NT, Board, true>(a.pv, a.wo, a.bo, a.own);
}

void launch_policy_value_own_head(const PolicyValueOwnHeadArgs& a, hipStream_t st) {
  if (head_rows_mapping(a.pv.B, a.pv.S, a.pv.C))
    hipLaunchKernelGGL((policy_value_own_head_kernel<512, BoardRows<512>>), dim3(a.pv.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((policy_value_own_head_kernel<1024, BoardRegs<1024>>), dim3(a.pv.B), dim3(1024), 0, st, a);
}

template <int NT, class Board, bool OWN>
__global__ __launch_bounds__(NT) void policy_value_pass_head_kernel(PolicyValuePassHeadArgs a) {
  policy_value_head_body<NT, Board, OWN, true>(a.head.pv, a.head.wo, a.head.bo, a.head.own, a.pass);
}

template <bool OWN>
static void policy_value_pass_head_go(const PolicyValuePassHeadArgs& a, hipStream_t st) {
  const int B = a.head.pv.B;
  if (head_rows_mapping(B, a.head.pv.S, a.head.pv.C))
    hipLaunchKernelGGL((policy_value_pass_head_kernel<512, BoardRows<512>, OWN>), dim3(B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((policy_value_pass_head_kernel<1024, BoardRegs<1024>, OWN>), dim3(B), dim3(1024), 0, st, a);
}

void launch_policy_value_pass_head(const PolicyValuePassHeadArgs& a, hipStream_t st) {
  head_check_geometry("policy_value_pass_head", a.head.pv.B, a.head.pv.S, a.head.pv.C, a.head.pv.C_real);
  if (a.head.wo) policy_value_pass_head_go<true>(a, st);
  else policy_value_pass_head_go<false>(a, st);
  bounds_debug_check("policy_value_pass_head", st);
}

}  // namespace agk
