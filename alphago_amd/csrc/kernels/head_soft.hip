// Soft-target fused policy head: policy_head_kernel<TRAIN = true> (policy_head.h) with a target
// DISTRIBUTION per board (the root visit distribution of a search) in place of one move index.
//
// Per board, with s its D4 symmetry (the tensor pack_input got) and q_i = max(tdist[src_s(i)], 0)
// gathered through sym_inv -- the convention by which pack_input moves an integer target with
// sym_fwd, so a one-hot row lands exactly on pack_input's target_out:
//   m = sum_i q_i over the board points (a trailing pass column is never read),  qh = q / m
//   L = -sum_i qh_i log p_i,   dL/dz_i = (p_i - qh_i) * grad_scale * weight
//   correct = [argmax p == smallest index among the maxima of q]
// with log p_i = z_i - zmax - lse (never log(p_i)); terms with qh_i == 0 add nothing.  A board with
// m == 0 (an all-zero row, or all mass on the pass) has no loss: loss = correct = 0, and a zero
// gradient is still written (dz interior, dhead row).  NaN entries count as 0 like negatives; a board
// with an infinite entry (m == inf) has no loss either, so no output is ever non-finite because of
// the targets.  Unlike the one-hot loss there is no Keras
// clip of p to [1e-7, 1 - 1e-7]: the loss is the exact cross-entropy of its gradient.
//
// A __global__ and an argument struct of its own: PolicyHeadArgs, and with it the kernarg layout and
// code objects of the plain and REG kernels, stay exactly as they are.  From policy_head.h it uses
// head_stage_weights, the board holders with their backward, board_launder, block_argmax (for the
// logits and for q), the block reductions and head_bias_grad.  No legal mask, no temperature, no
// binary-CE loss, no entropy / KL terms or stats, no e5m2 dz.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "policy_head.h"
#include "symmetry.h"

namespace agk {

template <int NT, class Board>
__global__ __launch_bounds__(NT) void policy_head_soft_kernel(PolicyHeadSoftArgs a) {
  static_assert(NT >= 368, "one board point per thread");
  __shared__ float w_s[256];
  __shared__ float z_s[368];
  __shared__ float q_s[368];
  __shared__ float red[16];
  __shared__ int redi[16];
  // boards in reverse, as policy_head_kernel (the last-written boards are still in the Infinity Cache)
  const int b = (int)gridDim.x - 1 - (int)blockIdx.x;
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int HP = a.S + 2;
  // this thread's target entry (S * S <= 361 < NT: one point per thread), requested ahead of the board
  // so that its latency hides behind the board's loads; negative entries (and NaN) count as 0
  float qv = 0.f;
  if (tid < SS) {
    const int s = a.sym ? a.sym[b] : 0;
    const int i = tid / a.S, j = tid - i * a.S;
    int x, y;
    sym_inv(s, a.S, i, j, x, y);
    qv = fmaxf(a.tdist[(size_t)b * a.T + x * a.S + y], 0.f);
  }
  head_stage_weights<NT>({w_s}, {a.w}, a.C, a.C_real);
  Board board;
  board.load(a.y + (size_t)b * HP * HP * a.C, a.S, a.C);
  __syncthreads();
  const float bias = a.b[0];

  float lmax = -INFINITY;
  int lidx = 0x7fffffff;
  board.dots(w_s, z_s, a.S, a.C);
  board_launder(board);  // or the backward keeps the dots' fp32 copies: BoardRegs<1024> spilt 180 bytes per lane
  for (int p = tid; p < SS; p += NT) {
    const float z = z_s[p] + bias;
    z_s[p] = z;
    if (z > lmax) {  // first max wins (p increases within a thread)
      lmax = z;
      lidx = p;
    }
  }
  // block argmax / max of the logits and of q (ties -> smallest index)
  const ArgMax zm = block_argmax<NT>(lmax, lidx, red, redi);
  __syncthreads();  // red / redi are reused for q
  const ArgMax qm = block_argmax<NT>(tid < SS ? qv : -INFINITY, tid < SS ? tid : 0x7fffffff, red, redi);
  const float zmax = zm.v;
  float ls = 0.f;
  for (int p = tid; p < SS; p += NT) ls += __expf(z_s[p] - zmax);
  const float sum = block_reduce_sum(ls, red);
  const float inv = 1.f / sum;
  const float lse = __logf(sum);

  // board mass (fixed-order block sum), the renormalised target staged in LDS, the cross-entropy
  const float m = block_reduce_sum(qv, red);
  const bool has = m > 0.f && m < INFINITY;  // an infinite entry: no finite target, no loss
  float ce = 0.f;
  if (tid < SS) {
    const float qh = has ? qv / m : 0.f;
    q_s[tid] = qh;
    if (qh > 0.f) ce = qh * (z_s[tid] - zmax - lse);
  }
  ce = block_reduce_sum(ce, red);
  if (tid == 0) {
    a.loss[b] = has ? 0.f - ce : 0.f;
    a.correct[b] = (has && zm.idx == qm.idx) ? 1.f : 0.f;
  }
  const float sc = has ? a.grad_scale * (a.weight ? a.weight[b] : 1.f) : 0.f;
  for (int p = tid; p < SS; p += NT) z_s[p] = has ? (__expf(z_s[p] - zmax) * inv - q_s[p]) * sc : 0.f;
  __syncthreads();
  // the shared backward reads only these fields of the plain head's arguments
  PolicyHeadArgs pa{};
  pa.dz = a.dz;
  pa.dhead = a.dhead;
  pa.S = a.S;
  pa.C = a.C;
  pa.C_real = a.C_real;
  board.backward(pa, b, w_s, z_s);
  head_bias_grad<NT>(z_s, SS, red, a.dhead + (size_t)b * (a.C_real + 1) + a.C_real);
}

void launch_policy_head_soft(const PolicyHeadSoftArgs& a, hipStream_t st) {
  if (head_rows_mapping(a.B, a.S, a.C))
    hipLaunchKernelGGL((policy_head_soft_kernel<512, BoardRows<512>>), dim3(a.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((policy_head_soft_kernel<1024, BoardRegs<1024>>), dim3(a.B), dim3(1024), 0, st, a);
}

}  // namespace agk
