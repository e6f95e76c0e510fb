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
// policy_head_soft_pass (the pass head of the dual net) is the same body over NE = S * S + 1 entries, the
// pass logit (pass_logit, policy_head.h) last: tdist rows have width NE, the board part moves with sym,
// the pass entry does not, and m, the argmax pair and the cross-entropy run over all NE entries.  Thread
// S * S owns the pass entry in every loop and reduction, so with z_pass = -1e30 and a zero pass column each
// sum gets one more exact zero and the board's outputs carry policy_head_soft's bits.  Besides dz, dhead,
// loss and correct it writes dpass[b] = dL/dz_pass and the partial row
// dpw[b] = [dzp * pooled[b] (2 C_real) | dzp], which head_grad_sums turns into d pass_w and d pass_b.
//
// One body, policy_head_soft_body<.., PASS>, and two thin __global__s.  PolicyHeadSoftArgs is an argument
// struct of its own and the pass operands travel behind it (PolicyHeadSoftPassArgs), so PolicyHeadArgs and
// PolicyHeadSoftArgs, and with them the kernarg layout and code objects of the plain, REG and soft kernels,
// stay exactly as they are: everything the pass entry adds sits under if constexpr (PASS).  From
// policy_head.h the body uses head_stage_weights, the board holders with their backward, board_launder,
// block_argmax (for the logits and for q), the block reductions and head_bias_grad.  Sums run in a fixed
// order (wave xor-shuffles, then the waves in order): no atomics.  No legal mask, no temperature, no
// binary-CE loss, no entropy / KL terms or stats, no e5m2 dz.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "policy_head.h"
#include "symmetry.h"

namespace agk {

template <int NT, class Board, bool PASS>
__device__ __forceinline__ void policy_head_soft_body(const PolicyHeadSoftArgs& a, const PassHeadOperands& ps) {
  static_assert(NT >= 368, "one target entry per thread");
  __shared__ float w_s[256];
  __shared__ float z_s[368];
  __shared__ float q_s[368];
  __shared__ float red[16];
  __shared__ int redi[16];
  // boards in reverse, as policy_head_kernel (the last-written boards are still in the Infinity Cache)
  const int b = (int)gridDim.x - 1 - (int)blockIdx.x;
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int NE = PASS ? SS + 1 : SS;  // entries of the softmax: the board points, then the pass
  const int HP = a.S + 2;
  constexpr int NW = NT / 64;  // the block reductions' wave count (policy_head.h)
  // this thread's target entry (NE <= 362 < NT: one entry per thread), requested ahead of the board
  // so that its latency hides behind the board's loads; negative entries (and NaN) count as 0
  float qv = 0.f;
  if (tid < NE) {
    int col = SS;  // the pass column does not move with the symmetry
    if (!PASS || tid < SS) {
      const int s = a.sym ? a.sym[b] : 0;
      const int i = tid / a.S, j = tid - i * a.S;
      int x, y;
      sym_inv(s, a.S, i, j, x, y);
      col = x * a.S + y;
    }
    size_t at = (size_t)b * a.T + col;
    if constexpr (PASS) at = bounds_at((long long)at, ps.tdist_elems);
    qv = fmaxf(a.tdist[at], 0.f);
  }
  head_stage_weights<NT>({w_s}, {a.w}, a.C, a.C_real);
  Board board;
  board.load(a.y + (size_t)b * HP * HP * a.C, a.S, a.C);
  float zp = 0.f, pv = 0.f;  // the pass logit; this thread's pooled value
  if constexpr (PASS) zp = pass_logit<NT>(ps, b, a.C, red, pv) + ps.pass_b[0];
  __syncthreads();  // w_s is staged (PASS: red is free again)
  const float bias = a.b[0];

  float lmax = -INFINITY;
  int lidx = 0x7fffffff;
  board.dots(w_s, z_s, a.S, a.C);
  board_launder(board);  // or the backward keeps the dots' fp32 copies: BoardRegs<1024> spilt 180 bytes per lane
  for (int p = tid; p < NE; p += NT) {
    const float z = (!PASS || p < SS) ? z_s[p] + bias : zp;
    z_s[p] = z;
    if (z > lmax) {  // first max wins (p increases within a thread)
      lmax = z;
      lidx = p;
    }
  }
  // block argmax / max of the logits and of q (ties -> smallest index)
  const ArgMax zm = block_argmax<NT>(lmax, lidx, red, redi);
  __syncthreads();  // red / redi are reused for q
  const ArgMax qm = block_argmax<NT>(tid < NE ? qv : -INFINITY, tid < NE ? tid : 0x7fffffff, red, redi);
  const float zmax = zm.v;
  float ls = 0.f;
  for (int p = tid; p < NE; p += NT) ls += __expf(z_s[p] - zmax);
  const float sum = block_reduce_sum<NW>(ls, red);
  const float inv = 1.f / sum;
  const float lse = __logf(sum);

  // the target's mass (fixed-order block sum), the renormalised target staged in LDS, the cross-entropy
  const float m = block_reduce_sum<NW>(qv, red);
  const bool has = m > 0.f && m < INFINITY;  // an infinite entry: no finite target, no loss
  float ce = 0.f;
  if (tid < NE) {
    const float qh = has ? qv / m : 0.f;
    q_s[tid] = qh;
    if (qh > 0.f) ce = qh * (z_s[tid] - zmax - lse);
  }
  ce = block_reduce_sum<NW>(ce, red);
  if (tid == 0) {
    a.loss[b] = has ? 0.f - ce : 0.f;
    a.correct[b] = (has && zm.idx == qm.idx) ? 1.f : 0.f;
  }
  const float sc = has ? a.grad_scale * (a.weight ? a.weight[b] : 1.f) : 0.f;
  for (int p = tid; p < NE; p += NT) z_s[p] = has ? (__expf(z_s[p] - zmax) * inv - q_s[p]) * sc : 0.f;
  __syncthreads();
  if constexpr (PASS) {
    // the pass entry's gradient and its per-board partial row [dzp * pooled (2 C_real) | dzp]
    const float dzp = z_s[SS];
    const long long row = (long long)b * (2 * a.C_real + 1);
    if (tid < 2 * a.C) {
      const int k = tid >= a.C, c = tid - k * a.C;
      if (c < a.C_real) ps.dpw[bounds_at(row + k * a.C_real + c, ps.dpw_elems)] = dzp * pv;
    }
    if (tid == 0) {
      ps.dpw[bounds_at(row + 2 * a.C_real, ps.dpw_elems)] = dzp;
      ps.dpass[bounds_at(b, ps.dpass_elems)] = dzp;
    }
  }
  // the shared backward reads only these fields of the plain head's arguments
  PolicyHeadArgs pa{};
  pa.dz = a.dz;
  pa.dhead = a.dhead;
  pa.S = a.S;
  pa.C = a.C;
  pa.C_real = a.C_real;
  board.backward(pa, b, w_s, z_s);
  head_bias_grad<NT, NW>(z_s, SS, red, a.dhead + (size_t)b * (a.C_real + 1) + a.C_real);
}

template <int NT, class Board>
__global__ __launch_bounds__(NT) void policy_head_soft_kernel(PolicyHeadSoftArgs a) {
  policy_head_soft_body<NT, Board, false>(a, {});
}

void launch_policy_head_soft(const PolicyHeadSoftArgs& a, hipStream_t st) {
  if (head_rows_mapping(a.B, a.S, a.C))
    hipLaunchKernelGGL((policy_head_soft_kernel<512, BoardRows<512>>), dim3(a.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((policy_head_soft_kernel<1024, BoardRegs<1024>>), dim3(a.B), dim3(1024), 0, st, a);
}

template <int NT, class Board>
__global__ __launch_bounds__(NT) void policy_head_soft_pass_kernel(PolicyHeadSoftPassArgs a) {
  policy_head_soft_body<NT, Board, true>(a.head, a.pass);
}

void launch_policy_head_soft_pass(const PolicyHeadSoftPassArgs& a, hipStream_t st) {
  const PolicyHeadSoftArgs& h = a.head;
  head_check_geometry("policy_head_soft_pass", h.B, h.S, h.C, h.C_real);
  if (head_rows_mapping(h.B, h.S, h.C))
    hipLaunchKernelGGL((policy_head_soft_pass_kernel<512, BoardRows<512>>), dim3(h.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((policy_head_soft_pass_kernel<1024, BoardRegs<1024>>), dim3(h.B), dim3(1024), 0, st, a);
  bounds_debug_check("policy_head_soft_pass", st);
}

}  // namespace agk
