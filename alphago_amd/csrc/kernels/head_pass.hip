// The pass head of the dual net: one more logit next to the S * S board logits of the 1x1 policy head,
//   z_pass[b] = P[b].reshape(2 C) . pass_w + pass_b
// with P (B, 2, C) the mean and max of the trunk output over the board (a preceding gpool_fwd) and pass_w a
// zero-padded (2, C) copy of the net's (2 F, 1) weight.  The softmax runs over NP + 1 = S * S + 1 entries,
// the pass last (index NP, so it loses ties in every argmax).
//
// policy_head_soft_pass: policy_head_soft_kernel (head_soft.hip) over NP + 1 entries.  tdist rows have
// width NP + 1; the board part moves with sym, the pass entry is invariant.  q = max(t, 0) (NaN -> 0),
// m = the sum of all NP + 1 entries, has = 0 < m < inf, qh = q / m,
//   L = -sum_i qh_i log p_i,  dL/dz_i = (p_i - qh_i) * grad_scale * weight,  correct = [argmax z == first argmax q]
// Thread NP owns the pass entry in every loop and reduction, so with z_pass = -1e30 and a zero pass column
// each sum gets one more exact zero and the board's outputs carry policy_head_soft's bits.  Besides dz, dhead,
// loss and correct it writes dpass[b] = dL/dz_pass and the partial row dpw[b] = [dzp * P[b] (2 C_real) | dzp],
// which head_grad_sums turns into d pass_w and d pass_b.
//
// policy_value_pass_head<OWN>: policy_value_head_body (policy_head.h) with the pass entry in the masked
// softmax at temperature 1; the pass is always legal.  probs rows have NP + 1 entries; zv (and own) carry
// policy_value_head's (policy_value_own_head's) bits.
//
// __global__s and argument structs of their own; from policy_head.h: head_stage_weights, the board holders
// with their backward, board_launder, block_argmax, the block reductions, the masked softmax steps and
// head_bias_grad.  Sums run in a fixed order (wave xor-shuffles, then the waves in order): no atomics.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "policy_head.h"
#include "symmetry.h"

namespace agk {

#ifdef AGK_DEBUG
// Debug build: the accesses that are new here (pooled, pass_w, the target row, dpass, the partial row, the
// probability row) are checked against the tensors' extents; a violation sets this word and the access is
// redirected to element 0.  The launchers wait and raise on the word.  The extents themselves are checked on the
// host by the ops (ops.cpp) in every build, before any launch.
static __device__ unsigned g_pass_err;
#define PASS_DCHECK(cond) ((cond) ? true : (atomicOr(&::agk::g_pass_err, 1u), false))
static void pass_debug_check(const char* what, hipStream_t st) {
  hip_check(hipStreamSynchronize(st), "debug: stream synchronize");
  unsigned code = 0, zero = 0;
  hip_check(hipMemcpyFromSymbol(&code, HIP_SYMBOL(g_pass_err), sizeof(code)), "debug: read error word");
  if (code) {
    hip_check(hipMemcpyToSymbol(HIP_SYMBOL(g_pass_err), &zero, sizeof(zero)), "debug: clear error word");
    throw std::runtime_error(std::string(what) + ": device bounds check failed (debug build)");
  }
}
#else
#define PASS_DCHECK(cond) true
#endif

// index i into a tensor of n elements, 0 after a failed debug check
__device__ __forceinline__ long long pass_at(long long i, long long n) {
  return PASS_DCHECK(i >= 0 && i < n) ? i : 0;
}

// This thread's term of z_pass (thread t < 2 C owns entry t of the board's pooled row; pv keeps the pooled
// value for the partial row) summed over the block in a fixed order.
template <int NT>
__device__ __forceinline__ float pass_logit(const float* pooled, long long pooled_elems, const float* pass_w, int b,
                                            int C, float* red, float& pv) {
  static_assert(NT >= 512, "one pooled entry per thread (2 C <= 512)");
  const int tid = threadIdx.x;
  float term = 0.f;
  pv = 0.f;
  if (tid < 2 * C) {
    pv = pooled[pass_at((long long)b * 2 * C + tid, pooled_elems)];
    term = pv * pass_w[tid];
  }
  return block_reduce_sum(term, red);
}

template <int NT, class Board>
__global__ __launch_bounds__(NT) void policy_head_soft_pass_kernel(PolicyHeadSoftPassArgs a) {
  static_assert(NT >= 368, "one target entry per thread");
  __shared__ float w_s[256];
  __shared__ float z_s[368];
  __shared__ float q_s[368];
  __shared__ float red[16];
  __shared__ int redi[16];
  const int b = (int)gridDim.x - 1 - (int)blockIdx.x;  // policy_head_soft_kernel's board order
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int NE = SS + 1;  // entries of the softmax: the board points, then the pass
  const int HP = a.S + 2;
  // this thread's target entry (NE <= 362 < NT), requested ahead of the board
  float qv = 0.f;
  if (tid < NE) {
    int col = SS;  // the pass entry does not move with the symmetry
    if (tid < SS) {
      const int s = a.sym ? a.sym[b] : 0;
      const int i = tid / a.S, j = tid - i * a.S;
      int x, y;
      sym_inv(s, a.S, i, j, x, y);
      col = x * a.S + y;
    }
    qv = fmaxf(a.tdist[pass_at((long long)b * NE + col, a.tdist_elems)], 0.f);
  }
  head_stage_weights<NT>({w_s}, {a.w}, a.C, a.C_real);
  Board board;
  board.load(a.y + (size_t)b * HP * HP * a.C, a.S, a.C);
  float pv;
  const float zp = pass_logit<NT>(a.pooled, a.pooled_elems, a.pass_w, b, a.C, red, pv) + a.pass_b[0];
  __syncthreads();  // w_s is staged; red is free again
  const float bias = a.b[0];

  float lmax = -INFINITY;
  int lidx = 0x7fffffff;
  board.dots(w_s, z_s, a.S, a.C);
  board_launder(board);
  for (int p = tid; p < NE; p += NT) {
    const float z = p < SS ? z_s[p] + bias : zp;
    z_s[p] = z;
    if (z > lmax) {
      lmax = z;
      lidx = p;
    }
  }
  const ArgMax zm = block_argmax<NT>(lmax, lidx, red, redi);
  __syncthreads();  // red / redi are reused for q
  const ArgMax qm = block_argmax<NT>(tid < NE ? qv : -INFINITY, tid < NE ? tid : 0x7fffffff, red, redi);
  const float zmax = zm.v;
  float ls = 0.f;
  for (int p = tid; p < NE; p += NT) ls += __expf(z_s[p] - zmax);
  const float sum = block_reduce_sum(ls, red);
  const float inv = 1.f / sum;
  const float lse = __logf(sum);

  const float m = block_reduce_sum(qv, red);
  const bool has = m > 0.f && m < INFINITY;
  float ce = 0.f;
  if (tid < NE) {
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
  for (int p = tid; p < NE; p += NT) z_s[p] = has ? (__expf(z_s[p] - zmax) * inv - q_s[p]) * sc : 0.f;
  __syncthreads();
  // the pass entry's gradient and its per-board partial row [dzp * P (2 C_real) | dzp]
  const float dzp = z_s[SS];
  const long long row = (long long)b * (2 * a.C_real + 1);
  if (tid < 2 * a.C) {
    const int k = tid >= a.C, c = tid - k * a.C;
    if (c < a.C_real) a.dpw[pass_at(row + k * a.C_real + c, a.dpw_elems)] = dzp * pv;
  }
  if (tid == 0) {
    a.dpw[pass_at(row + 2 * a.C_real, a.dpw_elems)] = dzp;
    a.dpass[pass_at(b, a.dpass_elems)] = dzp;
  }
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

void launch_policy_head_soft_pass(const PolicyHeadSoftPassArgs& a, hipStream_t st) {
  if (a.C % 8 || a.C < 8 || a.C > 256 || a.C_real < 1 || a.C_real > a.C || a.B < 1 || a.S < 1 || a.S > 19)
    throw std::invalid_argument("policy_head_soft_pass: C a multiple of 8 in 8..256, 1 <= C_real <= C, B >= 1, S in 1..19");
  if (head_rows_mapping(a.B, a.S, a.C))
    hipLaunchKernelGGL((policy_head_soft_pass_kernel<512, BoardRows<512>>), dim3(a.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((policy_head_soft_pass_kernel<1024, BoardRegs<1024>>), dim3(a.B), dim3(1024), 0, st, a);
#ifdef AGK_DEBUG
  pass_debug_check("policy_head_soft_pass", st);
#endif
}

template <int NT, class Board, bool OWN>
__global__ __launch_bounds__(NT) void policy_value_pass_head_kernel(PolicyValuePassHeadArgs a) {
  __shared__ float wp_s[256];
  __shared__ float wv_s[256];
  __shared__ float z_s[368];
  __shared__ float zv_s[368];
  __shared__ float red[16];
  float* wo_s = nullptr;
  float* zo_s = nullptr;
  const int b = (int)gridDim.x - 1 - (int)blockIdx.x;  // policy_head_kernel's board order
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int NE = SS + 1;
  const int HP = a.S + 2;
  if constexpr (OWN) {
    __shared__ float wo_lds[256];
    __shared__ float zo_lds[368];
    wo_s = wo_lds;
    zo_s = zo_lds;
    head_stage_weights<NT>({wp_s, wv_s, wo_s}, {a.wp, a.wv, a.wo}, a.C, a.C_real);
  } else {
    head_stage_weights<NT>({wp_s, wv_s}, {a.wp, a.wv}, a.C, a.C_real);
  }
  Board board;
  board.load(a.y + (size_t)b * HP * HP * a.C, a.S, a.C);
  float pv;
  const float zp = pass_logit<NT>(a.pooled, a.pooled_elems, a.pass_w, b, a.C, red, pv) + a.pass_b[0];
  __syncthreads();
  const float bias = a.bp[0];
  const float vbias = a.bv[0];
  const float obias = OWN ? a.bo[0] : 0.f;
  const uint8_t* legal = a.legal ? a.legal + (size_t)b * SS : nullptr;

  board.dots(wp_s, z_s, a.S, a.C);  // ends with a barrier
  board_launder(board);
  board.dots(wv_s, zv_s, a.S, a.C);
  if constexpr (OWN) {
    board_launder(board);
    board.dots(wo_s, zo_s, a.S, a.C);
  }
  for (int p = tid; p < SS; p += NT) {
    a.zv[(size_t)b * SS + p] = zv_s[p] + vbias;
    if constexpr (OWN) a.own[(size_t)b * SS + p] = tanhf(zo_s[p] + obias);
  }
  // the masked softmax over the board points and the pass (thread SS owns the pass entry)
  float lmax = head_mask_logits<NT>(z_s, SS, bias, 1.f, legal).v;
  if (tid == SS) {
    z_s[SS] = zp;
    lmax = zp;
  }
  const float zmax = block_reduce_max(lmax, red);  // its barriers publish z_s
  const float inv = 1.f / head_exp_sum<NT>(z_s, NE, zmax, red);
  float* row = a.probs + pass_at((long long)b * NE, a.probs_elems - SS);
  head_write_probs<NT>(row, z_s, NE, zmax, inv);
}

template <bool OWN>
static void policy_value_pass_head_go(const PolicyValuePassHeadArgs& a, hipStream_t st) {
  if (head_rows_mapping(a.B, a.S, a.C))
    hipLaunchKernelGGL((policy_value_pass_head_kernel<512, BoardRows<512>, OWN>), dim3(a.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((policy_value_pass_head_kernel<1024, BoardRegs<1024>, OWN>), dim3(a.B), dim3(1024), 0, st, a);
}

void launch_policy_value_pass_head(const PolicyValuePassHeadArgs& a, hipStream_t st) {
  if (a.C % 8 || a.C < 8 || a.C > 256 || a.C_real < 1 || a.C_real > a.C || a.B < 1 || a.S < 1 || a.S > 19)
    throw std::invalid_argument("policy_value_pass_head: C a multiple of 8 in 8..256, 1 <= C_real <= C, B >= 1, S in 1..19");
  if (a.wo) policy_value_pass_head_go<true>(a, st);
  else policy_value_pass_head_go<false>(a, st);
#ifdef AGK_DEBUG
  pass_debug_check("policy_value_pass_head", st);
#endif
}

}  // namespace agk
