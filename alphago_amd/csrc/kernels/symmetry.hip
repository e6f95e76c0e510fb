// D4 symmetry ensembling for inference: the trunk runs on G orientations of every board (G = 8: all
// symmetries; G = 1: one drawn symmetry per board) and the head folds them back into the board's
// own frame.
//  * d4_expand: one featurized conv input [B] -> its G * B orientations (a 16-byte-chunk gather), so
//    the featurizer runs once per position.
//  * policy_head_d4: the policy head (1x1 conv, legal-masked softmax) of the G orientations of a
//    board, each mapped back to the original frame, averaged in fixed g order.
//  * group_mean: the same average for the value net's scalar outputs.
// Symmetry convention: symmetry.h (pack_input's).  From policy_head.h the head uses head_stage_weights,
// the board holders, the block reductions and head_rows_mapping.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "policy_head.h"
#include "symmetry.h"

namespace agk {

// dst[k][i][j][:] = src[k % B][sym_inv(sym[k], i, j)][:] over the interior; thread = one 16-byte
// channel chunk, consecutive threads consecutive chunks of a destination pixel row (the source
// pixel's row is contiguous too: Cp * 2 bytes).
__global__ __launch_bounds__(256) void d4_expand_kernel(D4ExpandArgs a) {
  const int SS = a.S * a.S;
  const int C8 = a.Cp >> 3;
  const int HP = a.S + 2 * a.P;
  const int64_t total = (int64_t)a.GB * SS * C8;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(idx % C8);
    const int64_t rest = idx / C8;
    const int p = (int)(rest % SS);
    const int k = (int)(rest / SS);
    const int i = p / a.S, j = p - i * a.S;
    int x, y;
    sym_inv(a.sym[k], a.S, i, j, x, y);
    const int b = k % a.B;
    const size_t so = ((size_t)(b * HP + x + a.P) * HP + y + a.P) * a.Cp + c8 * 8;
    const size_t dof = ((size_t)((size_t)k * HP + i + a.P) * HP + j + a.P) * a.Cp + c8 * 8;
    *(bf16x8*)(a.dst + dof) = *(const bf16x8*)(a.src + so);
  }
}

void launch_d4_expand(const D4ExpandArgs& a, hipStream_t st) {
  const int64_t total = (int64_t)a.GB * a.S * a.S * (a.Cp >> 3);
  int64_t blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(d4_expand_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
}

// One workgroup per original board b.  For g = 0 .. G - 1: board g * B + b of the trunk output is
// read once into registers (Board, as policy_head_kernel), its logits go to LDS in the transformed
// frame, thread p < S * S (S * S <= 361 < NT: one point per thread) picks up z[fwd_s(p)], masks it by
// legal[b][p] (original frame) and runs policy_head_kernel<false>'s softmax (same exp, same
// all-illegal -> 0 rule); the G probabilities of point p add up in thread p's register in g order
// and leave as acc * (1 / G).  No atomics: two runs give the same bits.
template <int NT, class Board>
__global__ __launch_bounds__(NT) void policy_head_d4_kernel(PolicyHeadD4Args a) {
  __shared__ float w_s[256];
  __shared__ float z_s[368];
  __shared__ float red[16];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int HP = a.S + 2;
  head_stage_weights<NT>({w_s}, {a.w}, a.C, a.C_real);
  const float bias = a.b[0];
  const bool own = tid < SS;
  const bool ok = own && (!a.legal || a.legal[(size_t)(b % a.LB) * SS + tid]);
  const int px = tid / a.S, py = tid - px * a.S;
  float acc = 0.f;
  for (int g = 0; g < a.G; ++g) {
    const int k = g * a.B + b;
    Board board;
    board.load(a.y + (size_t)k * HP * HP * a.C, a.S, a.C);
    __syncthreads();  // w_s staged (g = 0); the previous pass has read z_s
    board.dots(w_s, z_s, a.S, a.C);
    float z = -INFINITY;
    if (ok) {
      int qx, qy;
      sym_fwd(a.sym[k], a.S, px, py, qx, qy);
      z = (z_s[qx * a.S + qy] + bias) * a.inv_temp;
    }
    const float zmax = block_reduce_max(z, red);
    const float e = (z == -INFINITY) ? 0.f : __expf(z - zmax);
    const float sum = block_reduce_sum(e, red);
    const float inv = 1.f / sum;
    acc += (z == -INFINITY) ? 0.f : e * inv;
  }
  if (own) a.probs[(size_t)b * SS + tid] = acc * a.inv_g;
}

// The thread mapping follows head_rows_mapping at the trunk batch G * B, so the
// logits of an orientation carry the bits policy_head_probs gives the same board in a G * B batch.
//
// Few positions (B < kD4SplitBelow, G > 1, scratch given): B workgroups walking G boards one after
// the other leave most CUs idle for G board-load latencies (16 positions: +73 us on a 486 us forward,
// profiles/r10/README.md).  Then the same kernel runs over the G * B orientations as G * B "positions"
// of one orientation each (legal rows repeating with period B) into scratch, and group_mean adds the
// G rows of a position in g order: still fixed-order fp32, no atomics.
void launch_policy_head_d4(const PolicyHeadD4Args& a0, hipStream_t st) {
  PolicyHeadD4Args a = a0;
  a.inv_g = (float)(1.0 / a.G);
  a.LB = a.B;
  const bool rows = head_rows_mapping((int64_t)a.G * a.B, a.S, a.C);
  const bool split = a.G > 1 && a.scratch && a.B < kD4SplitBelow;
  if (split) {
    a.probs = a.scratch;
    a.B = a0.G * a0.B;
    a.G = 1;
    a.inv_g = 1.f;
  }
  if (rows) hipLaunchKernelGGL((policy_head_d4_kernel<512, BoardRows<512>>), dim3(a.B), dim3(512), 0, st, a);
  else hipLaunchKernelGGL((policy_head_d4_kernel<1024, BoardRegs<1024>>), dim3(a.B), dim3(1024), 0, st, a);
  if (split) launch_group_mean(a0.scratch, a0.probs, a0.B * a0.S * a0.S, a0.G, st);
}

__global__ __launch_bounds__(256) void group_mean_kernel(const float* __restrict__ v, float* __restrict__ out, int B,
                                                         int G, float inv_g) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += v[(size_t)g * B + b];
  out[b] = s * inv_g;
}

void launch_group_mean(const float* v, float* out, int B, int G, hipStream_t st) {
  hipLaunchKernelGGL(group_mean_kernel, dim3((B + 255) / 256), dim3(256), 0, st, v, out, B, G, (float)(1.0 / G));
}

}  // namespace agk
