// The ownership head of the dual network: a third 1x1 head on the trunk, tanh per board point, whose
// target is the final territory map in the mover's frame.
//
// value_own_head: the training / evaluation forward of both non-policy heads.  One workgroup per
// board reads the board once into registers (BoardRows / BoardRegs, policy_head.h) and takes the
// value row (head_logits' quantity, BoardRegs: its bits) and the ownership row from that copy.  With
// a target it also writes the per-board MSE, the sign-agreement count and the gradient with respect
// to the ownership logits.  The target is gathered through the board's symmetry as policy_head_soft
// gathers tdist (sym_inv), so no host work moves it with the augmented planes.
//
// head_backward_add2: head_backward_add (head_pv.hip) for two heads, one read of y and one
// read-modify-write of dz instead of two each.
//
// policy_value_own_head: policy_value_head (head_pv.hip) plus the ownership row, for inference.
//
// A translation unit of its own: the code objects of head.hip / head_reg.hip / head_soft.hip /
// head_pv.hip do not depend on these kernels (LDS variables are laid out per module).  No atomics:
// every sum has a fixed order.
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
  for (int c = tid; c < a.C; c += NT) {
    wv_s[c] = c < a.C_real ? a.wv[c] : 0.f;
    wo_s[c] = c < a.C_real ? a.wo[c] : 0.f;
  }
  Board board;
  board.load(a.y + (size_t)b * HP * HP * a.C, a.S, a.C);
  __syncthreads();
  const float vbias = a.bv[0];
  const float obias = a.bo[0];

  board.dots(wv_s, zv_s, a.S, a.C);
  // laundered as in policy_value_head: the second pass converts the packed bf16 again instead of
  // keeping the first pass's fp32 copies of the board live
#pragma unroll
  for (int u = 0; u < Board::P; ++u) asm volatile("" : "+v"(board.v[u]));
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

// policy_head_go's split
void launch_value_own_head(const ValueOwnHeadArgs& a, hipStream_t st) {
  if (a.B >= kHeadWideBelow && a.S * (a.C >> 3) <= 512)
    hipLaunchKernelGGL((value_own_head_kernel<512, BoardRows<512>>), dim3(a.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((value_own_head_kernel<1024, BoardRegs<1024>>), dim3(a.B), dim3(1024), 0, st, a);
}

// head_backward_add_kernel (head_pv.hip) with two gradient rows.  Thread (r, cg) walks positions
// r, r + R, ... and keeps both heads' dW partials in that order; each head's R partials per channel
// are summed through the one LDS block in r order, head 1 first, so dhead1 has head_backward_add's
// bits, and with g2 == 0 so has dz (fma(0, w2, x) == x; a -0 sum becomes +0).
template <int NT>
__global__ __launch_bounds__(NT) void head_backward_add2_kernel(HeadBackwardAdd2Args a) {
  __shared__ float w1_s[256];
  __shared__ float w2_s[256];
  __shared__ float g1_s[368];
  __shared__ float g2_s[368];
  __shared__ float red[16];
  __shared__ float part[NT * 8];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int HP = a.S + 2;
  for (int c = tid; c < a.C; c += NT) {
    w1_s[c] = c < a.C_real ? a.w1[c] : 0.f;
    w2_s[c] = c < a.C_real ? a.w2[c] : 0.f;
  }
  float gs1 = 0.f, gs2 = 0.f;
  for (int p = tid; p < SS; p += NT) {
    const float g1 = a.g1[(size_t)b * SS + p];
    const float g2 = a.g2[(size_t)b * SS + p];
    g1_s[p] = g1;
    g2_s[p] = g2;
    gs1 += g1;
    gs2 += g2;
  }
  __syncthreads();
  const int C8 = a.C >> 3;
  const int R = NT / C8;  // positions processed concurrently
  const int r = tid / C8, cg = tid - r * C8;
  const __bf16* base = a.y + (size_t)b * HP * HP * a.C;
  __bf16* dzb = a.dz + (size_t)b * HP * HP * a.C;
  float acc1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float acc2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (r < R) {
    const int c8 = cg << 3;
    constexpr int BU = 4;  // positions in flight per thread (two 16-B loads each)
    for (int p0 = r; p0 < SS; p0 += BU * R) {
      bf16x8 v[BU], d[BU];
      size_t off[BU];
#pragma unroll
      for (int u = 0; u < BU; ++u) {
        const int p = p0 + u * R;
        const int pc = p < SS ? p : SS - 1;
        const int i = pc / a.S, j = pc - (pc / a.S) * a.S;
        off[u] = (size_t)((i + 1) * HP + j + 1) * a.C + c8;
        v[u] = *(const bf16x8*)(base + off[u]);
        d[u] = *(const bf16x8*)(dzb + off[u]);
      }
#pragma unroll
      for (int u = 0; u < BU; ++u) {
        const int p = p0 + u * R;
        if (p < SS) {
          const float g1 = g1_s[p], g2 = g2_s[p];
          bf16x8 o = d[u];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float y = (float)v[u][e];
            if (y > 0.f)
              o[e] = (__bf16)__builtin_fmaf(g2, w2_s[c8 + e], __builtin_fmaf(g1, w1_s[c8 + e], (float)d[u][e]));
            acc1[e] += g1 * y;
            acc2[e] += g2 * y;
          }
          *(bf16x8*)(dzb + off[u]) = o;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[tid * 8 + e] = acc1[e];
  __syncthreads();
  float* dh1 = a.dhead1 + (size_t)b * (a.C_real + 1);
  for (int c = tid; c < a.C_real; c += NT) {
    const int g8 = c >> 3, e = c & 7;
    float s = 0.f;
    for (int rr = 0; rr < R; ++rr) s += part[(rr * C8 + g8) * 8 + e];
    dh1[c] = s;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 8; ++e) part[tid * 8 + e] = acc2[e];
  __syncthreads();
  float* dh2 = a.dhead2 + (size_t)b * (a.C_real + 1);
  for (int c = tid; c < a.C_real; c += NT) {
    const int g8 = c >> 3, e = c & 7;
    float s = 0.f;
    for (int rr = 0; rr < R; ++rr) s += part[(rr * C8 + g8) * 8 + e];
    dh2[c] = s;
  }
  gs1 = block_reduce_sum(gs1, red);
  gs2 = block_reduce_sum(gs2, red);
  if (tid == 0) {
    dh1[a.C_real] = gs1;
    dh2[a.C_real] = gs2;
  }
}

// head_backward_add's split
void launch_head_backward_add2(const HeadBackwardAdd2Args& a, hipStream_t st) {
  if (a.B < kHeadWideBelow) hipLaunchKernelGGL(head_backward_add2_kernel<1024>, dim3(a.B), dim3(1024), 0, st, a);
  else hipLaunchKernelGGL(head_backward_add2_kernel<256>, dim3(a.B), dim3(256), 0, st, a);
}

// policy_value_head_kernel (head_pv.hip) with a third dot row: the policy and value expressions are
// its own, in its order (probs and zv carry its bits).
template <int NT, class Board>
__global__ __launch_bounds__(NT) void policy_value_own_head_kernel(PolicyValueOwnHeadArgs ao) {
  const PolicyValueHeadArgs& a = ao.pv;
  __shared__ float wp_s[256];
  __shared__ float wv_s[256];
  __shared__ float wo_s[256];
  __shared__ float z_s[368];
  __shared__ float zv_s[368];
  __shared__ float zo_s[368];
  __shared__ float red[16];
  const int b = (int)gridDim.x - 1 - (int)blockIdx.x;  // policy_head_kernel's board order
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int HP = a.S + 2;
  for (int c = tid; c < a.C; c += NT) {
    wp_s[c] = c < a.C_real ? a.wp[c] : 0.f;
    wv_s[c] = c < a.C_real ? a.wv[c] : 0.f;
    wo_s[c] = c < a.C_real ? ao.wo[c] : 0.f;
  }
  Board board;
  board.load(a.y + (size_t)b * HP * HP * a.C, a.S, a.C);
  __syncthreads();
  const float bias = a.bp[0];
  const float vbias = a.bv[0];
  const float obias = ao.bo[0];
  const uint8_t* legal = a.legal ? a.legal + (size_t)b * SS : nullptr;

  board.dots(wp_s, z_s, a.S, a.C);
#pragma unroll
  for (int u = 0; u < Board::P; ++u) asm volatile("" : "+v"(board.v[u]));
  board.dots(wv_s, zv_s, a.S, a.C);
#pragma unroll
  for (int u = 0; u < Board::P; ++u) asm volatile("" : "+v"(board.v[u]));
  board.dots(wo_s, zo_s, a.S, a.C);
  for (int p = tid; p < SS; p += NT) {
    a.zv[(size_t)b * SS + p] = zv_s[p] + vbias;
    ao.own[(size_t)b * SS + p] = tanhf(zo_s[p] + obias);
  }

  float lmax = -INFINITY;
  for (int p = tid; p < SS; p += NT) {
    float z = z_s[p] + bias;
    if (legal && !legal[p]) z = -INFINITY;
    z_s[p] = z;
    if (z > lmax) lmax = z;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(lmax, o, 64);
    if (ov > lmax) lmax = ov;
  }
  if ((tid & 63) == 0) red[tid >> 6] = lmax;
  __syncthreads();
  lmax = red[0];
  for (int w = 1; w < NT / 64; ++w)
    if (red[w] > lmax) lmax = red[w];
  const float zmax = lmax;
  float ls = 0.f;
  for (int p = tid; p < SS; p += NT) ls += (z_s[p] == -INFINITY) ? 0.f : __expf(z_s[p] - zmax);
  const float sum = block_reduce_sum(ls, red);
  const float inv = 1.f / sum;
  for (int p = tid; p < SS; p += NT)
    a.probs[(size_t)b * SS + p] = (z_s[p] == -INFINITY) ? 0.f : __expf(z_s[p] - zmax) * inv;
}

void launch_policy_value_own_head(const PolicyValueOwnHeadArgs& a, hipStream_t st) {
  if (a.pv.B >= kHeadWideBelow && a.pv.S * (a.pv.C >> 3) <= 512)
    hipLaunchKernelGGL((policy_value_own_head_kernel<512, BoardRows<512>>), dim3(a.pv.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((policy_value_own_head_kernel<1024, BoardRegs<1024>>), dim3(a.pv.B), dim3(1024), 0, st, a);
}

}  // namespace agk
