// The two head kernels of the dual (policy + value) network, one trunk with two 1x1 heads.
//
// policy_value_head: the inference head.  One workgroup per board reads the board's activations from
// HBM once into registers (BoardRows / BoardRegs, policy_head.h) and takes both heads' dot products
// from them: the policy row goes through policy_head_kernel<false>'s masked softmax at temperature 1
// (the same expressions in the same order: policy_head_probs' bits), the value row plus its bias goes
// out as fp32 logits, the quantity head_logits produces for dense_f32 / value_out.
//
// head_backward_add: head_backward (head.hip) that adds the value head's ReLU'-masked dY into the dZ
// the policy head wrote, so the dual trainer runs every policy-head kernel unchanged and the trunk
// backward sees the sum of both heads' gradients.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "policy_head.h"

namespace agk {

template <int NT, class Board>
__global__ __launch_bounds__(NT) void policy_value_head_kernel(PolicyValueHeadArgs a) {
  __shared__ float wp_s[256];
  __shared__ float wv_s[256];
  __shared__ float z_s[368];
  __shared__ float zv_s[368];
  __shared__ float red[16];
  const int b = (int)gridDim.x - 1 - (int)blockIdx.x;  // policy_head_kernel's board order
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int HP = a.S + 2;
  for (int c = tid; c < a.C; c += NT) {
    wp_s[c] = c < a.C_real ? a.wp[c] : 0.f;
    wv_s[c] = c < a.C_real ? a.wv[c] : 0.f;
  }
  Board board;
  board.load(a.y + (size_t)b * HP * HP * a.C, a.S, a.C);
  __syncthreads();
  const float bias = a.bp[0];
  const float vbias = a.bv[0];
  const uint8_t* legal = a.legal ? a.legal + (size_t)b * SS : nullptr;

  // both heads from the one register copy of the board (dots ends with a barrier)
  board.dots(wp_s, z_s, a.S, a.C);
  // laundered: the second pass converts the packed bf16 again instead of keeping the first pass's
  // fp32 copies of the whole board live (BoardRegs<1024>: 96 more VGPRs, a spill past 128)
#pragma unroll
  for (int u = 0; u < Board::P; ++u) asm volatile("" : "+v"(board.v[u]));
  board.dots(wv_s, zv_s, a.S, a.C);
  for (int p = tid; p < SS; p += NT) a.zv[(size_t)b * SS + p] = zv_s[p] + vbias;

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

// policy_head_go's split: large batches whose rows fit 512 lanes run BoardRows<512>, the rest
// BoardRegs<1024>
void launch_policy_value_head(const PolicyValueHeadArgs& a, hipStream_t st) {
  if (a.B >= kHeadWideBelow && a.S * (a.C >> 3) <= 512)
    hipLaunchKernelGGL((policy_value_head_kernel<512, BoardRows<512>>), dim3(a.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((policy_value_head_kernel<1024, BoardRegs<1024>>), dim3(a.B), dim3(1024), 0, st, a);
}

// head_input_backward (head.hip) with a read-modify-write of dZ.  Where y > 0:
//   dz[p, c] = bf16_rne(fma(dlogits[p], w[c], float(dz[p, c])))
// one fused multiply-add in fp32 (a single rounding of g * w + dz), then the bf16 round-to-nearest-
// even.  Elsewhere the element keeps its bits; the border is never addressed.  The dW_head partials
// are head_input_backward's: thread (r, cg) adds g[p] * y[p, c] over p = r, r + R, ... in order, the R
// partials of a channel are summed through LDS in r order (the same bits as head_backward's dhead).
template <int NT>
__global__ __launch_bounds__(NT) void head_backward_add_kernel(PolicyHeadArgs a, const float* dlogits) {
  __shared__ float w_s[256];
  __shared__ float g_s[368];
  __shared__ float red[16];
  __shared__ float part[NT * 8];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int HP = a.S + 2;
  for (int c = tid; c < a.C; c += NT) w_s[c] = c < a.C_real ? a.w[c] : 0.f;
  float gs = 0.f;
  for (int p = tid; p < SS; p += NT) {
    const float g = dlogits[(size_t)b * SS + p];
    g_s[p] = g;
    gs += g;
  }
  __syncthreads();
  const int C8 = a.C >> 3;
  const int R = NT / C8;  // positions processed concurrently
  const int r = tid / C8, cg = tid - r * C8;
  const __bf16* base = a.y + (size_t)b * HP * HP * a.C;
  __bf16* dzb = a.dz + (size_t)b * HP * HP * a.C;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
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
          const float g = g_s[p];
          bf16x8 o = d[u];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float y = (float)v[u][e];
            if (y > 0.f) o[e] = (__bf16)__builtin_fmaf(g, w_s[c8 + e], (float)d[u][e]);
            acc[e] += g * y;
          }
          *(bf16x8*)(dzb + off[u]) = o;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[tid * 8 + e] = acc[e];
  __syncthreads();
  float* dh = a.dhead + (size_t)b * (a.C_real + 1);
  for (int c = tid; c < a.C_real; c += NT) {
    const int g8 = c >> 3, e = c & 7;
    float s = 0.f;
    for (int rr = 0; rr < R; ++rr) s += part[(rr * C8 + g8) * 8 + e];
    dh[c] = s;
  }
  gs = block_reduce_sum(gs, red);
  if (tid == 0) dh[a.C_real] = gs;
}

void launch_head_backward_add(const PolicyHeadArgs& a, const float* dlogits, hipStream_t st) {
  if (a.B < kHeadWideBelow) hipLaunchKernelGGL(head_backward_add_kernel<1024>, dim3(a.B), dim3(1024), 0, st, a, dlogits);
  else hipLaunchKernelGGL(head_backward_add_kernel<256>, dim3(a.B), dim3(256), 0, st, a, dlogits);
}

}  // namespace agk
