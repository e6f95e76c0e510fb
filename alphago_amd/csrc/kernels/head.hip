// Fused policy head: 1x1 conv (F -> 1, scalar bias) + flatten + softmax over
// S*S + clipped categorical cross-entropy + top-1 accuracy + the whole backward
// of the head (dlogits, the ReLU-masked gradient into the last trunk layer, and
// per-board partials of the head weight/bias gradients).  One workgroup per
// board: the board's 361 x F activations are read from HBM once into registers
// (BoardRows / BoardRegs), and nothing of the head round-trips through HBM as a
// separate tensor.  The kernel template and the blocks it is made of are in
// policy_head.h; this file instantiates the plain kernels and holds the streaming
// kernels of the value net's head (head_logits, head_backward: head_dots,
// head_input_backward) with value_out and head_grad_sums.
//
// Reference ops replaced: policy.py:145-154 (Conv 1x1 / Flatten / Softmax),
// Keras categorical_crossentropy with output clipping (supervised_policy_trainer
// .py:200) and the 'accuracy' metric; inference renormalisation over legal
// moves replaces CNNPolicy._select_moves_and_normalize (policy.py:44-54).
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "policy_head.h"

namespace agk {

// z_s[p] = y[p, :] . w for every position of one board, coalesced and
// deterministic: each 32-lane half-wave owns one position at a time, lane c8
// (< C/8) reads 16 B of the position's row (one contiguous row per half-wave)
// and the 8-term partial dot products are summed with a fixed xor-shuffle tree.
__device__ __forceinline__ void head_dots(const __bf16* base, const float* w_s, float* z_s, int S, int C) {
  const int tid = threadIdx.x;
  const int SS = S * S;
  const int HP = S + 2;
  const int C8 = C >> 3;  // <= 32
  const int R = blockDim.x >> 5;
  const int l32 = tid & 31, slot = tid >> 5;
  const int c8 = l32 << 3;
  // HU rows in flight per half-wave: the loop is bound by load latency (one
  // workgroup per board, every workgroup resident at once), not bandwidth
  constexpr int HU = 8;
  for (int p0 = 0; p0 < SS; p0 += HU * R) {
    bf16x8 v[HU];
#pragma unroll
    for (int u = 0; u < HU; ++u) {
      const int p = p0 + u * R + slot;
      if (p < SS && l32 < C8) {
        const int i = p / S, j = p - (p / S) * S;
        v[u] = *(const bf16x8*)(base + (size_t)((i + 1) * HP + j + 1) * C + c8);
      } else {
        v[u] = bf16x8{};
      }
    }
#pragma unroll
    for (int u = 0; u < HU; ++u) {
      const int p = p0 + u * R + slot;
      float d = 0.f;
      if (l32 < C8) {  // w_s holds only the C real slots: lanes past them must not read it
#pragma unroll
        for (int e = 0; e < 8; ++e) d += (float)v[u][e] * w_s[c8 + e];
      }
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
      if (l32 == 0 && p < SS) z_s[p] = d;
    }
  }
  __syncthreads();
}

// Gradient of a 1x1 (F -> 1) head conv given dlogits g (in g_s, length S*S):
// ReLU'-masked dY into the trunk's last activation and per-board partials of
// dW_head (the dbias partial is written by the caller).
template <int NT>
__device__ __forceinline__ void head_input_backward(const PolicyHeadArgs& a, int b, const __bf16* base,
                                                    const float* w_s, const float* g_s) {
  // One pass over the board's activations (head_walk_positions, eight positions in flight): the
  // ReLU'-masked dY is written and sum_p g[p] * y[p, c] accumulated in registers; the R partials per
  // channel are then reduced through LDS.
  __shared__ float part[NT * 8];
  const int tid = threadIdx.x;
  const int HP = a.S + 2;
  const int C8 = a.C >> 3;
  const int c8 = (tid % C8) << 3;
  __bf16* dzb = a.dz + (size_t)b * HP * HP * a.C;
  uint8_t* dz8b = a.dz8 ? a.dz8 + (size_t)b * HP * HP * a.C : nullptr;
  const float sc8 = a.dz8 ? *a.dz8_scale : 0.f;
  float m8 = 0.f;  // max |bf16 dY| (e5m2 output)
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  head_walk_positions<NT, 8, false>(base, nullptr, a.S, a.C, [&](int p, size_t off, const bf16x8& v, const bf16x8&) {
    const float g = g_s[p];
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float y = (float)v[e];
      o[e] = (__bf16)(y > 0.f ? g * w_s[c8 + e] : 0.f);
      acc[e] += g * y;
    }
    if (dz8b) {
      // quantize_bf8_dev_kernel's conversion of the bf16 value: the same bytes and max, and the
      // bf16 dz is never written or re-read
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        f[e] = (float)o[e];
        m8 = fmaxf(m8, fabsf(f[e]));
        f[e] = fminf(fmaxf(f[e] * sc8, -57344.f), 57344.f);
      }
      int lo = __builtin_amdgcn_cvt_pk_bf8_f32(f[0], f[1], 0, false);
      lo = __builtin_amdgcn_cvt_pk_bf8_f32(f[2], f[3], lo, true);
      int hi = __builtin_amdgcn_cvt_pk_bf8_f32(f[4], f[5], 0, false);
      hi = __builtin_amdgcn_cvt_pk_bf8_f32(f[6], f[7], hi, true);
      *(int2*)(dz8b + off) = make_int2(lo, hi);
    } else {
      *(bf16x8*)(dzb + off) = o;
    }
  });
  if (dz8b) {  // one atomic per board into the spread amax slots
    __shared__ float red8[NT / 64];
    m8 = wave_max(m8);
    if ((tid & 63) == 0) red8[tid >> 6] = m8;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < NT / 64; ++w) m8 = fmaxf(m8, red8[w]);
      if (m8 > 0.f) atomicMax(a.dz8_amax + (b & (kFp8AmaxSlots - 1)), __float_as_uint(m8));
    }
  }
  head_channel_sums<NT>(part, acc, a.dhead + (size_t)b * (a.C_real + 1), a.C_real, C8, NT / C8);
}

// Head logits only: z[b][p] = y[b,p,:] . w + bias (value-net head input,
// value.py:23-26); the board's activations are read once.
template <int NT>
__global__ __launch_bounds__(NT) void head_logits_kernel(PolicyHeadArgs a) {
  __shared__ float w_s[256];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int HP = a.S + 2;
  head_stage_weights<NT>({w_s}, {a.w}, a.C, a.C_real);
  __syncthreads();
  __shared__ float z_s[368];
  const __bf16* base = a.y + (size_t)b * HP * HP * a.C;
  const float bias = a.b[0];
  head_dots(base, w_s, z_s, a.S, a.C);
  for (int p = tid; p < SS; p += NT) a.probs[(size_t)b * SS + p] = z_s[p] + bias;  // probs slot carries the logits
}

// Head backward from an externally computed dlogits (value net: dz = dh W1^T).
template <int NT>
__global__ __launch_bounds__(NT) void head_backward_kernel(PolicyHeadArgs a, const float* dlogits) {
  __shared__ float w_s[256];
  __shared__ float g_s[368];
  __shared__ float red[16];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int HP = a.S + 2;
  head_stage_weights<NT>({w_s}, {a.w}, a.C, a.C_real);
  float gs = 0.f;
  for (int p = tid; p < SS; p += NT) {
    const float g = dlogits[(size_t)b * SS + p];
    g_s[p] = g;
    gs += g;
  }
  __syncthreads();
  head_input_backward<NT>(a, b, a.y + (size_t)b * HP * HP * a.C, w_s, g_s);
  head_bias_grad(gs, red, a.dhead + (size_t)b * (a.C_real + 1) + a.C_real);
}

// Value output layer: v = tanh(h . w2 + b2) (value.py:28-29) and, with
// targets, MSE loss (v - t)^2, sign agreement, dv = 2 (v - t)(1 - v^2) * scale
// * weight[b], dh = dv w2 and per-board partials [dw2 | db2].  One workgroup
// per board, one thread per dense unit.
__global__ __launch_bounds__(256) void value_out_kernel(ValueOutArgs a) {
  __shared__ float red[8];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  float s = 0.f;
  for (int j = tid; j < a.D; j += 256) s += a.h[(size_t)b * a.D + j] * a.w2[j];
  s = block_reduce_sum(s, red);
  const float v = tanhf(s + a.b2[0]);
  if (tid == 0) a.v[b] = v;
  if (!a.target) return;
  const float t = a.target[b];
  const float e = v - t;
  if (tid == 0) {
    a.loss[b] = e * e;
    a.correct[b] = (v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f)) == (t > 0.f ? 1.f : (t < 0.f ? -1.f : 0.f)) ? 1.f : 0.f;
  }
  const float dv = 2.f * e * (1.f - v * v) * a.grad_scale * (a.weight ? a.weight[b] : 1.f);
  float* dp = a.dout + (size_t)b * (a.D + 1);
  for (int j = tid; j < a.D; j += 256) {
    a.dh[(size_t)b * a.D + j] = dv * a.w2[j];
    dp[j] = dv * a.h[(size_t)b * a.D + j];
  }
  if (tid == 0) dp[a.D] = dv;
}

// Column sums of the per-board head partials (dhead [B][N]) into the flat gradient, plus the two
// per-board metric vectors (loss, correct) into sums[0..1]: one launch instead of three library
// reductions.  One workgroup per column; each thread sums rows tid, tid + 256, ... in order, then a
// fixed tree (deterministic).
__global__ __launch_bounds__(256) void head_grad_sums_kernel(const float* dhead, int B, int N, const float* loss,
                                                            const float* correct, float* grad, float* sums) {
  __shared__ float red[4];
  const int col = blockIdx.x;
  const float* src = col < N ? dhead + col : (col == N ? loss : correct);
  const int stride = col < N ? N : 1;
  float s = 0.f;
  for (int r = threadIdx.x; r < B; r += 256) s += src[(size_t)r * stride];
  s = block_reduce_sum(s, red);
  if (threadIdx.x == 0) {
    if (col < N) grad[col] = s;
    else sums[col - N] = s;
  }
}

void launch_head_grad_sums(const float* dhead, int B, int N, const float* loss, const float* correct, float* grad,
                           float* sums, hipStream_t st) {
  hipLaunchKernelGGL(head_grad_sums_kernel, dim3(N + 2), dim3(256), 0, st, dhead, B, N, loss, correct, grad, sums);
}

void launch_head_logits(const PolicyHeadArgs& a, hipStream_t st) {
  if (head_wide_block(a.B)) hipLaunchKernelGGL(head_logits_kernel<1024>, dim3(a.B), dim3(1024), 0, st, a);
  else hipLaunchKernelGGL(head_logits_kernel<256>, dim3(a.B), dim3(256), 0, st, a);
}
void launch_head_backward(const PolicyHeadArgs& a, const float* dlogits, hipStream_t st) {
  if (head_wide_block(a.B)) hipLaunchKernelGGL(head_backward_kernel<1024>, dim3(a.B), dim3(1024), 0, st, a, dlogits);
  else hipLaunchKernelGGL(head_backward_kernel<256>, dim3(a.B), dim3(256), 0, st, a, dlogits);
}
void launch_value_out(const ValueOutArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(value_out_kernel, dim3(a.B), dim3(256), 0, st, a);
}

void launch_policy_head(const PolicyHeadArgs& a, bool train, hipStream_t st) {
  // the regularised variants only when something asks for them: the SL step runs the plain kernels
  // (head_reg.hip: a module of their own, so that these kernels' code objects do not depend on them)
  const bool reg = a.stats || a.ref_probs || a.ent_coef != 0.f || a.kl_coef != 0.f;
  if (reg) launch_policy_head_reg(a, train, st);
  else if (train) policy_head_go<true, false>(a, st);
  else policy_head_go<false, false>(a, st);
}

}  // namespace agk
