// The score head of the dual net: the fused output layer of its small MLP, in the shape of value_out (head.hip).
// upre (B, D) fp32 is dense_f32(pooled, sc1_w, bias = sc1_b); per board
//   u = max(upre, 0),  s = u . w2 + b2                       (s in units of S points)
// and, with a target t (the same unit), e = s - t, the Huber loss with threshold delta
//   loss = |e| <= delta ? 0.5 e^2 : delta (|e| - 0.5 delta),  abserr = |e|,
//   g = ((grad_scale * valid[b]) * weight[b]) * clamp(e, -delta, delta)
//   du[b, j] = upre[b, j] > 0 ? g * w2[j] : 0,  dout[b] = [g * u (D) | g]
// dout is the per-board partial row that head_grad_sums turns into [d sc2_w | d sc2_b]; d sc1_b is
// head_grad_sums over du.  Optionally (inference with a score utility) value[b] is rewritten in place as
//   (value[b] + lam * tanh(0.5 s)) / (1 + lam)               (0.5 s = score / (2 S))
//
// Mapping: one board per wave, four boards per 256-thread workgroup.  The whole head moves B * D * 4 bytes
// (139 KB at B = 2176, D = 64) and is launch-bound; a wave per board needs no LDS and no barrier, and D <= 512
// is at most 8 elements per lane.
// Rounding order of the dot product (fixed, no atomics: two runs give the same bits): lane i accumulates
// fmaf(u[j], w2[j], acc) over j = i, i + 64, i + 128, ... in ascending order from acc = 0; the 64 lane sums
// are combined by the xor butterfly with offsets 32, 16, 8, 4, 2, 1 (wave_sum); b2 is added last.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace agk {

constexpr int kScoreNT = 256;  // four waves, one board each

__global__ __launch_bounds__(kScoreNT) void score_out_kernel(ScoreOutArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (kScoreNT / 64) + (threadIdx.x >> 6);
  if (b >= a.B) return;  // wave-uniform: the shuffles below run on whole waves
  const int D = a.D;
  const float* up = a.upre + (size_t)b * D;
  float acc = 0.f;
  for (int j = lane; j < D; j += 64) {
    const long long i = bounds_at((long long)b * D + j, a.upre_elems);
    acc = fmaf(fmaxf(a.upre[i], 0.f), a.w2[j], acc);
  }
  const float s = wave_sum(acc) + a.b2[0];
  if (lane == 0) {
    a.s[b] = s;
    if (a.value) {
      const float v = a.value[b];
      a.value[b] = (v + a.lam * tanhf(0.5f * s)) / (1.f + a.lam);
    }
  }
  if (!a.target) return;
  const float e = s - a.target[b];
  const float ae = fabsf(e);
  if (lane == 0) {
    a.loss[b] = ae <= a.delta ? 0.5f * e * e : a.delta * (ae - 0.5f * a.delta);
    a.abserr[b] = ae;
  }
  float gs = a.grad_scale;
  if (a.valid) gs *= a.valid[b];
  if (a.weight) gs *= a.weight[b];
  const float g = gs * fminf(fmaxf(e, -a.delta), a.delta);
  float* dp = a.dout + bounds_at((long long)b * (D + 1), a.dout_elems);
  for (int j = lane; j < D; j += 64) {
    const float x = up[j];
    const long long i = bounds_at((long long)b * D + j, a.du_elems);
    a.du[i] = x > 0.f ? g * a.w2[j] : 0.f;
    if (AGK_BOUNDS_CHECK((long long)b * (D + 1) + j < a.dout_elems)) dp[j] = g * fmaxf(x, 0.f);
  }
  if (lane == 0 && AGK_BOUNDS_CHECK((long long)b * (D + 1) + D < a.dout_elems)) dp[D] = g;
}

void launch_score_out(const ScoreOutArgs& a, hipStream_t st) {
  if (a.D % 8 || a.D < 8 || a.D > 512 || a.B < 1)
    throw std::invalid_argument("score_out: D must be a multiple of 8 in 8..512 and B >= 1");
  const int per = kScoreNT / 64;
  hipLaunchKernelGGL(score_out_kernel, dim3((a.B + per - 1) / per), dim3(kScoreNT), 0, st, a);
  bounds_debug_check("score_out", st);
}

}  // namespace agk
