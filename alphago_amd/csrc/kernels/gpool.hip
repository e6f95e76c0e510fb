// Global pooling branch of the residual trunk (ConvStack gpool): five memory-bound kernels over the
// zero-bordered NHWC bf16 activations (B, S + 2, S + 2, C), border 1.  They read and write interior pixels
// only.  The gate's dense layer and its two backward products run on dense_f32.
//  * gpool_fwd: per board and channel the sum over the S * S pixels times inv, and (FULL) the maximum and
//    the lowest pixel index r * S + col attaining it.  FULL = false is the backward's column sum
//    dg[b, c] = sum_p dZ[b, p, c]: the same loop and the same summation order, no second implementation.
//  * gpool_bias_add: out = bf16(float(skip) + g[b, c]), the per-board bias folded into a block's skip
//    operand; out may be skip itself.
//  * gpool_bwd_fill: the gradient of the pooling with respect to its input,
//    out = bf16(dp[b, 0, c] * inv + (p == argmax[b, c] ? dp[b, 1, c] : 0)), two fp32 roundings.
//  * gpool_bwd_add_masked (the pass head of the dual net): that gradient for dp[b, k, c] = dpass[b] * w[k, c],
//    added into an existing dZ where the pooled activation is positive; a kernel of its own at the end of the file.
//  * gpool_bwd_add_masked_dp (the score head): the same accumulation for a general dp (B, 2, C), optionally with
//    the pass head's addend in the same pass; the last kernel of the file.
// Summation order of gpool_fwd (fixed, no atomics): thread (pg, cg) owns the 8 channels 8 cg .. 8 cg + 7
// and adds the pixels pg, pg + PG, pg + 2 PG, ... in that order; then thread c adds the PG partials of
// channel c in pg order.  Two runs give the same bits.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace agk {

// Debug build: every 16-byte activation access is checked against the tensor's extent (AGK_BOUNDS_CHECK,
// common.h); a violation redirects the access to element 0, and the launchers wait and raise on it.

constexpr int kGpoolNT = 512;          // threads of a gpool_fwd workgroup
constexpr int kGpoolSlots = 8 * kGpoolNT;  // PG * C <= 8 * NT partials per quantity

// element offset of channel 0 of interior pixel p of board b
__device__ __forceinline__ int64_t gpool_pixel(int b, int p, int S, int C) {
  const int HP = S + 2;
  const int i = p / S, j = p - i * S;
  return ((int64_t)(b * HP + i + 1) * HP + j + 1) * C;
}

// One workgroup per board.  tid = pg * C8 + cg (C8 = C / 8 16-byte channel groups, PG = NT / C8 pixel
// groups; the threads past PG * C8 only take part in the barriers).
template <bool FULL>
__global__ __launch_bounds__(kGpoolNT) void gpool_fwd_kernel(GpoolFwdArgs a) {
  __shared__ float s_sum[kGpoolSlots];
  __shared__ float s_max[FULL ? kGpoolSlots : 1];
  __shared__ int s_arg[FULL ? kGpoolSlots : 1];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int C = a.C, C8 = C >> 3, NP = a.S * a.S;
  const int PG = kGpoolNT / C8;
  const int pg = tid / C8, cg = tid - pg * C8;
  if (pg < PG) {
    float sum[8], mx[8];
    int arg[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sum[e] = 0.f;
      mx[e] = -INFINITY;
      arg[e] = 0;
    }
#pragma unroll 4
    for (int p = pg; p < NP; p += PG) {
      int64_t o = gpool_pixel(b, p, a.S, C) + cg * 8;
      if (!AGK_BOUNDS_CHECK(o >= 0 && o + 8 <= a.y_elems)) o = 0;
      const bf16x8 v = *(const bf16x8*)(a.y + o);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = bf2f(v[e]);
        sum[e] += f;
        if (FULL && f > mx[e]) {  // ascending p: the first pixel attaining the maximum stays
          mx[e] = f;
          arg[e] = p;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int s = pg * C + cg * 8 + e;
      s_sum[s] = sum[e];
      if (FULL) {
        s_max[s] = mx[e];
        s_arg[s] = arg[e];
      }
    }
  }
  __syncthreads();
  if (tid < C) {
    float sum = s_sum[tid];
    float mx = FULL ? s_max[tid] : 0.f;
    int arg = FULL ? s_arg[tid] : 0;
    for (int g = 1; g < PG; ++g) {
      const int s = g * C + tid;
      sum += s_sum[s];
      if (FULL) {
        const float m = s_max[s];
        const int r = s_arg[s];
        if (m > mx || (m == mx && r < arg)) {
          mx = m;
          arg = r;
        }
      }
    }
    if (FULL) {
      a.pooled[((size_t)b * 2 + 0) * C + tid] = sum * a.inv;
      a.pooled[((size_t)b * 2 + 1) * C + tid] = mx;
      a.argmax[(size_t)b * C + tid] = arg;
    } else {
      a.pooled[(size_t)b * C + tid] = sum * a.inv;
    }
  }
}

void launch_gpool_fwd(const GpoolFwdArgs& a, hipStream_t st) {
  if (a.C % 8 || a.C < 8 || a.C > kGpoolNT || a.B < 1)
    throw std::invalid_argument("gpool_fwd: C must be a multiple of 8 in 8..512 and B >= 1");
  if (a.argmax) hipLaunchKernelGGL(gpool_fwd_kernel<true>, dim3(a.B), dim3(kGpoolNT), 0, st, a);
  else hipLaunchKernelGGL(gpool_fwd_kernel<false>, dim3(a.B), dim3(kGpoolNT), 0, st, a);
  bounds_debug_check("gpool_fwd", st);
}

// The two elementwise kernels.  Workgroup (b, s) covers board b; thread (pg, cg) as in gpool_fwd keeps the 8
// per-channel operands of its channel group in registers (g, or dp * inv, dp[1] and the argmax: they do not
// depend on the pixel) and walks the pixels pg + PG * s, pg + PG * (s + gridDim.y), ...: one 16-byte load
// (bias add) and one 16-byte store per pixel, consecutive threads on consecutive bytes.  gridDim.y splits a
// board's pixels over several workgroups when there are few boards.  FILL = false: bias add; true: backward fill.
template <bool FILL>
__global__ __launch_bounds__(kGpoolNT) void gpool_map_kernel(GpoolMapArgs a) {
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int C = a.C, C8 = C >> 3, NP = a.S * a.S;
  const int PG = kGpoolNT / C8;
  const int pg = tid / C8, cg = tid - pg * C8;
  if (pg >= PG) return;
  float v0[8], v1[8];
  int am[8];
  bf16x8 base;
  if (FILL) {
    const float* d0 = a.g + ((size_t)b * 2 + 0) * C + cg * 8;
    const float* d1 = a.g + ((size_t)b * 2 + 1) * C + cg * 8;
    const int* ap = a.argmax + (size_t)b * C + cg * 8;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 x0 = *(const f32x4*)(d0 + 4 * h), x1 = *(const f32x4*)(d1 + 4 * h);
      const int4 xa = *(const int4*)(ap + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v0[4 * h + e] = __fmul_rn(x0[e], a.inv);
        v1[4 * h + e] = x1[e];
      }
      am[4 * h + 0] = xa.x; am[4 * h + 1] = xa.y; am[4 * h + 2] = xa.z; am[4 * h + 3] = xa.w;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) base[e] = f2bf(__fadd_rn(v0[e], 0.f));  // every pixel but the argmax
  } else {
    const float* g = a.g + (size_t)b * C + cg * 8;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 x = *(const f32x4*)(g + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) v0[4 * h + e] = x[e];
    }
  }
#pragma unroll 4
  for (int p = pg + PG * blockIdx.y; p < NP; p += PG * gridDim.y) {
    int64_t o = gpool_pixel(b, p, a.S, C) + cg * 8;
    if (!AGK_BOUNDS_CHECK(o >= 0 && o + 8 <= a.elems)) o = 0;
    bf16x8 r;
    if (FILL) {
      r = base;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (am[e] == p) r[e] = f2bf(__fadd_rn(v0[e], v1[e]));
    } else {
      const bf16x8 v = *(const bf16x8*)(a.skip + o);
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = f2bf(bf2f(v[e]) + v0[e]);
    }
    *(bf16x8*)(a.out + o) = r;
  }
}

void launch_gpool_map(const GpoolMapArgs& a, bool fill, hipStream_t st) {
  if (a.C % 8 || a.C < 8 || a.C > kGpoolNT || a.B < 1)
    throw std::invalid_argument("gpool: C must be a multiple of 8 in 8..512 and B >= 1");
  // about 512 workgroups at least: few boards are split over up to 8 workgroups each
  int ny = (512 + a.B - 1) / a.B;
  ny = ny > 8 ? 8 : ny;
  if (fill) hipLaunchKernelGGL(gpool_map_kernel<true>, dim3(a.B, ny), dim3(kGpoolNT), 0, st, a);
  else hipLaunchKernelGGL(gpool_map_kernel<false>, dim3(a.B, ny), dim3(kGpoolNT), 0, st, a);
  bounds_debug_check(fill ? "gpool_bwd_fill" : "gpool_bias_add", st);
}

// The pass head's pooling gradient added into the dZ of the trunk's top layer (gpool_map_kernel's layout, a
// read-modify-write).  With dP[b, k, c] = dpass[b] * w[k, c] and y the top layer's output after its ReLU:
//   dz[b, p, c] = bf16(float(dz[b, p, c]) + (dP[b, 0, c] * inv + (p == argmax[b, c] ? dP[b, 1, c] : 0)))  where y > 0
// every product and sum an fp32 rounding of its own (no FMA); where y <= 0 the element keeps its bits.
__global__ __launch_bounds__(kGpoolNT) void gpool_bwd_add_masked_kernel(GpoolBwdAddArgs a) {
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int C = a.C, C8 = C >> 3, NP = a.S * a.S;
  const int PG = kGpoolNT / C8;
  const int pg = tid / C8, cg = tid - pg * C8;
  if (pg >= PG) return;
  float v0[8], v01[8];
  int am[8];
  const float g = a.dpass[b];
  const float* w0 = a.w + cg * 8;
  const float* w1 = a.w + C + cg * 8;
  const int* ap = a.argmax + (size_t)b * C + cg * 8;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int4 xa = *(const int4*)(ap + 4 * h);
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // dword loads: w may be a view into the flat parameters at any 4-byte offset
      v0[4 * h + e] = __fmul_rn(__fmul_rn(g, w0[4 * h + e]), a.inv);
      v01[4 * h + e] = __fadd_rn(v0[4 * h + e], __fmul_rn(g, w1[4 * h + e]));  // the argmax pixel's addend
    }
    am[4 * h + 0] = xa.x; am[4 * h + 1] = xa.y; am[4 * h + 2] = xa.z; am[4 * h + 3] = xa.w;
  }
#pragma unroll 4
  for (int p = pg + PG * blockIdx.y; p < NP; p += PG * gridDim.y) {
    int64_t o = gpool_pixel(b, p, a.S, C) + cg * 8;
    if (!AGK_BOUNDS_CHECK(o >= 0 && o + 8 <= a.elems)) o = 0;
    const bf16x8 v = *(const bf16x8*)(a.y + o);
    bf16x8 r = *(const bf16x8*)(a.dz + o);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (bf2f(v[e]) > 0.f) r[e] = f2bf(__fadd_rn(bf2f(r[e]), am[e] == p ? v01[e] : v0[e]));
    *(bf16x8*)(a.dz + o) = r;
  }
}

void launch_gpool_bwd_add_masked(const GpoolBwdAddArgs& a, hipStream_t st) {
  if (a.C % 8 || a.C < 8 || a.C > kGpoolNT || a.B < 1)
    throw std::invalid_argument("gpool_bwd_add_masked: C must be a multiple of 8 in 8..512 and B >= 1");
  int ny = (512 + a.B - 1) / a.B;  // launch_gpool_map's split
  ny = ny > 8 ? 8 : ny;
  hipLaunchKernelGGL(gpool_bwd_add_masked_kernel, dim3(a.B, ny), dim3(kGpoolNT), 0, st, a);
  bounds_debug_check("gpool_bwd_add_masked", st);
}

// The pooling gradient of a general dP (B, 2, C) added into the dZ of the trunk's top layer, gpool_bwd_add_masked's
// layout and workgroup split: one 16-byte load of y and of dz and one 16-byte store per 8 channels.  With
//   q[b, p, c] = dP[b, 0, c] * inv + (p == argmax[b, c] ? dP[b, 1, c] : 0)
// and, when dpass / w are given (the pass head's term, gpool_bwd_add_masked's addend),
//   r0 = (dpass[b] * w[0, c]) * inv,   r[b, p, c] = p == argmax[b, c] ? fma(dpass[b], w[1, c], r0) : r0,   add = r + q
// (add = q without them):
//   dz[b, p, c] = bf16(float(dz[b, p, c]) + add)   where y > 0 and add != 0
// every product and sum an fp32 rounding of its own: the products that feed a sum pass through rounded_product,
// which keeps the compiler from contracting them, and the one fused multiply-add is written out.  It is there because gpool_bwd_add_masked's compiled code has it (its source leaves
// the contraction of dpass * w[1, c] into the sum to the compiler, which fuses it), and r must carry that kernel's
// bits for a net with both heads to get the dZ of a pass-only net.  Elements with y <= 0 keep their bits, and so
// do elements whose addend is zero (a silent head leaves dZ as it found it, the sign of a zero included).
__device__ __forceinline__ float rounded_product(float x, float y) {
  float p = x * y;
  asm("" : "+v"(p));  // opaque to the optimiser: a later sum cannot absorb the product into a fused multiply-add
  return p;
}

__global__ __launch_bounds__(kGpoolNT) void gpool_bwd_add_masked_dp_kernel(GpoolBwdAddDpArgs a) {
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int C = a.C, C8 = C >> 3, NP = a.S * a.S;
  const int PG = kGpoolNT / C8;
  const int pg = tid / C8, cg = tid - pg * C8;
  if (pg >= PG) return;
  float v0[8], v01[8];
  int am[8];
  const float* d0 = a.dp + ((size_t)b * 2) * C + cg * 8;
  const float* d1 = d0 + C;
  const int* ap = a.argmax + (size_t)b * C + cg * 8;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int4 xa = *(const int4*)(ap + 4 * h);
    const float4 x0 = *(const float4*)(d0 + 4 * h);
    const float4 x1 = *(const float4*)(d1 + 4 * h);
    const float q0[4] = {x0.x, x0.y, x0.z, x0.w}, q1[4] = {x1.x, x1.y, x1.z, x1.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v0[4 * h + e] = rounded_product(q0[e], a.inv);
      v01[4 * h + e] = __fadd_rn(v0[4 * h + e], q1[e]);
    }
    am[4 * h + 0] = xa.x; am[4 * h + 1] = xa.y; am[4 * h + 2] = xa.z; am[4 * h + 3] = xa.w;
  }
  if (a.dpass) {
    const float g = a.dpass[b];
    const float* w0 = a.w + cg * 8;
    const float* w1 = a.w + C + cg * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {  // dword loads: w may be a view into the flat parameters at any 4-byte offset
      const float r0 = rounded_product(rounded_product(g, w0[e]), a.inv);
      const float r01 = __builtin_fmaf(g, w1[e], r0);  // gpool_bwd_add_masked's argmax addend, as compiled
      v0[e] = __fadd_rn(r0, v0[e]);
      v01[e] = __fadd_rn(r01, v01[e]);
    }
  }
#pragma unroll 4
  for (int p = pg + PG * blockIdx.y; p < NP; p += PG * gridDim.y) {
    int64_t o = gpool_pixel(b, p, a.S, C) + cg * 8;
    if (!AGK_BOUNDS_CHECK(o >= 0 && o + 8 <= a.elems)) o = 0;
    const bf16x8 v = *(const bf16x8*)(a.y + o);
    bf16x8 r = *(const bf16x8*)(a.dz + o);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float add = am[e] == p ? v01[e] : v0[e];
      if (bf2f(v[e]) > 0.f && add != 0.f) r[e] = f2bf(__fadd_rn(bf2f(r[e]), add));
    }
    *(bf16x8*)(a.dz + o) = r;
  }
}

void launch_gpool_bwd_add_masked_dp(const GpoolBwdAddDpArgs& a, hipStream_t st) {
  if (a.C % 8 || a.C < 8 || a.C > kGpoolNT || a.B < 1)
    throw std::invalid_argument("gpool_bwd_add_masked_dp: C must be a multiple of 8 in 8..512 and B >= 1");
  int ny = (512 + a.B - 1) / a.B;  // launch_gpool_map's split
  ny = ny > 8 ? 8 : ny;
  hipLaunchKernelGGL(gpool_bwd_add_masked_dp_kernel, dim3(a.B, ny), dim3(kGpoolNT), 0, st, a);
  bounds_debug_check("gpool_bwd_add_masked_dp", st);
}

}  // namespace agk
