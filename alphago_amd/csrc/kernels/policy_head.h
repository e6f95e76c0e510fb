// The fused policy head kernel (see head.hip) as a template, shared by the two translation units
// that instantiate it: head.hip holds the plain kernels of the SL / RL step, head_reg.hip the
// regularised variants (REG).  They are compiled apart so that the plain kernels' code objects do
// not depend on the variants' presence (LDS variables are laid out per module).
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace agk {

// boards below which the per-board head kernels run 1024 threads per workgroup instead of 256
constexpr int kHeadWideBelow = 256;

__device__ __forceinline__ float block_reduce_max(float v, float* red) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = fmaxf(r, red[i]);
  return r;
}
__device__ __forceinline__ float block_reduce_sum(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += red[i];
  return r;
}

// One board's interior activations held in registers between the policy head's forward and
// backward passes, so the board is read from HBM once (head_dots + head_input_backward read it
// twice).  Half-wave `slot` owns positions slot, slot + R, ... (R = NT / 32); lane l32 < C / 8 owns
// the 16-byte channel group l32 of each.  P = ceil(361 / R) covers every board up to 19 x 19.
template <int NT>
struct BoardRegs {
  static constexpr int R = NT / 32;
  static constexpr int P = (361 + R - 1) / R;
  bf16x8 v[P];

  __device__ __forceinline__ static size_t offset(int p, int S, int C, int c8) {
    const int i = p / S, j = p - i * S;
    return (size_t)((i + 1) * (S + 2) + j + 1) * C + c8;
  }

  // every load issued before any is used: P outstanding 16-B loads per lane
  __device__ __forceinline__ void load(const __bf16* base, int S, int C) {
    const int l32 = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const int SS = S * S;
    const bool lane = l32 < (C >> 3);
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int p = u * R + slot;
      v[u] = (p < SS && lane) ? *(const bf16x8*)(base + offset(p, S, C, l32 << 3)) : bf16x8{};
    }
  }

  // z_s[p] = y[p, :] . w with head_dots' xor-shuffle order (same bits)
  __device__ __forceinline__ void dots(const float* w_s, float* z_s, int S, int C) const {
    const int l32 = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const int SS = S * S;
    const int c8 = l32 << 3;
    const bool lane = l32 < (C >> 3);
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int p = u * R + slot;
      float d = 0.f;
      if (lane) {
#pragma unroll
        for (int e = 0; e < 8; ++e) d += (float)v[u][e] * w_s[c8 + e];
      }
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
      if (l32 == 0 && p < SS) z_s[p] = d;
    }
    __syncthreads();
  }

  // ReLU'-masked dY = g[p] w into the trunk's last activation gradient and per-board partials of
  // dW_head (sum_p g[p] y[p, c], slot partials summed through LDS in slot order)
  __device__ __forceinline__ void backward(const PolicyHeadArgs& a, int b, const float* w_s,
                                           const float* g_s) const {
    __shared__ float part[NT * 8];
    const int tid = threadIdx.x;
    // laundered so the store addresses are recomputed here instead of kept live from load()
    // (23 x 64-bit addresses would push the 512-thread kernel past 128 VGPRs)
    int lane_id = tid;
    asm volatile("" : "+v"(lane_id));
    const int l32 = lane_id & 31, slot = lane_id >> 5;
    const int SS = a.S * a.S;
    const int c8 = l32 << 3;
    const bool lane = l32 < (a.C >> 3);
    __bf16* dzb = a.dz + (size_t)b * (a.S + 2) * (a.S + 2) * a.C;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float wl[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) wl[e] = lane ? w_s[c8 + e] : 0.f;
#pragma unroll
    for (int u = 0; u < P; ++u) {
      const int p = u * R + slot;
      if (p < SS && lane) {
        const float g = g_s[p];
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float y = (float)v[u][e];
          o[e] = (__bf16)(y > 0.f ? g * wl[e] : 0.f);
          acc[e] += g * y;
        }
        *(bf16x8*)(dzb + offset(p, a.S, a.C, c8)) = o;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[tid * 8 + e] = acc[e];
    __syncthreads();
    float* dh = a.dhead + (size_t)b * (a.C_real + 1);
    for (int c = tid; c < a.C_real; c += NT) {
      const int g8 = c >> 3, e = c & 7;
      float s = 0.f;
      for (int r = 0; r < R; ++r) s += part[(r * 32 + g8) * 8 + e];
      dh[c] = s;
    }
  }
};

// The same for large batches with fewer registers: thread t < S * C / 8 owns 16-byte chunk t of
// every board row (a row's interior is contiguous in the padded layout), so the 19 loads of a lane
// differ by one uniform row stride and no per-load address stays live.  A position's dot product
// is the fixed-order sum of its C / 8 lanes' partials through LDS.  Needs S * C / 8 <= NT.
template <int NT>
struct BoardRows {
  static constexpr int P = 19;
  bf16x8 v[P];

  __device__ __forceinline__ static size_t offset(int u, int S, int C, int t) {
    return (size_t)((u + 1) * (S + 2) + 1) * C + t * 8;
  }

  __device__ __forceinline__ void load(const __bf16* base, int S, int C) {
    const int t = threadIdx.x;
    const bool lane = t < S * (C >> 3);
#pragma unroll
    for (int u = 0; u < P; ++u) v[u] = (u < S && lane) ? *(const bf16x8*)(base + offset(u, S, C, t)) : bf16x8{};
  }

  __device__ __forceinline__ void dots(const float* w_s, float* z_s, int S, int C) const {
    __shared__ float dpart[P * NT];
    const int t = threadIdx.x;
    const int C8 = C >> 3;
    const int cg = t % C8;
    const bool lane = t < S * C8;
#pragma unroll
    for (int u = 0; u < P; ++u) {
      float d = 0.f;
      if (lane) {
#pragma unroll
        for (int e = 0; e < 8; ++e) d += (float)v[u][e] * w_s[cg * 8 + e];
      }
      dpart[u * NT + t] = d;
    }
    __syncthreads();
    for (int p = t; p < S * S; p += NT) {
      const int u = p / S, j = p - u * S;
      const float* q = dpart + u * NT + j * C8;
      float d = 0.f;
      for (int k = 0; k < C8; ++k) d += q[k];
      z_s[p] = d;
    }
    __syncthreads();
  }

  __device__ __forceinline__ void backward(const PolicyHeadArgs& a, int b, const float* w_s,
                                           const float* g_s) const {
    __shared__ float part[NT * 8];
    const int t = threadIdx.x;
    const int S = a.S, C8 = a.C >> 3;
    const int j = t / C8, cg = t - j * C8;
    const bool lane = t < S * C8;
    __bf16* dzb = a.dz + (size_t)b * (S + 2) * (S + 2) * a.C;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float wl[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) wl[e] = lane ? w_s[cg * 8 + e] : 0.f;
#pragma unroll
    for (int u = 0; u < P; ++u) {
      if (u < S && lane) {
        const float g = g_s[u * S + j];
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float y = (float)v[u][e];
          o[e] = (__bf16)(y > 0.f ? g * wl[e] : 0.f);
          acc[e] += g * y;
        }
        *(bf16x8*)(dzb + offset(u, S, a.C, t)) = o;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[t * 8 + e] = acc[e];
    __syncthreads();
    float* dh = a.dhead + (size_t)b * (a.C_real + 1);
    for (int c = t; c < a.C_real; c += NT) {
      const int g8 = c >> 3, e = c & 7;
      float s = 0.f;
      for (int jj = 0; jj < S; ++jj) s += part[(jj * C8 + g8) * 8 + e];
      dh[c] = s;
    }
  }
};

// Reference RL loss (reinforcement_policy_trainer.py:109, Keras 1.0
// binary_crossentropy on the softmax output): per board
//   L = -1/SS * sum_j [y_j log pc_j + (1 - y_j) log(1 - pc_j)],  pc = clip(p, 1e-7, 1 - 1e-7)
// with y the one-hot move; clip has zero gradient outside its range (Theano
// clip), and the softmax backward is dz_i = p_i (g_i - sum_j p_j g_j).
template <int NT, class Board>
__device__ void policy_bce_train(const PolicyHeadArgs& a, int b, int t, float wb, float zmax, float inv, int lidx,
                                 const Board& board, const float* w_s, float* z_s, float* red) {
  __shared__ float p_s[368];
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const float eps = 1e-7f;
  float ls = 0.f, pg = 0.f;
  for (int p = tid; p < SS; p += NT) {
    const float pr = (z_s[p] == -INFINITY) ? 0.f : __expf(z_s[p] - zmax) * inv;
    const float pc = fminf(fmaxf(pr, eps), 1.f - eps);
    const bool y = p == t;
    ls += y ? __logf(pc) : __logf(1.f - pc);
    const float g = (pr < eps || pr > 1.f - eps) ? 0.f : -(y ? 1.f / pr : -1.f / (1.f - pr)) / (float)SS;
    p_s[p] = pr;
    z_s[p] = g;
    pg += pr * g;
  }
  ls = block_reduce_sum(ls, red);
  pg = block_reduce_sum(pg, red);
  if (tid == 0) {
    a.loss[b] = t >= 0 ? -ls / (float)SS : 0.f;
    a.correct[b] = (t >= 0 && lidx == t) ? 1.f : 0.f;
  }
  const float sc = t >= 0 ? a.grad_scale * wb : 0.f;
  for (int p = tid; p < SS; p += NT) z_s[p] = p_s[p] * (z_s[p] - pg) * sc;
  __syncthreads();
  board.backward(a, b, w_s, z_s);
  float gs = 0.f;
  for (int p = tid; p < SS; p += NT) gs += z_s[p];
  gs = block_reduce_sum(gs, red);
  if (tid == 0) a.dhead[(size_t)b * (a.C_real + 1) + a.C_real] = gs;
}

// The anchor distribution of one board, staged in LDS by the REG kernels only (read for KL(q || p)
// and again for the gradient).
template <bool REG>
__device__ __forceinline__ float* head_anchor_lds() {
  if constexpr (REG) {
    __shared__ float q_s[368];
    return q_s;
  } else {
    return nullptr;
  }
}

// One workgroup per board, its activations read once into registers (Board).  Large batches: 512
// threads with BoardRows (126 VGPRs, two boards per CU).  Below kHeadWideBelow boards, or when a
// row does not fit 512 lanes: 1024 threads with BoardRegs (B = 16 has only 16 workgroups: a board's
// loads get all the lanes).
//
// REG (launched only when stats, ref_probs or a coefficient is set; the plain instantiations hold
// none of its code): per-board diagnostics stats[b] = {H(p), KL(q || p), max |z|} and, for
// loss_kind 0, the regularised objective
//   L_b = -w_b log p_t - beta H(p) + kappa KL(q || p),
//   dL_b/dz_i = w_b (p_i - 1{i=t}) + beta p_i (log p_i + H) + kappa (p_i - q_i)
// with log p_i = z_i - zmax - lse (never log(p_i)); masked logits have p_i = 0 and add nothing.
template <bool TRAIN, int NT, class Board, bool REG = false>
__global__ __launch_bounds__(NT) void policy_head_kernel(PolicyHeadArgs a) {
  __shared__ float w_s[256];
  __shared__ float z_s[368];
  __shared__ float red[16];
  __shared__ int redi[16];
  // boards in reverse: the last-written boards of the final forward are the ones still in the
  // Infinity Cache, and they are read before this kernel's own dZ writes evict them
  const int b = (int)gridDim.x - 1 - (int)blockIdx.x;
  const int tid = threadIdx.x;
  const int SS = a.S * a.S;
  const int HP = a.S + 2;
  for (int c = tid; c < a.C; c += NT) w_s[c] = c < a.C_real ? a.w[c] : 0.f;
  Board board;
  board.load(a.y + (size_t)b * HP * HP * a.C, a.S, a.C);
  __syncthreads();
  const float bias = a.b[0];
  const uint8_t* legal = a.legal ? a.legal + (size_t)b * SS : nullptr;

  float lmax = -INFINITY;
  int lidx = 0x7fffffff;
  board.dots(w_s, z_s, a.S, a.C);
  for (int p = tid; p < SS; p += NT) {
    float z = (z_s[p] + bias) * a.inv_temp;
    if (legal && !legal[p]) z = -INFINITY;
    z_s[p] = z;
    if (z > lmax) {  // first max wins (p increases within a thread)
      lmax = z;
      lidx = p;
    }
  }
  // block argmax / max (ties -> smallest index)
  {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      float ov = __shfl_xor(lmax, o, 64);
      int oi = __shfl_xor(lidx, o, 64);
      if (ov > lmax || (ov == lmax && oi < lidx)) {
        lmax = ov;
        lidx = oi;
      }
    }
    if ((tid & 63) == 0) {
      red[tid >> 6] = lmax;
      redi[tid >> 6] = lidx;
    }
    __syncthreads();
    lmax = red[0];
    lidx = redi[0];
    for (int w = 1; w < NT / 64; ++w)
      if (red[w] > lmax || (red[w] == lmax && redi[w] < lidx)) {
        lmax = red[w];
        lidx = redi[w];
      }
  }
  const float zmax = lmax;
  float ls = 0.f;
  for (int p = tid; p < SS; p += NT) ls += (z_s[p] == -INFINITY) ? 0.f : __expf(z_s[p] - zmax);
  const float sum = block_reduce_sum(ls, red);
  const float inv = 1.f / sum;
  if (a.probs) {
    for (int p = tid; p < SS; p += NT)
      a.probs[(size_t)b * SS + p] = (z_s[p] == -INFINITY) ? 0.f : __expf(z_s[p] - zmax) * inv;
  }
  float* q_s = head_anchor_lds<REG>();
  float lse = 0.f, ent = 0.f;
  if constexpr (REG) {
    lse = __logf(sum);
    const float* q = a.ref_probs ? a.ref_probs + (size_t)b * SS : nullptr;
    float sh = 0.f, skl = 0.f, mz = 0.f;
    for (int p = tid; p < SS; p += NT) {
      const float z = z_s[p];
      const bool fin = z != -INFINITY;
      if (fin) {
        sh += __expf(z - zmax) * inv * (z - zmax);
        mz = fmaxf(mz, fabsf(z));
      }
      if (q) {
        const float qi = q[p];
        q_s[p] = qi;
        // a masked logit under q_i > 0: log p_i = -inf, the term (and the sum) is +inf
        if (qi > 0.f) skl += qi * (__logf(qi) - (z - zmax - lse));
      }
    }
    ent = lse - block_reduce_sum(sh, red);
    skl = block_reduce_sum(skl, red);
    mz = block_reduce_max(mz, red);
    if (a.stats && tid == 0) {
      a.stats[(size_t)b * 3 + 0] = ent;
      a.stats[(size_t)b * 3 + 1] = skl;
      a.stats[(size_t)b * 3 + 2] = mz;
    }
  }
  if constexpr (TRAIN) {
    const int t = a.target[b];
    const float wb = a.weight ? a.weight[b] : 1.f;
    if (a.loss_kind == 1) {
      policy_bce_train<NT, Board>(a, b, t, wb, zmax, inv, lidx, board, w_s, z_s, red);
      return;
    }
    if (tid == 0) {
      if (t >= 0) {
        float pt = __expf(z_s[t] - zmax) * inv;
        pt = fminf(fmaxf(pt, 1e-7f), 1.f - 1e-7f);  // Keras clip
        a.loss[b] = -__logf(pt);
        a.correct[b] = (lidx == t) ? 1.f : 0.f;
      } else {
        a.loss[b] = 0.f;
        a.correct[b] = 0.f;
      }
    }
    __syncthreads();  // everyone has read z_s[t]
    if (REG && (a.ent_coef != 0.f || a.kl_coef != 0.f)) {
      const bool anchored = a.kl_coef != 0.f && a.ref_probs;
      for (int p = tid; p < SS; p += NT) {
        const float z = z_s[p];
        float g = 0.f;
        if (t >= 0 && z != -INFINITY) {  // a masked logit is a constant: no gradient
          const float pr = __expf(z - zmax) * inv;
          float r = a.ent_coef * pr * (z - zmax - lse + ent);
          if (anchored) r += a.kl_coef * (pr - q_s[p]);
          g = ((pr - (p == t ? 1.f : 0.f)) * wb + r) * a.grad_scale;
        }
        z_s[p] = g;
      }
    } else {  // the plain kernels' loop, also the REG kernels' with both coefficients 0 (same bits)
      for (int p = tid; p < SS; p += NT) {
        float g = 0.f;
        if (t >= 0) g = (__expf(z_s[p] - zmax) * inv - (p == t ? 1.f : 0.f)) * a.grad_scale * wb;
        z_s[p] = g;
      }
    }
    __syncthreads();
    board.backward(a, b, w_s, z_s);
    float gs = 0.f;
    for (int p = tid; p < SS; p += NT) gs += z_s[p];
    gs = block_reduce_sum(gs, red);
    if (tid == 0) a.dhead[(size_t)b * (a.C_real + 1) + a.C_real] = gs;
  }
}

template <bool TRAIN, bool REG>
static void policy_head_go(const PolicyHeadArgs& a, hipStream_t st) {
  if (a.B >= kHeadWideBelow && a.S * (a.C >> 3) <= 512)
    hipLaunchKernelGGL((policy_head_kernel<TRAIN, 512, BoardRows<512>, REG>), dim3(a.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((policy_head_kernel<TRAIN, 1024, BoardRegs<1024>, REG>), dim3(a.B), dim3(1024), 0, st, a);
}

// the REG instantiations (head_reg.hip)
void launch_policy_head_reg(const PolicyHeadArgs& a, bool train, hipStream_t st);

}  // namespace agk
