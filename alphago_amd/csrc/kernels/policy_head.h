// The building blocks of the 1x1 head family (head.hip, head_reg.hip, head_soft.hip, head_pv.hip,
// head_own.hip, symmetry.hip): block reductions, weight staging, the pass logit, the board holders with
// their dot products and backward, the masked softmax, the dW / dbias reductions, the accumulating
// backward for NH heads and the launch rules.  The fused policy head kernel is a template here because
// two translation units instantiate it: head.hip holds the plain kernels of the SL / RL step,
// head_reg.hip the regularised variants (REG).  Every file of the family is a module of its own, so
// that one file's code objects do not depend on another's kernels (LDS variables are laid out per
// module).
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace agk {

// boards below which the per-board head kernels run 1024 threads per workgroup
constexpr int kHeadWideBelow = 256;

// The kernels that hold a board in registers, one workgroup per board.  Large batches: 512 threads
// with BoardRows (126 VGPRs, two boards per CU).  Below kHeadWideBelow boards, or when a row does
// not fit 512 lanes: 1024 threads with BoardRegs (16 boards are only 16 workgroups: a board's loads
// get all the lanes).
inline bool head_rows_mapping(int64_t boards, int S, int C) {
  return boards >= kHeadWideBelow && S * (C >> 3) <= 512;
}
// The kernels that stream a board (head_dots, the backward walkers): 1024 threads for few boards,
// for the same reason, else 256.
inline bool head_wide_block(int64_t boards) { return boards < kHeadWideBelow; }
// what the launchers of the pass variants check before they choose a mapping
inline void head_check_geometry(const char* op, int B, int S, int C, int C_real) {
  if (C % 8 || C < 8 || C > 256 || C_real < 1 || C_real > C || B < 1 || S < 1 || S > 19)
    throw std::invalid_argument(std::string(op) +
                                ": C a multiple of 8 in 8..256, 1 <= C_real <= C, B >= 1, S in 1..19");
}

// The block reductions: the waves' results in wave order.  NW is the workgroup's wave count where the caller
// knows it (0: blockDim.x >> 6).  The bodies that several __global__s share pass it: inside a __device__
// function the compiler does not fold blockDim.x to the kernel's uniform workgroup size, and the read it
// leaves is a global load whose wait also drains the board's loads in flight.
template <int NW = 0>
__device__ __forceinline__ float block_reduce_max(float v, float* red) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < (NW ? NW : (int)(blockDim.x >> 6)); ++i) r = fmaxf(r, red[i]);
  return r;
}
template <int NW = 0>
__device__ __forceinline__ float block_reduce_sum(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < (NW ? NW : (int)(blockDim.x >> 6)); ++i) r += red[i];
  return r;
}

// Block argmax, ties to the smallest index: (v, idx) is this thread's candidate, the return value the
// block's.  red / redi may be reused only after a barrier of the caller's.  They are taken as arrays,
// not pointers, so that the compiler knows redi[w] may be read before red[w] == v is decided (with
// pointers the cross-wave loop becomes a chain of branches).
struct ArgMax {
  float v;
  int idx;
};
template <int NT>
__device__ __forceinline__ ArgMax block_argmax(float v, int idx, float (&red)[16], int (&redi)[16]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > v || (ov == v && oi < idx)) {
      v = ov;
      idx = oi;
    }
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = v;
    redi[tid >> 6] = idx;
  }
  __syncthreads();
  v = red[0];
  idx = redi[0];
  for (int w = 1; w < NT / 64; ++w)
    if (red[w] > v || (red[w] == v && redi[w] < idx)) {
      v = red[w];
      idx = redi[w];
    }
  return {v, idx};
}

// The weights of NH heads into LDS: the C_real real entries, zeros up to the padded C.  One loop for
// all heads, so that their global loads are in flight together (a loop per head costs every workgroup
// one more load latency before its board loads).  The caller's next barrier publishes them.
template <int NT, int NH>
__device__ __forceinline__ void head_stage_weights(float* const (&w_s)[NH], const float* const (&w)[NH], int C,
                                                   int C_real) {
  for (int c = threadIdx.x; c < C; c += NT) {
    float v[NH];  // every load before the first store
#pragma unroll
    for (int h = 0; h < NH; ++h) v[h] = c < C_real ? w[h][c] : 0.f;
#pragma unroll
    for (int h = 0; h < NH; ++h) w_s[h][c] = v[h];
  }
}

// The pass entry of the PASS kernels: one more logit after the S * S board logits,
//   z_pass[b] = pooled[b].reshape(2 C) . pass_w + pass_b,
// with pooled (B, 2, C) the mean and max of the trunk output over the board (a preceding gpool_fwd) and
// pass_w a zero-padded (2, C) copy of the net's (2 F, 1) weight.  It is the last entry of the softmax (index
// S * S, so it loses ties in every argmax) and thread S * S owns it in every loop and reduction.
// pass_logit: this thread's term of z_pass without the bias (thread t < 2 C owns entry t of the board's
// pooled row; pv keeps the pooled value for the training head's partial row) summed over the block in a
// fixed order.  The accesses the PASS kernels add are bounds-checked in the debug build (bounds_at, common.h).
template <int NT>
__device__ __forceinline__ float pass_logit(const PassHeadOperands& ps, int b, int C, float* red, float& pv) {
  static_assert(NT >= 512, "one pooled entry per thread (2 C <= 512)");
  const int tid = threadIdx.x;
  float term = 0.f;
  pv = 0.f;
  if (tid < 2 * C) {
    pv = ps.pooled[bounds_at((long long)b * 2 * C + tid, ps.pooled_elems)];
    term = pv * ps.pass_w[tid];
  }
  return block_reduce_sum<NT / 64>(term, red);
}

// The masked softmax of one board's logits, in three steps that share z_s.
// 1. head_mask_logits: z_s holds the dot products on entry and the masked logits (z + bias) * inv_temp,
//    -inf where legal[p] == 0, on return; the result is this thread's maximum and its first index.
template <int NT>
__device__ __forceinline__ ArgMax head_mask_logits(float* z_s, int SS, float bias, float inv_temp,
                                                   const uint8_t* legal) {
  float lmax = -INFINITY;
  int lidx = 0x7fffffff;
  for (int p = threadIdx.x; p < SS; p += NT) {
    float z = (z_s[p] + bias) * inv_temp;
    if (legal && !legal[p]) z = -INFINITY;
    z_s[p] = z;
    if (z > lmax) {  // first max wins (p increases within a thread)
      lmax = z;
      lidx = p;
    }
  }
  return {lmax, lidx};
}
// 2. the block's maximum zmax: block_argmax where the arg-max is wanted (policy_head_kernel), inside
//    head_masked_softmax otherwise.  3. head_exp_sum: the sum of exp(z - zmax) over the unmasked points.
template <int NT, int NW = 0>
__device__ __forceinline__ float head_exp_sum(const float* z_s, int SS, float zmax, float* red) {
  float ls = 0.f;
  for (int p = threadIdx.x; p < SS; p += NT) ls += (z_s[p] == -INFINITY) ? 0.f : __expf(z_s[p] - zmax);
  return block_reduce_sum<NW>(ls, red);
}
struct HeadSoftmax {
  float zmax, inv;
};
// all three steps for a head that needs no arg-max
template <int NT>
__device__ __forceinline__ HeadSoftmax head_masked_softmax(float* z_s, int SS, float bias, float inv_temp,
                                                           const uint8_t* legal, float* red) {
  const int tid = threadIdx.x;
  float lmax = head_mask_logits<NT>(z_s, SS, bias, inv_temp, legal).v;
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
  return {lmax, 1.f / head_exp_sum<NT>(z_s, SS, lmax, red)};
}
// the probabilities of head_masked_softmax's logits: a masked point gets 0
template <int NT>
__device__ __forceinline__ void head_write_probs(float* probs, const float* z_s, int SS, float zmax, float inv) {
  for (int p = threadIdx.x; p < SS; p += NT) probs[p] = (z_s[p] == -INFINITY) ? 0.f : __expf(z_s[p] - zmax) * inv;
}

// dW_head of one board from the threads' partials: thread t's eight channel sums acc go to
// part[t * 8 ..]; channel c (group g8 = c / 8) is then the sum over r < rows of the partial of thread
// r * stride + g8, in r order, and lands in dh[c].  part may be reused after a barrier.
template <int NT>
__device__ __forceinline__ void head_channel_sums(float* part, const float (&acc)[8], float* dh, int C_real,
                                                  int stride, int rows) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 8; ++e) part[tid * 8 + e] = acc[e];
  __syncthreads();
  for (int c = tid; c < C_real; c += NT) {
    const int g8 = c >> 3, e = c & 7;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += part[(r * stride + g8) * 8 + e];
    dh[c] = s;
  }
}

// The bias gradient of one board, dhead[b][C_real]: the fixed-order block sum of the dlogits, from the
// threads' partial sums or from the row in LDS.
template <int NW = 0>
__device__ __forceinline__ void head_bias_grad(float gs, float* red, float* dst) {
  gs = block_reduce_sum<NW>(gs, red);
  if (threadIdx.x == 0) *dst = gs;
}
template <int NT, int NW = 0>
__device__ __forceinline__ void head_bias_grad(const float* g_s, int SS, float* red, float* dst) {
  float gs = 0.f;
  for (int p = threadIdx.x; p < SS; p += NT) gs += g_s[p];
  head_bias_grad<NW>(gs, red, dst);
}

// The board's registers made opaque between two uses (a second dots, the backward): otherwise the
// compiler keeps the first pass's fp32 conversions of the whole board live, twice the registers of the
// packed bf16 (BoardRegs<1024>: 96 more VGPRs, a spill past 128).
template <class Board>
__device__ __forceinline__ void board_launder(Board& board) {
#pragma unroll
  for (int u = 0; u < Board::P; ++u) asm volatile("" : "+v"(board.v[u]));
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
    head_channel_sums<NT>(part, acc, a.dhead + (size_t)b * (a.C_real + 1), a.C_real, 32, R);
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
    head_channel_sums<NT>(part, acc, a.dhead + (size_t)b * (a.C_real + 1), a.C_real, C8, S);
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
  head_bias_grad<NT>(z_s, SS, red, a.dhead + (size_t)b * (a.C_real + 1) + a.C_real);
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

// One workgroup per board, its activations read once into registers (Board, chosen by
// head_rows_mapping).
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
  head_stage_weights<NT>({w_s}, {a.w}, a.C, a.C_real);
  Board board;
  board.load(a.y + (size_t)b * HP * HP * a.C, a.S, a.C);
  __syncthreads();
  const float bias = a.b[0];
  const uint8_t* legal = a.legal ? a.legal + (size_t)b * SS : nullptr;

  board.dots(w_s, z_s, a.S, a.C);
  const ArgMax lm = head_mask_logits<NT>(z_s, SS, bias, a.inv_temp, legal);
  const ArgMax zm = block_argmax<NT>(lm.v, lm.idx, red, redi);
  const float zmax = zm.v;
  const int lidx = zm.idx;
  const float sum = head_exp_sum<NT>(z_s, SS, zmax, red);
  const float inv = 1.f / sum;
  if (a.probs) head_write_probs<NT>(a.probs + (size_t)b * SS, z_s, SS, zmax, inv);
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
    head_bias_grad<NT>(z_s, SS, red, a.dhead + (size_t)b * (a.C_real + 1) + a.C_real);
  }
}

template <bool TRAIN, bool REG>
static void policy_head_go(const PolicyHeadArgs& a, hipStream_t st) {
  if (head_rows_mapping(a.B, a.S, a.C))
    hipLaunchKernelGGL((policy_head_kernel<TRAIN, 512, BoardRows<512>, REG>), dim3(a.B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((policy_head_kernel<TRAIN, 1024, BoardRegs<1024>, REG>), dim3(a.B), dim3(1024), 0, st, a);
}

// The body of the dual network's inference heads, one workgroup per board: both (OWN: all three)
// heads' dot products come from the one register copy of the board.  The policy row goes through
// policy_head_kernel<false>'s masked softmax at temperature 1 (policy_head_probs' bits), the value
// row plus its bias leaves as fp32 logits (head_logits' quantity), the ownership row as tanh.
// PASS: the softmax has the pass entry behind the board points (always legal; probs rows of S * S + 1); zv
// and own keep their bits.
template <int NT, class Board, bool OWN, bool PASS = false>
__device__ __forceinline__ void policy_value_head_body(const PolicyValueHeadArgs& a, const float* wo, const float* bo,
                                                       float* own, const PassHeadOperands& ps = {}) {
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
  const int HP = a.S + 2;
  if constexpr (OWN) {
    __shared__ float wo_lds[256];
    __shared__ float zo_lds[368];
    wo_s = wo_lds;
    zo_s = zo_lds;
    head_stage_weights<NT>({wp_s, wv_s, wo_s}, {a.wp, a.wv, wo}, a.C, a.C_real);
  } else {
    head_stage_weights<NT>({wp_s, wv_s}, {a.wp, a.wv}, a.C, a.C_real);
  }
  Board board;
  board.load(a.y + (size_t)b * HP * HP * a.C, a.S, a.C);
  float zp = 0.f;
  if constexpr (PASS) {
    float pv;
    zp = pass_logit<NT>(ps, b, a.C, red, pv) + ps.pass_b[0];
  }
  __syncthreads();  // the weights are staged; red is free again
  const float bias = a.bp[0];
  const float vbias = a.bv[0];
  const float obias = OWN ? bo[0] : 0.f;
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
    if constexpr (OWN) own[(size_t)b * SS + p] = tanhf(zo_s[p] + obias);
  }
  if constexpr (PASS) {  // thread SS owns the pass entry
    const int NE = SS + 1;
    float lmax = head_mask_logits<NT>(z_s, SS, bias, 1.f, legal).v;
    if (tid == SS) {
      z_s[SS] = zp;
      lmax = zp;
    }
    const float zmax = block_reduce_max<NT / 64>(lmax, red);  // its barriers publish z_s
    const float inv = 1.f / head_exp_sum<NT, NT / 64>(z_s, NE, zmax, red);
    float* row = a.probs + bounds_at((long long)b * NE, ps.probs_elems - SS);
    head_write_probs<NT>(row, z_s, NE, zmax, inv);
  } else {
    const HeadSoftmax sm = head_masked_softmax<NT>(z_s, SS, bias, 1.f, legal, red);
    head_write_probs<NT>(a.probs + (size_t)b * SS, z_s, SS, sm.zmax, sm.inv);
  }
}

// The walker of the streaming backward kernels.  Thread (r, cg) = (tid / (C / 8), tid % (C / 8)) visits
// positions p = r, r + R, ... (R = NT / (C / 8)) for its 8-channel group; consecutive threads cover
// consecutive 16-B channel groups of one position (coalesced rows).  The loop is bound by load latency,
// so BU positions' loads of y (with RMW also of dz) are issued before the first is used.  For every
// position in order f(p, off, v, d) gets the element offset of the group in the padded board, y's
// eight values and (RMW) dz's.
template <int NT, int BU, bool RMW, class F>
__device__ __forceinline__ void head_walk_positions(const __bf16* base, const __bf16* dzb, int S, int C, F f) {
  const int tid = threadIdx.x;
  const int SS = S * S;
  const int HP = S + 2;
  const int C8 = C >> 3;
  const int R = NT / C8;  // positions processed concurrently
  const int r = tid / C8, cg = tid - r * C8;
  if (r >= R) return;
  const int c8 = cg << 3;
  for (int p0 = r; p0 < SS; p0 += BU * R) {
    bf16x8 v[BU], d[RMW ? BU : 1];
    size_t off[BU];
#pragma unroll
    for (int u = 0; u < BU; ++u) {
      const int p = p0 + u * R;
      const int pc = p < SS ? p : SS - 1;
      const int i = pc / S, j = pc - (pc / S) * S;
      off[u] = (size_t)((i + 1) * HP + j + 1) * C + c8;
      v[u] = *(const bf16x8*)(base + off[u]);
      if constexpr (RMW) d[u] = *(const bf16x8*)(dzb + off[u]);
    }
#pragma unroll
    for (int u = 0; u < BU; ++u) {
      const int p = p0 + u * R;
      if (p < SS) f(p, off[u], v[u], d[RMW ? u : 0]);
    }
  }
}

// The accumulating backward of NH 1x1 heads on one trunk, one workgroup per board: one read of y and
// one read-modify-write of the dZ another head wrote.  Where y > 0:
//   dz[p, c] = bf16_rne(fma(g_NH[p], w_NH[c], ... fma(g_1[p], w_1[c], float(dz[p, c]))))
// every fma in fp32 with a single rounding, head 1 innermost, then the bf16 round-to-nearest-even.
// Elsewhere the element keeps its bits; the border is never addressed.  Thread (r, cg) walks positions
// p = r, r + R, ... for its 8-channel group and adds g_h[p] * y[p, c] in that order; each head's R
// partials per channel are summed through the one LDS block in r order, head 1 first
// (head_input_backward's order: head_backward's dhead bits).  dhead[h][b] = [dW_h | sum_p g_h[p]].
template <int NT, int NH>
__device__ __forceinline__ void head_backward_accumulate(const __bf16* y, __bf16* dz, const float* const (&w)[NH],
                                                         const float* const (&g)[NH], float* const (&dhead)[NH],
                                                         int S, int C, int C_real) {
  __shared__ float w_s[NH][256];
  __shared__ float g_s[NH][368];
  __shared__ float red[16];
  __shared__ float part[NT * 8];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int SS = S * S;
  const int HP = S + 2;
  float* w_rows[NH];
  float gs[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    w_rows[h] = w_s[h];
    gs[h] = 0.f;
  }
  head_stage_weights<NT>(w_rows, w, C, C_real);
  for (int p = tid; p < SS; p += NT) {
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const float gv = g[h][(size_t)b * SS + p];
      g_s[h][p] = gv;
      gs[h] += gv;
    }
  }
  __syncthreads();
  const int C8 = C >> 3;
  const int c8 = (tid % C8) << 3;
  __bf16* dzb = dz + (size_t)b * HP * HP * C;
  float acc[NH][8];
#pragma unroll
  for (int h = 0; h < NH; ++h)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[h][e] = 0.f;
  // four positions in flight per thread (two 16-B loads each)
  head_walk_positions<NT, 4, true>(y + (size_t)b * HP * HP * C, dzb, S, C,
                                   [&](int p, size_t off, const bf16x8& v, const bf16x8& d) {
    float gp[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) gp[h] = g_s[h][p];
    bf16x8 o = d;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float yv = (float)v[e];
      if (yv > 0.f) {
        float x = (float)d[e];
#pragma unroll
        for (int h = 0; h < NH; ++h) x = __builtin_fmaf(gp[h], w_s[h][c8 + e], x);
        o[e] = (__bf16)x;
      }
#pragma unroll
      for (int h = 0; h < NH; ++h) acc[h][e] += gp[h] * yv;
    }
    *(bf16x8*)(dzb + off) = o;
  });
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    if (h) __syncthreads();  // part is reused
    head_channel_sums<NT>(part, acc[h], dhead[h] + (size_t)b * (C_real + 1), C_real, C8, NT / C8);
  }
#pragma unroll
  for (int h = 0; h < NH; ++h) head_bias_grad(gs[h], red, dhead[h] + (size_t)b * (C_real + 1) + C_real);
}

// the REG instantiations (head_reg.hip)
void launch_policy_head_reg(const PolicyHeadArgs& a, bool train, hipStream_t st);

}  // namespace agk
