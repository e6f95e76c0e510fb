// Shared pieces of the implicit-GEMM conv kernels (conv.hip: production
// kernels and dispatch; conv_fwd_variants.hip: the forward kernel lab).
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "common.h"
#include "kernels.h"

namespace agk {

// Debug build (AGK_DEBUG): device bounds checks.  AGK_DCHECK(cond, code)
// evaluates to cond; when it is false the code is OR-ed into a per-module error
// word (a vector atomic) and the caller skips / redirects the access, so a bad
// offset is reported (debug_error_fetch_and_clear -> Python RuntimeError)
// instead of touching memory outside the tensor.  Release builds: always true.
#ifdef AGK_DEBUG
static __device__ unsigned g_dbg_err;
#define AGK_DCHECK(cond, code) \
  ((cond) ? true : (atomicOr(&::agk::g_dbg_err, (unsigned)(code)), false))
#else
#define AGK_DCHECK(cond, code) true
#endif
enum : unsigned {
  DBG_FWD_X = 1u << 0,   // conv_fwd: activation (pixel operand) staging offset
  DBG_FWD_W = 1u << 1,   // conv_fwd: weight staging offset
  DBG_FWD_Y = 1u << 2,   // conv_fwd: epilogue store offset
  DBG_WG_X = 1u << 3,    // conv_wgrad: activation staging offset
  DBG_WG_DZ = 1u << 4,   // conv_wgrad: gradient staging offset
};

// s_waitcnt vmcnt(N) for any immediate N (gfx950: 0..63)
template <int N>
__device__ __forceinline__ void vmcnt_n() {
  static_assert(N >= 0 && N <= 63, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS-ring wait: at most `later` stages of PW DMA instructions each may still be outstanding
// (later = 0 .. MAXL, wave-uniform); the exact count, not a clamped one, so the ring keeps its depth
template <int PW, int MAXL>
__device__ __forceinline__ void ring_wait(int later) {
  static_assert(MAXL >= 0 && MAXL <= 3 && PW * MAXL <= 63, "ring depth");
  if (MAXL >= 3 && later >= 3) vmcnt_n<PW * (MAXL >= 3 ? 3 : 0)>();
  else if (MAXL >= 2 && later >= 2) vmcnt_n<PW * (MAXL >= 2 ? 2 : 0)>();
  else if (MAXL >= 1 && later >= 1) vmcnt_n<PW * (MAXL >= 1 ? 1 : 0)>();
  else vmcnt_n<0>();
}

__device__ __forceinline__ void vmcnt_wait_dyn(int n) {
  switch (n) {
    case 0: vmcnt_n<0>(); break;
    case 1: vmcnt_n<1>(); break;
    case 2: vmcnt_n<2>(); break;
    case 3: vmcnt_n<3>(); break;
    case 4: vmcnt_n<4>(); break;
    case 5: vmcnt_n<5>(); break;
    case 6: vmcnt_n<6>(); break;
    case 7: vmcnt_n<7>(); break;
    default: vmcnt_n<8>(); break;
  }
}

// ---- wgrad helpers (conv.hip, conv_wgrad_row.hip)
// s_waitcnt lgkmcnt(CNT) tying one read pair: issued for each pair of a group whose reads are all
// older than the CNT most recent ones (the first wait blocks, the rest are already satisfied)
template <int CNT>
__device__ __forceinline__ void lgkm_wait_pair(bf16x4& a, bf16x4& b) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(CNT));
}

// (operand lists of lgkm_fence: read pair i, four pairs from i)
#define AGK_P(i) "+v"(a[i]), "+v"(b[i])
#define AGK_P4(i) AGK_P(i), AGK_P(i + 1), AGK_P(i + 2), AGK_P(i + 3)
#define AGK_FENCE(...) asm volatile("s_waitcnt lgkmcnt(0)" : __VA_ARGS__)
// s_waitcnt lgkmcnt(0) with every listed read result as an in/out operand:
// nothing that uses them can be scheduled above the wait.
template <int N>
__device__ __forceinline__ void lgkm_fence(bf16x4 (&a)[N], bf16x4 (&b)[N]) {
  static_assert(N >= 1 && N <= 15, "lgkm_fence supports 1..15 pairs (30 asm operands)");
  if constexpr (N == 15) AGK_FENCE(AGK_P4(0), AGK_P4(4), AGK_P4(8), AGK_P(12), AGK_P(13), AGK_P(14));
  else if constexpr (N == 14) AGK_FENCE(AGK_P4(0), AGK_P4(4), AGK_P4(8), AGK_P(12), AGK_P(13));
  else if constexpr (N == 13) AGK_FENCE(AGK_P4(0), AGK_P4(4), AGK_P4(8), AGK_P(12));
  else if constexpr (N == 12) AGK_FENCE(AGK_P4(0), AGK_P4(4), AGK_P4(8));
  else if constexpr (N == 11) AGK_FENCE(AGK_P4(0), AGK_P4(4), AGK_P(8), AGK_P(9), AGK_P(10));
  else if constexpr (N == 10) AGK_FENCE(AGK_P4(0), AGK_P4(4), AGK_P(8), AGK_P(9));
  else if constexpr (N == 9) AGK_FENCE(AGK_P4(0), AGK_P4(4), AGK_P(8));
  else if constexpr (N == 8) AGK_FENCE(AGK_P4(0), AGK_P4(4));
  else if constexpr (N == 7) AGK_FENCE(AGK_P4(0), AGK_P(4), AGK_P(5), AGK_P(6));
  else if constexpr (N == 6) AGK_FENCE(AGK_P4(0), AGK_P(4), AGK_P(5));
  else if constexpr (N == 5) AGK_FENCE(AGK_P4(0), AGK_P(4));
  else if constexpr (N == 4) AGK_FENCE(AGK_P4(0));
  else if constexpr (N == 3) AGK_FENCE(AGK_P(0), AGK_P(1), AGK_P(2));
  else if constexpr (N == 2) AGK_FENCE(AGK_P(0), AGK_P(1));
  else if constexpr (N == 1) AGK_FENCE(AGK_P(0));
}
#undef AGK_FENCE
#undef AGK_P4
#undef AGK_P

// ds_read_b64_tr_b16 through inline asm.  The builtin form makes hipcc wait
// vmcnt(0) before every such read while any LDS-DMA is outstanding (it cannot
// tell the read from the DMA target), which would drain the ring; the caller
// waits lgkmcnt itself (lgkm_fence below) before touching the results.
// f(std::integral_constant<int, 0>{}) ... f(<N - 1>): a loop whose index is a compile-time constant
// inside the body (immediate operands of inline asm)
template <class F, int... I>
__device__ __forceinline__ void static_for_seq(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_seq(f, std::make_integer_sequence<int, N>{});
}

// OFF: the instruction's immediate byte offset (16-bit, unsigned) -- the reads of a stage share one
// address register instead of one VALU add each.
template <int OFF = 0>
__device__ __forceinline__ bf16x4 ds_read_tr16_at(uint32_t lds_addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds_read offset: 16-bit unsigned");
  bf16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(lds_addr), "n"(OFF));
  return v;
}
template <int OFF = 0>
__device__ __forceinline__ bf16x4 ds_read_tr16_asm(const char* p) {
  return ds_read_tr16_at<OFF>((uint32_t)(uintptr_t)(AG_LDS(p)));
}

// 16-byte global -> LDS DMA from a wave-uniform base pointer plus a 32-bit per-lane byte offset
// (global_load_lds_dwordx4 v, s[base:base+1]): no 64-bit vector pointer per piece.  This is the form
// hipcc selects for `uniform base + zero-extended 32-bit lane offset`; it is the compiler's choice, not
// a guarantee (pin the base with sgpr_ptr so that it is not folded into the lane's part).  Where it
// does not match, the code is still correct and builds the 64-bit address with a v_lshl_add_u64.
// pins a wave-uniform pointer to a scalar register pair (no instruction): the compiler cannot fold
// it into the per-lane part of an address
__device__ __forceinline__ const char* sgpr_ptr(const char* p) {
  const uint64_t v = (uint64_t)(uintptr_t)p;
  uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  asm("" : "+s"(lo), "+s"(hi));
  return (const char*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ void glds16_so(const void* sbase, uint32_t voff, void* lds_wave_base) {
  glds16((const char*)sbase + (size_t)voff, lds_wave_base);
}


// Shared epilogue of the forward/dgrad kernels: lane owns output channels
// nbase + 16 i + [0, 4) of pixel mrow + 16 j.  load() issues every operand
// load (bias, or the ReLU' mask of dgrad) with clamped pixel indices — no
// per-element branches, so the loads overlap instead of forming 24
// load -> wait -> store round trips; the kernels call it a few K-steps before
// the end of the main loop so the mask read hides under the last MFMAs.
// MODE & MODE_RES (residual blocks): the skip operand a.res is added in fp32 before the ReLU / the mask.
// It is loaded inside store() in groups of RG pixel rows (RG x NB x 8 bytes per lane, at most 36 VGPRs; RG below),
// every load of a group issued before the group's first store: a preloaded NB x MB tile would cost what
// MODE_MASK's mk[][] costs (2 NB MB VGPRs on top of the accumulators), while one row at a time is one
// memory round trip per row (the compiler cannot move a row's loads above the previous row's stores: y
// and res might alias for all it knows).  The pixel indices are clamped, so a row past M loads in range
// and is not stored.  Interior pixels only, so the operand's border is never read.
template <int NB, int MB, int MODE>
struct ConvEpilogue {
  static constexpr int BASE = MODE & 3;
  static constexpr bool RES = (MODE & MODE_RES) != 0;
  static_assert(!RES || BASE == MODE_BIAS_RELU || BASE == MODE_MASKBITS, "skip operand: bias + ReLU or bitmask dgrad");
  static constexpr bool BF8 = BASE == MODE_MASKBITS && !RES;  // the e5m2 copy: not with a skip operand
  // rows per skip-load group: 3 at NB = 6 on the 96-pixel wave tiles (MB = 6), whose accumulators leave the
  // registers; the smaller tiles keep their accumulators next to 96 AGPRs and take one row at a time
  static constexpr int RG = !(RES && MB >= 6) ? 1 : (18 / NB < 1 ? 1 : (18 / NB > MB ? MB : 18 / NB));
  int ooff[MB];
  int pix[MB];
  f32x4 bb[NB];
  bf16x4 mk[NB][MB];
  uint32_t mw[MB];
  float gsc;  // MODE_MASKBITS with an e5m2 copy: *a.bf8_scale
  int mslot, mwords;

  // ReLU' bitmask layout: per padded pixel, (Cout/BN)*8 32-bit words; word
  // (blockIdx.y*8 + wn*4 + lane/16) holds bit 4i+r for channel nbase+16i+r —
  // exactly the channels one lane owns, so producer and consumer never
  // exchange data (12x less traffic than re-reading the bf16 activation).
  __device__ __forceinline__ void load(const ConvFwdArgs& a, int mrow, int nbase, int wn = 0) {
    const int SS = a.S * a.S;
    mslot = blockIdx.y * 8 + wn * 4 + ((threadIdx.x & 63) >> 4);
    mwords = gridDim.y * 8;
#pragma unroll
    for (int j = 0; j < MB; ++j) {
      int m = mrow + j * 16;
      m = m < a.M ? m : a.M - 1;
      const int b = fdiv(m, a.divSS);
      const int rem = m - b * SS;
      const int ii = fdiv(rem, a.divS);
      const int jj = rem - ii * a.S;
      pix[j] = (b * a.HPo + ii + a.Po) * a.HPo + jj + a.Po;
      ooff[j] = pix[j] * a.Cout + nbase;
    }
    if constexpr (BASE == MODE_BIAS_RELU) {
#pragma unroll
      for (int i = 0; i < NB; ++i) bb[i] = *(const f32x4*)(a.bias + nbase + i * 16);
    } else if constexpr (BASE == MODE_MASK) {
#pragma unroll
      for (int j = 0; j < MB; ++j)
#pragma unroll
        for (int i = 0; i < NB; ++i) mk[i][j] = *(const bf16x4*)(a.mask + ooff[j] + i * 16);
    } else if constexpr (BASE == MODE_MASKBITS) {
#pragma unroll
      for (int j = 0; j < MB; ++j) mw[j] = a.mbits_in[(size_t)pix[j] * mwords + mslot];
      if constexpr (BF8) gsc = a.y_bf8 ? *a.bf8_scale : 0.f;
    }
  }

  // Retires every operand load of load() once, after the K loop and before the first store: each
  // loaded register passes through an empty asm, so the compiler waits for it here and knows it
  // complete afterwards.  Without this the rows' exec-masked `continue` makes the waitcnt
  // insertion re-emit the operand waits at every row's join, and since vmcnt retires in issue
  // order those waits bind on the previous row's stores: one store round trip per pixel row.
  // Kernels that call load() inside the K loop call this after the loop (their in-loop waits are
  // inline asm, invisible to the compiler; the loads have long landed and the wait costs nothing).
  __device__ __forceinline__ void settle() {
    // with a skip operand the rows load in groups between their stores anyway, and pinning the bias
    // registers ahead of the first group costs the 384-pixel tiles 14 spilled VGPRs
    if constexpr (RES) return;
    if constexpr (BASE == MODE_BIAS_RELU) {
#pragma unroll
      for (int i = 0; i < NB; ++i) asm volatile("" : "+v"(bb[i]));
    } else if constexpr (BASE == MODE_MASK) {
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < MB; ++j) asm volatile("" : "+v"(mk[i][j]));
    } else if constexpr (BASE == MODE_MASKBITS) {
#pragma unroll
      for (int j = 0; j < MB; ++j) asm volatile("" : "+v"(mw[j]));
      if constexpr (BF8) {
        asm volatile("" : "+v"(gsc));
        gsc = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(gsc)));  // wave-uniform: a scalar
      }
    }
  }

  // blocks stored in pairs (store_rows): all but an odd last one; none with a skip operand, whose row
  // groups already fill the registers (paired, the 384-pixel residual tiles spill 14-16 VGPRs)
  static constexpr int NBP = RES ? 0 : NB;
  // 8-byte-aligned 16-byte store / 4-byte-aligned 8-byte store (global memory takes both at dword alignment)
  typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
  typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

  __device__ __forceinline__ void store(const ConvFwdArgs& a, const f32x4 (&acc)[NB][MB], int mrow) const {
    float gmax = 0.f;  // MODE_MASKBITS with an e5m2 copy: max |dx| of the lane
    // the wave-uniform choices are made once, not per row or per store
    if constexpr (BF8) {
      if (a.y_bf8) store_rows<0, true>(a, acc, mrow, gmax);
      else store_rows<0, false>(a, acc, mrow, gmax);
      if (a.y_bf8 && a.bf8_amax) {
        gmax = wave_max(gmax);
        if ((threadIdx.x & 63) == 0 && gmax > 0.f) atomicMax(a.bf8_amax + (blockIdx.x & 63), __float_as_uint(gmax));
      }
    } else if constexpr (BASE == MODE_BIAS_RELU && RES) {
      store_rows<2, false>(a, acc, mrow, gmax);  // (two copies of the row groups spill on the 384-pixel tiles)
    } else if constexpr (BASE == MODE_BIAS_RELU) {
      if (a.mbits_out) store_rows<1, false>(a, acc, mrow, gmax);
      else store_rows<0, false>(a, acc, mrow, gmax);
    } else {
      store_rows<0, false>(a, acc, mrow, gmax);
    }
  }

  // Channel blocks i, i + 1 are stored as a pair.  Lanes l and l ^ 16 hold the same pixel; a
  // v_permlane16_swap per packed dword (odd 16-lane rows of block i <-> even rows of block i + 1) leaves
  // the even rows with 8 consecutive channels of block i and the odd rows with 8 of block i + 1: one
  // 16-byte store per lane and pair, 64 contiguous bytes per pixel and instruction, where the unpaired
  // form writes 16 separate 32-byte segments per instruction.  An odd NB keeps its last block on the
  // 8-byte store.  Both lanes of a pair share the pixel, hence the row-past-M test.
  // BITS: the ReLU' words are written (1), not written (0) or written where a.mbits_out is set (2); they
  // are computed before the swap, so their layout is the unpaired one.
  // E5M2: the e5m2 copy is written, paired the same way (two 4-byte words -> one 8-byte store).
  template <int BITS, bool E5M2>
  __device__ __forceinline__ void store_rows(const ConvFwdArgs& a, const f32x4 (&acc)[NB][MB], int mrow,
                                             float& gmax) const {
    const int po = (threadIdx.x & 16) ? 12 : 0;  // odd row: block i + 1, from the even partner's channel
    bf16x4 rs[RG][RES ? NB : 1];
    // block i of row j: epilogue arithmetic, the packed bf16 pair of dwords, the e5m2 word, the ReLU' bits
    auto block = [&](int i, int j, uint2& ow, uint32_t& pk, uint32_t& bits) {
      f32x4 v = acc[i][j];
      if constexpr (RES) {  // acc + bias + res (forward), acc + res (dgrad)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          v[r] = (BASE == MODE_BIAS_RELU ? v[r] + bb[i][r] : v[r]) + (float)rs[j % RG][i][r];
      }
      if constexpr (BASE == MODE_BIAS_RELU && RES) {
        v[0] = fmaxf(v[0], 0.f);
        v[1] = fmaxf(v[1], 0.f);
        v[2] = fmaxf(v[2], 0.f);
        v[3] = fmaxf(v[3], 0.f);
      } else if constexpr (BASE == MODE_BIAS_RELU) {
        v[0] = fmaxf(v[0] + bb[i][0], 0.f);
        v[1] = fmaxf(v[1] + bb[i][1], 0.f);
        v[2] = fmaxf(v[2] + bb[i][2], 0.f);
        v[3] = fmaxf(v[3] + bb[i][3], 0.f);
      } else if constexpr (BASE == MODE_MASK) {
        v[0] = (float)mk[i][j][0] > 0.f ? v[0] : 0.f;
        v[1] = (float)mk[i][j][1] > 0.f ? v[1] : 0.f;
        v[2] = (float)mk[i][j][2] > 0.f ? v[2] : 0.f;
        v[3] = (float)mk[i][j][3] > 0.f ? v[3] : 0.f;
      } else if constexpr (BASE == MODE_MASKBITS) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = ((mw[j] >> (4 * i + r)) & 1u) ? v[r] : 0.f;
      }
      bf16x4 o;
      o[0] = (__bf16)v[0];
      o[1] = (__bf16)v[1];
      o[2] = (__bf16)v[2];
      o[3] = (__bf16)v[3];
      if constexpr (BASE == MODE_BIAS_RELU) {
        // the bit records what the bf16 value the dgrad would re-read says: y > 0
#pragma unroll
        for (int r = 0; r < 4; ++r) bits |= ((float)o[r] > 0.f ? 1u : 0u) << (4 * i + r);
      }
      ow = __builtin_bit_cast(uint2, o);
      if constexpr (E5M2) {
        float sv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          gmax = fmaxf(gmax, fabsf(v[r]));
          sv[r] = fminf(fmaxf(v[r] * gsc, -57344.f), 57344.f);
        }
        int p = __builtin_amdgcn_cvt_pk_bf8_f32(sv[0], sv[1], 0, false);
        pk = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(sv[2], sv[3], p, true);
      }
    };
#pragma unroll
    for (int j = 0; j < MB; ++j) {
      if constexpr (RES) {
        if (j % RG == 0) {
#pragma unroll
          for (int jg = 0; jg < RG; ++jg)
#pragma unroll
            for (int i = 0; i < NB; ++i)
              if (j + jg < MB) rs[jg][i] = *(const bf16x4*)(a.res + ooff[j + jg < MB ? j + jg : j] + i * 16);
        }
      }
      if (mrow + j * 16 >= a.M) continue;
      uint32_t bits = 0u;
#pragma unroll
      for (int i = 0; i + 1 < NBP; i += 2) {
        uint2 o0, o1;
        uint32_t p0 = 0u, p1 = 0u;
        block(i, j, o0, p0, bits);
        block(i + 1, j, o1, p1, bits);
        const auto sx = __builtin_amdgcn_permlane16_swap(o0.x, o1.x, false, false);
        const auto sy = __builtin_amdgcn_permlane16_swap(o0.y, o1.y, false, false);
        u32x4_a8 q;
        q[0] = sx[0];
        q[1] = sy[0];
        q[2] = sx[1];
        q[3] = sy[1];
#ifdef AGK_DEBUG
        const long long yo = (long long)ooff[j] + i * 16 + po;
        if (AGK_DCHECK(yo >= 0 && yo + 8 <= a.y_elems, DBG_FWD_Y)) *(u32x4_a8*)(a.y + yo) = q;
#else
        *(u32x4_a8*)(a.y + ooff[j] + i * 16 + po) = q;
#endif
        if constexpr (E5M2) {
          const auto sp = __builtin_amdgcn_permlane16_swap(p0, p1, false, false);
          u32x2_a4 q8;
          q8[0] = sp[0];
          q8[1] = sp[1];
          *(u32x2_a4*)(a.y_bf8 + ooff[j] + i * 16 + po) = q8;
        }
      }
#pragma unroll
      for (int i = NBP / 2 * 2; i < NB; ++i) {  // unpaired blocks: the last one of an odd NB, all with a skip operand
        uint2 o0;
        uint32_t p0 = 0u;
        block(i, j, o0, p0, bits);
#ifdef AGK_DEBUG
        const long long yo = (long long)ooff[j] + i * 16;
        if (AGK_DCHECK(yo >= 0 && yo + 4 <= a.y_elems, DBG_FWD_Y)) *(uint2*)(a.y + yo) = o0;
#else
        *(uint2*)(a.y + ooff[j] + i * 16) = o0;
#endif
        if constexpr (E5M2) *(uint32_t*)(a.y_bf8 + ooff[j] + i * 16) = p0;
      }
      if constexpr (BITS != 0)
        if (BITS == 1 || a.mbits_out) a.mbits_out[(size_t)pix[j] * mwords + mslot] = bits;
    }
  }
};

template <int NB, int MB, int MODE>
__device__ __forceinline__ void conv_store_tile(const ConvFwdArgs& a, const f32x4 (&acc)[NB][MB], int mrow,
                                                int nbase, int wn) {
  ConvEpilogue<NB, MB, MODE> ep;
  ep.load(a, mrow, nbase, wn);
  ep.settle();
  ep.store(a, acc, mrow);
}

// ---------------- epilogue for the 32x32x16 MFMA layout (weights as A, pixels as B)
// acc[i][j] (f32x16) of a wave: output channel nbase + 32 i + 8 g + 4 h + r
// (h = lane >> 5, reg = 4 g + r) of pixel mrow + 32 j, mrow = the lane's pixel
// of block 0.  ReLU' bitmask: ConvEpilogue's layout, so any tile's dgrad can read this tile's bits
// and the reverse.  With cw = 32 i + 8 g + 4 h + r the channel's offset in its wave half, the
// layout's word is wn*4 + (cw % 16) / 4 and its bit 4 (cw / 16) + cw % 4: the lane's 16*NB bits sit in
// words blockIdx.y*8 + wn*4 + h (even g) and + 2 (odd g), bit 8 i + 4 (g / 2) + r.
template <int NB, int MB, int MODE>
struct ConvEpilogue32 {
  static constexpr int BASE = MODE & 3;
  static constexpr bool RES = (MODE & MODE_RES) != 0;  // skip operand, loaded per 4-channel group in store()
  static_assert(!RES || BASE == MODE_BIAS_RELU || BASE == MODE_MASKBITS, "skip operand: bias + ReLU or bitmask dgrad");
  int ooff[MB];
  int pix[MB];
  f32x4 bb[NB][4];
  bf16x4 mk[NB][MB][4];
  uint2 mw[MB];
  int mslot, mwords;

  __device__ __forceinline__ void load(const ConvFwdArgs& a, int mrow, int nbase, int wn) {
    const int SS = a.S * a.S;
    const int h = (threadIdx.x & 63) >> 5;
    mslot = blockIdx.y * 8 + wn * 4 + h;
    mwords = gridDim.y * 8;
#pragma unroll
    for (int j = 0; j < MB; ++j) {
      int m = mrow + j * 32;
      m = m < a.M ? m : a.M - 1;
      const int b = fdiv(m, a.divSS);
      const int rem = m - b * SS;
      const int ii = fdiv(rem, a.divS);
      const int jj = rem - ii * a.S;
      pix[j] = (b * a.HPo + ii + a.Po) * a.HPo + jj + a.Po;
      ooff[j] = pix[j] * a.Cout + nbase + 4 * h;
    }
    if constexpr (BASE == MODE_BIAS_RELU) {
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) bb[i][g] = *(const f32x4*)(a.bias + nbase + 4 * h + i * 32 + g * 8);
    } else if constexpr (BASE == MODE_MASK) {
#pragma unroll
      for (int j = 0; j < MB; ++j)
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int g = 0; g < 4; ++g) mk[i][j][g] = *(const bf16x4*)(a.mask + ooff[j] + i * 32 + g * 8);
    } else if constexpr (BASE == MODE_MASKBITS) {
#pragma unroll
      for (int j = 0; j < MB; ++j) {
        const uint32_t* p = a.mbits_in + (size_t)pix[j] * mwords + mslot;
        mw[j] = make_uint2(p[0], p[2]);
      }
    }
  }

  __device__ __forceinline__ void store(const ConvFwdArgs& a, const f32x16 (&acc)[NB][MB], int mrow) const {
#pragma unroll
    for (int j = 0; j < MB; ++j) {
      if (mrow + j * 32 >= a.M) continue;
      uint32_t bits[2] = {0u, 0u};
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = acc[i][j][4 * g + r];
          const int bit0 = 8 * i + 4 * (g >> 1);  // in word (g & 1)
          if constexpr (RES) {  // acc + bias + res (forward), acc + res (dgrad)
            const bf16x4 rs = *(const bf16x4*)(a.res + ooff[j] + i * 32 + g * 8);
#pragma unroll
            for (int r = 0; r < 4; ++r)
              v[r] = (BASE == MODE_BIAS_RELU ? v[r] + bb[i][g][r] : v[r]) + (float)rs[r];
          }
          if constexpr (BASE == MODE_BIAS_RELU && RES) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
          } else if constexpr (BASE == MODE_BIAS_RELU) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r] + bb[i][g][r], 0.f);
          } else if constexpr (BASE == MODE_MASK) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (float)mk[i][j][g][r] > 0.f ? v[r] : 0.f;
          } else if constexpr (BASE == MODE_MASKBITS) {
            const uint32_t w = (g & 1) ? mw[j].y : mw[j].x;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = ((w >> (bit0 + r)) & 1u) ? v[r] : 0.f;
          }
          bf16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (__bf16)v[r];
          if constexpr (BASE == MODE_BIAS_RELU) {
#pragma unroll
            for (int r = 0; r < 4; ++r) bits[g & 1] |= ((float)o[r] > 0.f ? 1u : 0u) << (bit0 + r);
          }
          *(bf16x4*)(a.y + ooff[j] + i * 32 + g * 8) = o;
        }
      if constexpr (BASE == MODE_BIAS_RELU)
        if (a.mbits_out) {
          uint32_t* p = a.mbits_out + (size_t)pix[j] * mwords + mslot;
          p[0] = bits[0];
          p[2] = bits[1];
        }
    }
  }
};


// forward variants in conv_fwd_variants.hip (tile codes -1, 2, 4, 5, 6, 32);
// returns false when the variant does not apply to the geometry
bool launch_conv_fwd_variant(int code, const ConvFwdArgs& a, int mode, hipStream_t st);

}  // namespace agk
