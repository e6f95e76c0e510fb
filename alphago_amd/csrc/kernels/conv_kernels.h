// Conv kernel templates shared by the production launchers (conv.hip) and the kernel lab
// (conv_lab.hip): the implicit-GEMM forward / dgrad kernel and the split-K wgrad kernel.  See conv.hip
// for the layout and the algorithm.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "common.h"
#include "conv_common.h"
#include "kernels.h"

namespace agk {

// ----------------------------------------------------------------- forward: tile descriptions
// A forward / dgrad tile is one type: its tile code, BM pixels per workgroup as waves of 16 MBW pixels x
// BN/2 channels, the K loop it runs and the loop's options.  conv_fwd_kernel<BN, MODE, Tile, STR>, the
// launchers, the dispatch (conv.hip) and the conv_fwd_tile_info op all read the same type.
enum class FwdLoop {
  Pipelined,        // two fragment sets: step ks + 1's first k-half is read under step ks's MFMAs; the epilogue
                    // operands ride along with the last stages
  PipelinedLateEp,  // the same loop, epilogue operands loaded after it (kernel lab)
  Plain,            // one fragment set (large wave tiles): read, then MFMA, per k-half
  DmaSpread,        // Plain with the next stage's LDS-DMA spread through the first k-half's MFMAs
  Mfma32,           // Plain on v_mfma_f32_32x32x16_bf16 (kernel lab)
  Ring,             // Pipelined on a SLOTS-deep LDS ring (kernel lab)
  CompactHalo,      // conv_fwd_halo384_kernel: the pixel rows staged once per 64-channel chunk
};

struct FwdTileDefaults {
  // chunk outer: the K loop runs the 64-channel chunk in the outer loop and the taps inside it, instead of
  // all chunks of one tap before the next tap.  A tile's pixel rows for one chunk (BM + 2 halo rows x
  // 128 B) are then re-read by the 9 taps while they are hot in the XCD's L2, where the tap-outer order
  // cycles through every chunk of the tile (BM x Cin x 2 B per tile, ~5 MB for the 32 tiles of an XCD at
  // Cin 192 -- more than its 4 MB L2).
  static constexpr bool CHUNK_OUTER = false;
  // split-K (small batches): blockIdx.z = split z of gridDim.z; the workgroup runs K-steps
  // [nK z / nz, nK (z+1) / nz) and writes its raw fp32 partial tile to a.sk_ws[z][m][n];
  // conv_splitk_finish_kernel sums the splits and applies the epilogue.  At B = 16 a 3x3 layer is 181
  // 32-pixel tiles of 27 serial K-steps (~0.7 us each, whatever the DMA scheme): splitting K shortens
  // that chain and fills the CUs.
  static constexpr bool SPLITK = false;
  // LDS stage buffers.  More than 2 (small batches): a ring, the DMA of step ks + SLOTS - 1 issued while
  // step ks computes.  With few workgroups per CU nothing else hides the global->LDS latency of a
  // 2-buffer loop (~0.75 us per K-step at B = 16, 27 steps per 3x3 layer: profiles/r3_small_batch/).
  static constexpr int SLOTS = 2;
};
template <int CODE_, int BM_, int MBW_, FwdLoop LOOP_>
struct FwdTileOf : FwdTileDefaults {
  static constexpr int CODE = CODE_, BM = BM_, MBW = MBW_;
  static constexpr FwdLoop LOOP = LOOP_;
};

// one type per tile code (docs/ARCHITECTURE.md has the table)
struct Tile36 : FwdTileOf<36, 32, 1, FwdLoop::Pipelined> {};  // 32 pixels on 4 waves of 16 x BN/2
struct Tile37 : FwdTileOf<37, 32, 2, FwdLoop::Pipelined> {};  // 32 pixels on 2 waves of 32 x BN/2
struct Tile38 : FwdTileOf<38, 32, 1, FwdLoop::Pipelined> { static constexpr bool SPLITK = true; };  // 36 with split-K
struct Tile64 : FwdTileOf<64, 64, 2, FwdLoop::Pipelined> {};
struct Tile128 : FwdTileOf<128, 128, 4, FwdLoop::Pipelined> {};
struct Tile256 : FwdTileOf<256, 256, 4, FwdLoop::Pipelined> {};
struct Tile384 : FwdTileOf<384, 384, 6, FwdLoop::Plain> {};  // 96 x BN/2 per wave
struct Tile385 : FwdTileOf<385, 384, 6, FwdLoop::DmaSpread> {};
struct Tile386 : FwdTileOf<386, 384, 6, FwdLoop::DmaSpread> { static constexpr bool CHUNK_OUTER = true; };
struct Tile387 : FwdTileOf<387, 384, 6, FwdLoop::Plain> { static constexpr bool CHUNK_OUTER = true; };
struct Tile388 : FwdTileOf<388, 384, 6, FwdLoop::CompactHalo> {  // 386's MFMA sequence, compact-halo staging
  static constexpr bool CHUNK_OUTER = true;
};
#ifdef AGK_KERNEL_LAB
// measured slower or equal, kernel lab only: the 64 / 128-pixel tiles on a 4 / 3-slot LDS ring (round 4), the
// epilogue operands loaded late, 128-pixel waves, the DMA spread and the 32x32 MFMA on other tiles
// (profiles/r1_fwd_kernel_experiments.md)
struct Tile65 : FwdTileOf<65, 64, 2, FwdLoop::Ring> { static constexpr int SLOTS = 4; };
struct Tile130 : FwdTileOf<130, 128, 4, FwdLoop::Ring> { static constexpr int SLOTS = 3; };
struct Tile2560 : FwdTileOf<2560, 256, 4, FwdLoop::PipelinedLateEp> {};
struct Tile2568 : FwdTileOf<2568, 256, 8, FwdLoop::Pipelined> {};
struct Tile7 : FwdTileOf<7, 384, 6, FwdLoop::Mfma32> {};
struct Tile8 : FwdTileOf<8, 256, 4, FwdLoop::Mfma32> {};
struct Tile10 : FwdTileOf<10, 256, 4, FwdLoop::DmaSpread> {};  // (lab code 9 is Tile385)
#endif

// compact-halo tile (conv_fwd_halo384_kernel below)
constexpr int H384_BM = 384;
constexpr int H384_SMAX = 19;                                          // largest board side covered
constexpr int H384_DATA = (H384_BM + 2 * (H384_SMAX + 1) + 7) / 8 * 8;  // data rows (whole 1-KB pieces): 424
constexpr int H384_ROWS = H384_DATA + 8;                               // + 8 zero rows
constexpr int H384_PIECES = H384_DATA / 8;                             // 53

// Launch geometry of a tile at output width BN, and what a tile may combine (the only place that says).
// STR: straddled K-steps (Cin % 64 == 32), a run-time property of the layer.
template <class T, int BN, bool STR = false>
struct FwdGeo {
  static constexpr bool HALO = T::LOOP == FwdLoop::CompactHalo;
  static constexpr int WAVES = T::BM / (16 * T::MBW) * 2;  // (BM / (16 MBW)) x 2, each 16 MBW (m) x BN/2 (n)
  static constexpr int THREADS = 64 * WAVES;
  static constexpr int LDS_BYTES = HALO ? 2 * H384_ROWS * 128 + 2 * BN * 128 : T::SLOTS * (T::BM * 128 + BN * 128);
  // per-wave weight rows that are no multiple of 8 (BN = 160): 8-row pieces dealt round-robin over the waves
  static constexpr bool BDIST = (BN / WAVES) % 8 != 0;
  static_assert(BN % 32 == 0 && (T::BM / WAVES) % 8 == 0, "tile geometry");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
  static_assert((T::SLOTS > 2) == (T::LOOP == FwdLoop::Ring), "more than two LDS slots: the ring loop, and only it");
  static_assert(T::LOOP != FwdLoop::Ring || !BDIST, "ring: the pipelined 16x16 loop, contiguous weight staging");
  static_assert(T::LOOP != FwdLoop::Mfma32 || (!BDIST && !STR && T::MBW % 2 == 0 && BN % 64 == 0),
                "32x32 loop: whole 32x32 tiles, no round-robin weight staging, no straddled K-steps");
  static_assert(!T::SPLITK || (T::LOOP == FwdLoop::Pipelined && !T::CHUNK_OUTER), "split-K: the pipelined 2-buffer loop, tap-outer order");
  static_assert(!HALO || (T::BM == H384_BM && T::MBW == 6 && T::CHUNK_OUTER && !STR), "compact halo: the 384-pixel chunk-outer tile");
  static dim3 grid(const ConvFwdArgs& a, int nz = 1) { return dim3((a.M + T::BM - 1) / T::BM, a.Cout / BN, nz); }
};

// MFMAs f0 <= f < f1 of a wave tile's NB x MB blocks (f = block (f / MB, f % MB)), unrolled: the DMA-spread
// loops issue them in runs between DMA pieces
template <int NB, int MB>
__device__ __forceinline__ void mfma_range(f32x4 (&acc)[NB][MB], const bf16x8 (&wa)[NB], const bf16x8 (&xa)[MB], int f0,
                                           int f1) {
#pragma unroll
  for (int f = 0; f < NB * MB; ++f)
    if (f >= f0 && f < f1) acc[f / MB][f % MB] = mfma16x16x32(wa[f / MB], xa[f % MB], acc[f / MB][f % MB]);
}

// ----------------------------------------------------------------- forward
// STR (Cin % 64 == 32, e.g. the value net's 152 filters padded to 160): a
// 64-channel K-step may straddle two taps -- the 32-channel half h of every
// staged row comes from its own (tap, channel) source, selected per lane by
// the row piece's logical chunk, so no MFMA multiplies padding.  The last
// step's second half (K = taps * Cin is an odd multiple of 32) reads an extra
// all-zero weight tap (packed weights then hold K*K + 1 taps).
template <int BN, int MODE, class Tile, bool STR = false>
__global__ __launch_bounds__((FwdGeo<Tile, BN, STR>::THREADS), 1) void conv_fwd_kernel(ConvFwdArgs a) {
  using G = FwdGeo<Tile, BN, STR>;
  constexpr int BM = Tile::BM, MBW = Tile::MBW, NS = Tile::SLOTS;
  constexpr FwdLoop LOOP = Tile::LOOP;
  constexpr bool EPF = LOOP == FwdLoop::Pipelined || LOOP == FwdLoop::Ring;  // epilogue operands prefetched
  constexpr bool PIPE = EPF || LOOP == FwdLoop::PipelinedLateEp;
  constexpr bool M32 = LOOP == FwdLoop::Mfma32, ILV = LOOP == FwdLoop::DmaSpread;
  constexpr bool CO = Tile::CHUNK_OUTER, SK = Tile::SPLITK;
  static_assert(!G::HALO, "the compact-halo tile has its own kernel");
  constexpr int NW = G::WAVES;  // waves per workgroup
  constexpr int NB = BN / 32;  // 16-wide n blocks per wave (a wave covers BN/2 channels)
  constexpr int MB = MBW;      // 16-wide m blocks per wave
  constexpr int A_BYTES = BM * 128;
  constexpr int B_BYTES = BN * 128;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int A_ROWS_PW = BM / NW;   // pixel rows staged per wave
  constexpr int A_INSTR = A_ROWS_PW / 8;
  constexpr bool BDIST = G::BDIST;  // weight pieces dealt round-robin
  constexpr int B_ROWS_PW = BN / NW;   // weight rows staged per wave (contiguous layout)
  constexpr int B_INSTR = BDIST ? (BN / 8 + NW - 1) / NW : B_ROWS_PW / 8;  // glds instructions per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int SS = a.S * a.S;
  const int CC = a.Cin >> 6;  // 64-channel chunks
  const int nK = STR ? (a.K * a.K * a.Cin + 63) >> 6 : a.K * a.K * CC;

  // --- staging addresses (element offsets)
  int arow[A_INSTR];
  bool ahi[A_INSTR], bhi[B_INSTR];  // STR: the piece's 32-channel half of the K-step
#pragma unroll
  for (int i = 0; i < A_INSTR; ++i) {
    const int r = wave * A_ROWS_PW + i * 8 + (lane >> 3);
    ahi[i] = (((lane & 7) ^ ((r >> 1) & 7)) >> 2) != 0;
    int m = m0 + r;
    m = m < a.M ? m : a.M - 1;
    const int b = fdiv(m, a.divSS);
    const int rem = m - b * SS;
    const int ii = fdiv(rem, a.divS);
    const int jj = rem - ii * a.S;
    const int logical = (lane & 7) ^ ((r >> 1) & 7);
    // STR: channel part (logical & 3) * 8 only; the half (logical >> 2) picks the source
    arow[i] = ((b * a.HPi + ii + a.offi) * a.HPi + jj + a.offi) * a.Cin + (STR ? (logical & 3) : logical) * 8;
  }
  int brow[B_INSTR], bldsrow[B_INSTR];
#pragma unroll
  for (int i = 0; i < B_INSTR; ++i) {
    const int piece = BDIST ? wave + i * NW : wave * (B_ROWS_PW / 8) + i;  // 8-row piece of the weight tile
    const int r = piece * 8 + (lane >> 3);
    const int logical = (lane & 7) ^ ((r >> 1) & 7);
    bhi[i] = (logical >> 2) != 0;
    brow[i] = (n0 + (r < BN ? r : BN - 1)) * a.Cin + (STR ? (logical & 3) : logical) * 8;
    bldsrow[i] = piece * 8;
  }

  const size_t wtap = (size_t)a.Cout * a.Cin;

  // staging cursor over (tap, 64-channel chunk), advanced incrementally with
  // scalar adds (no per-step integer divisions)
  int st_c0 = 0, st_kw = 0, st_a = 0, st_t = 0;
  size_t st_w = 0;
  // source offsets (without the lane's row/channel part) of the step's two
  // 32-channel halves; equal unless STR
  auto st_offsets = [&](int& xo0, int& xo1, size_t& wo0, size_t& wo1) {
    xo0 = st_a + st_c0;
    xo1 = xo0;
    wo0 = st_w + st_c0;
    wo1 = wo0;
    if constexpr (STR && CO) {
      // chunk outer: the 64-channel chunks run full steps tap by tap; the 32-channel tail chunk
      // (Cin % 64 == 32) pairs taps t and t+1 in one step (t = K*K: the all-zero extra tap)
      const bool part = st_c0 + 64 > a.Cin;
      const int a_next = st_a + (st_kw + 1 == a.K ? (a.HPi - a.K + 1) * a.Cin : a.Cin);
      xo1 = part ? (st_t + 1 < a.K * a.K ? a_next : st_a) + st_c0 : xo0 + 32;
      wo1 = part ? st_w + wtap + st_c0 : wo0 + 32;
    } else if constexpr (STR) {
      const int c1 = st_c0 + 32;
      const bool nx = c1 >= a.Cin;  // the second half opens the next tap
      const int a_next = st_a + (st_kw + 1 == a.K ? (a.HPi - a.K + 1) * a.Cin : a.Cin);
      // past the last tap: any in-range pixel rows (the weight tap there is all zero)
      xo1 = nx ? (st_t + 1 < a.K * a.K ? a_next : xo0) : st_a + c1;
      wo1 = nx ? st_w + wtap : st_w + c1;
    }
  };
  // DMA piece d of a stage: pixel pieces 0 .. A_INSTR-1, then weight pieces
  auto st_piece = [&](int d, char* base, int xo0, int xo1, size_t wo0, size_t wo1) {
    if (d < A_INSTR) {
      const int xo = arow[d] + ((STR && ahi[d]) ? xo1 : xo0);
      const bool ok = AGK_DCHECK(xo >= 0 && (long long)xo + 8 <= a.x_elems, DBG_FWD_X);
      glds16(a.x + (ok ? xo : 0), base + (wave * A_ROWS_PW + d * 8) * 128);
    } else {
      const int i = d - A_INSTR;
      if (BDIST && wave + i * NW >= BN / 8) return;  // wave-uniform: fewer pieces on the last waves
      const size_t wo = ((STR && bhi[i]) ? wo1 : wo0) + brow[i];
      const bool ok = AGK_DCHECK((long long)wo + 8 <= a.w_elems, DBG_FWD_W);
      glds16(ok ? a.w + wo : a.w, base + A_BYTES + bldsrow[i] * 128);
    }
  };
  // branch-free cursor advance (selects), so a caller can interleave the
  // DMA with MFMAs inside one basic block
  auto st_advance = [&]() {
    if constexpr (CO) {
      // one tap (two in the STR tail chunk, whose steps pair taps)
      const int nt = (STR && st_c0 + 64 > a.Cin) ? 2 : 1;
      st_t += nt;
      st_kw += nt;
      st_w += nt * wtap;
      st_a += nt * a.Cin;
      const bool wrap2 = st_kw >= a.K;
      st_kw = wrap2 ? st_kw - a.K : st_kw;
      st_a += wrap2 ? (a.HPi - a.K) * a.Cin : 0;
      const bool wrapt = st_t == a.K * a.K;  // all taps of the chunk done: next chunk, tap 0
      st_t = wrapt ? 0 : st_t;
      st_w = wrapt ? 0 : st_w;
      st_a = wrapt ? 0 : st_a;
      st_c0 += wrapt ? 64 : 0;
      return;
    }
    st_c0 += 64;
    const bool wrap = STR ? st_c0 >= a.Cin : st_c0 == a.Cin;
    st_c0 = wrap ? st_c0 - a.Cin : st_c0;
    st_w += wrap ? wtap : 0;
    st_t += wrap ? 1 : 0;
    st_kw += wrap ? 1 : 0;
    const bool wrap2 = st_kw == a.K;
    st_kw = wrap2 ? 0 : st_kw;
    st_a += (wrap ? a.Cin : 0) + (wrap2 ? (a.HPi - a.K) * a.Cin : 0);
  };
  auto stage = [&](int buf) {
    char* base = smem + buf * STAGE;
    int xo0, xo1;
    size_t wo0, wo1;
    st_offsets(xo0, xo1, wo0, wo1);
#pragma unroll
    for (int d = 0; d < A_INSTR + B_INSTR; ++d) st_piece(d, base, xo0, xo1, wo0, wo1);
    st_advance();
  };

  f32x4 acc[NB][MB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < MB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment read offsets: row*128 + (chunk ^ swz)*16, swz = ((row>>1)&7) = (lane&15)>>1
  const int swz = (lane & 15) >> 1;
  const int xrow0 = (wm * 16 * MB + (lane & 15)) * 128;
  const int wrow0 = A_BYTES + (wn * (BN / 2) + (lane & 15)) * 128;

  auto read_frags = [&](const char* base, int kk, bf16x8 (&xf)[MB], bf16x8 (&wf)[NB]) {
    const int choff = (((kk << 2) + (lane >> 4)) ^ swz) << 4;
#pragma unroll
    for (int j = 0; j < MB; ++j) xf[j] = *(const bf16x8*)(base + xrow0 + j * 16 * 128 + choff);
#pragma unroll
    for (int i = 0; i < NB; ++i) wf[i] = *(const bf16x8*)(base + wrow0 + i * 16 * 128 + choff);
  };
  auto mfmas = [&](const bf16x8 (&xf)[MB], const bf16x8 (&wf)[NB]) {
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < MB; ++j) acc[i][j] = mfma16x16x32(wf[i], xf[j], acc[i][j]);
  };

  // software pipeline: the first half (k 0..31) of step ks+1 is read right
  // after the barrier that publishes it, so its LDS latency hides under the
  // staging issue and the second-half reads of the next iteration.
  bf16x8 xa[MB], wa[NB], xb[MB], wb[NB];
  const int ep_mrow = m0 + wm * 16 * MB + (lane & 15);
  const int ep_nbase = n0 + wn * (BN / 2) + ((lane >> 4) << 2);
  ConvEpilogue<NB, MB, MODE> ep;
  const int ep_at = EPF ? (nK > 2 ? nK - 2 : 0) : nK - 1;
  if constexpr (NS > 2) {
    // DMA instructions per wave per stage (the vmcnt unit of one stage)
    constexpr int PW = A_INSTR + B_INSTR;
    static_assert(PW * (NS - 2) <= 63, "vmcnt range");
#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
      if (s < nK) stage(s);  // workgroup-uniform
    for (int ks = 0; ks < nK; ++ks) {
      // step ks has landed once at most (stages issued after it) x PW DMAs are outstanding
      const int later = (nK - 1 - ks) < (NS - 2) ? (nK - 1 - ks) : (NS - 2);
      ring_wait<PW, NS - 2>(later);
      __syncthreads();  // every wave's DMA of step ks is visible; slot (ks - 1) % NS is free
      if (ks + NS - 1 < nK) stage((ks + NS - 1) % NS);
      const char* base = smem + (ks % NS) * STAGE;
      read_frags(base, 0, xa, wa);
      read_frags(base, 1, xb, wb);
      if (ks == ep_at) ep.load(a, ep_mrow, ep_nbase, wn);
      __builtin_amdgcn_s_setprio(1);
      mfmas(xa, wa);
      mfmas(xb, wb);
      __builtin_amdgcn_s_setprio(0);
    }
    ep.settle();
    ep.store(a, acc, ep_mrow);
    return;
  }
  if constexpr (SK) {
    const int z = blockIdx.z, nz = gridDim.z;
    const int kb = (int)((long)nK * z / nz), ke = (int)((long)nK * (z + 1) / nz);
    for (int i = 0; i < kb; ++i) st_advance();  // scalar cursor to step kb
    if (kb < ke) {  // workgroup-uniform
      stage(0);
      wait_vmcnt0();
      __syncthreads();
      read_frags(smem, 0, xa, wa);
      for (int ks = kb; ks < ke; ++ks) {
        const int cur = (ks - kb) & 1;
        const char* base = smem + cur * STAGE;
        if (ks + 1 < ke) stage(cur ^ 1);
        read_frags(base, 1, xb, wb);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        mfmas(xa, wa);
        mfmas(xb, wb);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        wait_vmcnt0();
        __syncthreads();
        if (ks + 1 < ke) read_frags(smem + (cur ^ 1) * STAGE, 0, xa, wa);
      }
    }
    // raw partial sums: lane owns channels ep_nbase + 16 i + [0, 4) of pixel ep_mrow + 16 j
    float* ws = a.sk_ws + (size_t)z * a.M * a.Cout;
#pragma unroll
    for (int j = 0; j < MB; ++j) {
      const int m = ep_mrow + j * 16;
      if (m >= a.M) continue;
#pragma unroll
      for (int i = 0; i < NB; ++i) *(f32x4*)(ws + (size_t)m * a.Cout + ep_nbase + i * 16) = acc[i][j];
    }
    return;
  }
  int xo00, xo01;  // step 0's source offsets (ILV: the re-staged operands when nK == 1)
  size_t wo00, wo01;
  st_offsets(xo00, xo01, wo00, wo01);
  stage(0);
  wait_vmcnt0();
  __syncthreads();
  if constexpr (M32) {
    // v_mfma_f32_32x32x16_bf16: an MFMA holds the SIMD's vector issue for 8 of
    // 32 cycles (8 of 16 for 16x16x32), leaving the co-resident wave more room
    // for its LDS reads and DMA issue.  Wave tile 16*MBW pixels x BN/2 channels
    // as (MBW/2) x (BN/64) 32x32 tiles; epilogue in the 32x32 C/D layout.
    constexpr int NB2 = BN / 64, MB2 = MBW / 2;
    f32x16 acc2[NB2][MB2];
#pragma unroll
    for (int i = 0; i < NB2; ++i)
#pragma unroll
      for (int j = 0; j < MB2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc2[i][j][e] = 0.f;
    const int h = lane >> 5;
    const int l31 = lane & 31;
    const int xr0 = wm * 16 * MB + l31;         // tile row of block 0 (blocks are 32-aligned)
    const int wr0 = wn * (BN / 2) + l31;
    const int sw = (l31 >> 1) & 7;               // (row >> 1) & 7 for every 32-aligned block
    for (int ks = 0; ks < nK; ++ks) {
      const int cur = ks & 1;
      const char* base = smem + cur * STAGE;
      if (ks + 1 < nK) stage(cur ^ 1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 xf2[2][MB2], wf2[2][NB2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const int co = ((((2 * kk + s2) << 1) + h) ^ sw) << 4;
#pragma unroll
          for (int j = 0; j < MB2; ++j) xf2[s2][j] = *(const bf16x8*)(base + (xr0 + j * 32) * 128 + co);
#pragma unroll
          for (int i = 0; i < NB2; ++i) wf2[s2][i] = *(const bf16x8*)(base + A_BYTES + (wr0 + i * 32) * 128 + co);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int i = 0; i < NB2; ++i)
#pragma unroll
            for (int j = 0; j < MB2; ++j)
              acc2[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf2[s2][i], xf2[s2][j], acc2[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
      wait_vmcnt0();
      __syncthreads();
    }
    ConvEpilogue32<NB2, MB2, MODE> ep2;
    ep2.load(a, m0 + wm * 16 * MB + l31, n0 + wn * (BN / 2), wn);
    ep2.store(a, acc2, m0 + wm * 16 * MB + l31);
    return;
  }
  if constexpr (!PIPE && ILV) {
    // The 2-buffer loop issues the next stage's LDS-DMA as one burst at the top
    // of every step; with both waves of a SIMD in lockstep the matrix pipe
    // idles while they wait on DMA issue.  Here the burst is spread through
    // the first k-half's MFMAs (one DMA piece per MPD MFMAs, order pinned with
    // sched_barrier) so DMA issue overlaps matrix work.
    constexpr int NDMA = A_INSTR + B_INSTR;
    constexpr int NMF = NB * MB;
    constexpr int MPD = NMF / (NDMA + 1);
    // The last step re-stages its own (in-range) operands into the idle buffer instead of
    // branching around each DMA piece: a uniform `if (more)` compiled to one s_cbranch per piece
    // inside the MFMA stream.
    int lxo0 = xo00, lxo1 = xo01;
    size_t lwo0 = wo00, lwo1 = wo01;
    for (int ks = 0; ks < nK; ++ks) {
      const int cur = ks & 1;
      const char* base = smem + cur * STAGE;
      const bool more = ks + 1 < nK;
      read_frags(base, 0, xa, wa);
      char* nb = smem + (cur ^ 1) * STAGE;
      int xo0, xo1;
      size_t wo0, wo1;
      st_offsets(xo0, xo1, wo0, wo1);
      xo0 = more ? xo0 : lxo0;
      xo1 = more ? xo1 : lxo1;
      wo0 = more ? wo0 : lwo0;
      wo1 = more ? wo1 : lwo1;
      lxo0 = xo0;
      lxo1 = xo1;
      lwo0 = wo0;
      lwo1 = wo1;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int d = 0; d < NDMA; ++d) {
        mfma_range(acc, wa, xa, d * MPD, (d + 1) * MPD);
        __builtin_amdgcn_sched_barrier(0);
        st_piece(d, nb, xo0, xo1, wo0, wo1);
        __builtin_amdgcn_sched_barrier(0);
      }
      mfma_range(acc, wa, xa, NDMA * MPD, NMF);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      st_advance();
      read_frags(base, 1, xa, wa);
      __builtin_amdgcn_s_setprio(1);
      mfmas(xa, wa);
      __builtin_amdgcn_s_setprio(0);
      wait_vmcnt0();
      __syncthreads();
    }
    ep.load(a, ep_mrow, ep_nbase, wn);
    ep.settle();
    ep.store(a, acc, ep_mrow);
    return;
  }
  if constexpr (!PIPE) {  // one fragment set (large wave tiles): read, then MFMA, per k-half
    for (int ks = 0; ks < nK; ++ks) {
      const int cur = ks & 1;
      const char* base = smem + cur * STAGE;
      if (ks + 1 < nK) stage(cur ^ 1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        read_frags(base, kk, xa, wa);
        __builtin_amdgcn_s_setprio(1);
        mfmas(xa, wa);
        __builtin_amdgcn_s_setprio(0);
      }
      wait_vmcnt0();
      __syncthreads();
    }
    ep.load(a, ep_mrow, ep_nbase, wn);
    ep.settle();
    ep.store(a, acc, ep_mrow);
    return;
  }
  read_frags(smem, 0, xa, wa);
  for (int ks = 0; ks < nK; ++ks) {
    const int cur = ks & 1;
    const char* base = smem + cur * STAGE;
    if (ks + 1 < nK) stage(cur ^ 1);
    if (ks == ep_at) ep.load(a, ep_mrow, ep_nbase, wn);  // epilogue operands ride along with the last stages
    read_frags(base, 1, xb, wb);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    mfmas(xa, wa);
    mfmas(xb, wb);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    wait_vmcnt0();
    __syncthreads();
    if (ks + 1 < nK) read_frags(base + (cur ^ 1) * STAGE - cur * STAGE, 0, xa, wa);
  }

  // --- epilogue: lane owns channels n..n+3 of pixel m for every (i, j) block
  ep.settle();
  ep.store(a, acc, ep_mrow);
}

// Launch KERNEL with LDS bytes of dynamic LDS: the limit is raised once per kernel (thread-safe static) and checked
template <auto KERNEL, int THREADS, int LDS, class... Args>
static void launch_dyn_lds(dim3 grid, hipStream_t st, const Args&... args) {
  static const hipError_t attr = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  hip_check(attr, "hipFuncSetAttribute(max dynamic LDS)");
  hipLaunchKernelGGL(KERNEL, grid, dim3(THREADS), LDS, st, args...);
}

// one launch of conv_fwd_kernel: threads, LDS and grid are the tile's (FwdGeo)
template <int BN, int MODE, class Tile, bool STR>
static void launch_fwd_kernel(const ConvFwdArgs& a, dim3 grid, hipStream_t st) {
  using G = FwdGeo<Tile, BN, STR>;
  launch_dyn_lds<conv_fwd_kernel<BN, MODE, Tile, STR>, G::THREADS, G::LDS_BYTES>(grid, st, a);
}

// ----------------------------------------------------------------- forward, compact-halo 384 tile (code 388)
// The production 384-pixel loop (96 x 96 per wave, chunk-outer K order, one vmcnt(0) + barrier per
// K-step, DMA spread through the first k-half's MFMAs) with the pixel operand staged ONCE per
// 64-channel chunk instead of once per tap.  The nine taps of a chunk read the same pixel rows, only
// shifted: tile 386 gathers 9 x 48 KB of them from L2 per chunk where 384 + 2 (S + 1) rows (53 KB at
// S = 19) are distinct.  Here a K-step's DMA is the 24 KB weight tile (3 pieces per wave) plus, in the
// first seven taps of a chunk, one piece per wave of the NEXT chunk's halo: 4 pieces per wave and step
// instead of 9.
// Halo rows are compact pixel indices: row r of a halo buffer holds interior pixel m0 - (S + 1) + r
// (clamped into [0, M)), so the 16 pixels of an MFMA block are 16 consecutive rows for every tap; a
// tap that leaves the board reads one of the 8 zero rows behind the data rows (the zero border of the
// padded layout).  Inside a 16-pixel block the lanes take even pixels (lanes 0-3, 12-15) and odd
// pixels (lanes 4-11), which keeps ds_read_b128 conflict-free at every row alignment the tap shifts
// produce (conv_fwd_hpp_kernel, kernel-lab tile 5, measured this layout).
// Every accumulator sees tile 386's MFMA sequence with the same operands (chunks outer, taps
// ascending, k-halves ascending; zero rows for the zero border), so the outputs are bit-identical.
// The nine taps are unrolled: tap offsets, the border test and the DMA schedule of a step are
// compile-time, and the MFMA stream has no branch.  LDS: 2 halo buffers + 2 weight slots.

template <int V>
struct IntC { static constexpr int value = V; };

// STAMP (kernel lab, the op's stamp buffer): four cycle counts per wave around the epilogue, see the end
template <int BN, int MODE, bool STAMP = false>
__global__ __launch_bounds__(512, 1) void conv_fwd_halo384_kernel(ConvFwdArgs a) {
  constexpr int BM = H384_BM, MB = 6, NW = 8;
  constexpr int NB = BN / 32;
  constexpr int NMF = NB * MB;
  constexpr int H_BYTES = H384_ROWS * 128;
  constexpr int W_BYTES = BN * 128;
  constexpr int WP = BN / 8 / NW;                      // weight pieces per wave and step
  constexpr int HPW = (H384_PIECES + NW - 1) / NW;     // halo pieces per wave and chunk
  static_assert(BN % 64 == 0 && BM == NW / 2 * 16 * MB, "tile geometry");
  static_assert(2 * H_BYTES + 2 * W_BYTES <= 160 * 1024, "LDS: two halo buffers and two weight slots, S <= 19");
  static_assert(HPW <= 7, "the next chunk's halo is issued in the first seven taps");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const hbuf = smem;
  char* const wbuf = smem + 2 * H_BYTES;

  unsigned long long t_begin = 0;
  if constexpr (STAMP) t_begin = __builtin_amdgcn_s_memtime();
  const int lane = threadIdx.x & 63;
  const int wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int S = a.S;
  const int SS = S * S;
  const int CC = a.Cin >> 6;
  const int G = S + 1;  // largest |tap shift| in the compact pixel index
  const int Pc = a.offi + 1;

  // --- DMA sources.  Halo piece i of a wave is piece min(8 i + wave, last) of the chunk (the waves
  // past the last piece re-issue it: same bytes to the same rows); the padded-NHWC address of a row's
  // pixel does not depend on the chunk, so it is computed once.
  int hoff[HPW];
#pragma unroll
  for (int i = 0; i < HPW; ++i) {
    const int k = i * NW + wave < H384_PIECES ? i * NW + wave : H384_PIECES - 1;
    const int r = k * 8 + (lane >> 3);
    int m = m0 - G + r;
    m = m < 0 ? 0 : (m >= a.M ? a.M - 1 : m);
    const int b = fdiv(m, a.divSS);
    const int rem = m - b * SS;
    const int ii = fdiv(rem, a.divS);
    const int q = (b * a.HPi + ii + Pc) * a.HPi + (rem - ii * S) + Pc;
    hoff[i] = q * a.Cin + (((lane & 7) ^ ((r >> 1) & 7)) << 3);
  }
  auto halo_piece = [&](int i, int c, int buf) {
    const int k = i * NW + wave < H384_PIECES ? i * NW + wave : H384_PIECES - 1;
    const int xo = hoff[i] + c * 64;
    const bool ok = AGK_DCHECK(xo >= 0 && (long long)xo + 8 <= a.x_elems, DBG_FWD_X);
    glds16(a.x + (ok ? xo : 0), hbuf + buf * H_BYTES + k * 1024);
  };
  int wrow[WP];
#pragma unroll
  for (int i = 0; i < WP; ++i) {
    const int r = (wave * WP + i) * 8 + (lane >> 3);
    wrow[i] = (n0 + r) * a.Cin + (((lane & 7) ^ ((r >> 1) & 7)) << 3);
  }
  const int wtap = a.Cout * a.Cin;  // 32-bit weight offsets (the launcher checks 9 taps fit)
  auto w_piece = [&](int i, int wo, int slot) {  // wo: (tap, chunk) offset of the step
    const int o = wo + wrow[i];
    const bool ok = AGK_DCHECK((long long)o + 8 <= a.w_elems, DBG_FWD_W);
    glds16(ok ? a.w + o : a.w, wbuf + slot * W_BYTES + (wave * WP + i) * 1024);
  };

  // --- the lane's pixels: block j holds pixel m0 + 96 wm + 16 j + pix16; bit 6 t + j of okm (taps 0-4
  // in word 0, 5-8 in word 1) = tap t of block j stays on the board.  Pixels past M (last tile) read
  // in-range rows and are not stored.
  const int li = lane & 15;
  const int pix16 = li < 4 ? 2 * li : (li < 12 ? 2 * (li - 4) + 1 : 2 * (li - 12) + 8);
  const int prel0 = G + wm * 16 * MB + pix16;  // halo row of block 0's pixel at the centre tap
  int okm[2] = {0, 0};
#pragma unroll
  for (int j = 0; j < MB; ++j) {
    int m = m0 + wm * 16 * MB + j * 16 + pix16;
    m = m < a.M ? m : a.M - 1;
    const int b = fdiv(m, a.divSS);
    const int rem = m - b * SS;
    const int py = fdiv(rem, a.divS);
    const int px = rem - py * S;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const bool ok = (unsigned)(py + t / 3 - 1) < (unsigned)S && (unsigned)(px + t % 3 - 1) < (unsigned)S;
      okm[t / 5] |= ok ? 1 << ((t % 5) * MB + j) : 0;
    }
  }

  f32x4 acc[NB][MB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < MB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int kq = lane >> 4;  // the lane's 16-B chunk of a k-half
  const int wfrag0 = (wn * (BN / 2) + (lane & 15)) * 128 + ((kq ^ ((lane & 15) >> 1)) << 4);
  bf16x8 xa[MB], wa[NB];

  // prologue: the zero rows of both halo buffers, chunk 0's halo, W(tap 0, chunk 0)
  if (wave < 2) *(uint4*)(hbuf + wave * H_BYTES + H384_DATA * 128 + lane * 16) = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int i = 0; i < HPW; ++i) halo_piece(i, 0, 0);
#pragma unroll
  for (int i = 0; i < WP; ++i) w_piece(i, 0, 0);
  wait_vmcnt0();
  __syncthreads();

  int ws = 0;  // weight slot of the current step
  // one K-step: tap T of chunk c.  NEXT: chunk c + 1 exists (its halo is prefetched; tap 8 stages its W).
  auto step = [&](auto tc, auto nc, int c) {
    constexpr int T = decltype(tc)::value;
    constexpr bool NEXT = decltype(nc)::value != 0;
    constexpr int NWP = (T < 8 || NEXT) ? WP : 0;       // weight pieces of the next step
    constexpr int NHP = (NEXT && T < HPW) ? 1 : 0;      // halo piece of the next chunk
    constexpr int NDMA = NWP + NHP;
    constexpr int MPD = NMF / (NDMA + 1);
    const char* hb = hbuf + (c & 1) * H_BYTES;
    const char* wb = wbuf + ws * W_BYTES + wfrag0;
    const int toff = (T / 3 - 1) * S + (T % 3 - 1);
    // The fragment offsets of a tap do not depend on the chunk: left alone, the compiler hoists all
    // 9 x 6 x 2 of them (and 54 lane masks of the border test) out of the chunk loop and spills.  The
    // empty asm makes them per-step values.
    int pr = prel0, om = okm[T / 5];
    asm volatile("" : "+v"(pr), "+v"(om));
    int xo[MB];
#pragma unroll
    for (int j = 0; j < MB; ++j) {
      const int r = pr + j * 16 + toff;
      // a tap off the board: the zero row with the lane's (row parity, chunk) bank slot
      const int row = (om & (1 << ((T % 5) * MB + j))) ? r : H384_DATA + (r & 7);
      xo[j] = row * 128 + ((kq ^ ((r >> 1) & 7)) << 4);
    }
#pragma unroll
    for (int j = 0; j < MB; ++j) xa[j] = *(const bf16x8*)(hb + xo[j]);
#pragma unroll
    for (int i = 0; i < NB; ++i) wa[i] = *(const bf16x8*)(wb + i * 16 * 128);
    int wo = T < 8 ? (T + 1) * wtap + c * 64 : (c + 1) * 64;
    asm volatile("" : "+s"(wo));  // likewise: no per-tap 64-bit lane addresses hoisted out of the chunk loop
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int d = 0; d < NDMA; ++d) {
      mfma_range(acc, wa, xa, d * MPD, (d + 1) * MPD);
      __builtin_amdgcn_sched_barrier(0);
      if (d < NWP) w_piece(d, wo, ws ^ 1);
      else halo_piece(T, c + 1, (c + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    mfma_range(acc, wa, xa, NDMA * MPD, NMF);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    // second k-half: chunk index ^ 4 = byte offset ^ 64
#pragma unroll
    for (int j = 0; j < MB; ++j) xa[j] = *(const bf16x8*)(hb + (xo[j] ^ 64));
#pragma unroll
    for (int i = 0; i < NB; ++i) wa[i] = *(const bf16x8*)(wbuf + ws * W_BYTES + (wfrag0 ^ 64) + i * 16 * 128);
    __builtin_amdgcn_s_setprio(1);
    mfma_range(acc, wa, xa, 0, NMF);
    __builtin_amdgcn_s_setprio(0);
    wait_vmcnt0();
    __syncthreads();
    ws ^= 1;
  };
  auto chunk = [&](auto nc, int c) {
    step(IntC<0>{}, nc, c);
    step(IntC<1>{}, nc, c);
    step(IntC<2>{}, nc, c);
    step(IntC<3>{}, nc, c);
    step(IntC<4>{}, nc, c);
    step(IntC<5>{}, nc, c);
    step(IntC<6>{}, nc, c);
    step(IntC<7>{}, nc, c);
    step(IntC<8>{}, nc, c);
  };
  for (int c = 0; c + 1 < CC; ++c) chunk(IntC<1>{}, c);
  chunk(IntC<0>{}, CC - 1);

  // (opaque: the epilogue's pixel addresses share the border test's divisions; computed before the
  // loop they would be spilled across it)
  int ep_mrow = m0 + wm * 16 * MB + pix16;
  asm volatile("" : "+v"(ep_mrow));
  const int ep_nbase = n0 + wn * (BN / 2) + ((lane >> 4) << 2);
  ConvEpilogue<NB, MB, MODE> ep;
  if constexpr (STAMP) {
    // diagnostic instantiation: cycles from the K loop's last barrier to (1) the operands settled, (2) the
    // last store issued, (3) every store acknowledged, and the wave's whole time; the debug buffer only
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    ep.load(a, ep_mrow, ep_nbase, wn);
    ep.settle();
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    ep.store(a, acc, ep_mrow);
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t2 = __builtin_amdgcn_s_memtime();
    wait_vmcnt0();
    const unsigned long long t3 = __builtin_amdgcn_s_memtime();
    if (lane == 0) {
      unsigned long long* d = a.dbg + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * NW + wave) * 4;
      d[0] = t1 - t0;
      d[1] = t2 - t0;
      d[2] = t3 - t0;
      d[3] = t3 - t_begin;
    }
    return;
  }
  ep.load(a, ep_mrow, ep_nbase, wn);
  ep.settle();
  ep.store(a, acc, ep_mrow);
}

// tile code 388: covers 3x3, Cin % 64 == 0, S <= 19 at BN = 192 in the bias + ReLU forward and the bitmask dgrad
static inline bool halo384_covers(int bn, int mode, int S, int K, int Cin, int Cout, int offi) {
  return bn == 192 && ((mode & 3) == MODE_BIAS_RELU || (mode & 3) == MODE_MASKBITS) && K == 3 && Cin % 64 == 0 &&
         Cin >= 64 && S <= H384_SMAX && offi >= 0 && 9ll * Cout * Cin < (1ll << 31);
}

template <int BN, int MODE>
static void launch_fwd_halo384(const ConvFwdArgs& a, hipStream_t st) {
  if constexpr (BN == 192 && ((MODE & 3) == MODE_BIAS_RELU || (MODE & 3) == MODE_MASKBITS)) {
    using G = FwdGeo<Tile388, BN>;
    auto plain = [&] { launch_dyn_lds<conv_fwd_halo384_kernel<BN, MODE>, G::THREADS, G::LDS_BYTES>(G::grid(a), st, a); };
#ifdef AGK_KERNEL_LAB
    if (a.dbg)  // diagnostic instantiation with epilogue stamps: 4 counts per wave, 8 waves per workgroup
      return launch_dyn_lds<conv_fwd_halo384_kernel<BN, MODE, true>, G::THREADS, G::LDS_BYTES>(G::grid(a), st, a);
#endif
    plain();
  } else {
    throw std::invalid_argument("conv_fwd: tile 388 is the 192-wide forward / bitmask dgrad");
  }
}

// Split-K finish: one thread per (pixel, bitmask word); word w of a pixel covers the channels
// tn * BN + wn * BN/2 + 4 q + 16 i + r (tn = w / 8, wn = (w / 4) % 2, q = w % 4; i < NB = BN / 32,
// r < 4) -- the channels one lane of the conv epilogue owns, so the bitmask layout is the tile's.
template <int MODE, int NB>
__global__ __launch_bounds__(256) void conv_splitk_finish_kernel(ConvFwdArgs a) {
  constexpr int BN = 32 * NB;
  constexpr int BASE = MODE & 3;
  constexpr bool RES = (MODE & MODE_RES) != 0;  // skip operand: added to the summed splits
  const int WPP = (a.Cout / BN) * 8;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long)a.M * WPP) return;
  const int m = (int)(gid / WPP), w = (int)(gid - (long)m * WPP);
  const int base = (w >> 3) * BN + ((w >> 2) & 1) * (BN / 2) + 4 * (w & 3);
  f32x4 v[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int z = 0; z < a.sk_nsplit; ++z) {
    const float* src = a.sk_ws + ((size_t)z * a.M + m) * a.Cout + base;
#pragma unroll
    for (int i = 0; i < NB; ++i) v[i] += *(const f32x4*)(src + 16 * i);
  }
  const int SS = a.S * a.S;
  const int b = fdiv(m, a.divSS);
  const int rem = m - b * SS;
  const int ii = fdiv(rem, a.divS);
  const int jj = rem - ii * a.S;
  const size_t pix = (size_t)(b * a.HPo + ii + a.Po) * a.HPo + jj + a.Po;
  uint32_t mw = 0u, bits = 0u;
  if constexpr (BASE == MODE_MASKBITS) mw = a.mbits_in[pix * WPP + w];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    float o4[4];
    bf16x4 rs;
    if constexpr (RES) rs = *(const bf16x4*)(a.res + pix * a.Cout + base + 16 * i);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float x = v[i][r];
      if constexpr (BASE == MODE_BIAS_RELU && RES) x = fmaxf(x + a.bias[base + 16 * i + r] + (float)rs[r], 0.f);
      else if constexpr (RES) x += (float)rs[r];
      else if constexpr (BASE == MODE_BIAS_RELU) x = fmaxf(x + a.bias[base + 16 * i + r], 0.f);
      if constexpr (BASE == MODE_MASKBITS) x = ((mw >> (4 * i + r)) & 1u) ? x : 0.f;
      o4[r] = x;
    }
    bf16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      o[r] = (__bf16)o4[r];
      if constexpr (BASE == MODE_BIAS_RELU) bits |= ((float)o[r] > 0.f ? 1u : 0u) << (4 * i + r);
    }
    *(bf16x4*)(a.y + pix * a.Cout + base + 16 * i) = o;
  }
  if constexpr (BASE == MODE_BIAS_RELU)
    if (a.mbits_out) a.mbits_out[pix * WPP + w] = bits;
}

// tile code 38: the 32-pixel tile (36) with split-K over a.sk_nsplit workgroups per tile, then the finish
// (BN = 160, the value width: STR straddled K-steps when Cin % 64 == 32, weight pieces dealt round-robin)
template <int BN, int MODE, class Tile, bool STR>
static void launch_fwd_splitk(const ConvFwdArgs& a, hipStream_t st) {
  if constexpr ((MODE & 3) == MODE_MASK) {
    throw std::invalid_argument("conv_fwd split-K: modes 0 (bias + ReLU), 2 (none) and 3 (bitmask dgrad)");
  } else {
    if (!a.sk_ws || a.sk_nsplit < 1 || a.y_bf8)
      throw std::invalid_argument("conv_fwd split-K (tile 38): needs a workspace and nsplit >= 1, no e5m2 copy");
    // the split pass writes raw partial sums: a skip operand (MODE_RES) is the finish kernel's alone
    launch_fwd_kernel<BN, MODE & 3, Tile, STR>(a, FwdGeo<Tile, BN>::grid(a, a.sk_nsplit), st);
    const long threads = (long)a.M * (a.Cout / BN) * 8;
    hipLaunchKernelGGL((conv_splitk_finish_kernel<MODE, BN / 32>), dim3((unsigned)((threads + 255) / 256)), dim3(256),
                       0, st, a);
  }
}

// launch a tile: the split-K pair, the compact-halo kernel, or conv_fwd_kernel over the tile's grid
template <int BN, int MODE, class Tile, bool STR = false>
static void launch_fwd_tile(const ConvFwdArgs& a, hipStream_t st) {
  if constexpr (Tile::SPLITK) launch_fwd_splitk<BN, MODE, Tile, STR>(a, st);
  else if constexpr (FwdGeo<Tile, BN>::HALO) launch_fwd_halo384<BN, MODE>(a, st);
  else launch_fwd_kernel<BN, MODE, Tile, STR>(a, FwdGeo<Tile, BN>::grid(a), st);
}

// ----------------------------------------------------------------- packed-tap forward (thin first layer)
// The first layer's input has cin_real <= 64 real planes in a 64-channel padded tensor (48 policy,
// 49 value).  conv_fwd_kernel multiplies all 64 channels of every tap, so a quarter of the layer-0
// MACs are zeros.  Here the K loop runs over (tap, 8-channel chunk) pairs of the real channels only:
// cpt = ceil(cin_real / 8) chunks per tap, 8 chunks (one 64-wide K-step) per step, chunk j of step s
// is q = 8 s + j = (tap q / cpt, channels 8 (q % cpt) ..).  48 planes: 25 x 6 = 150 chunks in 19 steps
// instead of 25.  Weights packed [step][Cout][64] in the same chunk order (pack_weights_kernel with
// PackLayer::pk_cpt), zero past the last chunk.  Each lane's DMA source is its own (tap, chunk): the
// wave-uniform step state keeps the offsets of taps t0, t0 + 1, t0 + 2 (a step spans at most three
// taps when cpt >= 4) and a piece selects one of them.  The MFMA loop, LDS layout and epilogue are
// those of the 384-pixel tile (96 x 96 per wave, one DMA burst per step).
template <int BN, int BM, int MBW>
__global__ __launch_bounds__(BM / MBW * 8, 1) void conv_fwd_pk_kernel(ConvFwdArgs a, int cpt) {
  constexpr int NW = BM / (16 * MBW) * 2;
  constexpr int NB = BN / 32;
  constexpr int MB = MBW;
  constexpr int A_BYTES = BM * 128;
  constexpr int B_BYTES = BN * 128;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int A_ROWS_PW = BM / NW;
  constexpr int A_INSTR = A_ROWS_PW / 8;
  constexpr bool BDIST = (BN / NW) % 8 != 0;
  constexpr int B_ROWS_PW = BN / NW;
  constexpr int B_INSTR = BDIST ? (BN / 8 + NW - 1) / NW : B_ROWS_PW / 8;
  static_assert(BN % 32 == 0 && A_ROWS_PW % 8 == 0, "tile geometry");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int SS = a.S * a.S;
  const int T = a.K * a.K;
  const int nK = (T * cpt + 7) >> 3;

  int arow[A_INSTR], alg[A_INSTR];
#pragma unroll
  for (int i = 0; i < A_INSTR; ++i) {
    const int r = wave * A_ROWS_PW + i * 8 + (lane >> 3);
    int m = m0 + r;
    m = m < a.M ? m : a.M - 1;
    const int b = fdiv(m, a.divSS);
    const int rem = m - b * SS;
    const int ii = fdiv(rem, a.divS);
    const int jj = rem - ii * a.S;
    alg[i] = (lane & 7) ^ ((r >> 1) & 7);
    arow[i] = ((b * a.HPi + ii + a.offi) * a.HPi + jj + a.offi) * a.Cin;
  }
  int brow[B_INSTR], bldsrow[B_INSTR];
#pragma unroll
  for (int i = 0; i < B_INSTR; ++i) {
    const int piece = BDIST ? wave + i * NW : wave * (B_ROWS_PW / 8) + i;
    const int r = piece * 8 + (lane >> 3);
    const int logical = (lane & 7) ^ ((r >> 1) & 7);
    brow[i] = (n0 + (r < BN ? r : BN - 1)) * 64 + logical * 8;
    bldsrow[i] = piece * 8;
  }

  // wave-uniform staging cursor: first chunk st_c of tap st_t = (st_kh, st_kw), weight step offset
  int st_c = 0, st_t = 0, st_kh = 0, st_kw = 0;
  size_t st_w = 0;
  const size_t wstep = (size_t)a.Cout * 64;
  auto stage = [&](int buf) {
    char* base = smem + buf * STAGE;
    // offsets of taps st_t, st_t + 1, st_t + 2 (past the last tap: the last tap's pixels, zero weights)
    int kh1 = st_kh, kw1 = st_kw + 1;
    if (kw1 == a.K) { kw1 = 0; ++kh1; }
    int kh2 = kh1, kw2 = kw1 + 1;
    if (kw2 == a.K) { kw2 = 0; ++kh2; }
    const int o0 = (st_kh * a.HPi + st_kw) * a.Cin;
    const int o1 = st_t + 1 < T ? (kh1 * a.HPi + kw1) * a.Cin : o0;
    const int o2 = st_t + 2 < T ? (kh2 * a.HPi + kw2) * a.Cin : o1;
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i) {
      const int e = st_c + alg[i];
      const int dt = (e >= cpt ? 1 : 0) + (e >= 2 * cpt ? 1 : 0);
      const int off = (dt == 0 ? o0 : dt == 1 ? o1 : o2) + (e - dt * cpt) * 8;
#ifdef AGK_DEBUG
      const int xo = arow[i] + off;
      const bool ok = AGK_DCHECK(xo >= 0 && (long long)xo + 8 <= a.x_elems, DBG_FWD_X);
      glds16(a.x + (ok ? xo : 0), base + (wave * A_ROWS_PW + i * 8) * 128);
#else
      glds16(a.x + arow[i] + off, base + (wave * A_ROWS_PW + i * 8) * 128);
#endif
    }
#pragma unroll
    for (int i = 0; i < B_INSTR; ++i) {
      if (BDIST && wave + i * NW >= BN / 8) continue;  // wave-uniform
      const bool ok = AGK_DCHECK((long long)(st_w + brow[i]) + 8 <= a.w_elems, DBG_FWD_W);
      glds16(ok ? a.w + st_w + brow[i] : a.w, base + A_BYTES + bldsrow[i] * 128);
    }
    // advance by 8 chunks (at most two tap boundaries when cpt >= 4)
    st_w += wstep;
    st_c += 8;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (st_c >= cpt) {
        st_c -= cpt;
        ++st_t;
        if (++st_kw == a.K) { st_kw = 0; ++st_kh; }
      }
    }
  };

  f32x4 acc[NB][MB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < MB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int swz = (lane & 15) >> 1;
  const int xrow0 = (wm * 16 * MB + (lane & 15)) * 128;
  const int wrow0 = A_BYTES + (wn * (BN / 2) + (lane & 15)) * 128;
  bf16x8 xf[MB], wf[NB];
  ConvEpilogue<NB, MB, MODE_BIAS_RELU> ep;
  const int ep_mrow = m0 + wm * 16 * MB + (lane & 15);
  const int ep_nbase = n0 + wn * (BN / 2) + ((lane >> 4) << 2);

  stage(0);
  wait_vmcnt0();
  __syncthreads();
  for (int ks = 0; ks < nK; ++ks) {
    const int cur = ks & 1;
    const char* base = smem + cur * STAGE;
    if (ks + 1 < nK) stage(cur ^ 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int choff = (((kk << 2) + (lane >> 4)) ^ swz) << 4;
#pragma unroll
      for (int j = 0; j < MB; ++j) xf[j] = *(const bf16x8*)(base + xrow0 + j * 16 * 128 + choff);
#pragma unroll
      for (int i = 0; i < NB; ++i) wf[i] = *(const bf16x8*)(base + wrow0 + i * 16 * 128 + choff);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < MB; ++j) acc[i][j] = mfma16x16x32(wf[i], xf[j], acc[i][j]);
      __builtin_amdgcn_s_setprio(0);
    }
    wait_vmcnt0();
    __syncthreads();
  }
  ep.load(a, ep_mrow, ep_nbase, wn);
  ep.settle();
  ep.store(a, acc, ep_mrow);
}

// ----------------------------------------------------------------- wgrad
// (lgkm_fence / ds_read_tr16_asm: conv_common.h)

// 512 threads = 8 waves as 2 (n) x 4 (c).  One pipeline stage = KSUB sub-steps
// of 32 pixels (one barrier per KSUB*32 pixels); each sub-step region is laid
// out [16-channel block][32 px][16 ch] for the transpose reads.
//
// TAPS > 1 (tap-merged, used when the c tile is 64 wide, i.e. the thin first
// layer): one workgroup owns a whole kernel row (TAPS == K taps, kw = 0..K-1)
// and reuses each staged dz tile for all of them; the x image of tap kw is the
// tap-0 image shifted by kw columns (kw * Cin elements).  This triples (5x5:
// quintuples) the MFMAs per staged dz byte, the limiter of the 64-wide tile.
// the split's partial tile D[n][c] (lane owns n..n+3 at column c) and the bias partial
template <int WN, int WC, int NWC, int TAPS, int NWN = 2>
__device__ __forceinline__ void wgrad_store(const ConvWgradArgs& a,
                                            const f32x4 (&acc)[TAPS][WN / (16 * NWN)][WC / (16 * NWC)],
                                            const float (&dbs)[WN / (16 * NWN)], unsigned bmask, int split, int t,
                                            int n0, int c0, int wn, int wc, int lane, int zero_split) {
  constexpr int NBn = WN / (16 * NWN), NBc = WC / (16 * NWC);
  const int nb0 = n0 + wn * (WN / NWN) + ((lane >> 4) << 2);
  const int cbase = c0 + wc * (WC / NWC) + (lane & 15);
  if (a.grad_w) {  // split-free plan: this workgroup holds the whole pixel sum -> the OIHW gradient
    const float sc = a.scale, be = a.beta;
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
      for (int i = 0; i < NBn; ++i)
#pragma unroll
        for (int j = 0; j < NBc; ++j) {
          const int c = cbase + j * 16;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int n = nb0 + i * 16 + r;
            if (n < a.cout_real && c < a.cin_real) {
              float* g = a.grad_w + ((size_t)n * a.cin_real + c) * a.T + t + tp;
              *g = (be != 0.f ? be * *g : 0.f) + sc * acc[tp][i][j][r];  // beta 0: no read of g
            }
          }
        }
    if (bmask && a.grad_b) {
#pragma unroll
      for (int i = 0; i < NBn; ++i) {
        if (!(bmask & (1u << i))) continue;
        float s = dbs[i];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        const int n = n0 + wn * (WN / NWN) + i * 16 + lane;
        if (lane < 16 && n < a.cout_real) a.grad_b[n] = (be != 0.f ? be * a.grad_b[n] : 0.f) + sc * s;
      }
    }
    return;
  }
#pragma unroll
  for (int tp = 0; tp < TAPS; ++tp) {
    float* out = a.slab + ((size_t)split * a.T + t + tp) * (size_t)a.Cout * a.Cin;
#pragma unroll
    for (int i = 0; i < NBn; ++i)
#pragma unroll
      for (int j = 0; j < NBc; ++j) {
        const int n = nb0 + i * 16;
        const int c = cbase + j * 16;
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(size_t)(n + r) * a.Cin + c] = acc[tp][i][j][r];
      }
  }
  if (zero_split >= 0) {  // PAIR's odd tap: the second split it covered contributes zeros
    float* out = a.slab + ((size_t)zero_split * a.T + t) * (size_t)a.Cout * a.Cin;
#pragma unroll
    for (int i = 0; i < NBn; ++i)
#pragma unroll
      for (int j = 0; j < NBc; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(size_t)(nb0 + i * 16 + r) * a.Cin + cbase + j * 16] = 0.f;
  }
  if (bmask) {
#pragma unroll
    for (int i = 0; i < NBn; ++i) {
      if (!(bmask & (1u << i))) continue;
      float s = dbs[i];
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (lane < 16) a.dbias_slab[(size_t)split * a.Cout + n0 + wn * (WN / NWN) + i * 16 + lane] = s;
    }
  }
}


// PAIR (3x3 only, with TAPS == 2, KSUB == 2): a workgroup owns two consecutive taps t, t+1 of
// any kernel rows (tstep = the element offset from tap t's x image to tap t+1's) and reuses each
// staged dz tile for both; per 64-pixel stage it moves 72 KB for 4.7 M MACs -- the forward's
// ratio and its one workgroup per CU -- instead of the per-tap kernel's 24 KB for 1.2 M.  The
// odd last tap (K*K = 9) runs the one-tap body over two splits' pixels, so every workgroup of
// the grid does the same MFMA work; it writes its sum into the first split's slab and zeros
// into the second's.
// NS > 2 (small batches): an NS-slot LDS ring instead of the double buffer (see conv_fwd_kernel);
// only for geometries whose waves each stage exactly IPW pieces per stage (the vmcnt unit).
// NWN: waves along n (2; the thin first layer's 12-wave variant has 4, see launch_wgrad_taps48).
// UP: unit pipelining inside a sub-step -- the x fragments of column unit u + 1 (a (tap, c block)
// pair) are read while the MFMAs of unit u run, instead of every fragment before the first MFMA;
// only the dz fragments and unit 0 stay exposed after the barrier.
template <int WN, int WC, int KSUB, int NWC, int TAPS, int NS = 2, int NWN = 2, bool UP = false, bool SPREAD = true>
__device__ __forceinline__ void wgrad_tile(const ConvWgradArgs& a, int split, int ks_begin, int ks_end, int t,
                                           int tstep, int n0, int c0, int zero_split) {
  // NWN (n) x NWC (c) waves; NWC = 2 gives each wave a 96x96 tile at 192x192
  // (a third fewer LDS fragment reads per MFMA than NWC = 4)
  constexpr int NWAVES = NWN * NWC;
  constexpr int NBn = WN / (16 * NWN);  // n blocks per wave (wave covers WN/NWN)
  constexpr int NBc = WC / (16 * NWC);  // c blocks per wave (wave covers WC/NWC)
  constexpr int DZ_BYTES = WN * 64;  // [WN/16][32 px][16 ch] bf16
  constexpr int X_BYTES = WC * 64 * TAPS;  // [TAPS][WC/16][32 px][16 ch]
  constexpr int SUB = DZ_BYTES + X_BYTES;
  constexpr int STAGE = SUB * KSUB;
  constexpr int XP = WC / 16;  // x pieces per tap
  constexpr int NINSTR = (WN / 16 + XP * TAPS) * KSUB;  // 1 KB glds pieces per stage
  constexpr int IPW = (NINSTR + NWAVES - 1) / NWAVES;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = wave_id();
  const int wn = wave / NWC, wc = wave % NWC;
  const int kh = t / a.K, kw = t - (t / a.K) * a.K;
  const int toff = (kh * a.HPi + kw) * a.Cin + c0;
  const int SS = a.S * a.S;

  // ---- staging addresses.  A lane's pixel of consecutive sub-steps advances by 32, and stage() is
  // called for consecutive stages of [ks_begin, ks_end), so the pixel's (board, row, column) is split by
  // division ONCE here and then stepped: (sj, si) and the running byte offsets move by the host's
  // per-step deltas (ConvWgradArgs::st_*), with one compare per wrap.  Offsets are 32-bit byte offsets
  // from wave-uniform base pointers (n0 / the tap offset / the piece live in the scalar base).
  // ONE: every wave stages only dz pieces or only x pieces (one scalar branch per stage instead of one
  // per piece) and walks only that tensor: the walk's constants are wave-uniform selects.
  // The step is split as whole boards + st_q rows + st_r columns (st_q, st_r < S), so one column wrap
  // and one row wrap per step cover every board size, those below 64 points included.
  // WALK false: the 5x5 tap-merged rows of the 160-wide n tile (162 VGPRs) have no room for the walk's
  // state at the workgroups per CU their grid is sized for (wgrad_plan), so they keep the division per
  // sub-step; everything else in this function is the same for them.
  constexpr bool ONE = KSUB == 1 && (WN / 16) % IPW == 0 && NINSTR == NWAVES * IPW;
  constexpr bool WALK = !(WN == 160 && TAPS == 5);
  constexpr int NT = ONE ? 1 : 2;            // tensors a wave walks: [0] = dz (ONE: its own), [1] = x
  constexpr int NDZW = ONE ? (WN / 16) / IPW : 0;  // ONE: waves below stage dz
  const bool wdz = !ONE || wave < NDZW;
  const int wHP[2] = {wdz ? a.HPo : a.HPi, a.HPi}, wP[2] = {wdz ? a.Po : a.offi, a.offi};
  const int wC[2] = {wdz ? a.Cout : a.Cin, a.Cin};
  const int wst[2] = {wdz ? a.dz_st : a.x_st, a.x_st}, wrow[2] = {wdz ? a.dz_row : a.x_row, a.x_row};
  const int wbrd[2] = {wdz ? a.dz_brd : a.x_brd, a.x_brd};
  const uint32_t half2 = (lane & 1) * 16;
  // lanes past the last pixel: dz element 0 (a zero border), x pixel M - 1 (finite)
  const uint32_t wtail[2] = {(wdz ? 0u : a.x_last) + half2, a.x_last + half2};
  const char* const dzb = (const char*)(a.dz + n0);
  const char* const xb = (const char*)(a.x + toff);
  int px = ks_begin * (32 * KSUB) + (lane >> 1);
  int sj, si;
  uint32_t woff[NT];
  auto locate = [&](int pm) {
    const int b = fdiv(pm, a.divSS);
    const int rem = pm - b * SS;
    si = fdiv(rem, a.divS);
    sj = rem - si * a.S;
#pragma unroll
    for (int k = 0; k < NT; ++k)
      woff[k] = (uint32_t)(((b * wHP[k] + si + wP[k]) * wHP[k] + sj + wP[k]) * wC[k]) * 2u + half2;
  };
  if constexpr (WALK) locate(px);
  auto advance = [&]() {
    px += 32;
    if constexpr (!WALK) return;
    sj += a.st_r;
    si += a.st_q;
    const bool cw = sj >= a.S;  // next row
    sj = cw ? sj - a.S : sj;
    si = cw ? si + 1 : si;
    const bool rw = si >= a.S;  // next board
    si = rw ? si - a.S : si;
#pragma unroll
    for (int k = 0; k < NT; ++k) woff[k] += (uint32_t)(wst[k] + (cw ? wrow[k] : 0) + (rw ? wbrd[k] : 0));
  };
  // source of x piece xj: tap xj / XP, channel piece xj % XP.  ONE: each of the wave's IPW piece bases
  // is pinned to a scalar register pair here, before the loop (sgpr_ptr), and the DMA takes it with the
  // lane's 32-bit offset.  The general path pins the two tensor bases only and adds the piece's
  // (wave-uniform) constant per piece: pinning every piece there would cost two v_readfirstlane per
  // piece inside the loop.
  const char* const dzp = sgpr_ptr(dzb);
  const char* const xp = sgpr_ptr(xb);
  auto xpiece = [&](int xj) { return xp + ((xj / XP) * tstep + (xj % XP) * 16) * 2; };
  auto dzpiece = [&](int jj) { return dzp + jj * 32; };
  const char* pb[IPW];  // ONE: this wave's piece bases
  if constexpr (ONE) {
#pragma unroll
    for (int i = 0; i < IPW; ++i)
      pb[i] = sgpr_ptr(wdz ? dzpiece(wave * IPW + i) : xpiece(wave * IPW + i - WN / 16));
  }

  // DEFER (one sub-step per stage): the caller advances after the stage's MFMAs are issued, so the
  // address arithmetic runs in their shadow and not between the barrier and the fragment reads
  constexpr bool DEFER = KSUB == 1;
  auto stage = [&](int buf) {
    char* base = smem + buf * STAGE;
#pragma unroll
    for (int sub = 0; sub < KSUB; ++sub) {
      uint32_t o[NT];
      if constexpr (!WALK) locate(px < a.M ? px : a.M - 1);
#pragma unroll
      for (int k = 0; k < NT; ++k) o[k] = px < a.M ? woff[k] : wtail[k];
      if constexpr (!DEFER) advance();
      // Debug build: every piece's element range is checked on the path the production build runs.
      // The offsets are unsigned, so an offset that went below zero shows as one far above the extent.
      if constexpr (ONE) {
#pragma unroll
        for (int i = 0; i < IPW; ++i) {
          const int pc = wave * IPW + i, xj = pc - WN / 16;
          const long long e =
              (long long)(o[0] >> 1) + (wdz ? n0 + pc * 16 : toff + (xj / XP) * tstep + (xj % XP) * 16);
          if (!AGK_DCHECK(e + 8 <= (wdz ? a.dz_elems : a.x_elems), wdz ? DBG_WG_DZ : DBG_WG_X)) {
            glds16(wdz ? a.dz : a.x, base + (wave * IPW + i) * 1024);
            continue;
          }
          glds16_so(pb[i], o[0], base + (wave * IPW + i) * 1024);
        }
        continue;
      }
      // dz pieces and x pieces in separate loops: a per-piece select between the
      // two source tensors makes hipcc drain vmcnt(0) before the LDS reads that
      // follow, which would turn the double buffer into a synchronous load
#pragma unroll
      for (int i = 0; i < IPW; ++i) {
        const int jj = wave * IPW + i - sub * (NINSTR / KSUB);
        if (jj >= 0 && jj < WN / 16) {
          const long long e = (long long)(o[0] >> 1) + n0 + jj * 16;
          if (!AGK_DCHECK(e + 8 <= a.dz_elems, DBG_WG_DZ)) {
            glds16(a.dz, base + sub * SUB + jj * 1024);
            continue;
          }
          glds16_so(dzpiece(jj), o[0], base + sub * SUB + jj * 1024);
        }
        // LDS ring with unequal piece counts: a wave past the last piece re-issues dz piece 0 (same
        // bytes to the same LDS address), so every wave has exactly IPW DMAs per stage -- the
        // vmcnt unit ring_wait counts in
        if constexpr (NS > 2) {
          if (jj >= NINSTR / KSUB) glds16_so(dzpiece(0), o[0], base + sub * SUB);
        }
      }
#pragma unroll
      for (int i = 0; i < IPW; ++i) {
        const int jj = wave * IPW + i - sub * (NINSTR / KSUB);
        if (jj >= WN / 16 && jj < NINSTR / KSUB) {
          const int xj = jj - WN / 16;
          const long long e = (long long)(o[NT - 1] >> 1) + toff + (xj / XP) * tstep + (xj % XP) * 16;
          if (!AGK_DCHECK(e + 8 <= a.x_elems, DBG_WG_X)) {
            glds16(a.x, base + sub * SUB + jj * 1024);
            continue;
          }
          glds16_so(xpiece(xj), o[NT - 1], base + sub * SUB + jj * 1024);
        }
      }
    }
  };

  f32x4 acc[TAPS][NBn][NBc];
#pragma unroll
  for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
    for (int i = 0; i < NBn; ++i)
#pragma unroll
      for (int j = 0; j < NBc; ++j) acc[tp][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbs[NBn];
#pragma unroll
  for (int i = 0; i < NBn; ++i) dbs[i] = 0.f;
  // bias partials (the pixel sums of dz).  Every wave with the same wn holds the same dz fragments in
  // the same lanes, in every tap's workgroup of the c0 == 0 column, so the NBn 16-channel blocks are
  // dealt out: block i goes to (tap group, wc) slot i % slots -- 36 slots for 6 blocks in the 3x3
  // 192 x 192 kernel, 15 for 3 in the first layer's rows -- and no wave carries more than one where the
  // slots suffice.  The per-lane sum is the same whoever computes it.  bmask bit i: this wave sums block i.
  // SPREAD false (PAIR, whose odd tap covers two splits): all blocks on the wc == 0 waves of tap 0.
  unsigned bmask = 0;
  if (c0 == 0) {
    if constexpr (SPREAD) {
      const int slots = (a.T / TAPS) * NWC, slot = (t / TAPS) * NWC + wc;
#pragma unroll
      for (int i = 0; i < NBn; ++i) bmask |= (i % slots == slot ? 1u : 0u) << i;
    } else if (t == 0 && wc == 0) {
      bmask = (1u << NBn) - 1u;
    }
  }
  bmask = __builtin_amdgcn_readfirstlane(bmask);
  // each block's sum under its own wave-uniform branch: eight elements in order, then the running
  // sum (separate chains per block are never packed into v_pk_add_f32)
  auto bias_add = [&](const bf16x8 (&af)[NBn]) {
    if (bmask == 0) return;
#pragma unroll
    for (int i = 0; i < NBn; ++i)
      if (bmask & (1u << i)) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s += (float)af[i][e];
        dbs[i] += s;
      }
  };

  // transposed-read addresses: group g = lane>>4, row q = (lane&15)>>2, col 4p, p = lane&3; the lane
  // reads rows 4g..4g+3 at tr0 and rows 16+4g..16+4g+3 512 bytes on.  One dz and one x address register
  // per wave (the buffer's offset folded in per stage); block, tap and sub-step are immediate offsets.
  const int g = lane >> 4;
  const int q = (lane & 15) >> 2;
  const int p = lane & 3;
  const uint32_t tr0 = (uint32_t)(uintptr_t)AG_LDS(smem) + (4 * g + q) * 32 + p * 8;
  const uint32_t fr_dz = tr0 + wn * NBn * 1024;
  const uint32_t fr_x = tr0 + DZ_BYTES + wc * NBc * 1024;
  constexpr int TRH = 16 * 32;  // second row group
  constexpr int NF = NBn + TAPS * NBc;  // fragments read per sub-step
  static_assert((KSUB - 1) * SUB + (TAPS * XP) * 1024 + TRH < 65536, "fragment reads: 16-bit immediate offsets");

  constexpr bool RING = NS > 2;
  static_assert(!RING || KSUB == 1, "ring: one sub-step per stage");
  static_assert(!RING || IPW * (NS - 2) <= 63, "vmcnt range");
  if constexpr (RING) {
#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
      if (ks_begin + s < ks_end) {
        stage(s);
        if constexpr (DEFER) advance();
      }
  } else if (ks_begin < ks_end) {
    stage(0);
    if constexpr (DEFER) advance();
    wait_vmcnt0();
    __syncthreads();
  }
  for (int ks = ks_begin; ks < ks_end; ++ks) {
    int cur = (ks - ks_begin) & 1;
    bool staged = false;
    if constexpr (RING) {
      const int later = (ks_end - 1 - ks) < (NS - 2) ? (ks_end - 1 - ks) : (NS - 2);
      ring_wait<IPW, (NS > 2 ? NS - 2 : 0)>(later);
      __syncthreads();  // stage ks visible to every wave; the slot read last step is free
      cur = (ks - ks_begin) % NS;
      if (ks + NS - 1 < ks_end) {
        stage((ks - ks_begin + NS - 1) % NS);
        staged = true;
      }
    } else if (ks + 1 < ks_end) {
      stage(cur ^ 1);
      staged = true;
    }
    const uint32_t cdz = fr_dz + cur * STAGE, cx = fr_x + cur * STAGE;
    static_for<KSUB>([&](auto sub_c) {
      constexpr int sub = decltype(sub_c)::value;
      bf16x4 tl[NF], th[NF];
      static_for<NBn>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        tl[i] = ds_read_tr16_at<sub * SUB + i * 1024>(cdz);
        th[i] = ds_read_tr16_at<sub * SUB + i * 1024 + TRH>(cdz);
      });
      if constexpr (UP) {
        constexpr int NU = TAPS * NBc;  // column units u = tp * NBc + j
        auto read_unit = [&](auto uc) {
          constexpr int u = decltype(uc)::value;
          constexpr int xo = sub * SUB + ((u / NBc) * XP + (u % NBc)) * 1024;
          tl[NBn + u] = ds_read_tr16_at<xo>(cx);
          th[NBn + u] = ds_read_tr16_at<xo + TRH>(cx);
        };
        read_unit(std::integral_constant<int, 0>{});
        bf16x8 af[NBn];
        static_for<NU>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          if constexpr (u + 1 < NU) read_unit(std::integral_constant<int, u + 1>{});
          // all but the two reads of unit u + 1 have returned (LDS reads complete in order)
          if constexpr (u == 0) {
#pragma unroll
            for (int i = 0; i < NBn; ++i) {
              if (NU > 1) lgkm_wait_pair<2>(tl[i], th[i]);
              else lgkm_wait_pair<0>(tl[i], th[i]);
              af[i] = bf16x8{tl[i][0], tl[i][1], tl[i][2], tl[i][3], th[i][0], th[i][1], th[i][2], th[i][3]};
            }
          }
          if (u + 1 < NU) lgkm_wait_pair<2>(tl[NBn + u], th[NBn + u]);
          else lgkm_wait_pair<0>(tl[NBn + u], th[NBn + u]);
          const bf16x8 bu = bf16x8{tl[NBn + u][0], tl[NBn + u][1], tl[NBn + u][2], tl[NBn + u][3],
                                   th[NBn + u][0], th[NBn + u][1], th[NBn + u][2], th[NBn + u][3]};
#pragma unroll
          for (int i = 0; i < NBn; ++i) acc[u / NBc][i][u % NBc] = mfma16x16x32(af[i], bu, acc[u / NBc][i][u % NBc]);
        });
        bias_add(af);
      } else {
        static_for<TAPS * NBc>([&](auto uc) {
          constexpr int u = decltype(uc)::value;  // tp * NBc + j
          constexpr int xo = sub * SUB + ((u / NBc) * XP + (u % NBc)) * 1024;
          tl[NBn + u] = ds_read_tr16_at<xo>(cx);
          th[NBn + u] = ds_read_tr16_at<xo + TRH>(cx);
        });
        lgkm_fence<NF>(tl, th);
        bf16x8 af[NBn], bfm[TAPS * NBc];
#pragma unroll
        for (int i = 0; i < NBn; ++i)
          af[i] = bf16x8{tl[i][0], tl[i][1], tl[i][2], tl[i][3], th[i][0], th[i][1], th[i][2], th[i][3]};
#pragma unroll
        for (int j = 0; j < TAPS * NBc; ++j)
          bfm[j] = bf16x8{tl[NBn + j][0], tl[NBn + j][1], tl[NBn + j][2], tl[NBn + j][3],
                          th[NBn + j][0], th[NBn + j][1], th[NBn + j][2], th[NBn + j][3]};
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
          for (int i = 0; i < NBn; ++i)
#pragma unroll
            for (int j = 0; j < NBc; ++j)
              acc[tp][i][j] = mfma16x16x32(af[i], bfm[tp * NBc + j], acc[tp][i][j]);
        bias_add(af);
      }
    });
    if constexpr (DEFER) {
      if (staged) advance();
    }
    if constexpr (!RING) {
      wait_vmcnt0();
      __syncthreads();
    }
  }

  wgrad_store<WN, WC, NWC, TAPS, NWN>(a, acc, dbs, bmask, split, t, n0, c0, wn, wc, lane, zero_split);
}

// LINE staging (wgrad variants 6 and 7): every DMA piece moves 8 whole 128-byte pixel lines (one
// 64-channel chunk of 8 pixels; lanes 8r..8r+7 fill line r, their 16-byte chunks XOR-swizzled by
// ((r >> 1) & 3) << 1) -- 8 cache lines per instruction instead of the 32 partial (32-byte) lines
// of wgrad_tile's [16 ch][32 px] pieces.  The LDS image of a sub-step is [64-ch chunk][32 px][128 B]
// and the transposed fragment reads address it directly (conflict-free: the 8 rows of a 32-lane
// group land on 8 distinct 8-bank column groups).  Piece gi = wave + NWAVES * d always has row
// group gi & 3 = wave & 3, so each lane stages one pixel per sub-step, as before.
template <int WN, int WC, int KSUB, int NWC, int TAPS, bool ILVW = false>
__device__ __forceinline__ void wgrad_tile_line(const ConvWgradArgs& a, int split, int ks_begin, int ks_end,
                                                int t, int tstep, int n0, int c0, int zero_split) {
  constexpr int NWAVES = 2 * NWC;
  static_assert(NWAVES % 4 == 0 && WN % 64 == 0 && WC % 64 == 0 && KSUB <= 2, "line staging geometry");
  constexpr int NBn = WN / 32;          // n blocks per wave (wave covers WN/2)
  constexpr int NBc = WC / (16 * NWC);  // c blocks per wave (wave covers WC/NWC)
  constexpr int NCN = WN / 64, NCC = WC / 64;  // 64-channel chunks of the two operands
  constexpr int DZ_BYTES = WN * 64;
  constexpr int X_BYTES = WC * 64 * TAPS;
  constexpr int SUB = DZ_BYTES + X_BYTES;
  constexpr int STAGE = SUB * KSUB;
  constexpr int DZP = WN / 16 * KSUB, XPS = WC / 16 * TAPS * KSUB;  // 1 KB pieces per stage
  static_assert((DZP + XPS) % NWAVES == 0, "pieces per wave");
  constexpr int NPW = (DZP + XPS) / NWAVES;  // piece gi = wave + NWAVES * d: dz pieces first, then x
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = wave_id();
  const int wn = wave / NWC, wc = wave % NWC;
  const int kh = t / a.K, kw = t - (t / a.K) * a.K;
  const int toff = (kh * a.HPi + kw) * a.Cin + c0;
  const int SS = a.S * a.S;
  const int pp = wave & 3;                  // row group (8 pixels) of every piece this wave stages
  const int r_st = pp * 8 + (lane >> 3);    // the pixel (LDS row) this lane stages in a sub-step
  const int lchunk = ((lane & 7) ^ (((r_st >> 1) & 3) << 1)) * 8;  // its swizzled 16-B chunk (elements)

  int dzr[KSUB], xr[KSUB];
  auto stage_addr = [&](int ks) {
#pragma unroll
    for (int sub = 0; sub < KSUB; ++sub) {
      const int px = (ks * KSUB + sub) * 32 + r_st;
      const int pm = px < a.M ? px : a.M - 1;
      const int b = fdiv(pm, a.divSS);
      const int rem = pm - b * SS;
      const int ii = fdiv(rem, a.divS);
      const int jx = rem - ii * a.S;
      dzr[sub] = (px < a.M ? ((b * a.HPo + ii + a.Po) * a.HPo + jx + a.Po) * a.Cout : 0) + n0 + lchunk;
      xr[sub] = ((b * a.HPi + ii + a.offi) * a.HPi + jx + a.offi) * a.Cin + toff + lchunk;
    }
  };
  // DMA pieces d0 <= d < d1 of the stage whose addresses stage_addr computed.  dz and x pieces in
  // separate loops under wave-uniform conditions (see wgrad_tile: a per-piece select between the
  // two tensors makes hipcc drain vmcnt before the LDS reads)
  auto stage_pieces = [&](int buf, int d0, int d1) {
    char* base = smem + buf * STAGE + pp * 1024;
#pragma unroll
    for (int d = 0; d < NPW; ++d) {
      if (d < d0 || d >= d1) continue;
      const int idx = (wave >> 2) + (NWAVES / 4) * d;  // (sub, chunk) of a dz piece
      if (idx >= DZP / 4) continue;
      const int sub = idx / NCN, cc = idx - sub * NCN;
      const int o = (KSUB == 2 && sub ? dzr[KSUB - 1] : dzr[0]) + cc * 64;
      const bool ok = AGK_DCHECK(o >= 0 && (long long)o + 8 <= a.dz_elems, DBG_WG_DZ);
      glds16(ok ? a.dz + o : a.dz, base + sub * SUB + cc * 4096);
    }
#pragma unroll
    for (int d = 0; d < NPW; ++d) {
      if (d < d0 || d >= d1) continue;
      const int idx = (wave >> 2) + (NWAVES / 4) * d - DZP / 4;  // (sub, tap, chunk) of an x piece
      if (idx < 0) continue;
      const int sub = idx / (TAPS * NCC), rem = idx - sub * (TAPS * NCC);
      const int tp = rem / NCC, cc = rem - tp * NCC;
      const int o = (KSUB == 2 && sub ? xr[KSUB - 1] : xr[0]) + tp * tstep + cc * 64;
      const bool ok = AGK_DCHECK(o >= 0 && (long long)o + 8 <= a.x_elems, DBG_WG_X);
      glds16(ok ? a.x + o : a.x, base + sub * SUB + DZ_BYTES + (tp * NCC + cc) * 4096);
    }
  };
  auto stage = [&](int ks, int buf) {
    stage_addr(ks);
    stage_pieces(buf, 0, NPW);
  };

  f32x4 acc[TAPS][NBn][NBc];
#pragma unroll
  for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
    for (int i = 0; i < NBn; ++i)
#pragma unroll
      for (int j = 0; j < NBc; ++j) acc[tp][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbs[NBn];
#pragma unroll
  for (int i = 0; i < NBn; ++i) dbs[i] = 0.f;
  const bool do_bias = (t == 0) && (c0 == 0) && (wc == 0);

  // transposed reads: lane (g = lane>>4, q = (lane&15)>>2, p = lane&3) reads row 4g+q (16+4g+q),
  // channels 4p..4p+3 of a 16-channel block: byte 32 (blk & 3) + 8p of the row, swizzled
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int rr = 4 * g + q;
  const int swz = ((rr >> 1) & 3) << 1;
  const int roff0 = rr * 128 + (p & 1) * 8;
  const int roff1 = roff0 + 16 * 128;
  auto blk_off = [&](int blk) { return (blk >> 2) * 4096 + (((((blk & 3) << 1) | (p >> 1)) ^ swz) << 4); };
  int dzo[NBn], xo[NBc];
#pragma unroll
  for (int i = 0; i < NBn; ++i) dzo[i] = blk_off(wn * NBn + i);
#pragma unroll
  for (int j = 0; j < NBc; ++j) xo[j] = DZ_BYTES + blk_off(wc * NBc + j);
  constexpr int NF = NBn + TAPS * NBc;  // fragments read per sub-step

  if constexpr (TAPS == 2) {
    // tap pairs: the second tap's x fragments are read while the first tap's MFMAs run (counted
    // lgkmcnt); ILVW spreads the next stage's DMA pieces through the first sub-step's MFMAs (the
    // last iteration re-stages clamped in-range rows into the idle buffer: no branch among them)
    constexpr int N0 = NBn + NBc;  // dz + tap-0 fragments
    constexpr int NMF = NBn * NBc;
    if (ks_begin < ks_end) {
      stage(ks_begin, 0);
      wait_vmcnt0();
      __syncthreads();
    }
    for (int ks = ks_begin; ks < ks_end; ++ks) {
      const int cur = (ks - ks_begin) & 1;
      if constexpr (ILVW) stage_addr(ks + 1);
      else if (ks + 1 < ks_end) stage(ks + 1, cur ^ 1);
#pragma unroll
      for (int sub = 0; sub < KSUB; ++sub) {
        const char* base = smem + cur * STAGE + sub * SUB;
        bf16x4 tl[NF], th[NF];
#pragma unroll
        for (int i = 0; i < NBn; ++i) {
          tl[i] = ds_read_tr16_asm(base + dzo[i] + roff0);
          th[i] = ds_read_tr16_asm(base + dzo[i] + roff1);
        }
#pragma unroll
        for (int tp = 0; tp < 2; ++tp)
#pragma unroll
          for (int j = 0; j < NBc; ++j) {
            tl[NBn + tp * NBc + j] = ds_read_tr16_asm(base + tp * NCC * 4096 + xo[j] + roff0);
            th[NBn + tp * NBc + j] = ds_read_tr16_asm(base + tp * NCC * 4096 + xo[j] + roff1);
          }
#pragma unroll
        for (int f = 0; f < N0; ++f) lgkm_wait_pair<2 * NBc>(tl[f], th[f]);
        bf16x8 af[NBn], bfm[2 * NBc];
#pragma unroll
        for (int i = 0; i < NBn; ++i)
          af[i] = bf16x8{tl[i][0], tl[i][1], tl[i][2], tl[i][3], th[i][0], th[i][1], th[i][2], th[i][3]};
#pragma unroll
        for (int j = 0; j < NBc; ++j)
          bfm[j] = bf16x8{tl[NBn + j][0], tl[NBn + j][1], tl[NBn + j][2], tl[NBn + j][3],
                          th[NBn + j][0], th[NBn + j][1], th[NBn + j][2], th[NBn + j][3]};
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        constexpr int MPD = ILVW ? (NMF / NPW > 0 ? NMF / NPW : 1) : NMF + 1;
#pragma unroll
        for (int f = 0; f < NMF; ++f) {
          acc[0][f / NBc][f % NBc] = mfma16x16x32(af[f / NBc], bfm[f % NBc], acc[0][f / NBc][f % NBc]);
          if (ILVW && sub == 0 && f % MPD == MPD - 1 && f / MPD < NPW) {
            __builtin_amdgcn_sched_barrier(0);
            stage_pieces(cur ^ 1, f / MPD, f / MPD + 1);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        if (ILVW && sub == 0 && NMF / MPD < NPW) stage_pieces(cur ^ 1, NMF / MPD, NPW);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < NBc; ++j) lgkm_wait_pair<0>(tl[N0 + j], th[N0 + j]);
#pragma unroll
        for (int j = 0; j < NBc; ++j)
          bfm[NBc + j] = bf16x8{tl[N0 + j][0], tl[N0 + j][1], tl[N0 + j][2], tl[N0 + j][3],
                                th[N0 + j][0], th[N0 + j][1], th[N0 + j][2], th[N0 + j][3]};
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int f = 0; f < NMF; ++f)
          acc[1][f / NBc][f % NBc] = mfma16x16x32(af[f / NBc], bfm[NBc + f % NBc], acc[1][f / NBc][f % NBc]);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        if (do_bias) {
#pragma unroll
          for (int i = 0; i < NBn; ++i) {
            float sm = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) sm += (float)af[i][e];
            dbs[i] += sm;
          }
        }
      }
      wait_vmcnt0();
      __syncthreads();
    }
    wgrad_store<WN, WC, NWC, TAPS>(a, acc, dbs, do_bias ? (1u << NBn) - 1u : 0u, split, t, n0, c0, wn, wc, lane, zero_split);
    return;
  }
  if (ks_begin < ks_end) {
    stage(ks_begin, 0);
    wait_vmcnt0();
    __syncthreads();
  }
  for (int ks = ks_begin; ks < ks_end; ++ks) {
    const int cur = (ks - ks_begin) & 1;
    if (ks + 1 < ks_end) stage(ks + 1, cur ^ 1);
#pragma unroll
    for (int sub = 0; sub < KSUB; ++sub) {
      const char* base = smem + cur * STAGE + sub * SUB;
      bf16x4 tl[NF], th[NF];
#pragma unroll
      for (int i = 0; i < NBn; ++i) {
        tl[i] = ds_read_tr16_asm(base + dzo[i] + roff0);
        th[i] = ds_read_tr16_asm(base + dzo[i] + roff1);
      }
#pragma unroll
      for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
        for (int j = 0; j < NBc; ++j) {
          tl[NBn + tp * NBc + j] = ds_read_tr16_asm(base + tp * NCC * 4096 + xo[j] + roff0);
          th[NBn + tp * NBc + j] = ds_read_tr16_asm(base + tp * NCC * 4096 + xo[j] + roff1);
        }
      lgkm_fence<NF>(tl, th);
      bf16x8 af[NBn], bfm[TAPS * NBc];
#pragma unroll
      for (int i = 0; i < NBn; ++i)
        af[i] = bf16x8{tl[i][0], tl[i][1], tl[i][2], tl[i][3], th[i][0], th[i][1], th[i][2], th[i][3]};
#pragma unroll
      for (int j = 0; j < TAPS * NBc; ++j)
        bfm[j] = bf16x8{tl[NBn + j][0], tl[NBn + j][1], tl[NBn + j][2], tl[NBn + j][3],
                        th[NBn + j][0], th[NBn + j][1], th[NBn + j][2], th[NBn + j][3]};
#pragma unroll
      for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
        for (int i = 0; i < NBn; ++i)
#pragma unroll
          for (int j = 0; j < NBc; ++j)
            acc[tp][i][j] = mfma16x16x32(af[i], bfm[tp * NBc + j], acc[tp][i][j]);
      if (do_bias) {
#pragma unroll
        for (int i = 0; i < NBn; ++i) {
          float sm = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) sm += (float)af[i][e];
          dbs[i] += sm;
        }
      }
    }
    wait_vmcnt0();
    __syncthreads();
  }
  wgrad_store<WN, WC, NWC, TAPS>(a, acc, dbs, do_bias ? (1u << NBn) - 1u : 0u, split, t, n0, c0, wn, wc, lane, zero_split);
}

// ----------------------------------------------------------------- wgrad: tile descriptions
// A wgrad workgroup tile is one type; conv_wgrad_kernel<Cfg>, the launchers and wgrad_plan (through
// wgrad_choose, conv.hip) read the same one.
struct WgradDefaults {
  static constexpr int KSUB = 1;          // 32-pixel sub-steps per pipeline stage
  static constexpr int NWN = 2, NWC = 4;  // waves along n and along c
  static constexpr int TAPS = 1;          // taps per workgroup (tap-merged kernel rows: K)
  static constexpr int SLOTS = 2;         // LDS stage buffers; more: a ring (wgrad_tile NS)
  // minimum waves per SIMD the register allocation must allow (0: the default -- 4 for the line-staged lab
  // kernel, else 1)
  static constexpr int MIN_WAVES = 0;
  static constexpr bool PAIR = false, LINE = false, LINE_DMA_SPREAD = false, UNIT_PIPE = false;  // see wgrad_tile*
  // Resident workgroups per CU the trainers size the split count for.  Stated, not derived: two 8-wave
  // workgroups of <= 128 VGPRs and 48 KB of LDS share a CU.
  static constexpr int PER_CU = 2;
};
// one tap per workgroup: WN x WC on 8 waves (2 n x 4 c)
template <int WN_, int WC_>
struct WgradTap : WgradDefaults { static constexpr int WN = WN_, WC = WC_; };
// 160 x 160 on 4 waves (2 n x 2 c, 80 x 80 per wave): the value net's padded width; 40 KB of LDS
struct WgradTap160x160 : WgradTap<160, 160> { static constexpr int NWC = 2; };
// tap-merged kernel row (64-wide c tile): the K taps of a row per workgroup
template <int WN_, int TAPS_>
struct WgradRow : WgradTap<WN_, 64> {
  static constexpr int TAPS = TAPS_;
  // the 5x5 rows of the 160-wide n tile (value layer 0, 49 planes) take 154 VGPRs, which leaves room for one
  // 8-wave workgroup -- a grid sized for two ran as two rounds (251 us per step, profiles/r3_fp8_wgrad.md)
  static constexpr int PER_CU = (WN_ == 160 && TAPS_ == 5) ? 1 : 2;
};
// the thin first layer (48 real planes of 64): a 48-wide c tile on 6 waves (2 n x 3 c) skips the zero
// channels -- 25% fewer MFMAs and x bytes on the backward's serial tail.  The 5x5 rows of a 192-wide layer
// run as 96-wide halves (WN 96): half the accumulators per wave (104 VGPRs instead of 180), so two
// workgroups share a CU and one resident round covers the grid (profiles/r5/README.md); the 192-wide
// rows stay compiled beside them.
template <int WN_, int TAPS_>
struct WgradRow48 : WgradTap<WN_, 48> { static constexpr int TAPS = TAPS_, NWC = 3; };
// split-free small-batch plan (launch_conv_wgrad_direct): 32 x WC per tap over all pixels, one per CU
template <int WC_, int KSUB_>
struct WgradDirect : WgradTap<32, WC_> {
  static constexpr int KSUB = KSUB_, NWC = WC_ / 16, PER_CU = 1;
};
#ifdef AGK_KERNEL_LAB
// kernel-lab re-cuts (equal or slower, profiles/r3_wgrad_pair.md, profiles/r4/README.md)
template <int WN_, int WC_, int NWC_>
struct WgradRing : WgradTap<WN_, WC_> {  // variant 9: 4-slot LDS ring, one workgroup per CU
  static constexpr int NWC = NWC_, SLOTS = 4, PER_CU = 1;
};
template <int WN_, int WC_>
struct WgradTap4Waves : WgradTap<WN_, WC_> {  // variant 2: 256-thread tile
  static constexpr int NWC = 2;
};
// The thin first layer's rows run one workgroup per CU (180 VGPRs on 6 waves): ~1.16 us per 32-pixel stage,
// 26-29 % MFMA busy (profiles/r3_final/pmc).  Variant 13 caps them at 168 VGPRs (11 dwords spilled) so that
// two share a CU; 10: 12 waves (4 n x 3 c, 48 x 48 per wave per tap, 104 VGPRs): 559 us vs 556 us; 11: the 6
// waves with unit pipelining (wgrad_tile UP): 557 us; 12: 12 waves with unit pipelining: 556 us.  Measured and
// removed: the 6 waves on a 4-slot LDS ring (601 us), 12 waves + UP capped at 85 VGPRs for two workgroups
// per CU (56 B spilled, bench -4.5 %), UP on the 3x3 per-tap kernel (517 vs 500 us).
template <int WN_, int TAPS_>
struct WgradRow48TwoPerCu : WgradRow48<WN_, TAPS_> {
  static constexpr int MIN_WAVES = 3;
};
template <int WN_, int TAPS_, bool UP_>
struct WgradRow48Waves12 : WgradRow48<WN_, TAPS_> {
  static constexpr int NWN = 4;
  static constexpr bool UNIT_PIPE = UP_;
};
template <int WN_, int TAPS_>
struct WgradRow48UnitPipe : WgradRow48<WN_, TAPS_> {
  static constexpr bool UNIT_PIPE = true;
};
// variants 6 / 8: tap pairs, 64-pixel stages, line staging (8: DMA spread); 7: per tap, line staging
template <bool SPREAD_>
struct WgradPair : WgradTap<192, 192> {
  static constexpr int KSUB = 2, TAPS = 2, PER_CU = 1;
  static constexpr bool PAIR = true, LINE = true, LINE_DMA_SPREAD = SPREAD_;
};
struct WgradLine : WgradTap<192, 192> { static constexpr bool LINE = true; };
#endif

// launch geometry of a wgrad tile, and what it may combine
template <class C>
struct WgradGeo {
  static constexpr int THREADS = 64 * C::NWN * C::NWC;
  static constexpr int LDS_BYTES = C::SLOTS * (C::WN + C::WC * C::TAPS) * 64 * C::KSUB;
  static constexpr int MIN_WAVES = C::MIN_WAVES > 0 ? C::MIN_WAVES : (C::LINE && !C::PAIR) ? 4 : 1;
  static_assert(!C::PAIR || C::TAPS == 2, "PAIR: two taps per workgroup");
  static_assert(C::NWN == 2 || (!C::PAIR && !C::LINE), "NWN != 2: the plain per-tap / tap-merged body only");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

template <class C>
__global__ __launch_bounds__((WgradGeo<C>::THREADS), (WgradGeo<C>::MIN_WAVES)) void conv_wgrad_kernel(ConvWgradArgs a) {
  constexpr int WN = C::WN, WC = C::WC, KSUB = C::KSUB, NWC = C::NWC, TAPS = C::TAPS, NS = C::SLOTS, NWN = C::NWN;
  constexpr bool PAIR = C::PAIR, LINE = C::LINE, ILVW = C::LINE_DMA_SPREAD, UP = C::UNIT_PIPE;
  // workgroup -> (split, tap group, channel block).  xcd_group (tap-merged rows): the hardware
  // deals workgroups to the 8 XCDs round robin in launch order, which puts the K kernel-row
  // workgroups of a split -- all reading the same dZ rows -- on K different L2s, so every dZ
  // byte comes from the Infinity Cache K times (layer 0: 3 % L2 hits, profiles/r3_small_batch.md).
  // Grouped, each XCD runs a contiguous range of split-major work and a split's rows share an L2.
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (TAPS > 1 && !PAIR && a.xcd_group) {
    const int gyz = gridDim.y * gridDim.z;
    const int nwg = gridDim.x * gyz;
    const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const int xcd = lin & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int l = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (lin >> 3);
    bx = l / gyz;
    const int rem = l - bx * gyz;
    by = rem / gridDim.z;
    bz = rem - by * gridDim.z;
  }
  const int split = bx;
  const int ncb = a.Cin / WC;
  const int n0 = (bz / ncb) * WN;
  const int c0 = (bz % ncb) * WC;
  // a.ksteps_per_split is in units of one stage (KSUB*32 pixels)
  const int nks_total = (a.M + 32 * KSUB - 1) / (32 * KSUB);
  const int t = by * TAPS;  // first tap of the group
  if constexpr (PAIR) {
    if (t + 1 >= a.T) {  // the odd last tap: one tap over the pixels of splits 2 bx and 2 bx + 1
      const int s0 = 2 * split;
      if (s0 >= a.nsplit) return;  // workgroup-uniform: no barrier reached yet
      const int kb = s0 * a.ksteps_per_split;
      int ke = kb + 2 * a.ksteps_per_split;
      if (ke > nks_total) ke = nks_total;
      if constexpr (LINE) wgrad_tile_line<WN, WC, KSUB, NWC, 1>(a, s0, kb, ke, t, 0, n0, c0, s0 + 1 < a.nsplit ? s0 + 1 : -1);
      else wgrad_tile<WN, WC, KSUB, NWC, 1, 2, 2, false, false>(a, s0, kb, ke, t, 0, n0, c0, s0 + 1 < a.nsplit ? s0 + 1 : -1);
      return;
    }
  }
  const int ks_begin = split * a.ksteps_per_split;
  int ks_end = ks_begin + a.ksteps_per_split;
  if (ks_end > nks_total) ks_end = nks_total;
  int tstep = a.Cin;  // kernel rows: tap t+1 is one column right
  if constexpr (PAIR) {
    const int t1 = t + 1;
    tstep = ((t1 / a.K - t / a.K) * a.HPi + (t1 % a.K - t % a.K)) * a.Cin;
  }
  if constexpr (LINE) wgrad_tile_line<WN, WC, KSUB, NWC, TAPS, ILVW>(a, split, ks_begin, ks_end, t, tstep, n0, c0, -1);
  else wgrad_tile<WN, WC, KSUB, NWC, TAPS, NS, NWN, UP, !PAIR>(a, split, ks_begin, ks_end, t, tstep, n0, c0, -1);
}

// one launch of conv_wgrad_kernel: threads and LDS are the tile's; the grid (splits x tap groups x channel
// blocks) is the caller's
template <class C>
static void launch_wgrad_cfg(const ConvWgradArgs& a, dim3 grid, hipStream_t st) {
  launch_dyn_lds<conv_wgrad_kernel<C>, WgradGeo<C>::THREADS, WgradGeo<C>::LDS_BYTES>(grid, st, a);
}

constexpr int kWgradKsub = WgradDefaults::KSUB;
// ConvWgradArgs::variant: 0 = production 2-buffer kernel (tap-merged rows for
// 64-wide c tiles); kernel-lab build only: 1 = one tap per workgroup,
// 2 = 256-thread tile, 3 / 4 = LDS ring with that many slots

#ifdef AGK_KERNEL_LAB
// kernel-lab tile codes and wgrad variants (conv_lab.hip); true when the code was a lab code
bool launch_conv_fwd_lab(int bm, const ConvFwdArgs& a, int bn, int mode, hipStream_t st);
bool launch_conv_wgrad_lab(const ConvWgradArgs& a, int wn, int wc, dim3 grid, hipStream_t st);
bool launch_conv_wgrad_line_lab(const ConvWgradArgs& a, hipStream_t st);  // wgrad variants 6-8
#endif

}  // namespace agk
