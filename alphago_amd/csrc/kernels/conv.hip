// Implicit-GEMM convolution for 19x19 boards on CDNA4 MFMA (gfx950).
//
// Activation layout: zero-bordered ("padded") NHWC bf16.  Element (b, i, j, c)
// of a tensor with padded side HP lives at ((b*HP + i)*HP + j)*C + c, the
// board interior is i, j in [P, P+S).  Borders are zero and never written, so
// every tap of a 'same' convolution is a plain load — no boundary branches.
//
// conv_fwd_kernel   D[n][m] = sum_{t,c} W_t[n][c] * X[m + shift_t][c]
//   M = boards*S*S output pixels, N = Cout, K = taps*Cin.  Workgroup tile
//   128(m) x BN(n), K-step = one tap x 64 channels.  Both operands are staged
//   global->LDS with global_load_lds_dwordx4 (the A rows are a per-lane gather:
//   row address of pixel m + tap offset); the 16-B chunks of each 128-B LDS row
//   are XOR-swizzled on the *source* address so the 16x16x32 bf16 MFMA fragment
//   reads (ds_read_b128) are bank-conflict free.  Double-buffered LDS.
//   The MFMA is issued "swapped" (A = weights, B = pixels) so each lane owns 4
//   consecutive output channels of one pixel: the epilogue (bias + ReLU, or the
//   ReLU-derivative mask for dgrad) stores 8 bytes per lane.
//   The same kernel computes dgrad with flipped/transposed packed weights.
//   A tile code names one tile description (conv_kernels.h: Tile36 ... Tile388; pixels per workgroup,
//   wave tile, K loop, K order, LDS slots); FwdTiles below lists the codes of each output width,
//   fwd_resolve_tile holds the automatic rule, conv_fwd_tile_info reports the tile that runs.
//
// conv_wgrad_kernel dW_t[n][c] = sum_m dZ[m][n] * X[m + shift_t][c]
//   K = pixels (split over workgroups), tile 192(n) x 192(c) per workgroup for
//   one tap.  Tiles are staged as [16-channel block][32 pixels][16 ch] and the
//   pixel-contiguous MFMA operands are read with the gfx950 hardware transpose
//   read ds_read_b64_tr_b16.  The k (pixel) order inside a K-step is permuted
//   identically for both operands so that each 32-lane half reads 8 distinct
//   contiguous rows (conflict free).  Partial sums go to a per-split fp32 slab
//   that conv_wgrad_reduce_kernel sums deterministically into the OIHW fp32
//   gradient (and the bias gradient).  Staging addresses are stepped: a lane splits its
//   first pixel into (board, row, column) once and then advances 32 pixels per stage by
//   compares and adds of host-precomputed byte deltas (ConvWgradArgs::st_*), after the
//   stage's MFMAs are issued; the DMA takes a scalar base and a 32-bit lane offset, the
//   fragment reads immediate offsets.  The bias pixel sums are dealt out over the taps'
//   workgroups: one 16-channel block per (tap, wave column) of the c0 == 0 column.
//   A wgrad tile is one description too (WgradTap, WgradRow, WgradRow48, ...); the launcher run without
//   launching (wgrad_choose) is what wgrad_plan tells the trainers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <numeric>

#include "conv_kernels.h"

namespace agk {


// ----------------------------------------------------------------- forward launchers

// The dispatch table: the tile codes an output width takes (conv_kernels.h has the types, docs/ARCHITECTURE.md
// the table in words).  160-wide (the value net: 152 filters padded to 160, straddled K-steps when
// Cin % 64 == 32) has no 37 and no compact-halo tile (388 runs 386 there, fwd_resolve_tile); 65 / 130 exist in
// the kernel lab only.
// ORDER: dispatch does not depend on it, but the code object does.  The compiler emits the kernels in the order
// with_tile's left fold names them, and scripts/isa_compare.py pairs the kernels of two builds by position.
// Reordering a list (or turning the fold around) changes no kernel and still fails that comparison against an
// older build, so both lists keep the order of the if-chains they replaced.
template <class... T>
struct TileList {};
#ifdef AGK_KERNEL_LAB
#define AGK_LAB_RING_TILES Tile65, Tile130,
#else
#define AGK_LAB_RING_TILES
#endif
template <int BN>
struct FwdTiles {
  using type = TileList<Tile384, Tile256, Tile128, Tile64, Tile36, Tile38, Tile37, AGK_LAB_RING_TILES Tile385, Tile386,
                        Tile387, Tile388>;
};
template <>
struct FwdTiles<160> {
  using type = TileList<Tile384, Tile385, Tile386, Tile387, Tile256, Tile128, Tile64, AGK_LAB_RING_TILES Tile38, Tile36>;
};
#undef AGK_LAB_RING_TILES

// f(Tile{}) for the list's tile with this code; false when the list has none
template <class F, class... T>
static bool with_tile(TileList<T...>, int code, F&& f) {
  return (... || (code == T::CODE ? (f(T{}), true) : false));
}

// f(IntC<BN>{}) for the output-width tile of a layer: 160 (the value net), else the largest of 192 / 128 / 64
// that divides Cout
template <class F>
static auto with_n_tile(int Cout, F&& f) {
  if (Cout == 160) return f(IntC<160>{});
  if (Cout % 192 == 0) return f(IntC<192>{});
  if (Cout % 128 == 0) return f(IntC<128>{});
  return f(IntC<64>{});
}

// The automatic rule (tile 0) and the one substitution of an explicit code.  Every threshold is a measured
// crossover; the measurements are in profiles/: r2_dma_spread.md (385), r3_chunk_outer.md (386),
// r3_small_batch.md (64 below 128 x 256 pixels), r4/README.md and r4/raw/tiles_160_graph.txt (36, and where
// the 160-wide layers take it), r8/README.md (388 where 386 was).
int fwd_resolve_tile(const FwdShape& g, int mode, int tile) {
  const int bn = with_n_tile(g.Cout, [](auto bnc) { return decltype(bnc)::value; });
  const bool halo = halo384_covers(bn, mode, g.S, g.K, g.Cin, g.Cout, g.offi);
  if (tile == 388) return halo ? 388 : 386;  // shapes the compact-halo kernel does not cover run 386
  if (tile != 0) return tile;
  if (g.M < (bn == 160 ? 8192 : 64 * 256)) return 36;
  if (g.M >= 384 * 512) return halo ? 388 : 386;
  return g.M >= 256 * 512 ? 256 : g.M >= 128 * 256 ? 128 : 64;
}

[[noreturn]] static void fwd_unknown_tile(int bn, int code) {
  if (bn == 160)
    throw std::invalid_argument("conv_fwd: 160-wide tiles support tile codes 36 / 38 / 64 / 128 / 256 / 384-387");
  throw std::invalid_argument("conv_fwd: unknown tile code " + std::to_string(code));
}

template <int BN, int MODE, bool STR>
static void launch_fwd_code(const ConvFwdArgs& a, int code, hipStream_t st) {
  if (with_tile(typename FwdTiles<BN>::type{}, code,
                [&](auto tile) { launch_fwd_tile<BN, MODE, decltype(tile), STR>(a, st); }))
    return;
#ifdef AGK_KERNEL_LAB
  // kernel-lab tile codes (conv_lab.hip, profiles/r1_fwd_kernel_experiments.md)
  if (BN != 160 && launch_conv_fwd_lab(code, a, BN, MODE, st)) return;
#endif
  fwd_unknown_tile(BN, code);
}

template <int BN, int MODE>
static void launch_fwd_t(const ConvFwdArgs& a, hipStream_t st) {
  const int code = fwd_resolve_tile({a.M, a.S, a.K, a.Cin, a.Cout, a.offi}, MODE, a.tile);
  if constexpr (BN == 160) {
    if (a.Cin % 64 == 32) launch_fwd_code<160, MODE, true>(a, code, st);
    else launch_fwd_code<160, MODE, false>(a, code, st);
  } else {
    if (a.Cin % 64 != 0) throw std::invalid_argument("conv_fwd: Cin % 64 == 32 needs the 160-wide tile");
    launch_fwd_code<BN, MODE, false>(a, code, st);
  }
}

// {resolved code, BM, waves, threads, LDS bytes, loop kind (FwdLoop), chunk-outer, LDS slots} of the tile
// launch_conv_fwd would run -- read from the type the launcher instantiates.  The codes of this file only: the
// kernel lab's own codes (conv_lab.hip: 7 - 10, 2560, 2568 and the variant kernels) raise here though they launch
void conv_fwd_tile_info(const FwdShape& g, int mode, int tile, int out[8]) {
  const int code = fwd_resolve_tile(g, mode, tile);
  with_n_tile(g.Cout, [&](auto bnc) {
    constexpr int BN = decltype(bnc)::value;
    const bool known = with_tile(typename FwdTiles<BN>::type{}, code, [&](auto tile) {
      using T = decltype(tile);
      using G = FwdGeo<T, BN>;
      const int v[8] = {T::CODE, T::BM, G::WAVES, G::THREADS, G::LDS_BYTES, (int)T::LOOP, T::CHUNK_OUTER, T::SLOTS};
      std::copy(v, v + 8, out);
    });
    if (!known) fwd_unknown_tile(BN, code);
  });
}

template <int MODE>
static void launch_fwd_mode(const ConvFwdArgs& a, hipStream_t st) {
  with_n_tile(a.Cout, [&](auto bnc) { launch_fwd_t<decltype(bnc)::value, MODE>(a, st); });
}

void launch_conv_fwd(const ConvFwdArgs& a_in, int mode, hipStream_t st) {
  ConvFwdArgs a = a_in;
  a.divSS = make_fastdiv((uint32_t)(a.S * a.S));
  a.divS = make_fastdiv((uint32_t)a.S);
  if (a.res) {
    // residual block: the skip operand selects the MODE_RES instantiations of the same kernels (a
    // compile-time flag -- the kernels without it are untouched)
    if (mode != MODE_BIAS_RELU && mode != MODE_MASKBITS)
      throw std::invalid_argument("conv_fwd: a skip operand (res) goes with modes 0 (bias + ReLU) and 3 (bitmask dgrad)");
    if (a.y_bf8) throw std::invalid_argument("conv_fwd: a skip operand (res) cannot be combined with the e5m2 copy");
#ifdef AGK_KERNEL_LAB
    throw std::invalid_argument("conv_fwd: the kernel-lab library has no skip operand (res)");
#else
    if (a.tile == 40) launch_conv_ws(a, mode | MODE_RES, 0, st);
    else if (mode == MODE_BIAS_RELU) launch_fwd_mode<MODE_BIAS_RELU | MODE_RES>(a, st);
    else launch_fwd_mode<MODE_MASKBITS | MODE_RES>(a, st);
    return;
#endif
  }
  if (a.tile == 40) {  // weight-stationary small-batch kernel (conv_ws.hip)
    launch_conv_ws(a, mode, 0, st);
    return;
  }
#ifdef AGK_KERNEL_LAB
  if (a.tile > 1000 && a.tile < 1064) {  // its probes (which part sets the layer's time)
    launch_conv_ws(a, mode, 0, st, a.tile - 1000);
    return;
  }
#endif
  if (mode == MODE_BIAS_RELU) launch_fwd_mode<MODE_BIAS_RELU>(a, st);
  else if (mode == MODE_MASK) launch_fwd_mode<MODE_MASK>(a, st);
  else if (mode == MODE_MASKBITS) launch_fwd_mode<MODE_MASKBITS>(a, st);
  else launch_fwd_mode<MODE_NONE>(a, st);
}

#ifdef AGK_KERNEL_LAB
// packed-tap first layer (conv_fwd_pk_kernel): 384-pixel tile, 96 x 96 (or 96 x 80) per wave; equal to the
// 64-channel kernel in the step (399.5 vs 398.1 us, round 4), kernel lab only
template <int BN>
static void launch_fwd_pk_t(const ConvFwdArgs& a, int cpt, hipStream_t st) {
  constexpr int BM = 384, MBW = 6;
  const dim3 grid((a.M + BM - 1) / BM, a.Cout / BN);
  launch_dyn_lds<conv_fwd_pk_kernel<BN, BM, MBW>, BM / MBW * 8, 2 * (BM * 128 + BN * 128)>(grid, st, a, cpt);
}

void launch_conv_fwd_pk(const ConvFwdArgs& a_in, int cpt, hipStream_t st) {
  ConvFwdArgs a = a_in;
  a.divSS = make_fastdiv((uint32_t)(a.S * a.S));
  a.divS = make_fastdiv((uint32_t)a.S);
  if (cpt < 4 || cpt > 8 || a.Cin != 64) throw std::invalid_argument("conv_fwd_pk: 32 < cin_real <= 64 in a 64-channel input");
  with_n_tile(a.Cout, [&](auto bnc) { launch_fwd_pk_t<decltype(bnc)::value>(a, cpt, st); });
}
#endif  // AGK_KERNEL_LAB

// ----------------------------------------------------------------- wgrad: choice and launchers
// launch_conv_wgrad and wgrad_choose are ONE walk over the launchers below.  A launch runs the kernel of the
// tile it arrives at; a choice (WgradRun::plan) records that tile's constants and its grid instead, so what
// wgrad_plan tells the trainers is what the launch does.
struct WgradRun {
  const ConvWgradArgs& a;
  hipStream_t st;
  WgradChoice* plan;  // non-null: record the choice, launch nothing
};

template <class C>
static void wgrad_run(const WgradRun& r, dim3 grid) {
  if (r.plan) *r.plan = {C::TAPS, (int)(grid.y * grid.z), C::PER_CU, WgradGeo<C>::THREADS, C::WN, C::WC, WgradGeo<C>::LDS_BYTES};
  else launch_wgrad_cfg<C>(r.a, grid, r.st);
}

// kernel rows: grid = splits x rows x channel blocks (the 48-wide c tile covers the layer's real planes)
template <class C>
static void wgrad_run_rows(const WgradRun& r) {
  const ConvWgradArgs& a = r.a;
  wgrad_run<C>(r, dim3(a.nsplit, a.T / C::TAPS, (a.Cout / C::WN) * (C::WC == 48 ? 1 : a.Cin / C::WC)));
}

template <int WN, int TAPS>
static void launch_wgrad_rows(const WgradRun& r) {
  if (r.a.cin_real <= 48) {  // thin first layer (48 real planes padded to 64): the slab columns 48..63 stay
                             // unwritten (the reduce reads only cin_real of them)
#ifdef AGK_KERNEL_LAB  // round-4 re-cuts of this kernel (equal or slower): variants 10-12, 13 = two per CU
    if (TAPS == 5 && r.a.variant == 13) return wgrad_run_rows<WgradRow48TwoPerCu<WN, TAPS>>(r);
    if constexpr (TAPS == 5 && (WN / 16) % 4 == 0) {
      if (r.a.variant == 10) return wgrad_run_rows<WgradRow48Waves12<WN, TAPS, false>>(r);
      if (r.a.variant == 12) return wgrad_run_rows<WgradRow48Waves12<WN, TAPS, true>>(r);
    }
    if constexpr (TAPS == 5) {
      if (r.a.variant == 11) return wgrad_run_rows<WgradRow48UnitPipe<WN, TAPS>>(r);
    }
#endif
    if constexpr (TAPS == 5 && WN == 192) return wgrad_run_rows<WgradRow48<96, TAPS>>(r);  // as 96-wide halves
    return wgrad_run_rows<WgradRow48<WN, TAPS>>(r);
  }
  wgrad_run_rows<WgradRow<WN, TAPS>>(r);
}

#ifdef AGK_KERNEL_LAB
// variant 9 (small batches): the per-tap kernel on a 4-slot LDS ring, one workgroup per CU, for the
// tile geometries whose waves stage equal piece counts (192 x 192, 128 x 128, 160 x 160); the SL step at
// B = 16 measured 0.901 ms with it against 0.863 ms without (round 4): kernel lab only
template <int WN, int WC, int NWC>
static bool launch_wgrad_ring(const WgradRun& r, dim3 grid) {
  constexpr int NWAVES = 2 * NWC;
  constexpr int NINSTR = WN / 16 + WC / 16;
  constexpr int IPW = (NINSTR + NWAVES - 1) / NWAVES;
  if constexpr ((WN / 16) % IPW == 0 && NINSTR == NWAVES * IPW) {
    wgrad_run<WgradRing<WN, WC, NWC>>(r, grid);
    return true;
  }
  return false;
}
#endif  // AGK_KERNEL_LAB

template <int WN, int WC>
static void launch_wgrad_t(const WgradRun& r) {
  const ConvWgradArgs& a = r.a;
  dim3 grid(a.nsplit, a.T, (a.Cout / WN) * (a.Cin / WC));
#ifdef AGK_KERNEL_LAB
  if (WC != 64 && a.variant == 9 && launch_wgrad_ring<WN, WC, 4>(r, grid)) return;
  // lab variants 2 / 3 / 4 (conv_lab.hip)
  if (a.variant != 9 && !r.plan && launch_conv_wgrad_lab(a, WN, WC, grid, r.st)) return;
#else
  if (a.variant != 0 && !r.plan)
    throw std::invalid_argument("conv_wgrad: variant " + std::to_string(a.variant) + " is a kernel-lab variant");
#endif
  if constexpr (WC == 64) {
    // tap-merged kernel rows (see conv_wgrad_kernel); lab variant 1 forces one tap per workgroup
    if (a.variant != 1 && (a.K == 3 || a.K == 5)) {
      if (a.K == 3) launch_wgrad_rows<WN, 3>(r);
      else launch_wgrad_rows<WN, 5>(r);
      return;
    }
  }
  wgrad_run<WgradTap<WN, WC>>(r, grid);
}

static void launch_wgrad_160x160(const WgradRun& r) {
  const ConvWgradArgs& a = r.a;
#ifdef AGK_KERNEL_LAB
  if (a.variant == 9 && launch_wgrad_ring<160, 160, 2>(r, dim3(a.nsplit, a.T, 1))) return;
#endif
  if (a.variant != 0 && !r.plan) throw std::invalid_argument("conv_wgrad: 160-wide tiles have no production variants");
  wgrad_run<WgradTap160x160>(r, dim3(a.nsplit, a.T, 1));
}

int wgrad_stage_pixels() { return 32 * kWgradKsub; }

// Split-free small-batch wgrad (kWgradDirect).  At B <= 16 the split-K plan spends ~10 us per layer on
// its reduce launch beside a ~15 us wgrad (profiles/r5/README.md, B = 16 trace), and its one-round grid
// gives each split only a few hundred pixels.  Here every workgroup owns one 32 (n) x WC (c) tile of
// one tap over ALL B*S*S pixels: 6 x 4 x 9 = 216 workgroups for a 192 -> 192 3x3 layer (150 for the
// 5x5 first layer's 48 real input planes), at most one per CU.  Each streams (32 + WC) channels x M
// pixels through an LDS double buffer of KS 32-pixel sub-steps (one barrier per 32 KS pixels) and
// writes its fp32 sums straight into the OIHW gradient (wgrad_store, grad_w != nullptr): deterministic
// (one workgroup per output element, fixed pixel order), no slab and no reduce launch.
template <int WC>
static void launch_wgrad_direct_t(const ConvWgradArgs& a, int ksub, hipStream_t st) {
  const dim3 grid(1, a.T, (a.Cout / 32) * (a.Cin / WC));
  if (ksub == 1) launch_wgrad_cfg<WgradDirect<WC, 1>>(a, grid, st);
  else if (ksub == 2) launch_wgrad_cfg<WgradDirect<WC, 2>>(a, grid, st);
  else if (ksub == 8) launch_wgrad_cfg<WgradDirect<WC, 8>>(a, grid, st);
  else launch_wgrad_cfg<WgradDirect<WC, 4>>(a, grid, st);
}

// c tile of the split-free plan: 48 (192-multiple widths; the first layer's 48 real planes of 64), else 32
int wgrad_direct_wc(int Cin, int cin_real) {
  if (Cin == 64 && cin_real <= 48) return 48;
  if (Cin % 48 == 0 && cin_real == Cin) return 48;
  if (Cin % 32 == 0) return 32;
  return 0;
}

bool wgrad_direct_supported(int Cout, int Cin, int cin_real, int K) {
  return Cout % 32 == 0 && wgrad_direct_wc(Cin, cin_real) > 0 && (K == 1 || K == 3 || K == 5);
}

void launch_conv_wgrad_direct(const ConvWgradArgs& a_in, int ksub, hipStream_t st) {
  ConvWgradArgs a = a_in;
  a.divSS = make_fastdiv((uint32_t)(a.S * a.S));
  a.divS = make_fastdiv((uint32_t)a.S);
  a.xcd_group = 0;
  a.nsplit = 1;
  wgrad_fill_steps(a);
  if (!a.grad_w || !wgrad_direct_supported(a.Cout, a.Cin, a.cin_real, a.K))
    throw std::invalid_argument("conv_wgrad_direct: needs grad_w, Cout % 32 == 0 and a 48 / 32 c tile");
  if (wgrad_direct_wc(a.Cin, a.cin_real) == 48) launch_wgrad_direct_t<48>(a, ksub, st);
  else launch_wgrad_direct_t<32>(a, ksub, st);
}

#ifdef AGK_DEBUG
unsigned debug_error_fetch_and_clear(hipStream_t st) {
  hip_check(hipStreamSynchronize(st), "debug: stream synchronize");
  unsigned code = 0, zero = 0;
  hip_check(hipMemcpyFromSymbol(&code, HIP_SYMBOL(g_dbg_err), sizeof(code)), "debug: read error word");
  if (code) hip_check(hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_err), &zero, sizeof(zero)), "debug: clear error word");
  return code;
}
#endif

// the tile for a layer's widths (and, inside launch_wgrad_t, its kernel size and real planes)
static void wgrad_dispatch(const WgradRun& r) {
  const ConvWgradArgs& a = r.a;
  if (a.variant == kWgradSmall) {
    // small batches (ops.wgrad_config): 64 x 64 output tiles with the kernel row's taps merged -- three
    // times the workgroups per pixel split of a 192 -> 192 layer
    if (!r.plan && (a.Cout % 64 || a.Cin % 64 || a.cin_real != a.Cin || (a.K != 3 && a.K != 5)))
      throw std::invalid_argument("conv_wgrad: the small-batch tiles need 64-multiple widths and a 3x3 / 5x5 kernel");
    ConvWgradArgs s = a;
    s.variant = 0;
    s.cin_real = s.Cin;
    launch_wgrad_t<64, 64>({s, r.st, r.plan});
    return;
  }
  const bool n192 = a.Cout % 192 == 0, c192 = a.Cin % 192 == 0;
  const bool n128 = a.Cout % 128 == 0, c128 = a.Cin % 128 == 0;
  if (a.Cout == 160) {  // value net (152 filters padded to 160)
    if (a.Cin == 160) launch_wgrad_160x160(r);
    else if (a.Cin % 64 == 0 && a.Cin % 128 != 0 && a.Cin % 192 != 0) launch_wgrad_t<160, 64>(r);
    else throw std::invalid_argument("conv_wgrad: Cout 160 supports Cin 160 or an odd multiple of 64");
  } else if (a.Cin == 160) {
    throw std::invalid_argument("conv_wgrad: Cin 160 needs Cout 160");
  } else if (n192 && c192) launch_wgrad_t<192, 192>(r);
  else if (n192 && c128) launch_wgrad_t<192, 128>(r);
  else if (n192) launch_wgrad_t<192, 64>(r);
  else if (n128 && c128) launch_wgrad_t<128, 128>(r);
  else if (n128 && c192) launch_wgrad_t<128, 192>(r);
  else if (n128) launch_wgrad_t<128, 64>(r);
  else if (c192) launch_wgrad_t<64, 192>(r);
  else if (c128) launch_wgrad_t<64, 128>(r);
  else launch_wgrad_t<64, 64>(r);
}

// tap-pair / line-staged wgrads (variants 6-8): kernel lab (conv_lab.hip, profiles/r3_wgrad_pair.md)
static bool wgrad_pair_applies(int Cout, int Cin, int cin_real, int K) {
  return K == 3 && Cout == 192 && Cin == 192 && cin_real == Cin;
}

WgradChoice wgrad_choose(int Cout, int Cin, int cin_real, int K, int variant) {
  // The kernel-lab variants, in this one place.  The production library answers for them as it always has
  // (its launch raises for them): 6 / 8 where they apply are the tap pairs, 4.5 workgroups per split (9 per
  // two splits) and one per CU -- reported as 9 per split pair and 2 per CU so that nsplit = CUs * per_cu /
  // wgs_per_split stays an integer division; 1-4 are one tap per workgroup; 9 with one tap per workgroup is
  // the 4-slot ring, one workgroup per CU; 5 where the kernel lab has a row geometry is one kernel row per
  // workgroup, one per CU (~170 VGPRs, 8 or 6 waves); every other one is planned as the production tile.
  if ((variant == 6 || variant == 8) && wgrad_pair_applies(Cout, Cin, cin_real, K)) return {2, 9, 2, 512, 192, 192, 147456};
#ifdef AGK_KERNEL_LAB
  if (const int code = variant == 5 ? wgrad_row_code(Cout, Cin, cin_real, K) : 0)
    return {K, wgrad_row_wgs_per_split(code, Cout, Cin, cin_real, K), 1, 256, 0, 0, 0};
#endif
  ConvWgradArgs a{};
  a.Cout = Cout, a.Cin = Cin, a.cin_real = cin_real, a.K = K, a.T = K * K, a.nsplit = 1;
  a.variant = variant == kWgradSmall ? variant : (variant >= 1 && variant <= 4) ? 1 : 0;
  WgradChoice c{};
  wgrad_dispatch({a, nullptr, &c});
  if (variant == 9 && c.taps == 1) c.per_cu = 1;
  // a thin layer that runs one tap per workgroup (no such layer in either net) has always been reported
  // with the thin rows' 6 waves, though the 8-wave per-tap kernel runs it; nothing sizes a launch from it
  if (c.taps == 1 && Cin == 64 && cin_real <= 48 && variant != kWgradSmall) c.threads = 384;
  return c;
}

int wgrad_tap_group(int Cout, int Cin, int K, int variant) {
  // (asked with a kernel-lab variant: one tap, as this has always answered)
  return (variant == 0 || variant == kWgradSmall) ? wgrad_choose(Cout, Cin, Cin, K, variant).taps : 1;
}

void wgrad_plan(int Cout, int Cin, int cin_real, int K, int variant, int out[4]) {
  const WgradChoice c = wgrad_choose(Cout, Cin, cin_real, K, variant);
  out[0] = c.taps, out[1] = c.wgs_per_split, out[2] = c.per_cu, out[3] = c.threads;
}

void launch_conv_wgrad(const ConvWgradArgs& a_in, hipStream_t st) {
  ConvWgradArgs a = a_in;
  a.divSS = make_fastdiv((uint32_t)(a.S * a.S));
  a.divS = make_fastdiv((uint32_t)a.S);
  a.xcd_group = 1;  // kernel-row workgroups of a split on one XCD (conv_wgrad_kernel)
  wgrad_fill_steps(a);  // stepped staging addresses (wgrad_tile)
#ifdef AGK_KERNEL_LAB
  if (a.variant == 5) {
    // one-kernel-row wgrad (conv_wgrad_row.hip), kernel lab: in the power-limited steady state it ran
    // 607-694 us per 192 -> 192 layer against 548-583 us for the per-tap kernel
    // (profiles/r3_wgrad_row.md); layers it does not cover run the per-tap kernel
    const int code = wgrad_row_code(a.Cout, a.Cin, a.cin_real, a.K);
    if (code) {
      wgrad_row_launch(code, a, st);
      return;
    }
    a.variant = 0;
  }
  if (a.variant >= 6 && a.variant <= 8) {  // tap pairs (8: DMA spread) / line-staged per-tap kernel
    if (wgrad_pair_applies(a.Cout, a.Cin, a.cin_real, a.K) && launch_conv_wgrad_line_lab(a, st)) return;
    a.variant = 0;
  }
#endif
  wgrad_dispatch({a, st, nullptr});
}

// Sum split partials into the fp32 OIHW gradient (real channel counts) + bias.
// Fixed summation order per element (deterministic): four partial sums over
// the splits, s_k = sum of splits sp = k (mod 4) below the last multiple of 4
// in increasing order, the leftover splits added to s_0, then
// (s0 + s1) + (s2 + s3).  Wave k of a 256-thread block computes s_k for 64
// float4 elements (4 consecutive input channels of one tap and output
// channel), up to 8 16-B loads in flight; the four partials meet in LDS.  The OIHW
// write is strided but touches the (small) gradient once.
__device__ __forceinline__ void wgrad_reduce_body(const WgradReduceArgs& a, int bid, int nblk) {
  __shared__ f32x4 part[4][64];
  const int C4 = a.Cin >> 2;
  const int total = a.T * a.Cout_real * C4;
  const size_t tile = (size_t)a.Cout * a.Cin;
  const size_t sstride = (size_t)a.T * tile;
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n4 = a.nsplit & ~3;
  if (bid == 0 && a.grad_b) {
    // bias: one sequential sum per channel (fixed order).  The FIRST block issues it before its share
    // of the slab, so its dependent load-add rounds run under the other blocks; as the last block's
    // epilogue (up to round 6) they were the launch's tail.  16 loads in flight per round.
    for (int n = threadIdx.x; n < a.Cout_real; n += blockDim.x) {
      const float* d = a.dbias_slab + n;
      float sum = 0.f;
      int sp = 0;
      for (; sp + 16 <= a.nsplit; sp += 16) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = d[(size_t)(sp + i) * a.Cout];
#pragma unroll
        for (int i = 0; i < 16; ++i) sum += v[i];
      }
      for (; sp + 8 <= a.nsplit; sp += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = d[(size_t)(sp + i) * a.Cout];
#pragma unroll
        for (int i = 0; i < 8; ++i) sum += v[i];
      }
      for (; sp < a.nsplit; ++sp) sum += d[(size_t)sp * a.Cout];
      a.grad_b[n] = (a.beta != 0.f ? a.beta * a.grad_b[n] : 0.f) + a.scale * sum;  // beta 0: no read
    }
  }
  for (int base = bid * 64; base < total; base += nblk * 64) {  // block-uniform trip count
    const int idx = base + lane;
    const int e = idx < total ? idx : total - 1;
    const int c = (e % C4) << 2;
    const int tn = e / C4;
    const int n = tn % a.Cout_real;
    const int t = tn / a.Cout_real;
    const float* s = a.slab + (size_t)t * tile + (size_t)n * a.Cin + c;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (c < a.Cin_real) {
      // up to 8 of this wave's splits loaded before they are added (round 5: 4 loads in flight left
      // the reduce latency-bound, ~4.4 TB/s); same order of additions as one split at a time
      for (int sp0 = k; sp0 < n4; sp0 += 32) {
        const int cnt = (n4 - sp0 + 3) >> 2;
        const float* p = s + (size_t)sp0 * sstride;
        f32x4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i < cnt) v[i] = *(const f32x4*)(p + (size_t)(4 * i) * sstride);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i < cnt) acc += v[i];
      }
      if (k == 0)
        for (int sp = n4; sp < a.nsplit; ++sp) acc += *(const f32x4*)(s + (size_t)sp * sstride);
    }
    part[k][lane] = acc;
    __syncthreads();
    if (k == 0 && idx < total && c < a.Cin_real) {
      const f32x4 sum = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (c + i >= a.Cin_real) break;
        float* g = a.grad_w + ((size_t)n * a.Cin_real + c + i) * a.T + t;
        *g = (a.beta != 0.f ? a.beta * *g : 0.f) + a.scale * sum[i];  // beta 0: no read of g
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(WgradReduceArgs a) {
  wgrad_reduce_body(a, blockIdx.x, gridDim.x);
}

// Every layer's split-K reduce in ONE launch (the deferred small-batch backward, ops.conv_wgrad_reduce_multi):
// block b runs job j's reduce body as block b - first[j] of nblk[j], the same fixed summation order as
// the per-layer kernel, so the gradients are bitwise equal to twelve separate launches.
__global__ __launch_bounds__(256) void conv_wgrad_reduce_multi_kernel(WgradReduceMultiArgs m) {
  int j = 0;
  while (j + 1 < m.n && (int)blockIdx.x >= m.first[j + 1]) ++j;  // block-uniform
  wgrad_reduce_body(m.job[j], (int)blockIdx.x - m.first[j], m.nblk[j]);
}

static int wgrad_reduce_blocks(const WgradReduceArgs& a) {
  const int total = a.T * a.Cout_real * (a.Cin >> 2);
  int blocks = (total + 63) / 64;
  return blocks > 8192 ? 8192 : blocks;
}

void launch_wgrad_reduce_multi(const std::vector<WgradReduceArgs>& jobs, hipStream_t st) {
  if (jobs.empty()) return;
  if ((int)jobs.size() > kMaxReduceJobs) throw std::invalid_argument("conv_wgrad_reduce_multi: too many layers");
  WgradReduceMultiArgs m{};
  m.n = (int)jobs.size();
  int blocks = 0;
  for (int j = 0; j < m.n; ++j) {
    m.job[j] = jobs[j];
    m.first[j] = blocks;
    m.nblk[j] = wgrad_reduce_blocks(jobs[j]);
    blocks += m.nblk[j];
  }
  hipLaunchKernelGGL(conv_wgrad_reduce_multi_kernel, dim3(blocks), dim3(256), 0, st, m);
}

void launch_wgrad_reduce(const WgradReduceArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(wgrad_reduce_blocks(a)), dim3(256), 0, st, a);
}

}  // namespace agk
