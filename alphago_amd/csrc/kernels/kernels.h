// Kernel argument structs and host launchers (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "common.h"

namespace agk {

enum { MODE_BIAS_RELU = 0, MODE_MASK = 1, MODE_NONE = 2, MODE_MASKBITS = 3 };
// Skip operand of a residual block (ConvFwdArgs::res): a flag on top of the two epilogues that take one.
// The launchers set it when res is non-null, so a kernel template's MODE is the epilogue (MODE & 3) plus
// this bit and the instantiations without a skip are the ones that existed before it.
//   MODE_BIAS_RELU | MODE_RES: y = relu(acc + bias + res) (the ReLU' bit from the stored bf16, as always)
//   MODE_MASKBITS  | MODE_RES: y = (acc + res) masked by mbits_in (the skip gradient joins before ReLU')
enum { MODE_RES = 4 };
constexpr int mode_base(int mode) { return mode & 3; }
constexpr bool mode_res(int mode) { return (mode & MODE_RES) != 0; }

struct ConvFwdArgs {
  const __bf16* x;     // padded NHWC input
  const __bf16* w;     // packed [T][Cout][Cin]
  const float* bias;   // [Cout]           (MODE_BIAS_RELU)
  const __bf16* mask;  // layout of y      (MODE_MASK: keep where mask > 0)
  __bf16* y;           // padded NHWC output (interior written, borders untouched)
  uint32_t* mbits_out;       // MODE_BIAS_RELU: optional ReLU'(y) bitmask, (Cout/BN)*8 words per padded pixel
  const uint32_t* mbits_in;  // MODE_MASKBITS: the bitmask written by the layer's forward
  int M, S, Cin, Cout, K;
  int HPi, offi;       // input padded side, (input pad - K/2)
  int HPo, Po;         // output padded side and pad
  FastDiv divSS, divS; // filled by the launcher
  int tile;            // 0 = automatic; 128/256/384 fixed tiles; other codes: kernel-lab build only
  unsigned long long* dbg;  // kernel lab: diagnostic segment-cycle stamps, else null
  long long x_elems, w_elems, y_elems;  // tensor extents (debug-build bounds checks)
  // MODE_MASKBITS (dgrad) only, optional: an e5m2 copy of the output (y * *bf8_scale) for the fp8
  // wgrad, and max |y| folded into 64 amax slots (the next step's delayed gradient scale)
  uint8_t* y_bf8;
  const float* bf8_scale;
  unsigned* bf8_amax;
  // split-K (tile code 38, small batches): fp32 partial sums [sk_nsplit][M][Cout], finished by
  // conv_splitk_finish_kernel (bias + ReLU + bitmask, or the bitmask of dgrad)
  float* sk_ws;
  int sk_nsplit;
  // MODE_BIAS_RELU / MODE_MASKBITS only, optional: the skip operand of a residual block, a bf16 tensor in
  // y's layout (never y itself), read at interior pixels only and added in fp32 before the ReLU / the mask
  const __bf16* res;
};

struct ConvWgradArgs {
  const __bf16* x;     // layer input (padded NHWC, Cin)
  const __bf16* dz;    // gradient at the layer's pre-activation output (padded NHWC, Cout, zero borders)
  float* slab;         // [nsplit][T][Cout][Cin]
  float* dbias_slab;   // [nsplit][Cout]
  int M, S, Cin, Cout, K, T;
  int HPi, offi, HPo, Po;
  int ksteps_per_split, nsplit;
  int cin_real;        // real input channels (<= Cin); the zero padding above it is skipped when possible
  FastDiv divSS, divS; // filled by the launcher
  int variant;         // 0 = production per-tap kernel; 5 = one-kernel-row wgrad (conv_wgrad_row.hip);
                       // 1-4 kernel-lab build only
  long long x_elems, dz_elems;  // tensor extents (debug-build bounds checks)
  int xcd_group;       // filled by the launcher: 1 = the kernel-row workgroups of a split share an XCD
  // split-free plan (kWgradDirect, nsplit 1): the tile is written straight into the OIHW fp32 gradient
  // grad_w[n][c][t] = beta * grad_w + scale * sum (n < cout_real, c < cin_real) and the bias into
  // grad_b -- no slab, no reduce launch.  grad_w == nullptr: the split slab as above.
  float* grad_w;
  float* grad_b;
  float scale, beta;
  int cout_real;
  // stepped staging addresses (filled by the launcher, wgrad_fill_steps): a lane's pixel advances by 32
  // per sub-step = whole boards + st_q rows + st_r columns (st_q, st_r < S, so at most one column wrap
  // and one row wrap per step at any board size); *_st / *_row / *_brd are the byte deltas of that step,
  // of a column wrap (next row) and of a row wrap (next board) in each padded tensor.  x_last: byte
  // offset of pixel M - 1 in x (tap (0, 0)), the source of lanes past the last pixel.
  int st_q, st_r;
  int dz_st, dz_row, dz_brd;
  int x_st, x_row, x_brd;
  unsigned x_last;
};

// The staging offsets are 32-bit byte offsets from a scalar base, so both tensors must stay below 4 GiB.
// The guard is the op wrappers' check (conv_wgrad_impl, conv_wgrad_direct: numel < 2^31, "tensor too
// large for int32 offsets"), the limit the int32 element offsets had before; nothing is checked here.
inline void wgrad_fill_steps(ConvWgradArgs& a) {
  const int S = a.S;
  const int st_b = 32 / (S * S);
  a.st_q = (32 % (S * S)) / S;
  a.st_r = 32 % S;
  a.dz_st = ((st_b * a.HPo + a.st_q) * a.HPo + a.st_r) * a.Cout * 2;
  a.dz_row = (a.HPo - S) * a.Cout * 2;
  a.dz_brd = (a.HPo - S) * a.HPo * a.Cout * 2;
  a.x_st = ((st_b * a.HPi + a.st_q) * a.HPi + a.st_r) * a.Cin * 2;
  a.x_row = (a.HPi - S) * a.Cin * 2;
  a.x_brd = (a.HPi - S) * a.HPi * a.Cin * 2;
  a.x_last = 0;
  if (a.M > 0) {
    const int m = a.M - 1, b = m / (S * S), rem = m % (S * S), ii = rem / S, jx = rem % S;
    a.x_last = (unsigned)(((b * a.HPi + ii + a.offi) * a.HPi + jx + a.offi) * a.Cin) * 2u;
  }
}

// fp8 wgrad (conv_wgrad_fp8.hip): e5m2 dZ x e4m3 X on the block-scaled MFMA, same slab as the bf16 wgrad
struct ConvWgradFp8Args {
  const uint8_t* x8;   // e4m3 layer input (padded NHWC, Cin), quantised with multiplier 2^ex
  const uint8_t* dz8;  // e5m2 output gradient (padded NHWC, Cout, zero borders), multiplier 2^eg
  float* slab;         // [nsplit][T][Cout][Cin]
  float* dbias_slab;   // [nsplit][Cout]
  const int* xscale;   // device E8M0 exponent 127 - ex
  const int* gscale;   // device E8M0 exponent 127 - eg
  const float* gmul;   // device 2^eg (the bias sums undo it)
  unsigned* amax;      // optional: max |dZ| (float bits, 64 slots) from the tap-0 workgroups' e5m2 bytes
  int M, S, Cin, Cout, K, T;
  int HPi, offi, HPo, Po;
  int ksteps_per_split, nsplit;  // in 128-pixel steps
  FastDiv divSS, divS;           // filled by the launcher
  int probe;                     // kernel-lab timing probe (0 = production)
};
int wgrad_fp8_supported(int Cout, int Cin, int K);
int wgrad_fp8_stage_pixels();
void launch_conv_wgrad_fp8(const ConvWgradFp8Args& a, hipStream_t st);

struct WgradReduceArgs {
  const float* slab;
  const float* dbias_slab;
  float* grad_w;  // OIHW fp32 [Cout_real][Cin_real][K][K]
  float* grad_b;  // [Cout_real] or null
  int T, Cout, Cin, Cout_real, Cin_real, nsplit;
  float scale, beta;  // grad = beta*grad + scale*sum
};
constexpr int kMaxReduceJobs = 16;
struct WgradReduceMultiArgs {
  WgradReduceArgs job[kMaxReduceJobs];
  int first[kMaxReduceJobs], nblk[kMaxReduceJobs];
  int n;
};

struct PolicyHeadArgs {
  const __bf16* y;     // padded NHWC (HP = S+2, P = 1, C)
  const float* w;      // [C_real]
  const float* b;      // [1]
  const int* target;   // [B] flat move index or -1 (no loss)
  const uint8_t* legal;  // [B][S*S] or null (inference renormalisation)
  const float* weight;   // [B] per-board gradient weight (REINFORCE reward) or null
  __bf16* dz;          // padded NHWC grad (training) or null
  float* loss;         // [B]
  float* correct;      // [B]
  float* dhead;        // [B][C_real + 1] per-board partials of dW_head, db_head
  float* probs;        // [B][S*S] or null
  uint8_t* dz8;        // head_backward only: dY as e5m2 (dz8 = e5m2(bf16(dY) * dz8_scale[0])) instead of
  const float* dz8_scale;  // the bf16 dz, for an fp8 trunk backward; max |bf16(dY)| into dz8_amax
  unsigned* dz8_amax;  // [kFp8AmaxSlots] float bits (the quantize_bf8 contract)
  int B, S, C, C_real;
  float grad_scale;    // d(mean loss)/d(logit) scale = 1/global_batch
  float inv_temp;
  int loss_kind;       // 0 = categorical CE (SL / REINFORCE), 1 = reference RL binary CE on the softmax
  // Regularised head (the REG kernel variants; all null / 0 launches the plain kernels):
  //   L_b = -w_b log p_t - ent_coef * H(p) + kl_coef * KL(q || p)
  const float* ref_probs;  // [B][S*S] anchor distribution q per board, or null
  float* stats;            // [B][3] per-board H(p), KL(q || p) (0 without q), max |logit|, or null
  float ent_coef, kl_coef;  // >= 0; loss_kind 0 only; neither is multiplied by weight[b]
};

// Soft-target training head (head_soft.hip): the plain training head's arguments with a target
// distribution per board in place of the move index.  A struct of its own, so that PolicyHeadArgs (the
// kernarg layout of the plain and REG kernels) stays as it is.
struct PolicyHeadSoftArgs {
  const __bf16* y;      // padded NHWC (HP = S+2, P = 1, C)
  const float* w;       // [C_real]
  const float* b;       // [1]
  const float* tdist;   // [B][T] target distribution, T = S*S or S*S + 1 (a trailing pass column is not
                        // read); negatives / NaN count as 0, the board part is renormalised, zero or infinite mass = no loss
  const int* sym;       // [B] in 0..7 or null: the symmetry pack_input applied to the board's planes
  const float* weight;  // [B] per-board gradient weight or null
  __bf16* dz;           // padded NHWC grad
  float* loss;          // [B]
  float* correct;       // [B]
  float* dhead;         // [B][C_real + 1] per-board partials of dW_head, db_head
  int B, S, C, C_real, T;
  float grad_scale;     // d(mean loss)/d(logit) scale = 1/global_batch
};

struct ValueOutArgs {
  const float* h;       // [B][D] dense-1 output
  const float* w2;      // [D]
  const float* b2;      // [1]
  const float* target;  // [B] in [-1, 1] or null (inference)
  const float* weight;  // [B] or null
  float* v;             // [B]
  float* loss;          // [B]
  float* correct;       // [B]
  float* dh;            // [B][D]
  float* dout;          // [B][D + 1] per-board partials of [dw2 | db2]
  int B, D;
  float grad_scale;
};

struct PackInputArgs {
  const uint8_t* planes;  // [B][Creal][S][S], or [npool][Creal][S][S] with rows
  const int64_t* rows;    // [B] pool row of each board or null (board b = planes[b]); rows outside
                          // [0, npool) pack an all-zero board (no out-of-bounds read)
  int64_t npool;
  const int* sym;         // [B] in 0..7 or null (identity)
  const int* target;      // [B] or null
  int* target_out;        // [B] or null
  __bf16* out;            // padded NHWC [B][S+2P][S+2P][Cp]
  uint8_t* out8;          // the same planes as e4m3 (scale 1: exact for 0/1, saturating at 448) or null
  int B, S, Creal, Cp, P;
};

constexpr int kMaxPackLayers = 24;
struct PackLayer {
  const float* w;  // OIHW fp32 [Cout_real][Cin_real][K][K]
  __bf16* wf;      // [T][Cout_p][Cin_p]; pk_cpt > 0: [ceil(T * pk_cpt / 8)][Cout_p][64] (conv_fwd_pk_kernel)
  __bf16* wd;      // [T][Cin_p][Cout_p] flipped (dgrad) or null
  int Cout_real, Cin_real, Cout_p, Cin_p, K;
  int pk_cpt;      // packed-tap first layer: 8-channel chunks per tap, else 0
};
struct PackWeightsArgs {
  PackLayer layers[kMaxPackLayers];
  int nlayers;
};

constexpr int kFzMaxFeatures = 16;
constexpr int kFzMaxChannels = 64;
struct FeaturizeArgs {
  const int8_t* board;    // [B][S*S] in {-1,0,1}
  const uint8_t* ages;    // [B][S*S] turns_since plane or 255
  const int* meta;        // [B][2] {ko or -1, player to move}
  const uint8_t* ladder;  // [B][S*S] bit0 capture, bit1 escape; or null
  uint8_t* planes;        // [B][nplanes][S][S] or null
  __bf16* nhwc;           // [B][S+2P][S+2P][Cp] or null
  uint8_t* sensible;      // [B][S*S] or null
  uint8_t* legal;         // [B][S*S] or null
  int* overflow;          // [B] or null (set to 1 when the eye DFS overflowed)
  int B, S, P, Cp, nf, nplanes, need_eye;
  int fids[kFzMaxFeatures];
  int fplanes[kFzMaxFeatures];
  uint8_t chan_feat[kFzMaxChannels];
  uint8_t chan_plane[kFzMaxChannels];
};

constexpr int kFp8AmaxSlots = 64;  // per-layer amax accumulators (spread atomics)

struct ConvFp8Args {
  const uint8_t* x;         // padded NHWC e4m3 [B][HPi][HPi][Cin], Cin % 64 == 0
  const uint8_t* w;         // e4m3 [nch][Cout][64], chunk q = tap * (Cin/64) + c, nch even (zero tail)
  const float* bias;        // [Cout]
  const int* scales;        // [2] E8M0 exponents for the MFMA: {activations, weights} (127 = 2^0)
  const float* out_scale;   // [1] multiplier applied before the e4m3 output conversion
  __bf16* y_bf16;           // optional padded NHWC bf16 output
  uint8_t* y_fp8;           // optional padded NHWC e4m3 output
  unsigned* amax;           // optional running max of the ReLU output (float bits), kFp8AmaxSlots slots
  int M, S, Cin, Cout, K;
  int HPi, offi, HPo, Po;
  int nch;                  // packed chunks (cw channels each; a K-step holds 128 / cw chunks)
  int cw;                   // chunk width: 64, or 32 for 160-channel operands packed in 32-channel chunks
  FastDiv divSS, divS;      // filled by the launcher
  FastDiv divCC, divK;      // chunks per tap, kernel width (launcher)
  int variant;              // 0 = production (pixel operand from L2, 48 px/wave); lab: 1, 3, 4 other tilings,
                            // 5 = LDS-staged operands
  // dgrad mode (production kernel only): x holds e5m2 gradients, w the transposed/flipped e4m3
  // weights; the epilogue masks by mask > 0 (the forward's bf16 activation), takes no bias,
  // tracks max |dx| and writes bf16 and/or e5m2 (out_scale) outputs
  int dgrad;
  const __bf16* mask;
  // forward, production kernel: optional ReLU'(y) bitmask in conv_fwd_kernel's layout
  // (ConvEpilogue: (Cout/BN)*8 words per padded pixel) so the bf16 dgrad can run MODE_MASKBITS
  uint32_t* mbits_out;
  // dgrad with a bf16 gradient operand (dgrad_bf16): x is the bf16 dZ (padded NHWC, Cin channels),
  // converted to e5m2 in registers as it is loaded (multiplier *in_scale); the ReLU' mask comes from
  // the forward's bitmask (mbits_in, conv_fwd_kernel's layout); bf16 output only
  int dgrad_bf16;
  const float* in_scale;
  const uint32_t* mbits_in;
  // forward, optional: stochastic rounding of the e4m3 output (v_cvt_sr_fp8_f32), random bits hashed
  // from (pixel, channel, *sr_seed); the trainer advances the device seed every step
  const int* sr_seed;
};
// ConvFp8Args plus the skip operand of a residual block: the kernel argument of the RES instantiations
// (conv_fwd_fp8_ga_kernel).  res is a bf16 tensor of the bf16 output's shape and padding in real (unscaled)
// units, never an output of the same launch, read at interior pixels only and added in fp32 before the
// ReLU (forward) or the ReLU' bitmask (mbits_in dgrad); the 192-wide production tile only.  It is a struct
// of its own because the hidden kernel arguments (gridDim) follow the explicit ones: a field added to
// ConvFp8Args would move them, and with them one load offset in every kernel that has no skip.
struct ConvFp8ResArgs : ConvFp8Args {
  const __bf16* res;
};

// Kernel choices are explicit launch arguments (ConvFwdArgs::tile,
// ConvWgradArgs::variant, ConvFp8Args::variant): no process-global state.
void launch_conv_fwd(const ConvFwdArgs& a, int mode, hipStream_t st);
// What of a forward / dgrad launch the tile choice reads (M pixels, board side, kernel side, padded widths,
// ConvFwdArgs::offi), and the choice itself (host only): the tile code launch_conv_fwd runs for a requested
// code (0 = automatic), and that tile's {code, BM, waves, threads, LDS bytes, loop kind, chunk-outer, LDS slots}.
struct FwdShape {
  int M, S, K, Cin, Cout, offi;
};
int fwd_resolve_tile(const FwdShape& g, int mode, int tile);  // mode: with MODE_RES or without, the same tile
void conv_fwd_tile_info(const FwdShape& g, int mode, int tile, int out[8]);
// packed-tap first-layer forward (bias + ReLU, optional bitmask): cpt 8-channel chunks per tap
void launch_conv_fwd_pk(const ConvFwdArgs& a, int cpt, hipStream_t st);
void launch_conv_wgrad(const ConvWgradArgs& a, hipStream_t st);
// split-free wgrad (kWgradDirect): a.grad_w / grad_b / scale / beta / cout_real set; ksub 4 / 8 / 12
void launch_conv_wgrad_direct(const ConvWgradArgs& a, int ksub, hipStream_t st);
bool wgrad_direct_supported(int Cout, int Cin, int cin_real, int K);
// weight-stationary small-batch conv (conv_ws.hip, tile code 40): modes 0 / 2 / 3; target_wgs <= 0: 256
void launch_conv_ws(const ConvFwdArgs& a, int mode, int target_wgs, hipStream_t st, int probe = 0);
// conv_wgrad's small-batch plan (64 x 64 tap-merged tiles; ops.wgrad_config picks it)
constexpr int kWgradSmall = 14;
// split-free small-batch plan: 32 x 48 (or 32 x 32) per-tap tiles, each workgroup owns the whole pixel
// range and writes the OIHW gradient itself (ConvWgradArgs::grad_w; conv_wgrad_direct)
constexpr int kWgradDirect = 15;
// weight-stationary order of standard (tap, Cout, Cin) bf16 packs (conv_ws.hip; tile 40 reads it)
struct WsPackJob {
  const __bf16* src;
  __bf16* dst;
  int Cout, Cin, K;
  int nblk, kw, bn, nwv, ws, slices;  // filled by launch_ws_pack
};
constexpr int kMaxWsPackJobs = 32;
struct WsPackArgs {
  WsPackJob job[kMaxWsPackJobs];
  int n;
};
void launch_ws_pack(const std::vector<WsPackJob>& jobs, hipStream_t st);
bool conv_ws_supported(int Cout, int Cin, int K);
int wgrad_stage_pixels();  // pixels per wgrad pipeline stage (units of ksteps_per_split)
int wgrad_tap_group(int Cout, int Cin, int K, int variant);  // taps per wgrad workgroup (tap-merged 64-wide c tiles)
// one-kernel-row wgrad (conv_wgrad_row.hip): geometry code (0 = not applicable), grid per split, launch
int wgrad_row_code(int Cout, int Cin, int cin_real, int K);
int wgrad_row_wgs_per_split(int code, int Cout, int Cin, int cin_real, int K);
void wgrad_row_launch(int code, const ConvWgradArgs& a, hipStream_t st);
// The tile launch_conv_wgrad runs for a layer and variant (host only; the launch and this are one walk over
// the launchers): taps per workgroup, workgroups per split, the resident workgroups per CU its grid is sized
// for, threads per workgroup, and the tile's n x c widths.  wgrad_plan: the first four, for the trainers.
// Both raise for width pairs the launcher has no tile for (Cout 160 with a Cin that is neither 160 nor an odd
// multiple of 64; Cin 160 with another Cout), as the launch does.
struct WgradChoice {
  int taps, wgs_per_split, per_cu, threads, wn, wc, lds_bytes;
};
WgradChoice wgrad_choose(int Cout, int Cin, int cin_real, int K, int variant);
void wgrad_plan(int Cout, int Cin, int cin_real, int K, int variant, int out[4]);
// a launch the runtime must reject (block of 2048 threads): tests the error path
void launch_invalid_config_probe(hipStream_t st);
#ifdef AGK_DEBUG
// debug build: waits for the stream, returns and clears the bounds-violation
// code recorded by the conv kernels (0 = none)
unsigned debug_error_fetch_and_clear(hipStream_t st);
#endif
void launch_wgrad_reduce(const WgradReduceArgs& a, hipStream_t st);
void launch_wgrad_reduce_multi(const std::vector<WgradReduceArgs>& jobs, hipStream_t st);
void launch_policy_head(const PolicyHeadArgs& a, bool train, hipStream_t st);
void launch_policy_head_soft(const PolicyHeadSoftArgs& a, hipStream_t st);
void launch_head_logits(const PolicyHeadArgs& a, hipStream_t st);
void launch_head_backward(const PolicyHeadArgs& a, const float* dlogits, hipStream_t st);
void launch_value_out(const ValueOutArgs& a, hipStream_t st);

// Dual-head inference (head_pv.hip): one pass over the trunk's last activation gives the policy
// head's masked softmax and the value head's 1x1-conv logits (the input of dense_f32 / value_out).
struct PolicyValueHeadArgs {
  const __bf16* y;       // padded NHWC (HP = S+2, P = 1, C)
  const float* wp;       // [C_real] policy head
  const float* bp;       // [1]
  const float* wv;       // [C_real] value head
  const float* bv;       // [1]
  const uint8_t* legal;  // [B][S*S] or null
  float* probs;          // [B][S*S] policy_head_probs' bits
  float* zv;             // [B][S*S] y . wv + bv (head_logits' quantity)
  int B, S, C, C_real;
};
void launch_policy_value_head(const PolicyValueHeadArgs& a, hipStream_t st);
// head_backward that adds into dz instead of overwriting it (PolicyHeadArgs: y, w, dz, dhead, B, S, C, C_real)
void launch_head_backward_add(const PolicyHeadArgs& a, const float* dlogits, hipStream_t st);

// The ownership head of the dual net (head_own.hip): a third 1x1 head, tanh per board point, trained
// on the final territory map in the mover's frame.
//
// value_own_head: one read of the board gives the value head's logits zv (head_logits' quantity) and the
// ownership row o = y . wo + bo, own = tanhf(o).  With a target t (int8 in {-1, 0, +1}, stored frame,
// gathered through the board's symmetry as policy_head_soft gathers tdist) also, per board,
//   oloss = (1 / SS) sum_p (own - t)^2,  oagree = #{p : t != 0 and sign(own) == t},
//   dlo[p] = grad_scale * k * (2 / SS) * (own - t) * (1 - own^2),  k = valid[b] * weight[b] (null = 1);
// a board with k == 0 writes zeros to dlo and still writes oloss and oagree.
struct ValueOwnHeadArgs {
  const __bf16* y;       // padded NHWC (HP = S+2, P = 1, C)
  const float* wv;       // [C_real] value head
  const float* bv;       // [1]
  const float* wo;       // [C_real] ownership head
  const float* bo;       // [1]
  const int8_t* target;  // [B][S*S] or null (forward only)
  const int* sym;        // [B] in 0..7 or null
  const float* valid;    // [B] or null
  const float* weight;   // [B] or null
  float* zv;             // [B][S*S]
  float* own;            // [B][S*S] or null
  float* olog;           // [B][S*S] or null: the ownership row before tanh
  float* oloss;          // [B]        (with a target)
  float* oagree;         // [B]        (with a target)
  float* dlo;            // [B][S*S]   (with a target)
  int B, S, C, C_real;
  float grad_scale;
};
void launch_value_own_head(const ValueOwnHeadArgs& a, hipStream_t st);

// head_backward_add for two heads in one pass over y and dz.  Where y > 0:
//   dz[p, c] = bf16_rne(fma(g2[p], w2[c], fma(g1[p], w1[c], float(dz[p, c]))))
// and two partial blocks [B][C_real + 1], each in head_backward_add's order.
struct HeadBackwardAdd2Args {
  const __bf16* y;
  const float* w1;  // [C_real]
  const float* w2;  // [C_real]
  const float* g1;  // [B][S*S]
  const float* g2;  // [B][S*S]
  __bf16* dz;
  float* dhead1;    // [B][C_real + 1]
  float* dhead2;    // [B][C_real + 1]
  int B, S, C, C_real;
};
void launch_head_backward_add2(const HeadBackwardAdd2Args& a, hipStream_t st);

// policy_value_head plus the ownership row: probs and zv with policy_value_head's bits, own = tanhf(y . wo + bo)
struct PolicyValueOwnHeadArgs {
  PolicyValueHeadArgs pv;
  const float* wo;  // [C_real]
  const float* bo;  // [1]
  float* own;       // [B][S*S]
};
void launch_policy_value_own_head(const PolicyValueOwnHeadArgs& a, hipStream_t st);

// fused move sampling (sample.hip): out[b] = a draw from probs[b]**beta, -1 where has[b] == 0
struct SampleArgs {
  const float* probs;    // [B][NP]
  const uint8_t* has;    // [B] any sensible move, or null: then
  const uint8_t* legal;  // [B][NP] sensible-move mask, "has" = any nonzero entry of the row
  int64_t* out;          // [B]
  int B, NP;
  float beta;
  uint64_t seed;
};
void launch_sample_moves(const SampleArgs& a, hipStream_t st);
void launch_head_grad_sums(const float* dhead, int B, int N, const float* loss, const float* correct, float* grad,
                           float* sums, hipStream_t st);
void launch_pack_input(const PackInputArgs& a, hipStream_t st);

// D4 symmetry ensembling at inference (symmetry.hip).  A trunk batch of G * B boards holds board b of
// the submission under symmetry sym[g * B + b] at index g * B + b.
struct D4ExpandArgs {
  const __bf16* src;  // padded NHWC [B][S+2P][S+2P][Cp]
  __bf16* dst;        // [GB][S+2P][S+2P][Cp]: board k = board k % B of src under sym[k] (interior only)
  const int* sym;     // [GB] in 0..7
  int B, GB, S, P, Cp;
};
struct PolicyHeadD4Args {
  const __bf16* y;       // trunk output of the G * B boards, padded NHWC (P = 1, C)
  const float* w;        // [C_real]
  const float* b;        // [1]
  const uint8_t* legal;  // [B][S*S] in the original frame, or null
  const int* sym;        // [G * B]
  float* probs;          // [B][S*S] original frame: the mean over g of the G distributions mapped back
  float* scratch;        // [G * B][S*S] or null: lets small batches run one workgroup per orientation
  int B, G, S, C, C_real;
  float inv_temp;
  float inv_g;           // (float)(1.0 / G), filled by the launcher
  int LB;                // period of legal's rows over the kernel's boards (launcher)
};
// positions below which policy_head_d4 (G > 1, scratch given) runs one workgroup per orientation and a
// group_mean pass instead of one workgroup per position walking its G orientations
constexpr int kD4SplitBelow = 128;
void launch_d4_expand(const D4ExpandArgs& a, hipStream_t st);
void launch_policy_head_d4(const PolicyHeadD4Args& a, hipStream_t st);
// out[b] = (v[b] + v[B + b] + ... + v[(G - 1) B + b]) * (1 / G), fp32 in g order
void launch_group_mean(const float* v, float* out, int B, int G, hipStream_t st);
void launch_pack_weights(const PackWeightsArgs& a, hipStream_t st);

// Global pooling branch of the residual trunk (gpool.hip).  Activations are padded NHWC bf16 (P = 1, C a
// multiple of 8); only interior pixels are read or written.
struct GpoolFwdArgs {
  const __bf16* y;   // [B][S+2][S+2][C]
  float* pooled;     // argmax given: [B][2][C] {sum * inv, max}; argmax null (sum mode): [B][C] sum * inv
  int* argmax;       // [B][C] lowest pixel index r * S + col attaining the maximum, or null
  int B, S, C;
  float inv;         // float32(1 / (S * S)) for the mean; 1 for a plain sum
  long long y_elems; // tensor extent (debug-build bounds checks)
};
void launch_gpool_fwd(const GpoolFwdArgs& a, hipStream_t st);
struct GpoolMapArgs {
  const __bf16* skip;  // bias add: [B][S+2][S+2][C] (may be out); fill: unused
  const float* g;      // bias add: [B][C]; fill: dp [B][2][C]
  const int* argmax;   // fill: [B][C]
  __bf16* out;         // [B][S+2][S+2][C]
  int B, S, C;
  float inv;           // fill: float32(1 / (S * S))
  long long elems;     // extent of skip and out (debug-build bounds checks)
};
// fill = false: out = bf16(float(skip) + g[b][c]); true: out = bf16(dp[b][0][c] * inv + (p == argmax[b][c] ?
// dp[b][1][c] : 0)), product and sum rounded separately
void launch_gpool_map(const GpoolMapArgs& a, bool fill, hipStream_t st);

// The pass head of the dual net (the pooling gradient in gpool.hip): one more policy logit
// z_pass[b] = pooled[b].reshape(2 C) . pass_w + pass_b from gpool_fwd's (B, 2, C) of the trunk output, the
// softmax over S*S + 1 entries with the pass last.  Both pass kernels take their plain sibling's arguments
// plus these operands; the *_elems fields are tensor extents for the debug build's bounds checks.
struct PassHeadOperands {
  const float* pooled;   // [B][2][C] gpool_fwd(y)
  const float* pass_w;   // [2][C] zero-padded copy of the (2 C_real, 1) weight
  const float* pass_b;   // [1]
  float* dpass;          // [B] dL/dz_pass                                              (training head)
  float* dpw;            // [B][2 C_real + 1] partials [dzp * pooled (2 C_real) | dzp]  (training head)
  long long pooled_elems, tdist_elems, dpass_elems, dpw_elems, probs_elems;
};
// policy_head_soft over S*S + 1 entries (head_soft.hip): head.tdist rows are [S*S + 1] with the pass last
// (head.T == S*S + 1); the board part moves with sym, the pass entry does not
struct PolicyHeadSoftPassArgs {
  PolicyHeadSoftArgs head;
  PassHeadOperands pass;
};
void launch_policy_head_soft_pass(const PolicyHeadSoftPassArgs& a, hipStream_t st);
// policy_value_head / policy_value_own_head (head.wo given) with the pass entry (head_own.hip): probs rows of
// S*S + 1; the pass is always legal
struct PolicyValuePassHeadArgs {
  PolicyValueOwnHeadArgs head;  // wo, bo, own null: no ownership row
  PassHeadOperands pass;
};
void launch_policy_value_pass_head(const PolicyValuePassHeadArgs& a, hipStream_t st);
// dz += ReLU'(y) * (dpass[b] * w[0][c] * inv + (p == argmax[b][c] ? dpass[b] * w[1][c] : 0)), interior only
struct GpoolBwdAddArgs {
  const float* dpass;  // [B]
  const float* w;      // [2][C] zero-padded pass_w
  const int* argmax;   // [B][C] gpool_fwd's
  const __bf16* y;     // [B][S+2][S+2][C] the pooled activation (after its ReLU)
  __bf16* dz;          // [B][S+2][S+2][C] read-modify-write
  int B, S, C;
  float inv;           // float32(1 / (S * S))
  long long elems;     // extent of y and dz
};
void launch_gpool_bwd_add_masked(const GpoolBwdAddArgs& a, hipStream_t st);
// dz += ReLU'(y) * (dp[b][0][c] * inv + (p == argmax[b][c] ? dp[b][1][c] : 0)) for a general dp (the score head),
// with GpoolBwdAddArgs' pass term in the same pass when dpass / w are given (gpool.hip)
struct GpoolBwdAddDpArgs {
  const float* dp;     // [B][2][C], 16-byte aligned
  const float* dpass;  // [B] or null
  const float* w;      // [2][C] zero-padded pass_w, or null
  const int* argmax;   // [B][C] gpool_fwd's
  const __bf16* y;     // [B][S+2][S+2][C] the pooled activation (after its ReLU)
  __bf16* dz;          // [B][S+2][S+2][C] read-modify-write
  int B, S, C;
  float inv;           // float32(1 / (S * S))
  long long elems;     // extent of y and dz
};
void launch_gpool_bwd_add_masked_dp(const GpoolBwdAddDpArgs& a, hipStream_t st);
// The score head's output layer (head_score.hip): s = relu(upre) . w2 + b2; with a target the Huber loss, |e|,
// du and the per-board partial row [g * u | g]; with value, the score utility written over the value column.
// The *_elems fields are tensor extents for the debug build's bounds checks.
struct ScoreOutArgs {
  const float* upre;    // [B][D]
  const float* w2;      // [D]
  const float* b2;      // [1]
  float* s;             // [B]
  const float* target;  // [B] in units of S points, or null (forward only)
  const float* valid;   // [B] or null
  const float* weight;  // [B] or null
  float* loss;          // [B]
  float* abserr;        // [B]
  float* du;            // [B][D]
  float* dout;          // [B][D + 1]
  float* value;         // [B] or null: rewritten as (value + lam * tanh(s / 2)) / (1 + lam)
  int B, D;
  float grad_scale, delta, lam;
  long long upre_elems, du_elems, dout_elems;
};
void launch_score_out(const ScoreOutArgs& a, hipStream_t st);
void launch_featurize(const FeaturizeArgs& a, hipStream_t st);
// res: the skip operand (ConvFp8ResArgs::res) or null
void launch_conv_fwd_fp8(const ConvFp8Args& a, hipStream_t st, const __bf16* res = nullptr);
void launch_pack_weights_fp8(const float* w, uint8_t* out, int Cout_real, int Cin_real, int K, int Cout_p, int Cin_p,
                             int nch, float scale, const float* scale_dev, int transposed, int cw, hipStream_t st);
struct Fp8WeightScalesArgs {
  const float* w[kMaxPackLayers];
  int n[kMaxPackLayers];
  float* wscale;  // [L]
  int* scales8;   // [L][2]
};
void launch_fp8_weight_scales(const Fp8WeightScalesArgs& a, int L, hipStream_t st);
// every fp8 weight pack of a repack (forward and transposed dgrad packs of all layers) in one launch
constexpr int kMaxFp8PackJobs = 48;
struct Fp8PackJob {
  const float* w;         // OIHW fp32
  uint8_t* out;           // [nch][rows_p][64] e4m3
  const float* scale;     // device scale (one float)
  int Cout_real, Cin_real, K, Cout_p, Cin_p, nch, transposed;
  int cw;                 // chunk width (channels per chunk): 64, or 32 for the 160-channel value layers
};
struct Fp8PackArgs {
  Fp8PackJob jobs[kMaxFp8PackJobs];
  int n;
};
void launch_pack_weights_fp8_multi(const Fp8PackArgs& a, hipStream_t st);
void launch_fp8_act_scales(unsigned* amax, int* scales8, float* osc, int L, int margin, int max_drop, hipStream_t st);
void launch_fp8_grad_scales(unsigned* amax, int* gscales8, float* gosc, int L, int margin, hipStream_t st);
void launch_quantize_bf8_dev(const __bf16* x, uint8_t* y, long n, const float* scale, unsigned* amax, hipStream_t st,
                             bool e4m3 = false);
void launch_quantize_fp8(const __bf16* x, uint8_t* y, long n, float scale, hipStream_t st);
#ifdef AGK_KERNEL_LAB
void launch_bf8_convert_probe(const __bf16* x, uint8_t* y, long n, float scale, int mode, hipStream_t st);
#endif
// p, g: 16-byte aligned (float4 accesses; ops.cpp refuses anything else)
void launch_sgd(float* p, const float* g, int64_t n, float lr, float gscale, hipStream_t st);

// fused SGD + bf16 weight packs (pack.hip sgd_pack_kernel)
constexpr int kSgdPackMaxTaps = 25;
constexpr int kSgdPackMaxRanges = 64;
struct SgdPackLayer {
  int64_t off;     // OIHW fp32 weights at p + off (and their gradient at g + off)
  __bf16* wf;      // forward pack [T][Cout_p][Cin_p], or the packed-tap layout when pk_cpt > 0
  __bf16* wd;      // transposed dgrad pack [T][Cin_p][Cout_p] (taps flipped) or null
                   // Never written (they keep the allocation's zeros): a trailing extra tap of wf / wd, and in
                   // the packed-tap layout the chunks of the last step past tap T - 1 (q >= T * pk_cpt), which
                   // pack_weights_kernel does zero
  int Cout_real, Cin_real, Cout_p, Cin_p, K, pk_cpt;
};
struct SgdPackArgs {
  float* p;
  const float* g;
  float lr, gscale;
  double* sched;   // device Keras schedule {lr0, decay, iterations, lr} (advanced first) or null: lr
  SgdPackLayer layers[kMaxPackLayers];
  int nlayers;
  int64_t range_off[kSgdPackMaxRanges];
  int range_len[kSgdPackMaxRanges];
  int nranges;
  // optimizer (Keras 1.0 SGD / Adam semantics): 0 = SGD (p -= lr g), 1 = SGD with momentum
  // (v = mom v - lr g; p += v, or p += mom v - lr g with nesterov), 2 = Adam (m1, m2 = first and second
  // moments; the bias-corrected step lr_t comes from the device schedule or the host).  m1 / m2 are flat
  // fp32 buffers parallel to p.
  int opt;
  float* m1;
  float* m2;
  float mom, b1, b2, eps;
  int nesterov;
};
void launch_sgd_pack(const SgdPackArgs& a, hipStream_t st);
// RCCL all-reduce stand-in (comm_proxy.hip): channels workgroups copy n floats and hold their CUs wire_us
void launch_comm_proxy(const float* src, float* dst, long n, int channels, double wire_us, hipStream_t st);

// fp32 dense layer GEMM (value head): C[M][N] = beta*C + A.B (+ bias[n]);
// A is [M][K] (lda) or, transposed, [K][M]; B is [K][N] (ldb) or [N][K]
struct DenseArgs {
  const float* A;
  const float* B;
  const float* bias;  // [N] or null
  float* C;
  int M, N, K, lda, ldb, ldc;
  float beta;
  int splits;  // split-K factor (dense_splits); > 1 needs ws of splits*M*N floats
  int kchunk;  // set by the launcher
  float* ws;
};
int dense_splits(int M, int N, int K);

// GPU ladder planes (ladder.hip; search code ../engine/ladder_bb.h)
struct LadderBoard {
  uint64_t black[6], white[6], cand[6];
  int ko, me;
};
struct LadderArgs {
  const int8_t* board;     // [B][S*S] +1 black, -1 white, 0 empty
  const int32_t* meta;     // [B][2] {ko point or -1, player to move}
  LadderBoard* boards;     // [B] prep output
  int32_t* counts;         // [B] candidate points per board
  const int32_t* offsets;  // [B] exclusive prefix sum of counts
  int32_t* counter;        // zeroed task counter of the search kernel
  void* frames;            // search threads x ladder_frame_bytes() (frame stacks)
  int budget;              // node visits per capture / escape read (lb::kLadderVisits)
  uint8_t* out;            // [B][S*S] zeroed; bit 0 = ladder capture, bit 1 = ladder escape
  int B, S;
};
size_t ladder_frame_bytes();
void launch_ladder_prep(const LadderArgs& a, hipStream_t st);
void launch_ladder_search(const LadderArgs& a, int threads, hipStream_t st);
void launch_dense_f32(const DenseArgs& a, bool transA, bool transB, hipStream_t st);
// device-side schedule (graph-capturable): sched = {lr0, decay, iterations, lr_current} f64
void launch_sgd_sched(float* p, const float* g, int64_t n, double* sched, float gscale, hipStream_t st);

// ---- kernel lab: Winograd F(2x2, 3x3) forward (winograd.hip), bias + ReLU, padded NHWC bf16
struct WinoArgs {
  const __bf16* x;    // padded NHWC input (HP = S + 2), Cin channels
  const __bf16* u;    // transformed weights, packed [16 xi][Cin/32][Cout/16][64 lanes][8]
  const float* bias;  // [Cout] or null
  __bf16* y;          // padded NHWC output (HP = S + 2), Cout channels
  int S, Cin, Cout, ntiles, TS;  // TS = (S + 1) / 2 tiles per row; ntiles = B * TS * TS
};
void launch_wino_fwd(const WinoArgs& a, hipStream_t st);

// kernel lab: ds_read_b64_tr_b8 lane-mapping probe (lab_probes.hip)
void launch_tr8_probe(const uint8_t* lds_init, int nbytes, const int* addr, unsigned long long* out, hipStream_t st);

}  // namespace agk
