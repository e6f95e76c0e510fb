"""HIP (gfx950) kernel library: loading + thin Python wrappers.

The kernels live in ``alphago_amd/csrc/kernels`` and are compiled in-tree into
``alphago_amd/_hip_kernels.so`` (``python -m alphago_amd._build hip``).  They
are registered as ``torch.ops.alphago_amd.*``.  There is no silent fallback:
``load()`` raises if the library is missing on a machine with a GPU.

Tensor conventions (see csrc/kernels/conv.hip): activations are zero-bordered
NHWC bf16 ``(B, S+2P, S+2P, C)`` with C a multiple of 64; packed conv weights
are bf16 ``(K*K, Cout_p, Cin_p)``.
"""
from __future__ import annotations

import functools
import os
import threading
from typing import NamedTuple, Optional

import torch

from .. import _build

_lock = threading.Lock()
_loaded = False

MODE_BIAS_RELU, MODE_MASK, MODE_NONE, MODE_MASKBITS = 0, 1, 2, 3


def flavor() -> str:
    """Kernel library flavor: ``prod`` (default) or ``debug`` (device bounds
    checks, synchronising ops; ``ALPHAGO_AMD_KERNELS=debug``)."""
    f = os.environ.get("ALPHAGO_AMD_KERNELS", "prod")
    if f not in ("prod", "debug"):
        raise ValueError("ALPHAGO_AMD_KERNELS must be prod or debug")
    return f


def library_path() -> str:
    return _build.hip_path(flavor())


def load(build_if_missing: bool = True) -> None:
    """Load the HIP kernel library (building it first if it is absent)."""
    global _loaded
    if _loaded:
        return
    with _lock:
        if _loaded:
            return
        path = library_path()
        if not os.path.exists(path) or os.environ.get("ALPHAGO_AMD_REBUILD"):
            if not build_if_missing:
                raise RuntimeError("alphago_amd HIP kernels not built: %s" % path)
            _build.build_hip(flavor=flavor())
        torch.ops.load_library(path)
        _loaded = True


_lab_loaded = False


def lab():
    """The kernel-lab library (non-production conv tilings and variants) as
    ``torch.ops.alphago_amd_lab``; loads next to the production library."""
    global _lab_loaded
    load()
    with _lock:
        if not _lab_loaded:
            path = _build.hip_path("lab")
            if not os.path.exists(path):
                _build.build_hip(flavor="lab")
            torch.ops.load_library(path)
            _lab_loaded = True
    return torch.ops.alphago_amd_lab


def is_loaded() -> bool:
    return _loaded


def _ops():
    load()
    return torch.ops.alphago_amd


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def pad_filters(F: int) -> int:
    """Padded trunk width for the bf16 conv kernels: multiples of 64, except
    129..160 -> 160 (the value net's 152 filters, AlphaGo/models/value.py:7),
    which runs on 160-wide tiles with straddled K-steps instead of 192."""
    return 160 if 128 < F <= 160 else round_up(F, 64)


def conv_n_tile(C: int) -> int:
    """Output-channel tile of the conv kernels for C padded channels."""
    return 160 if C == 160 else 192 if C % 192 == 0 else 128 if C % 128 == 0 else 64


# ----------------------------------------------------------------- layout helpers
def padded_empty(B: int, S: int, P: int, C: int, device, dtype=torch.bfloat16) -> torch.Tensor:
    """Zero-initialised padded NHWC buffer (borders must stay zero)."""
    return torch.zeros((B, S + 2 * P, S + 2 * P, C), device=device, dtype=dtype)


def to_padded(x: torch.Tensor, P: int, Cp: Optional[int] = None) -> torch.Tensor:
    """NCHW (any float) -> zero-bordered NHWC bf16 with channels padded to Cp."""
    B, C, S, _ = x.shape
    Cp = Cp or round_up(C, 64)
    out = padded_empty(B, S, P, Cp, x.device)
    out[:, P:P + S, P:P + S, :C] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    return out


def from_padded(y: torch.Tensor, P: int, C: Optional[int] = None) -> torch.Tensor:
    """Zero-bordered NHWC -> NCHW fp32 interior."""
    S = y.shape[1] - 2 * P
    C = C or y.shape[3]
    return y[:, P:P + S, P:P + S, :C].permute(0, 3, 1, 2).float()


# ----------------------------------------------------------------- op wrappers
def conv_fwd(x, w_packed, bias, y, K: int, S: int, Pin: int, Po: int = 1, mode: int = MODE_BIAS_RELU, mask=None,
             mbits=None, tile: int = 0, res=None):
    """Conv + epilogue.  mode 0: bias + ReLU (mbits: also write the ReLU' bitmask);
    1: dgrad masked by ``mask`` > 0; 3: dgrad masked by the ``mbits`` bitmask.
    ``res`` (modes 0 and 3, a bf16 tensor of ``y``'s shape that is not ``y``): the skip operand of a
    residual block, ``relu(conv + bias + res)`` / ``(dgrad + res)`` under the bitmask, read at interior
    pixels only.
    ``tile``: 0 = automatic, 40 = weight-stationary, or a tile code of docs/ARCHITECTURE.md's table;
    ``conv_fwd_tile_info`` tells which tile a layer and code run."""
    if res is None:
        _ops().conv_fwd(x, w_packed, bias, mask, y, K, S, Pin, Po, mode, mbits, tile)
    else:
        _ops().conv_fwd(x, w_packed, bias, mask, y, K, S, Pin, Po, mode, mbits, tile, res)
    return y


FWD_LOOPS = ("pipelined", "pipelined, late epilogue load", "plain", "dma-spread", "mfma32", "ring", "compact-halo")


class FwdTileInfo(NamedTuple):
    code: int
    bm: int
    waves: int
    threads: int
    lds_bytes: int
    loop: str
    chunk_outer: bool
    slots: int


def conv_fwd_tile_info(M: int, S: int, K: int, cin_p: int, cout_p: int, mode: int = MODE_BIAS_RELU,
                       res: bool = False, tile: int = 0, Pin: int = -1) -> FwdTileInfo:
    """The tile ``conv_fwd`` runs for ``M`` output pixels of side-``S`` boards and a requested ``tile`` code
    (0 = automatic; not the weight-stationary code 40): the resolved code and its geometry, read on the
    host from the description the launcher instantiates.  ``loop`` is one of ``FWD_LOOPS``."""
    v = [int(t) for t in _ops().conv_fwd_tile_info(M, S, K, cin_p, cout_p, mode, res, tile, Pin)]
    return FwdTileInfo(v[0], v[1], v[2], v[3], v[4], FWD_LOOPS[v[5]], bool(v[6]), v[7])


# split-K forward / dgrad (tile 38) below this many output pixels (B <= 8 at 19 x 19); ALPHAGO_AMD_SPLITK=0
# turns it off.  SL step (profiles/r4/README.md): B = 1 1.33k -> 1.74k positions/s, B = 4 5.3k -> 6.27k,
# B = 8 10.54k -> 11.09k; at B = 16 the count below is 1 (181 tiles already fill ~144 workgroups).
# Split count: ~144 workgroups per layer -- graph-timed 192 -> 192 3x3 forwards
# (scripts/r4/launch_floor.py) are fastest at 9 splits for B = 1 (11.4 us vs 16.8 unsplit), 6 for
# B = 2 and 3 for B = 4 (14.7 us; 9 splits 16.3): more splits cost more in partials than they hide
SPLITK_MAX_M = int(os.environ.get("ALPHAGO_AMD_SPLITK_MAX_M", "3000"))
SPLITK_TARGET_WGS = int(os.environ.get("ALPHAGO_AMD_SPLITK_WGS", "144"))


def splitk_nsplit(M: int, cout_p: int, cin_p: int, K: int, target_wgs: int = SPLITK_TARGET_WGS) -> int:
    """Split count of the small-batch split-K conv (conv_fwd_splitk): enough 32-pixel workgroups for
    ``target_wgs``, at least three K-steps (64-channel chunks of a tap; 160-channel inputs run
    straddled steps) per split; 1 = no split (large M, ALPHAGO_AMD_SPLITK=0)."""
    if M >= SPLITK_MAX_M or os.environ.get("ALPHAGO_AMD_SPLITK", "1") == "0":
        return 1
    tiles = (M + 31) // 32 * (cout_p // conv_n_tile(cout_p))
    nk = -(-K * K * cin_p // 64)
    return max(1, min(nk // 3, -(-target_wgs // tiles), 64))


# Weight-stationary small-batch conv (tile 40, conv_ws.hip): the output-channel slice's weights stay in
# the workgroup's VGPRs (read once, in the weight-stationary order of ws_pack) while 16-pixel chunks stream
# past through an LDS ring of input rows.  Automatic up to these output-pixel counts (graph-timed chains of
# 11 layers with distinct weights, scripts/r5/ws_bench.py, profiles/r5/README.md): 192-wide layers
# 6.7 / 9.8 / 12.6 / 18.7 us at B = 1 / 8 / 16 / 32 vs 20.3 / 19.4 / 19.9 / 22.6 on the automatic tile
# (30.1 vs 25.5 at B = 64), 160-wide 7.2 .. 16.7 us vs 20.1 .. 20.5.  Training steps stop at B = 16: there
# the forward and dgrad share the GPU with the side-stream wgrad, and the one-workgroup-per-CU kernel
# (122 KB of LDS) lost at B = 32 (SL 34.4k vs 36.2k positions/s; B = 16: 22.8k vs 22.0k, same box).
# ALPHAGO_AMD_WS=0: off.
WS_MAX_M = {192: 32 * 361, 160: 32 * 361}
WS_MAX_M_TRAIN = {192: 16 * 361, 160: 16 * 361}


def ws_pack(srcs, dsts) -> None:
    """Weight-stationary order (what conv_fwd tile 40 reads) of standard (T, Cout, Cin) bf16 packs into
    same-shape tensors, all pairs in one launch."""
    srcs, dsts = list(srcs), list(dsts)
    if srcs:
        _ops().ws_pack(srcs, dsts)


def ws_packed_like(w_packed: torch.Tensor) -> torch.Tensor:
    """A tensor for the weight-stationary copy of a standard bf16 pack (``ws_pack``)."""
    return torch.empty_like(w_packed)


def conv_ws_supported(cout_p: int, cin_p: int, K: int) -> bool:
    """Whether the weight-stationary kernel (tile 40) has an instantiation for this layer shape."""
    return bool(_ops().conv_ws_supported(cout_p, cin_p, K))


def ws_applies(M: int, cout_p: int, cin_p: int, K: int, training: bool = False) -> bool:
    """Whether a conv of M output pixels runs on the weight-stationary kernel (tile 40); ``training``:
    inside a training step (lower limit, see WS_MAX_M_TRAIN)."""
    limit = (WS_MAX_M_TRAIN if training else WS_MAX_M).get(conv_n_tile(cout_p), 0)
    if os.environ.get("ALPHAGO_AMD_WS", "1") == "0" or M > limit:
        return False
    return bool(_ops().conv_ws_supported(cout_p, cin_p, K))


def conv_fwd_splitk(x, w_packed, bias, y, K: int, S: int, Pin: int, Po: int, mode: int, mbits, ws, nsplit: int,
                    res=None):
    """conv_fwd on the 32-pixel tile with its K loop split over ``nsplit`` workgroups per tile (fp32
    partials in ``ws``, >= nsplit * M * Cout floats) and one finishing pass: modes 0 (bias + ReLU,
    optional bitmask), 2 (none), 3 (bitmask dgrad).  ``res``: conv_fwd's skip operand (modes 0 and 3),
    added by the finishing pass."""
    if res is None:
        _ops().conv_fwd_splitk(x, w_packed, bias, y, K, S, Pin, Po, mode, mbits, ws, nsplit)
    else:
        _ops().conv_fwd_splitk(x, w_packed, bias, y, K, S, Pin, Po, mode, mbits, ws, nsplit, res)
    return y


class ConvPlan(NamedTuple):
    """Which kernel runs one bf16 conv layer (forward or bitmask dgrad) at one batch: ``plan_conv``."""
    kind: str    # "ws" (weight-stationary, tile 40), "splitk" (32-pixel tile, K loop split) or "tile"
    nsplit: int  # split count of "splitk", otherwise 1
    tile: int    # conv_fwd's tile argument ("tile": 0 = the library chooses)


def plan_conv(M: int, cout_p: int, cin_p: int, K: int, *, training: bool = False, tile: int = 0,
              small: bool = True) -> ConvPlan:
    """The one place that picks the kernel of a bf16 conv layer with M output pixels: the weight-stationary
    tile where ``ws_applies``, else the split-K tile where ``splitk_nsplit`` is above 1, else the library's
    tile -- the only outcome with an explicit ``tile`` or ``small=False`` (fp8 engines, kernel-lab runs).
    Kind "tile" with tile 0 means the library chooses among its own tiles (conv.hip launch_fwd_t).
    ALPHAGO_AMD_WS and ALPHAGO_AMD_SPLITK are read at every call."""
    if tile == 0 and small:
        if ws_applies(M, cout_p, cin_p, K, training=training):
            return ConvPlan("ws", 1, 40)
        ns = splitk_nsplit(M, cout_p, cin_p, K)
        if ns > 1:
            return ConvPlan("splitk", ns, 38)
    return ConvPlan("tile", 1, tile)


def splitk_workspace_numel(plans, M: int, cout_p: int) -> int:
    """Floats of the fp32 partials workspace the split-K plans among ``plans`` (None entries skipped)
    share: the largest ``nsplit * M * cout_p``; 0 when none splits."""
    return max([p.nsplit * M * cout_p for p in plans if p is not None and p.kind == "splitk"], default=0)


def conv_planned(plan: ConvPlan, x, w, w_ws, bias, y, K: int, S: int, pin: int, mode: int = MODE_BIAS_RELU,
                 mbits=None, sk_ws=None, res=None):
    """The one launch of a planned conv layer into ``y`` (output border 1).  ``w``: the standard pack,
    ``w_ws``: its weight-stationary copy ("ws" plans only), ``sk_ws``: the split-K workspace.  The bitmask
    dgrad is ``mode=MODE_MASKBITS`` on the transposed packs without bias.  ``res``: the skip operand of a
    residual block's last layer (conv_fwd), on every plan kind."""
    if res is not None:
        if plan.kind == "splitk":
            _ops().conv_fwd_splitk(x, w, bias, y, K, S, pin, 1, mode, mbits, sk_ws, plan.nsplit, res)
        else:
            _ops().conv_fwd(x, w_ws if plan.kind == "ws" else w, bias, None, y, K, S, pin, 1, mode, mbits,
                            plan.tile, res)
    elif plan.kind == "splitk":
        _ops().conv_fwd_splitk(x, w, bias, y, K, S, pin, 1, mode, mbits, sk_ws, plan.nsplit)
    else:
        _ops().conv_fwd(x, w_ws if plan.kind == "ws" else w, bias, None, y, K, S, pin, 1, mode, mbits, plan.tile)
    return y


def sample_moves(probs: torch.Tensor, has: torch.Tensor, beta: float, seed: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,) int64 device moves: one draw per board from probs ** beta (a counter-based hash of
    (seed, board) supplies the uniform), -1 where ``has`` is false (sample.hip).  ``has``: (B,) flags,
    or the (B, NP) uint8 sensible-move mask (the kernel reduces each row)."""
    if out is None:
        out = torch.empty(probs.shape[0], dtype=torch.int64, device=probs.device)
    _ops().sample_moves(probs.contiguous(), has.contiguous(), out, float(beta), int(seed) & ((1 << 63) - 1))
    return out


def pk_shape_ok(cin_real: int, cin_p: int) -> bool:
    """Whether the packed-tap forward (conv_fwd_pk) can run a first layer: 32 < cin_real < 64 real input
    channels in a 64-channel padded input (48 policy / 49 value planes)."""
    return cin_p == 64 and 32 < cin_real < 64




def packed_weight_pk(w_oihw: torch.Tensor, cout_p: int, device=None) -> torch.Tensor:
    """Zeroed packed-tap weights (ceil(K*K*cpt/8), Cout, 64), cpt = ceil(cin_real/8); pack_weights fills
    them (chunk j of step s = tap (8s + j) // cpt, channels 8 ((8s + j) % cpt) ..)."""
    K, cin = w_oihw.shape[2], w_oihw.shape[1]
    cpt = (cin + 7) // 8
    return torch.zeros(((K * K * cpt + 7) // 8, cout_p, 64), device=w_oihw.device if device is None else device,
                       dtype=torch.bfloat16)


def conv_fwd_pk(x, w_pk, bias, y, K: int, S: int, Pin: int, Po: int, cin_real: int, mbits=None):
    """Kernel lab: the first layer (bias + ReLU, optional ReLU' bitmask) on the packed-tap K loop -- only
    the cin_real real channels of the 64-channel padded input are multiplied (48 planes: 19 K-steps
    instead of 25).  It multiplies 24 % fewer MFMAs but a K-step's row gathers from two or three pixels,
    and at B = 2176 it measured 399.5 us against the 64-channel kernel's ~381-398 us (round 4), so the
    trainers no longer use it."""
    lab().conv_fwd_pk(x, w_pk, bias, y, K, S, Pin, Po, cin_real, mbits)
    return y


def mbits_words(cout_p: int) -> int:
    """32-bit ReLU'-bitmask words per padded pixel for a conv with cout_p output channels."""
    return cout_p // conv_n_tile(cout_p) * 8


def conv_wgrad(x, dz, slab, dbslab, K: int, S: int, Pin: int, Po: int = 1, cin_real: int = 0, variant: int = 0):
    """Split-K weight gradient into ``slab``; ``cin_real`` (< padded Cin) lets
    the kernel skip zero-padded input channels (only slab columns < cin_real are written).
    ``variant`` 0 = the production per-tap kernel; any other variant is a kernel-lab kernel
    (torch.ops.alphago_amd_lab: 9 = LDS ring, 10-13 = first-layer re-cuts, ...)."""
    (_ops() if variant in (0, WGRAD_SMALL) else lab()).conv_wgrad(x, dz, slab, dbslab, K, S, Pin, Po, cin_real,
                                                                  variant)


def conv_wgrad_reduce(slab, dbslab, grad_w, grad_b=None, scale: float = 1.0, beta: float = 0.0):
    _ops().conv_wgrad_reduce(slab, dbslab, grad_w, grad_b, scale, beta)


def conv_wgrad_reduce_multi(slabs, dbslabs, grad_ws, grad_bs, scale: float = 1.0, beta: float = 0.0):
    """Every listed layer's split-K reduce in ONE launch (<= 16 layers); bitwise equal to one
    ``conv_wgrad_reduce`` per layer (same fixed summation order)."""
    _ops().conv_wgrad_reduce_multi(list(slabs), list(dbslabs), list(grad_ws), list(grad_bs), float(scale),
                                   float(beta))


def conv_wgrad_direct(x, dz, grad_w, grad_b, K: int, S: int, Pin: int, Po: int = 1, scale: float = 1.0,
                      beta: float = 0.0, ksub: int = 4):
    """Split-free weight gradient (C++ kWgradDirect): every workgroup owns one 32 x 48 (or 32 x 32) tile of
    one tap over all B*S*S pixels and writes ``grad_w`` (OIHW fp32, real channel counts: grad_w.shape[1] <
    the padded Cin skips the zero planes) = beta * grad_w + scale * dW, and ``grad_b`` likewise -- no split
    slab, no reduce launch, deterministic.  ``ksub``: 32-pixel sub-steps per pipeline stage (1 / 2 / 4 / 8)."""
    _ops().conv_wgrad_direct(x, dz, grad_w, grad_b, K, S, Pin, Po, float(scale), float(beta), int(ksub))


def wgrad_direct_supported(cout_p: int, cin_p: int, cin_real: int, K: int) -> bool:
    return bool(_ops().wgrad_direct_supported(cout_p, cin_p, cin_real or cin_p, K))


def policy_head_train(y, w, b, target, dz, loss, correct, dhead, S: int, grad_scale: float, weight=None,
                      bce: bool = False, ref_probs=None, stats=None, ent_coef: float = 0.0, kl_coef: float = 0.0,
                      probs=None):
    """Fused policy head training step; ``bce`` selects the reference RL loss
    (binary CE on the softmax, reinforcement_policy_trainer.py:109) instead of CE.

    ``ent_coef`` (beta) and ``kl_coef`` (kappa, needs the anchor distribution ``ref_probs`` (B, S*S))
    add -beta H(p) + kappa KL(ref_probs || p) per board to the CE objective (not with ``bce``; neither
    is multiplied by ``weight``).  ``stats`` (B, 3) receives per board H(p), KL(ref_probs || p) (0
    without ``ref_probs``) and max |logit|; ``probs`` (B, S*S) the softmax itself.  With all of them
    left out the plain kernels run."""
    _ops().policy_head(y, w, b, target, None, weight, dz, loss, correct, dhead, probs, S, grad_scale, 1.0,
                       1 if bce else 0, ref_probs, stats, float(ent_coef), float(kl_coef))


def policy_head_train_soft(y, w, b, tdist, dz, loss, correct, dhead, S: int, grad_scale: float, weight=None,
                           sym=None):
    """Fused policy head training step towards a target DISTRIBUTION per board (a search's root visit
    distribution) instead of one move: ``tdist`` (B, S*S) or (B, S*S + 1) f32 in the planes' original
    frame -- a trailing pass column is not read, negative entries count as 0 and the board part is
    renormalised.  ``sym`` (B,) int32 is the tensor ``pack_input`` got: the kernel moves the
    distribution with the board.  Per board ``loss`` = -sum_i q_i log p_i (no clip) and ``correct`` =
    [argmax p == first argmax q]; a row without board mass is "no loss" (zero loss, metric and
    gradient), and so is a row with an infinite entry (NaN entries count as 0).  No ``bce``, regularisers, ``stats`` or ``probs``: those belong to ``policy_head_train``."""
    _ops().policy_head_soft(y, w, b, tdist, sym, weight, dz, loss, correct, dhead, S, float(grad_scale))


def head_grad_sums(dhead, loss, correct, grad, sums):
    """grad = dhead.sum(0) and sums[:2] = (loss.sum(), correct.sum()) in one deterministic launch."""
    _ops().head_grad_sums(dhead, loss, correct, grad, sums)


def policy_head_probs(y, w, b, probs, S: int, legal=None, temperature: float = 1.0, ref_probs=None, stats=None):
    """Softmax of the head (renormalised over ``legal``); ``stats`` (B, 3): per-board entropy,
    KL(ref_probs || p) and max |logit| as in ``policy_head_train``."""
    _ops().policy_head(y, w, b, None, legal, None, None, None, None, None, probs, S, 0.0, temperature, 0,
                       ref_probs, stats)
    return probs


def pack_input(planes_u8, out, P: int, sym=None, target=None, target_out=None, rows=None, out8=None):
    """uint8 planes -> padded NHWC bf16 with the per-board D4 symmetry ``sym`` (and the target moved
    with it).  ``rows`` (int64, B): board b is ``planes_u8[rows[b]]`` -- the minibatch gather from a
    resident pool fused into the pack (a row outside the pool packs an all-zero board).  ``out8``
    (uint8, out's shape): the same values as e4m3 too (``quantize_fp8(out, out8, 0)``'s bytes)."""
    _ops().pack_input(planes_u8, sym, target, target_out, out, P, rows, out8)
    return out


def d4_expand(src, dst, sym, S: int, P: int):
    """Padded NHWC ``src`` (B boards) -> ``dst`` (G*B boards): board ``k`` of ``dst`` is board ``k % B`` of
    ``src`` under the D4 symmetry ``sym[k]`` (int32, pack_input's convention); interior only, a pure
    16-byte-chunk gather.  One featurizer run feeds all G orientations of the ensembled engines."""
    _ops().d4_expand(src, dst, sym, S, P)
    return dst


def policy_head_probs_d4(y, w, b, probs, S: int, sym, G: int, legal=None, temperature: float = 1.0, scratch=None):
    """Symmetry-ensembled ``policy_head_probs``: ``y`` holds the trunk output of G*B boards, board
    ``g*B + b`` being board b under symmetry ``sym[g*B + b]``.  ``probs`` (B, S*S) is the mean over g, in
    g order, of the G legal-masked softmaxes mapped back to the original frame; ``legal`` (B, S*S) is in
    the original frame.  Deterministic (no atomics).  ``scratch`` (G*B, S*S) fp32, optional: with it, fewer
    than 128 positions run one workgroup per orientation into ``scratch`` and a ``group_mean`` pass (the
    same fixed g order) instead of one workgroup per position walking its G orientations."""
    _ops().policy_head_d4(y, w, b, probs, S, sym, G, legal, temperature, scratch)
    return probs


def group_mean(v, out, G: int):
    """out[b] = (v[b] + v[B + b] + ... + v[(G-1) B + b]) * float32(1 / G), fp32 in that order."""
    _ops().group_mean(v, out, G)
    return out


@functools.lru_cache(maxsize=None)
def gpool_inv(S: int) -> float:
    """float32(1 / (S * S)) as a Python float: the factor of the pooling branch's mean, computed once on the
    host (ConvStack.gate_torch multiplies by the same fp32 value)."""
    return float(torch.tensor(1.0 / (S * S), dtype=torch.float32))


def gpool_fwd(y, pooled, argmax, S: int):
    """Global pooling of a padded NHWC bf16 activation ``y`` (B, S+2, S+2, C) over its interior, per board and
    channel: ``pooled`` (B, 2, C) fp32 = {sum * float32(1 / S*S), max}, ``argmax`` (B, C) int32 = the lowest
    pixel index r * S + col attaining the maximum.  fp32 sums in a fixed order, no atomics: two runs give
    the same bits.  ``argmax=None`` is the sum mode: ``pooled`` (B, C) = the plain sum (the same summation),
    the column sum of the branch's backward."""
    _ops().gpool_fwd(y, pooled, argmax, S, 1.0 if argmax is None else gpool_inv(S))
    return pooled


def gpool_bias_add(skip, g, out, S: int):
    """out[b, p, c] = bf16(float(skip[b, p, c]) + g[b, c]) over the interior (one fp32 add, round to nearest
    even); borders are not written.  ``out`` may be ``skip`` (in place)."""
    _ops().gpool_bias_add(skip, g, out, S)
    return out


def gpool_bwd_fill(dp, argmax, out, S: int):
    """Gradient of ``gpool_fwd`` with respect to its input from ``dp`` (B, 2, C) fp32:
    out[b, p, c] = bf16(dp[b, 0, c] * inv + (p == argmax[b, c] ? dp[b, 1, c] : 0)), inv = float32(1 / S*S),
    product and sum rounded separately (no FMA).  Interior only."""
    _ops().gpool_bwd_fill(dp, argmax, out, S, gpool_inv(S))
    return out


def policy_head_soft_pass(y, w, b, pooled, pass_w, pass_b, tdist, dz, loss, correct, dhead, dpass, dpw, S: int,
                          grad_scale: float, weight=None, sym=None):
    """``policy_head_train_soft`` for a net with the pass head: the softmax, the loss, ``correct`` and the
    gradient run over S*S + 1 entries, the pass last.  ``pooled`` (B, 2, C) is ``gpool_fwd(y)``, ``pass_w`` the
    zero-padded (2, C) copy of the net's (2F, 1) weight, ``pass_b`` (1); z_pass = pooled . pass_w + pass_b.
    ``tdist`` must be (B, S*S + 1); its board part moves with ``sym``, the pass entry does not.  Besides
    ``policy_head_train_soft``'s outputs: ``dpass`` (B) = dL/dz_pass and ``dpw`` (B, 2 C_real + 1) =
    [dpass * pooled | dpass] per board, the partials ``head_grad_sums`` turns into d pass_w and d pass_b."""
    _ops().policy_head_soft_pass(y, w, b, pooled, pass_w, pass_b, tdist, sym, weight, dz, loss, correct, dhead, dpass,
                                 dpw, S, float(grad_scale))


def policy_value_pass_head(y, wp, bp, wv, bv, pooled, pass_w, pass_b, probs, zv, S: int, legal=None, wo=None, bo=None,
                           own=None):
    """``policy_value_head`` (with ``wo``, ``bo``, ``own``: ``policy_value_own_head``) for a net with the pass
    head: ``probs`` (B, S*S + 1) is the softmax at temperature 1 over the legal board points and the pass,
    which is always legal; ``zv`` and ``own`` carry the other op's bits."""
    _ops().policy_value_pass_head(y, wp, bp, wv, bv, wo, bo, pooled, pass_w, pass_b, probs, zv, own, S, legal)


def gpool_bwd_add_masked(dpass, pass_w, argmax, y, dz, S: int):
    """The pass head's pooling gradient, accumulated into the top layer's ``dz`` where ``y`` > 0:
    dz[b, p, c] = bf16(float(dz[b, p, c]) + (dpass[b] * pass_w[0, c] * inv + (p == argmax[b, c] ?
    dpass[b] * pass_w[1, c] : 0))), inv = float32(1 / S*S), every product and sum rounded separately.
    Interior only; elements with ``y`` <= 0 keep their bits."""
    _ops().gpool_bwd_add_masked(dpass, pass_w, argmax, y, dz, S, gpool_inv(S))
    return dz


def gpool_bwd_add_masked_dp(dp, argmax, y, dz, S: int, dpass=None, pass_w=None):
    """The pooling gradient of a general ``dp`` (B, 2, C) fp32 (the score head's), accumulated into the top
    layer's ``dz`` where ``y`` > 0.  With inv = float32(1 / S*S) and

        q  = dp[b, 0, c] * inv + (p == argmax[b, c] ? dp[b, 1, c] : 0)
        r0 = (dpass[b] * pass_w[0, c]) * inv
        r  = p == argmax[b, c] ? fma(dpass[b], pass_w[1, c], r0) : r0

    (``r`` is ``gpool_bwd_add_masked``'s addend with that kernel's bits, taken along in the same pass when
    ``dpass`` / ``pass_w`` are given), add = r + q, or q alone, and dz[b, p, c] = bf16(float(dz[b, p, c]) + add).
    Every product and sum is an fp32 rounding of its own, in the order written (the kernel keeps the compiler from contracting them); the one
    fused multiply-add is the one ``gpool_bwd_add_masked`` executes.  Interior only; elements with ``y`` <= 0
    keep their bits, and so do elements whose addend is zero."""
    _ops().gpool_bwd_add_masked_dp(dp, argmax, y, dz, S, gpool_inv(S), dpass, pass_w)
    return dz


def score_out(upre, w2, b2, s, target=None, valid=None, weight=None, loss=None, abserr=None, du=None, dout=None,
              grad_scale: float = 1.0, delta: float = 1.0, value=None, utility: float = 0.0):
    """The score head's output layer: u = max(upre, 0), s = u . w2 + b2 per board (``upre`` (B, D) fp32, D a
    multiple of 8 in 8..512).  Rounding order of the dot product: lane i of the board's wave accumulates
    fmaf(u[j], w2[j], acc) over j = i, i + 64, ... ascending from 0; the 64 lane sums meet in an xor butterfly
    with offsets 32, 16, 8, 4, 2, 1; ``b2`` is added last.  No atomics: two runs give the same bits.

    With ``target`` (B,) fp32 in the unit of ``s``: e = s - t, ``loss`` = Huber_delta(e) (0.5 e^2 if |e| <= delta,
    else delta (|e| - 0.5 delta)), ``abserr`` = |e|, g = grad_scale * valid[b] * weight[b] * clamp(e, -delta, delta),
    ``du`` = (upre > 0 ? g * w2 : 0) and ``dout`` (B, D + 1) = [g * u | g], the per-board rows ``head_grad_sums``
    turns into [d w2 | d b2].  ``value`` (B,) with ``utility`` = lam: rewritten in place as
    (value + lam * tanh(s / 2)) / (1 + lam), the search utility of the inference engines."""
    _ops().score_out(upre, w2, b2, s, target, valid, weight, loss, abserr, du, dout, float(grad_scale), float(delta),
                     value, float(utility))
    return s


def pack_weights(ws, wf, wd=()):
    _ops().pack_weights(list(ws), list(wf), list(wd))


def comm_proxy(src, dst, channels: int, wire_us: float):
    """RCCL all-reduce stand-in on the current stream (csrc/kernels/comm_proxy.hip)."""
    _ops().comm_proxy(src, dst, channels, wire_us)


def sgd_update(p, g, lr: float, gscale: float = 1.0):
    _ops().sgd_update(p, g, lr, gscale)


OPT_SGD, OPT_MOMENTUM, OPT_ADAM = 0, 1, 2


def sgd_pack(p, g, lr: float, w_meta, wf, wd, ranges, sched=None, gscale: float = 1.0, opt: int = OPT_SGD,
             m1=None, m2=None, momentum: float = 0.0, beta_1: float = 0.9, beta_2: float = 0.999,
             epsilon: float = 1e-8, nesterov: bool = False):
    """Fused optimizer step + bf16 weight packs in one launch (pack.hip sgd_pack_kernel): conv layer i's
    weights at flat offset w_meta[i][0] with shape (Cout, Cin, K, K) = w_meta[i][1:]; the same update over
    ``ranges`` ((offset, length) pairs: biases, head); ``sched`` (device Keras schedule) replaces ``lr``.
    ``opt``: OPT_SGD, OPT_MOMENTUM (velocity ``m1``) or OPT_ADAM (moments ``m1``, ``m2``; ``lr`` is then the
    bias-corrected lr_t, or ``sched`` an 8-entry schedule that computes it) -- Keras 1.0 semantics."""
    meta = [int(v) for m in w_meta for v in m]
    _ops().sgd_pack(p, g, float(lr), sched, float(gscale), meta, list(wf), list(wd), [int(o) for o, _ in ranges],
                    [int(n) for _, n in ranges], int(opt), m1, m2,
                    [float(momentum), float(beta_1), float(beta_2), float(epsilon), 1.0 if nesterov else 0.0])


def dense_f32(A, B, C, bias=None, trans_a: bool = False, trans_b: bool = False, beta: float = 0.0):
    """C = beta*C + op(A) @ op(B) (+ bias) in exact fp32 on the f32 MFMA (value-head dense layers);
    op(X) = X.T when trans_* (read in place, no copies)."""
    _ops().dense_f32(A, B, bias, C, trans_a, trans_b, beta)
    return C


def ladder_planes(board, meta, out, S: int, budget: int = 0):
    """Ladder bits on the device from the compact encoding (board int8 (B, S*S),
    meta int32 (B, 2) {ko, player to move}): out uint8 (B, S*S), bit 0 = ladder
    capture, bit 1 = ladder escape -- the host encoder's ladder bits.  ``budget``:
    node visits per read (0 = the engine's current budget, as the CPU reader)."""
    if budget <= 0:
        from .._native import engine

        budget = engine().ladder_budget()
    lab().ladder_planes(board, meta, out, S, budget)  # kernel lab (ladder.hip: slower than the host reader)
    return out


def sgd_update_sched(p, g, sched, gscale: float = 1.0):
    """SGD with the Keras decay schedule on the device: sched = float64
    {lr0, decay, iterations, lr}; advances iterations (HIP-graph capturable)."""
    _ops().sgd_update_sched(p, g, sched, gscale)


def packed_weight_like(w_oihw: torch.Tensor, cin_p: int, cout_p: int, transposed: bool = False,
                       device=None) -> torch.Tensor:
    """Zeroed packed bf16 weights (K*K, Cout, Cin) -- transposed (K*K, Cin, Cout) for dgrad.  When the
    reduction width (Cin, or Cout for dgrad) is an odd multiple of 32 there is one extra all-zero tap:
    the straddled K-steps' last half reads it."""
    K = w_oihw.shape[2]
    red = cout_p if transposed else cin_p
    T = K * K + (1 if red % 64 == 32 else 0)
    shape = (T, cin_p, cout_p) if transposed else (T, cout_p, cin_p)
    return torch.zeros(shape, device=w_oihw.device if device is None else device, dtype=torch.bfloat16)


def wgrad_tap_group(cout_p: int, cin_p: int, K: int) -> int:
    """Kernel taps one wgrad workgroup covers (K for tap-merged 64-wide c tiles, else 1)."""
    return int(_ops().wgrad_tap_group(cout_p, cin_p, K))


def wgrad_choice(cout_p: int, cin_p: int, K: int, cin_real: int = 0, variant: int = 0):
    """The tile conv_wgrad launches: ``wgrad_plan``'s four values, then the tile's n and c widths and its dynamic
    LDS bytes (host only; read from the launcher's own choice)."""
    return tuple(int(v) for v in _ops().wgrad_choice(cout_p, cin_p, cin_real, K, variant))


def wgrad_plan(cout_p: int, cin_p: int, K: int, cin_real: int = 0, variant: int = 0):
    """(taps per workgroup, workgroups per split, resident workgroups per CU, threads per workgroup) of
    the wgrad kernel the production library runs for this layer."""
    t, w, c, th = _ops().wgrad_plan(cout_p, cin_p, cin_real, K, variant)
    return int(t), int(w), int(c), int(th)


WGRAD_MIN_STAGES = int(os.environ.get("ALPHAGO_AMD_WGRAD_MIN_STAGES", "8"))


def wgrad_nsplit(M: int, cout_p: int, cin_p: int, K: int, cin_real: int = 0, target_wgs: int = 0,
                 cus: int = 256, variant: int = 0) -> int:
    """Pixel splits of the production wgrad: one resident round of workgroups over ``cus`` CUs
    (``target_wgs`` > 0 overrides the workgroup count).  A second, partial round of workgroups costs
    30-70 % (profiles/r2_wgrad_variants.md), so the grid never exceeds one round."""
    _, per_split, per_cu, _ = wgrad_plan(cout_p, cin_p, K, cin_real, variant)
    target = target_wgs if target_wgs > 0 else cus * per_cu
    nks = (M + 31) // 32
    # at least WGRAD_MIN_STAGES 32-pixel stages per split: at small batches one resident round of
    # 3-stage splits spends its time writing a 75-MB slab that the reduce then reads back
    # (B = 16: 16.6 us wgrad + 16.3 us reduce per layer, profiles/r3_small_batch.md)
    return max(1, min(target // per_split, nks // WGRAD_MIN_STAGES if target_wgs <= 0 else nks))


# conv_wgrad's small-batch plan (C++ kWgradSmall): 64 x 64 output tiles with the kernel row's three taps
# merged -- 27 workgroups per pixel split of a 192 -> 192 layer instead of 9 -- on one resident round
# (two per CU).  SL positions/s, same box, per-tap plan -> small plan (profiles/r5/README.md): B = 24
# 30.5k -> 32.1k, B = 32 35.7k -> 39.9k, B = 48 45.0k -> 46.7k, B = 64 54.2k -> 58.3k; B <= 16 equal or
# mixed (22.0-22.8k either way), so it starts above 16 boards.
WGRAD_SMALL = 14
WGRAD_SMALL_M = (16 * 361, 64 * 361)  # (exclusive, inclusive) output-pixel range


def wgrad_config(M: int, cout_p: int, cin_p: int, K: int, cin_real: int = 0, target_wgs: int = 0, cus: int = 256,
                 variant: int = 0):
    """(variant, nsplit) of a layer's wgrad: the requested variant and wgrad_nsplit, or in the small-batch
    range (WGRAD_SMALL_M) the small-batch plan for the 3x3 layers of 64-multiple widths.  (Round 4's
    small-batch LDS-ring variant 9 and the first-layer variants 10-12 are kernel-lab kernels since
    round 5: measured slower or equal.)"""
    if (variant == 0 and WGRAD_SMALL_M[0] < M <= WGRAD_SMALL_M[1] and K == 3 and cout_p % 64 == 0 and
            cin_p % 64 == 0 and cout_p != 160 and (cin_real == 0 or cin_real == cin_p)):
        _, per_split, per_cu, _ = wgrad_plan(cout_p, cin_p, K, cin_real, WGRAD_SMALL)
        target = target_wgs if target_wgs > 0 else cus * per_cu
        nks = (M + 31) // 32
        return WGRAD_SMALL, max(1, min(target // per_split, nks // WGRAD_MIN_STAGES))
    return variant, wgrad_nsplit(M, cout_p, cin_p, K, cin_real, target_wgs, cus, variant)


def wgrad_splits(M: int, T: int, n_tiles: int = 1, target_wgs: int = 512) -> int:
    """Number of pixel splits so the wgrad grid has ~target_wgs workgroups."""
    nks = (M + 31) // 32
    s = max(1, target_wgs // max(1, T * n_tiles))
    return max(1, min(s, nks))


def featurize(board, ages, meta, fids, fplanes, S: int, ladder=None, planes=None, nhwc=None, P: int = 0,
              sensible=None, legal=None, overflow=None):
    """GPU featurizer (csrc/kernels/featurize.hip); see alphago_amd.ops.gpu_features."""
    _ops().featurize(board, ages, meta, ladder, list(fids), list(fplanes), planes, nhwc, sensible, legal, overflow, S, P)


def head_logits(y, w, b, z, S: int):
    """z (B, S*S) fp32 = 1x1 conv of the padded NHWC activation y (value-net head)."""
    _ops().head_logits(y, w, b, z, S)
    return z


def head_backward(y, w, dlogits, dz, dhead, S: int, dz8=None, dz8_scale=None, dz8_amax=None):
    """ReLU'-masked dY of a 1x1 head conv from dlogits, plus per-board [dW | db] partials.  With
    ``dz8`` (uint8, y's shape) dY goes out as e5m2 of bf16(dY) * dz8_scale[0] with max |bf16(dY)| into
    ``dz8_amax`` (int32[64]) -- the bytes quantize_bf8 would make -- and ``dz`` is not written."""
    _ops().head_backward(y, w, dlogits, dz, dhead, S, dz8, dz8_scale, dz8_amax)


def head_backward_add(y, w, dlogits, dz, dhead, S: int, dz8=None):
    """``head_backward`` that accumulates: where y > 0, dz = bf16(dz + dlogits x w) (one fp32 fma, then
    round-to-nearest-even); elsewhere dz keeps its bits.  ``dhead`` as ``head_backward``.  The dual
    trainer's value head adds into the dZ the policy head wrote.  ``dz8`` is refused: an e5m2 buffer
    cannot be accumulated into."""
    _ops().head_backward_add(y, w, dlogits, dz, dhead, S, dz8)


def policy_value_head(y, wp, bp, wv, bv, probs, zv, S: int, legal=None):
    """Both heads of the dual net from one read of the trunk output: ``probs`` (B, S*S) is
    ``policy_head_probs(y, wp, bp, legal)`` bit for bit, ``zv`` (B, S*S) fp32 the value head's 1x1 conv
    ``y . wv + bv`` (``head_logits``' quantity, the input of ``dense_f32``)."""
    _ops().policy_value_head(y, wp, bp, wv, bv, probs, zv, S, legal)
    return probs, zv


def value_own_head(y, wv, bv, wo, bo, zv, S: int, own=None, olog=None, target=None, sym=None, valid=None,
                   weight=None, oloss=None, oagree=None, dlo=None, grad_scale: float = 1.0):
    """The value and ownership heads of the dual net from one read of the trunk output: ``zv`` (B, S*S)
    is ``head_logits(y, wv, bv)``, ``olog = y . wo + bo`` and ``own = tanh(olog)`` (both optional).
    With ``target`` (int8 (B, S*S) in the stored frame; ``sym`` moves it with the board as
    ``policy_head_soft`` moves its distribution) it also writes per board ``oloss`` = mean squared
    error, ``oagree`` = points with target != 0 whose sign ``own`` matches, and ``dlo`` (B, S*S) =
    grad_scale * valid[b] * weight[b] * (2 / S*S) * (own - t) * (1 - own**2)."""
    _ops().value_own_head(y, wv, bv, wo, bo, zv, own, olog, target, sym, valid, weight, oloss, oagree, dlo, S,
                          grad_scale)
    return zv


def head_backward_add2(y, w1, g1, w2, g2, dz, dhead1, dhead2, S: int, dz8=None):
    """``head_backward_add`` for two heads in one pass over ``y`` and ``dz``: where y > 0,
    dz = bf16(fma(g2, w2, fma(g1, w1, dz))); ``dhead1`` / ``dhead2`` as ``head_backward_add``'s
    ``dhead``.  ``dz8`` is refused."""
    _ops().head_backward_add2(y, w1, g1, w2, g2, dz, dhead1, dhead2, S, dz8)


def policy_value_own_head(y, wp, bp, wv, bv, wo, bo, probs, zv, own, S: int, legal=None):
    """``policy_value_head`` plus ``own`` (B, S*S) fp32 = tanh(y . wo + bo), the ownership head."""
    _ops().policy_value_own_head(y, wp, bp, wv, bv, wo, bo, probs, zv, own, S, legal)
    return probs, zv, own


def value_out(h, w2, b2, v, target=None, weight=None, loss=None, correct=None, dh=None, dout=None,
              grad_scale: float = 1.0):
    """v = tanh(h w2 + b2); with target: MSE loss, sign agreement, dh and per-board [dw2 | db2]."""
    _ops().value_out(h, w2, b2, target, weight, v, loss, correct, dh, dout, grad_scale)
    return v


# ----------------------------------------------------------------- fp8 (e4m3)
FP8_MAX = 448.0
FP8_AMAX_SLOTS = 64  # per-layer amax accumulator slots (kFp8AmaxSlots)


def fp8_amax_buffer(L: int, device) -> torch.Tensor:
    """(L, 64) int32 per-layer amax accumulators (float bits); amax of layer l = view(float32)[l].max()."""
    return torch.zeros((L, FP8_AMAX_SLOTS), dtype=torch.int32, device=device)


def fp8_exponent(amax: float, margin: int = 1) -> int:
    """Power-of-two scale exponent e so that amax * 2^e fits e4m3 with `margin` bits of headroom.
    Host helper for initial values only.  It returns 0 for a non-finite amax, and there it differs
    from the device: fp8_weight_scales / fp8_act_scales / fp8_grad_scales turn an infinite amax into
    their lower clamp (-60 / -60 / -100, the smallest multiplier); nor does it clamp to +-60."""
    import math

    if not amax or amax <= 0 or not math.isfinite(amax):
        return 0
    return int(math.floor(math.log2(FP8_MAX / amax))) - margin


def fp8_nchunks(K: int, cin_p: int) -> int:
    """64-channel e4m3 weight chunks (even count); cin_p = 160 uses three chunks per tap."""
    n = K * K * ((cin_p + 63) // 64)
    return n + (n & 1)


def fp8_chunk_width(cin_p: int) -> int:
    """Channels per packed fp8 weight chunk: 32 for 160-channel reductions (the value width: five
    32-channel chunks per tap, no zero half; ALPHAGO_AMD_FP8_CW32=0 restores 64), else 64."""
    return 32 if cin_p == 160 and os.environ.get("ALPHAGO_AMD_FP8_CW32", "1") == "1" else 64


def fp8_weight_shape(K: int, cin_p: int, rows_p: int):
    """Shape of packed e4m3 weights reducing over cin_p channels (forward: input channels; transposed
    dgrad pack: output channels) with rows_p rows: (chunks, rows_p, chunk width); the chunk count
    covers K*K taps and is a multiple of the chunks per 128-K step."""
    cw = fp8_chunk_width(cin_p)
    per = 128 // cw
    n = K * K * ((cin_p + cw - 1) // cw)
    return ((n + per - 1) // per * per, rows_p, cw)


def pack_weights_fp8(w_oihw: torch.Tensor, cout_p: int, cin_p: int, exponent=None):
    """fp32 OIHW -> (uint8 e4m3 (nch, cout_p, 64) scaled by 2^e, e)."""
    w = w_oihw.detach().float().contiguous()
    if exponent is None:
        exponent = fp8_exponent(float(w.abs().max()), margin=0)
    out = torch.empty(fp8_weight_shape(w.shape[2], cin_p, cout_p), dtype=torch.uint8, device=w.device)
    _ops().pack_weights_fp8(w, out, float(2.0 ** exponent), None)
    return out, exponent


def pack_weights_fp8_into(w_oihw: torch.Tensor, out: torch.Tensor, scale_dev: torch.Tensor, transposed: bool = False):
    """Re-pack into an existing buffer with a device-resident scale (no host sync); ``transposed``:
    the dgrad weights (rows = input channels, chunks over output channels, taps flipped)."""
    _ops().pack_weights_fp8(w_oihw, out, 1.0, scale_dev, transposed)


def pack_weights_fp8_multi(ws, outs, scales_dev: torch.Tensor, layer, transposed):
    """Every fp8 weight pack of a repack in ONE launch: job i packs ws[i] into outs[i] with the device
    scale scales_dev[layer[i]]; transposed[i] selects the dgrad layout (rows = input channels,
    taps flipped)."""
    ws, outs, layer, transposed = list(ws), list(outs), [int(x) for x in layer], [int(bool(x)) for x in transposed]
    for i in range(0, len(ws), FP8_PACK_MAX_JOBS):  # the kernel's job table holds 48 entries
        j = i + FP8_PACK_MAX_JOBS
        _ops().pack_weights_fp8_multi(ws[i:j], outs[i:j], scales_dev, layer[i:j], transposed[i:j])


FP8_PACK_MAX_JOBS = 48  # kMaxFp8PackJobs (csrc/kernels/ops.cpp)


def conv_dgrad_bits_bf8(dz, wd, dx, mbits, dx8, scale, K: int, S: int, amax=None, tile: int = 0):
    """Bitmask dgrad (conv_fwd mode 3) that also writes dx8 = e5m2(dx * scale[0]) for the fp8 wgrad
    and folds max |dx| into ``amax`` (int32[64] float bits: the next step's delayed scale)."""
    _ops().conv_dgrad_bits_bf8(dz, wd, dx, mbits, dx8, scale, amax, K, S, tile)


def conv_wgrad_fp8(x8, dz8, slab, dbslab, xscale, gscale, gmul, K: int, S: int, Pin: int, Po: int = 1, amax=None):
    """fp8 weight gradient of a 160 -> 160 (value trunk) or 192 -> 192 (policy trunk) 3x3 layer
    (conv_wgrad_fp8.hip): e4m3 x8 (E8M0 exponent xscale[0]) x e5m2 dz8 (gscale[0]; gmul[0] = its 2^e
    multiplier, undone in the bias sums) into the same split slab as conv_wgrad, (nsplit, 9, C, C) with
    nsplit from ``wgrad_fp8_nsplit(M, width=C)``; reduce with conv_wgrad_reduce.  ``amax`` (int32[64]):
    max |dZ| from the e5m2 bytes (the next step's delayed scale).  Other shapes raise."""
    _ops().conv_wgrad_fp8(x8, dz8, slab, dbslab, xscale, gscale, gmul, K, S, Pin, Po, amax)


def wgrad_fp8_supported(cout_p: int, cin_p: int, K: int) -> bool:
    """Shapes the fp8 wgrad kernel covers: square 3x3 layers at the padded widths 160 (value trunk)
    and 192 (policy trunk); the same rule as the C++ ``wgrad_fp8_supported``."""
    return cout_p in (160, 192) and cin_p == cout_p and K == 3


def wgrad_fp8_tiles(width: int = 160) -> int:
    """Workgroups per (split, tap) of the fp8 wgrad: one 160 x 160 tile, or two 192 (n) x 96 (c) tiles."""
    return 2 if width == 192 else 1


def wgrad_fp8_nsplit(M: int, K: int = 3, target_wgs: int = 512, width: int = 160) -> int:
    """Pixel splits of the fp8 wgrad (128-pixel steps; per tap and split one 160 x 160 tile, or at
    ``width`` 192 two 192 x 96 tiles; two workgroups per CU either way): the grid
    nsplit x K*K x tiles stays within one resident round of ``target_wgs`` workgroups."""
    nks = (M + 127) // 128
    return max(1, min(target_wgs // (K * K * wgrad_fp8_tiles(width)), nks))


def wino_pack_weights(w_oihw: torch.Tensor) -> torch.Tensor:
    """Kernel-lab Winograd F(2x2, 3x3) weights (winograd.hip): U = G g G^T per (cout, cin), bf16,
    packed [16 xi][Cin/32][Cout/16][64 lanes][8] so that one MFMA B fragment is one 16-B load per
    lane (lane -> cout 16 nb + lane % 16, cin 32 ks + 8 (lane // 16) + e)."""
    w = w_oihw.detach().float()
    cout, cin = w.shape[:2]
    g = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], device=w.device)
    u = torch.einsum("ik,nckl,jl->ijnc", g, w, g).reshape(16, cout, cin)
    u = u.reshape(16, cout // 16, 16, cin // 32, 4, 8).permute(0, 3, 1, 4, 2, 5)
    return u.contiguous().to(torch.bfloat16)


def absmax_bf16(x, amax):
    """max |x| of a bf16 tensor folded into fp8 amax slots (int32 float bits, per-slot atomicMax)."""
    _ops().absmax_bf16(x, amax, amax.view(torch.float32))


def conv_dgrad_fp8(dz8, w8t, mask, scales, out_scale, K: int, S: int, y_bf16, y_fp8=None, amax=None):
    """fp8 dgrad: dx = conv(dz8 (e5m2, E8M0 scale scales[0]), w8t (transposed e4m3, scales[1]))
    masked by mask > 0 (bf16 activation of the layer below); bf16 y_bf16 and optional e5m2
    y_fp8 (x out_scale); amax accumulates max |dx|."""
    _ops().conv_dgrad_fp8(dz8, w8t, mask, scales, out_scale, amax, y_bf16, y_fp8, K, S)


def conv_dgrad_fp8_bits(dz8, w8t, mbits, scales, out_scale, K: int, S: int, y_bf16=None, y_fp8=None, amax=None,
                        res=None):
    """fp8 dgrad of the all-fp8 backward (160 channels: value trunk; 192: policy trunk): dz8 e5m2 (the
    copy the previous dgrad wrote for the fp8 wgrad; MFMA scale scales[0]) x the transposed flipped
    e4m3 weights (scales[1]), ReLU' from the forward's bitmask ``mbits``; writes y_fp8 =
    e5m2(dx * out_scale[0]) and/or bf16 y_bf16; ``amax`` accumulates max |dx|.  Other widths raise.
    ``res`` (192 wide, with y_bf16; bf16 of y_bf16's shape, not an output): the skip gradient of a residual
    block in real units, dx = bit ? acc + res : 0."""
    _ops().conv_dgrad_fp8_bits(dz8, w8t, mbits, scales, out_scale, amax, y_bf16, y_fp8, K, S, res)


def conv_dgrad_fp8_bf16(dz, w8t, mbits, scales, in_scale, K: int, S: int, dx, amax=None):
    """fp8 dgrad straight from the bf16 gradient: dz (padded NHWC bf16) is converted to e5m2 in
    registers as the kernel loads it (multiplier in_scale[0], MFMA E8M0 scale scales[0]), times the
    transposed flipped e4m3 weights (scales[1]); ReLU' from the forward's bitmask ``mbits``; bf16 dx;
    ``amax`` accumulates max |dx| (the next layer's gradient scale)."""
    _ops().conv_dgrad_fp8_bf16(dz, w8t, mbits, scales, in_scale, amax, dx, K, S)


def fp8_grad_scales(amax, gscales8, gosc, margin: int = 1):
    """Delayed e5m2 gradient scaling: gosc[l] = 2^e, gscales8[l, 0] = 127 - e from amax[l] (cleared),
    e = clamp(floor(log2(57344 / amax)) - margin, -100, 100).  amax 0 gives e = 0; an infinite amax
    yields the smallest multiplier, e = -100."""
    _ops().fp8_grad_scales(amax, gscales8, gosc, margin)


def quantize_bf8(x_bf16: torch.Tensor, out: torch.Tensor, scale_dev: torch.Tensor, amax: torch.Tensor):
    """e5m2 quantisation (x * scale_dev[0]) with max |x| accumulated into amax (int32[64])."""
    _ops().quantize_bf8(x_bf16, out, scale_dev, amax)
    return out


def quantize_fp8_dev(x_bf16: torch.Tensor, out: torch.Tensor, scale_dev: torch.Tensor, amax: torch.Tensor):
    """e4m3 quantisation (x * scale_dev[0]) with max |x| accumulated into amax (int32[64]): a bf16 layer's
    output as the next fp8 layer's input in the mixed-precision fp8 step."""
    _ops().quantize_fp8_dev(x_bf16, out, scale_dev, amax)
    return out


def bf8_to_float(t_u8: torch.Tensor, exponent: int = 0) -> torch.Tensor:
    """Decode e5m2 bytes (and undo a 2^exponent scale)."""
    return t_u8.view(torch.float8_e5m2).float() * (2.0 ** -exponent)


def fp8_weight_scales(ws, wscale, scales8):
    """Per-layer e4m3 weight exponents on the device: wscale[l] = 2^e_l, scales8[l, 1] = 127 - e_l."""
    _ops().fp8_weight_scales(list(ws), wscale, scales8)


def fp8_act_scales(amax, scales8, osc, margin: int = 1, max_drop: int = 0):
    """Delayed activation scaling from the per-layer output amax (also clears amax).  ``max_drop`` > 0:
    underflow guard -- each layer's exponent falls by at most that many binades per step (outliers of a
    sudden amax rise saturate instead of flushing the bulk of the activations to zero).
    e = clamp(floor(log2(448 / amax)) - margin, -60, 60) for the input of layer l + 1 (osc[l] = 2^e,
    scales8[l + 1, 0] = 127 - e); amax 0 gives e = 0.  An infinite amax (a bf16 overflow) yields the
    smallest multiplier, e = -60, and the guard applies to it as to any other falling exponent."""
    _ops().fp8_act_scales(amax, scales8, osc, margin, max_drop)


def quantize_fp8(x_bf16: torch.Tensor, out: torch.Tensor, exponent: int):
    _ops().quantize_fp8(x_bf16, out, float(2.0 ** exponent))
    return out


def conv_fwd_fp8(x8, w8, bias, scales, out_scale, K: int, S: int, Pin: int, Po: int = 1, y_bf16=None, y_fp8=None,
                 amax=None, mbits=None, sr_seed=None, res=None):
    """fp8 conv + bias + ReLU.  scales: int32 device tensor {127 - e_x, 127 - e_w} (MFMA E8M0);
    out_scale: f32 device tensor [2^e_y] for the e4m3 output; amax: int32[64] running max slots (float bits);
    sr_seed: int32 device scalar -> the e4m3 output is stochastically rounded (training forward);
    res (Cout 192, with y_bf16; bf16 of y_bf16's shape, not an output): the skip operand of a residual block
    in real units, y = relu(acc + bias + res), and every output follows the sum."""
    _ops().conv_fwd_fp8(x8, w8, bias, scales, out_scale, amax, y_bf16, y_fp8, K, S, Pin, Po, mbits, sr_seed, res)


def fp8_to_float(t_u8: torch.Tensor, exponent: int = 0) -> torch.Tensor:
    """Decode e4m3 bytes (and undo a 2^exponent scale)."""
    return t_u8.view(torch.float8_e4m3fn).float() * (2.0 ** -exponent)
