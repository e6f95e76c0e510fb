"""Training-step engines for the policy network.

``HipPolicyTrainer`` is the MI355X path.  One SL step (reference:
supervised_policy_trainer.py:199-213, Keras ``train_on_batch`` + SGD) is a
fixed sequence of hand-written kernels over preallocated buffers:

  pack_input (uint8 planes -> padded NHWC bf16, per-board D4 symmetry, targets)
  L x conv_fwd (implicit GEMM on MFMA, fused bias+ReLU)
  policy_head (1x1 conv + softmax + clipped CE + top-1 + head backward)
  for l = L..1:
     conv_wgrad(l) -> split slab -> reduce into the flat fp32 grad
        -> async RCCL all-reduce of the bucket once complete (RCCL's own stream)
     conv_fwd in dgrad mode (flipped weights, ReLU' mask fused)
  sgd (flat fp32 master) + pack_weights (bf16 forward and dgrad copies)

The gradient all-reduce of a bucket overlaps the remaining backward.  dgrad
and wgrad of a layer are independent; ``overlap=True`` runs the wgrad on a
second HIP stream, but on MI355X the two big-LDS kernels then split the CUs
and the step is slower (alternating A/B, scripts/overlap_ab.sh: SL 118.7k vs
120.3k, value 131.2k vs 136.8k positions/s), so large batches run serial.  For
B = 8 .. 256 (``overlap=None``, the default) the kernels leave CUs idle and the overlap wins
(SL B = 16 19.6k -> 22.3k positions/s, round 4).  Every
activation and gradient has its own buffer (HBM is plentiful: ~2 GB at
batch 512), so there are no cross-stream reuse hazards.

``TorchPolicyTrainer`` is the same step with torch autograd (fp32 numerics
oracle; CPU path for tests and the "32-filter 2-layer on CPU" config).
"""
from __future__ import annotations

import os
import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from .. import ops
from ..utils.profiling import trace_range
from ..models.nets import PolicyNet, ValueNet, first_argmax  # noqa: F401 - first_argmax: its users import it from here
from ..parallel import dist as agdist

# The 8 D4 symmetries as flat-index permutations (numpy semantics of the
# reference BOARD_TRANSFORMATIONS, supervised_policy_trainer.py:71-80).
_SYM_FWD = [
    lambda n, x, y: (x, y),
    lambda n, x, y: (n - 1 - y, x),
    lambda n, x, y: (n - 1 - x, n - 1 - y),
    lambda n, x, y: (y, n - 1 - x),
    lambda n, x, y: (x, n - 1 - y),
    lambda n, x, y: (n - 1 - x, y),
    lambda n, x, y: (y, x),
    lambda n, x, y: (n - 1 - y, n - 1 - x),
]


def symmetry_tables(n: int, device=None) -> torch.Tensor:
    """(8, n*n) long: fwd[s][p] = index of point p after symmetry s."""
    t = torch.empty(8, n * n, dtype=torch.long)
    for s, f in enumerate(_SYM_FWD):
        for x in range(n):
            for y in range(n):
                ox, oy = f(n, x, y)
                t[s, x * n + y] = ox * n + oy
    return t.to(device) if device is not None else t


def apply_symmetry(planes: torch.Tensor, targets: Optional[torch.Tensor], sym: torch.Tensor, table: torch.Tensor):
    """Torch implementation of the per-sample D4 augmentation (oracle for pack_input)."""
    B, C, S, _ = planes.shape
    fwd = table[sym.long()]  # (B, S*S)
    inv = torch.argsort(fwd, dim=1)
    flat = planes.reshape(B, C, S * S)
    out = torch.gather(flat, 2, inv.unsqueeze(1).expand(B, C, S * S)).reshape(B, C, S, S)
    tout = None
    if targets is not None:
        tl = targets.long()
        tout = torch.where(tl >= 0, torch.gather(fwd, 1, tl.clamp_min(0).unsqueeze(1)).squeeze(1), tl)
    return out, tout


def apply_symmetry_dist(dist: torch.Tensor, sym: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """A (B, T) target distribution moved with its board: the mass of point p goes to fwd[s][p], the
    rule ``apply_symmetry`` applies to an integer target (a one-hot row stays the one-hot of the
    transformed move).  T = S*S or S*S + 1; a trailing pass column stays where it is."""
    SS = table.shape[1]
    if dist.dim() != 2 or dist.shape[1] not in (SS, SS + 1):
        raise ValueError("target distribution must be (B, %d) or (B, %d)" % (SS, SS + 1))
    inv = torch.argsort(table[sym.long()], dim=1)  # inv[b][i] = the point that lands on i
    out = dist.clone()
    out[:, :SS] = torch.gather(dist[:, :SS], 1, inv)
    return out


_SOFT_REFUSED = ("soft (distribution) targets train the plain cross-entropy only: leave policy_loss at 'ce' and "
                 "ent_coef, kl_coef and collect_* off")


_SOFT_NO_GRAPH = ("soft (distribution) targets are not supported in graph mode: the captured SL step takes one "
                  "move per board")


def is_soft_target(targets: torch.Tensor) -> bool:
    """Floating (B, T) targets are per-board distributions (the soft-target head); integer targets
    are move indices."""
    return targets.is_floating_point() and targets.dim() == 2


def soft_target_loss(logits: torch.Tensor, dist: torch.Tensor):
    """The soft-target objective in torch ops (ops.policy_head_train_soft's): negatives clamped to
    0 (NaN too), a pass column dropped, the board part renormalised; per board (CE = -sum q log p,
    top-1 agreement, has-loss flag).  Both top-1 indices are the smallest among the maxima, the
    kernel's tie rule (visit counts tie often; torch.argmax promises no order).  Terms with q_i == 0
    add nothing, also where log p_i = -inf.  A row without board mass, or with an infinite entry,
    has no loss."""
    SS = logits.shape[1]
    q = dist[:, :SS].to(logits.dtype)
    q = torch.where(q > 0, q, torch.zeros_like(q))
    m = q.sum(1, keepdim=True)
    ok = (m > 0) & torch.isfinite(m)
    has = ok.squeeze(1)
    qh = torch.where(ok, q / torch.where(ok, m, torch.ones_like(m)), torch.zeros_like(q))
    logp = torch.log_softmax(logits, 1)
    ce = -torch.where(qh > 0, qh * logp, torch.zeros_like(logp)).sum(1)
    correct = ((first_argmax(logits) == first_argmax(q)) & has).float()
    return ce, correct, has


class FlatParams:
    """fp32 master parameters and gradients, each in ONE flat device buffer.

    Module parameters are re-bound to views of the flat buffer so the rest of
    PyTorch (save/load, eval) sees ordinary parameters."""

    def __init__(self, named: Sequence[Tuple[str, torch.nn.Parameter]], device):
        self.names = [n for n, _ in named]
        sizes = [p.numel() for _, p in named]
        total = (sum(sizes) + 3) // 4 * 4
        self.flat = torch.zeros(total, device=device, dtype=torch.float32)
        self.grad = torch.zeros(total, device=device, dtype=torch.float32)
        self.segments: Dict[str, Tuple[int, int]] = {}
        self.views: Dict[str, torch.Tensor] = {}
        self.grad_views: Dict[str, torch.Tensor] = {}
        off = 0
        for (name, p), n in zip(named, sizes):
            v = self.flat[off:off + n].view(p.shape)
            v.copy_(p.data.to(device))
            p.data = v
            self.segments[name] = (off, n)
            self.views[name] = v
            self.grad_views[name] = self.grad[off:off + n].view(p.shape)
            off += n
        self.numel = off


OPTIMIZERS = ("sgd", "momentum", "adam")


class KerasSGDSchedule:
    """Keras 1.0 optimizer step size: lr / (1 + decay * iterations) (``SGD(lr, decay)``, the reference's
    optimizer, supervised_policy_trainer.py:199).  ``optimizer="momentum"`` is Keras ``SGD(lr, momentum,
    decay, nesterov)``; ``"adam"`` is Keras ``Adam(lr, beta_1, beta_2, epsilon)``, whose step is the
    bias-corrected lr_t = lr sqrt(1 - beta_2^t) / (1 - beta_1^t), t = iterations + 1 (the decay factor
    applies to it as well; Keras 1.0 Adam has none, so keep decay 0 for parity)."""

    def __init__(self, lr: float, decay: float = 0.0, iterations: int = 0, optimizer: str = "sgd",
                 momentum: float = 0.0, nesterov: bool = False, beta_1: float = 0.9, beta_2: float = 0.999,
                 epsilon: float = 1e-8):
        if optimizer not in OPTIMIZERS:
            raise ValueError("optimizer must be one of %s" % (OPTIMIZERS,))
        if optimizer == "momentum" and not 0.0 <= momentum < 1.0:
            raise ValueError("momentum must be in [0, 1)")
        self.lr, self.decay, self.iterations = lr, decay, iterations
        self.optimizer, self.momentum, self.nesterov = optimizer, momentum, nesterov
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon

    @property
    def opt_code(self) -> int:
        return OPTIMIZERS.index(self.optimizer)

    @property
    def n_moments(self) -> int:
        """Flat fp32 state buffers the optimizer keeps (velocity; Adam's two moments)."""
        return {"sgd": 0, "momentum": 1, "adam": 2}[self.optimizer]

    def current(self) -> float:
        lr = self.lr / (1.0 + self.decay * self.iterations)
        if self.optimizer == "adam":
            t = self.iterations + 1.0
            lr = lr * math.sqrt(1.0 - math.pow(self.beta_2, t)) / (1.0 - math.pow(self.beta_1, t))
        return lr

    def advance(self) -> None:
        self.iterations += 1

    def kernel_kwargs(self) -> dict:
        """Optimizer arguments of ops.sgd_pack."""
        return dict(opt=self.opt_code, momentum=self.momentum, beta_1=self.beta_1, beta_2=self.beta_2,
                    epsilon=self.epsilon, nesterov=self.nesterov)


def optimizer_update_(p: torch.Tensor, g: torch.Tensor, state: List[torch.Tensor], sched: KerasSGDSchedule,
                      step: float) -> None:
    """The fused kernel's update (pack.hip opt_update) in torch fp32 ops, same operation order."""
    with torch.no_grad():
        if sched.optimizer == "sgd":
            p.sub_(g * step)
        elif sched.optimizer == "momentum":
            v = state[0]
            v.mul_(sched.momentum).sub_(g * step)
            if sched.nesterov:
                p.add_(v * sched.momentum - g * step)
            else:
                p.add_(v)
        else:
            m, v = state
            m.mul_(sched.beta_1).add_(g * (1.0 - sched.beta_1))
            v.mul_(sched.beta_2).add_(g * g * (1.0 - sched.beta_2))
            p.sub_(step * m / (v.sqrt() + sched.epsilon))


# automatic wgrad / dgrad stream overlap between these pixel counts per step (B = 17 .. 256 at 19 x 19;
# round 5: with the weight-stationary forward / dgrad at B <= 16 -- one 12-wave workgroup per CU -- the
# side-stream wgrad no longer finds idle CUs there: B = 8 12.1k overlapped vs 14.1k serial, B = 16 23.0k
# vs 23.4k; B = 32 40.0k vs 35.8k, profiles/r5/README.md)
OVERLAP_AUTO_MIN_PIXELS, OVERLAP_AUTO_MAX_PIXELS = 17 * 361, 256 * 361
# split-free wgrad (ops.conv_wgrad_direct) up to this many output pixels per step: per 192 -> 192 layer
# B = 1 7.8 vs 19.3 us (split-K + reduce), B = 4 16.9 vs 21.2, B = 8 27.1 vs 24.8, B = 16 48.6 vs 26.2
# (ksub 4; profiles/r6/raw/wgrad_direct_bench_v1.jsonl)
WGRAD_DIRECT_MAX_PIXELS = 4 * 361
# one merged split-K reduce launch per backward (HipConvTrainer merged_reduce) up to this many pixels
# off: slower at every batch measured (B = 16 / 32 / 64 / 128 / 2176: -4 / -10 / -4 / -7 / -0.6 %; the merged
# launch reads twelve cold slabs, profiles/r6/README.md); merged_reduce=True opts in
MERGED_REDUCE_MAX_PIXELS = 0


def _trunk_named(tr) -> List[Tuple[str, torch.nn.Parameter]]:
    """(name, parameter) of a ConvStack in flat-buffer order: w0, b0, w1, b1, ...  A trunk with pooling
    branches (gpool) has the gate of a branch block right after the bias of the block's last layer l,
    ``g<l>``: its gradient is complete when that layer's is, so it belongs to the layer's bucket segment."""
    named = [(n % l, p[l]) for l in range(tr.layers) for n, p in (("w%d", tr.weights), ("b%d", tr.biases))]
    for i, j in enumerate(getattr(tr, "gpool_blocks", ())):
        at = [n for n, _ in named].index("b%d" % (2 * j + 2)) + 1
        named.insert(at, ("g%d" % (2 * j + 2), tr.gpool_w[i]))
    return named


class _Layer(NamedTuple):
    """Shape of a trunk layer as the conv kernels take it (HipConvTrainer._layers; its input buffer and
    border: _layer_in)."""
    K: int         # kernel width
    cin_p: int     # padded input channels
    cin_real: int  # input planes the wgrad kernels read, 0 = all (only layer 0 has fewer than cin_p)


class HipConvTrainer:
    """MFMA conv-trunk training engine; subclasses provide the head."""

    def __init__(self, net, batch: int, lr: float = 0.003, decay: float = 0.0, device=None, bucket_mb: float = 4.0,
                 overlap: Optional[bool] = None, wgrad_target_wgs: int = 0, iterations: int = 0, precision: str = "bf16",
                 wgrad_priority: Optional[int] = None, conv_tile: int = 0, fp8_dgrad: Optional[bool] = None,
                 reduce_stream: Optional[bool] = None, wgrad_variant: Optional[int] = None,
                 fp8_wgrad: Optional[bool] = None, optimizer: str = "sgd", momentum: float = 0.0,
                 nesterov: bool = False, fp8_bf16_layers: Optional[Sequence[int]] = None,
                 wgrad_direct: Optional[bool] = None, wgrad_ksub: int = 4, fp8_scale_guard: int = 0,
                 merged_reduce: Optional[bool] = None):
        ops.load()
        self._rows = None  # pool rows of the current training forward (compute_grads(rows=...))
        # fp8 underflow guard: activation scale exponents fall by at most this many binades per step
        # (ops.fp8_act_scales max_drop; 0 = the plain one-step delayed scale, the default: SL at lr 0.05
        # over 5 seeds collapsed 3 times with a 1-binade guard vs once unguarded and once in bf16,
        # profiles/r6/README.md)
        self.fp8_scale_guard = int(fp8_scale_guard)
        # wgrad kernel: 0 = per-tap kernel (default), 5 = one-kernel-row wgrad (opt-in, slower so far)
        self.wgrad_variant = int(os.environ.get("ALPHAGO_AMD_WGRAD_VARIANT", "0")) if wgrad_variant is None \
            else int(wgrad_variant)
        self.conv_tile = conv_tile  # forward/dgrad tiling: 0 = automatic, or a production code (ops.conv_fwd)
        # kernel-lab A/B only: the 3x3 forwards and dgrads on a lab tiling of the lab library
        # (torch.ops.alphago_amd_lab), e.g. 5 = compact halo + ping-pong (profiles/r3_chunk_outer.md)
        self.lab_tile = int(os.environ.get("ALPHAGO_AMD_LAB_TILE", "0"))
        if precision not in ("bf16", "fp8"):
            raise ValueError("precision must be bf16 or fp8")
        self.precision = precision
        # global pooling branches (ConvStack gpool): after the first layer l of a branch block, gpool_fwd pools
        # Y[l], dense_f32 makes the gate g and gpool_bias_add writes R = Y[l-1] + g, which layer l + 1 takes as its
        # skip operand in Y[l-1]'s place; the backward mirrors it before wgrad(l + 1) (_gpool_backward).  bf16 only
        self.gpool_blocks = list(getattr(net.trunk, "gpool_blocks", ()))
        if self.gpool_blocks and precision == "fp8":
            raise ValueError("a trunk with global pooling branches (gpool=%d) trains in bf16 only: the fp8 trunk keeps "
                             "no bf16 output of a block's first layer to pool (precision=\"fp8\")" % net.trunk.gpool)
        if self.gpool_blocks and self.lab_tile:
            raise ValueError("a trunk with global pooling branches (gpool=%d) cannot run on a kernel-lab tiling: the "
                             "kernel-lab library has no skip operand (ALPHAGO_AMD_LAB_TILE=%d)"
                             % (net.trunk.gpool, self.lab_tile))
        # residual trunk (ConvStack residual=True): the skip-add is fused into the conv epilogues --
        # forward of an even layer l >= 2 adds Y[l-2], dgrad of an odd layer l adds DZ[l+1].  The fp8 kernels
        # take the skip on the 192-wide tile only; the residual stream (Y and DZ of the even layers) stays bf16
        self.residual = bool(getattr(net.trunk, "residual", False))
        if self.residual and precision == "fp8" and ops.pad_filters(net.trunk.filters) != 192:
            raise ValueError("a residual trunk of %d filters trains in bf16 only: the fp8 conv kernels have their "
                             "skip operand on the 192-wide tile alone (precision=\"fp8\")" % net.trunk.filters)
        if self.residual and self.lab_tile:
            raise ValueError("a residual trunk cannot run on a kernel-lab tiling: the kernel-lab library has no "
                             "skip operand (ALPHAGO_AMD_LAB_TILE=%d)" % self.lab_tile)
        self.env = agdist.env()
        self.device = torch.device(device) if device is not None else self.env.device
        if self.device.type != "cuda":
            raise RuntimeError("%s needs a GPU device" % type(self).__name__)
        self.net = net.to(self.device)
        self.batch = batch
        self.sched = KerasSGDSchedule(lr, decay, iterations, optimizer=optimizer, momentum=momentum,
                                      nesterov=nesterov)
        self.fp8_bf16_layers = frozenset(int(l) for l in (fp8_bf16_layers or ()))
        if reduce_stream is None:
            reduce_stream = os.environ.get("ALPHAGO_AMD_REDUCE_STREAM", "0") == "1"
        if overlap is None and reduce_stream:
            overlap = False  # an explicit reduce stream is a serial-backward mode: it wins over the auto overlap
        if overlap is None:
            # automatic: the wgrad on a side stream beside the dgrad at small batches, where both
            # kernels leave CUs idle -- SL B = 16 19.6k -> 22.3k, B = 256 95.3k -> 99.4k positions/s --
            # and serial from B = 512 on (108.8k vs 107.0k) and at the bench batch
            # (profiles/r4/raw/overlap_small_batch_ab.txt); ALPHAGO_AMD_OVERLAP=0 keeps it serial
            # Below B = 8 the steps are ~0.6 ms and the two-stream step measured mixed (B = 1 +8 %,
            # B = 2 -9 %, B = 4 -13..+2 %; raw/auto_overlap_splitk_batches.txt): serial there
            px = batch * net.board * net.board
            overlap = (precision == "bf16" and OVERLAP_AUTO_MIN_PIXELS <= px <= OVERLAP_AUTO_MAX_PIXELS
                       and os.environ.get("ALPHAGO_AMD_OVERLAP", "auto") != "0")
        self.overlap = overlap
        self.comm_events = None  # list: record the all-reduce wait of each backward as (start, end) events
        self._init_buffers(net)
        self._init_plans(wgrad_target_wgs, wgrad_direct, reduce_stream)
        self.wgrad_ksub = int(wgrad_ksub)
        self._init_streams(reduce_stream, wgrad_priority)
        self._init_buckets(bucket_mb, merged_reduce)
        self.fp8_wgrad = False
        self._w8layers = set()
        if precision == "fp8":
            self._init_fp8(fp8_dgrad, fp8_wgrad)
        # Keras-SGD schedule mirrored on the device (float64 {lr0, decay, iterations, lr}) so that
        # the SGD step reads its learning rate from memory: the whole step is graph-capturable
        self._sched_dev = torch.zeros(8, dtype=torch.float64, device=self.device)
        # fused SGD + bf16 packs (ops.sgd_pack); ALPHAGO_AMD_FUSED_UPDATE=0: sgd_update + pack_weights
        self._fused_update = os.environ.get("ALPHAGO_AMD_FUSED_UPDATE", "1") == "1"
        self._pack_plan = None
        self.enable_graphs(False)
        self._init_head()
        self.repack()

    def _init_buffers(self, net) -> None:
        """Trunk geometry, the flat master parameters, the weight packs and the activation buffers."""
        tr = net.trunk
        self.S = net.board
        self.L = tr.layers
        self.K = list(tr.widths)
        self.C0 = tr.in_planes
        self.C0p = ops.round_up(self.C0, 64)
        self.F = tr.filters
        # 152 filters (value net) run on 160-wide tiles, bf16 and fp8
        self.Fp = ops.pad_filters(self.F)
        if self.F > 256:
            raise ValueError("head kernels support up to 256 filters")
        self.P0 = self.K[0] // 2
        self._M = self.batch * self.S * self.S  # output pixels of a layer
        self._layers = [_Layer(self.K[0], self.C0p, self.C0)] + [_Layer(K, self.Fp, 0) for K in self.K[1:]]
        head = self._head_named_params()
        self.head_names = [n for n, _ in head]
        self.fp = FlatParams(_trunk_named(tr) + head, self.device)
        if self.env.distributed:
            agdist.broadcast_(self.fp.flat, 0)
        # optimizer state (momentum velocity / Adam moments), flat fp32 like the master weights
        self.opt_state = [torch.zeros_like(self.fp.flat) for _ in range(self.sched.n_moments)]
        dev, B, S = self.device, self.batch, self.S
        # unpadded filters: the kernels read the biases straight from the flat
        # master parameters (no per-step copies); padded: zero-tailed copies
        self._bias_alias = self.Fp == self.F
        self.bias_p = ([self.fp.views["b%d" % l] for l in range(self.L)] if self._bias_alias
                       else [torch.zeros(self.Fp, device=dev) for _ in range(self.L)])
        self.wf, self.wd = [], []
        for l, ly in enumerate(self._layers):
            w = self.fp.views["w%d" % l]
            self.wf.append(ops.packed_weight_like(w, ly.cin_p, self.Fp))
            self.wd.append(ops.packed_weight_like(w, ly.cin_p, self.Fp, transposed=True) if l > 0
                           else torch.empty(0, device=dev, dtype=torch.bfloat16))
        # activations / gradients (zero borders are never written)
        self.X0 = ops.padded_empty(B, S, self.P0, self.C0p, dev)
        self.Y = [ops.padded_empty(B, S, 1, self.Fp, dev) for _ in range(self.L)]
        self.DZ = [ops.padded_empty(B, S, 1, self.Fp, dev) for _ in range(self.L)]
        # ReLU' bitmasks of Y[0..L-2], written by the forward epilogue and read
        # by the dgrad epilogue instead of the bf16 activations (12x fewer bytes)
        hw = B * (S + 2) * (S + 2) * ops.mbits_words(self.Fp)
        self.MBITS = [torch.zeros(hw, dtype=torch.int32, device=dev) for _ in range(self.L - 1)]
        self.loss = torch.zeros(B, device=dev)
        self.correct = torch.zeros(B, device=dev)
        if self.gpool_blocks:
            self._init_gpool()

    def _init_gpool(self) -> None:
        """Buffers of the pooling branches.  Per branch block (keyed by its last layer l + 1): the pooled
        vector P and the argmax, kept for the backward.  Shared by all blocks: the gate g, the skip operand
        R = Y[l-1] + g (its gradient with respect to Y[l-1] is the identity, so the backward never reads it),
        and the backward's dg, dP and G2 (the pooling's gradient into Y[l], the skip operand of dgrad(l + 1)).
        Padded widths (F < Fp): the kernels see zero-padded (2 Fp, Fp) copies of the gates (rows F.. of each
        half and columns F.. stay zero, so padded channels get g = 0) and dWg lands in a padded scratch whose
        real blocks are copied into the flat gradient; unpadded, both are the flat views themselves."""
        dev, B, S, Fp, F = self.device, self.batch, self.S, self.Fp, self.F
        self._gp_layers = [2 * j + 2 for j in self.gpool_blocks]
        self._gp_P = {l: torch.zeros(B, 2, Fp, device=dev) for l in self._gp_layers}
        self._gp_arg = {l: torch.zeros(B, Fp, dtype=torch.int32, device=dev) for l in self._gp_layers}
        self._gp_g = torch.zeros(B, Fp, device=dev)
        self._gp_dg = torch.zeros(B, Fp, device=dev)
        self._gp_dP = torch.zeros(B, 2, Fp, device=dev)
        self._gp_R = ops.padded_empty(B, S, 1, Fp, dev)
        self._gp_G2 = ops.padded_empty(B, S, 1, Fp, dev)
        if self._bias_alias:
            self._gp_w = {l: self.fp.views["g%d" % l] for l in self._gp_layers}
            self._gp_dw = {l: self.fp.grad_views["g%d" % l] for l in self._gp_layers}
        else:
            self._gp_w = {l: torch.zeros(2 * Fp, Fp, device=dev) for l in self._gp_layers}
            self._gp_dw = {l: torch.zeros(2 * Fp, Fp, device=dev) for l in self._gp_layers}

    def _gpool_forward(self, l: int) -> torch.Tensor:
        """After layer l - 1, the first layer of a branch block ending at l: pool Y[l-1], gate, and the skip
        operand R = Y[l-2] + g of layer l."""
        S = self.S
        ops.gpool_fwd(self.Y[l - 1], self._gp_P[l], self._gp_arg[l], S)
        ops.dense_f32(self._gp_P[l].view(self.batch, -1), self._gp_w[l], self._gp_g)  # g = P Wg
        return ops.gpool_bias_add(self.Y[l - 2], self._gp_g, self._gp_R, S)

    def _gpool_backward(self, l: int) -> None:
        """Before wgrad(l) and dgrad(l) of a branch block's last layer l: dg = sum_p DZ[l], dWg = P^T dg into
        the flat gradient, dP = dg Wg^T, and G2 = the pooling's gradient into Y[l-1], which dgrad(l) adds
        before ReLU'.  All on the caller's stream, ahead of the event wgrad(l) waits on: dWg is complete
        when layer l's bucket is launched."""
        B, F, Fp = self.batch, self.F, self.Fp
        P = self._gp_P[l].view(B, -1)
        ops.gpool_fwd(self.DZ[l], self._gp_dg, None, self.S)
        ops.dense_f32(P, self._gp_dg, self._gp_dw[l], trans_a=True)  # dWg = P^T dg
        if not self._bias_alias:
            gv = self.fp.grad_views["g%d" % l]
            gv[:F].copy_(self._gp_dw[l][:F, :F])
            gv[F:].copy_(self._gp_dw[l][Fp:Fp + F, :F])
        ops.dense_f32(self._gp_dg, self._gp_w[l], self._gp_dP.view(B, -1), trans_b=True)  # dP = dg Wg^T
        ops.gpool_bwd_fill(self._gp_dP, self._gp_arg[l], self._gp_G2, self.S)

    def _init_plans(self, wgrad_target_wgs: int, wgrad_direct: Optional[bool], reduce_stream: bool) -> None:
        """Per-layer kernel choices (wgrad variant and split, forward / dgrad plans) and what they need."""
        M = self._M
        # one resident round of wgrad workgroups (the kernel's own occupancy, ops.wgrad_plan); small
        # batches: the LDS-ring variant with longer splits (ops.wgrad_config)
        cfg = [ops.wgrad_config(M, self.Fp, ly.cin_p, ly.K, ly.cin_real, wgrad_target_wgs, self._num_cus(),
                                self.wgrad_variant) for ly in self._layers]
        self.wgrad_var = [var for var, _ in cfg]
        self.nsplit = [ns for _, ns in cfg]
        # split-free wgrad (ops.conv_wgrad_direct: whole pixel range per workgroup, OIHW gradient written
        # in the kernel, no slab and no reduce launch); automatic up to WGRAD_DIRECT_MAX_PIXELS, off with
        # the reduce stream (its slabs are the point) and for kernel-lab wgrad variants
        if wgrad_direct is None:
            wgrad_direct = M <= WGRAD_DIRECT_MAX_PIXELS
        self.wgrad_direct = [bool(wgrad_direct) and not reduce_stream and self.wgrad_variant in (0, ops.WGRAD_SMALL)
                             and ops.wgrad_direct_supported(self.Fp, ly.cin_p, ly.cin_real or ly.cin_p, ly.K)
                             for ly in self._layers]
        # forward and bitmask dgrad (ops.plan_conv).  Small batches, bf16 path with the automatic tiling
        # only: the weight-stationary kernel (tile 40) where it applies, else (B <= 8, ops.SPLITK_MAX_M)
        # the split-K 32-pixel tile (ops.conv_fwd_splitk: the K loop of a tile over several workgroups,
        # one finishing pass)
        small = self.conv_tile == 0 and self.precision == "bf16" and not self.lab_tile
        self.fwd_plan = [ops.plan_conv(M, self.Fp, ly.cin_p, ly.K, training=True, tile=self.conv_tile, small=small)
                         for ly in self._layers]
        self.dg_plan = [None] + self.fwd_plan[1:]  # the dgrad of a layer >= 1 is a conv of its forward's shape
        # their weights in the weight-stationary order (ops.ws_pack after every update, repack())
        self.wf_ws = [ops.ws_packed_like(w) if p.kind == "ws" else None for w, p in zip(self.wf, self.fwd_plan)]
        self.wd_ws = [ops.ws_packed_like(w) if p is not None and p.kind == "ws" else None
                      for w, p in zip(self.wd, self.dg_plan)]
        n = ops.splitk_workspace_numel(self.fwd_plan + self.dg_plan, M, self.Fp)
        self._sk_ws = torch.empty(n, device=self.device) if n else None

    def _init_streams(self, reduce_stream: bool, wgrad_priority: Optional[int]) -> None:
        """The reduce and wgrad side streams and the wgrad split slabs."""
        # Split-K reduce on a side stream (serial backward only): the memory-bound reduce of
        # layer l runs beside dgrad(l) instead of between the two big conv kernels.  The
        # slabs are double-buffered by layer parity, so wgrad(l-1) never waits for
        # reduce(l); wgrad(l-2) waits for reduce(l) through an event.
        self.s_r = (torch.cuda.Stream(device=self.device, priority=-1) if reduce_stream and not self.overlap else None)
        nslab = 2 if self.s_r is not None else 1
        slab_max = max(ns * ly.K ** 2 * self.Fp * ly.cin_p for ns, ly in zip(self.nsplit, self._layers))
        self._slabs = [torch.empty(slab_max, device=self.device) for _ in range(nslab)]
        self._dbslabs = [torch.zeros(max(self.nsplit) * self.Fp, device=self.device) for _ in range(nslab)]
        self._slab_free = [None] * nslab  # event: the reduce that last read slab i has finished
        # wgrad stream at high priority (-1): its workgroups are dispatched ahead of the
        # concurrent dgrad's, so the wgrad/reduce/all-reduce chain of a layer finishes
        # earlier and less of it is left after the last dgrad (+0.9 % positions/s,
        # 3 alternating A/B pairs of 100 steps; ALPHAGO_AMD_WGRAD_PRIO=0 restores equal priority)
        if wgrad_priority is None:
            wgrad_priority = int(os.environ.get("ALPHAGO_AMD_WGRAD_PRIO", "-1"))
        self.s_w = torch.cuda.Stream(device=self.device, priority=wgrad_priority) if self.overlap else None

    def _init_buckets(self, bucket_mb: float, merged_reduce: Optional[bool]) -> None:
        """Gradient buckets and their all-reducer, and the merged split-K reduce."""
        # buckets over the flat grad, segments in backward order (head first)
        h0 = self.fp.segments[self.head_names[0]][0]
        h1 = sum(self.fp.segments[n][1] for n in self.head_names)
        segs = [(h0, h1)]
        self._seg_layer = [-1] + list(reversed(range(self.L)))  # -1: the head
        for l in reversed(range(self.L)):
            ow, nw = self.fp.segments["w%d" % l]
            _, nb = self.fp.segments["b%d" % l]
            ng = self.fp.segments["g%d" % l][1] if "g%d" % l in self.fp.segments else 0  # a branch block's gate
            segs.append((ow, nw + nb + ng))
        self.buckets = agdist.make_buckets(segs, int(bucket_mb * (1 << 20)), last_alone=True)
        self._bucket_after_layer = {self._seg_layer[ids[-1]]: bi for bi, (_, _, ids) in enumerate(self.buckets)}
        self.reducer = agdist.BucketAllReducer(self.fp.grad, self.buckets)
        # one-GPU contention proxy of the overlapped all-reduce (ALPHAGO_AMD_COMM_PROXY, world 1 only)
        self._proxy = agdist.CommProxy.from_env(self.fp.grad, self.buckets) if not self.env.distributed else None
        if self._proxy is not None:
            self.reducer = self._proxy
        # merged reduce (one process, small batches): every layer's wgrad keeps its own split slab and ONE
        # ops.conv_wgrad_reduce_multi launch after the backward sums them all (the same fixed order per
        # element as the per-layer reduce, so bitwise equal) instead of a reduce launch per layer.  Without
        # a gradient all-reduce to overlap nothing waits for an early reduce.
        if merged_reduce is None:
            merged_reduce = self._M <= MERGED_REDUCE_MAX_PIXELS
        self.merged_reduce = (bool(merged_reduce) and not self.env.distributed and self._proxy is None
                              and self.s_r is None and self.L <= 16)
        self._mslabs = [None] * self.L  # per-layer (slab, dbias slab), allocated at first use
        self._pending_reduce = []
        # ALPHAGO_AMD_DEFER_ALLREDUCE=1: launch every bucket after the backward instead of at its bucket
        # point (no overlap, no CU contention with the dgrad / wgrad kernels)
        self.defer_allreduce = os.environ.get("ALPHAGO_AMD_DEFER_ALLREDUCE", "0") == "1"

    def _init_fp8(self, fp8_dgrad: Optional[bool], fp8_wgrad: Optional[bool]) -> None:
        """Packs, scales and buffers of the fp8 trunk (precision "fp8")."""
        # fp8 forward (block-scaled MFMA) with bf16 activations kept for the
        # backward; per-tensor power-of-two scales, all device-side:
        # weights from their amax at every repack, activations delayed by
        # one step from the amax the fp8 kernels accumulate.
        dev, L = self.device, self.L
        self.w8 = [torch.zeros(ops.fp8_weight_shape(ly.K, ly.cin_p, self.Fp), dtype=torch.uint8, device=dev)
                   for ly in self._layers]
        self.wscale8 = torch.ones(L, device=dev)
        self.scales8 = torch.full((L, 2), 127, dtype=torch.int32, device=dev)
        # this step's activation exponents, kept for the fp8 wgrad: X8[l] was quantised with
        # them, while scales8[:, 0] already holds the next step's delayed exponents by then
        self.xscale8 = torch.full((L, 1), 127, dtype=torch.int32, device=dev)
        self.osc8 = torch.ones(L, device=dev)
        self.amax8 = ops.fp8_amax_buffer(L, dev)
        # ALPHAGO_AMD_FP8_SR=1: the training forward rounds its e4m3 activations stochastically
        # (v_cvt_sr_fp8_f32; a device seed advanced every step); evaluation keeps round-to-nearest
        self.fp8_sr = os.environ.get("ALPHAGO_AMD_FP8_SR", "0") == "1"
        self._sr_seed = torch.zeros(1, dtype=torch.int32, device=dev)
        self._train_fwd = False
        self.X08 = torch.zeros(self.X0.shape, dtype=torch.uint8, device=dev)
        self.Y8 = [torch.zeros(self.Y[0].shape, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._fp8_calibrated = False
        # fp8 dgrad (opt-in): e5m2 gradients x transposed e4m3 weights; per-layer delayed
        # gradient scales from the max |dZ| of the previous step (the first step runs bf16
        # dgrads and calibrates them).  Round 3: the kernel reads the bf16 dZ and converts it to
        # e5m2 in registers (no quantisation pass, no e5m2 tensor), takes ReLU' from the
        # forward's bitmask, and the transposed packs ride the one batched repack launch.
        self.wd8 = [None] + [torch.zeros(ops.fp8_weight_shape(self.K[l], self.Fp, self.Fp), dtype=torch.uint8,
                                         device=dev) for l in range(1, L)]
        self.gscales8 = torch.full((L, 2), 127, dtype=torch.int32, device=dev)
        self.gosc8 = torch.ones(L, device=dev)
        self.gamax8 = ops.fp8_amax_buffer(L, dev)
        self._g8_calibrated = False
        # fp8 wgrad (160 -> 160 and 192 -> 192 3x3 layers, conv_wgrad_fp8.hip): e4m3 inputs kept per
        # layer (the forward's e4m3 outputs instead of a two-buffer ring), e5m2 output gradients
        # written by the bitmask dgrad's epilogue (the head's by one quantise pass), delayed gradient
        # scales as the fp8 dgrad's.  Layer 0 (48 / 49 planes) keeps the bf16 wgrad.  On by default
        # on the 160-wide value trunk (143 vs 201 us per layer at B = 1024, profiles/r3_fp8_wgrad.md);
        # ALPHAGO_AMD_FP8_WGRAD=0 keeps the bf16 wgrad there.  At 192 (policy trunk) it is opt-in:
        # only an explicit fp8_wgrad=True turns it on, whatever the environment says, so the
        # default fp8 policy step keeps its bf16 backward (profiles/r9/README.md).
        if fp8_wgrad is None:
            fp8_wgrad = self.Fp == 160 and os.environ.get("ALPHAGO_AMD_FP8_WGRAD", "1") == "1"
        self.fp8_wgrad = bool(fp8_wgrad) and all(
            ops.wgrad_fp8_supported(self.Fp, self.Fp, self.K[l]) for l in range(1, L))
        # per-layer precision: the layers in fp8_bf16_layers run their forward, dgrad and wgrad in bf16
        # (their weights are never quantised); the others stay on the fp8 kernels
        self._w8layers = (set(range(1, L)) - self.fp8_bf16_layers) if self.fp8_wgrad else set()
        # With the fp8 wgrad the dgrad reads the same e5m2 dZ copy and writes e5m2 for the layer
        # below (conv_dgrad_fp8_bits): the all-fp8 backward is the default there (value 12 x 152,
        # B = 1024: 156.3k -> 179.9k positions/s, profiles/r3_fp8_wgrad.md);
        # ALPHAGO_AMD_FP8_DGRAD=0 keeps the bf16 dgrad.  Elsewhere (the 192-wide policy trunk
        # included) fp8 dgrad stays opt-in: fp8_dgrad=True next to fp8_wgrad=True is the all-fp8 backward.
        if fp8_dgrad is None:
            fp8_dgrad = self.fp8_wgrad and self.Fp == 160 and os.environ.get("ALPHAGO_AMD_FP8_DGRAD", "1") == "1"
        self.fp8_dgrad = bool(fp8_dgrad)
        if self.residual and (self.fp8_dgrad != self.fp8_wgrad or self.fp8_bf16_layers):
            # conv_dgrad_bits_bf8 and conv_dgrad_fp8_bf16 (the mixed arms and the per-layer bf16 fallback) have no
            # skip operand
            raise ValueError("a residual fp8 trunk has two backward arms: the bf16 backward (fp8_dgrad=False, "
                             "fp8_wgrad=False, the default) and the all-fp8 backward (fp8_dgrad=True, "
                             "fp8_wgrad=True), both without fp8_bf16_layers; got fp8_dgrad=%s, fp8_wgrad=%s, "
                             "fp8_bf16_layers=%s" % (self.fp8_dgrad, self.fp8_wgrad, sorted(self.fp8_bf16_layers)))
        if self.fp8_wgrad:
            self.X8 = [None] + [torch.zeros(self.Y[0].shape, dtype=torch.uint8, device=dev) for _ in range(1, L)]
            self.DZ8 = [None] + [torch.zeros(self.DZ[0].shape, dtype=torch.uint8, device=dev) for _ in range(1, L)]
            self.nsplit8 = ops.wgrad_fp8_nsplit(self._M, 3, width=self.Fp)
            need = self.nsplit8 * 9 * self.Fp * self.Fp
            if need > self._slabs[0].numel():
                self._slabs = [torch.empty(need, device=dev) for _ in self._slabs]
            if self.nsplit8 * self.Fp > self._dbslabs[0].numel():
                self._dbslabs = [torch.zeros(self.nsplit8 * self.Fp, device=dev) for _ in self._dbslabs]

    # ------------------------------------------------------------------ schedule / graphs
    def sync_schedule(self) -> None:
        """Copy the host schedule (lr, decay, iterations) to the device copy used by graph replays."""
        sc = self.sched
        self._sched_dev.copy_(torch.tensor([sc.lr, sc.decay, float(sc.iterations), 0.0, sc.beta_1, sc.beta_2,
                                            float(sc.opt_code), 0.0], dtype=torch.float64))

    def enable_graphs(self, on: bool = True) -> None:
        """Run ``step`` as HIP-graph replays (bf16, per-board weights not supported): the first
        call runs eagerly (loads code objects, sets kernel attributes), the second captures
        the step -- pack, forward, head, backward (wgrad on its stream), SGD, repack -- and
        every call replays it.  With world > 1 the gradient all-reduce runs eagerly between a
        forward/backward graph and an update graph.  Replays are bitwise identical to eager steps.
        The learning-rate schedule is read from its device copy (synced from ``self.sched`` at
        capture); changing ``sched.lr`` afterwards needs ``sync_schedule()``."""
        if on and self.precision != "bf16":
            raise ValueError("graph-captured steps support the bf16 trainer only")
        self.use_graph = on
        self._graphs = None
        self._g_in = None
        self._graph_warm = False
        if on:
            self.sync_schedule()

    # ------------------------------------------------------------------ head API
    def _head_named_params(self):
        raise NotImplementedError

    def _init_head(self):
        pass

    def _head_train(self, targets, gscale: float, weight, sym=None) -> None:
        """Head forward + backward into dZ[L-1] and the head gradient; ``sym`` is the forward's."""
        raise NotImplementedError

    # ------------------------------------------------------------------ helpers
    def repack(self, bf16: bool = True) -> None:
        """Device copies of the master weights the kernels read: padded biases, the bf16 packs (unless
        the fused update already wrote them: ``bf16=False``) and the fp8 packs."""
        if not self._bias_alias:
            torch._foreach_copy_([b[:self.F] for b in self.bias_p], [self.fp.views["b%d" % l] for l in range(self.L)])
            for l in (self._gp_layers if self.gpool_blocks else ()):  # the gates' zero-padded copies
                g = self.fp.views["g%d" % l]
                self._gp_w[l][:self.F, :self.F].copy_(g[:self.F])
                self._gp_w[l][self.Fp:self.Fp + self.F, :self.F].copy_(g[self.F:])
        ws = [self.fp.views["w%d" % l] for l in range(self.L)]
        if bf16:
            ops.pack_weights(ws, self.wf, self.wd)
        # the weight-stationary copies of the small-batch layers (from the bf16 packs, however written)
        pairs = [(w, c) for w, c in zip(self.wf + self.wd, self.wf_ws + self.wd_ws) if c is not None]
        ops.ws_pack([w for w, _ in pairs], [c for _, c in pairs])
        if self.precision == "fp8":
            ops.fp8_weight_scales(ws, self.wscale8, self.scales8)
            # every e4m3 pack of the step (forward, and the transposed dgrad packs) in ONE launch
            # (round 2: 12 + 11 launches of pack_weights_fp8 per step)
            dg = list(range(1, self.L)) if self.fp8_dgrad else []
            ops.pack_weights_fp8_multi([ws[l] for l in range(self.L)] + [ws[l] for l in dg],
                                       self.w8 + [self.wd8[l] for l in dg], self.wscale8,
                                       list(range(self.L)) + dg, [0] * self.L + [1] * len(dg))
            if self.fp8_dgrad:
                self.gscales8[:, 1].copy_(self.scales8[:, 1])

    _head_wrote_e5m2 = False  # this step's head wrote DZ8[L-1] (and its amax) instead of the bf16 DZ[L-1]

    def _top_e5m2_fusable(self) -> bool:
        """The fp8 backward reads only the e5m2 copy of the head's dZ (fp8 wgrad and dgrad of the top
        layer, scales calibrated), so a head can write that copy directly."""
        return (self.precision == "fp8" and self.fp8_wgrad and self.fp8_dgrad and self._g8_calibrated
                and (self.L - 1) in self._w8layers and not self.residual)  # residual: dZ[L-1] is a bf16 skip too

    def _layer_in(self, l):
        return (self.X0, self.P0) if l == 0 else (self.Y[l - 1], 1)

    def forward_trunk(self, planes: torch.Tensor, sym=None, move_targets=None, target_out=None) -> None:
        # fp8 trunk: the pack writes the e4m3 input copy too (was a quantize_fp8 pass over X0)
        ops.pack_input(planes, self.X0, self.P0, sym=sym, target=move_targets, target_out=target_out,
                       rows=self._rows, out8=self.X08 if self.precision == "fp8" else None)
        if self.precision == "fp8":
            if not self._fp8_calibrated:
                self._fp8_calibrate()
            self._forward_fp8()
            return
        for l in range(self.L):
            self._fwd_layer(l, self.MBITS[l] if l < self.L - 1 else None)

    def _fwd_layer(self, l: int, mbits=None) -> None:
        """bf16 forward of layer l into Y[l]."""
        x, pin = self._layer_in(l)
        if self.lab_tile and self.K[l] == 3:
            ops.lab().conv_fwd(x, self.wf[l], self.bias_p[l], None, self.Y[l], 3, self.S, pin, 1, 0, mbits,
                               self.lab_tile)
        else:
            # residual trunk: a block's last layer adds the block's input before its ReLU
            res = self.Y[l - 2] if self.residual and l >= 2 and l % 2 == 0 else None
            if res is not None and self.gpool_blocks and l in self._gp_layers:
                res = self._gpool_forward(l)
            ops.conv_planned(self.fwd_plan[l], x, self.wf[l], self.wf_ws[l], self.bias_p[l], self.Y[l], self.K[l],
                             self.S, pin, ops.MODE_BIAS_RELU, mbits, self._sk_ws, res=res)

    def _forward_fp8(self) -> None:
        x8, pin = self.X08, self.P0  # e4m3 input written by forward_trunk's pack_input (exact: 0/1 planes)
        # all-fp8 backward (fp8 wgrad + dgrad): below the last layer nothing reads the bf16
        # activations (wgrad reads the e4m3 copies, dgrad the ReLU' bits), so only e4m3 is written
        # (the first, calibrating backward runs bf16 wgrads on these activations)
        e4m3_only = self.fp8_wgrad and self.fp8_dgrad and self._g8_calibrated
        sr = self._sr_seed if (self.fp8_sr and self._train_fwd) else None
        bfl = self.fp8_bf16_layers
        for l in range(self.L):
            last = l == self.L - 1
            nxt_bf = l + 1 in bfl  # the next layer reads this output in bf16
            y8 = None if (last or nxt_bf) else (self.X8[l + 1] if self.fp8_wgrad else self.Y8[l % 2])
            if l in bfl:  # bf16 layer: bf16 conv, then the e4m3 copy the next (fp8) layer reads
                self._fwd_layer(l, None if last else self.MBITS[l])
                if y8 is not None:
                    ops.quantize_fp8_dev(self.Y[l], y8, self.osc8[l:l + 1], self.amax8[l])
            else:
                # residual trunk: the stream (the stem's and every block end's output) is kept in bf16 next to
                # its e4m3 copy, and a block end adds the stream of two layers below before its ReLU
                stream = self.residual and l % 2 == 0
                keep_bf16 = last or nxt_bf or not e4m3_only or stream
                ops.conv_fwd_fp8(x8, self.w8[l], self.bias_p[l], self.scales8[l], self.osc8[l:l + 1], self.K[l],
                                 self.S, pin, 1, y_bf16=self.Y[l] if keep_bf16 else None, y_fp8=y8,
                                 amax=self.amax8[l], mbits=None if last else self.MBITS[l], sr_seed=sr,
                                 res=self.Y[l - 2] if stream and l >= 2 else None)
            x8, pin = y8, 1
        if sr is not None:
            self._sr_seed.add_(1)
        if self.fp8_wgrad:
            self.xscale8.copy_(self.scales8[:, 0:1])
        ops.fp8_act_scales(self.amax8, self.scales8, self.osc8, 1, self.fp8_scale_guard)  # next step's scales

    @torch.no_grad()
    def _fp8_calibrate(self) -> None:
        """First step: activation scales from a bf16 forward of this batch."""
        amax = []
        for l in range(self.L):
            self._fwd_layer(l)
            amax.append(self.Y[l].amax().float())
        self.amax8.zero_()
        self.amax8[:, 0].copy_(torch.stack(amax).view(torch.int32))
        ops.fp8_act_scales(self.amax8, self.scales8, self.osc8, 1)
        self._fp8_calibrated = True

    def _num_cus(self) -> int:
        try:
            return int(torch.cuda.get_device_properties(self.device).multi_processor_count)
        except Exception:  # noqa: BLE001 - a query failure keeps the MI355X default
            return 256

    def _wgrad_layer(self, l: int, red: bool = False) -> None:
        """wgrad(l) into a split slab, then the deterministic reduce into the flat grad (and
        the async all-reduce of a completed bucket when ``red``).  With the reduce stream the
        reduce and the all-reduce launch run there; the caller's stream goes on to dgrad(l)."""
        x, pin = self._layer_in(l)
        ly = self._layers[l]
        f8 = l in self._w8layers and self._g8_calibrated
        direct = self.wgrad_direct[l] and not f8
        merged = self.merged_reduce and not direct
        ns = self.nsplit8 if f8 else self.nsplit[l]
        nw, nb = ns * ly.K ** 2 * self.Fp * ly.cin_p, ns * self.Fp
        i = l % len(self._slabs)
        sl, db = self._slabs[i], self._dbslabs[i]
        if merged:  # this layer's own slab; the reduce waits for the merged launch after the backward
            if self._mslabs[l] is None or self._mslabs[l][0].numel() < nw:
                self._mslabs[l] = (torch.empty(nw, device=self.device), torch.zeros(nb, device=self.device))
            sl, db = self._mslabs[l]
        slab = sl[:nw].view(ns, ly.K ** 2, self.Fp, ly.cin_p)
        dbs = db[:nb].view(ns, self.Fp)
        gw, gb = self.fp.grad_views["w%d" % l], self.fp.grad_views["b%d" % l]
        sr = self.s_r
        if sr is not None and self._slab_free[i] is not None:
            torch.cuda.current_stream(self.device).wait_event(self._slab_free[i])
        if f8:  # e5m2 dZ x e4m3 X, dequantised by the MFMA's block scales
            # (its tap-0 workgroups also fold max |dZ| into the delayed-scale slots of layer l)
            ops.conv_wgrad_fp8(self.X8[l], self.DZ8[l], slab, dbs, self.xscale8[l], self.gscales8[l, 0:1],
                               self.gosc8[l:l + 1], ly.K, self.S, pin, 1,
                               amax=self.gamax8[l] if l < self.L - 1 else None)
        elif direct:  # split-free: the OIHW gradient straight from the kernel
            ops.conv_wgrad_direct(x, self.DZ[l], gw, gb, ly.K, self.S, pin, 1, 1.0, 0.0, self.wgrad_ksub)
        else:
            ops.conv_wgrad(x, self.DZ[l], slab, dbs, ly.K, self.S, pin, 1, cin_real=ly.cin_real,
                           variant=self.wgrad_var[l])
        if direct:
            self._launch_bucket_after(l, red)
        elif merged:
            self._pending_reduce.append((slab, dbs, l))
        elif sr is None:
            ops.conv_wgrad_reduce(slab, dbs, gw, gb, 1.0, 0.0)
            self._launch_bucket_after(l, red)
        else:
            sr.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(sr):
                ops.conv_wgrad_reduce(slab, dbs, gw, gb, 1.0, 0.0)
                self._launch_bucket_after(l, red)
                self._slab_free[i] = sr.record_event()

    def _launch_bucket_after(self, l: int, red: bool) -> None:
        """Start the all-reduce of the bucket that layer l's gradient completes (-1: the head's)."""
        if red and not self.defer_allreduce and l in self._bucket_after_layer:
            self.reducer.launch(self._bucket_after_layer[l])

    def _dgrad_layer(self, l: int) -> None:
        """dgrad of layer l >= 1: DZ[l] (or its e5m2 copy) into DZ[l-1], ReLU' of Y[l-1] fused (and, in
        a residual trunk, the skip gradient of the block that layer l opens)."""
        w8 = self.fp8_wgrad and self._g8_calibrated
        if w8 and self.fp8_dgrad and l in self._w8layers:
            # all-fp8 backward: the e5m2 dZ copy wgrad(l) read is also this dgrad's operand;
            # the output goes out as e5m2 (wgrad(l-1) and dgrad(l-1) read it) and as bf16 only
            # for the first layer's bf16 wgrad; its max |dx| comes from wgrad(l-1)'s bytes
            f8out = l - 1 in self._w8layers
            # residual trunk, odd l (a block's first layer): the skip gradient DZ[l+1] joins before ReLU', and
            # DZ[l-1] goes out in bf16 as well -- it is the skip gradient of the block below
            skip = self.residual and l % 2 == 1
            ops.conv_dgrad_fp8_bits(self.DZ8[l], self.wd8[l], self.MBITS[l - 1], self.gscales8[l],
                                    self.gosc8[l - 1:l], self.K[l], self.S,
                                    y_bf16=None if f8out and not skip else self.DZ[l - 1],
                                    y_fp8=self.DZ8[l - 1] if f8out else None,
                                    amax=None if f8out else self.gamax8[l - 1],
                                    res=self.DZ[l + 1] if skip else None)
        elif w8 and l - 1 in self._w8layers:  # bitmask dgrad + the e5m2 copy wgrad(l-1) reads
            ops.conv_dgrad_bits_bf8(self.DZ[l], self.wd[l], self.DZ[l - 1], self.MBITS[l - 1],
                                    self.DZ8[l - 1], self.gosc8[l - 1:l], self.K[l], self.S,
                                    tile=self.conv_tile)
        elif (self.precision == "fp8" and self.fp8_dgrad and self._g8_calibrated
              and l not in self.fp8_bf16_layers):
            # fp8 dgrad straight from the bf16 dZ: converted to e5m2 in the kernel's registers
            # (delayed per-layer scale gosc8[l]), ReLU' from the forward's bitmask, bf16 dx
            # whose max |dx| sets the next step's scale of layer l-1
            if l == self.L - 1:  # the head's dZ: its max |dZ| for the next step's scale
                ops.absmax_bf16(self.DZ[l], self.gamax8[l])
            ops.conv_dgrad_fp8_bf16(self.DZ[l], self.wd8[l], self.MBITS[l - 1], self.gscales8[l],
                                    self.gosc8[l:l + 1], self.K[l], self.S, self.DZ[l - 1],
                                    amax=self.gamax8[l - 1])
        elif self.lab_tile and self.K[l] == 3:  # kernel-lab A/B (see __init__)
            ops.lab().conv_fwd(self.DZ[l], self.wd[l], None, None, self.DZ[l - 1], 3, self.S, 1, 1,
                               ops.MODE_MASKBITS, self.MBITS[l - 1], self.lab_tile)
        else:  # ReLU' bitmask from the forward epilogue (bf16 and fp8 forwards write it); small batches
            # on the weight-stationary or the split-K tile (dg_plan).  Residual trunk, odd l (a block's
            # first layer): DZ[l-1] = (W_l^T DZ[l] + DZ[l+1]) * ReLU'(Y[l-1]) -- the skip carries the
            # already-masked gradient at the block's output, which nothing writes again in this backward
            # (the side-stream wgrad only reads it)
            res = self.DZ[l + 1] if self.residual and l % 2 == 1 else None
            if self.gpool_blocks and l in self._gp_layers:  # a branch block's last layer: the pooling's gradient
                res = self._gp_G2
            ops.conv_planned(self.dg_plan[l], self.DZ[l], self.wd[l], self.wd_ws[l], None, self.DZ[l - 1],
                             self.K[l], self.S, 1, ops.MODE_MASKBITS, self.MBITS[l - 1], self._sk_ws, res=res)

    def backward_trunk(self, reduce: bool = True) -> None:
        """dZ[L-1] (and head grads) must be ready on the current stream.
        ``reduce=False`` leaves the local gradient (gradient accumulation: the
        caller all-reduces the sum once)."""
        main = torch.cuda.current_stream(self.device)
        red = reduce and (self.env.distributed or self._proxy is not None)
        self._launch_bucket_after(-1, red)
        top = self.L - 1
        if self.fp8_wgrad and self._g8_calibrated and top in self._w8layers and not self._head_wrote_e5m2:
            # the head's dZ in e5m2 for wgrad(L-1), and its max |dZ| (the value head writes it itself)
            ops.quantize_bf8(self.DZ[top], self.DZ8[top], self.gosc8[top:top + 1], self.gamax8[top])
        for l in reversed(range(self.L)):
            if self.gpool_blocks and l in self._gp_layers:
                self._gpool_backward(l)
            if self.s_w is not None:
                ev = main.record_event()
                with torch.cuda.stream(self.s_w):
                    self.s_w.wait_event(ev)
                    self._wgrad_layer(l, red)
            else:
                self._wgrad_layer(l, red)
            if l > 0:
                self._dgrad_layer(l)
        # join the side streams first: the fp8 wgrads still running there read gscales8 / gosc8
        # and fold max |dZ| into gamax8, which the scale update below rewrites and clears
        if self.s_w is not None:
            main.wait_stream(self.s_w)
        if self.s_r is not None:
            main.wait_stream(self.s_r)
        if self._pending_reduce:  # merged reduce: every deferred layer's split slab in one launch
            pr = self._pending_reduce
            ops.conv_wgrad_reduce_multi([p[0] for p in pr], [p[1] for p in pr],
                                        [self.fp.grad_views["w%d" % p[2]] for p in pr],
                                        [self.fp.grad_views["b%d" % p[2]] for p in pr], 1.0, 0.0)
            self._pending_reduce = []
        if self.precision == "fp8" and (self.fp8_dgrad or self.fp8_wgrad):
            if self._g8_calibrated:
                ops.fp8_grad_scales(self.gamax8, self.gscales8, self.gosc8, 1)  # next step's gradient scales
            else:
                self._fp8_grad_calibrate()
        if red:
            if self.defer_allreduce:
                for bi in range(len(self.buckets)):
                    self.reducer.launch(bi)
            if self.comm_events is not None:  # exposed all-reduce time (utils.metrics.StepMetrics)
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record(main)
            self.reducer.wait()
            if self.comm_events is not None:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record(main)
                self.comm_events.append((e0, e1))

    @torch.no_grad()
    def _fp8_grad_calibrate(self) -> None:
        """First backward (bf16 dgrads): e5m2 scales of dZ_1..dZ_{L-1} from this step's max |dZ|."""
        amax = torch.stack([self.DZ[l].abs().amax().float() for l in range(self.L)])
        self.gamax8.zero_()
        self.gamax8[:, 0].copy_(amax.view(torch.int32))
        ops.fp8_grad_scales(self.gamax8, self.gscales8, self.gosc8, 1)
        self._g8_calibrated = True

    def compute_grads(self, planes: torch.Tensor, targets: torch.Tensor, sym: Optional[torch.Tensor] = None,
                      weight: Optional[torch.Tensor] = None, reduce: bool = True,
                      rows: Optional[torch.Tensor] = None):
        """Forward + backward into self.fp.grad (all-reduced when distributed,
        unless ``reduce=False``).  ``rows`` (int64, B): the minibatch is ``planes[rows]`` of a
        device-resident pool, gathered by the input-pack kernel itself (no separate index_select);
        ``targets``, ``sym`` and ``weight`` stay per board."""
        B = planes.shape[0] if rows is None else rows.numel()
        if B != self.batch:
            raise ValueError("batch %d != configured %d" % (B, self.batch))
        with trace_range("forward"):
            self._train_fwd = True
            self._rows = rows
            try:
                self._forward_for_head(planes, targets, sym)
            finally:
                self._train_fwd = False
                self._rows = None
        with trace_range("head"):
            self._head_train(targets, 1.0 / (B * self.env.world_size), weight, sym)
        with trace_range("backward+allreduce"):
            self.backward_trunk(reduce)

    def _sgd_pack_plan(self):
        """(per-layer (flat offset, Cout, Cin, K, K), plain SGD ranges) of the fused update."""
        meta, wsegs = [], set()
        for l in range(self.L):
            off, n = self.fp.segments["w%d" % l]
            w = self.fp.views["w%d" % l]
            meta.append((off, w.shape[0], w.shape[1], w.shape[2]))
            wsegs.add(off)
        ranges = []
        for name in self.fp.names:
            off, n = self.fp.segments[name]
            if off in wsegs:
                continue
            if ranges and ranges[-1][0] + ranges[-1][1] == off:
                ranges[-1] = (ranges[-1][0], ranges[-1][1] + n)
            else:
                ranges.append((off, n))
        return meta, ranges

    def apply_update(self, device_schedule: bool = False) -> None:
        with trace_range("sgd+repack"):
            if self._fused_update:
                # one launch: SGD over the flat master weights + the bf16 forward / dgrad packs
                if self._pack_plan is None:
                    self._pack_plan = self._sgd_pack_plan()
                meta, ranges = self._pack_plan
                sched = None
                if device_schedule:  # the SGD kernels read the 4-entry prefix, Adam all 8
                    sched = self._sched_dev if self.sched.optimizer == "adam" else self._sched_dev[:4]
                st = self.opt_state
                ops.sgd_pack(self.fp.flat, self.fp.grad, 0.0 if device_schedule else self.sched.current(), meta,
                             self.wf, self.wd, ranges, sched=sched, m1=st[0] if st else None,
                             m2=st[1] if len(st) > 1 else None, **self.sched.kernel_kwargs())
                self.sched.advance()
                self.repack(bf16=False)
                return
            if self.sched.optimizer != "sgd":
                raise ValueError("momentum / Adam run in the fused update only (ALPHAGO_AMD_FUSED_UPDATE=1)")
            if device_schedule:
                # graph replays: lr = lr0 / (1 + decay * t) evaluated on the device (the same f64
                # expression as KerasSGDSchedule.current()) from the copy synced at capture time
                ops.sgd_update_sched(self.fp.flat, self.fp.grad, self._sched_dev[:4], 1.0)
            else:
                ops.sgd_update(self.fp.flat, self.fp.grad, self.sched.current(), 1.0)
            self.sched.advance()
            self.repack()

    def step(self, planes: torch.Tensor, targets: torch.Tensor, sym: Optional[torch.Tensor] = None,
             weight: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None):
        """One SGD step.  Returns (sum of per-board loss, metric sum) as device scalars (local;
        in graph mode static tensors, valid until the next step).  ``rows``: see compute_grads
        (eager steps only)."""
        if self.use_graph and weight is None:
            if rows is not None:
                raise ValueError("graph mode: pass the gathered minibatch, not pool rows")
            return self._graph_step(planes, targets, sym)
        self.compute_grads(planes, targets, sym, weight, rows=rows)
        self.apply_update()
        return self._step_metrics()

    def _step_metrics(self):
        return self.loss.sum(), self.correct.sum()

    def static_inputs(self, planes: torch.Tensor, targets: torch.Tensor, sym: Optional[torch.Tensor] = None):
        """Graph mode: the captured step's input buffers (allocated like the given tensors on first
        use).  A data pipeline that writes a batch straight into them (``index_select(out=...)``, a
        host copy) and passes them to ``step`` saves the step's three input copies."""
        if self._g_in is None:
            self._g_in = (torch.empty_like(planes), torch.empty_like(targets),
                          None if sym is None else torch.empty_like(sym))
            self._g_out = (torch.zeros((), device=self.device), torch.zeros((), device=self.device))
        return self._g_in

    def _graph_step(self, planes, targets, sym):
        gp, gt, gs = self.static_inputs(planes, targets, sym)
        if (sym is None) != (gs is None) or planes.shape != gp.shape:
            raise ValueError("graph mode: inputs must keep their shape and symmetry argument")
        if planes.data_ptr() != gp.data_ptr():  # the caller's own buffers: copy into the static ones
            gp.copy_(planes, non_blocking=True)
        if targets.data_ptr() != gt.data_ptr():
            gt.copy_(targets, non_blocking=True)
        if gs is not None and sym.data_ptr() != gs.data_ptr():
            gs.copy_(sym, non_blocking=True)
        # ALPHAGO_AMD_GRAPH_ALLREDUCE=1: the bucketed async all-reduce is captured inside the graph
        # (launched at its bucket points on RCCL's stream, joined before the update), so a graph step
        # keeps the eager step's overlap; by default the all-reduce runs eagerly between two graphs
        cap_ar = self.env.distributed and os.environ.get("ALPHAGO_AMD_GRAPH_ALLREDUCE", "0") == "1"
        dist = self.env.distributed and not cap_ar

        def grads():
            self.compute_grads(gp, gt, gs, None, reduce=not dist)

        def update():
            self.apply_update(device_schedule=True)
            l, c = self._step_metrics()  # the eager step's sums (same summation order: bitwise equal)
            self._g_out[0].copy_(l)
            self._g_out[1].copy_(c)

        if self._graphs is None:
            if not self._graph_warm:  # eager first step: code objects loaded, LDS attributes set
                self.sync_schedule()
                grads()
                if dist:
                    agdist.all_reduce_sum_(self.fp.grad)
                update()
                self._graph_warm = True
                return self._g_out
            torch.cuda.synchronize(self.device)
            self.sync_schedule()  # the device schedule continues from the host counter
            parts = [grads, update] if dist else [lambda: (grads(), update())]
            self._graphs = []
            # the wgrad side stream is captured as a parallel branch only on request
            # (ALPHAGO_AMD_GRAPH_OVERLAP=1); by default the graph is one serial chain
            keep_sw, keep_sr = self.s_w, self.s_r
            self.s_r = None  # captured serially: its slab events were recorded outside the capture
            if os.environ.get("ALPHAGO_AMD_GRAPH_OVERLAP", "0") != "1":
                self.s_w = None
            try:
                for fn in parts:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        fn()
                    self._graphs.append(g)
            finally:
                self.s_w, self.s_r = keep_sw, keep_sr
            # the capture ran nothing; the iteration counters it advanced on the host are undone
            self.sched.iterations -= 1
        self._graphs[0].replay()
        if dist:
            agdist.all_reduce_sum_(self.fp.grad)
            self._graphs[1].replay()
        self.sched.advance()
        return self._g_out


class HipPolicyTrainer(HipConvTrainer):
    """Policy net: fused HIP head (softmax + clipped CE + top-1 + backward).
    ``weight`` (per board) scales each board's gradient — REINFORCE rewards."""

    def _head_named_params(self):
        return [("head_w", self.net.head_w), ("head_b", self.net.head_b)]

    def _init_head(self):
        self.dhead = torch.zeros(self.batch, self.F + 1, device=self.device)
        self.tgt = torch.zeros(self.batch, dtype=torch.int32, device=self.device)

    def _forward_for_head(self, planes, targets, sym):
        if is_soft_target(targets):  # no move target to transform: the soft head moves the distribution itself
            self._check_soft(targets)
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(_SOFT_NO_GRAPH)
            self.forward_trunk(planes, sym)
            return
        self.forward_trunk(planes, sym, targets, self.tgt)

    def _check_soft(self, dist) -> None:
        """Soft targets (``is_soft_target``) run the plain soft-target head."""
        if self.policy_loss == "bce" or self.ent_coef or self.kl_coef or self.collect_stats or self.collect_probs:
            raise ValueError(_SOFT_REFUSED)
        SS = self.S * self.S
        if dist.shape[0] != self.batch or dist.shape[1] not in (SS, SS + 1):
            raise ValueError("soft targets must be (%d, %d) or (%d, %d), got %s"
                             % (self.batch, SS, self.batch, SS + 1, tuple(dist.shape)))

    def _head_soft(self, dist, gscale, weight, sym) -> None:
        if dist.dtype != torch.float32 or not dist.is_contiguous():
            dist = dist.float().contiguous()
        ops.policy_head_train_soft(self.Y[-1], self.fp.views["head_w"].view(-1), self.fp.views["head_b"], dist,
                                   self.DZ[-1], self.loss, self.correct, self.dhead, self.S, gscale, weight=weight,
                                   sym=sym)

    def step(self, planes: torch.Tensor, targets: torch.Tensor, sym: Optional[torch.Tensor] = None,
             weight: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None):
        if is_soft_target(targets) and self.use_graph:  # before the graph path allocates its static inputs
            raise RuntimeError(_SOFT_NO_GRAPH)
        return super().step(planes, targets, sym, weight, rows)

    policy_loss = "ce"  # or "bce": the reference RL loss (binary CE on the softmax)

    # Regularised objective of the fused head (policy_loss "ce" only), per board
    #   L_b = -w_b log p_t - ent_coef * H(p) + kl_coef * KL(ref_probs || p),
    # each divided by the global batch like the CE term.  All off (the defaults): the plain head
    # kernels run and nothing below is allocated.
    ent_coef = 0.0
    kl_coef = 0.0
    ref_probs = None        # (batch, S*S) f32 anchor distribution, filled by the caller
    collect_stats = False   # head_stats (batch, 3) <- H(p), KL(ref_probs || p), max |logit| per board on
    head_stats = None       # every compute_grads / evaluate
    collect_probs = False   # head_probs (batch, S*S) <- p of the last compute_grads
    head_probs = None

    def _head_extras(self, train: bool) -> dict:
        """Keyword arguments of the regularised head ({}: the plain kernels, today's call);
        ``train=False`` (evaluate): the diagnostics only."""
        if not (self.collect_stats or (train and (self.ent_coef or self.kl_coef or self.collect_probs))):
            return {}
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the captured SL step runs the plain head: leave ent_coef, kl_coef and "
                               "collect_* off in graph mode")
        kw = {"ref_probs": self.ref_probs}
        if self.collect_stats:
            if self.head_stats is None:
                self.head_stats = torch.zeros(self.batch, 3, device=self.device)
            kw["stats"] = self.head_stats
        if train:
            kw.update(ent_coef=self.ent_coef, kl_coef=self.kl_coef)
            if self.collect_probs:
                if self.head_probs is None:
                    self.head_probs = torch.zeros(self.batch, self.S * self.S, device=self.device)
                kw["probs"] = self.head_probs
        return kw

    def _head_train(self, targets, gscale, weight, sym=None):
        if is_soft_target(targets):
            self._head_soft(targets, gscale, weight, sym)
        else:
            self._head_hard(gscale, weight)
        ho, hn = self.fp.segments["head_w"]
        # head gradient and the step's two metric sums in one launch (a fresh 2-vector per step, so
        # the returned scalars stay valid after the next step)
        self._metric_sums = torch.empty(2, device=self.device)
        ops.head_grad_sums(self.dhead, self.loss, self.correct, self.fp.grad[ho:ho + hn + 1], self._metric_sums)

    def _head_hard(self, gscale, weight):
        hw = self.fp.views["head_w"].view(-1)
        hb = self.fp.views["head_b"]
        ops.policy_head_train(self.Y[-1], hw, hb, self.tgt, self.DZ[-1], self.loss, self.correct, self.dhead,
                              self.S, gscale, weight=weight, bce=self.policy_loss == "bce",
                              **self._head_extras(True))

    def _step_metrics(self):
        return self._metric_sums[0], self._metric_sums[1]

    @torch.no_grad()
    def evaluate(self, planes: torch.Tensor, targets: torch.Tensor):
        """Loss/accuracy without update (validation)."""
        if is_soft_target(targets):
            self._check_soft(targets)
            self.forward_trunk(planes)
            self._head_soft(targets, 0.0, None, None)
            return self.loss.sum(), self.correct.sum()
        self.forward_trunk(planes, None, targets, self.tgt)
        hw = self.fp.views["head_w"].view(-1)
        ops.policy_head_train(self.Y[-1], hw, self.fp.views["head_b"], self.tgt, self.DZ[-1], self.loss,
                              self.correct, self.dhead, self.S, 0.0, **self._head_extras(False))
        return self.loss.sum(), self.correct.sum()

    @torch.no_grad()
    def policy_stats(self, planes: torch.Tensor, ref_probs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(batch, 3) per board: entropy H(p), KL(ref_probs || p) (0 without ``ref_probs``) and
        max |logit| of the current weights.  Forward only (the trunk, then the head in its inference
        form): neither the gradient nor the schedule is touched."""
        if planes.shape[0] != self.batch:
            raise ValueError("batch %d != configured %d" % (planes.shape[0], self.batch))
        self.forward_trunk(planes)
        out = torch.empty(self.batch, 3, device=self.device)
        ops.policy_head_probs(self.Y[-1], self.fp.views["head_w"].view(-1), self.fp.views["head_b"], None, self.S,
                              ref_probs=ref_probs, stats=out)
        return out


class HipValueTrainer(HipConvTrainer):
    """Value net (reference value.py:12-31): HIP trunk + 1x1 conv -> Dense(256)
    -> Dense(1) -> tanh head; MSE against game outcomes in [-1, 1].

    Head forward: ``head_logits`` (one pass over the last activation) -> z
    (B, 361) fp32; the 361x256 dense layer on the hand-written fp32 MFMA GEMM
    (``dense_f32``, csrc/kernels/dense.hip); ``value_out`` fuses the 256->1
    layer, tanh, MSE, sign accuracy and its backward.  Head backward:
    dz = dh W1^T and dW1 = z^T dh (the same kernel, operands read transposed
    in place, dW1 written straight into the flat gradient buffer), then
    ``head_backward`` writes the ReLU'-masked gradient into the MFMA trunk
    backward plus per-board partials of the 1x1 conv weight/bias.
    ``correct`` counts sign(v) == sign(z)."""

    def _head_named_params(self):
        n = self.net
        return [("head_w", n.head_w), ("head_b", n.head_b), ("fc1_w", n.fc1_w), ("fc1_b", n.fc1_b),
                ("fc2_w", n.fc2_w), ("fc2_b", n.fc2_b)]

    def _init_head(self):
        B, NP, dev = self.batch, self.S * self.S, self.device
        D = self.net.fc1_w.shape[1]
        self.D = D
        self.z = torch.zeros(B, NP, device=dev)
        self.h = torch.zeros(B, D, device=dev)
        self.dh = torch.zeros(B, D, device=dev)
        self.dzl = torch.zeros(B, NP, device=dev)
        self.val = torch.zeros(B, device=dev)
        self.dout = torch.zeros(B, D + 1, device=dev)
        self.dhead = torch.zeros(B, self.F + 1, device=dev)
        self.tval = torch.zeros(B, device=dev)

    def _forward_for_head(self, planes, targets, sym):
        self.forward_trunk(planes, sym, None, None)

    def _head_forward(self):
        v = self.fp.views
        ops.head_logits(self.Y[-1], v["head_w"].view(-1), v["head_b"], self.z, self.S)
        ops.dense_f32(self.z, v["fc1_w"], self.h, bias=v["fc1_b"])  # h = z W1 + b1

    def _head_train(self, targets, gscale, weight, sym=None):
        v, gv = self.fp.views, self.fp.grad_views
        self._head_forward()
        self.tval.copy_(targets)
        ops.value_out(self.h, v["fc2_w"].view(-1), v["fc2_b"], self.val, target=self.tval, weight=weight,
                      loss=self.loss, correct=self.correct, dh=self.dh, dout=self.dout, grad_scale=gscale)
        ops.dense_f32(self.z, self.dh, gv["fc1_w"], trans_a=True)  # dW1 = z^T dh
        # column sums of the per-board partials on the fixed-order head_grad_sums kernel (torch's
        # column reductions were 4 launches, ~50 us of the 4.3 ms fp8 step); every call also writes
        # the step's (loss, correct) sums into a fresh 2-vector
        self._metric_sums = torch.empty(2, device=self.device)
        ops.head_grad_sums(self.dh, self.loss, self.correct, gv["fc1_b"], self._metric_sums)
        o2, n2 = self.fp.segments["fc2_w"]
        ops.head_grad_sums(self.dout, self.loss, self.correct, self.fp.grad[o2:o2 + n2 + 1],
                           self._metric_sums)  # [dw2 | db2]
        ops.dense_f32(self.dh, v["fc1_w"], self.dzl, trans_b=True)  # dz = dh W1^T
        # fp8 backward: dZ goes out as e5m2 straight from the head (no bf16 dZ write + quantize_bf8
        # re-read: 37 us of the 4.2 ms fp8 step, round 6)
        top = self.L - 1
        self._head_wrote_e5m2 = self._top_e5m2_fusable()
        e5 = (self.DZ8[top], self.gosc8[top:top + 1], self.gamax8[top]) if self._head_wrote_e5m2 else ()
        ops.head_backward(self.Y[-1], v["head_w"].view(-1), self.dzl, self.DZ[-1], self.dhead, self.S, *e5)
        ho, hn = self.fp.segments["head_w"]
        ops.head_grad_sums(self.dhead, self.loss, self.correct, self.fp.grad[ho:ho + hn + 1],
                           self._metric_sums)  # [dW_head | db_head]

    def _step_metrics(self):
        return self._metric_sums[0], self._metric_sums[1]

    @torch.no_grad()
    def evaluate(self, planes: torch.Tensor, targets: torch.Tensor):
        val = self.predict(planes)
        z = targets.float()
        return ((val - z) ** 2).sum(), (torch.sign(val) == torch.sign(z)).float().sum()

    @torch.no_grad()
    def predict(self, planes: torch.Tensor) -> torch.Tensor:
        self.forward_trunk(planes, None, None, None)
        self._head_forward()
        v = self.fp.views
        ops.value_out(self.h, v["fc2_w"].view(-1), v["fc2_b"], self.val)
        return self.val.clone()


_PV_NO_GRAPH = ("the dual (policy + value) trainer is not supported in graph mode: the captured SL step takes one "
                "move per board and no outcome")

_PV_REFUSED = ("the dual (policy + value) trainer trains the plain cross-entropy plus the value MSE only: leave "
               "policy_loss at 'ce' and ent_coef, kl_coef and collect_* off")


def _pv_targets(targets, ownership: bool = False):
    """(pi_or_moves, z, own) of a dual-trainer target: a pair (own = None) or, for a net with the
    ownership head, a triple whose last entry is (own_t (B, S*S) int8 in the mover's frame, own_valid
    (B,))."""
    if isinstance(targets, (tuple, list)) and len(targets) == 3:
        if not ownership:
            raise ValueError("a target triple (pi, z, (own_t, own_valid)) needs a net with the ownership head")
        own = targets[2]
        if not isinstance(own, (tuple, list)) or len(own) != 2:
            raise ValueError("the ownership target is a pair (own_t (B, S*S), own_valid (B,))")
        return targets[0], targets[1], (own[0], own[1])
    if not isinstance(targets, (tuple, list)) or len(targets) != 2:
        raise ValueError("the dual trainer's targets are a pair (moves or pi, outcomes z)" +
                         (" or a triple with (own_t, own_valid)" if ownership else ""))
    return targets[0], targets[1], None


def _pv_score_target(targets, score_head: bool):
    """(targets without the fourth slot, score): a 4-tuple (pi, z, own_or_None, (score_t, score_valid)) carries
    the score target -- ``score_t`` (B,) in points in the mover's frame, komi included, ``score_valid`` (B,)
    marking the boards of scored games; pairs and triples mean what they always meant (score = None)."""
    if not (isinstance(targets, (tuple, list)) and len(targets) == 4):
        return targets, None
    if not score_head:
        raise ValueError("a target 4-tuple (pi, z, own, (score_t, score_valid)) needs a net with the score head "
                         "(score_head=1)")
    sc = targets[3]
    if not isinstance(sc, (tuple, list)) or len(sc) != 2:
        raise ValueError("the score target is a pair (score_t (B,), score_valid (B,))")
    base = (targets[0], targets[1]) if targets[2] is None else (targets[0], targets[1], targets[2])
    return base, (sc[0], sc[1])


def pass_target_rows(moves: torch.Tensor, NP: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, NP + 1) one-hot rows of hard move targets for a net with the pass head: a move of -1 (a pass) has
    its 1 at column NP.  The rows take the soft-target path, which moves them with the board."""
    idx = moves.long().view(-1)
    idx = torch.where(idx < 0, torch.full_like(idx, NP), idx)
    rows = torch.zeros(idx.numel(), NP + 1, device=moves.device) if out is None else out.zero_()
    return rows.scatter_(1, idx[:, None], 1.0)


def _pass_rows_checked(pi, batch: int, NP: int):
    if tuple(pi.shape) != (batch, NP + 1):
        raise ValueError("a net with the pass head takes soft targets of shape (%d, %d) with the pass last (a row "
                         "of %d has no pass entry), got %s" % (batch, NP + 1, NP, tuple(pi.shape)))
    return pi


def own_agreement_share(own, own_t):
    """Per board, the share of the points with a non-zero target whose sign ``own`` matches (0 for a
    board without such points): the trainers' sixth metric before the sum over valid boards."""
    t = own_t.to(own.dtype)
    nz = t != 0
    return ((torch.sign(own) == t) & nz).to(own.dtype).sum(1) / nz.sum(1).clamp_min(1).to(own.dtype)


class HipPolicyValueTrainer(HipPolicyTrainer):
    """Dual net (PolicyValueNet): one HIP trunk, the policy trainer's fused head and the value
    trainer's head on its output.  Called as ``step(planes, (pi_or_moves, z), sym=None, weight=None)``
    / ``compute_grads(...)``; the loss is policy CE (hard moves or a soft ``(B, S*S [+ 1])``
    distribution, exactly HipPolicyTrainer's heads) + ``value_coef`` * MSE(v, z), each term divided
    by the global batch.  ``value_coef`` (default 1.0, AlphaGo Zero's equal weighting) enters through
    ``value_out``'s ``grad_scale``.

    Order of a step: trunk forward; the policy head (writes dZ[L-1] and its per-board head partials);
    ``head_logits`` -> ``dense_f32`` -> ``value_out`` and the two ``dense_f32`` backward calls as in
    HipValueTrainer; ``head_backward_add`` adds the value head's ReLU'-masked dY into dZ[L-1]; the
    ``head_grad_sums`` calls; the unchanged trunk backward and update.  All eight head tensors live
    in the flat parameters, so the fused optimizer, the buckets and data parallelism need nothing new.

    ``step`` returns (policy loss sum, top-1 sum, value squared-error sum, sign-agreement sum).

    A net with the ownership head (``PolicyValueNet(ownership=1)``) takes targets
    ``(pi_or_moves, z, (own_t, own_valid))``: ``own_t`` (B, S*S) int8 is the final territory map in the
    mover's frame of the stored planes (the head kernel moves it with ``sym``), ``own_valid`` (B,) marks
    the boards whose game was scored.  The loss gains ``own_coef`` * (1 / B_global) sum_b valid_b w_b
    MSE_b(own, own_t); ``own_coef`` defaults to 1.0, a conventional starting point that is not tuned.
    In the step ``value_own_head`` takes ``head_logits``' place (one read of Y[L-1] for both heads) and
    ``head_backward_add2`` ``head_backward_add``'s (one read-modify-write of dZ[L-1] for both), with one
    more ``head_grad_sums`` call for ``ohead_w`` / ``ohead_b``, which follow ``fc2_b`` in the flat
    parameters.  ``step`` and ``evaluate`` then return six sums: the four above, the sum over valid
    boards of the per-board mean squared error, and the sum over valid boards of the share of decided
    points (target != 0) whose sign the head matches.  A pair ``(pi, z)`` is still accepted: it runs
    the step of a net without the head, leaves ``ohead_*`` without gradient and reports 0 for both.
    A net without the head launches exactly the kernels above and returns four sums.

    A net with the pass head (``PolicyValueNet(pass_head=1)``): the policy softmax, loss and top-1 run over
    S*S + 1 entries, the pass last.  Soft targets must be (B, S*S + 1); hard moves become one-hot rows of that
    width (a move of -1, a pass, at column S*S) and take the same path.  Per step: ``gpool_fwd(Y[L-1])``, then
    ``policy_head_soft_pass`` in the soft head's place; the value and ownership steps unchanged;
    ``gpool_bwd_add_masked`` adds the pooling's ReLU'-masked gradient into dZ[L-1] last; one more
    ``head_grad_sums`` for ``pass_w`` / ``pass_b``, which follow the ownership entries in the flat parameters.
    The metric sums are the same; policy loss and top-1 now count pass rows.  A net without the head
    launches exactly the kernels above.

    A net with the score head (``PolicyValueNet(score_head=1)``) takes a fourth target slot,
    ``(pi_or_moves, z, own_or_None, (score_t, score_valid))``: ``score_t`` (B,) fp32 is the final margin in
    points in the mover's frame, komi included (the trainer divides by S), ``score_valid`` (B,) marks the boards
    of scored games.  The loss gains ``score_coef`` * (1 / B_global) sum_b valid_b w_b Huber_delta(s_b - t_b / S);
    ``score_coef`` = 1.0 and ``score_delta`` = 1.0 (S points) are conventional starting points, not tuned.  The
    score does not move with ``sym``.  Per step: ``gpool_fwd(Y[L-1])`` once (shared with the pass head),
    ``dense_f32`` (upre = P sc1_w + sc1_b), ``score_out``, ``dense_f32`` twice (d sc1_w = P^T du,
    dP = du sc1_w^T), then ``gpool_bwd_add_masked_dp`` as the last accumulation into dZ[L-1] -- with the pass
    head's term in the same pass, in ``gpool_bwd_add_masked``'s place -- and two ``head_grad_sums`` calls
    (``sc1_b`` from du, ``sc2_w | sc2_b`` from the partial rows).  The four tensors follow the pass entries in
    the flat parameters.  ``step`` / ``evaluate`` append two sums: the Huber loss over valid boards and
    |e| * S over valid boards, the absolute error in points.  A pair or triple trains without the score term,
    zeroes the four gradients and reports 0 for both.  A net without the head launches exactly the kernels above.

    fp8: the head writes the bf16 dZ only (``_top_e5m2_fusable`` is False: a sum of two heads cannot
    be accumulated in e5m2), so an fp8 backward works through the unfused ``quantize_bf8`` pass over
    the summed dZ[L-1], the policy trainer's path.  Graph mode and the regularised head options
    (``ent_coef``, ``kl_coef``, ``collect_*``, ``policy_loss='bce'``) are refused."""

    def __init__(self, net, batch: int, lr: float = 0.003, decay: float = 0.0, value_coef: float = 1.0,
                 own_coef: float = 1.0, score_coef: float = 1.0, score_delta: float = 1.0, **kw):
        self.value_coef = float(value_coef)
        self.own_coef = float(own_coef)
        self.score_coef = float(score_coef)    # 1.0: a conventional starting point, not tuned
        self.score_delta = float(score_delta)  # Huber threshold in units of S points; 1.0 is not tuned either
        self.has_own = bool(getattr(net, "ownership", False))
        self.has_pass = bool(getattr(net, "pass_head", False))
        self.has_score = bool(getattr(net, "score_head", False))
        super().__init__(net, batch, lr, decay, **kw)

    def _head_named_params(self):
        n = self.net
        named = [("head_w", n.head_w), ("head_b", n.head_b), ("vhead_w", n.vhead_w), ("vhead_b", n.vhead_b),
                 ("fc1_w", n.fc1_w), ("fc1_b", n.fc1_b), ("fc2_w", n.fc2_w), ("fc2_b", n.fc2_b)]
        if self.has_own:  # appended: the existing segments keep their offsets
            named += [("ohead_w", n.ohead_w), ("ohead_b", n.ohead_b)]
        if self.has_pass:  # after the ownership entries
            named += [("pass_w", n.pass_w), ("pass_b", n.pass_b)]
        if self.has_score:  # after the pass entries
            named += [("sc1_w", n.sc1_w), ("sc1_b", n.sc1_b), ("sc2_w", n.sc2_w), ("sc2_b", n.sc2_b)]
        return named

    def _init_head(self):
        super()._init_head()
        B, NP, dev = self.batch, self.S * self.S, self.device
        if self.has_pass or self.has_score:  # the pooled trunk output, shared by both heads
            F, Fp = self.F, self.Fp
            self._ps_P = torch.zeros(B, 2, Fp, device=dev)
            self._ps_arg = torch.zeros(B, Fp, dtype=torch.int32, device=dev)
        if self.has_score:
            SD = self.net.score_dense
            self._sc_up = torch.zeros(B, SD, device=dev)
            self._sc_s = torch.zeros(B, device=dev)
            self._sc_t = torch.zeros(B, device=dev)
            self._sc_valid = torch.zeros(B, device=dev)
            self._sc_loss = torch.zeros(B, device=dev)
            self._sc_abs = torch.zeros(B, device=dev)
            self._sc_du = torch.zeros(B, SD, device=dev)
            self._sc_dout = torch.zeros(B, SD + 1, device=dev)
            self._sc_dP = torch.zeros(B, 2, Fp, device=dev)
            # dense_f32 reads a (2 Fp, D) weight: the flat views, or zero-padded scratch (repack) when F < Fp
            if F == Fp:
                self._sc_w1, self._sc_dw1 = self.fp.views["sc1_w"], self.fp.grad_views["sc1_w"]
            else:
                self._sc_w1 = torch.zeros(2 * Fp, SD, device=dev)
                self._sc_dw1 = torch.zeros(2 * Fp, SD, device=dev)
        if self.has_pass:
            self._ps_d = torch.zeros(B, device=dev)
            self._ps_dpw = torch.zeros(B, 2 * F + 1, device=dev)
            self._ps_rows = torch.zeros(B, NP + 1, device=dev)
            # the kernels read a (2, Fp) weight: the flat view itself, or a zero-padded copy (repack)
            self._ps_w = self.fp.views["pass_w"].view(2, F) if F == Fp else torch.zeros(2, Fp, device=dev)
        D = self.net.fc1_w.shape[1]
        self.z = torch.zeros(B, NP, device=dev)
        self.h = torch.zeros(B, D, device=dev)
        self.dh = torch.zeros(B, D, device=dev)
        self.dzl = torch.zeros(B, NP, device=dev)
        self.val = torch.zeros(B, device=dev)
        self.dout = torch.zeros(B, D + 1, device=dev)
        self.vdhead = torch.zeros(B, self.F + 1, device=dev)
        self.tval = torch.zeros(B, device=dev)
        self.vloss = torch.zeros(B, device=dev)
        self.vcorrect = torch.zeros(B, device=dev)
        if self.has_own:
            self.own = torch.zeros(B, NP, device=dev)
            self.dlo = torch.zeros(B, NP, device=dev)
            self.odhead = torch.zeros(B, self.F + 1, device=dev)
            self.oloss = torch.zeros(B, device=dev)
            self.oagree = torch.zeros(B, device=dev)
            self.own_t = torch.zeros(B, NP, dtype=torch.int8, device=dev)
            self.own_valid = torch.zeros(B, device=dev)

    def repack(self, bf16: bool = True) -> None:
        super().repack(bf16)
        if self.has_pass and self.F < self.Fp:  # the pass head's zero-padded weight copy
            self._ps_w[:, :self.F].copy_(self.fp.views["pass_w"].view(2, self.F))
        if self.has_score and self.F < self.Fp:  # the score head's zero-padded first layer
            w = self.fp.views["sc1_w"]
            self._sc_w1[:self.F].copy_(w[:self.F])
            self._sc_w1[self.Fp:self.Fp + self.F].copy_(w[self.F:])

    def enable_graphs(self, on: bool = True) -> None:
        if on:
            raise RuntimeError(_PV_NO_GRAPH)
        super().enable_graphs(False)

    def _pass_pi(self, pi):
        """The policy target of a pass-head net as (B, S*S + 1) rows: soft rows checked, hard moves as one-hot
        rows in the planes' original frame (the head kernel moves them with ``sym``)."""
        NP = self.S * self.S
        if is_soft_target(pi):
            return _pass_rows_checked(pi, self.batch, NP)
        if pi.numel() != self.batch:
            raise ValueError("move targets must hold %d entries, got %d" % (self.batch, pi.numel()))
        return pass_target_rows(pi.to(self.device), NP, self._ps_rows)

    def _head_soft(self, dist, gscale, weight, sym) -> None:
        if not self.has_pass:
            return super()._head_soft(dist, gscale, weight, sym)
        if dist.dtype != torch.float32 or not dist.is_contiguous():
            dist = dist.float().contiguous()
        v = self.fp.views
        ops.gpool_fwd(self.Y[-1], self._ps_P, self._ps_arg, self.S)
        ops.policy_head_soft_pass(self.Y[-1], v["head_w"].view(-1), v["head_b"], self._ps_P, self._ps_w, v["pass_b"],
                                  dist, self.DZ[-1], self.loss, self.correct, self.dhead, self._ps_d, self._ps_dpw,
                                  self.S, gscale, weight=weight, sym=sym)

    def _top_e5m2_fusable(self) -> bool:
        return False

    def _check_plain(self) -> None:
        if self.policy_loss != "ce" or self.ent_coef or self.kl_coef or self.collect_stats or self.collect_probs:
            raise ValueError(_PV_REFUSED)

    def _forward_for_head(self, planes, targets, sym):
        self._check_plain()
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(_PV_NO_GRAPH)
        targets, score = _pv_score_target(targets, self.has_score)
        pi, z, own = _pv_targets(targets, self.has_own)
        if z.numel() != self.batch:
            raise ValueError("outcomes must hold %d entries, got %d" % (self.batch, z.numel()))
        if own is not None:
            self._check_own(own)
        if score is not None:
            self._check_score(score)
        if self.has_pass:
            pi = self._pi_rows = self._pass_pi(pi)  # converted once per step: _head_train takes these rows
        super()._forward_for_head(planes, pi, sym)

    def _check_own(self, own) -> None:
        NP = self.S * self.S
        if tuple(own[0].shape) != (self.batch, NP) or own[1].numel() != self.batch:
            raise ValueError("the ownership target is (own_t (%d, %d), own_valid (%d,)), got %s and %s"
                             % (self.batch, NP, self.batch, tuple(own[0].shape), tuple(own[1].shape)))

    def _check_score(self, score) -> None:
        if score[0].numel() != self.batch or score[1].numel() != self.batch:
            raise ValueError("the score target is (score_t (%d,), score_valid (%d,)), got %s and %s"
                             % (self.batch, self.batch, tuple(score[0].shape), tuple(score[1].shape)))

    def _score_forward(self, score, pooled: bool) -> None:
        """upre = P sc1_w + sc1_b from the pooled trunk output (``pooled``: gpool_fwd already ran this step) and
        the target in units of S points."""
        if not pooled:
            ops.gpool_fwd(self.Y[-1], self._ps_P, self._ps_arg, self.S)
        ops.dense_f32(self._ps_P.view(self.batch, -1), self._sc_w1, self._sc_up, bias=self.fp.views["sc1_b"])
        self._sc_t.copy_(score[0].view(-1))
        self._sc_t.div_(float(self.S))
        self._sc_valid.copy_(score[1].view(-1))

    def _score_metric_vectors(self):
        """(valid_b * Huber_b, valid_b * |e_b| * S): the loss in the head's unit, the absolute error in points."""
        return self._sc_loss * self._sc_valid, self._sc_abs * self._sc_valid * float(self.S)

    def _score_train(self, score, gscale, weight) -> None:
        """The score head's forward, loss and backward; the last accumulation into dZ[L-1] (the pass head's
        pooling gradient rides along) and the head's four gradients."""
        B, F, Fp = self.batch, self.F, self.Fp
        v, gv = self.fp.views, self.fp.grad_views
        self._score_forward(score, pooled=self.has_pass)
        ops.score_out(self._sc_up, v["sc2_w"].view(-1), v["sc2_b"], self._sc_s, target=self._sc_t,
                      valid=self._sc_valid, weight=weight, loss=self._sc_loss, abserr=self._sc_abs, du=self._sc_du,
                      dout=self._sc_dout, grad_scale=gscale * self.score_coef, delta=self.score_delta)
        P = self._ps_P.view(B, -1)
        ops.dense_f32(P, self._sc_du, self._sc_dw1, trans_a=True)  # d sc1_w = P^T du
        if F < Fp:
            gv["sc1_w"][:F].copy_(self._sc_dw1[:F])
            gv["sc1_w"][F:].copy_(self._sc_dw1[Fp:Fp + F])
        ops.dense_f32(self._sc_du, self._sc_w1, self._sc_dP.view(B, -1), trans_b=True)  # dP = du sc1_w^T
        ops.gpool_bwd_add_masked_dp(self._sc_dP, self._ps_arg, self.Y[-1], self.DZ[-1], self.S,
                                    dpass=self._ps_d if self.has_pass else None,
                                    pass_w=self._ps_w if self.has_pass else None)
        self._smetric_sums = torch.empty(2, device=self.device)
        sl, sa = self._score_metric_vectors()
        ops.head_grad_sums(self._sc_du, sl, sa, gv["sc1_b"], self._smetric_sums)
        so, sn = self.fp.segments["sc2_w"]
        ops.head_grad_sums(self._sc_dout, sl, sa, self.fp.grad[so:so + sn + 1], torch.empty(2, device=self.device))

    def _own_forward(self, own, sym, weight, gscale):
        """value_own_head in head_logits' place: z, own, the per-board ownership loss / agreement and dlo."""
        v = self.fp.views
        self.own_t.copy_(own[0])
        self.own_valid.copy_(own[1])
        ops.value_own_head(self.Y[-1], v["vhead_w"].view(-1), v["vhead_b"], v["ohead_w"].view(-1), v["ohead_b"],
                           self.z, self.S, own=self.own, target=self.own_t, sym=sym, valid=self.own_valid,
                           weight=weight, oloss=self.oloss, oagree=self.oagree, dlo=self.dlo, grad_scale=gscale)
        ops.dense_f32(self.z, v["fc1_w"], self.h, bias=v["fc1_b"])  # h = z W1 + b1

    def _own_metric_vectors(self):
        """(valid_b * MSE_b, valid_b * share_b): the kernel's per-board loss and agreement count times the
        caller's validity column, the count over the board's decided points."""
        nz = (self.own_t != 0).sum(1).clamp_min(1).float()
        return self.oloss * self.own_valid, self.oagree * self.own_valid / nz

    def _value_forward(self):
        v = self.fp.views
        ops.head_logits(self.Y[-1], v["vhead_w"].view(-1), v["vhead_b"], self.z, self.S)
        ops.dense_f32(self.z, v["fc1_w"], self.h, bias=v["fc1_b"])  # h = z W1 + b1

    def _head_train(self, targets, gscale, weight, sym=None):
        targets, score = _pv_score_target(targets, self.has_score)
        pi, z, own = _pv_targets(targets, self.has_own)
        v, gv = self.fp.views, self.fp.grad_views
        if self.has_pass:  # (B, S*S + 1) rows, hard moves included (_forward_for_head made them)
            pi = self._pi_rows
        # 1. the policy head, unchanged: dZ[L-1] and its [dW_head | db_head] partials
        if is_soft_target(pi):
            self._head_soft(pi, gscale, weight, sym)
        else:
            self._head_hard(gscale, weight)
        # 2. the value head's forward, output layer and dense backward (HipValueTrainer._head_train); with
        #    an ownership target the same read of Y[L-1] gives the ownership head's forward and dlo
        if own is not None:
            self._own_forward(own, sym, weight, gscale * self.own_coef)
        else:
            self._value_forward()
        self.tval.copy_(z)
        ops.value_out(self.h, v["fc2_w"].view(-1), v["fc2_b"], self.val, target=self.tval, weight=weight,
                      loss=self.vloss, correct=self.vcorrect, dh=self.dh, dout=self.dout,
                      grad_scale=gscale * self.value_coef)
        ops.dense_f32(self.z, self.dh, gv["fc1_w"], trans_a=True)  # dW1 = z^T dh
        ops.dense_f32(self.dh, v["fc1_w"], self.dzl, trans_b=True)  # dz = dh W1^T
        # 3. the value head's dY (and the ownership head's, in the same pass) added into the policy head's dZ[L-1]
        if own is not None:
            ops.head_backward_add2(self.Y[-1], v["vhead_w"].view(-1), self.dzl, v["ohead_w"].view(-1), self.dlo,
                                   self.DZ[-1], self.vdhead, self.odhead, self.S)
        else:
            ops.head_backward_add(self.Y[-1], v["vhead_w"].view(-1), self.dzl, self.DZ[-1], self.vdhead, self.S)
        # 4. column sums of every per-board partial, and the four metric sums (fresh vectors per step)
        self._metric_sums = torch.empty(2, device=self.device)
        self._vmetric_sums = torch.empty(2, device=self.device)
        ho, hn = self.fp.segments["head_w"]
        ops.head_grad_sums(self.dhead, self.loss, self.correct, self.fp.grad[ho:ho + hn + 1], self._metric_sums)
        ops.head_grad_sums(self.dh, self.vloss, self.vcorrect, gv["fc1_b"], self._vmetric_sums)
        o2, n2 = self.fp.segments["fc2_w"]
        ops.head_grad_sums(self.dout, self.vloss, self.vcorrect, self.fp.grad[o2:o2 + n2 + 1], self._vmetric_sums)
        vo, vn = self.fp.segments["vhead_w"]
        ops.head_grad_sums(self.vdhead, self.vloss, self.vcorrect, self.fp.grad[vo:vo + vn + 1], self._vmetric_sums)
        if self.has_own:
            oo, on = self.fp.segments["ohead_w"]
            if own is not None:
                self._ometric_sums = torch.empty(2, device=self.device)
                ol, oa = self._own_metric_vectors()
                ops.head_grad_sums(self.odhead, ol, oa, self.fp.grad[oo:oo + on + 1], self._ometric_sums)
            else:  # a pair: no ownership term
                self._ometric_sums = torch.zeros(2, device=self.device)
                self.fp.grad[oo:oo + on + 1].zero_()
        if self.has_score:
            # 6 (before 5's sums, in 5's accumulation's place). the score head; its gpool_bwd_add_masked_dp is
            #    the last accumulation into dZ[L-1] and carries the pass head's term
            if score is not None:
                self._score_train(score, gscale, weight)
            else:  # a pair or triple: no score term
                self._smetric_sums = torch.zeros(2, device=self.device)
                so = self.fp.segments["sc1_w"][0]
                eo, en = self.fp.segments["sc2_b"]
                self.fp.grad[so:eo + en].zero_()
        if self.has_pass:
            # 5. the pass head: its pooling's ReLU'-masked gradient into dZ[L-1], last of the accumulations,
            #    and [d pass_w | d pass_b] from the per-board partial rows
            if not (self.has_score and score is not None):
                ops.gpool_bwd_add_masked(self._ps_d, self._ps_w, self._ps_arg, self.Y[-1], self.DZ[-1], self.S)
            po, pn = self.fp.segments["pass_w"]
            ops.head_grad_sums(self._ps_dpw, self.loss, self.correct, self.fp.grad[po:po + pn + 1],
                               torch.empty(2, device=self.device))

    def step(self, planes, targets, sym: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None,
             rows: Optional[torch.Tensor] = None):
        if self.use_graph:
            raise RuntimeError(_PV_NO_GRAPH)
        self.compute_grads(planes, targets, sym, weight, rows=rows)
        self.apply_update()
        return self._step_metrics()

    def _step_metrics(self):
        m = (self._metric_sums[0], self._metric_sums[1], self._vmetric_sums[0], self._vmetric_sums[1])
        if self.has_own:
            m += (self._ometric_sums[0], self._ometric_sums[1])
        if self.has_score:
            m += (self._smetric_sums[0], self._smetric_sums[1])
        return m

    @torch.no_grad()
    def predict(self, planes: torch.Tensor) -> torch.Tensor:
        """Values (batch,) of the current weights, forward only."""
        self.forward_trunk(planes, None, None, None)
        self._value_forward()
        v = self.fp.views
        ops.value_out(self.h, v["fc2_w"].view(-1), v["fc2_b"], self.val)
        return self.val.clone()

    @torch.no_grad()
    def evaluate(self, planes: torch.Tensor, targets):
        """The four metric sums (six for a net with the ownership head, two more for one with the score head)
        without an update (validation)."""
        self._check_plain()
        targets, score = _pv_score_target(targets, self.has_score)
        pi, z, own = _pv_targets(targets, self.has_own)
        if own is not None:
            self._check_own(own)
        if score is not None:
            self._check_score(score)
        if self.has_pass:
            pi = self._pass_pi(pi)
        pl, pc = super().evaluate(planes, pi)  # leaves the trunk output in Y[-1]
        if own is not None:
            self._own_forward(own, None, None, 0.0)
        else:
            self._value_forward()
        v = self.fp.views
        ops.value_out(self.h, v["fc2_w"].view(-1), v["fc2_b"], self.val)
        zt = z.float()
        m = (pl, pc, ((self.val - zt) ** 2).sum(), (torch.sign(self.val) == torch.sign(zt)).float().sum())
        if self.has_own:
            if own is not None:
                ol, oa = self._own_metric_vectors()
                m += (ol.sum(), oa.sum())
            else:
                m += (torch.zeros((), device=self.device), torch.zeros((), device=self.device))
        if self.has_score:
            if score is not None:
                self._score_forward(score, pooled=False)
                ops.score_out(self._sc_up, v["sc2_w"].view(-1), v["sc2_b"], self._sc_s)
                e = self._sc_s - self._sc_t
                d = self.score_delta
                hub = torch.where(e.abs() <= d, 0.5 * e * e, d * (e.abs() - 0.5 * d))
                m += ((hub * self._sc_valid).sum(), (e.abs() * self._sc_valid).sum() * float(self.S))
            else:
                m += (torch.zeros((), device=self.device), torch.zeros((), device=self.device))
        return m

    def policy_stats(self, planes, ref_probs=None):
        raise ValueError(_PV_REFUSED)


class _TorchTrainerBase:
    def _setup(self, net, batch, lr, decay, device, dtype, iterations, named, optimizer="sgd", momentum=0.0,
               nesterov=False):
        self.env = agdist.env()
        self.device = torch.device(device) if device is not None else self.env.device
        self.net = net.to(self.device)
        self.batch = batch
        self.dtype = dtype
        self.sched = KerasSGDSchedule(lr, decay, iterations, optimizer=optimizer, momentum=momentum,
                                      nesterov=nesterov)
        self.params = [p for _, p in named]
        self.fp = FlatParams(named, self.device)
        if self.env.distributed:
            agdist.broadcast_(self.fp.flat, 0)
        self.opt_state = [torch.zeros_like(self.fp.flat) for _ in range(self.sched.n_moments)]
        self.table = symmetry_tables(net.board, self.device)

    def compute_grads(self, planes, targets, sym=None, weight=None, reduce: bool = True, rows=None):
        if rows is not None:  # the HIP trainers gather inside the pack kernel
            planes = planes.index_select(0, rows)
        for p in self.params:
            p.grad = None
        obj, per, metric = self._loss(planes, targets, sym, weight)
        obj.backward()
        for (name, p) in zip(self.fp.names, self.params):
            if p.grad is None:
                self.fp.grad_views[name].zero_()
            else:
                self.fp.grad_views[name].copy_(p.grad)
        if reduce and self.env.distributed:
            agdist.all_reduce_sum_(self.fp.grad)
        self._last = (per.detach(), metric.detach())

    def apply_update(self):
        with torch.no_grad():
            if self.sched.optimizer == "sgd":
                self.fp.flat.add_(self.fp.grad, alpha=-self.sched.current())
            else:
                optimizer_update_(self.fp.flat, self.fp.grad, self.opt_state, self.sched, self.sched.current())
        self.sched.advance()

    def step(self, planes, targets, sym=None, weight=None, rows=None):
        self.compute_grads(planes, targets, sym, weight, rows=rows)
        self.apply_update()
        per, metric = self._last
        return per.sum(), metric.sum()

    @torch.no_grad()
    def evaluate(self, planes, targets):
        obj, per, metric = self._loss(planes, targets, None, None)
        return per.sum(), metric.sum()


class TorchPolicyTrainer(_TorchTrainerBase):
    """Autograd implementation of the same SL/RL step (fp32 by default)."""

    policy_loss = "ce"  # or "bce" (reference RL loss), as HipPolicyTrainer

    def __init__(self, net: PolicyNet, batch: int, lr: float = 0.003, decay: float = 0.0, device=None,
                 dtype=torch.float32, iterations: int = 0, optimizer: str = "sgd", momentum: float = 0.0,
                 nesterov: bool = False):
        named = _trunk_named(net.trunk) + [("head_w", net.head_w), ("head_b", net.head_b)]
        self._setup(net, batch, lr, decay, device, dtype, iterations, named, optimizer, momentum, nesterov)

    def _loss_soft(self, planes, dist, sym, weight):
        """Targets are distributions (B, S*S [+ pass]): mean over the batch of -sum_i q_i log p_i,
        the objective of the HIP soft-target head."""
        if self.policy_loss == "bce" or self.ent_coef or self.kl_coef or self.collect_stats or self.collect_probs:
            raise ValueError(_SOFT_REFUSED)
        if sym is not None:
            planes, _ = apply_symmetry(planes, None, sym, self.table)
            dist = apply_symmetry_dist(dist, sym, self.table)
        logits = self.net.logits_torch(planes.to(self.dtype))
        per, correct, has = soft_target_loss(logits, dist)
        w = has.to(per.dtype) if weight is None else has.to(per.dtype) * weight
        return (per * w).sum() / (planes.shape[0] * self.env.world_size), per, correct

    def _loss(self, planes, targets, sym, weight):
        if is_soft_target(targets):
            return self._loss_soft(planes, targets, sym, weight)
        if sym is not None:
            planes, targets = apply_symmetry(planes, targets, sym, self.table)
        x = planes.to(self.dtype)
        logits = self.net.logits_torch(x)
        t = targets.long()
        valid = t >= 0
        correct = ((logits.argmax(1) == t) & valid).float()
        w = valid.float() if weight is None else valid.float() * weight
        norm = planes.shape[0] * self.env.world_size
        regularised = bool(self.ent_coef or self.kl_coef)
        if self.policy_loss == "bce":
            if regularised:
                raise ValueError("ent_coef / kl_coef go with the CE loss, not the reference binary CE")
            # reference RL loss: Keras binary_crossentropy on the softmax output,
            # mean over the S*S outputs, clipped probabilities
            prob = torch.softmax(logits, 1).clamp(1e-7, 1 - 1e-7)
            y = torch.nn.functional.one_hot(t.clamp_min(0), logits.shape[1]).to(prob.dtype)
            per = -(y * prob.log() + (1 - y) * (1 - prob).log()).mean(1) * valid
            if self.collect_stats:
                self._policy_stats(logits.detach(), self.ref_probs, store=True)
            return (per * w).sum() / norm, per, correct
        logp = torch.log_softmax(logits, 1)
        lt = logp.gather(1, t.clamp_min(0).unsqueeze(1)).squeeze(1)
        per = -torch.clamp(lt, min=math.log(1e-7), max=math.log(1 - 1e-7)) * valid
        # gradient of mean CE (unclipped, see kernels/head.hip); optional per-board weights (REINFORCE)
        obj = (-(lt * w)).sum() / norm
        if regularised:
            # - ent_coef * H(p) + kl_coef * KL(ref_probs || p) per board with a target, under the same
            # 1 / norm as the CE term and not multiplied by the reward weight
            p = logp.exp()
            if self.ent_coef:
                obj = obj + self.ent_coef * ((p * logp).sum(1) * valid).sum() / norm
            if self.kl_coef:
                if self.ref_probs is None:
                    raise ValueError("kl_coef > 0 needs ref_probs")
                q = self.ref_probs.to(logp.dtype)
                obj = obj + self.kl_coef * ((torch.xlogy(q, q) - q * logp).sum(1) * valid).sum() / norm
        if self.collect_stats:
            self._policy_stats(logits.detach(), self.ref_probs, store=True)
        if self.collect_probs and torch.is_grad_enabled():  # compute_grads, not evaluate
            self.head_probs = logp.detach().exp()
        return obj, per, correct

    ent_coef = 0.0   # the surface of HipPolicyTrainer (see there)
    kl_coef = 0.0
    ref_probs = None
    collect_stats = False
    head_stats = None
    collect_probs = False
    head_probs = None

    def _policy_stats(self, logits, ref_probs, store: bool = False) -> torch.Tensor:
        logp = torch.log_softmax(logits, 1)
        p = logp.exp()
        ent = -(p * logp).sum(1)
        if ref_probs is None:
            kl = torch.zeros_like(ent)
        else:
            q = ref_probs.to(logp.dtype)
            kl = (torch.xlogy(q, q) - q * logp).sum(1)
        out = torch.stack([ent, kl, logits.abs().amax(1)], 1).float()
        if store:
            self.head_stats = out
        return out

    @torch.no_grad()
    def policy_stats(self, planes, ref_probs=None) -> torch.Tensor:
        """(batch, 3) per board: H(p), KL(ref_probs || p) (0 without ``ref_probs``), max |logit|;
        forward only."""
        return self._policy_stats(self.net.logits_torch(planes.to(self.dtype)), ref_probs)


class TorchValueTrainer(_TorchTrainerBase):
    def __init__(self, net: ValueNet, batch: int, lr: float = 0.003, decay: float = 0.0, device=None,
                 dtype=torch.float32, iterations: int = 0, optimizer: str = "sgd", momentum: float = 0.0,
                 nesterov: bool = False):
        named = _trunk_named(net.trunk) + [("head_w", net.head_w), ("head_b", net.head_b), ("fc1_w", net.fc1_w),
                                           ("fc1_b", net.fc1_b), ("fc2_w", net.fc2_w), ("fc2_b", net.fc2_b)]
        self._setup(net, batch, lr, decay, device, dtype, iterations, named, optimizer, momentum, nesterov)

    def _loss(self, planes, targets, sym, weight):
        if sym is not None:
            planes, _ = apply_symmetry(planes, None, sym, self.table)
        v = self.net.forward_torch(planes.to(self.dtype))
        z = targets.float()
        err = (v - z) ** 2
        w = err if weight is None else err * weight
        obj = w.sum() / (planes.shape[0] * self.env.world_size)
        return obj, err, (torch.sign(v) == torch.sign(z)).float()


class TorchPolicyValueTrainer(_TorchTrainerBase):
    """Autograd twin of HipPolicyValueTrainer: mean over the global batch of the policy CE (hard or soft
    targets, TorchPolicyTrainer's expressions) + ``value_coef`` * (v - z)^2 on one trunk output; for a net
    with the ownership head and a target triple also ``own_coef`` * valid_b * mean_p (own - own_t)^2 (the
    target moved with the board by ``sym``).  ``own_coef`` defaults to 1.0, untuned.  For a net with the score
    head and a target 4-tuple also ``score_coef`` * valid_b * Huber_delta(score_torch(h) / S - score_t / S), which
    does not move with ``sym``; ``score_coef`` = 1.0 and ``score_delta`` = 1.0 are untuned starting points."""

    policy_loss = "ce"
    ent_coef = 0.0
    kl_coef = 0.0
    collect_stats = False
    collect_probs = False

    def __init__(self, net, batch: int, lr: float = 0.003, decay: float = 0.0, device=None, dtype=torch.float32,
                 iterations: int = 0, optimizer: str = "sgd", momentum: float = 0.0, nesterov: bool = False,
                 value_coef: float = 1.0, own_coef: float = 1.0, score_coef: float = 1.0, score_delta: float = 1.0):
        self.value_coef = float(value_coef)
        self.own_coef = float(own_coef)
        self.score_coef = float(score_coef)    # 1.0: a conventional starting point, not tuned
        self.score_delta = float(score_delta)  # Huber threshold in units of S points, not tuned either
        self.has_own = bool(getattr(net, "ownership", False))
        self.has_pass = bool(getattr(net, "pass_head", False))
        self.has_score = bool(getattr(net, "score_head", False))
        named = _trunk_named(net.trunk) + [(n, getattr(net, n)) for n in (
            "head_w", "head_b", "vhead_w", "vhead_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b") +
            (("ohead_w", "ohead_b") if self.has_own else ()) + (("pass_w", "pass_b") if self.has_pass else ()) +
            (("sc1_w", "sc1_b", "sc2_w", "sc2_b") if self.has_score else ())]
        self._setup(net, batch, lr, decay, device, dtype, iterations, named, optimizer, momentum, nesterov)

    def _loss(self, planes, targets, sym, weight):
        if self.policy_loss != "ce" or self.ent_coef or self.kl_coef or self.collect_stats or self.collect_probs:
            raise ValueError(_PV_REFUSED)
        targets, score = _pv_score_target(targets, self.has_score)
        pi, z, own = _pv_targets(targets, self.has_own)
        if self.has_pass:  # logits of S*S + 1 entries: rows with the pass last, hard moves as one-hot rows
            NP = self.net.board ** 2
            pi = (_pass_rows_checked(pi, planes.shape[0], NP) if is_soft_target(pi)
                  else pass_target_rows(pi.to(planes.device), NP))
        soft = is_soft_target(pi)
        if own is not None:
            own_t, own_valid = own[0].to(self.dtype), own[1].to(self.dtype)
            if sym is not None:
                own_t = apply_symmetry_dist(own_t, sym, self.table)
        if sym is not None:
            if soft:
                planes, _ = apply_symmetry(planes, None, sym, self.table)
                pi = apply_symmetry_dist(pi, sym, self.table)
            else:
                planes, pi = apply_symmetry(planes, pi, sym, self.table)
        h = self.net.trunk.forward_torch(planes.to(self.dtype))
        logits, v = self.net.heads_torch(h)
        norm = planes.shape[0] * self.env.world_size
        if soft:
            per, correct, has = soft_target_loss(logits, pi)
            w = has.to(per.dtype) if weight is None else has.to(per.dtype) * weight
            pobj = (per * w).sum() / norm
        else:
            t = pi.long()
            valid = t >= 0
            correct = ((logits.argmax(1) == t) & valid).float()
            w = valid.float() if weight is None else valid.float() * weight
            lt = torch.log_softmax(logits, 1).gather(1, t.clamp_min(0).unsqueeze(1)).squeeze(1)
            per = -torch.clamp(lt, min=math.log(1e-7), max=math.log(1 - 1e-7)) * valid
            pobj = (-(lt * w)).sum() / norm
        zt = z.to(v.dtype)
        err = (v - zt) ** 2
        vobj = (err if weight is None else err * weight).sum() / norm
        self._vlast = (err.detach(), (torch.sign(v) == torch.sign(zt)).float().detach())
        obj = pobj + self.value_coef * vobj
        if own is not None:
            o = self.net.ownership_torch(h)
            oerr = ((o - own_t) ** 2).mean(1)
            ow = own_valid if weight is None else own_valid * weight
            obj = obj + self.own_coef * (oerr * ow).sum() / norm
            self._olast = ((oerr * own_valid).detach(), (own_agreement_share(o.detach(), own_t) * own_valid))
        elif self.has_own:
            self._olast = (torch.zeros_like(err.detach()), torch.zeros_like(err.detach()))
        if score is not None:
            S = float(self.net.board)
            sv = score[1].to(v.dtype).view(-1)
            e = self.net.score_torch(h).to(v.dtype) / S - score[0].to(v.dtype).view(-1) / S
            d = self.score_delta
            hub = torch.where(e.abs() <= d, 0.5 * e * e, d * (e.abs() - 0.5 * d))
            sw = sv if weight is None else sv * weight
            obj = obj + self.score_coef * (hub * sw).sum() / norm
            self._slast = ((hub * sv).detach(), (e.abs() * sv * S).detach())
        elif self.has_score:
            self._slast = (torch.zeros_like(err.detach()), torch.zeros_like(err.detach()))
        return obj, per, correct

    def _metrics(self, pl, pc):
        m = (pl, pc, self._vlast[0].sum(), self._vlast[1].sum())
        if self.has_own:
            m += (self._olast[0].sum(), self._olast[1].sum())
        if self.has_score:
            m += (self._slast[0].sum(), self._slast[1].sum())
        return m

    def step(self, planes, targets, sym=None, weight=None, rows=None):
        return self._metrics(*super().step(planes, targets, sym, weight, rows))

    @torch.no_grad()
    def evaluate(self, planes, targets):
        return self._metrics(*super().evaluate(planes, targets))

    @torch.no_grad()
    def predict(self, planes) -> torch.Tensor:
        return self.net.logits_value_torch(planes.to(self.dtype))[1]


def make_value_trainer(net: ValueNet, batch: int, lr: float, decay: float = 0.0, backend: str = "auto",
                       device=None, **kw):
    dev = torch.device(device) if device is not None else agdist.env().device
    if backend == "auto":
        backend = "hip" if dev.type == "cuda" else "torch"
    if backend == "hip":
        return HipValueTrainer(net, batch, lr, decay, device=dev, **kw)
    return TorchValueTrainer(net, batch, lr, decay, device=dev, **_torch_kw(kw))


def make_policy_trainer(net: PolicyNet, batch: int, lr: float, decay: float = 0.0, backend: str = "auto",
                        device=None, **kw):
    dev = torch.device(device) if device is not None else agdist.env().device
    if backend == "auto":
        backend = "hip" if dev.type == "cuda" else "torch"
    if backend == "hip":
        return HipPolicyTrainer(net, batch, lr, decay, device=dev, **kw)
    return TorchPolicyTrainer(net, batch, lr, decay, device=dev, **_torch_kw(kw))


def make_policy_value_trainer(net, batch: int, lr: float, decay: float = 0.0, backend: str = "auto", device=None,
                              **kw):
    """The dual net's trainer: HipPolicyValueTrainer on a GPU, TorchPolicyValueTrainer otherwise
    (``value_coef``, ``own_coef``, ``score_coef`` and ``score_delta`` go to both)."""
    dev = torch.device(device) if device is not None else agdist.env().device
    if backend == "auto":
        backend = "hip" if dev.type == "cuda" else "torch"
    if backend == "hip":
        return HipPolicyValueTrainer(net, batch, lr, decay, device=dev, **kw)
    tkw = _torch_kw(kw)
    for k in ("value_coef", "own_coef", "score_coef", "score_delta"):
        if k in kw:
            tkw[k] = kw[k]
    return TorchPolicyValueTrainer(net, batch, lr, decay, device=dev, **tkw)


def _torch_kw(kw: dict) -> dict:
    """The HIP-trainer keywords the autograd trainers share (the rest are kernel options)."""
    return {k: kw[k] for k in ("iterations", "optimizer", "momentum", "nesterov") if k in kw}
