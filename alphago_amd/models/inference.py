"""Batched network evaluation for play, search and self-play.

On a GPU the whole forward (uint8 planes -> padded NHWC bf16 -> L x MFMA conv
-> fused head/softmax with legal-move renormalisation) is captured once per
batch bucket into a HIP graph (torch.cuda.CUDAGraph is hipGraph on ROCm) and
replayed: a search step is one H2D copy, one graph launch and one D2H copy,
instead of ~15 kernel launches.  Batches are padded up to the next bucket.

With a feature list, ``evaluate_encoded`` takes the engine's compact board
encoding (~2 bytes/point, ``Forest.leaf_encode_into`` / ``encode_batch``)
instead of uint8 planes: the GPU featurizer (ops/gpu_features.py) runs as the
first node of the same graph, writing the conv input and the sensible-move
mask directly (24x less H2D traffic than 48 uint8 planes, no CPU featurizing).

Symmetry ensembling (``symmetries="random"`` / ``"all"``): a position is evaluated under G of the 8
board symmetries (G = 1 drawn per board per submission, or all 8) and the outputs are mapped back to
the board's own frame and averaged.  Symmetry s is ``pack_input``'s (``train/engine.symmetry_tables``):
policy = 1/G sum_g P_s[fwd_s(p)], value = 1/G sum_g V(board under s).  A bucket of B positions then
owns a trunk batch of G*B boards, board g*B + b being position b under symmetry sym[g*B + b]; the conv
input is fanned out on the device (``pack_input`` with rows / sym, or ``d4_expand`` after the
featurizer, which still runs once per position), the head folds the G outputs back inside one kernel
(``policy_head_probs_d4`` / ``group_mean``), all in the same captured graph.  Masks, planes and the
overflow list stay in the original frame.  Memory: an ``"all"`` bucket holds 8x the activations of a
plain one -- a 1024-position bucket is an 8192-board trunk, about 2.8 GB per slot at 19x19x192 --
so buckets stay lazy.  ``"none"`` (the default) is the plain single-orientation path, unchanged.

Reference paths replaced: CNNPolicy.forward / batch_eval_state
(policy.py:26-79) which featurised in Python and ran a Theano function per
call; MCTS policy/value callables (mcts.py:107-118).
"""
from __future__ import annotations

import os
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .. import ops
from .nets import PolicyNet, PolicyValueNet, ValueNet

DEFAULT_BUCKETS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)

SYMMETRY_MODES = ("none", "random", "all")


def _check_symmetries(mode: str) -> str:
    if mode not in SYMMETRY_MODES:
        raise ValueError("symmetries must be one of %s, not %r" % (", ".join(SYMMETRY_MODES), mode))
    return mode


class _Bucket:
    pass


class Fp8LayerPlan(NamedTuple):
    """What one layer of the fp8 trunk writes and adds (fp8_trunk_plan): indices into a bucket's buffers."""
    y_bf16: Optional[int]  # bf16 output buffer (bk.Y) or None
    y_fp8: Optional[int]   # e4m3 output buffer (bk.Y8) or None; layer l + 1 reads it
    res: Optional[int]     # bf16 buffer (bk.Y) holding the skip operand of a block end, or None


def fp8_trunk_plan(layers: int, residual: bool) -> List[Fp8LayerPlan]:
    """Per-layer outputs and skip operand of the fp8 inference trunk (HipTrunkInference._trunk_fp8).

    Every layer but the top writes e4m3 into Y8[l % 2] for the next one; the top writes bf16 only, for the
    heads.  A plain trunk writes no other bf16.  A residual trunk keeps its stream in bf16: the even layers
    (the stem and every block end) also write bf16, into Y[(l // 2) % 2], and a block end (even l >= 2) adds
    the stream written two layers earlier, Y[((l - 2) // 2) % 2] -- the other buffer of the pair, so the
    skip is never an output of its own launch, the top layer included."""
    plan = []
    for l in range(layers):
        last = l == layers - 1
        stream = residual and l % 2 == 0
        yb = (l // 2) % 2 if stream else (0 if last else None)
        res = ((l - 2) // 2) % 2 if stream and l >= 2 else None
        plan.append(Fp8LayerPlan(yb, None if last else l % 2, res))
    return plan


class HipTrunkInference:
    """Forward-only runner of a ConvStack (+ head) on the HIP kernels."""

    def __init__(self, net, device, buckets: Sequence[int] = DEFAULT_BUCKETS, use_graphs: bool = True,
                 feature_list: Optional[Sequence[str]] = None, precision: Optional[str] = None,
                 symmetries: str = "none", symmetry_seed: int = 0):
        self.symmetries = _check_symmetries(symmetries)
        self.G = 8 if symmetries == "all" else 1  # orientations per position
        self._sym = symmetries != "none"
        self._rng = np.random.default_rng(symmetry_seed)
        self._last_sub = None  # (bucket, n) of the last submission
        ops.load()
        self.net = net
        self.precision = precision or os.environ.get("ALPHAGO_AMD_PRECISION", "bf16")
        if self.precision not in ("bf16", "fp8"):
            raise ValueError("precision must be bf16 or fp8")
        self.device = torch.device(device)
        tr = net.trunk
        # residual trunk: the skip-add rides in the conv epilogue (conv_planned / conv_fwd_fp8 res=); three Y
        # buffers in rotation instead of two, so the block input outlives the block's first layer.  The fp8
        # kernels take the skip on the 192-wide tile only (fp8_trunk_plan: the stream stays bf16)
        self.residual = bool(getattr(tr, "residual", False))
        if self.residual and self.precision == "fp8" and ops.pad_filters(tr.filters) != 192:
            raise ValueError("a residual trunk of %d filters runs in bf16 only: the fp8 conv kernels have their "
                             "skip operand on the 192-wide tile alone (precision=\"fp8\" argument or "
                             "ALPHAGO_AMD_PRECISION=fp8)" % tr.filters)
        # global pooling branches (ConvStack gpool), bf16 trunk: after the first layer l of a branch block the
        # bucket's gpool_fwd / dense_f32 / gpool_bias_add add the gate g[b, c] in place to the block's skip buffer
        # Y[(l-1) % 3], which nothing reads after the block's last layer
        self.gpool_blocks = list(getattr(tr, "gpool_blocks", ()))
        if self.gpool_blocks and self.precision == "fp8":
            raise ValueError("a trunk with global pooling branches (gpool=%d) runs in bf16 only: the fp8 trunk keeps "
                             "no bf16 output of a block's first layer to pool (precision=\"fp8\" argument or "
                             "ALPHAGO_AMD_PRECISION=fp8)" % tr.gpool)
        self._gp_layer = {2 * j + 1: i for i, j in enumerate(self.gpool_blocks)}  # pooled layer -> branch
        self.gpool_w = None
        self._ny = 3 if self.residual else 2
        self.S, self.L, self.K = net.board, tr.layers, list(tr.widths)
        self.C0, self.F = tr.in_planes, tr.filters
        self.C0p = ops.round_up(self.C0, 64)
        self.Fp = ops.pad_filters(self.F)
        self.P0 = self.K[0] // 2
        self.buckets = sorted(buckets)
        self.use_graphs = use_graphs
        # fp8 engines run buckets below this many boards on the bf16 trunk: the fp8 forward's 384-pixel
        # tiles leave a small batch with a handful of workgroups (~480 us per policy forward at B <= 64 vs
        # 185-325 us bf16; even at B = 128, 520 / 451 us vs 515 / 427 bf16 for policy / value; fp8 wins
        # from B = 256 on, 578 / 488 us vs 817 / 702; profiles/r4/README.md); ALPHAGO_AMD_FP8_MIN_BATCH
        # overrides
        self.fp8_min_batch = int(os.environ.get("ALPHAGO_AMD_FP8_MIN_BATCH", "256"))
        dev = self.device
        # packed on the engine's device whatever device the module's parameters are on
        self.cin_p = [self.C0p] + [self.Fp] * (self.L - 1)  # padded input channels of each layer
        self.wf = [ops.packed_weight_like(tr.weights[l], self.cin_p[l], self.Fp, device=dev) for l in range(self.L)]
        # weight-stationary copies (tile 40, small buckets) of the layers that kernel covers, whatever
        # buckets come later
        self.wf_ws = [ops.ws_packed_like(self.wf[l]) if ops.conv_ws_supported(self.Fp, self.cin_p[l], self.K[l])
                      else None for l in range(self.L)]
        self.bias_p = [torch.zeros(self.Fp, device=dev) for _ in range(self.L)]
        self.head_w = torch.zeros(self.F, device=dev)
        self.head_b = torch.zeros(1, device=dev)
        self._b: Dict[int, _Bucket] = {}
        if self.precision == "fp8":
            L = self.L
            self.w8: List[torch.Tensor] = [None] * L
            self.ew = [0] * L
            self.ex = [0] * (L + 1)  # e4m3 exponent of each layer's input (layer 0: binary planes, exact at 0)
            self.scales8 = torch.full((L, 2), 127, dtype=torch.int32, device=dev)
            self.osc8 = torch.ones(L, device=dev)
            self.amax8 = ops.fp8_amax_buffer(L, dev)
            self.calibrated = False
        # encoded path: also write the uint8 planes of every board into the bucket (RL learner records
        # stay on the device, search/selfplay.py); toggled before capture (set_encoded_planes)
        self.encoded_planes = False
        self._last_bk = None
        self.fz = None
        if feature_list is not None:
            from ..ops.gpu_features import GpuFeaturizer
            fz = GpuFeaturizer(feature_list, board=self.S, device=dev)
            if fz.nplanes != self.C0:
                raise ValueError("feature list has %d planes, network expects %d" % (fz.nplanes, self.C0))
            self.fz = fz
        self.sync_weights()

    @property
    def supports_encoded(self) -> bool:
        return self.fz is not None

    @property
    def needs_ladder(self) -> bool:
        """Whether callers must encode ladder bits on the host (False when the
        GPU featurizer reads ladders on the device)."""
        return self.fz is not None and self.fz.host_needs_ladder

    @torch.no_grad()
    def sync_weights(self) -> None:
        """Re-read the module's parameters into the engine's device copies.

        Contract: no device tensor that a captured graph reads is ever rebound.  A bucket's graph holds
        the addresses of ``wf``, ``wf_ws``, ``bias_p``, ``head_w``, ``head_b``, ``gpool_w``, ``w8``, ``scales8``,
        ``osc8`` (and a subclass's own weights, ``_after_sync``) from the moment it is captured, so a
        refresh writes into those tensors in place; a tensor bound to a fresh allocation here would
        leave every captured bucket replaying the old weights out of freed memory."""
        tr = self.net.trunk
        ws = [w.detach().to(self.device, torch.float32).contiguous() for w in tr.weights]
        ops.pack_weights(ws, self.wf)
        ops.ws_pack([self.wf[l] for l in range(self.L) if self.wf_ws[l] is not None],
                    [w for w in self.wf_ws if w is not None])
        for l in range(self.L):
            self.bias_p[l][:self.F].copy_(tr.biases[l].detach())
        self.head_w.copy_(self.net.head_w.detach().view(-1))
        self.head_b.copy_(self.net.head_b.detach().view(-1))
        if self.gpool_blocks:
            F, Fp = self.F, self.Fp
            if self.gpool_w is None:  # allocated once; zero-padded (2 Fp, Fp): padded channels get g = 0
                self.gpool_w = [torch.zeros(2 * Fp, Fp, device=self.device) for _ in self.gpool_blocks]
            for dst, g in zip(self.gpool_w, tr.gpool_w):
                dst[:F, :F].copy_(g.detach()[:F])
                dst[Fp:Fp + F, :F].copy_(g.detach()[F:])
        if self.precision == "fp8":
            for l in range(self.L):
                w8, self.ew[l] = ops.pack_weights_fp8(ws[l], self.Fp, self.cin_p[l])
                if self.w8[l] is None:
                    self.w8[l] = w8
                else:  # captured fp8 graphs read this buffer
                    self.w8[l].copy_(w8)
                self.scales8[l, 1] = 127 - self.ew[l]
            self.calibrated = False  # activation ranges change with the weights
        self._after_sync()

    def _after_sync(self):
        pass

    def bucket_for(self, n: int) -> int:
        for b in self.buckets:
            if b >= n:
                return b
        return ops.round_up(n, self.buckets[-1])

    def _make_bucket(self, B: int) -> _Bucket:
        dev, S = self.device, self.S
        bk = _Bucket()
        bk.B = B
        Bt = bk.Bt = B * self.G  # trunk batch: every position under its G symmetries
        bk.planes = torch.zeros((B, self.C0, S, S), dtype=torch.uint8, device=dev)
        bk.legal = torch.ones((B, S * S), dtype=torch.uint8, device=dev)
        bk.X0 = ops.padded_empty(Bt, S, self.P0, self.C0p, dev)
        bk.Y = [ops.padded_empty(Bt, S, 1, self.Fp, dev) for _ in range(self._ny)]
        if self._sym:
            # trunk board g * B + b is position b under sym[g * B + b]; "random" refills sym per submission
            bk.sym = torch.arange(self.G, dtype=torch.int32, device=dev).repeat_interleave(B) if self.G > 1 \
                else torch.zeros(Bt, dtype=torch.int32, device=dev)
            bk.rows = torch.arange(Bt, dtype=torch.int64, device=dev) % B
            bk.last_sym = np.zeros(B, dtype=np.int32)
            if self.fz is not None:  # the featurizer's single-orientation output, fanned out by d4_expand
                bk.X0f = ops.padded_empty(B, S, self.P0, self.C0p, dev)
        # small buckets (ops.plan_conv): the weight-stationary kernel (tile 40) where it applies, else the
        # split-K 32-pixel conv (ops.conv_fwd_splitk), fp32 partials in bk.ws; not the buckets an fp8
        # engine runs in fp8 (their bf16 calibration forward runs the plain tiles)
        M = Bt * S * S
        small = self.precision != "fp8" or Bt < self.fp8_min_batch
        bk.plan = [ops.plan_conv(M, self.Fp, c, K, small=small) for c, K in zip(self.cin_p, self.K)]
        n = ops.splitk_workspace_numel(bk.plan, M, self.Fp)
        bk.ws = torch.empty(n, device=dev) if n else None
        if self.gpool_blocks:  # one set per bucket, shared by its branch blocks
            bk.gp_P = torch.zeros(Bt, 2, self.Fp, device=dev)
            bk.gp_arg = torch.zeros(Bt, self.Fp, dtype=torch.int32, device=dev)
            bk.gp_g = torch.zeros(Bt, self.Fp, device=dev)
        if self.precision == "fp8":
            bk.X08 = torch.zeros(bk.X0.shape, dtype=torch.uint8, device=dev)
            bk.Y8 = [torch.zeros(bk.Y[0].shape, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._alloc_outputs(bk)
        bk.graph = None
        bk.graph_enc = None
        if self.fz is not None:
            NP = S * S
            bk.e_board = torch.zeros((B, NP), dtype=torch.int8, device=dev)
            bk.e_ages = torch.full((B, NP), 255, dtype=torch.uint8, device=dev)
            bk.e_meta = torch.tensor([[-1, 1]] * B, dtype=torch.int32, device=dev)
            bk.e_ladder = torch.zeros((B, NP), dtype=torch.uint8, device=dev) if self.fz.need_ladder else None
            bk.ovf = torch.zeros((B,), dtype=torch.int32, device=dev)
        return bk

    def _alloc_outputs(self, bk):
        bk.probs = torch.zeros((bk.B, self.S * self.S), device=self.device)
        # "all": per-orientation rows for the head's small-batch path (ops.policy_head_probs_d4)
        bk.probs_g = torch.zeros((bk.Bt, self.S * self.S), device=self.device) if self.G > 1 else None

    def set_encoded_planes(self, on: bool) -> None:
        """Make the encoded path also write uint8 planes (``encoded_planes_view``); re-captures graphs."""
        if bool(on) != self.encoded_planes:
            self.encoded_planes = bool(on)
            for bk in self._b.values():
                bk.graph_enc = None

    def encoded_planes_view(self, n: int) -> torch.Tensor:
        """(n, C, S, S) uint8 device planes of the last encoded submission (valid until the bucket is
        submitted again); needs ``set_encoded_planes(True)``."""
        if not self.encoded_planes or self._last_bk is None:
            raise RuntimeError("encoded planes are off")
        return self._last_bk.planes[:n]

    def _trunk(self, bk, encoded: bool = False) -> torch.Tensor:
        if encoded:
            bk.ovf.zero_()
            self.fz.run(bk.e_board, bk.e_ages, bk.e_meta, bk.e_ladder, nhwc=bk.X0f if self._sym else bk.X0, P=self.P0,
                        sensible=bk.legal, overflow=bk.ovf, planes=bk.planes if self.encoded_planes else None)
            if self._sym:
                ops.d4_expand(bk.X0f, bk.X0, bk.sym, self.S, self.P0)
        elif self._sym:
            ops.pack_input(bk.planes, bk.X0, self.P0, sym=bk.sym, rows=bk.rows)
        else:
            ops.pack_input(bk.planes, bk.X0, self.P0)
        if self.precision == "fp8" and not getattr(self, "_calibrating", False) and bk.Bt >= self.fp8_min_batch:
            return self._trunk_fp8(bk)
        x, pin = bk.X0, self.P0
        for l in range(self.L):
            y = bk.Y[l % self._ny]
            # residual trunk: layer l's input is Y[(l-1) % 3] and a block end's skip Y[(l-2) % 3], so the
            # skip is never the buffer being written
            res = bk.Y[(l - 2) % 3] if self.residual and l >= 2 and l % 2 == 0 else None
            ops.conv_planned(bk.plan[l], x, self.wf[l], self.wf_ws[l], self.bias_p[l], y, self.K[l], self.S, pin,
                             sk_ws=bk.ws, res=res)
            if getattr(self, "_calibrating", False):
                self._cal_amax[l] = max(self._cal_amax[l], float(y.amax()))
            if l in self._gp_layer:  # the block's skip Y[(l-1) % 3] += g, before layer l + 1 reads it as res
                ops.gpool_fwd(y, bk.gp_P, bk.gp_arg, self.S)
                ops.dense_f32(bk.gp_P.view(bk.Bt, -1), self.gpool_w[self._gp_layer[l]], bk.gp_g)
                ops.gpool_bias_add(bk.Y[(l - 1) % 3], bk.gp_g, bk.Y[(l - 1) % 3], self.S)
            x, pin = y, 1
        return x

    # ------------------------------------------------------------------ fp8
    def _trunk_fp8(self, bk) -> torch.Tensor:
        """e4m3 trunk on the block-scaled MFMA: every layer reads and (but the
        last) writes e4m3 activations; the last writes bf16 for the head.  A residual trunk also keeps
        its stream in bf16 and adds it in the block ends' epilogues (fp8_trunk_plan)."""
        ops.quantize_fp8(bk.X0, bk.X08, 0)  # 0/1 planes are exact in e4m3
        x8, pin = bk.X08, self.P0
        yb = None
        for l, p in enumerate(fp8_trunk_plan(self.L, self.residual)):
            yb = None if p.y_bf16 is None else bk.Y[p.y_bf16]
            y8 = None if p.y_fp8 is None else bk.Y8[p.y_fp8]
            ops.conv_fwd_fp8(x8, self.w8[l], self.bias_p[l], self.scales8[l], self.osc8[l:l + 1], self.K[l], self.S,
                             pin, 1, y_bf16=yb, y_fp8=y8, amax=self.amax8[l],
                             res=None if p.res is None else bk.Y[p.res])
            x8, pin = y8, 1
        return yb

    @torch.no_grad()
    def calibrate(self, bk, encoded: bool = False, margin: int = 1) -> None:
        """Set per-layer e4m3 activation scales from a bf16 forward of the
        current bucket inputs (delayed scaling afterwards: recalibrate())."""
        self._cal_amax = [0.0] * self.L
        self._calibrating = True
        try:
            self._trunk(bk, encoded)
        finally:
            self._calibrating = False
        self._set_act_exponents([ops.fp8_exponent(a, margin) for a in self._cal_amax])
        self.calibrated = True

    def recalibrate(self, margin: int = 1) -> None:
        """Re-derive activation scales from the running amax tracked by the fp8 kernels."""
        amax = self.amax8.view(torch.float32).amax(1).tolist()
        self._set_act_exponents([ops.fp8_exponent(a, margin) for a in amax])

    def _set_act_exponents(self, out_exp) -> None:
        self.ex = [0] + list(out_exp)
        for l in range(self.L):
            self.scales8[l, 0] = 127 - self.ex[l]
            self.osc8[l] = 2.0 ** self.ex[l + 1]

    def _head(self, bk, y):
        if self._sym:
            ops.policy_head_probs_d4(y, self.head_w, self.head_b, bk.probs, self.S, bk.sym, self.G, legal=bk.legal,
                                     scratch=bk.probs_g)
        else:
            ops.policy_head_probs(y, self.head_w, self.head_b, bk.probs, self.S, legal=bk.legal)

    def _draw_symmetries(self, bk, n: int) -> None:
        """Per-submission part of the symmetry modes: "random" draws one symmetry per board on the host
        and queues its copy with the other inputs (padding boards keep whatever they had)."""
        self._last_sub = (bk, n)
        if self.symmetries == "random":
            bk.last_sym = self._rng.integers(0, 8, size=n, dtype=np.int32)
            bk.sym[:n].copy_(torch.from_numpy(bk.last_sym), non_blocking=True)

    def last_symmetries(self, handle=None) -> np.ndarray:
        """Symmetries of the last submission (or of ``handle``'s bucket, valid until it is submitted
        again): int32 (n,) -- zeros for "none", the draw for "random" -- or (8, n) for "all", row g
        holding g."""
        if handle is not None:
            bk, n = handle[0], handle[1]
        elif self._last_sub is not None:
            bk, n = self._last_sub
        else:
            raise RuntimeError("nothing submitted yet")
        if self.symmetries == "random":
            return bk.last_sym[:n].copy()
        if self.symmetries == "all":
            return np.repeat(np.arange(8, dtype=np.int32)[:, None], n, 1)
        return np.zeros(n, dtype=np.int32)

    def _run(self, bk, encoded: bool = False):
        self._head(bk, self._trunk(bk, encoded))

    def _capture(self, bk, encoded: bool):
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            self._run(bk, encoded)  # warm-up (also sets kernel attributes outside capture)
        torch.cuda.current_stream(self.device).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._run(bk, encoded)
        return g

    def _get(self, n: int, encoded: bool = False, slot: int = 0) -> _Bucket:
        B = self.bucket_for(n)
        key = (B, slot)
        if key not in self._b:
            self._b[key] = self._make_bucket(B)
        bk = self._b[key]
        if self.use_graphs:
            if encoded and bk.graph_enc is None:
                bk.graph_enc = self._capture(bk, True)
            elif not encoded and bk.graph is None:
                bk.graph = self._capture(bk, False)
        return bk

    @torch.no_grad()
    def submit_encoded(self, board, ages, meta, ladder=None, slot: int = 0, to_host: bool = False):
        """Asynchronous half of evaluate_encoded: H2D copies (non-blocking from
        pinned host buffers) + graph replay on the current stream; with
        ``to_host`` also the D2H copy of the results into pinned host buffers,
        followed by an event.  ``slot`` selects an independent set of bucket
        buffers, so two batches can be in flight; the GPU work stays serial on
        one stream (two overlapping batches would delay each other's results).
        Returns a handle for collect()."""
        assert self.fz is not None, "engine built without a feature list"
        n = board.shape[0]
        bk = self._get(n, encoded=True, slot=slot)
        bk.e_board[:n].copy_(torch.as_tensor(board), non_blocking=True)
        bk.e_ages[:n].copy_(torch.as_tensor(ages), non_blocking=True)
        bk.e_meta[:n].copy_(torch.as_tensor(meta), non_blocking=True)
        if bk.e_ladder is not None and self.fz.host_needs_ladder:
            if ladder is None:
                raise ValueError("this feature list needs ladder bits")
            bk.e_ladder[:n].copy_(torch.as_tensor(ladder), non_blocking=True)
        if n < bk.B:
            bk.e_board[n:].zero_()
            bk.e_ages[n:].fill_(255)
        self._draw_symmetries(bk, n)
        if self.precision == "fp8" and not self.calibrated:
            self.calibrate(bk, encoded=True)
        if bk.graph_enc is not None:
            bk.graph_enc.replay()
        else:
            self._run(bk, True)
        self._last_bk = bk
        host = None
        if to_host:
            if not hasattr(bk, "h_out"):
                out = self._outputs(bk, bk.B)
                bk.h_out = torch.empty(out.shape, dtype=torch.float32, pin_memory=True)
                bk.h_mask = torch.empty(bk.legal.shape, dtype=torch.uint8, pin_memory=True)
                bk.h_ovf = torch.empty(bk.ovf.shape, dtype=torch.int32, pin_memory=True)
            bk.h_out[:n].copy_(self._outputs(bk, n), non_blocking=True)
            bk.h_mask[:n].copy_(bk.legal[:n], non_blocking=True)
            bk.h_ovf[:n].copy_(bk.ovf[:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            host = ev
        return bk, n, host

    def collect(self, handle):
        """(outputs (n, ...), sensible mask (n, S*S), overflow board indices).
        For a to_host submission: numpy views of the pinned host buffers (valid
        until the slot is submitted again), waiting only for that batch's event."""
        bk, n, ev = handle
        if ev is not None:
            ev.synchronize()
            bad = np.nonzero(bk.h_ovf[:n].numpy())[0].tolist()
            return bk.h_out[:n].numpy(), bk.h_mask[:n].numpy(), bad
        bad = torch.nonzero(bk.ovf[:n]).flatten().tolist()
        return self._outputs(bk, n), bk.legal[:n], bad

    def outputs(self, handle):
        """Device views (outputs (n, ...), sensible mask (n, S*S) uint8) of a submission, no waiting."""
        bk, n, _ = handle
        return self._outputs(bk, n), bk.legal[:n]

    @torch.no_grad()
    def evaluate_encoded(self, board, ages, meta, ladder=None, slot: int = 0):
        """Forward from the compact encoding (GPU featurizer in the graph).

        Returns (outputs (n, ...), sensible mask (n, S*S) uint8 device tensor,
        list of board indices whose eye recursion overflowed the kernel and
        must be re-evaluated from CPU planes)."""
        return self.collect(self.submit_encoded(board, ages, meta, ladder, slot))

    @torch.no_grad()
    def evaluate(self, planes, legal=None, slot: int = 0):
        """planes: (n, C, S, S) uint8 (numpy or tensor); legal: (n, S*S) uint8 or None.
        Returns the bucket's output tensors (views of the first n rows).  ``slot`` selects the
        bucket buffers as in submit_encoded (a caller with encoded batches in flight uses a slot
        none of them holds)."""
        n = planes.shape[0]
        bk = self._get(n, encoded=False, slot=slot)
        src = torch.as_tensor(planes)
        bk.planes[:n].copy_(src, non_blocking=True)
        if n < bk.B:
            bk.planes[n:].zero_()
        if legal is not None:
            bk.legal[:n].copy_(torch.as_tensor(legal), non_blocking=True)
            if n < bk.B:
                bk.legal[n:].fill_(1)
        else:
            bk.legal.fill_(1)
        self._draw_symmetries(bk, n)
        if self.precision == "fp8" and not self.calibrated:
            self.calibrate(bk)
        if bk.graph is not None:
            bk.graph.replay()
        else:
            self._run(bk)
        return self._outputs(bk, n)

    def _outputs(self, bk, n):
        return bk.probs[:n]


class HipValueInference(HipTrunkInference):
    """Value net: HIP trunk, then the head as head_logits (1x1 conv) -> dense_f32
    (Dense 256, fp32 MFMA GEMM) -> value_out (Dense 1 + tanh), all inside the
    captured graph."""

    def __init__(self, net: ValueNet, device, **kw):
        self.fc = None
        super().__init__(net, device, **kw)

    def _after_sync(self):
        n = self.net
        src = [t.detach() for t in (n.fc1_w, n.fc1_b, n.fc2_w, n.fc2_b)]
        if self.fc is None:  # allocated once: the captured dense_f32 / value_out read these addresses
            self.fc = [torch.empty(t.shape, dtype=torch.float32, device=self.device) for t in src]
        for dst, t in zip(self.fc, src):
            dst.copy_(t)

    def _alloc_outputs(self, bk):
        bk.values = torch.zeros((bk.B,), device=self.device)
        bk.z = torch.zeros((bk.Bt, self.S * self.S), device=self.device)
        bk.h = torch.zeros((bk.Bt, self.fc[0].shape[1]), device=self.device)
        if self.G > 1:  # the G values of every position, averaged by group_mean
            bk.values_g = torch.zeros((bk.Bt,), device=self.device)

    def _head(self, bk, y):
        w1, b1, w2, b2 = self.fc
        ops.head_logits(y, self.head_w, self.head_b, bk.z, self.S)
        ops.dense_f32(bk.z, w1, bk.h, bias=b1)
        if self.G > 1:
            ops.value_out(bk.h, w2.view(-1), b2, bk.values_g)
            ops.group_mean(bk.values_g, bk.values, self.G)
        else:  # "random": the value of the one drawn orientation is the output
            ops.value_out(bk.h, w2.view(-1), b2, bk.values)

    def _outputs(self, bk, n):
        return bk.values[:n]


class HipPolicyValueInference(HipTrunkInference):
    """Dual net: HIP trunk, then both heads from one read of its output -- policy_value_head (the
    policy head's masked softmax and the value head's 1x1 conv) -> dense_f32 -> value_out, all inside
    the captured graph.

    The outputs of a bucket are one (B, S*S + 1) row per position, the move probabilities followed by
    the value, so that ``submit_encoded(to_host=True)`` / ``collect`` (the base class's, unchanged)
    bring both to the host in one copy behind one event; ``split_outputs`` takes such rows apart.
    ``evaluate`` returns the pair (probs (n, S*S), values (n,)).  No symmetry ensembling yet.

    ``ownership=True`` (a net with the ownership head only; off by default, so search does not pay for
    it): ``policy_value_own_head`` takes the place of ``policy_value_head`` and also fills the bucket's
    ``own`` (B, S*S), tanh of the third head in the mover's frame.  The output rows stay (B, S*S + 1);
    ``ownership_view`` gives the device rows of a submission.

    A net with the pass head (``pass_head=1``): per bucket ``gpool_fwd`` pools the trunk output and
    ``policy_value_pass_head`` takes the head's place (with ``ownership=True`` it fills ``own`` too), both
    inside the captured graph.  The output rows are (B, S*S + 2), the S*S + 1 probabilities (the pass last)
    and the value; ``split_outputs`` and ``evaluate`` return ``probs`` of shape (n, S*S + 1).  ``pass_head``
    on the engine tells search to take the pass prior from the last column.

    ``score=True`` (a net with the score head only; off by default): per bucket, inside the captured graph,
    ``gpool_fwd`` (the pass head's, run once for both), ``dense_f32`` (upre = P sc1_w + sc1_b) and ``score_out``
    in forward mode fill the bucket's ``score`` (B,) in units of S points; ``score_view`` gives the device rows
    of a submission in points, in the mover's frame, komi included.

    ``score_utility = lam > 0`` implies ``score=True``; the value column of the output rows then holds the
    utility (v + lam * tanh(score / (2 S))) / (1 + lam), still in [-1, 1], written by ``score_out`` on the device
    inside the graph, so the search and the C++ forest need no change.  Root values and the resign threshold
    then speak of this utility, not of the win/loss value.  ``lam`` has no tuned value.  With ``lam`` = 0
    nothing extra is launched and the rows keep their bits."""

    dual = True

    def __init__(self, net: PolicyValueNet, device, ownership: bool = False, score: bool = False,
                 score_utility: float = 0.0, **kw):
        if kw.get("symmetries", "none") != "none":
            raise ValueError("the dual (policy + value) engine does not ensemble over symmetries yet: "
                             "symmetries must be \"none\", not %r" % (kw["symmetries"],))
        if ownership and not getattr(net, "ownership", False):
            raise ValueError("ownership=True needs a PolicyValueNet with the ownership head (ownership=1)")
        self.score_utility, self.score = _check_score_options(net, score, score_utility)
        self.ownership = bool(ownership)
        self.pass_head = bool(getattr(net, "pass_head", False))
        self.vhead = None
        self.ohead = None
        self.phead = None
        self.shead = None
        super().__init__(net, device, **kw)

    def _after_sync(self):
        n = self.net
        src = [n.vhead_w.detach().view(-1), n.vhead_b.detach().view(-1)] + \
              [t.detach() for t in (n.fc1_w, n.fc1_b, n.fc2_w, n.fc2_b)]
        if self.vhead is None:  # allocated once: the captured head kernels read these addresses
            self.vhead = [torch.empty(t.shape, dtype=torch.float32, device=self.device) for t in src]
        for dst, t in zip(self.vhead, src):
            dst.copy_(t)
        if self.ownership:
            osrc = [n.ohead_w.detach().view(-1), n.ohead_b.detach().view(-1)]
            if self.ohead is None:
                self.ohead = [torch.empty(t.shape, dtype=torch.float32, device=self.device) for t in osrc]
            for dst, t in zip(self.ohead, osrc):
                dst.copy_(t)
        if self.pass_head:
            if self.phead is None:  # [pass_w zero-padded (2, Fp), pass_b (1)], allocated once
                self.phead = [torch.zeros(2, self.Fp, device=self.device), torch.zeros(1, device=self.device)]
            self.phead[0][:, :self.F].copy_(n.pass_w.detach().view(2, self.F))
            self.phead[1].copy_(n.pass_b.detach().view(-1))
        if self.score:
            if self.shead is None:  # [sc1_w zero-padded (2 Fp, D), sc1_b (D), sc2_w (D), sc2_b (1)], allocated once
                D = n.score_dense
                self.shead = [torch.zeros(2 * self.Fp, D, device=self.device), torch.zeros(D, device=self.device),
                              torch.zeros(D, device=self.device), torch.zeros(1, device=self.device)]
            w1 = n.sc1_w.detach()
            self.shead[0][:self.F].copy_(w1[:self.F])
            self.shead[0][self.Fp:self.Fp + self.F].copy_(w1[self.F:])
            self.shead[1].copy_(n.sc1_b.detach().view(-1))
            self.shead[2].copy_(n.sc2_w.detach().view(-1))
            self.shead[3].copy_(n.sc2_b.detach().view(-1))

    @property
    def NE(self) -> int:
        """Entries of a probability row: S*S, with the pass head S*S + 1."""
        return self.S * self.S + (1 if self.pass_head else 0)

    def _alloc_outputs(self, bk):
        SS = self.S * self.S
        bk.probs = torch.zeros((bk.B, self.NE), device=self.device)
        if self.pass_head or self.score:
            bk.ps_P = torch.zeros((bk.B, 2, self.Fp), device=self.device)
            bk.ps_arg = torch.zeros((bk.B, self.Fp), dtype=torch.int32, device=self.device)
        if self.score:
            bk.sc_up = torch.zeros((bk.B, self.shead[1].numel()), device=self.device)
            bk.score = torch.zeros((bk.B,), device=self.device)
        bk.z = torch.zeros((bk.B, SS), device=self.device)
        if self.ownership:
            bk.own = torch.zeros((bk.B, SS), device=self.device)
        bk.h = torch.zeros((bk.B, self.vhead[2].shape[1]), device=self.device)
        bk.values = torch.zeros((bk.B,), device=self.device)
        bk.out = torch.zeros((bk.B, self.NE + 1), device=self.device)

    def _head(self, bk, y):
        vw, vb, w1, b1, w2, b2 = self.vhead
        NE = self.NE
        if self.pass_head:
            ops.gpool_fwd(y, bk.ps_P, bk.ps_arg, self.S)
            own = dict(wo=self.ohead[0], bo=self.ohead[1], own=bk.own) if self.ownership else {}
            ops.policy_value_pass_head(y, self.head_w, self.head_b, vw, vb, bk.ps_P, self.phead[0], self.phead[1],
                                       bk.probs, bk.z, self.S, legal=bk.legal, **own)
        elif self.ownership:
            ops.policy_value_own_head(y, self.head_w, self.head_b, vw, vb, self.ohead[0], self.ohead[1], bk.probs,
                                      bk.z, bk.own, self.S, legal=bk.legal)
        else:
            ops.policy_value_head(y, self.head_w, self.head_b, vw, vb, bk.probs, bk.z, self.S, legal=bk.legal)
        ops.dense_f32(bk.z, w1, bk.h, bias=b1)
        ops.value_out(bk.h, w2.view(-1), b2, bk.values)
        if self.score:
            if not self.pass_head:
                ops.gpool_fwd(y, bk.ps_P, bk.ps_arg, self.S)
            ops.dense_f32(bk.ps_P.view(bk.B, -1), self.shead[0], bk.sc_up, bias=self.shead[1])
            util = dict(value=bk.values, utility=self.score_utility) if self.score_utility else {}
            ops.score_out(bk.sc_up, self.shead[2], self.shead[3], bk.score, **util)
        bk.out[:, :NE].copy_(bk.probs)
        bk.out[:, NE].copy_(bk.values)

    def _outputs(self, bk, n):
        return bk.out[:n]

    def split_outputs(self, out):
        """(probs (n, S*S), with the pass head (n, S*S + 1), values (n,)) views of output rows (device tensor
        or collect()'s numpy)."""
        NE = self.NE
        return out[:, :NE], out[:, NE]

    def ownership_view(self, handle=None):
        """Device rows (n, S*S) of the ownership head for the last submission (or ``handle``'s bucket,
        valid until it is submitted again), in the mover's frame."""
        if not self.ownership:
            raise RuntimeError("this engine was built without ownership=True")
        if handle is not None:
            bk, n = handle[0], handle[1]
        elif self._last_sub is not None:
            bk, n = self._last_sub
        else:
            raise RuntimeError("nothing submitted yet")
        return bk.own[:n]

    def score_view(self, handle=None):
        """Device rows (n,) of the score head for the last submission (or ``handle``'s bucket, valid until it is
        submitted again): points in the mover's frame, komi included."""
        if not self.score:
            raise RuntimeError("this engine was built without score=True")
        if handle is not None:
            bk, n = handle[0], handle[1]
        elif self._last_sub is not None:
            bk, n = self._last_sub
        else:
            raise RuntimeError("nothing submitted yet")
        return bk.score[:n] * float(self.S)

    @torch.no_grad()
    def evaluate(self, planes, legal=None, slot: int = 0):
        """As HipTrunkInference.evaluate; returns (probs (n, S*S), with the pass head (n, S*S + 1), values (n,))."""
        return self.split_outputs(super().evaluate(planes, legal, slot))


def _check_score_options(net, score, score_utility):
    """(lam, score) of the dual engines' ``score`` / ``score_utility`` options: a utility implies the score."""
    lam = float(score_utility)
    if lam < 0:
        raise ValueError("score_utility must be >= 0, not %r" % (score_utility,))
    score = bool(score) or lam > 0
    if score and not getattr(net, "score_head", False):
        raise ValueError("score=True / score_utility > 0 need a PolicyValueNet with the score head (score_head=1)")
    return lam, score


class _TorchSymmetries:
    """The symmetry modes of the torch engines: the module docstring's definition in plain torch
    (index tables from ``train/engine.symmetry_tables``)."""

    def _init_symmetries(self, symmetries: str, symmetry_seed: int) -> None:
        self.symmetries = _check_symmetries(symmetries)
        self.G = 8 if symmetries == "all" else 1
        self._rng = np.random.default_rng(symmetry_seed)
        self._last_sym = None
        self._table = None

    def _draw(self, n: int) -> torch.Tensor:
        """(G, n) long symmetries of this submission."""
        if self.symmetries == "all":
            sym = np.repeat(np.arange(8, dtype=np.int32)[:, None], n, 1)
            self._last_sym = sym
        elif self.symmetries == "random":
            self._last_sym = self._rng.integers(0, 8, size=n, dtype=np.int32)
            sym = self._last_sym[None]
        else:
            self._last_sym = np.zeros(n, dtype=np.int32)
            sym = self._last_sym[None]
        return torch.as_tensor(sym, device=self.device).long()

    def _tables(self, sym_row: torch.Tensor):
        """fwd, inv (n, S*S): transformed[fwd[p]] = original[p]; transformed = original.gather(inv)."""
        if self._table is None:
            from ..train.engine import symmetry_tables
            self._table = symmetry_tables(self.net.board, self.device)
        fwd = self._table[sym_row]
        return fwd, torch.argsort(fwd, dim=1)

    @staticmethod
    def _transform(x: torch.Tensor, inv: torch.Tensor) -> torch.Tensor:
        n, C, S, _ = x.shape
        return torch.gather(x.reshape(n, C, S * S), 2, inv.unsqueeze(1).expand(n, C, S * S)).reshape(n, C, S, S)

    def last_symmetries(self, handle=None) -> np.ndarray:
        """As HipTrunkInference.last_symmetries."""
        if self._last_sym is None:
            raise RuntimeError("nothing submitted yet")
        return self._last_sym.copy()


class TorchPolicyInference(_TorchSymmetries):
    """CPU / reference path with the same interface."""

    supports_encoded = False
    needs_ladder = False

    def __init__(self, net: PolicyNet, device="cpu", symmetries: str = "none", symmetry_seed: int = 0):
        self.net, self.device = net, torch.device(device)
        self._init_symmetries(symmetries, symmetry_seed)

    def sync_weights(self):
        pass

    def _plain(self, x, legal):
        logits = self.net.logits_torch(x.float())
        if legal is not None:
            logits = logits.masked_fill(legal == 0, float("-inf"))
        p = torch.softmax(logits, 1)
        return torch.nan_to_num(p, nan=0.0)

    @torch.no_grad()
    def evaluate(self, planes, legal=None, slot: int = 0):
        x = torch.as_tensor(planes).to(self.device)
        if legal is not None:
            legal = torch.as_tensor(legal).to(self.device)
        sym = self._draw(x.shape[0])
        if self.symmetries == "none":
            return self._plain(x, legal)
        acc = None
        for g in range(self.G):  # fixed g order, fp32
            fwd, inv = self._tables(sym[g])
            p = self._plain(self._transform(x, inv), legal.gather(1, inv) if legal is not None else None)
            p = p.gather(1, fwd)  # back to the original frame: P_s[fwd_s(p)]
            acc = p if acc is None else acc + p
        return acc * (1.0 / self.G)


class TorchValueInference(_TorchSymmetries):
    supports_encoded = False
    needs_ladder = False

    def __init__(self, net: ValueNet, device="cpu", symmetries: str = "none", symmetry_seed: int = 0):
        self.net, self.device = net, torch.device(device)
        self._init_symmetries(symmetries, symmetry_seed)

    def sync_weights(self):
        pass

    @torch.no_grad()
    def evaluate(self, planes, legal=None, slot: int = 0):
        x = torch.as_tensor(planes).to(self.device)
        sym = self._draw(x.shape[0])
        if self.symmetries == "none":
            return self.net.forward_torch(x.float())
        acc = None
        for g in range(self.G):
            v = self.net.forward_torch(self._transform(x, self._tables(sym[g])[1]).float())
            acc = v if acc is None else acc + v
        return acc * (1.0 / self.G)


class TorchPolicyValueInference:
    """CPU / fp32 oracle of the dual net: TorchPolicyInference._plain's and TorchValueInference's op
    sequences on one shared trunk output.  ``evaluate`` returns (probs (n, S*S), values (n,)); with the pass
    head the rows have S*S + 1 entries, the pass last and always legal.  ``score`` / ``score_utility`` as on
    HipPolicyValueInference: ``score_view`` in points, the value column as the utility when ``lam`` > 0."""

    supports_encoded = False
    needs_ladder = False
    dual = True
    symmetries = "none"

    def __init__(self, net: PolicyValueNet, device="cpu", symmetries: str = "none", symmetry_seed: int = 0,
                 ownership: bool = False, score: bool = False, score_utility: float = 0.0):
        if _check_symmetries(symmetries) != "none":
            raise ValueError("the dual (policy + value) engine does not ensemble over symmetries yet: "
                             "symmetries must be \"none\", not %r" % (symmetries,))
        if ownership and not getattr(net, "ownership", False):
            raise ValueError("ownership=True needs a PolicyValueNet with the ownership head (ownership=1)")
        self.net, self.device = net, torch.device(device)
        self.ownership = bool(ownership)
        self.pass_head = bool(getattr(net, "pass_head", False))
        self.score_utility, self.score = _check_score_options(net, score, score_utility)
        self._own = None
        self._score = None

    def sync_weights(self):
        pass

    def ownership_view(self, handle=None):
        """(n, S*S) ownership rows of the last evaluate, in the mover's frame."""
        if not self.ownership:
            raise RuntimeError("this engine was built without ownership=True")
        if self._own is None:
            raise RuntimeError("nothing submitted yet")
        return self._own

    def score_view(self, handle=None):
        """(n,) score rows of the last evaluate: points in the mover's frame, komi included."""
        if not self.score:
            raise RuntimeError("this engine was built without score=True")
        if self._score is None:
            raise RuntimeError("nothing submitted yet")
        return self._score

    @torch.no_grad()
    def evaluate(self, planes, legal=None, slot: int = 0):
        x = torch.as_tensor(planes).to(self.device)
        if self.ownership or self.score:
            h = self.net.trunk.forward_torch(x.float())
            logits, values = self.net.heads_torch(h)
            if self.ownership:
                self._own = self.net.ownership_torch(h)
            if self.score:
                self._score = self.net.score_torch(h)
                if self.score_utility:
                    lam = self.score_utility
                    values = (values + lam * torch.tanh(self._score / (2.0 * self.net.board))) / (1.0 + lam)
        else:
            logits, values = self.net.logits_value_torch(x.float())
        if legal is not None:
            legal = torch.as_tensor(legal).to(self.device)
            if self.pass_head:  # (n, S*S + 1) logits: the pass is always legal
                legal = torch.cat([legal, torch.ones_like(legal[:, :1])], 1)
            logits = logits.masked_fill(legal == 0, float("-inf"))
        return torch.nan_to_num(torch.softmax(logits, 1), nan=0.0), values


def _torch_kw(kw):
    """The engine keywords the torch engines take too (feature_list etc. are unused: CPU featurizer path)."""
    return {k: v for k, v in kw.items() if k in ("symmetries", "symmetry_seed", "ownership", "score", "score_utility")}


def make_policy_inference(net, device, **kw):
    """HIP engine on a GPU (pass ``feature_list`` to enable evaluate_encoded), torch on CPU;
    ``symmetries`` ("none" / "random" / "all") and ``symmetry_seed`` apply to both."""
    device = torch.device(device)
    if device.type == "cuda":
        return HipTrunkInference(net, device, **kw)
    return TorchPolicyInference(net, device, **_torch_kw(kw))


def make_value_inference(net, device, **kw):
    device = torch.device(device)
    if device.type == "cuda":
        return HipValueInference(net, device, **kw)
    return TorchValueInference(net, device, **_torch_kw(kw))


def make_policy_value_inference(net, device, **kw):
    """The dual net's engine: HIP on a GPU, torch on CPU.  ``symmetries`` other than "none" raises."""
    device = torch.device(device)
    if device.type == "cuda":
        return HipPolicyValueInference(net, device, **kw)
    return TorchPolicyValueInference(net, device, **_torch_kw(kw))
