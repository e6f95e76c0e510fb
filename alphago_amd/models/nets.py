"""Network definitions: policy CNN and value CNN.

Architecture parity with the reference Keras builders:

* policy (AlphaGo/models/policy.py:93-156): Conv(k1=5, F, ReLU, same) ->
  (layers-1) x Conv(k=3 or filter_width_K, F, ReLU, same) -> Conv(1x1, 1, linear,
  scalar bias) -> Flatten -> Softmax over S*S.  Defaults board=19, F=128,
  layers=12, Keras ``uniform`` init (U(-0.05, 0.05), zero bias).
* value (AlphaGo/models/value.py:12-31): 49 planes, Conv 5x5 K=152 ReLU,
  11 x Conv 3x3 ReLU, Conv 1x1 linear, Flatten, Dense(256, linear), Dense(1, tanh).

Parameters are kept as fp32 master tensors in PyTorch OIHW cross-correlation
layout.  Execution goes through one of two backends:

* ``"hip"`` — the MI355X path: hand-written CDNA4 kernels in
  ``alphago_amd.ops`` (implicit-GEMM conv on MFMA over zero-padded NHWC bf16,
  fused bias+ReLU epilogues, fused head/softmax/CE).
* ``"torch"`` — plain ``torch.nn.functional`` (the fp32 numerics oracle; also
  the CPU path).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

KERAS_UNIFORM_SCALE = 0.05


def keras_uniform_(t: torch.Tensor, scale: float = KERAS_UNIFORM_SCALE, generator=None) -> torch.Tensor:
    with torch.no_grad():
        return t.uniform_(-scale, scale, generator=generator)


def he_uniform_(net: nn.Module, generator=None) -> nn.Module:
    """Fan-in scaled uniform init (He for the ReLU trunk and the 1x1 head conv, LeCun for the dense
    layers) of a PolicyNet / ValueNet, biases zero: the reference's ``uniform(-0.05, 0.05)`` shrinks a
    12-layer trunk's signal ~30x (value.py:17,21), which plain SGD does not recover from.

    A residual trunk gets the Fixup rule for two-layer branches: the first conv of each block its He bound
    times ``n_blocks ** -0.5``, the second conv of each block zero; the stem and the heads as above.  With
    the zero biases every block is then the identity on its (non-negative) input, so the trunk's output
    equals the stem's exactly.  The gates of the pooling branches (``trunk.gpool_w``) are the last linear
    map of their branch and get zero by the same rule: right after this init the net computes exactly what
    the same net without ``gpool`` computes."""
    with torch.no_grad():
        residual = getattr(net.trunk, "residual", False)
        n_blocks = (net.trunk.layers - 1) // 2
        for l, w in enumerate(list(net.trunk.weights) + [net.head_w]):
            bound = (6.0 / (w.shape[1] * w.shape[2] * w.shape[3])) ** 0.5
            if residual and 0 < l < net.trunk.layers:
                if l % 2 == 0:  # block end
                    w.zero_()
                    continue
                bound *= n_blocks ** -0.5
            w.uniform_(-bound, bound, generator=generator)
        vh = getattr(net, "vhead_w", None)  # PolicyValueNet's second 1x1 head
        if vh is not None:
            bound = (6.0 / (vh.shape[1] * vh.shape[2] * vh.shape[3])) ** 0.5
            vh.uniform_(-bound, bound, generator=generator)
        for name in ("fc1_w", "fc2_w"):  # Keras (in, out) layout: fan_in = rows
            w = getattr(net, name, None)
            if w is not None:
                bound = (3.0 / w.shape[0]) ** 0.5
                w.uniform_(-bound, bound, generator=generator)
        oh = getattr(net, "ohead_w", None)  # the ownership head, like vhead_w; drawn last, so that the other
        if oh is not None:                  # tensors get the values they get in a net without it
            bound = (6.0 / (oh.shape[1] * oh.shape[2] * oh.shape[3])) ** 0.5
            oh.uniform_(-bound, bound, generator=generator)
        for g in getattr(net.trunk, "gpool_w", ()):
            g.zero_()
        if getattr(net, "pass_head", False):  # the last linear map of its branch: the pass logit starts at pass_b
            net.pass_w.zero_()
        if getattr(net, "score_head", False):
            # the ReLU layer gets its He bound (Keras layout: fan_in = rows), drawn last of all, so that the other
            # tensors get the values they get in a net without the head; the output layer gets zero: a fresh head
            # predicts sc2_b = 0 and sends no gradient into the trunk
            bound = (3.0 / net.sc1_w.shape[0]) ** 0.5
            net.sc1_w.uniform_(-bound, bound, generator=generator)
            net.sc2_w.zero_()
    return net


def first_argmax(z: torch.Tensor) -> torch.Tensor:
    """(B,) smallest index among each row's maxima."""
    n = z.shape[1]
    idx = torch.arange(n, device=z.device).expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, idx, torch.full_like(idx, n)).min(1).values


def gpool_blocks(layers: int, k: int) -> List[int]:
    """Blocks j = 0 .. n_blocks - 1 of a residual trunk that carry a pooling branch: (j + 1) % k == 0."""
    return [j for j in range((layers - 1) // 2) if (j + 1) % k == 0] if k else []


class ConvStack(nn.Module):
    """Shared trunk: conv(k_1) + (L-1) conv(k_i), all ReLU, 'same' padding.

    ``residual``: layer 0 is the stem and layers 1..L-1 form blocks of two, (1, 2), (3, 4), ...; the last
    layer of a block adds the block's input before its ReLU, ``Y[l] = relu(conv_l(Y[l-1]) + b_l + Y[l-2])``
    for even ``l >= 2``.  Parameter names, shapes and order are those of the plain stack.

    ``gpool = k >= 1`` (residual trunks only): block j (layers l = 2j + 1 and l + 1) has a global pooling
    branch when ``(j + 1) % k == 0``.  With NP = S * S,

        P[b, 0, c] = (sum_p Y[l][b, p, c]) * float32(1 / NP)
        P[b, 1, c] = max_p Y[l][b, p, c]          (ties: the lowest pixel index r * S + col)
        g[b, :]    = P[b].reshape(2F) @ Wg_j      (Wg_j (2F, F), Keras Dense layout, no bias)
        Y[l+1]     = relu(conv_{l+1}(Y[l]) + b_{l+1} + (Y[l-1] + g[b]))

    ``gpool_w`` holds one ``Wg_j`` per branch block, in block order."""

    def __init__(self, in_planes: int, filters: int, layers: int, widths: List[int], residual: bool = False,
                 gpool: int = 0):
        super().__init__()
        assert len(widths) == layers
        if residual and (layers < 3 or layers % 2 == 0):
            lo = max(3, layers - 1 if layers % 2 == 0 else layers)
            raise ValueError("a residual trunk is a stem plus whole two-layer blocks: layers must be odd and "
                             ">= 3, not %d (nearest valid depths: %d and %d)" % (layers, lo, max(lo + 2, layers + 1)))
        self.residual = bool(residual)
        gpool = int(gpool)
        n_blocks = (layers - 1) // 2
        if gpool and not residual:
            raise ValueError("gpool=%d needs a residual trunk (residual=1): the pooling branch adds to a block's "
                             "skip; valid choices: residual=1 with gpool in 1..n_blocks, or no gpool" % gpool)
        if gpool and not 1 <= gpool <= n_blocks:
            raise ValueError("gpool=%d: a branch in every gpool-th block needs 1 <= gpool <= n_blocks = %d "
                             "(valid choices: %s)" % (gpool, n_blocks, ", ".join(map(str, range(1, n_blocks + 1)))))
        self.gpool = gpool
        self.gpool_blocks = gpool_blocks(layers, gpool)
        for w in widths:
            if w % 2 != 1:
                raise ValueError("filter widths must be odd")
        self.in_planes, self.filters, self.layers, self.widths = in_planes, filters, layers, list(widths)
        self.weights = nn.ParameterList()
        self.biases = nn.ParameterList()
        cin = in_planes
        for w in widths:
            self.weights.append(nn.Parameter(torch.empty(filters, cin, w, w)))
            self.biases.append(nn.Parameter(torch.zeros(filters)))
            cin = filters
        self.reset_parameters()

    def init_gpool(self, generator=None) -> None:
        """Create and draw the gates of the pooling branches.  The owning net calls it after it has drawn
        every other parameter, so those get the values they get without ``gpool``."""
        if self.gpool:
            self.gpool_w = nn.ParameterList(nn.Parameter(torch.empty(2 * self.filters, self.filters))
                                            for _ in self.gpool_blocks)
            for g in self.gpool_w:
                keras_uniform_(g, generator=generator)

    def reset_parameters(self, generator=None):
        for w in self.weights:
            keras_uniform_(w, generator=generator)
        for b in self.biases:
            nn.init.zeros_(b)

    def forward_torch(self, x: torch.Tensor) -> torch.Tensor:
        skip = None  # the current block's input (residual trunks)
        for l, (w, b, k) in enumerate(zip(self.weights, self.biases, self.widths)):
            z = F.conv2d(x, w.to(x.dtype), b.to(x.dtype), padding=k // 2)
            if self.residual and l % 2 == 0:  # the stem, or a block's last layer: the next block's input
                x = skip = F.relu(z if l == 0 else z + skip)
            else:
                x = F.relu(z)
                if self.gpool and (l - 1) // 2 in self.gpool_blocks:  # the block's pooling branch joins its skip
                    skip = skip + self.gate_torch(x, self.gpool_blocks.index((l - 1) // 2))[:, :, None, None]
        return x

    def gate_torch(self, y: torch.Tensor, i: int) -> torch.Tensor:
        """(B, F) gate of branch ``i`` from a block's first-layer output ``y`` (B, F, S, S): mean and max over
        the board (the max gathered at the lowest pixel index attaining it, which pins its gradient), then
        the dense layer ``gpool_w[i]``."""
        B, C = y.shape[:2]
        flat = y.reshape(B * C, -1)
        mean = flat.sum(1) * torch.tensor(1.0 / flat.shape[1], dtype=torch.float32).to(y.dtype)
        mx = flat.gather(1, first_argmax(flat.detach())[:, None])[:, 0]
        return torch.cat([mean.view(B, C), mx.view(B, C)], 1) @ self.gpool_w[i].to(y.dtype)


class PolicyNet(nn.Module):
    """SL/RL policy network (reference CNNPolicy.create_network)."""

    def __init__(self, input_dim: int, board: int = 19, filters_per_layer: int = 128, layers: int = 12,
                 **kwargs):
        super().__init__()
        widths = [int(kwargs.get("filter_width_%d" % i, 5 if i == 1 else 3)) for i in range(1, layers + 1)]
        self.arch = dict(input_dim=input_dim, board=board, filters_per_layer=filters_per_layer, layers=layers)
        for i, w in enumerate(widths, 1):
            if (i == 1 and w != 5) or (i > 1 and w != 3):
                self.arch["filter_width_%d" % i] = w
        self.board = board
        self.trunk = ConvStack(input_dim, filters_per_layer, layers, widths)
        self.head_w = nn.Parameter(torch.empty(1, filters_per_layer, 1, 1))
        self.head_b = nn.Parameter(torch.zeros(1))
        keras_uniform_(self.head_w)

    @property
    def input_dim(self):
        return self.arch["input_dim"]

    def logits_torch(self, x: torch.Tensor) -> torch.Tensor:
        h = self.trunk.forward_torch(x)
        z = F.conv2d(h, self.head_w.to(h.dtype), self.head_b.to(h.dtype))
        return z.flatten(1).float()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, C, S, S) float/uint8 planes -> (B, S*S) move probabilities."""
        if x.dtype == torch.uint8:
            x = x.float()
        return torch.softmax(self.logits_torch(x), dim=1)

    def flops_per_position(self) -> float:
        """Forward FLOPs per board (2*MACs), exact for stride-1 'same' convs."""
        s2 = self.board * self.board
        tot = 0.0
        cin = self.trunk.in_planes
        for k in self.trunk.widths:
            tot += 2.0 * s2 * cin * self.trunk.filters * k * k
            cin = self.trunk.filters
        tot += 2.0 * s2 * cin
        return tot


class ValueNet(nn.Module):
    """Value network (reference value.py:12-31) with a tanh scalar output."""

    def __init__(self, input_dim: int = 49, board: int = 19, filters_per_layer: int = 152, layers: int = 12,
                 dense: int = 256, **kwargs):
        super().__init__()
        widths = [int(kwargs.get("filter_width_%d" % i, 5 if i == 1 else 3)) for i in range(1, layers + 1)]
        self.arch = dict(input_dim=input_dim, board=board, filters_per_layer=filters_per_layer, layers=layers,
                         dense=dense)
        self.board = board
        self.trunk = ConvStack(input_dim, filters_per_layer, layers, widths)
        self.head_w = nn.Parameter(torch.empty(1, filters_per_layer, 1, 1))
        self.head_b = nn.Parameter(torch.zeros(1))
        self.fc1_w = nn.Parameter(torch.empty(board * board, dense))  # Keras Dense layout (in, out)
        self.fc1_b = nn.Parameter(torch.zeros(dense))
        self.fc2_w = nn.Parameter(torch.empty(dense, 1))
        self.fc2_b = nn.Parameter(torch.zeros(1))
        for p in (self.head_w, self.fc1_w, self.fc2_w):
            keras_uniform_(p)

    @property
    def input_dim(self):
        return self.arch["input_dim"]

    def flops_per_position(self) -> float:
        """Forward FLOPs per board (2*MACs): trunk, 1x1 head conv, Dense(S*S -> dense), Dense(dense -> 1)."""
        s2 = self.board * self.board
        tot, cin = 0.0, self.trunk.in_planes
        for k in self.trunk.widths:
            tot += 2.0 * s2 * cin * self.trunk.filters * k * k
            cin = self.trunk.filters
        d = self.arch["dense"]
        return tot + 2.0 * s2 * cin + 2.0 * s2 * d + 2.0 * d

    def forward_torch(self, x: torch.Tensor) -> torch.Tensor:
        h = self.trunk.forward_torch(x)
        z = F.conv2d(h, self.head_w.to(h.dtype), self.head_b.to(h.dtype)).flatten(1).float()
        z = z @ self.fc1_w + self.fc1_b  # linear (value.py:27)
        return torch.tanh(z @ self.fc2_w + self.fc2_b).squeeze(1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dtype == torch.uint8:
            x = x.float()
        return self.forward_torch(x)


class PolicyValueNet(nn.Module):
    """Dual-head network: one ConvStack, the policy head of PolicyNet (1x1 conv, softmax over S*S)
    and the value head of ValueNet (1x1 conv, Dense(dense, linear), Dense(1, tanh)) on its output.
    Reads the value net's planes (49 with ``color``).  ``residual``: a residual trunk (ConvStack), kept in
    ``arch`` only when set; ``layers`` must then be odd.  ``ownership``: a third 1x1 head (``ohead_w``,
    ``ohead_b``) with a tanh per board point, the owner of the point at the end of the game in the
    mover's frame (+1 = the player to move); kept in ``arch`` only when set.  ``gpool = k``: a global pooling
    branch in every k-th block of a residual trunk (ConvStack; ``trunk.gpool_w``), kept in ``arch`` only when
    set.

    ``pass_head``: a learned pass logit next to the S*S board logits (``pass_w`` (2F, 1) in the Keras Dense
    layout, ``pass_b`` (1)), kept in ``arch`` only when set.  With h = Y[L-1] the trunk output after its ReLU,
    NP = S * S and inv = float32(1 / NP):

        P[b, 0, c] = (sum_p h[b, p, c]) * inv
        P[b, 1, c] = max_p h[b, p, c]             (ties: the lowest pixel index, which pins the gradient)
        z_pass[b]  = P[b].reshape(2F) @ pass_w + pass_b
        z[b]       = [1x1 policy head logits (NP), z_pass[b]]     (NP + 1 entries, the pass last)

    ``pass_w`` is drawn after every other parameter (``trunk.gpool_w`` included) and zeroed by ``he_uniform_``;
    a net without the head draws what it always drew.

    ``score_head``: an estimate of the score lead of the player to move (``sc1_w`` (2F, D), ``sc1_b`` (D),
    ``sc2_w`` (D, 1), ``sc2_b`` (1), Keras Dense layouts, D = ``score_dense``), kept in ``arch`` only when set
    (``score_dense`` only when it is not 64).  With P the pooled vector above:

        u[b]     = relu(P[b].reshape(2F) @ sc1_w + sc1_b)
        s[b]     = u[b] @ sc2_w + sc2_b
        score[b] = S * s[b]                       (points, mover's frame, komi included)

    The unit of ``s`` (S points, 19 on a 19 x 19 board) is a definition, chosen so that ``s`` is O(1).  The four
    tensors are drawn after every other parameter (``pass_w`` included); ``he_uniform_`` draws ``sc1_w`` at its
    He bound, last of all, and zeroes ``sc2_w``: a fresh head predicts ``sc2_b`` = 0 and sends no gradient into
    the trunk."""

    def __init__(self, input_dim: int = 49, board: int = 19, filters_per_layer: int = 192, layers: int = 12,
                 dense: int = 256, residual: int = 0, ownership: int = 0, gpool: int = 0, pass_head: int = 0,
                 score_head: int = 0, score_dense: int = 64, **kwargs):
        super().__init__()
        widths = [int(kwargs.get("filter_width_%d" % i, 5 if i == 1 else 3)) for i in range(1, layers + 1)]
        self.arch = dict(input_dim=input_dim, board=board, filters_per_layer=filters_per_layer, layers=layers,
                         dense=dense)
        for i, w in enumerate(widths, 1):
            if (i == 1 and w != 5) or (i > 1 and w != 3):
                self.arch["filter_width_%d" % i] = w
        if residual:
            self.arch["residual"] = 1
        if ownership:
            self.arch["ownership"] = 1
        if gpool:
            self.arch["gpool"] = int(gpool)
        if pass_head:
            self.arch["pass_head"] = 1
        self.pass_head = bool(pass_head)
        self.score_head = bool(score_head)
        self.score_dense = int(score_dense)
        if score_head:
            if self.score_dense % 8 or not 8 <= self.score_dense <= 512:
                raise ValueError("score_dense must be a multiple of 8 in 8..512, not %d" % self.score_dense)
            self.arch["score_head"] = 1
            if self.score_dense != 64:
                self.arch["score_dense"] = self.score_dense
        self.ownership = bool(ownership)
        self.board = board
        self.trunk = ConvStack(input_dim, filters_per_layer, layers, widths, residual=bool(residual),
                               gpool=int(gpool))
        self.head_w = nn.Parameter(torch.empty(1, filters_per_layer, 1, 1))
        self.head_b = nn.Parameter(torch.zeros(1))
        self.vhead_w = nn.Parameter(torch.empty(1, filters_per_layer, 1, 1))
        self.vhead_b = nn.Parameter(torch.zeros(1))
        self.fc1_w = nn.Parameter(torch.empty(board * board, dense))  # Keras Dense layout (in, out)
        self.fc1_b = nn.Parameter(torch.zeros(dense))
        self.fc2_w = nn.Parameter(torch.empty(dense, 1))
        self.fc2_b = nn.Parameter(torch.zeros(1))
        for p in (self.head_w, self.vhead_w, self.fc1_w, self.fc2_w):
            keras_uniform_(p)
        if ownership:  # after the others: they draw what they draw without the head
            self.ohead_w = nn.Parameter(torch.empty(1, filters_per_layer, 1, 1))
            self.ohead_b = nn.Parameter(torch.zeros(1))
            keras_uniform_(self.ohead_w)
        self.trunk.init_gpool()  # after every other parameter: they draw what they draw without the branch
        if pass_head:  # last of all, for the same reason
            self.pass_w = nn.Parameter(torch.empty(2 * filters_per_layer, 1))
            self.pass_b = nn.Parameter(torch.zeros(1))
            keras_uniform_(self.pass_w)
        if score_head:  # after the pass head: every other tensor draws what it draws without the score head
            self.sc1_w = nn.Parameter(torch.empty(2 * filters_per_layer, self.score_dense))
            self.sc1_b = nn.Parameter(torch.zeros(self.score_dense))
            self.sc2_w = nn.Parameter(torch.empty(self.score_dense, 1))
            self.sc2_b = nn.Parameter(torch.zeros(1))
            keras_uniform_(self.sc1_w)
            keras_uniform_(self.sc2_w)

    @property
    def input_dim(self):
        return self.arch["input_dim"]

    def flops_per_position(self) -> float:
        """Forward FLOPs per board (2*MACs): the trunk once, both 1x1 head convs and the two dense layers."""
        s2 = self.board * self.board
        tot, cin = 0.0, self.trunk.in_planes
        for k in self.trunk.widths:
            tot += 2.0 * s2 * cin * self.trunk.filters * k * k
            cin = self.trunk.filters
        d = self.arch["dense"]
        tot += len(self.trunk.gpool_blocks) * 2.0 * 2 * cin * cin  # the gates: Dense(2F -> F) per branch block
        if self.pass_head:
            tot += 2.0 * 2 * cin  # the pass logit: Dense(2F -> 1)
        if self.score_head:  # Dense(2F -> D) with its bias, the ReLU'd Dense(D -> 1) with its bias
            sd = self.score_dense
            tot += 2.0 * 2 * cin * sd + sd + 2.0 * sd + 1
        return tot + (3 if self.ownership else 2) * (2.0 * s2 * cin) + 2.0 * s2 * d + 2.0 * d

    @staticmethod
    def pooled_torch(h: torch.Tensor) -> torch.Tensor:
        """(B, 2F) mean and max of the trunk output (B, F, S, S) over the board, the max gathered at the lowest
        pixel index attaining it: fp32 sums of a bf16 trunk, fp64 when given fp64."""
        B, C = h.shape[:2]
        flat = h.reshape(B * C, -1)
        flat = flat if flat.dtype == torch.float64 else flat.float()  # fp32 sums of a bf16 trunk; an fp64 oracle stays fp64
        mean = flat.sum(1) * torch.tensor(1.0 / flat.shape[1], dtype=torch.float32).to(flat.dtype)
        mx = flat.gather(1, first_argmax(flat.detach())[:, None])[:, 0]
        return torch.cat([mean.view(B, C), mx.view(B, C)], 1)

    def pass_logit_torch(self, h: torch.Tensor) -> torch.Tensor:
        """(B,) pass logit from the trunk output (B, F, S, S): mean and max over the board (the max gathered at
        the lowest pixel index attaining it), then the dense layer ``pass_w``, ``pass_b``."""
        if not self.pass_head:
            raise ValueError("this PolicyValueNet has no pass head (pass_head=1)")
        P = self.pooled_torch(h)
        return (P @ self.pass_w.to(P.dtype)).squeeze(1) + self.pass_b.to(P.dtype)

    def score_torch(self, h: torch.Tensor) -> torch.Tensor:
        """(B,) score lead of the player to move in points (komi included) from the trunk output (B, F, S, S):
        the pass head's pooling, Dense(2F -> D) + ReLU, Dense(D -> 1), times S."""
        if not self.score_head:
            raise ValueError("this PolicyValueNet has no score head (score_head=1)")
        P = self.pooled_torch(h)
        u = torch.relu(P @ self.sc1_w.to(P.dtype) + self.sc1_b.to(P.dtype))
        return ((u @ self.sc2_w.to(P.dtype)).squeeze(1) + self.sc2_b.to(P.dtype)) * self.board

    def policy_logits_torch(self, h: torch.Tensor) -> torch.Tensor:
        """Policy logits from the trunk output, in its dtype: (B, S*S) of the 1x1 head, with the pass head
        (B, S*S + 1) with the pass logit last."""
        z = F.conv2d(h, self.head_w.to(h.dtype), self.head_b.to(h.dtype)).flatten(1)
        if self.pass_head:
            z = torch.cat([z, self.pass_logit_torch(h).to(z.dtype)[:, None]], 1)
        return z

    def heads_torch(self, h: torch.Tensor):
        """(policy logits (B, S*S), value (B,)) from the trunk output: PolicyNet.logits_torch's and
        ValueNet.forward_torch's op sequences.  With the pass head the logits are (B, S*S + 1), the pass
        last."""
        z = self.policy_logits_torch(h).float()
        zv = F.conv2d(h, self.vhead_w.to(h.dtype), self.vhead_b.to(h.dtype)).flatten(1).float()
        zv = zv @ self.fc1_w + self.fc1_b
        return z, torch.tanh(zv @ self.fc2_w + self.fc2_b).squeeze(1)

    def ownership_torch(self, h: torch.Tensor) -> torch.Tensor:
        """(B, S*S) ownership in the mover's frame from the trunk output: tanh of the third 1x1 conv."""
        if not self.ownership:
            raise ValueError("this PolicyValueNet has no ownership head (ownership=1)")
        o = F.conv2d(h, self.ohead_w.to(h.dtype), self.ohead_b.to(h.dtype)).flatten(1)
        return torch.tanh(o if o.dtype == torch.float64 else o.float())  # fp32 from a bf16 trunk; an fp64 oracle stays fp64

    def logits_value_torch(self, x: torch.Tensor):
        return self.heads_torch(self.trunk.forward_torch(x))

    def forward(self, x: torch.Tensor):
        """x: (B, C, S, S) float/uint8 planes -> (probs (B, S*S), or (B, S*S + 1) with the pass head, value (B,))."""
        if x.dtype == torch.uint8:
            x = x.float()
        z, v = self.logits_value_torch(x)
        return torch.softmax(z, dim=1), v
