"""CNNPolicy / CNNValue: reference-compatible model wrappers.

API parity with the reference CNNPolicy (AlphaGo/models/policy.py:12-193):
``CNNPolicy(feature_list, **arch)``, ``.forward``, ``.eval_state``,
``.batch_eval_state``, ``create_network``, ``load_model``, ``save_model``,
``.model``, ``.preprocessor``.  The network is a torch module; evaluation runs
through :mod:`alphago_amd.models.inference` (HIP graphs on the GPU, torch on
CPU).  Featurisation is native C++ (batched, multithreaded).
"""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from ..features import DEFAULT_FEATURES, VALUE_FEATURES, Preprocess
from ..io import keras_compat
from ..utils.gorecords import flatten_idx
from .inference import (SYMMETRY_MODES, make_policy_inference, make_policy_value_inference,
                        make_value_inference)
from .nets import PolicyNet, PolicyValueNet, ValueNet


def default_device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


class _NetWrapper(object):
    _net_cls = PolicyNet

    def __init__(self, feature_list: Sequence[str], device=None, **kwargs):
        self.preprocessor = Preprocess(feature_list)
        kwargs["input_dim"] = self.preprocessor.output_dim
        self.device = torch.device(device) if device is not None else default_device()
        self.model = self.create_network(**kwargs).to(self.device)
        self._engine = None
        self._symmetries, self._symmetry_seed = "none", 0

    @classmethod
    def create_network(cls, **kwargs):
        return cls._net_cls(**kwargs)

    def _engine_kw(self):
        """GPU engines get the feature list so they can featurize on the device."""
        kw = {"symmetries": self._symmetries, "symmetry_seed": self._symmetry_seed}
        if self.device.type == "cuda" and self.preprocessor.output_dim <= 64:
            kw["feature_list"] = self.preprocessor.feature_list
        return kw

    def set_symmetries(self, mode: str, seed: int = 0) -> None:
        """Evaluate under board symmetries from now on: "none", "random" (one drawn per board per
        batch, generator seeded by ``seed``) or "all" (the mean over all 8); see models/inference.py.
        The engine is rebuilt on its next use."""
        if mode not in SYMMETRY_MODES:
            raise ValueError("symmetries must be one of %s, not %r" % (", ".join(SYMMETRY_MODES), mode))
        self._symmetries, self._symmetry_seed = mode, int(seed)
        self._engine = None

    @property
    def engine(self):
        if self._engine is None:
            self._engine = self._make_engine()
        return self._engine

    def refresh(self) -> None:
        """Re-read weights into the inference engine after training updates."""
        if self._engine is not None:
            self._engine.sync_weights()

    # ---------------------------------------------------------- persistence
    def save_model(self, json_file: str, weights_file: Optional[str] = None) -> None:
        specs = {"keras_model": keras_compat.model_to_keras_json(self.model),
                 "feature_list": self.preprocessor.feature_list}
        if weights_file is not None:
            keras_compat.save_weights(self.model, weights_file)
            specs["weights_file"] = weights_file
        with open(json_file, "w") as f:
            json.dump(specs, f)

    @classmethod
    def load_model(cls, json_file: str, device=None, weights_file: Optional[str] = None, symmetries: str = "none"):
        with open(json_file, "r") as f:
            specs = json.load(f)
        obj = cls.__new__(cls)
        obj.preprocessor = Preprocess(specs["feature_list"])
        obj.device = torch.device(device) if device is not None else default_device()
        net = cls._net_from_specs(specs)
        if not isinstance(net, cls._net_cls):
            raise ValueError("%s expects a %s spec" % (cls.__name__, cls._net_cls.__name__))
        obj.model = net.to(obj.device)
        obj._engine = None
        obj.set_symmetries(symmetries)
        wf = weights_file or specs.get("weights_file")
        if wf:
            if not os.path.isabs(wf) and not os.path.exists(wf):
                wf = os.path.join(os.path.dirname(os.path.abspath(json_file)), wf)
            keras_compat.load_weights(obj.model, wf)
        return obj

    @classmethod
    def _net_from_specs(cls, specs):
        if "keras_model" not in specs:  # e.g. a dual net's file ("pv_model"): not this wrapper's
            raise ValueError("%s expects a %s spec" % (cls.__name__, cls._net_cls.__name__))
        return keras_compat.model_from_keras_json(specs["keras_model"])

    def load_weights(self, weights_file: str) -> None:
        keras_compat.load_weights(self.model, weights_file)
        self.refresh()

    def save_weights(self, weights_file: str) -> None:
        keras_compat.save_weights(self.model, weights_file)


class CNNPolicy(_NetWrapper):
    """Policy network: state -> distribution over moves."""

    _net_cls = PolicyNet

    def __init__(self, feature_list: Sequence[str] = DEFAULT_FEATURES, device=None, **kwargs):
        super().__init__(feature_list, device=device, **kwargs)

    def _make_engine(self):
        return make_policy_inference(self.model, self.device, **self._engine_kw())

    def forward(self, planes, legal=None) -> np.ndarray:
        """(B, F, S, S) planes -> (B, S*S) probabilities (numpy)."""
        planes = np.asarray(planes)
        if planes.dtype != np.uint8:
            planes = planes.astype(np.uint8)
        return self.engine.evaluate(planes, legal).float().cpu().numpy()

    def batch_eval_state(self, states, moves_lists=None):
        """One batched forward for all states; returns [(move, prob), ...] per state
        renormalised over the given (default: legal) moves (policy.py:44-79)."""
        n = len(states)
        if n == 0:
            return []
        size = states[0].size
        if any(st.size != size for st in states):
            raise ValueError("all states must have the same size")
        planes = self.preprocessor.states_to_uint8(states)
        probs = self.forward(planes)
        moves_lists = moves_lists or [st.get_legal_moves() for st in states]
        return [self._select(probs[i], moves_lists[i], size) for i in range(n)]

    def eval_state(self, state, moves=None):
        return self.batch_eval_state([state], [moves] if moves is not None else None)[0]

    @staticmethod
    def _select(dist, moves, size):
        if not moves:
            return []
        idx = [flatten_idx(m, size) for m in moves]
        d = dist[idx].astype(np.float64)
        s = d.sum()
        d = d / s if s > 0 else np.full(len(idx), 1.0 / len(idx))
        return list(zip(moves, d))


class CNNValue(_NetWrapper):
    """Value network (reference value.py): state -> expected outcome in [-1, 1]
    for the player to move."""

    _net_cls = ValueNet

    def __init__(self, feature_list: Sequence[str] = VALUE_FEATURES, device=None, **kwargs):
        super().__init__(feature_list, device=device, **kwargs)

    def _make_engine(self):
        return make_value_inference(self.model, self.device, **self._engine_kw())

    def forward(self, planes) -> np.ndarray:
        planes = np.asarray(planes).astype(np.uint8, copy=False)
        return self.engine.evaluate(planes).float().cpu().numpy()

    def batch_eval_state(self, states) -> List[float]:
        if not states:
            return []
        return [float(v) for v in self.forward(self.preprocessor.states_to_uint8(states))]

    def eval_state(self, state) -> float:
        return self.batch_eval_state([state])[0]


def is_dual_spec(json_file: str) -> bool:
    """Whether a model JSON holds a dual (policy + value) net: decided by its spec key."""
    with open(json_file, "r") as f:
        return "pv_model" in json.load(f)


class CNNPolicyValue(_NetWrapper):
    """Dual-head network: one trunk, state -> (distribution over moves, expected outcome for the
    player to move).  ``eval_state`` / ``batch_eval_state`` are CNNPolicy's (the move list);
    ``batch_eval_value`` and ``batch_eval_both`` give the value head.  The model file carries the
    architecture under ``pv_model`` (the net is no Keras Sequential); weights use the layer-ordered
    HDF5 layout of the other nets."""

    _net_cls = PolicyValueNet
    _select = staticmethod(CNNPolicy._select)
    dual = True  # BatchedMCTS: one forward gives priors and values

    def __init__(self, feature_list: Sequence[str] = VALUE_FEATURES, device=None, **kwargs):
        super().__init__(feature_list, device=device, **kwargs)

    def _make_engine(self):
        kw = self._engine_kw()
        lam = getattr(self, "_score_utility", 0.0)
        if lam:  # the default engine is built exactly as before
            kw["score_utility"] = lam
        return make_policy_value_inference(self.model, self.device, **kw)

    # ---------------------------------------------------------- persistence
    def save_model(self, json_file: str, weights_file: Optional[str] = None) -> None:
        specs = {"pv_model": keras_compat.pv_spec(self.model), "feature_list": self.preprocessor.feature_list}
        if weights_file is not None:
            keras_compat.save_weights(self.model, weights_file)
            specs["weights_file"] = weights_file
        with open(json_file, "w") as f:
            json.dump(specs, f)

    @classmethod
    def _net_from_specs(cls, specs):
        if "pv_model" not in specs:
            raise ValueError("%s expects a %s spec" % (cls.__name__, cls._net_cls.__name__))
        return keras_compat.pv_from_spec(specs["pv_model"])

    # ----------------------------------------------------------- evaluation
    def forward(self, planes, legal=None):
        """(B, F, S, S) planes -> (probs (B, S*S), values (B,)) numpy; a net with the pass head gives
        (B, S*S + 1) with the pass last (the move lists of ``eval_state`` read the board part only)."""
        planes = np.asarray(planes)
        if planes.dtype != np.uint8:
            planes = planes.astype(np.uint8)
        probs, values = self.engine.evaluate(planes, legal)
        return probs.float().cpu().numpy(), values.float().cpu().numpy()

    def _check_states(self, states):
        size = states[0].size
        if any(st.size != size for st in states):
            raise ValueError("all states must have the same size")
        return size

    def batch_eval_both(self, states, moves_lists=None):
        """One forward: ([(move, prob), ...] per state as ``batch_eval_state``, [value per state])."""
        if not states:
            return [], []
        size = self._check_states(states)
        probs, values = self.forward(self.preprocessor.states_to_uint8(states))
        moves_lists = moves_lists or [st.get_legal_moves() for st in states]
        return ([self._select(probs[i], moves_lists[i], size) for i in range(len(states))],
                [float(v) for v in values])

    def batch_eval_state(self, states, moves_lists=None):
        return self.batch_eval_both(states, moves_lists)[0]

    def eval_state(self, state, moves=None):
        return self.batch_eval_state([state], [moves] if moves is not None else None)[0]

    def batch_eval_value(self, states) -> List[float]:
        if not states:
            return []
        self._check_states(states)
        return [float(v) for v in self.forward(self.preprocessor.states_to_uint8(states))[1]]

    # ------------------------------------------------------------ ownership
    @property
    def has_ownership(self) -> bool:
        return bool(getattr(self.model, "ownership", False))

    def batch_eval_ownership(self, states) -> List[np.ndarray]:
        """Per state an (S, S) float array of the ownership head, + = Black (the head's mover's-frame
        output times ``current_player``), indexed [x][y] like the board.  Runs on a second engine built
        on first use with ``ownership=True``; the search engine stays as it is."""
        if not self.has_ownership:
            raise ValueError("this net has no ownership head")
        if not states:
            return []
        size = self._check_states(states)
        if getattr(self, "_own_engine", None) is None:
            self._own_engine = make_policy_value_inference(self.model, self.device, ownership=True,
                                                           **self._engine_kw())
        eng = self._own_engine
        planes = self.preprocessor.states_to_uint8(states)
        eng.evaluate(np.asarray(planes, dtype=np.uint8))
        own = eng.ownership_view().float().cpu().numpy()
        return [own[i].reshape(size, size) * float(st.current_player) for i, st in enumerate(states)]

    def eval_ownership(self, state) -> np.ndarray:
        return self.batch_eval_ownership([state])[0]

    # ---------------------------------------------------------------- score
    @property
    def has_score(self) -> bool:
        return bool(getattr(self.model, "score_head", False))

    def set_score_utility(self, lam: float) -> None:
        """Search on the utility (v + lam * tanh(score / (2 S))) / (1 + lam) instead of the value from now on
        (see models/inference.py): the engine's value column, hence root values and the resign threshold, then
        speak of this utility.  ``lam`` = 0 restores the pure value.  ``lam`` has no tuned value.  The engine
        is rebuilt on its next use."""
        lam = float(lam)
        if lam < 0:
            raise ValueError("score_utility must be >= 0, not %r" % lam)
        if lam and not self.has_score:
            raise ValueError("score_utility needs a net with the score head (init-model pv --score-head)")
        self._score_utility = lam
        self._engine = None

    def batch_eval_score(self, states) -> List[float]:
        """Per state the score head's estimate of the final margin in points, komi included, + = Black (the
        head's mover's-frame output times ``current_player``).  Runs on a second engine built on first use
        with ``score=True``; the search engine stays as it is."""
        if not self.has_score:
            raise ValueError("this net has no score head")
        if not states:
            return []
        self._check_states(states)
        if getattr(self, "_score_engine", None) is None:
            self._score_engine = make_policy_value_inference(self.model, self.device, score=True,
                                                             **self._engine_kw())
        eng = self._score_engine
        planes = self.preprocessor.states_to_uint8(states)
        eng.evaluate(np.asarray(planes, dtype=np.uint8))
        sc = eng.score_view().float().cpu().numpy()
        return [float(sc[i]) * float(st.current_player) for i, st in enumerate(states)]

    def eval_score(self, state) -> float:
        return self.batch_eval_score([state])[0]

    def refresh(self) -> None:
        super().refresh()
        if getattr(self, "_own_engine", None) is not None:
            self._own_engine.sync_weights()
        if getattr(self, "_score_engine", None) is not None:
            self._score_engine.sync_weights()

    # ---------------------------------------------------------------- split
    def split(self):
        """(CNNPolicy, CNNValue) carrying copies of the trunk and the respective head, both on this
        net's feature list: the pair computes what the two heads compute, each on its own trunk."""
        a, fl = self.model.arch, list(self.preprocessor.feature_list)
        if getattr(self.model, "ownership", False):
            raise ValueError("split(): a net with the ownership head has no (policy, value) form: the pair "
                             "cannot carry the third head")
        if getattr(self.model, "score_head", False):
            raise ValueError("split(): a net with the score head has no (policy, value) form: the pair cannot "
                             "carry the score head")
        if self.model.trunk.residual:
            raise ValueError("split(): a residual trunk has no single-head form (the Keras Sequential of "
                             "CNNPolicy / CNNValue cannot express a skip connection)")
        kw = {k: v for k, v in a.items() if k.startswith("filter_width_")}
        pol = CNNPolicy(fl, device=self.device, board=a["board"], filters_per_layer=a["filters_per_layer"],
                        layers=a["layers"], **kw)
        val = CNNValue(fl, device=self.device, board=a["board"], filters_per_layer=a["filters_per_layer"],
                       layers=a["layers"], dense=a["dense"], **kw)
        m = self.model
        with torch.no_grad():
            for dst in (pol.model, val.model):
                for l in range(m.trunk.layers):
                    dst.trunk.weights[l].copy_(m.trunk.weights[l])
                    dst.trunk.biases[l].copy_(m.trunk.biases[l])
            pol.model.head_w.copy_(m.head_w)
            pol.model.head_b.copy_(m.head_b)
            val.model.head_w.copy_(m.vhead_w)
            val.model.head_b.copy_(m.vhead_b)
            for n in ("fc1_w", "fc1_b", "fc2_w", "fc2_b"):
                getattr(val.model, n).copy_(getattr(m, n))
        return pol, val
