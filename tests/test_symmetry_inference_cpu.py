"""Symmetry ensembling (symmetries="random" / "all") of the torch engines, the model wrappers and the
command line, against a float64 oracle written from the definition (models/inference.py):

  policy = 1/G sum_g P_s[fwd_s(p)],  value = 1/G sum_g V(board under s),

with P_s / V the plain ("none") engine on the board transformed by symmetry s (legal mask alike) and
fwd_s the point map of ``train/engine.symmetry_tables`` (``pack_input``'s convention).  Bound 1e-6:
engine and oracle average the same fp32 outputs, the engine in fp32 (at most 8 * 2^-24 away).
"""
import numpy as np
import pytest
import torch

from alphago_amd.models.inference import (TorchPolicyInference, TorchValueInference, make_policy_inference,
                                          make_value_inference)
from alphago_amd.models.nets import PolicyNet, ValueNet
from alphago_amd.train.engine import symmetry_tables

S, C, N = 9, 6, 5
BOUND = 1e-6
TABLE = symmetry_tables(S).numpy()  # fwd[s][p]


def transform(a, s):
    """(..., S*S) array in the original frame -> the frame of symmetry s: out[fwd[p]] = a[p]."""
    out = np.empty_like(a)
    out[..., TABLE[s]] = a
    return out


def back(a, s):
    """Transformed frame -> original frame: out[p] = a[fwd[p]]."""
    return a[..., TABLE[s]]


def t_planes(planes, s):
    n, c = planes.shape[:2]
    return transform(planes.reshape(n, c, S * S), s).reshape(planes.shape)


def roughen(net, std=0.2):
    """Weights large enough for the outputs to depend visibly on the orientation (the default
    initialisation gives a nearly uniform policy)."""
    with torch.no_grad():
        for p in net.parameters():
            p.normal_(0.0, std)
    return net


@pytest.fixture(scope="module")
def case():
    torch.manual_seed(3)
    pnet = roughen(PolicyNet(C, board=S, filters_per_layer=12, layers=3))
    vnet = roughen(ValueNet(C, board=S, filters_per_layer=12, layers=2, dense=16), 0.1)
    rng = np.random.default_rng(5)
    planes = (rng.random((N, C, S, S)) < 0.4).astype(np.uint8)
    legal = (rng.random((N, S * S)) < 0.6).astype(np.uint8)
    return pnet, vnet, planes, legal


def oracle_policy(pnet, planes, legal, syms):
    """float64 mean over the rows of ``syms`` (G, n) of the plain engine's outputs mapped back."""
    plain = TorchPolicyInference(pnet)
    acc = np.zeros((planes.shape[0], S * S))
    for row in syms:
        for b, s in enumerate(row):
            p = plain.evaluate(t_planes(planes[b:b + 1], s), transform(legal[b:b + 1], s)).numpy().astype(np.float64)
            acc[b] += back(p[0], s)
    return acc / len(syms)


def oracle_value(vnet, planes, syms):
    plain = TorchValueInference(vnet)
    acc = np.zeros(planes.shape[0])
    for row in syms:
        for b, s in enumerate(row):
            acc[b] += float(plain.evaluate(t_planes(planes[b:b + 1], s)).reshape(-1)[0])
    return acc / len(syms)


ALL = np.repeat(np.arange(8)[:, None], N, 1)


def test_all_matches_oracle(case):
    pnet, vnet, planes, legal = case
    out = TorchPolicyInference(pnet, symmetries="all").evaluate(planes, legal).numpy()
    ref = oracle_policy(pnet, planes, legal, ALL)
    assert np.abs(out - ref).max() <= BOUND
    assert np.all(out[legal == 0] == 0)
    np.testing.assert_allclose(out.sum(1), 1.0, atol=1e-5)
    v = TorchValueInference(vnet, symmetries="all").evaluate(planes).numpy().reshape(-1)
    assert np.abs(v - oracle_value(vnet, planes, ALL)).max() <= BOUND
    # the plain engine is not symmetric: the option changes something
    plain = TorchPolicyInference(pnet).evaluate(planes, legal).numpy()
    assert np.abs(plain - ref).max() > 1e-3


def test_all_without_mask_and_edge_rows(case):
    pnet, _, planes, _ = case
    eng = TorchPolicyInference(pnet, symmetries="all")
    out = eng.evaluate(planes).numpy()
    ones = np.ones((N, S * S), np.uint8)
    assert np.abs(out - oracle_policy(pnet, planes, ones, ALL)).max() <= BOUND
    legal = ones.copy()
    legal[1] = 0  # no legal point: all-zero row
    legal[0] = 0
    legal[0, 7] = 1  # one legal point: exactly 1
    out = eng.evaluate(planes, legal).numpy()
    assert np.all(out[1] == 0)
    assert out[0, 7] == 1.0 and out[0].sum() == 1.0


@pytest.mark.parametrize("t", range(8))
def test_all_is_equivariant(case, t):
    pnet, vnet, planes, legal = case
    eng = TorchPolicyInference(pnet, symmetries="all")
    base = eng.evaluate(planes, legal).numpy()
    moved = eng.evaluate(t_planes(planes, t), transform(legal, t)).numpy()
    assert np.abs(moved - transform(base, t)).max() <= BOUND
    val = TorchValueInference(vnet, symmetries="all")
    v0 = val.evaluate(planes).numpy().reshape(-1)
    v1 = val.evaluate(t_planes(planes, t)).numpy().reshape(-1)
    assert np.abs(v0 - v1).max() <= BOUND


def test_random_mode(case):
    pnet, vnet, _, _ = case
    rng = np.random.default_rng(11)
    planes = (rng.random((64, C, S, S)) < 0.4).astype(np.uint8)
    legal = (rng.random((64, S * S)) < 0.6).astype(np.uint8)
    e1 = TorchPolicyInference(pnet, symmetries="random", symmetry_seed=7)
    e2 = TorchPolicyInference(pnet, symmetries="random", symmetry_seed=7)
    o1, o2 = e1.evaluate(planes, legal).numpy(), e2.evaluate(planes, legal).numpy()
    s1 = e1.last_symmetries()
    assert s1.shape == (64,) and np.array_equal(s1, e2.last_symmetries())
    assert np.array_equal(o1, o2)
    assert len(set(s1.tolist())) > 1 and s1.min() >= 0 and s1.max() <= 7
    assert np.abs(o1 - oracle_policy(pnet, planes, legal, s1[None])).max() <= BOUND
    # a second submission draws again, and another seed draws differently
    e1.evaluate(planes, legal)
    assert not np.array_equal(e1.last_symmetries(), s1)
    e3 = TorchPolicyInference(pnet, symmetries="random", symmetry_seed=8)
    e3.evaluate(planes, legal)
    assert not np.array_equal(e3.last_symmetries(), s1)
    v = TorchValueInference(vnet, symmetries="random", symmetry_seed=7)
    out = v.evaluate(planes).numpy().reshape(-1)
    assert np.abs(out - oracle_value(vnet, planes, v.last_symmetries()[None])).max() <= BOUND


def test_bad_mode_raises(case):
    pnet, vnet, _, _ = case
    for bad in ("ALL", "8", "", None):
        with pytest.raises(ValueError):
            TorchPolicyInference(pnet, symmetries=bad)
        with pytest.raises(ValueError):
            TorchValueInference(vnet, symmetries=bad)
        with pytest.raises(ValueError):
            make_policy_inference(pnet, "cpu", symmetries=bad)
        with pytest.raises(ValueError):
            make_value_inference(vnet, "cpu", symmetries=bad)
    assert make_policy_inference(pnet, "cpu", symmetries="all", feature_list=["board"]).symmetries == "all"
    assert make_value_inference(vnet, "cpu").symmetries == "none"


FEATURES = ["board", "ones", "turns_since"]


def _wrapper_oracle(pol, planes, legal):
    acc = np.zeros((planes.shape[0], S * S))
    pol.set_symmetries("none")
    for s in range(8):
        acc += back(pol.forward(t_planes(planes, s), transform(legal, s)).astype(np.float64), s)
    return acc / 8


def test_wrapper_set_symmetries():
    from alphago_amd.models.policy import CNNPolicy

    torch.manual_seed(4)
    pol = CNNPolicy(FEATURES, device="cpu", board=S, filters_per_layer=8, layers=2)
    roughen(pol.model)
    c = pol.preprocessor.output_dim
    rng = np.random.default_rng(2)
    planes = (rng.random((3, c, S, S)) < 0.4).astype(np.uint8)
    legal = (rng.random((3, S * S)) < 0.7).astype(np.uint8)
    plain = pol.forward(planes, legal)
    ref = _wrapper_oracle(pol, planes, legal)
    assert np.abs(plain - ref).max() > 1e-3
    pol.set_symmetries("all")
    assert pol.engine.symmetries == "all"
    assert np.abs(pol.forward(planes, legal) - ref).max() <= BOUND
    pol.set_symmetries("none")
    assert np.array_equal(pol.forward(planes, legal), plain)
    with pytest.raises(ValueError):
        pol.set_symmetries("both")


def test_make_player_and_load_model(tmp_path):
    from alphago_amd.cli import make_player
    from alphago_amd.models.policy import CNNPolicy, CNNValue

    torch.manual_seed(1)
    pj, vj = str(tmp_path / "p.json"), str(tmp_path / "v.json")
    CNNPolicy(FEATURES, device="cpu", board=S, filters_per_layer=8, layers=2).save_model(pj, str(tmp_path / "p.h5"))
    CNNValue(FEATURES, device="cpu", board=S, filters_per_layer=8, layers=2).save_model(vj, str(tmp_path / "v.h5"))
    pl = make_player("policy:%s:greedy" % pj, device="cpu", symmetries="all")
    assert pl.policy.engine.symmetries == "all"
    assert make_player("policy:%s:greedy" % pj, device="cpu").policy.engine.symmetries == "none"
    m = make_player("mcts:%s,%s:8" % (pj, vj), device="cpu", symmetries="random")
    assert m.search.policy.engine.symmetries == "random" and m.search.value.engine.symmetries == "random"
    assert CNNValue.load_model(vj, device="cpu", symmetries="all").engine.G == 8
    with pytest.raises(ValueError):
        CNNPolicy.load_model(pj, device="cpu", symmetries="some")
    # the greedy player moves on a real position with the ensembled engine
    from alphago_amd import go

    assert pl.get_move(go.GameState(size=S)) is not None


def test_parsers_accept_symmetries(monkeypatch):
    from alphago_amd import cli
    from alphago_amd.serve.server import serve_parser

    assert cli.gtp_parser().parse_args(["--symmetries", "all"]).symmetries == "all"
    assert cli.match_parser().parse_args(["random", "random", "--symmetries", "random"]).symmetries == "random"
    assert serve_parser().parse_args(["p.json", "--symmetries", "all"]).symmetries == "all"
    assert cli.gtp_parser().parse_args([]).symmetries == "none"
    with pytest.raises(SystemExit):
        cli.gtp_parser().parse_args(["--symmetries", "four"])
    monkeypatch.setenv("ALPHAGO_AMD_SYMMETRIES", "random")
    assert cli.gtp_parser().parse_args([]).symmetries == "random"
    assert cli.match_parser().parse_args(["random", "random"]).symmetries == "random"
    assert serve_parser().parse_args(["p.json"]).symmetries == "random"
    assert serve_parser().parse_args(["p.json", "--symmetries", "none"]).symmetries == "none"
