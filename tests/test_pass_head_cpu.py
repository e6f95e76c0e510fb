"""The pass head of the dual net on the CPU: the fp64 reference of pass_head_refs.py against the net's torch
expression and its autograd, the parameter draws (a net without the head draws what the parent commit drew:
digests recorded from it), the spec and weight-file round trips, ``init-model pv --pass-head``, the torch
trainer on hard and one-hot targets, ``Forest.apply`` with and without ``pass_priors`` (the latter against a
replay recorded from the parent commit) and a search over a stub dual engine that wants to pass."""
import hashlib
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import head_refs as R
import pass_head_refs as PR

S, F, C0 = 5, 8, 6
NP = S * S


def _net(seed=0, live=False, he=False, **kw):
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_

    torch.manual_seed(seed)
    kw.setdefault("layers", 2)
    net = PolicyValueNet(C0, S, F, dense=16, **kw)
    if he:
        he_uniform_(net, generator=torch.Generator().manual_seed(seed + 1))
    if live:
        g = torch.Generator().manual_seed(seed + 2)
        with torch.no_grad():
            for p in net.parameters():
                p.uniform_(-0.3, 0.3, generator=g)
    return net


def _digest(net):
    h = hashlib.sha256()
    for n, p in net.named_parameters():
        h.update(n.encode())
        h.update(p.detach().numpy().tobytes())
    return h.hexdigest()[:16]


# ----------------------------------------------------------------------------- the function
def _case(with_sym, weighted):
    """A 2-layer F = 8, S = 5 net in fp64, its trunk output with a planted tie, an all-zero channel and a dead
    board, eight target rows (every kind), and the net's objective on them."""
    from alphago_amd.train.engine import apply_symmetry_dist, soft_target_loss, symmetry_tables

    B = 8
    net = _net(seed=5, live=True, pass_head=1).double()
    x = torch.rand(B, C0, S, S, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        h0 = net.trunk.forward_torch(x)
        h0[0, 3, 1, 2] = h0[0, 3, 4, 0] = h0[0, 3].max() + 0.25  # two equal maxima: pixel 7 wins over pixel 20
        h0[1, 5] = 0.0                                             # an all-zero channel: argmax 0, no gradient
        h0[2, 6, 4, 4] = h0[2, 6].max() + 0.5                      # the maximum at the last pixel
        h0[3] = 0.0                                                # a dead board
    assert bool((h0 == 0).any()) and bool((h0 > 0).any())
    tdist, sym, kind = PR.pass_targets(F, F, B, S, with_sym)
    assert sorted(kind.tolist()) == list(range(8))
    weight = torch.tensor(R.SIGNED_WEIGHTS + (0.25, 1.5))[:B].double() if weighted else None
    u = h0.clone().requires_grad_(True)  # the pre-activation: relu(u) == h0 and torch's relu'(0) is 0
    z = net.policy_logits_torch(torch.relu(u))
    rows = tdist.double()
    if sym is not None:
        rows = apply_symmetry_dist(rows, sym, symmetry_tables(S))
    per, correct, has = soft_target_loss(z, rows)
    wt = has.double() if weight is None else has.double() * weight
    gs = 1.0 / B
    ((per * wt).sum() * gs).backward()
    y = h0.permute(0, 2, 3, 1).contiguous()  # NHWC, the reference's layout
    ref = PR.pass_head_ref(y, net.head_w.detach().view(-1), net.head_b.detach(), net.pass_w.detach().view(-1),
                           float(net.pass_b.detach()), tdist, sym, weight, gs)
    return SimpleNamespace(net=net, u=u, z=z.detach(), per=per.detach(), correct=correct, has=has, ref=ref, kind=kind)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("with_sym", [False, True])
def test_torch_expression_and_autograd_are_the_reference(with_sym, weighted):
    c = _case(with_sym, weighted)
    ref, net = c.ref, c.net
    pairs = {
        "logits": (c.z, ref.logits),
        "loss": (c.per * c.has, ref.loss),
        "correct": (c.correct.double(), ref.correct),
        "dz + dpool": (c.u.grad.permute(0, 2, 3, 1), ref.dz + ref.dpool),
        "d head_w": (net.head_w.grad.view(-1), ref.dhead[:, :F].sum(0)),
        "d head_b": (net.head_b.grad.view(-1), ref.dhead[:, F].sum().view(1)),
        "d pass_w": (net.pass_w.grad.view(-1), ref.dpw[:, :2 * F].sum(0)),
        "d pass_b": (net.pass_b.grad.view(-1), ref.dpw[:, 2 * F].sum().view(1)),
    }
    for name, (got, want) in pairs.items():
        err = float((got.double() - want).abs().max())
        print("%-10s max |torch - ref| = %.3g of %.3g" % (name, err, float(want.abs().max())))
        assert err <= 1e-10, name
        assert float(want.abs().max()) > 1e-4, name  # nothing is compared at zero
    # what the reference says about the rows: only the all-zero row has no loss; a pass-only row has one
    assert torch.equal(~ref.has, c.kind == PR.ZERO)
    assert float(ref.loss[c.kind == PR.PASS_ONLY]) > 0
    assert bool((ref.dlogits[~ref.has] == 0).all()) and bool((ref.dpool[~ref.has] == 0).all())
    # the pooling's gradient: nothing where h == 0 (the all-zero channel's argmax pixel 0 included), the max part
    # on exactly the lowest-index pixel
    assert ref.argmax[0, 3] == 7 and ref.argmax[1, 5] == 0 and ref.argmax[2, 6] == NP - 1
    assert not bool(ref.dpool[1, :, :, 5].any()) and not bool(ref.dpool[3].any())
    assert 0 < float(ref.correct.sum()) < 8


def test_pass_loses_ties_and_is_always_legal():
    """z_pass equal to the top board logit: argmax stays on the board (index NP loses ties); the torch engine gives
    p_pass = 1 on a board with no legal point and exact zeros on illegal points."""
    from alphago_amd.models.inference import TorchPolicyValueInference
    from alphago_amd.models.nets import first_argmax

    z = torch.tensor([[0.5, 2.0, 2.0], [2.0, 0.5, 2.0], [0.0, 0.0, 3.0]])
    assert first_argmax(z).tolist() == [1, 0, 2]
    net = _net(seed=6, live=True, pass_head=1)
    eng = TorchPolicyValueInference(net, "cpu")
    assert eng.pass_head
    planes = (torch.rand(3, C0, S, S, generator=torch.Generator().manual_seed(2)) < 0.4).to(torch.uint8)
    legal = (torch.rand(3, NP, generator=torch.Generator().manual_seed(3)) < 0.5).to(torch.uint8)
    legal[1] = 0
    p, v = eng.evaluate(planes, legal)
    assert tuple(p.shape) == (3, NP + 1) and tuple(v.shape) == (3,)
    assert torch.allclose(p.sum(1), torch.ones(3), atol=1e-6)
    assert bool((p[:, :NP][legal == 0] == 0).all()) and float(p[1, NP]) == 1.0 and bool((p[:, NP] > 0).all())
    p0, _ = eng.evaluate(planes)
    want = torch.softmax(net.logits_value_torch(planes.float())[0], 1)
    assert torch.equal(p0, want) and tuple(want.shape) == (3, NP + 1)


# ----------------------------------------------------------------------------- parameters
# sha256[:16] over (name, bytes) of every parameter of PolicyValueNet(6, 5, 8, dense=16, **kw) after
# torch.manual_seed(11), and after he_uniform_ with generator seed 12: recorded from the parent commit
PARENT_DRAWS = {
    "plain": (dict(layers=4), "50bb87a1ceb4109c", "e6e4e106130c8921"),
    "residual": (dict(layers=5, residual=1), "d5ccfa4bf22f095a", "3e4c70fa83c1d247"),
    "ownership": (dict(layers=5, residual=1, ownership=1), "8dc43ad9c4ccc88d", "0848bf271542380d"),
    "gpool": (dict(layers=5, residual=1, gpool=1), "123abe3f814a9ff2", "07b4975083a94727"),
    "all": (dict(layers=5, residual=1, gpool=2, ownership=1), "5840e73722a1165d", "8ba5168d57eee90c"),
}


@pytest.mark.parametrize("variant", sorted(PARENT_DRAWS))
def test_draws_without_the_head_are_the_parents_and_the_head_draws_last(variant):
    from alphago_amd.models.nets import he_uniform_

    kw, d0, d1 = PARENT_DRAWS[variant]
    a = _net(seed=11, **kw)
    assert _digest(a) == d0 and "pass_head" not in a.arch and not a.pass_head
    b = _net(seed=11, pass_head=1, **kw)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    # created after every other parameter of the net itself; drawn after all of them, trunk.gpool_w included, or
    # the comparison below would see shifted draws
    assert [n for n in pb if n not in pa] == ["pass_w", "pass_b"]
    assert [n for n in pb if "." not in n] == [n for n in pa if "." not in n] + ["pass_w", "pass_b"]
    for n, p in pa.items():
        assert torch.equal(p, pb[n]), n
    assert tuple(b.pass_w.shape) == (2 * F, 1) and tuple(b.pass_b.shape) == (1,)
    bound = (6.0 / (2 * F + 1)) ** 0.5  # the Keras uniform draw of a (2F, 1) Dense kernel
    assert bool(b.pass_w.any()) and float(b.pass_w.detach().abs().max()) <= bound and float(b.pass_b.detach()) == 0.0
    he_uniform_(a, generator=torch.Generator().manual_seed(12))
    he_uniform_(b, generator=torch.Generator().manual_seed(12))
    assert _digest(a) == d1
    for n, p in a.named_parameters():
        assert torch.equal(p, dict(b.named_parameters())[n]), n
    assert not bool(b.pass_w.any()) and float(b.pass_b.detach()) == 0.0  # he_uniform_ zeroes pass_w


def test_flops_add_the_dense_layer():
    assert _net(pass_head=1).flops_per_position() - _net().flops_per_position() == 2 * 2 * F


# ----------------------------------------------------------------------------- persistence, CLI
def test_spec_round_trip_and_unchanged_spec_without_the_head():
    from alphago_amd.io import keras_compat

    net = _net(layers=5, residual=1, gpool=2, ownership=1, pass_head=1)
    spec = keras_compat.pv_spec(net)
    assert spec["pass_head"] == 1 and list(spec)[-1] == "pass_head"
    back = keras_compat.pv_from_spec(json.loads(json.dumps(spec)))
    assert back.arch == net.arch and back.pass_head
    plain = keras_compat.pv_spec(_net(layers=5, residual=1, gpool=2, ownership=1))
    assert list(plain) == ["input_dim", "board", "filters_per_layer", "layers", "dense", "residual", "ownership",
                           "gpool"]


@pytest.mark.parametrize("kw", [dict(), dict(layers=5, residual=1, gpool=1, ownership=1)])
def test_weight_file_round_trip(tmp_path, kw):
    from alphago_amd.io import keras_compat
    from alphago_amd.io.h5lite import H5File

    net = _net(seed=8, live=True, pass_head=1, **kw)
    path = str(tmp_path / "w.hdf5")
    keras_compat.save_weights(net, path)
    with H5File(path) as f:
        names = [n.decode() if isinstance(n, bytes) else str(n) for n in f.attrs["layer_names"]]
    assert names[-1] == "pass_dense_1"  # after the gpool entries
    if kw:
        assert names[-3:-1] == ["gpool_dense_1", "gpool_dense_2"]
    other = _net(seed=9, pass_head=1, **kw)
    keras_compat.load_weights(other, path)
    for (n, p), (_, q) in zip(net.named_parameters(), other.named_parameters()):
        assert torch.equal(p, q), n
    keras_compat.save_weights(_net(**kw), path)  # a net without the head writes the entries it always wrote
    with H5File(path) as f:
        assert not any(b"pass" in (n if isinstance(n, bytes) else str(n).encode()) for n in f.attrs["layer_names"])
    with pytest.raises(ValueError):
        keras_compat.load_weights(other, path)


def test_init_model_pass_head(tmp_path, capsys):
    from alphago_amd.cli import main
    from alphago_amd.models.policy import CNNPolicyValue

    js = str(tmp_path / "m.json")
    assert main(["init-model", "pv", js, "--weights", str(tmp_path / "m.hdf5"), "--board", "9", "--filters", "8",
                 "--layers", "5", "--residual", "--gpool", "2", "--ownership", "--pass-head"]) == 0
    with open(js) as f:
        arch = json.load(f)["pv_model"]
    assert arch["pass_head"] == 1 and arch["gpool"] == 2 and arch["ownership"] == 1 and arch["residual"] == 1
    m = CNNPolicyValue.load_model(js, device="cpu")
    assert m.model.pass_head and tuple(m.model.pass_w.shape) == (16, 1)
    assert main(["init-model", "pv", str(tmp_path / "p.json"), "--board", "9", "--filters", "8", "--layers", "3"]) == 0
    with open(str(tmp_path / "p.json")) as f:
        assert "pass_head" not in json.load(f)["pv_model"]
    with pytest.raises(SystemExit):
        main(["init-model", "policy", str(tmp_path / "e.json"), "--board", "9", "--filters", "8", "--layers", "3",
              "--pass-head"])
    assert "init-model pv" in capsys.readouterr().err
    # the players' move lists read the board part of the wider row
    from alphago_amd import go

    moves = m.eval_state(go.GameState(size=9))
    assert len(moves) == 81 and abs(sum(p for _, p in moves) - 1.0) < 1e-6


# ----------------------------------------------------------------------------- trainer
def _batch(B=4):
    rng = np.random.default_rng(0)
    planes = torch.from_numpy((rng.random((B, C0, S, S)) < 0.4).astype(np.uint8))
    z = torch.tensor([1.0, -1.0, 1.0, -1.0])[:B]
    return planes, z


def test_torch_trainer_hard_moves_are_their_one_hot_rows():
    from alphago_amd.train.engine import TorchPolicyValueTrainer, pass_target_rows

    planes, z = _batch()
    moves = torch.tensor([3, -1, NP - 1, 0], dtype=torch.int32)  # the second position was a pass
    rows = pass_target_rows(moves, NP)
    assert tuple(rows.shape) == (4, NP + 1) and rows[1].argmax() == NP and bool((rows.sum(1) == 1).all())
    sym = torch.tensor([0, 3, 5, 6], dtype=torch.int32)
    weight = torch.tensor([1.0, 2.0, -0.5, 1.0])
    nets = [_net(seed=10, live=True, pass_head=1, layers=3, residual=1, ownership=1) for _ in range(2)]
    own = (torch.randint(-1, 2, (4, NP), generator=torch.Generator().manual_seed(4)).to(torch.int8), torch.ones(4))
    out = []
    for net, tgt in zip(nets, (moves, rows)):
        tr = TorchPolicyValueTrainer(net, 4, lr=0.1, device="cpu")
        assert tr.fp.names[-4:] == ["ohead_w", "ohead_b", "pass_w", "pass_b"]  # after the ownership entries
        ev = tr.evaluate(planes, (tgt, z, own))
        out.append((ev, tr.step(planes, (tgt, z, own), sym, weight)))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        assert torch.equal(a, b)
    assert float(out[0][0][0]) > 0 and len(out[0][1]) == 6
    for (n, p), (_, q) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        assert torch.equal(p, q), n
    ref = _net(seed=10, live=True, pass_head=1, layers=3, residual=1, ownership=1)
    assert bool((nets[0].pass_w != ref.pass_w).all()) and float(nets[0].pass_b.detach()) != float(ref.pass_b.detach())
    # a pass row alone has a loss and a gradient now
    tr = TorchPolicyValueTrainer(ref, 4, lr=0.1, device="cpu")
    only = torch.zeros(4, NP + 1)
    only[:, NP] = 1.0
    m = tr.step(planes, (only, z, own))
    assert float(m[0]) > 0
    with pytest.raises(ValueError, match="pass last"):
        tr.step(planes, (only[:, :NP].contiguous(), z, own))
    # a net without the head keeps its flat layout and still ignores a trailing pass column
    plain = TorchPolicyValueTrainer(_net(seed=10, live=True, layers=3, residual=1), 4, lr=0.1, device="cpu")
    assert "pass_w" not in plain.fp.names and float(plain.step(planes, (only, z))[0]) == 0.0


# ----------------------------------------------------------------------------- search
def _position():
    from alphago_amd import go

    st = go.GameState(size=9)
    for mv in [(2, 2), (6, 6), (2, 6), (6, 2), (4, 4), (4, 3), (3, 3), (5, 4)]:
        st.do_move(mv)
    return st


def _forest(seed=5):
    from alphago_amd._native import engine

    f = engine().Forest(1, 5.0, 0.0, 60, 1000, 3, seed, ["board", "ones", "sensibleness"])
    f.set_root(0, _position())
    return f


# root_stats after the replay below, recorded from the parent commit: the visit counts of the 73 children and the
# Q of the visited ones (6 decimals)
PARENT_VISITS = [1, 3, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 2, 2, 0, 1, 0, 0, 0, 0, 0, 0, 1, 2, 1, 7, 0, 1, 0, 1, 1, 0, 0, 1,
                 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 1, 0, 1, 2, 3, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 2, 0, 0, 1]
PARENT_Q = [-0.750317, 0.201986, -0.890915, -0.019821, 0.20302, -0.108746, 0.182762, -0.997431, -0.308966, 0.100515,
            0.439763, 0.107621, -0.688101, -0.150467, -0.3557, -0.563992, -0.354773, -0.528055, -0.562313, -0.582569,
            -0.072562, -0.111254, 0.259475, -0.083291, -0.500428, -0.665814, -0.170318, 0.902118, -0.232907]


def test_forest_without_pass_priors_is_the_parents():
    f = _forest()
    rng = np.random.default_rng(17)
    for _ in range(12):
        L = f.gather(4)
        if L == 0:
            continue
        f.apply(rng.random((L, 81), dtype=np.float32), rng.random(L, dtype=np.float32) * 2 - 1)
    moves, visits, q = f.root_stats(0)
    assert None not in moves and list(visits) == PARENT_VISITS
    assert np.allclose([x for x, v in zip(q, visits) if v > 0], PARENT_Q, atol=2e-6, rtol=0)


def test_forest_apply_with_pass_priors():
    f = _forest()
    assert f.gather(1) == 1
    rng = np.random.default_rng(3)
    pri = rng.random((1, 81), dtype=np.float32)
    mask = f.leaf_masks()
    sens = pri[0][mask[0] != 0].astype(np.float64)
    f.apply(pri, np.zeros(1, np.float32), None, np.array([7.5], np.float32))
    g = _forest()
    g.gather(1)
    g.apply(pri, np.zeros(1, np.float32))
    moves, _, _ = f.root_stats(0)
    base, _, _ = g.root_stats(0)
    assert moves[:-1] == base and moves[-1] is None and len(sens) == len(base)  # PASS is stored last
    pf, pg = np.array(f.root_priors(0)), np.array(g.root_priors(0))
    assert abs(pf.sum() - 1.0) < 1e-5 and abs(pf[-1] - 7.5 / (sens.sum() + 7.5)) < 1e-6
    assert np.allclose(pf[:-1], pg * sens.sum() / (sens.sum() + 7.5), atol=1e-6)
    # a negative pass prior counts as 0; the child is still there
    h = _forest()
    h.gather(1)
    h.apply(pri, np.zeros(1, np.float32), None, np.array([-1.0], np.float32))
    assert h.root_stats(0)[0][-1] is None and h.root_priors(0)[-1] == 0.0
    assert np.allclose(h.root_priors(0)[:-1], pg, atol=1e-7)
    with pytest.raises(ValueError):
        k = _forest()
        k.gather(1)
        k.apply(pri, np.zeros(1, np.float32), None, np.zeros(2, np.float32))


class _StubEngine:
    """A dual engine of a net with the pass head that puts 0.99 on the pass everywhere."""

    supports_encoded = False
    needs_ladder = False
    dual = True
    pass_head = True

    def evaluate(self, planes, legal=None, slot=0):
        n, npts = planes.shape[0], planes.shape[2] * planes.shape[3]
        p = torch.full((n, npts + 1), 0.01 / npts)
        p[:, npts] = 0.99
        return p, torch.zeros(n)


def test_search_over_a_passing_engine_passes():
    from alphago_amd.search.mcts import BatchedMCTS

    policy = SimpleNamespace(dual=True, engine=_StubEngine(),
                             preprocessor=SimpleNamespace(feature_list=["board", "ones", "sensibleness"]))
    mcts = BatchedMCTS(policy, n_trees=1, threads=2, pipeline=False)
    moves = mcts.search([_position()], 64, leaves_per_tree=4)
    assert moves == [None]  # PASS
    d = mcts.visit_distribution(0, 9)
    assert d.shape == (82,) and d.argmax() == 81 and d[81] > 0.5 and abs(d.sum() - 1.0) < 1e-6
    # the same search over an engine without the column never considers the pass here
    plain = SimpleNamespace(dual=True, preprocessor=policy.preprocessor, engine=SimpleNamespace(
        supports_encoded=False, needs_ladder=False, dual=True,
        evaluate=lambda planes, legal=None, slot=0: (torch.full((planes.shape[0], 81), 1.0 / 81),
                                                     torch.zeros(planes.shape[0]))))
    m2 = BatchedMCTS(plain, n_trees=1, threads=2, pipeline=False)
    assert m2.search([_position()], 32, leaves_per_tree=4) != [None] and m2.visit_distribution(0, 9)[81] == 0
