"""The dual (policy + value) network on the CPU: the net and its files, the autograd trainer, the
search against the split pair, the player spec and the command-line tools."""
import json
import math

import numpy as np
import pytest
import torch

from alphago_amd import go


def _pv(board=9, filters=8, layers=2, seed=5, **kw):
    from alphago_amd.models.nets import he_uniform_
    from alphago_amd.models.policy import CNNPolicyValue

    torch.manual_seed(seed)
    pv = CNNPolicyValue(device="cpu", board=board, filters_per_layer=filters, layers=layers, **kw)
    he_uniform_(pv.model, generator=torch.Generator().manual_seed(seed))
    return pv


def _planes(n, board=9, seed=0):
    return np.random.default_rng(seed).integers(0, 2, (n, 49, board, board), dtype=np.uint8)


# ------------------------------------------------------------------ net, files
def test_net_shapes_and_flops():
    from alphago_amd.models.nets import PolicyNet, PolicyValueNet, ValueNet, he_uniform_

    net = PolicyValueNet()
    assert net.arch == dict(input_dim=49, board=19, filters_per_layer=192, layers=12, dense=256)
    assert tuple(net.head_w.shape) == (1, 192, 1, 1) and tuple(net.vhead_w.shape) == (1, 192, 1, 1)
    assert tuple(net.fc1_w.shape) == (361, 256) and tuple(net.fc2_w.shape) == (256, 1)
    # one trunk and both heads: the policy net's FLOPs plus the value net's head part
    pol, val = PolicyNet(49, filters_per_layer=192), ValueNet(filters_per_layer=192)
    assert net.flops_per_position() == pol.flops_per_position() + val.flops_per_position() - \
        (pol.flops_per_position() - 2.0 * 361 * 192)
    small = PolicyValueNet(49, 9, 8, 2, dense=16)
    before = small.vhead_w.detach().clone()
    he_uniform_(small, generator=torch.Generator().manual_seed(1))
    bound = math.sqrt(6.0 / 8)
    assert not torch.equal(before, small.vhead_w) and float(small.vhead_w.detach().abs().max()) <= bound
    assert float(small.vhead_w.detach().abs().max()) > 0.05  # past the Keras uniform range: the head was re-drawn
    probs, value = small(torch.from_numpy(_planes(3)))
    assert probs.shape == (3, 81) and value.shape == (3,)
    assert torch.allclose(probs.sum(1), torch.ones(3), atol=1e-5) and bool((value.abs() <= 1).all())


def test_save_load_round_trip_and_wrong_loaders(tmp_path):
    from alphago_amd.features import VALUE_FEATURES
    from alphago_amd.models.policy import CNNPolicy, CNNPolicyValue, CNNValue, is_dual_spec

    pv = _pv(dense=16)
    assert list(pv.preprocessor.feature_list) == list(VALUE_FEATURES)
    js, wf = str(tmp_path / "pv.json"), str(tmp_path / "pv.hdf5")
    pv.save_model(js, wf)
    with open(js) as f:
        spec = json.load(f)
    assert "pv_model" in spec and "keras_model" not in spec and is_dual_spec(js)
    back = CNNPolicyValue.load_model(js, device="cpu")
    x = _planes(4)
    p0, v0 = pv.forward(x)
    p1, v1 = back.forward(x)
    assert np.array_equal(p0, p1) and np.array_equal(v0, v1)
    for cls in (CNNPolicy, CNNValue):
        with pytest.raises(ValueError, match="expects a"):
            cls.load_model(js, device="cpu")
    pol, val = pv.split()
    pj = str(tmp_path / "pol.json")
    pol.save_model(pj)
    assert not is_dual_spec(pj)
    with pytest.raises(ValueError, match="expects a"):
        CNNPolicyValue.load_model(pj, device="cpu")


def test_split_pair_computes_the_two_heads():
    pv = _pv()
    pol, val = pv.split()
    assert list(pol.preprocessor.feature_list) == list(val.preprocessor.feature_list) == \
        list(pv.preprocessor.feature_list)
    x = _planes(5)
    p, v = pv.forward(x)
    assert np.array_equal(p, pol.forward(x)) and np.array_equal(v, val.forward(x))
    # copies: the pair does not follow the dual net
    with torch.no_grad():
        pv.model.head_w.add_(1.0)
    assert not np.array_equal(pv.forward(x)[0], pol.forward(x))
    st = go.GameState(9)
    moves, values = pv.batch_eval_both([st, st])
    assert len(moves) == 2 and len(values) == 2 and abs(sum(pr for _, pr in moves[0]) - 1.0) < 1e-6
    assert pv.batch_eval_value([st, st]) == values  # the same batch: the same bits
    assert [m for m, _ in pv.eval_state(st)] == [m for m, _ in moves[0]]


def test_dual_engine_refuses_symmetries():
    pv = _pv()
    pv.set_symmetries("all")
    with pytest.raises(ValueError, match="does not ensemble"):
        pv.engine


# -------------------------------------------------------------------- trainer
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("value_coef", [1.0, 0.25])
def test_torch_trainer_matches_plain_autograd(soft, value_coef):
    """TorchPolicyValueTrainer's gradients against autograd of CE(pi) + value_coef * MSE written out
    here, with a symmetry per board, a no-loss row (move -1 / all mass on the pass) and both target
    kinds."""
    import copy

    from alphago_amd.models.nets import PolicyValueNet, he_uniform_
    from alphago_amd.train.engine import TorchPolicyValueTrainer, apply_symmetry, symmetry_tables

    B, S = 5, 9
    net = he_uniform_(PolicyValueNet(49, S, 8, 2, dense=16), generator=torch.Generator().manual_seed(2))
    ref = copy.deepcopy(net)
    g = torch.Generator().manual_seed(9)
    x = torch.from_numpy(_planes(B))
    z = torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0])
    sym = torch.tensor([0, 3, 5, 7, 2], dtype=torch.int32)
    table = symmetry_tables(S)
    if soft:
        pi = torch.rand(B, S * S + 1, generator=g)
        pi = pi / pi.sum(1, keepdim=True)
        pi[1] = 0
        pi[1, S * S] = 1.0
    else:
        pi = torch.randint(0, S * S, (B,), generator=g, dtype=torch.int32)
        pi[1] = -1
    tr = TorchPolicyValueTrainer(net, B, lr=0.01, device="cpu", value_coef=value_coef)
    tr.compute_grads(x, (pi, z), sym=sym)

    xt, tt = apply_symmetry(x, None if soft else pi, sym, table)
    logits, v = ref.logits_value_torch(xt.float())
    logp = torch.log_softmax(logits, 1)
    if soft:
        fwd = table[sym.long()]
        q = torch.zeros(B, S * S)
        q.scatter_(1, fwd, pi[:, :S * S])  # the mass of point p goes to fwd[p]
        m = q.sum(1, keepdim=True)
        has = (m > 0).squeeze(1)
        q = torch.where(m > 0, q / m.clamp_min(1e-30), torch.zeros_like(q))
        ce = -(q * logp).sum(1) * has
    else:
        valid = tt >= 0
        ce = -logp.gather(1, tt.clamp_min(0).unsqueeze(1)).squeeze(1) * valid
    obj = ce.sum() / B + value_coef * ((v - z) ** 2).sum() / B
    obj.backward()
    named = dict(ref.named_parameters())
    want = {"head_w": named["head_w"], "head_b": named["head_b"], "vhead_w": named["vhead_w"],
            "vhead_b": named["vhead_b"], "fc1_w": named["fc1_w"], "fc1_b": named["fc1_b"],
            "fc2_w": named["fc2_w"], "fc2_b": named["fc2_b"]}
    for l in range(2):
        want["w%d" % l] = ref.trunk.weights[l]
        want["b%d" % l] = ref.trunk.biases[l]
    assert set(tr.fp.names) == set(want)
    for name, p in want.items():
        got = tr.fp.grad_views[name]
        assert torch.allclose(got, p.grad, rtol=1e-4, atol=1e-6), name
    per, _ = tr._last
    assert float(per[1]) == 0.0  # the no-loss row
    out = tr.step(x, (pi, z), sym=sym)
    assert len(out) == 4 and all(torch.isfinite(o) for o in out)


def test_trainer_refuses_regularisers():
    from alphago_amd.models.nets import PolicyValueNet
    from alphago_amd.train.engine import make_policy_value_trainer

    tr = make_policy_value_trainer(PolicyValueNet(49, 9, 8, 2, dense=16), 2, 0.01, backend="torch", device="cpu")
    tr.ent_coef = 0.1
    with pytest.raises(ValueError, match="dual"):
        tr.step(torch.from_numpy(_planes(2)), (torch.tensor([1, 2], dtype=torch.int32), torch.tensor([1.0, -1.0])))


# --------------------------------------------------------------------- search
def _search(nets, n_playout=64):
    from alphago_amd.search.mcts import BatchedMCTS

    s = BatchedMCTS(*nets, n_trees=2, seed=11, threads=1, pipeline=False)
    states = [go.GameState(9), go.GameState(9)]
    states[1].do_move((2, 3))
    moves = s.search(states, n_playout, leaves_per_tree=4)
    return moves, [s.visit_distribution(i, 9) for i in range(2)], [s.root_value(i) for i in range(2)]


def test_search_with_dual_net_equals_search_with_the_split_pair():
    """One forward of the dual net per leaf batch gives the priors and values the pair gives: the
    visit distributions, root values and moves are exactly the pair search's (which is
    bit-reproducible run to run at this size)."""
    pv = _pv()
    a = _search((pv,))
    b = _search(pv.split())
    c = _search(pv.split())
    assert b[0] == c[0] and b[2] == c[2] and all(np.array_equal(x, y) for x, y in zip(b[1], c[1]))
    assert a[0] == b[0]
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    assert a[2] == b[2]
    assert any(v != 0.0 for v in a[2])  # the value head reached the tree


# ---------------------------------------------------------------------- tools
def test_make_player_loads_a_dual_spec(tmp_path):
    from alphago_amd.cli import make_player
    from alphago_amd.models.policy import CNNPolicyValue

    pv = _pv()
    js = str(tmp_path / "pv.json")
    pv.save_model(js, str(tmp_path / "pv.hdf5"))
    player = make_player("mcts:%s:32" % js, device="cpu")
    assert isinstance(player.search.policy, CNNPolicyValue) and player.search.value is None
    st = go.GameState(9)
    mv = player.get_move(st)
    assert mv is go.PASS_MOVE or st.is_legal(mv)
    with pytest.raises(ValueError, match="dual"):
        make_player("mcts:%s,%s:32" % (js, js), device="cpu")


def test_init_model_pv_writes_a_loadable_spec(tmp_path):
    from alphago_amd.cli import main
    from alphago_amd.models.policy import CNNPolicyValue

    js, wf = str(tmp_path / "m.json"), str(tmp_path / "m.hdf5")
    assert main(["init-model", "pv", js, "--weights", wf, "--board", "9", "--layers", "2"]) == 0
    m = CNNPolicyValue.load_model(js, device="cpu")
    assert m.model.arch["filters_per_layer"] == 192 and m.model.arch["board"] == 9
    assert m.preprocessor.output_dim == 49


def test_serve_refuses_a_dual_spec(tmp_path):
    from alphago_amd.serve.server import serve_cli

    js = str(tmp_path / "pv.json")
    _pv().save_model(js)
    with pytest.raises(SystemExit, match="dual"):
        serve_cli([js, "--device", "cpu"])


def _selfplay_file(path, pv, n_games=3, n_moves=4):
    """A tiny selfplay.h5 through SelfPlayWriter: a dozen positions, one with all its mass on the pass."""
    from alphago_amd.search.selfplay_mcts import GameRecord, SelfPlayWriter

    rng = np.random.default_rng(4)
    w = SelfPlayWriter(path, None, features=list(pv.preprocessor.feature_list), size=9)
    for gid in range(n_games):
        r = GameRecord(size=9, komi=7.5, game_id=gid, winner=1 if gid % 2 == 0 else -1)
        st = go.GameState(9, 7.5)
        for k in range(n_moves):
            d = np.zeros(82, np.float32)
            if gid == 0 and k == n_moves - 1:
                d[81] = 1.0  # all visits on the pass
                mv = -1
            else:
                legal = [m for m in st.get_legal_moves()]
                pick = [legal[i] for i in rng.choice(len(legal), 3, replace=False)]
                for m in pick:
                    d[m[0] * 9 + m[1]] = 1.0 / 3
                mv = pick[0][0] * 9 + pick[0][1]
            r.moves.append(mv)
            r.pi.append(d)
            r.players.append(st.current_player)
            r.root_values.append(0.0)
            st.do_move(None if mv < 0 else divmod(mv, 9))
        r.final_state = st
        w.add(r)
    return w.close()


@pytest.mark.parametrize("targets", ["pi", "played"])
def test_train_pv_runs_an_epoch_and_writes_loadable_weights(tmp_path, targets):
    from alphago_amd.cli import main
    from alphago_amd.models.policy import CNNPolicyValue

    pv = _pv()
    js = str(tmp_path / "pv.json")
    pv.save_model(js, str(tmp_path / "pv0.hdf5"))
    h5 = str(tmp_path / "selfplay.h5")
    assert _selfplay_file(h5, pv) == 12
    out = tmp_path / "out"
    metrics = str(tmp_path / "m.jsonl")
    assert main(["train-pv", js, h5, str(out), "--minibatch", "4", "--epochs", "1", "--backend", "torch",
                 "--targets", targets, "--train-val-test", "0.7", "0.3", "0", "--learning-rate", "0.01",
                 "--value-coef", "0.5", "--metrics", metrics]) == 0
    with open(out / "metadata.json") as f:
        meta = json.load(f)
    ep = meta["epochs"][0]
    for k in ("loss", "acc", "value_loss", "value_acc", "val_loss", "val_value_loss"):
        assert k in ep and math.isfinite(ep[k]), k
    assert meta["targets"] == targets and meta["value_coef"] == 0.5
    trained = CNNPolicyValue.load_model(js, device="cpu", weights_file=str(out / "weights.00000.hdf5"))
    x = _planes(2)
    assert not np.array_equal(trained.forward(x)[0], CNNPolicyValue.load_model(js, device="cpu").forward(x)[0])
