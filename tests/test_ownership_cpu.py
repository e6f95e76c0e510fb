"""The ownership head on the CPU: the engine's map, the self-play records, the model files, the torch
trainer, ``train-pv`` end to end and the GTP command."""
import json
import math

import numpy as np
import pytest
import torch

from alphago_amd import go
from alphago_amd.features import VALUE_FEATURES
from alphago_amd.io.h5lite import H5File

B_, W_ = go.BLACK, go.WHITE


# ------------------------------------------------------------------------------ engine
def test_ownership_map_of_a_hand_made_position():
    """9x9: a Black eye at (0, 0), a White eye at (8, 8), an empty point (4, 4) next to both colours,
    an empty region far from any stone, stones of both colours."""
    st = go.GameState(9, 7.5)
    black = [(0, 1), (1, 0), (1, 1), (4, 3), (3, 4)]
    white = [(8, 7), (7, 8), (7, 7), (4, 5), (5, 4)]
    for b, w in zip(black, white):
        st.do_move(b, B_)
        st.do_move(w, W_)
    own = st.get_ownership()
    assert own.dtype == np.int8 and own.shape == (9, 9)
    want = np.zeros((9, 9), np.int8)
    for x, y in black:
        want[x, y] = 1
    for x, y in white:
        want[x, y] = -1
    want[0, 0] = 1    # Black eye
    want[8, 8] = -1   # White eye
    assert st.is_eyeish((0, 0), B_) and st.is_eyeish((8, 8), W_)
    assert not st.is_eyeish((4, 4), B_) and not st.is_eyeish((4, 4), W_)
    assert np.array_equal(own, want)
    assert own[4, 4] == 0 and own[0, 8] == 0


def _random_game(S, seed):
    """A seeded random game that avoids filling its own eyes, to the end."""
    rng = np.random.default_rng(seed)
    st = go.GameState(S, 7.5)
    n = 0
    while not st.is_end_of_game and n < 2 * S * S:
        mv = st.get_legal_moves(include_eyes=False)
        st.do_move(mv[rng.integers(len(mv))] if mv else None)
        n += 1
    return st


@pytest.mark.parametrize("S", [9, 13, 19])
def test_ownership_reproduces_get_winner(S):
    for seed in range(20):
        st = _random_game(S, 100 * S + seed)
        assert st.is_end_of_game and len(st.history) <= 2 * S * S, seed
        own = st.get_ownership()
        sb = int((own == 1).sum()) - st.passes_black
        sw = int((own == -1).sum()) + st.komi - st.passes_white
        assert st.get_winner() == (B_ if sb > sw else (W_ if sw > sb else 0))
        board = st.board
        for x in range(S):
            for y in range(S):
                if board[x, y] != 0:
                    assert own[x, y] == board[x, y]
                else:
                    e = 1 if st.is_eyeish((x, y), B_) else (-1 if st.is_eyeish((x, y), W_) else 0)
                    assert own[x, y] == e


# ------------------------------------------------------------------------------ writer
def _record(st, gid, n_keep=None, resigned=0, seed=0):
    """A GameRecord of the first ``n_keep`` moves of a finished game (all of them by default)."""
    from alphago_amd.search.selfplay_mcts import GameRecord

    S = st.size
    rng = np.random.default_rng(seed)
    hist = st.history_indices()
    moves = [int(m) if m >= 0 else -1 for m in hist][:n_keep]
    replay = go.GameState(S, st.komi)
    r = GameRecord(size=S, komi=st.komi, game_id=gid)
    for mv in moves:
        d = rng.random(S * S + 1).astype(np.float32)
        r.pi.append(d / d.sum())
        r.players.append(replay.current_player)
        r.root_values.append(0.0)
        r.moves.append(mv)
        replay.do_move(None if mv < 0 else divmod(mv, S))
    if resigned:
        r.moves[-1] = -1  # the record's last row: the position at which the player resigned
        r.resigned = r.players[-1]
        r.winner = -r.resigned
    else:
        r.winner = replay.get_winner()
    r.final_state = replay
    return r


def _three_games():
    full = _random_game(9, 7)
    assert full.history_indices()[-1] < 0 and full.history_indices()[-2] < 0
    other = _random_game(9, 8)
    return full, [_record(full, 0), _record(other, 1, n_keep=11, resigned=1), _record(other, 2, n_keep=12)]


def _write(path, recs, **kw):
    from alphago_amd.search.selfplay_mcts import SelfPlayWriter

    w = SelfPlayWriter(str(path), None, features=list(VALUE_FEATURES), size=9, **kw)
    for r in recs:
        w.add(r)
    n = w.close()
    return w, n


def _read(path):
    with H5File(str(path)) as f:
        return {k: np.asarray(f[k].read()) for k in f.keys()}


@pytest.mark.parametrize("ppg", [0, 4])
def test_writer_ownership_columns(tmp_path, ppg):
    full, recs = _three_games()
    assert recs[2].moves[-1] >= 0  # the capped game does not end in passes
    w, n = _write(tmp_path / "a.h5", recs, ownership=True, positions_per_game=ppg, seed=3)
    d = _read(tmp_path / "a.h5")
    assert set(d) == {"states", "pi", "outcomes", "moves", "game", "ownership", "ownership_valid"}
    assert d["ownership"].shape == (n, 81) and d["ownership"].dtype == np.int8
    assert d["ownership_valid"].shape == (n,) and d["ownership_valid"].dtype == np.uint8
    assert w.endings == {"two_passes": 1, "resignation": 1, "move_cap": 1}
    final = np.asarray(full.get_ownership(), np.int8).reshape(-1)
    g0 = d["game"] == 0
    n0 = int(g0.sum())
    assert n0 == (4 if ppg else len(recs[0].moves)) and w.own_positions == n0
    assert np.array_equal(d["ownership_valid"], g0.astype(np.uint8))
    assert not d["ownership"][~g0].any()
    # the mover's frame: the outcome column is winner * player, so player = outcome * winner
    players = d["outcomes"][g0].astype(np.int8) * np.int8(recs[0].winner)
    assert recs[0].winner != 0 and set(players.tolist()) == {1, -1}
    assert np.array_equal(d["ownership"][g0], final[None, :] * players[:, None])
    if not ppg:
        assert np.array_equal(players, np.array(recs[0].players, np.int8))


def test_writer_without_the_flag_writes_todays_datasets(tmp_path):
    _, recs = _three_games()
    _write(tmp_path / "a.h5", recs)
    assert set(_read(tmp_path / "a.h5")) == {"states", "pi", "outcomes", "moves", "game"}


def test_merge_carries_or_refuses(tmp_path):
    from alphago_amd.search.selfplay_mcts import merge_selfplay_files

    _, recs = _three_games()
    _write(tmp_path / "a.h5", recs[:2], ownership=True)
    _write(tmp_path / "b.h5", recs[2:], ownership=True)
    _write(tmp_path / "c.h5", recs[2:])
    n = merge_selfplay_files([str(tmp_path / "a.h5"), str(tmp_path / "b.h5")], str(tmp_path / "m.h5"))
    a, b, m = _read(tmp_path / "a.h5"), _read(tmp_path / "b.h5"), _read(tmp_path / "m.h5")
    assert n == len(m["ownership"]) == len(a["ownership"]) + len(b["ownership"])
    assert np.array_equal(m["ownership"], np.concatenate([a["ownership"], b["ownership"]]))
    assert np.array_equal(m["ownership_valid"], np.concatenate([a["ownership_valid"], b["ownership_valid"]]))
    with pytest.raises(ValueError, match="only some"):
        merge_selfplay_files([str(tmp_path / "a.h5"), str(tmp_path / "c.h5")], str(tmp_path / "x.h5"))
    merge_selfplay_files([str(tmp_path / "c.h5"), str(tmp_path / "c.h5")], str(tmp_path / "p.h5"))
    assert set(_read(tmp_path / "p.h5")) == {"states", "pi", "outcomes", "moves", "game"}


# ------------------------------------------------------------------------------- model
def _pv(ownership=1, **kw):
    from alphago_amd.models.policy import CNNPolicyValue

    torch.manual_seed(5)
    a = dict(board=9, filters_per_layer=8, layers=2, dense=16)
    a.update(kw)
    if ownership:
        a["ownership"] = 1
    return CNNPolicyValue(list(VALUE_FEATURES), device="cpu", **a)


def test_spec_and_weights_round_trip(tmp_path):
    from alphago_amd.models.nets import he_uniform_
    from alphago_amd.models.policy import CNNPolicyValue

    pv = _pv()
    he_uniform_(pv.model, torch.Generator().manual_seed(1))
    assert pv.model.ohead_w.shape == (1, 8, 1, 1) and pv.model.ohead_b.shape == (1,)
    assert 0 < float(pv.model.ohead_w.detach().abs().max()) <= (6.0 / 8) ** 0.5
    with torch.no_grad():
        pv.model.ohead_b.fill_(0.25)
    js, wf = str(tmp_path / "pv.json"), str(tmp_path / "pv.hdf5")
    pv.save_model(js, wf)
    with open(js) as f:
        assert json.load(f)["pv_model"]["ownership"] == 1
    with H5File(wf) as f:
        names = [n.decode() for n in f.attrs["layer_names"]]
    assert names[-4:] == ["value_convolution2d_1", "value_dense_1", "value_dense_2", "ownership_convolution2d_1"]
    back = CNNPolicyValue.load_model(js, device="cpu")
    assert back.has_ownership
    for (n, p), (_, q) in zip(pv.model.named_parameters(), back.model.named_parameters()):
        assert torch.equal(p, q), n
    with pytest.raises(ValueError, match="ownership head"):
        pv.split()
    with pytest.raises(ValueError):  # a plain net cannot read the longer file
        from alphago_amd.io import keras_compat
        keras_compat.load_weights(_pv(0).model, wf)


def test_plain_net_files_are_unchanged(tmp_path):
    from alphago_amd.io import keras_compat

    pv = _pv(0)
    assert keras_compat.pv_spec(pv.model) == dict(input_dim=49, board=9, filters_per_layer=8, layers=2, dense=16)
    wf = str(tmp_path / "pv.hdf5")
    pv.save_weights(wf)
    with H5File(wf) as f:
        names = [n.decode() for n in f.attrs["layer_names"]]
    assert names == ["convolution2d_1", "convolution2d_2", "convolution2d_3", "value_convolution2d_1",
                     "value_dense_1", "value_dense_2"]
    assert not pv.has_ownership and not hasattr(pv.model, "ohead_w")
    pol, val = pv.split()  # still splits
    # the same seed draws the same weights with and without the head
    with_head = dict(_pv(1).model.named_parameters())
    for n, p in pv.model.named_parameters():
        assert torch.equal(p, with_head[n]), n


def test_init_model_cli_flag(tmp_path):
    from alphago_amd.cli import main
    from alphago_amd.models.policy import CNNPolicyValue

    js = str(tmp_path / "pv.json")
    assert main(["init-model", "pv", js, "--weights", str(tmp_path / "w.hdf5"), "--board", "9", "--layers", "2",
                 "--filters", "8", "--ownership"]) == 0
    assert CNNPolicyValue.load_model(js, device="cpu").has_ownership
    with pytest.raises(SystemExit):
        main(["init-model", "policy", str(tmp_path / "p.json"), "--ownership"])


# ----------------------------------------------------------------------- torch trainer
def _batch(B=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    planes = torch.randint(0, 2, (B, 49, 9, 9), generator=g, dtype=torch.uint8)
    pi = torch.rand(B, 82, generator=g)
    z = torch.randint(0, 2, (B,), generator=g).float() * 2 - 1
    own_t = torch.randint(-1, 2, (B, 81), generator=g).to(torch.int8)
    valid = torch.ones(B)
    valid[1] = 0
    valid[4] = 0
    weight = torch.rand(B, generator=g) + 0.5
    return planes, pi, z, own_t, valid, weight


def _trainer(net, B=6, **kw):
    from alphago_amd.train.engine import TorchPolicyValueTrainer

    return TorchPolicyValueTrainer(net, B, lr=0.01, device="cpu", dtype=torch.float64, **kw)


def _grads(tr):
    return {n: tr.fp.grad_views[n].clone() for n in tr.fp.names}


def test_torch_loss_is_the_written_formula():
    net = _pv().model.double()
    planes, pi, z, own_t, valid, weight = _batch()
    tr = _trainer(net, own_coef=0.7)
    assert tr.fp.names[-2:] == ["ohead_w", "ohead_b"] and tr.fp.names[-3] == "fc2_b"
    with torch.no_grad():
        full = tr._loss(planes, (pi, z, (own_t, valid)), None, weight)[0]
        pair = tr._loss(planes, (pi, z), None, weight)[0]
        own = net.ownership_torch(net.trunk.forward_torch(planes.double()))
    assert own.shape == (6, 81) and bool((own.abs() <= 1).all())
    term = 0.7 * (valid.double() * weight.double() * ((own - own_t.double()) ** 2).sum(1) / 81).sum() / 6
    assert float(term) > 0
    assert math.isclose(float(full - pair), float(term), rel_tol=1e-10)
    m = tr.evaluate(planes, (pi, z, (own_t, valid)))
    assert len(m) == 6
    assert math.isclose(float(m[4]), float((valid.double() * ((own - own_t.double()) ** 2).mean(1)).sum()), rel_tol=1e-10)
    t = own_t.double()
    share = ((torch.sign(own) == t) & (t != 0)).double().sum(1) / (t != 0).sum(1)
    assert math.isclose(float(m[5]), float((share * valid.double()).sum()), rel_tol=1e-10)
    assert len(_trainer(_pv(0).model.double()).evaluate(planes, (pi, z))) == 4
    with pytest.raises(ValueError, match="ownership head"):
        _trainer(_pv(0).model.double()).evaluate(planes, (pi, z, (own_t, valid)))


def test_torch_zero_coefficient_and_invalid_boards():
    net = _pv().model.double()
    planes, pi, z, own_t, valid, weight = _batch()
    sym = torch.arange(6, dtype=torch.int32) % 8
    tr0 = _trainer(net, own_coef=0.0)
    tr0.compute_grads(planes, (pi, z, (own_t, valid)), sym, weight)
    g0 = _grads(tr0)
    tr0.compute_grads(planes, (pi, z), sym, weight)
    gp = _grads(tr0)
    for n in g0:
        assert torch.equal(g0[n], gp[n]), n
    assert not g0["ohead_w"].any()
    tr = _trainer(net, own_coef=1.0)
    tr.compute_grads(planes, (pi, z, (own_t, valid)), sym, weight)
    g1 = _grads(tr)
    assert g1["ohead_w"].abs().max() > 0 and not torch.equal(g1["w0"], gp["w0"])
    other = own_t.clone()
    other[1] = -other[1]
    other[4] = 1
    tr.compute_grads(planes, (pi, z, (other, valid)), sym, weight)
    for n, g in _grads(tr).items():
        assert torch.equal(g, g1[n]), n  # invalid boards add nothing
    tr.compute_grads(planes, (pi, z, (own_t, torch.zeros(6))), sym, weight)
    for n, g in _grads(tr).items():
        assert torch.allclose(g, gp[n], rtol=0, atol=0), n


@pytest.mark.parametrize("s", range(8))
def test_torch_symmetry_moves_the_target(s):
    from alphago_amd.train.engine import apply_symmetry, apply_symmetry_dist, symmetry_tables

    net = _pv().model.double()
    planes, pi, z, own_t, valid, weight = _batch()
    sym = torch.full((6,), s, dtype=torch.int32)
    tr = _trainer(net)
    tr.compute_grads(planes, (pi, z, (own_t, valid)), sym, weight)
    a, la = _grads(tr), tr._olast[0].clone()
    table = symmetry_tables(9)
    p2, _ = apply_symmetry(planes, None, sym, table)
    pi2 = apply_symmetry_dist(pi, sym, table)
    own2 = apply_symmetry_dist(own_t.double(), sym, table).to(torch.int8)
    tr.compute_grads(p2, (pi2, z, (own2, valid)), None, weight)
    b = _grads(tr)
    for n in a:
        assert torch.allclose(a[n], b[n], rtol=1e-12, atol=1e-15), n
    assert torch.allclose(la, tr._olast[0], rtol=1e-12, atol=0)


# ------------------------------------------------------------------- train-pv end to end
def _own_file(path, n_positions):
    """Positions of finished random 9x9 games through the writer, ownership columns included."""
    from alphago_amd.search.selfplay_mcts import SelfPlayWriter

    w = SelfPlayWriter(str(path), None, features=list(VALUE_FEATURES), size=9, positions_per_game=16, seed=1,
                       ownership=True)
    gid = 0
    while w.positions < n_positions:
        w.add(_record(_random_game(9, 40 + gid), gid, seed=gid))
        gid += 1
    assert w.positions == n_positions
    return w.close()


def test_train_pv_learns_the_ownership_target(tmp_path):
    from alphago_amd.cli import main

    pv = _pv(filters_per_layer=16)
    js = str(tmp_path / "pv.json")
    pv.save_model(js, str(tmp_path / "pv0.hdf5"))
    h5 = tmp_path / "selfplay.h5"
    assert _own_file(h5, 80) == 80
    out = tmp_path / "out"
    metrics = str(tmp_path / "m.jsonl")
    assert main(["train-pv", js, str(h5), str(out), "--minibatch", "16", "--epochs", "12", "--backend", "torch",
                 "--train-val-test", "0.8", "0.2", "0", "--learning-rate", "0.05", "--decay", "0",
                 "--ownership-coef", "2.0", "--metrics", metrics]) == 0
    with open(out / "metadata.json") as f:
        meta = json.load(f)
    assert meta["ownership_coef"] == 2.0
    eps = meta["epochs"]
    for k in ("own_loss", "own_acc", "val_own_loss", "val_own_acc", "loss", "value_loss", "val_loss"):
        assert all(k in e and math.isfinite(e[k]) for e in eps), k
    print("own_loss per epoch:", [round(e["own_loss"], 4) for e in eps])
    assert eps[-1]["own_loss"] < eps[0]["own_loss"]
    assert 0.0 <= eps[-1]["own_acc"] <= 1.0
    with open(metrics) as f:
        assert "own_loss" in json.loads(f.readline())


def test_train_pv_needs_the_datasets_and_plain_models_ignore_them(tmp_path):
    from alphago_amd.cli import main

    _, recs = _three_games()
    _write(tmp_path / "plain.h5", recs)
    _write(tmp_path / "own.h5", recs, ownership=True)
    js = str(tmp_path / "pv.json")
    _pv().save_model(js, str(tmp_path / "pv0.hdf5"))
    args = ["--minibatch", "8", "--epochs", "1", "--backend", "torch", "--train-val-test", "1", "0", "0"]
    with pytest.raises(ValueError, match="ownership"):
        main(["train-pv", js, str(tmp_path / "plain.h5"), str(tmp_path / "o1")] + args)
    js0 = str(tmp_path / "pv0.json")
    _pv(0).save_model(js0, str(tmp_path / "pv00.hdf5"))
    assert main(["train-pv", js0, str(tmp_path / "own.h5"), str(tmp_path / "o2")] + args) == 0
    with open(tmp_path / "o2" / "metadata.json") as f:
        ep = json.load(f)["epochs"][0]
    assert "own_loss" not in ep and "value_loss" in ep


# --------------------------------------------------------------------------------- GTP
def test_gtp_ownership():
    from alphago_amd.gtp.engine import GTPEngine
    from alphago_amd.search.players import GreedyPolicyPlayer

    pv = _pv()
    eng = GTPEngine(GreedyPolicyPlayer(pv), size=9)
    assert eng.send("known_command ownership") == "= true\n\n"
    assert "ownership" in eng.send("list_commands")
    eng.send("play b e5")
    reply = eng.send("ownership")
    assert reply.startswith("= ") and reply.endswith("\n\n")
    rows = [r.split() for r in reply[2:].strip().split("\n")]
    assert len(rows) == 9 and all(len(r) == 9 for r in rows)
    vals = np.array([[float(v) for v in r] for r in rows])
    assert (np.abs(vals) <= 1).all() and all(len(v.split(".")[1]) == 2 for r in rows for v in r)
    # + = Black, top row first: row i of the reply is y = 8 - i, column x
    own = pv.eval_ownership(eng.state)
    assert own.shape == (9, 9)
    assert np.allclose(vals, np.round(own.T[::-1], 2), atol=0.0051)
    mover = pv.model.ownership_torch(pv.model.trunk.forward_torch(
        torch.from_numpy(pv.preprocessor.states_to_uint8([eng.state])).float())).detach().numpy().reshape(9, 9)
    assert np.allclose(own, mover * eng.state.current_player, atol=1e-6)
    plain = GTPEngine(GreedyPolicyPlayer(_pv(0)), size=9)
    assert plain.send("ownership") == "? no ownership head\n\n"
