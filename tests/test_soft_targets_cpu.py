"""Soft (distribution) policy targets without a GPU: the autograd trainer's objective, the D4
transform of a distribution, selfplay-to-sl --target dist, PositionDataset(targets="pi") and
train-sl --targets pi on the torch backend."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from alphago_amd.data.dataset import PositionDataset
from alphago_amd.data.selfplay_to_sl import selfplay_to_sl
from alphago_amd.features import DEFAULT_FEATURES, VALUE_FEATURES
from alphago_amd.io.h5lite import H5File, H5Writer
from alphago_amd.models.nets import PolicyNet
from alphago_amd.train.engine import (TorchPolicyTrainer, apply_symmetry, apply_symmetry_dist, is_soft_target,
                                      symmetry_tables)

S = 9
SS = S * S


def _net(C=6):
    torch.manual_seed(3)
    return PolicyNet(C, board=S, filters_per_layer=8, layers=2)


def _batch(B=5, C=6, T=SS + 1, seed=0):
    g = torch.Generator().manual_seed(seed)
    planes = torch.randint(0, 2, (B, C, S, S), dtype=torch.uint8, generator=g)
    dist = torch.rand(B, T, generator=g)
    dist[0, :SS] = 0          # all mass on the pass (T = SS + 1) / an all-zero row
    dist[1, 3] = -0.5         # a negative entry counts as 0
    dist[2] = 0
    dist[2, 7] = 1.0          # exact one-hot
    return planes, dist


def test_is_soft_target():
    assert is_soft_target(torch.zeros(4, SS)) and is_soft_target(torch.zeros(4, SS + 1, dtype=torch.float64))
    assert not is_soft_target(torch.zeros(4, dtype=torch.int32)) and not is_soft_target(torch.zeros(4))


@pytest.mark.parametrize("T", [SS, SS + 1])
def test_torch_soft_loss_matches_formula(T):
    """Loss, top-1 and parameter gradients of TorchPolicyTrainer on soft targets against the
    formula written out by hand: q = max(dist, 0) on the board, qh = q / sum q,
    L = 1/B sum_b w_b (-sum_i qh_i log p_i) over the boards with mass."""
    net = _net()
    planes, dist = _batch(T=T)
    B = planes.shape[0]
    wt = torch.tensor([1.0, -1.0, 2.0, -0.5, 3.0])
    tr = TorchPolicyTrainer(copy.deepcopy(net), B, lr=0.01, device="cpu")
    tr.compute_grads(planes, dist, None, wt)
    per, corr = tr._last
    # by hand, in float64 on a copy of the net
    net64 = copy.deepcopy(net).double()
    z = net64.logits_torch(planes.double())
    p = torch.softmax(z, 1)
    loss = torch.zeros(B, dtype=torch.float64)
    hit = torch.zeros(B)
    obj = 0.0
    for b in range(B):
        q = dist[b, :SS].double().clamp_min(0)
        m = q.sum()
        if m > 0:
            loss[b] = -((q / m) * p[b].log()).sum()
            hit[b] = float(int(z[b].argmax()) == int(q.argmax()))
            obj = obj + wt[b].double() * loss[b]
    (obj / B).backward()
    assert loss[0].item() == 0 and per[0].item() == 0 and corr[0].item() == 0  # no board mass: no loss
    assert torch.allclose(per.double(), loss.detach(), rtol=1e-5, atol=1e-6)
    assert torch.equal(corr, hit)
    named = dict(net64.named_parameters())
    checked = 0
    for name, prm in tr.net.named_parameters():
        g64 = named[name].grad
        checked += 1
        if name == "head_b":  # sum_i (p_i - qh_i) == 0 exactly: only roundoff is left (test_hip_trainer.py's bound)
            assert abs(prm.grad.item()) < 1e-5 and abs(g64.item()) < 1e-5
            continue
        assert torch.allclose(prm.grad.double(), g64, rtol=1e-4, atol=1e-7), name
    assert checked >= 5
    # evaluate: the same sums, no gradient
    l, c = tr.evaluate(planes, dist)
    assert abs(l.item() - loss.sum().item()) < 1e-4 and c.item() == hit.sum().item()


def test_one_hot_soft_targets_give_integer_target_gradients():
    net = _net()
    planes, _ = _batch()
    B = planes.shape[0]
    g = torch.Generator().manual_seed(1)
    t = torch.randint(0, SS, (B,), generator=g, dtype=torch.int32)
    t[3] = -1  # no target <-> all-zero row
    sym = torch.tensor([0, 3, 5, 7, 1], dtype=torch.int32)
    dist = torch.zeros(B, SS + 1)
    for b in range(B):
        if t[b] >= 0:
            dist[b, t[b]] = 1.0
    a = TorchPolicyTrainer(copy.deepcopy(net), B, lr=0.01, device="cpu")
    s = TorchPolicyTrainer(copy.deepcopy(net), B, lr=0.01, device="cpu")
    a.compute_grads(planes, t, sym)
    s.compute_grads(planes, dist, sym)
    assert torch.allclose(a.fp.grad, s.fp.grad, rtol=1e-5, atol=1e-7)
    assert torch.allclose(a._last[0], s._last[0], rtol=1e-5, atol=1e-6) and torch.equal(a._last[1], s._last[1])


@pytest.mark.parametrize("n", [9, 19])
def test_distribution_symmetry_agrees_with_integer_targets(n):
    """For all 8 symmetries a one-hot row moves exactly as apply_symmetry moves the integer target,
    a dense row is the same permutation of its entries, and the pass column stays."""
    table = symmetry_tables(n)
    nn = n * n
    g = torch.Generator().manual_seed(n)
    for s in range(8):
        B = 6
        sym = torch.full((B,), s, dtype=torch.int32)
        t = torch.randint(0, nn, (B,), generator=g, dtype=torch.int32)
        planes = torch.zeros(B, 1, n, n, dtype=torch.uint8)
        planes.view(B, nn)[torch.arange(B), t.long()] = 1
        pl, tt = apply_symmetry(planes, t, sym, table)
        assert torch.equal(pl.view(B, nn).argmax(1), tt)  # planes and targets move together
        for T in (nn, nn + 1):
            hot = torch.zeros(B, T)
            hot[torch.arange(B), t.long()] = 1.0
            out = apply_symmetry_dist(hot, sym, table)
            assert torch.equal(out[:, :nn].argmax(1), tt) and bool((out.sum(1) == 1).all())
            dense = torch.rand(B, T, generator=g)
            out = apply_symmetry_dist(dense, sym, table)
            # the mass at the stone's point follows the stone
            assert torch.equal(out[torch.arange(B), tt], dense[torch.arange(B), t.long()])
            assert torch.equal(out[:, :nn].sort(1).values, dense[:, :nn].sort(1).values)
            if T == nn + 1:
                assert torch.equal(out[:, nn], dense[:, nn])
    with pytest.raises(ValueError):
        apply_symmetry_dist(torch.zeros(2, nn + 2), torch.zeros(2, dtype=torch.int32), table)


def _selfplay_file(path, n=40, seed=0):
    """A synthetic selfplay-mcts file at S = 9: value planes, pi (n, S*S + 1), moves, outcomes, game.
    Row 0's most-visited move is the pass, row 1 has all its mass on the pass."""
    rng = np.random.default_rng(seed)
    states = rng.integers(0, 2, (n, _value_planes(), S, S), dtype=np.uint8)
    pi = np.zeros((n, SS + 1), np.float32)
    for r in range(n):
        pts = rng.choice(SS + 1, 10, replace=False)
        cnt = rng.permutation(np.array([20, 9, 8, 7, 6, 5, 4, 3, 1, 1]))
        pi[r, pts] = cnt / 64.0
    pi[0] = 0
    pi[0, SS] = 0.5
    pi[0, 4] = 0.25
    pi[0, 5] = 0.25
    pi[1] = 0
    pi[1, SS] = 1.0
    with H5Writer(path) as w:
        w.attrs["features"] = np.array([x.encode() for x in VALUE_FEATURES])
        w.attrs["board_size"] = np.int64(S)
        w.create_dataset("states", data=states)
        w.create_dataset("pi", data=pi)
        w.create_dataset("moves", data=pi.argmax(1).astype(np.int16))
        w.create_dataset("outcomes", data=rng.integers(-1, 2, n).astype(np.int8))
        w.create_dataset("game", data=np.zeros(n, np.int32))
    return states, pi


def _value_planes():
    from alphago_amd.preprocessing.preprocessing import Preprocess

    return Preprocess(list(VALUE_FEATURES)).output_dim


@pytest.fixture(scope="module")
def dist_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("soft")
    sp, dst = str(d / "selfplay.h5"), str(d / "sl_dist.h5")
    states, pi = _selfplay_file(sp)
    res = selfplay_to_sl(sp, dst, "dist")
    return sp, dst, states, pi, res


def test_selfplay_to_sl_dist(dist_file, tmp_path):
    sp, dst, states, pi, res = dist_file
    keep = np.flatnonzero(pi.argmax(1) < SS)
    assert res == {"positions": len(pi), "written": len(keep), "dropped_pass": len(pi) - len(keep), "target": "dist"}
    assert 0 not in keep and 1 not in keep and res["dropped_pass"] >= 2  # pass-argmax rows are dropped
    hard = str(tmp_path / "hard.h5")
    assert selfplay_to_sl(sp, hard, "pi")["written"] == len(keep)  # the same rows as --target pi
    with H5File(dst) as f, H5File(hard) as h:
        st, acts, out = np.asarray(f["states"].read()), np.asarray(f["actions"].read()), np.asarray(f["pi"].read())
        assert np.array_equal(st, np.asarray(h["states"].read())) and np.array_equal(acts, np.asarray(h["actions"].read()))
        assert "pi" not in h
    assert np.array_equal(st, states[keep][:, :_policy_planes()])
    assert out.dtype == np.float32 and out.shape == (len(keep), SS)
    assert np.allclose(out.sum(1), 1.0, atol=1e-6)
    board = pi[keep][:, :SS].astype(np.float64)
    assert np.allclose(out, board / board.sum(1, keepdims=True), atol=1e-7)
    assert np.array_equal(acts[:, 0].astype(int) * S + acts[:, 1], out.argmax(1))
    assert (board.sum(1) < 0.99).any()  # some kept rows had pass visits: the renormalisation did something
    with pytest.raises(ValueError):
        selfplay_to_sl(sp, hard, "visits")


def _policy_planes():
    from alphago_amd.preprocessing.preprocessing import Preprocess

    return Preprocess(list(DEFAULT_FEATURES)).output_dim


def _rewrite(src, dst, mutate):
    with H5File(src) as f:
        st, acts, pi = (np.asarray(f[k].read()).copy() for k in ("states", "actions", "pi"))
        attrs = {k: np.asarray(f.attrs[k]) for k in ("features", "board_size")}
    pi = mutate(pi)
    with H5Writer(dst) as w:
        for k, v in attrs.items():
            w.attrs[k] = v
        w.create_dataset("states", data=st)
        w.create_dataset("actions", data=acts)
        if pi is not None:
            w.create_dataset("pi", data=pi)


def test_position_dataset_pi(dist_file, tmp_path):
    _, dst, _, _, res = dist_file
    with H5File(dst) as f:
        pi = np.asarray(f["pi"].read())
        st = np.asarray(f["states"].read())
    rows = np.array([5, 2, 9, 0, 7, 3])
    pos = np.array([4, 0, 5, 1])
    for resident in ("yes", "no"):
        ds = PositionDataset(dst, device="cpu", resident=resident, rows=rows, targets="pi")
        assert ds.resident == (resident == "yes") and ds.target_shape == (SS,)
        planes, dist = ds.batch(pos)
        assert dist.dtype == torch.float32 and tuple(dist.shape) == (4, SS)
        assert np.array_equal(dist.numpy(), pi[rows[pos]]) and np.array_equal(planes.numpy(), st[rows[pos]])
        if resident == "no":  # the prefetch ring carries (B, T) targets too
            pf = ds.prefetch([pos, pos[::-1].copy()], 4)
            got = [(p.clone(), d.clone()) for p, d in pf]
            pf.close()
            assert len(got) == 2 and np.array_equal(got[1][1].numpy(), pi[rows[pos[::-1]]])
            assert np.array_equal(got[0][0].numpy(), st[rows[pos]])
        ds.close()
    # the move targets of the same file still load
    hard = PositionDataset(dst, device="cpu", targets="actions")
    assert np.array_equal(hard.targets_np, pi.argmax(1).astype(np.int32)) and hard.target_shape == ()
    hard.close()

    def put(i, j, v):
        def f(p):
            p[i, j] = v
            return p
        return f

    def zero_row(p):
        p[3] = 0
        return p

    bad = str(tmp_path / "bad.h5")
    for mutate in (put(2, 5, np.nan), put(2, 5, np.inf), put(4, 1, -0.25), zero_row):
        _rewrite(dst, bad, mutate)
        with pytest.raises(ValueError, match="bad.h5"):
            PositionDataset(bad, device="cpu", targets="pi")
    _rewrite(dst, bad, lambda p: None)
    with pytest.raises(KeyError, match="bad.h5"):
        PositionDataset(bad, device="cpu", targets="pi")


def _model(tmp_path):
    from alphago_amd.models.policy import CNNPolicy

    pol = CNNPolicy(list(DEFAULT_FEATURES), board=S, filters_per_layer=8, layers=2, device="cpu")
    j = str(tmp_path / "model.json")
    pol.save_model(j)
    return j


def test_train_sl_targets_pi_torch_backend(dist_file, tmp_path):
    """Two steps of train-sl --targets pi on the torch backend; the validation shard's short last
    batch is padded with all-zero rows; metadata.json records the target kind."""
    from alphago_amd.train.sl import run_training

    _, dst, _, _, _ = dist_file
    out = str(tmp_path / "out")
    meta = run_training([_model(tmp_path), dst, out, "--epochs", "1", "-l", "16", "-B", "8", "--backend", "torch",
                         "--targets", "pi", "--train-val-test", "0.7", "0.3", "0.0"])
    ep = meta["epochs"]
    assert len(ep) == 1 and np.isfinite(ep[0]["loss"]) and ep[0]["loss"] > 0 and np.isfinite(ep[0]["val_loss"])
    assert 0.0 <= ep[0]["acc"] <= 1.0 and 0.0 <= ep[0]["val_acc"] <= 1.0
    with open(os.path.join(out, "metadata.json")) as f:
        assert json.load(f)["targets"] == "pi"
    # the default is the hard path, on the same file
    out2 = str(tmp_path / "out2")
    meta = run_training([_model(tmp_path), dst, out2, "--epochs", "1", "-l", "16", "-B", "8", "--backend", "torch"])
    assert meta["targets"] == "actions" and np.isfinite(meta["epochs"][0]["loss"])


def test_train_sl_refuses_graph_with_pi_targets(dist_file, tmp_path, capsys):
    from alphago_amd.train.sl import run_training

    _, dst, _, _, _ = dist_file
    with pytest.raises(SystemExit) as e:
        run_training([_model(tmp_path), dst, str(tmp_path / "o"), "--graph", "--targets", "pi"])
    assert e.value.code == 2 and "--targets pi" in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "o"))


def test_soft_target_loss_tie_rule_and_edge_entries():
    """soft_target_loss follows the kernel: both top-1 indices are the smallest among the maxima
    (visit counts tie), a zero target on a -inf log-probability adds nothing, NaN entries count as 0
    and a row with an infinite entry has no loss."""
    from alphago_amd.train.engine import first_argmax, soft_target_loss

    z = torch.zeros(5, SS)
    z[0, [7, 30]] = 2.0             # tied logits: the first, 7
    z[1, 12] = 1.0
    z[2, 0] = float("-inf")         # p_0 = 0 where the target is 0
    z[3, 5] = 1.0
    z[4, 5] = 1.0
    d = torch.zeros(5, SS + 1)
    d[0, [30, 7, 50]] = torch.tensor([0.25, 0.25, 0.125])   # tied visit counts: the first, 7
    d[1, [40, 12]] = 0.5                                    # first maximum is 12
    d[2, 3] = 1.0
    d[3, 5] = 1.0
    d[3, 9] = float("nan")
    d[4, 5] = float("inf")
    assert first_argmax(z).tolist()[:2] == [7, 12] and first_argmax(d[:, :SS])[:2].tolist() == [7, 12]
    ce, correct, has = soft_target_loss(z, d)
    assert has.tolist() == [True, True, True, True, False] and correct.tolist() == [1.0, 1.0, 0.0, 1.0, 0.0]
    assert bool(torch.isfinite(ce).all()) and ce[4].item() == 0
    logp = torch.log_softmax(z.double(), 1)
    assert abs(ce[2].item() + logp[2, 3].item()) < 1e-6 and abs(ce[3].item() + logp[3, 5].item()) < 1e-6
    assert abs(ce[0].item() + (0.4 * logp[0, 30] + 0.4 * logp[0, 7] + 0.2 * logp[0, 50]).item()) < 1e-6


def test_position_dataset_pi_validates_its_own_rows_only(dist_file, tmp_path):
    """A rank reads and checks its shard of 'pi', not the whole file: a bad row outside the shard
    does not stop it, the same row inside does."""
    _, dst, _, _, _ = dist_file
    bad = str(tmp_path / "bad.h5")

    def poison(p):
        p[6, 2] = np.nan
        return p

    _rewrite(dst, bad, poison)
    ds = PositionDataset(bad, device="cpu", rows=np.array([9, 0, 3]), targets="pi")
    assert ds.targets_np.shape == (3, SS) and np.isfinite(ds.targets_np).all()
    ds.close()
    with pytest.raises(ValueError, match="bad.h5"):
        PositionDataset(bad, device="cpu", rows=np.array([9, 6, 3]), targets="pi")
