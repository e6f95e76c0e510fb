"""Entropy bonus, KL anchor, KL-bounded steps and the policy diagnostics of ``train-rl`` on the
autograd backend (9 x 9 board, tiny net, CPU)."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from alphago_amd.models.policy import CNNPolicy
from alphago_amd.search.selfplay import GameRecords
from alphago_amd.train import rl
from alphago_amd.train.engine import TorchPolicyTrainer

FEATS = ["board", "ones", "turns_since", "sensibleness"]
CPU = torch.device("cpu")
B = 16


def _policy(seed):
    torch.manual_seed(seed)
    return CNNPolicy(FEATS, board=9, filters_per_layer=16, layers=2, device=CPU)


def _records(pol, winners, colors, n_pos=4, seed=0):
    """One game of ``n_pos`` random positions per winner / learner-colour pair."""
    rng = np.random.default_rng(seed)
    C = pol.preprocessor.output_dim
    planes = [rng.integers(0, 2, (n_pos, C, 9, 9), dtype=np.uint8) for _ in winners]
    moves = [rng.integers(0, 81, n_pos).astype(np.int32) for _ in winners]
    return GameRecords(planes=planes, moves=moves, winners=list(winners), learner_colors=list(colors))


# with the mean baseline an iteration lost entirely has z - b = 0 at every position: the REINFORCE
# term vanishes and only the regularisers move the weights
ALL_LOST = dict(winners=[-1, -1, -1, -1], colors=[1, 1, 1, 1])
MIXED = dict(winners=[1, 1, -1, -1], colors=[1, -1, 1, -1])


def _probs_of(model):
    @torch.no_grad()
    def f(planes):
        return torch.softmax(model.logits_torch(torch.as_tensor(planes).float()), 1)
    return f


def _all_planes(rec):
    return torch.from_numpy(np.concatenate(rec.planes))


def test_trainer_gradients_match_independent_fp64_objective():
    pol = _policy(0)
    net64 = copy.deepcopy(pol.model).double()
    tr = TorchPolicyTrainer(pol.model, 8, lr=0.1, device="cpu")
    g = torch.Generator().manual_seed(1)
    planes = torch.randint(0, 2, (8, pol.preprocessor.output_dim, 9, 9), generator=g, dtype=torch.uint8)
    tgt = torch.randint(0, 81, (8,), generator=g, dtype=torch.int32)
    tgt[3] = -1
    wt = torch.tensor([1.0, -1.0, 2.0, -0.5, 1.0, 3.0, 0.0, 0.25])
    q = torch.softmax(torch.randn(8, 81, generator=g), 1)
    q[1, :8] = 0.0
    q[1] /= q[1].sum()
    beta, kappa = 0.3, 0.7
    tr.ent_coef, tr.kl_coef, tr.ref_probs = beta, kappa, q
    tr.compute_grads(planes, tgt, None, wt)
    # the objective of the fused head, written out: explicit softmax / log_softmax in fp64
    h = net64.trunk.forward_torch(planes.double())
    z = F.conv2d(h, net64.head_w, net64.head_b).flatten(1)
    p, logp = torch.softmax(z, 1), torch.log_softmax(z, 1)
    q64 = q.double()
    total = 0.0
    for b in range(8):
        if tgt[b] < 0:
            continue
        ent = -(p[b] * logp[b]).sum()
        nz = q64[b] > 0
        kl = (q64[b][nz] * (q64[b][nz].log() - logp[b][nz])).sum()
        total = total - wt[b].double() * logp[b, tgt[b].long()] - beta * ent + kappa * kl
    (total / 8).backward()
    ref = {"head_w": net64.head_w.grad, "head_b": net64.head_b.grad}
    for l in range(net64.trunk.layers):
        ref["w%d" % l], ref["b%d" % l] = net64.trunk.weights[l].grad, net64.trunk.biases[l].grad
    for name in tr.fp.names:
        a, r = tr.fp.grad_views[name].double(), ref[name].reshape(tr.fp.grad_views[name].shape)
        if name == "head_b":  # every term is invariant to a shift of the logits: a cancelling sum, 0 exactly
            assert abs(a.item()) < 1e-5 and abs(r.item()) < 1e-12
            continue
        # fp32 trainer against fp64: 2^-24 per operation over sums of at most 8 * 81 * 16 * 9 terms
        assert (a - r).abs().max().item() <= 1e-4 * max(r.abs().max().item(), 1e-3), name
    # the coefficients really entered: the plain gradient differs
    tr.ent_coef = tr.kl_coef = 0.0
    g_reg = tr.fp.grad.clone()
    tr.compute_grads(planes, tgt, None, wt)
    assert (tr.fp.grad - g_reg).abs().max() > 1e-4
    # the reference binary CE takes no regulariser
    tr.ent_coef, tr.policy_loss = 0.1, "bce"
    with pytest.raises(ValueError):
        tr.compute_grads(planes, tgt, None, wt)


def test_rl_update_stats_and_defaults():
    pol = _policy(0)
    rec = _records(pol, **MIXED)
    mk = lambda: TorchPolicyTrainer(copy.deepcopy(pol.model), B, lr=0.5, device="cpu")  # noqa: E731
    a, b, c, d = mk(), mk(), mk(), mk()
    today = rl.rl_update(a, rec, B, CPU)
    assert set(today) == {"positions", "mean_reward", "baseline", "grad_norm", "skipped"}
    same = rl.rl_update(b, rec, B, CPU, entropy_coef=0.0, kl_coef=0.0, anchor=None, max_kl=0.0, stats=False)
    assert same == today and torch.equal(a.fp.flat, b.fp.flat)
    assert b.head_stats is None and b.head_probs is None and b.ref_probs is None
    info = rl.rl_update(c, rec, B, CPU, stats=True)
    assert "kl_anchor" not in info and torch.equal(c.fp.flat, a.fp.flat)  # logging changes no weight
    planes = _all_planes(rec)
    logits = pol.model.logits_torch(planes.float()).detach()
    lp = torch.log_softmax(logits, 1)
    assert abs(info["entropy"] - float(-(lp.exp() * lp).sum(1).mean())) < 1e-5
    assert abs(info["max_abs_logit"] - float(logits.abs().max())) < 1e-6
    assert {k: info[k] for k in today} == today
    assert (c.ent_coef, c.kl_coef, c.collect_stats, c.collect_probs) == (0.0, 0.0, False, False)
    # the learner as its own anchor: KL 0
    info = rl.rl_update(d, rec, B, CPU, stats=True, anchor=_probs_of(d.net))
    assert abs(info["kl_anchor"]) < 1e-6 and torch.equal(d.fp.flat, a.fp.flat)
    with pytest.raises(ValueError):
        rl.rl_update(d, rec, B, CPU, kl_coef=0.1)  # no anchor
    with pytest.raises(ValueError):
        rl.rl_update(d, rec, B, CPU, entropy_coef=-1.0)
    with pytest.raises(ValueError):
        rl.rl_update(d, rec, B, CPU, loss="reference", entropy_coef=0.1)


def test_more_chunks_than_one_average_over_positions():
    """n = 16 positions in chunks of 8 (and a padded chunk of 12): the same means and the same update
    as one chunk of 16."""
    pol = _policy(0)
    rec = _records(pol, **MIXED)
    anchor = _probs_of(_policy(7).model)
    out = []
    for chunk in (16, 8, 12):
        tr = TorchPolicyTrainer(copy.deepcopy(pol.model), chunk, lr=0.5, device="cpu")
        info = rl.rl_update(tr, rec, chunk, CPU, entropy_coef=0.2, kl_coef=0.4, anchor=anchor)
        out.append((info, tr.fp.flat.clone()))
    for info, flat in out[1:]:
        for k in ("entropy", "kl_anchor", "max_abs_logit", "grad_norm"):
            assert abs(info[k] - out[0][0][k]) < 1e-5 * max(1.0, abs(out[0][0][k])), k
        assert torch.allclose(flat, out[0][1], atol=1e-6)


def test_entropy_bonus_raises_entropy():
    pol = _policy(0)
    with torch.no_grad():
        pol.model.head_w.mul_(20.0)  # a peaked policy: room to rise
    rec = _records(pol, **ALL_LOST)
    tr = TorchPolicyTrainer(pol.model, B, lr=0.05, device="cpu")
    planes = _all_planes(rec)
    h0 = float(tr.policy_stats(planes)[:, 0].mean())
    info = rl.rl_update(tr, rec, B, CPU, entropy_coef=1.0)
    assert info["baseline"] == -1.0 and abs(info["entropy"] - h0) < 1e-5  # measured before the step
    assert info["grad_norm"] > 0  # from the bonus alone: every reward is 0
    h1 = float(tr.policy_stats(planes)[:, 0].mean())
    assert h1 > h0, (h0, h1)


def test_kl_anchor_pulls_towards_anchor():
    pol, other = _policy(0), _policy(7)
    with torch.no_grad():
        other.model.head_w.mul_(20.0)  # an anchor far from the learner
    anchor = _probs_of(other.model)
    rec = _records(pol, **ALL_LOST)
    tr = TorchPolicyTrainer(pol.model, B, lr=0.05, device="cpu")
    planes = _all_planes(rec)
    q = anchor(planes)
    k0 = float(tr.policy_stats(planes, q)[:, 1].mean())
    info = rl.rl_update(tr, rec, B, CPU, kl_coef=1.0, anchor=anchor)
    assert abs(info["kl_anchor"] - k0) < 1e-5 * max(1.0, k0) and info["grad_norm"] > 0
    k1 = float(tr.policy_stats(planes, q)[:, 1].mean())
    assert k1 < k0, (k0, k1)


def test_kl_bounded_step():
    pol = _policy(0)
    rec = _records(pol, **MIXED)
    mk = lambda lr, **kw: TorchPolicyTrainer(copy.deepcopy(pol.model), B, lr=lr, device="cpu", **kw)  # noqa: E731
    free = mk(50.0)
    w0 = free.fp.flat.clone()
    unb = rl.rl_update(free, rec, B, CPU, max_kl=1e9)  # measures the unbounded step
    assert unb["kl_backtracks"] == 0 and unb["step_scale"] == 1.0 and unb["kl_step"] > 1e-3
    plain = mk(50.0)
    rl.rl_update(plain, rec, B, CPU)
    assert torch.equal(plain.fp.flat, free.fp.flat)
    # kl_step is KL(old || new) over the first chunk
    planes = _all_planes(rec)
    lp_old = torch.log_softmax(pol.model.logits_torch(planes.float()).detach(), 1)
    lp_new = torch.log_softmax(free.net.logits_torch(planes.float()).detach(), 1)
    assert abs(unb["kl_step"] - float((lp_old.exp() * (lp_old - lp_new)).sum(1).mean())) < 1e-5 * max(1, unb["kl_step"])
    # KL grows with the square of a small step: a bound 10 times lower needs about two halvings
    max_kl = unb["kl_step"] / 10.0
    tr = mk(50.0)
    info = rl.rl_update(tr, rec, B, CPU, max_kl=max_kl)
    k = info["kl_backtracks"]
    assert 1 <= k <= 8 and info["step_scale"] == 0.5 ** k and info["kl_step"] <= max_kl
    assert torch.allclose(tr.fp.flat, w0 + info["step_scale"] * (free.fp.flat - w0), rtol=0, atol=1e-6)
    assert tr.sched.iterations == free.sched.iterations == 1
    # a bound no halving reaches: the old weights come back
    # (lr 200: 1/256 of that step still moves the policy by a KL far above fp32 noise)
    tr = mk(200.0)
    info = rl.rl_update(tr, rec, B, CPU, max_kl=1e-12)
    assert info["kl_backtracks"] == 8 and info["step_scale"] == 0.0 and info["kl_step"] == 0.0
    assert torch.equal(tr.fp.flat, w0) and tr.sched.iterations == 1
    # a tiny step passes untouched
    a, b = mk(1e-6), mk(1e-6)
    info = rl.rl_update(a, rec, B, CPU, max_kl=0.01)
    rl.rl_update(b, rec, B, CPU)
    assert info["kl_backtracks"] == 0 and info["step_scale"] == 1.0 and info["kl_step"] <= 0.01
    assert torch.equal(a.fp.flat, b.fp.flat)
    with pytest.raises(ValueError, match="plain SGD"):
        rl.rl_update(mk(0.1, optimizer="momentum", momentum=0.9), rec, B, CPU, max_kl=0.01)


FLAGS = ["--entropy-coef", "0.01", "--kl-coef", "0.1", "--max-kl", "0.01", "--backend", "torch"]
NEW_FIELDS = ("entropy", "kl_anchor", "max_abs_logit", "kl_step", "kl_backtracks", "step_scale")


def _save_policy(tmp_path):
    p = _policy(0)
    j, w = str(tmp_path / "p.json"), str(tmp_path / "p.hdf5")
    p.save_model(j, w)
    return j, w


def test_cli_writes_new_fields(tmp_path):
    j, w = _save_policy(tmp_path)
    metrics = str(tmp_path / "m.jsonl")
    out = rl.run([w, j, "--game_batch_size", "4", "--iterations", "2", "--minibatch", "64", "--max-moves", "60",
                  "--metrics", metrics] + FLAGS)
    with open(metrics) as f:
        rows = [json.loads(line) for line in f]
    assert len(rows) == 2 and len(out["history"]) == 2
    for row, hist in zip(rows, out["history"]):
        for k in NEW_FIELDS:
            assert k in row and row[k] == hist[k], k
        assert 0 < row["entropy"] <= np.log(81) + 1e-6 and row["kl_anchor"] >= -1e-6
    assert abs(rows[0]["kl_anchor"]) < 1e-6  # iteration 0: the learner is the anchor
    # --log-policy-stats alone: the diagnostics, no bounded step
    out = rl.run([w, j, "--game_batch_size", "4", "--iterations", "1", "--minibatch", "64", "--max-moves", "60",
                  "--log-policy-stats", "--backend", "torch"])
    row = out["history"][0]
    assert "entropy" in row and "kl_anchor" in row and "max_abs_logit" in row and "kl_step" not in row
    # defaults: none of the new fields
    out = rl.run([w, j, "--game_batch_size", "4", "--iterations", "1", "--minibatch", "64", "--max-moves", "60",
                  "--backend", "torch"])
    assert not set(NEW_FIELDS) & set(out["history"][0])


def test_resume_after_injected_fault_is_bit_identical_with_options(tmp_path, monkeypatch):
    from alphago_amd.train import checkpoint as ckpt
    from alphago_amd.utils import faults

    j, w = _save_policy(tmp_path)

    def args(folder):
        return [w, j, "--model_folder", folder, "--game_batch_size", "3", "--iterations", "4", "--save_every", "1",
                "--minibatch", "32", "--max-moves", "60", "--resume", "--seed", "3"] + FLAGS

    ref = rl.run(args(str(tmp_path / "ref")))
    marker = str(tmp_path / "fired")
    monkeypatch.setenv("ALPHAGO_AMD_FAULT", "raise@2:once=%s" % marker)
    faults.reload_from_env()
    try:
        with pytest.raises(faults.InjectedFault):
            rl.run(args(str(tmp_path / "run")))
        mid = ckpt.load(str(tmp_path / "run" / "rl_checkpoint.pt"))
        assert mid["iteration"] == 2
        got = rl.run(args(str(tmp_path / "run")))
    finally:
        monkeypatch.delenv("ALPHAGO_AMD_FAULT")
        faults.reload_from_env()
    a = ckpt.load(str(tmp_path / "ref" / "rl_checkpoint.pt"))
    b = ckpt.load(str(tmp_path / "run" / "rl_checkpoint.pt"))
    assert torch.equal(a["trainer"]["flat"], b["trainer"]["flat"])
    assert a["trainer"]["iterations"] == b["trainer"]["iterations"]
    assert [os.path.basename(p) for p in a["pool"]] == [os.path.basename(p) for p in b["pool"]]
    strip = lambda h: [{k: v for k, v in r.items() if not k.endswith("_per_s")} for r in h]  # noqa: E731
    assert strip(ref["history"]) == strip(got["history"])
    assert all(k in got["history"][-1] for k in NEW_FIELDS)
