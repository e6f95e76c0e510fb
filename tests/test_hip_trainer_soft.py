"""HipPolicyTrainer on soft (distribution) targets vs the autograd fp32 trainer: a small 9 x 9 net at
B = 8 (1024-thread head) and B = 264 (512-thread, row-mapped head)."""
import copy

import pytest
import torch

from alphago_amd.models.nets import PolicyNet
from alphago_amd.train.engine import HipPolicyTrainer, TorchPolicyTrainer

pytestmark = pytest.mark.gpu

S, C, F, L = 9, 48, 32, 3
SS = S * S


PEAK_GAP = 1.0  # the leading logit's margin the tests require: 50 x the 2e-2 a bf16 trunk is allowed to move a loss


def _setup(dev, B, seed=0):
    """A random-init net with one hand-set path that decides every board's top-1: plane 0 holds one
    stone per board, channel 0 of every layer carries 4 x that plane and nothing else (exact in
    bf16), and the head reads it with weight 1.5, so the stone's logit leads by about 6 while all
    other weights, and all other channels' view of channel 0, stay random.  Odd boards have their
    target maximum on that point, even boards on a random other one: both outcomes of the top-1
    flag occur.  Returns the net, planes, targets (with the pass column; row 1 has no board mass,
    row 2 a negative entry), a symmetry per board and the stone's point per board."""
    torch.manual_seed(seed)
    net = PolicyNet(C, board=S, filters_per_layer=F, layers=L)
    with torch.no_grad():
        for l, w in enumerate(net.trunk.weights):
            k = w.shape[2] // 2
            w[0] = 0
            w[0, 0, k, k] = 4.0 if l == 0 else 1.0
        net.head_w[0, 0, 0, 0] = 1.5
    g = torch.Generator().manual_seed(seed + B)
    planes = torch.randint(0, 2, (B, C, S, S), dtype=torch.uint8, generator=g)
    top = torch.randint(0, SS, (B,), generator=g)
    planes[:, 0] = 0
    planes[:, 0].view(B, SS)[torch.arange(B), top] = 1
    dist = torch.zeros(B, SS + 1)
    counts = torch.tensor([20., 9., 8., 7., 6., 5., 4., 3., 1., 1.]) / 64
    for b in range(B):
        peak = int(top[b]) if b % 2 == 1 else int((top[b] + 1 + torch.randint(0, SS - 1, (1,), generator=g)) % SS)
        rest = [p for p in torch.randperm(SS + 1, generator=g).tolist() if p != peak][:9]
        dist[b, torch.tensor([peak] + rest)] = counts
    dist[1] = 0
    dist[1, SS] = 1.0
    dist[2, int((dist[2, :SS] == 0).nonzero()[0])] = -0.25
    sym = torch.randint(0, 8, (B,), dtype=torch.int32, generator=g).to(dev)
    return net, planes.to(dev), dist.to(dev), sym, top.to(dev)


def _assert_decided(ref, planes, sym, top):
    """On the fp32 reference alone: every board's leading logit is the stone's point (moved with the
    board) and leads the runner-up by more than PEAK_GAP -- no board is left out."""
    from alphago_amd.train.engine import apply_symmetry

    with torch.no_grad():
        x, tt = (planes, top) if sym is None else apply_symmetry(planes, top, sym, ref.table)
        z = ref.net.logits_torch(x.float())
    top2 = z.topk(2, dim=1)
    assert torch.equal(top2.indices[:, 0], tt.long())
    gap = top2.values[:, 0] - top2.values[:, 1]
    print("leading-logit gap min %.3f" % gap.min().item())
    assert bool((gap > PEAK_GAP).all())


@pytest.mark.parametrize("B", [8, 264])
def test_hip_soft_grads_match_torch(cuda_device, B):
    """One compute_grads with soft targets and a random symmetry per board; the comparison and bounds
    of tests/test_hip_trainer.py::test_hip_grads_match_torch (cosine > 0.98, norm ratio within 5 %,
    loss rtol / atol 2e-2), and the top-1 flags equal on every board (decided by construction)."""
    net, planes, dist, sym, top = _setup(cuda_device, B)
    hip = HipPolicyTrainer(net, B, lr=0.01, device=cuda_device)
    ref = TorchPolicyTrainer(copy.deepcopy(net), B, lr=0.01, device=cuda_device)
    _assert_decided(ref, planes, sym, top)
    hip.compute_grads(planes, dist, sym)
    ref.compute_grads(planes, dist, sym)
    torch.cuda.synchronize()
    for name in hip.fp.names:
        a, b = hip.fp.grad_views[name], ref.fp.grad_views[name]
        if name == "head_b":  # sum_i (p_i - q_i) == 0 exactly
            assert abs(a.item()) < 1e-5 and abs(b.item()) < 1e-5
            continue
        cos = torch.nn.functional.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()
        ratio = a.norm().item() / max(b.norm().item(), 1e-12)
        print(name, "cos %.5f ratio %.4f" % (cos, ratio))
        assert cos > 0.98 and abs(ratio - 1) < 0.05, (name, cos, ratio)
    print("loss max diff %.3g" % (hip.loss - ref._last[0]).abs().max().item())
    assert torch.allclose(hip.loss, ref._last[0], rtol=2e-2, atol=2e-2)
    assert torch.equal(hip.correct, ref._last[1])
    expect = torch.arange(B, device=cuda_device) % 2 == 1
    expect[1] = False  # no board mass
    assert torch.equal(hip.correct.bool(), expect)
    assert hip.loss[1].item() == 0.0 and ref._last[0][1].item() == 0.0
    ls, cs = hip._step_metrics()
    assert abs(ls.item() - hip.loss.sum().item()) < 1e-3 * B and cs.item() == expect.sum().item()


@pytest.mark.parametrize("B", [8, 264])
def test_hip_soft_evaluate_matches_torch(cuda_device, B):
    """evaluate(planes, dist) returns the torch backend's loss sum within test_hip_trainer.py's loss
    bound (rtol / atol 2e-2: the bf16 trunk against fp32 autograd; also per board) and exactly its
    agreement sum: every board's top-1 is decided by construction, which is asserted, and the
    per-board flags are equal.  With the stone's logit about 6 ahead the loss depends on where the
    target mass sits (odd boards, on the stone: low; even boards: high)."""
    net, planes, dist, _, top = _setup(cuda_device, B, seed=1)
    hip = HipPolicyTrainer(net, B, lr=0.01, device=cuda_device)
    ref = TorchPolicyTrainer(copy.deepcopy(net), B, lr=0.01, device=cuda_device)
    _assert_decided(ref, planes, None, top)
    hip.enable_graphs()  # evaluate is eager: a graph-enabled trainer validates soft targets too
    before = hip.fp.flat.clone()
    lh, ch = hip.evaluate(planes, dist)
    lr_, cr = ref.evaluate(planes, dist)
    with torch.no_grad():
        _, per, corr = ref._loss(planes, dist, None, None)
    torch.cuda.synchronize()
    print("evaluate loss hip %.6f torch %.6f, agreement %d / %d" % (lh.item(), lr_.item(), ch.item(), cr.item()))
    assert torch.allclose(hip.loss, per, rtol=2e-2, atol=2e-2)
    assert torch.allclose(lh, lr_, rtol=2e-2, atol=2e-2)
    assert torch.equal(hip.correct, corr) and ch.item() == cr.item()
    assert 0 < cr.item() < B and cr.item() == B // 2 - 1  # the odd boards but the mass-less board 1
    odd = torch.arange(B, device=cuda_device) % 2 == 1
    odd[1] = False
    # the loss sees the targets: with log p about -0.2 on the stone and -6.2 elsewhere, an odd board (at
    # least 20/64 of its mass on the stone) stays below 4.4, an even one (at most 9/56 there) above 5.2
    assert per[odd].max().item() + 0.5 < per[~odd & (per > 0)].min().item()
    assert hip.loss[1].item() == 0.0 and hip.correct[1].item() == 0.0
    assert torch.equal(hip.fp.flat, before)  # no update


def test_hip_soft_step_is_deterministic(cuda_device):
    """Two trainers from the same weights, the same soft batch: bitwise equal gradients, metrics and
    updated weights."""
    B = 264
    net, planes, dist, sym, _ = _setup(cuda_device, B, seed=2)
    outs = []
    for _ in range(2):
        tr = HipPolicyTrainer(copy.deepcopy(net), B, lr=0.01, device=cuda_device)
        l, c = tr.step(planes, dist, sym)
        torch.cuda.synchronize()
        outs.append((tr.fp.grad.clone(), tr.fp.flat.clone(), l.clone(), c.clone(), tr.loss.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_hip_soft_targets_refused_where_unsupported(cuda_device):
    """Graph mode, the reference binary CE and the regularisers take one move per board."""
    B = 8
    net, planes, dist, sym, _ = _setup(cuda_device, B, seed=3)
    tr = HipPolicyTrainer(net, B, lr=0.01, device=cuda_device)
    for attr, val in (("policy_loss", "bce"), ("ent_coef", 0.1), ("kl_coef", 0.1), ("collect_stats", True),
                      ("collect_probs", True)):
        setattr(tr, attr, val)
        with pytest.raises(ValueError, match="soft"):
            tr.compute_grads(planes, dist, sym)
        delattr(tr, attr)  # back to the class default
    with pytest.raises(ValueError, match="soft targets must be"):
        tr.compute_grads(planes, dist[:, :SS - 1].contiguous(), sym)
    tr.enable_graphs()
    with pytest.raises(RuntimeError, match="graph mode"):
        tr.step(planes, dist, sym)
    assert tr._g_in is None  # refused before the graph path allocated anything
    tr.enable_graphs(False)
    tr.step(planes, dist, sym)  # the eager step still runs
    torch.cuda.synchronize()


def test_train_sl_targets_pi_hip_backend(tmp_path, cuda_device):
    """train-sl --targets pi end to end on the HIP backend: resident dataset, random symmetries, the
    validation shard's short last batch padded with all-zero rows (no loss in the kernel)."""
    import numpy as np

    from alphago_amd.features import DEFAULT_FEATURES
    from alphago_amd.io.h5lite import H5Writer
    from alphago_amd.models.policy import CNNPolicy
    from alphago_amd.train.sl import run_training

    rng = np.random.default_rng(0)
    n = 44
    pi = rng.random((n, SS)).astype(np.float32) ** 8
    pi /= pi.sum(1, keepdims=True)
    idx = pi.argmax(1)
    data = str(tmp_path / "dist.h5")
    with H5Writer(data) as w:
        w.attrs["features"] = np.array([x.encode() for x in DEFAULT_FEATURES])
        w.attrs["board_size"] = np.int64(S)
        w.create_dataset("states", data=rng.integers(0, 2, (n, C, S, S), dtype=np.uint8))
        w.create_dataset("actions", data=np.stack([idx // S, idx % S], 1).astype(np.uint8))
        w.create_dataset("pi", data=pi)
    model = str(tmp_path / "model.json")
    CNNPolicy(list(DEFAULT_FEATURES), board=S, filters_per_layer=F, layers=L, device="cuda").save_model(model)
    out = str(tmp_path / "out")
    meta = run_training([model, data, out, "--epochs", "2", "-B", "8", "--backend", "hip", "-r", "0.05",
                         "--targets", "pi", "--train-val-test", "0.75", "0.25", "0.0"])
    ep = meta["epochs"]
    assert meta["targets"] == "pi" and len(ep) == 2
    for e in ep:  # 11 validation rows: one batch of 8 and one of 3 + 5 padding rows
        assert all(np.isfinite(e[k]) for k in ("loss", "val_loss")) and 0 <= e["acc"] <= 1 and 0 <= e["val_acc"] <= 1
    # the cross-entropy against a distribution is bounded below by its entropy and starts near log(S*S)
    ent = float(-(pi * np.log(pi.clip(1e-30))).sum(1).min())
    assert ent <= ep[0]["val_loss"] < np.log(SS) + 1.0


def test_hip_soft_rows_gather_equals_gathered_batch(cuda_device):
    """``rows`` gathers the planes from a resident pool inside the input pack; the soft targets stay
    per board.  Bitwise the gradients and metrics of the batch gathered beforehand."""
    B = 8
    net, pool, dist, sym, _ = _setup(cuda_device, 3 * B, seed=4)
    rows = torch.randperm(3 * B, generator=torch.Generator().manual_seed(4))[:B].to(cuda_device)
    dist, sym = dist[:B].contiguous(), sym[:B].contiguous()
    tr = HipPolicyTrainer(net, B, lr=0.01, device=cuda_device)
    tr.compute_grads(pool, dist, sym, rows=rows)
    torch.cuda.synchronize()
    g, l, c = tr.fp.grad.clone(), tr.loss.clone(), tr.correct.clone()
    tr.compute_grads(pool.index_select(0, rows), dist, sym)
    torch.cuda.synchronize()
    assert torch.equal(g.view(torch.int32), tr.fp.grad.view(torch.int32))
    assert torch.equal(l.view(torch.int32), tr.loss.view(torch.int32)) and torch.equal(c, tr.correct)
    assert l[0].item() > 0
