"""Regularised fused policy head (entropy bonus, KL anchor, per-board diagnostics) vs fp32 torch
autograd on  L_b = -w_b log p_t - beta H(p) + kappa KL(q || p)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

# (C, B, S): BoardRegs-1024; BoardRows-512; the 1024 fallback at large B; boards smaller than the tiles
SHAPES = [(192, 7, 19), (192, 300, 19), (256, 300, 19), (64, 300, 9), (192, 7, 9)]
WSCALES = [0.05, 0.5]  # near-uniform and peaked softmax
COEFS = [(0.3, 0.0), (0.0, 0.7), (0.3, 0.7)]


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


def _bf(x):
    return x.to(torch.bfloat16).float()


def _rel_err(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


_CASES = {}


def _case(dev, C, B, S, ws):
    """Inputs of one shape and their fp32 oracle stats, built once and shared (never modified)."""
    key = (C, B, S, ws)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator(device="cpu").manual_seed(1000 * C + 10 * B + S + int(ws * 100))
    SS = S * S
    y = _bf(torch.randn(B, C, S, S, generator=g)).clamp_min(0).to(dev)
    w = (torch.randn(C, generator=g) * ws).to(dev)
    b = torch.randn(1, generator=g).to(dev)
    tgt = torch.randint(0, SS, (B,), generator=g, dtype=torch.int32)
    tgt[2] = -1  # no target
    wt = torch.tensor([1.0, -1.0, 2.0, -0.5, 1.0, 3.0]).repeat((B + 5) // 6)[:B].contiguous()
    q = torch.softmax(torch.randn(B, SS, generator=g), 1)
    q[1, torch.randperm(SS, generator=g)[:SS // 10]] = 0.0  # a tenth of board 1 exactly 0
    q[1] /= q[1].sum()
    c = dict(C=C, B=B, S=S, y=y, w=w, b=b, tgt=tgt.to(dev), wt=wt.to(dev), q=q.to(dev).contiguous())
    _CASES[key] = c
    return c


def _logits(c, y, w, b):
    return (y * w.view(1, c["C"], 1, 1)).sum(1).flatten(1) + b


def _stats_ref(logits, q, legal=None):
    """(B, 3) entropy, KL(q || p), max |finite logit| (fp32 torch)."""
    if legal is not None:
        logits = logits.masked_fill(legal == 0, float("-inf"))
    logp = torch.log_softmax(logits, 1)
    p = logp.exp()
    fin = torch.isfinite(logits)
    ent = -torch.where(fin, p * logp, torch.zeros_like(p)).sum(1)
    kl = torch.where(q > 0, torch.xlogy(q, q) - q * logp, torch.zeros_like(q)).sum(1)
    mx = torch.where(fin, logits.abs(), torch.zeros_like(logits)).amax(1)
    return torch.stack([ent, kl, mx], 1)


def _oracle_grads(c, beta, kappa):
    yr = c["y"].clone().requires_grad_(True)
    wr = c["w"].clone().requires_grad_(True)
    br = c["b"].clone().requires_grad_(True)
    logits = _logits(c, yr, wr, br)
    logp = torch.log_softmax(logits, 1)
    p = logp.exp()
    valid = (c["tgt"] >= 0).float()
    lt = logp.gather(1, c["tgt"].long().clamp_min(0).unsqueeze(1)).squeeze(1)
    ent = -(p * logp).sum(1)
    q = c["q"]
    kl = (torch.xlogy(q, q) - q * logp).sum(1)
    obj = ((-c["wt"] * lt - beta * ent + kappa * kl) * valid).sum() / c["B"]
    obj.backward()
    return yr.grad * (c["y"] > 0), wr.grad, br.grad


def _run(ops, c, **kw):
    B, C, S = c["B"], c["C"], c["S"]
    dev = c["y"].device
    out = dict(dz=ops.padded_empty(B, S, 1, C, dev), loss=torch.empty(B, device=dev),
               corr=torch.empty(B, device=dev), dh=torch.empty(B, C + 1, device=dev))
    ops.policy_head_train(ops.to_padded(c["y"], 1, C), c["w"], c["b"], c["tgt"], out["dz"], out["loss"], out["corr"],
                          out["dh"], S, 1.0 / B, weight=c["wt"], **kw)
    torch.cuda.synchronize()
    return out


def _close(a, b):  # loss-like scalars (test_policy_head_train's bound)
    return torch.allclose(a, b, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("ws", WSCALES)
@pytest.mark.parametrize("C,B,S", SHAPES)
def test_stats(ops, cuda_device, C, B, S, ws):
    c = _case(cuda_device, C, B, S, ws)
    logits = _logits(c, c["y"], c["w"], c["b"])
    ref = _stats_ref(logits, c["q"])
    st = torch.full((B, 3), float("nan"), device=cuda_device)
    _run(ops, c, ref_probs=c["q"], stats=st)
    for col in range(3):  # every board, the target-less one included
        assert _close(st[:, col], ref[:, col]), (col, (st[:, col] - ref[:, col]).abs().max().item())
    # reference loss (binary CE): stats only, the same numbers
    st_bce = torch.full((B, 3), float("nan"), device=cuda_device)
    _run(ops, c, ref_probs=c["q"], stats=st_bce, bce=True)
    assert torch.equal(st_bce, st)
    # no anchor: the KL column is 0
    st0 = torch.full((B, 3), float("nan"), device=cuda_device)
    _run(ops, c, stats=st0)
    assert torch.equal(st0[:, 1], torch.zeros(B, device=cuda_device))
    assert torch.equal(st0[:, 0], st[:, 0]) and torch.equal(st0[:, 2], st[:, 2])
    # inference form under a legal mask whose zeros fall only where q == 0
    legal = torch.ones(B, S * S, dtype=torch.uint8, device=cuda_device)
    legal[1] = (c["q"][1] > 0).to(torch.uint8)
    refm = _stats_ref(logits, c["q"], legal)
    sti = torch.full((B, 3), float("nan"), device=cuda_device)
    probs = torch.empty(B, S * S, device=cuda_device)
    ops.policy_head_probs(ops.to_padded(c["y"], 1, C), c["w"], c["b"], probs, S, legal=legal, ref_probs=c["q"],
                          stats=sti)
    torch.cuda.synchronize()
    for col in range(3):
        assert _close(sti[:, col], refm[:, col]), (col, (sti[:, col] - refm[:, col]).abs().max().item())
    pm = torch.softmax(logits.masked_fill(legal == 0, float("-inf")), 1)
    assert torch.allclose(probs, pm, atol=1e-5)


@pytest.mark.parametrize("beta,kappa", COEFS)
@pytest.mark.parametrize("ws", WSCALES)
@pytest.mark.parametrize("C,B,S", SHAPES)
def test_gradients(ops, cuda_device, C, B, S, ws, beta, kappa):
    c = _case(cuda_device, C, B, S, ws)
    dzr, dwr, dbr = _oracle_grads(c, beta, kappa)
    plain = _run(ops, c)
    got = _run(ops, c, ref_probs=c["q"], ent_coef=beta, kl_coef=kappa)
    dz = ops.from_padded(got["dz"], 1)
    e_dz, e_dh = _rel_err(dz, dzr), _rel_err(got["dh"][:, :C].sum(0), dwr)
    e_db = abs(got["dh"][:, C].sum().item() - dbr.item())
    print("dz %.3g dhead %.3g dbias %.3g" % (e_dz, e_dh, e_db))
    assert e_dz < 1e-2
    assert e_dh < 1e-3
    assert e_db < 1e-4
    # the target-less board gets no gradient at all, regularisers included
    assert not dz[2].any() and not got["dh"][2].any()
    # loss and correct keep their meaning: the clipped CE and top-1
    assert torch.equal(got["loss"], plain["loss"]) and torch.equal(got["corr"], plain["corr"])


@pytest.mark.parametrize("ws", WSCALES)
@pytest.mark.parametrize("C,B,S", SHAPES)
def test_off_means_off(ops, cuda_device, C, B, S, ws):
    """stats and ref_probs with zero coefficients: the regularised kernel, the plain kernel's bits."""
    c = _case(cuda_device, C, B, S, ws)
    plain = _run(ops, c)
    st = torch.empty(B, 3, device=cuda_device)
    probs = torch.empty(B, S * S, device=cuda_device)
    got = _run(ops, c, ref_probs=c["q"], stats=st, ent_coef=0.0, kl_coef=0.0, probs=probs)
    for k in ("dz", "dh", "loss", "corr"):
        assert torch.equal(got[k], plain[k]), k
    ref = torch.softmax(_logits(c, c["y"], c["w"], c["b"]), 1)
    assert torch.allclose(probs, ref, atol=1e-5)


@pytest.mark.parametrize("B", [6, 264])  # 1024-thread and 512-thread (row-mapped) head kernels
def test_trainer_parity(cuda_device, B):
    from alphago_amd.models.nets import PolicyNet
    from alphago_amd.train.engine import HipPolicyTrainer, TorchPolicyTrainer

    torch.manual_seed(5)
    C = 48
    net = PolicyNet(C, filters_per_layer=64, layers=3)
    net_ref = copy.deepcopy(net)
    planes = torch.randint(0, 2, (B, C, 19, 19), dtype=torch.uint8, device=cuda_device)
    tgt = torch.randint(0, 361, (B,), dtype=torch.int32, device=cuda_device)
    tgt[-1] = -1  # padding board: no loss, no gradient
    wt = torch.tensor([1.0, -1.0, 2.0, -0.5, 1.0, 3.0], device=cuda_device).repeat((B + 5) // 6)[:B].contiguous()
    q = torch.softmax(torch.randn(B, 361, device=cuda_device), 1).contiguous()
    hip = HipPolicyTrainer(net, B, lr=0.01, device=cuda_device)
    ref = TorchPolicyTrainer(net_ref, B, lr=0.01, device=cuda_device)
    for t in (hip, ref):
        t.ent_coef, t.kl_coef, t.ref_probs = 0.3, 0.7, q
        t.collect_stats = t.collect_probs = True
    hip.compute_grads(planes, tgt, None, wt)
    ref.compute_grads(planes, tgt, None, wt)
    torch.cuda.synchronize()
    for name in hip.fp.names:
        a, b = hip.fp.grad_views[name], ref.fp.grad_views[name]
        if name == "head_b":  # every term of the objective is invariant to a shift of the logits
            assert abs(a.item()) < 1e-5 and abs(b.item()) < 1e-5
            continue
        cos = torch.nn.functional.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()
        ratio = a.norm().item() / max(b.norm().item(), 1e-12)
        assert cos > 0.98 and abs(ratio - 1) < 0.05, (name, cos, ratio)
    assert torch.allclose(hip.loss, ref._last[0], rtol=2e-2, atol=1e-4)
    # bf16 trunk against the fp32 one: the bookkeeping bound of the loss above
    assert torch.allclose(hip.head_stats, ref.head_stats, rtol=2e-2, atol=2e-2)
    assert torch.allclose(hip.head_probs, ref.head_probs, rtol=2e-2, atol=1e-4)
    g0, it0 = hip.fp.grad.clone(), hip.sched.iterations
    sa, sb = hip.policy_stats(planes, q), ref.policy_stats(planes, q)
    assert sa.shape == (B, 3) and torch.allclose(sa, sb, rtol=2e-2, atol=2e-2)
    assert torch.equal(sa, hip.head_stats)  # the same weights and boards: the same numbers
    assert torch.equal(hip.fp.grad, g0) and hip.sched.iterations == it0
    assert torch.equal(hip.policy_stats(planes)[:, 1], torch.zeros(B, device=cuda_device))


def test_host_checks(ops, cuda_device):
    c = _case(cuda_device, 192, 7, 19, 0.05)
    with pytest.raises(RuntimeError, match=">= 0"):
        _run(ops, c, ent_coef=-0.1)
    with pytest.raises(RuntimeError, match=">= 0"):
        _run(ops, c, ref_probs=c["q"], kl_coef=-0.1)
    with pytest.raises(RuntimeError, match="ref_probs"):
        _run(ops, c, kl_coef=0.5)
    with pytest.raises(RuntimeError, match="loss_kind"):
        _run(ops, c, ent_coef=0.1, bce=True)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        _run(ops, c, ref_probs=c["q"].cpu(), kl_coef=0.5)
    with pytest.raises(RuntimeError, match="stats"):
        _run(ops, c, stats=torch.empty(c["B"], 2, device=cuda_device))
    with pytest.raises(RuntimeError, match="ref_probs"):
        _run(ops, c, ref_probs=c["q"][:, :-1].contiguous())
    with pytest.raises(RuntimeError):  # coefficients without a target
        torch.ops.alphago_amd.policy_head(ops.to_padded(c["y"], 1, 192), c["w"], c["b"], None, None, None, None,
                                          None, None, None, None, 19, 0.0, 1.0, 0, None, None, 0.1, 0.0)
