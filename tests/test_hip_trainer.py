"""Full HIP SL step vs the autograd fp32 step (same init, same batch/symmetries)."""
import copy

import pytest
import torch

from alphago_amd.models.nets import PolicyNet
from alphago_amd.train.engine import HipPolicyTrainer, TorchPolicyTrainer

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("F,L,C,B", [(64, 3, 48, 6), (192, 4, 48, 5), (128, 2, 12, 3)])
def test_hip_grads_match_torch(cuda_device, F, L, C, B):
    torch.manual_seed(0)
    net = PolicyNet(C, filters_per_layer=F, layers=L)
    net_ref = copy.deepcopy(net)
    planes = torch.randint(0, 2, (B, C, 19, 19), dtype=torch.uint8, device=cuda_device)
    tgt = torch.randint(0, 361, (B,), dtype=torch.int32, device=cuda_device)
    sym = torch.randint(0, 8, (B,), dtype=torch.int32, device=cuda_device)
    hip = HipPolicyTrainer(net, B, lr=0.01, device=cuda_device)
    ref = TorchPolicyTrainer(net_ref, B, lr=0.01, device=cuda_device)
    hip.compute_grads(planes, tgt, sym)
    ref.compute_grads(planes, tgt, sym)
    torch.cuda.synchronize()
    for name in hip.fp.names:
        a, b = hip.fp.grad_views[name], ref.fp.grad_views[name]
        if name == "head_b":  # d(mean CE)/d(scalar logit bias) == 0 exactly (softmax shift invariance)
            assert abs(a.item()) < 1e-5 and abs(b.item()) < 1e-5
            continue
        # bf16 activations/weights through a chain of dgrad layers: compare
        # direction and magnitude (per-kernel 1e-2 checks are in test_hip_kernels)
        cos = torch.nn.functional.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()
        ratio = a.norm().item() / max(b.norm().item(), 1e-12)
        assert cos > 0.98 and abs(ratio - 1) < 0.05, (name, cos, ratio)
    # loss / accuracy bookkeeping
    assert torch.allclose(hip.loss, ref._last[0], rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("B", [6, 264])  # 1024-thread and 512-thread (row-mapped) head kernels
def test_hip_bce_grads_match_torch(cuda_device, B):
    """Reference RL loss (binary CE on the softmax, per-board signed weights) on
    the fused HIP head (loss_kind=1) vs autograd."""
    torch.manual_seed(5)
    C = 48
    net = PolicyNet(C, filters_per_layer=64, layers=3)
    net_ref = copy.deepcopy(net)
    planes = torch.randint(0, 2, (B, C, 19, 19), dtype=torch.uint8, device=cuda_device)
    tgt = torch.randint(0, 361, (B,), dtype=torch.int32, device=cuda_device)
    tgt[-1] = -1  # padding board: no loss, no gradient
    wt = torch.tensor([1.0, -1.0, 2.0, -0.5, 1.0, 3.0], device=cuda_device).repeat((B + 5) // 6)[:B].contiguous()
    hip = HipPolicyTrainer(net, B, lr=0.01, device=cuda_device)
    ref = TorchPolicyTrainer(net_ref, B, lr=0.01, device=cuda_device)
    hip.policy_loss = ref.policy_loss = "bce"
    hip.compute_grads(planes, tgt, None, wt)
    ref.compute_grads(planes, tgt, None, wt)
    torch.cuda.synchronize()
    for name in hip.fp.names:
        a, b = hip.fp.grad_views[name], ref.fp.grad_views[name]
        if name == "head_b":
            assert abs(a.item()) < 1e-6 and abs(b.item()) < 1e-6
            continue
        cos = torch.nn.functional.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()
        ratio = a.norm().item() / max(b.norm().item(), 1e-12)
        assert cos > 0.98 and abs(ratio - 1) < 0.05, (name, cos, ratio)
    assert torch.allclose(hip.loss, ref._last[0], rtol=2e-2, atol=1e-4)
    assert hip.loss[-1].item() == 0.0


def test_step_rows_equals_gathered_batch(cuda_device):
    """step(pool, targets, sym, rows=idx) gathers inside the pack kernel: bitwise the same losses and
    weights as step(pool[idx], ...), for the policy and the value trainer (which also takes its
    head-gradient column sums and step metrics from head_grad_sums)."""
    from alphago_amd.models.nets import ValueNet
    from alphago_amd.train.engine import HipValueTrainer

    torch.manual_seed(4)
    B, C, npool = 8, 48, 40
    pool = torch.randint(0, 2, (npool, C, 19, 19), dtype=torch.uint8, device=cuda_device)
    ptgt = torch.randint(0, 361, (npool,), dtype=torch.int32, device=cuda_device)
    net = PolicyNet(C, filters_per_layer=64, layers=3)
    a = HipPolicyTrainer(copy.deepcopy(net), B, lr=0.01, device=cuda_device)
    b = HipPolicyTrainer(copy.deepcopy(net), B, lr=0.01, device=cuda_device)
    vnet = ValueNet(C + 1, filters_per_layer=64, layers=3)
    vpool = torch.randint(0, 2, (npool, C + 1, 19, 19), dtype=torch.uint8, device=cuda_device)
    pz = (torch.randint(0, 2, (npool,), device=cuda_device) * 2 - 1).float()
    va = HipValueTrainer(copy.deepcopy(vnet), B, lr=0.01, device=cuda_device)
    vb = HipValueTrainer(copy.deepcopy(vnet), B, lr=0.01, device=cuda_device)
    for _ in range(3):
        idx = torch.randint(0, npool, (B,), device=cuda_device)
        sym = torch.randint(0, 8, (B,), dtype=torch.int32, device=cuda_device)
        la = a.step(pool, ptgt.index_select(0, idx), sym, rows=idx)
        lb = b.step(pool.index_select(0, idx), ptgt.index_select(0, idx), sym)
        assert all(torch.equal(x, y) for x, y in zip(la, lb))
        lva = va.step(vpool, pz.index_select(0, idx), sym, rows=idx)
        lvb = vb.step(vpool.index_select(0, idx), pz.index_select(0, idx), sym)
        assert all(torch.equal(x, y) for x, y in zip(lva, lvb))
        # the value metrics are the per-board sums (head_grad_sums' fixed order)
        torch.testing.assert_close(lva[0], va.loss.sum(), rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(lva[1], va.correct.sum())
    assert torch.equal(a.fp.flat, b.fp.flat) and torch.equal(va.fp.flat, vb.fp.flat)
    with pytest.raises(ValueError):
        a.step(pool, ptgt[:B], None, rows=torch.zeros(B + 1, dtype=torch.long, device=cuda_device))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_hip_step_reduces_loss(cuda_device, seed):
    # lr 0.05: at 0.5 this 20-step fit of one batch is chaotic, and a last-bit change in the
    # head's reductions flipped its outcome (loss 188.5 -> 515.8 instead of down)
    torch.manual_seed(seed)
    B = 32
    net = PolicyNet(48, filters_per_layer=64, layers=3)
    tr = HipPolicyTrainer(net, B, lr=0.05, device=cuda_device)
    planes = torch.randint(0, 2, (B, 48, 19, 19), dtype=torch.uint8, device=cuda_device)
    tgt = torch.randint(0, 361, (B,), dtype=torch.int32, device=cuda_device)
    l0, _ = tr.evaluate(planes, tgt)
    l0 = l0.item()
    for _ in range(20):
        tr.step(planes, tgt)
    l1, _ = tr.evaluate(planes, tgt)
    assert l1.item() < l0
    # module parameters are views of the trained flat buffer
    assert torch.equal(net.head_w.detach().view(-1), tr.fp.views["head_w"].view(-1))


class _RoundFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).float()

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).float()


def test_hip_grads_match_bf16_emulation(cuda_device):
    """Same comparison against an fp32 reference that rounds exactly where the
    HIP path stores bf16 (weights, activations, pre-activation gradients): any
    real indexing/orientation bug shows up far above this tolerance."""
    import torch.nn.functional as F
    torch.manual_seed(0)
    B, C, Fn, L = 5, 48, 192, 4
    net = PolicyNet(C, filters_per_layer=Fn, layers=L)
    ws = [w.detach().clone().to(cuda_device) for w in net.trunk.weights]
    bs = [b.detach().clone().to(cuda_device) for b in net.trunk.biases]
    hw, hb = net.head_w.detach().clone().to(cuda_device), net.head_b.detach().clone().to(cuda_device)
    planes = torch.randint(0, 2, (B, C, 19, 19), dtype=torch.uint8, device=cuda_device)
    tgt = torch.randint(0, 361, (B,), dtype=torch.int32, device=cuda_device)
    hip = HipPolicyTrainer(net, B, lr=0.01, device=cuda_device)
    hip.compute_grads(planes, tgt, None)
    params = [p.requires_grad_(True) for p in ws + bs + [hw, hb]]
    x = planes.float()
    for l in range(L):
        z = F.conv2d(x, ws[l].to(torch.bfloat16).float(), bs[l], padding=net.trunk.widths[l] // 2)
        z = _RoundGrad.apply(z)
        x = _RoundFwd.apply(F.relu(z))
    logits = (x * hw.view(1, Fn, 1, 1)).sum(1).flatten(1) + hb
    loss = F.cross_entropy(logits, tgt.long(), reduction="sum") / B
    loss.backward()
    for l in range(L):
        for name, ref in (("w%d" % l, ws[l].grad), ("b%d" % l, bs[l].grad)):
            a = hip.fp.grad_views[name]
            cos = torch.nn.functional.cosine_similarity(a.flatten().double(), ref.flatten().double(), dim=0).item()
            assert cos > 0.999, (name, cos)


@pytest.mark.parametrize("F", [64, 152])
def test_hip_value_grads_match_torch(cuda_device, F):
    """HIP value trunk + head (head_logits -> dense -> value_out -> head_backward)
    vs autograd; F = 152 is the reference width, run on 160-wide tiles."""
    from alphago_amd.models.nets import ValueNet
    from alphago_amd.train.engine import HipValueTrainer, TorchValueTrainer

    torch.manual_seed(0)
    B, C = 6, 49
    net = ValueNet(C, filters_per_layer=F, layers=3)
    net_ref = copy.deepcopy(net)
    planes = torch.randint(0, 2, (B, C, 19, 19), dtype=torch.uint8, device=cuda_device)
    z = (torch.randint(0, 2, (B,), device=cuda_device) * 2 - 1).float()
    hip = HipValueTrainer(net, B, lr=0.01, device=cuda_device)
    assert hip.Fp == (160 if F == 152 else F)
    ref = TorchValueTrainer(net_ref, B, lr=0.01, device=cuda_device)
    hip.compute_grads(planes, z, None)
    ref.compute_grads(planes, z, None)
    torch.cuda.synchronize()
    for name in hip.fp.names:
        a, b = hip.fp.grad_views[name], ref.fp.grad_views[name]
        cos = torch.nn.functional.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()
        ratio = a.norm().item() / max(b.norm().item(), 1e-12)
        assert cos > 0.98 and abs(ratio - 1) < 0.05, (name, cos, ratio)
    v_hip = hip.predict(planes)
    v_ref = net_ref.forward_torch(planes.float())
    torch.testing.assert_close(v_hip, v_ref.float(), atol=2e-2, rtol=2e-2)


def test_value_out_kernel(cuda_device):
    from alphago_amd import ops

    torch.manual_seed(3)
    B, D = 7, 256
    h = torch.randn(B, D, device=cuda_device)
    w2 = torch.randn(D, device=cuda_device) * 0.05
    b2 = torch.randn(1, device=cuda_device) * 0.1
    t = torch.tensor([1., -1., 1., -1., 1., 1., -1.], device=cuda_device)
    wt = torch.rand(B, device=cuda_device)
    v, loss, corr = (torch.zeros(B, device=cuda_device) for _ in range(3))
    dh = torch.zeros(B, D, device=cuda_device)
    dout = torch.zeros(B, D + 1, device=cuda_device)
    ops.value_out(h, w2, b2, v, target=t, weight=wt, loss=loss, correct=corr, dh=dh, dout=dout, grad_scale=0.5)
    hr, w2r, b2r = h.clone().requires_grad_(), w2.clone().requires_grad_(), b2.clone().requires_grad_()
    vr = torch.tanh(hr @ w2r + b2r)
    ((vr - t) ** 2 * wt).sum().mul(0.5).backward()
    torch.testing.assert_close(v, vr.detach(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(loss, ((vr - t) ** 2).detach(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(corr, (torch.sign(vr) == torch.sign(t)).float())
    torch.testing.assert_close(dh, hr.grad, atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(dout[:, :D].sum(0), w2r.grad, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(dout[:, D].sum(0, keepdim=True), b2r.grad, atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("S", [9, 13])
@pytest.mark.parametrize("F,L", [(64, 3), (192, 4)])
def test_hip_trunk_small_boards_match_torch(cuda_device, S, F, L):
    """The HIP trunk (implicit-GEMM fwd, bitmask dgrad, split-K wgrad, fused head)
    at board sizes 9 and 13 (reference tests/test_policy.py:23-30 checks a 13x13
    policy) vs the fp32 autograd trainer: loss, gradients and the updated weights."""
    torch.manual_seed(S)
    B, C = 7, 48
    net = PolicyNet(C, board=S, filters_per_layer=F, layers=L)
    net_ref = copy.deepcopy(net)
    planes = torch.randint(0, 2, (B, C, S, S), dtype=torch.uint8, device=cuda_device)
    tgt = torch.randint(0, S * S, (B,), dtype=torch.int32, device=cuda_device)
    sym = torch.randint(0, 8, (B,), dtype=torch.int32, device=cuda_device)
    hip = HipPolicyTrainer(net, B, lr=0.05, device=cuda_device)
    ref = TorchPolicyTrainer(net_ref, B, lr=0.05, device=cuda_device)
    hip.compute_grads(planes, tgt, sym)
    ref.compute_grads(planes, tgt, sym)
    torch.cuda.synchronize()
    assert torch.allclose(hip.loss, ref._last[0], rtol=2e-2, atol=2e-2)
    for name in hip.fp.names:
        if name == "head_b":
            continue
        a, b = hip.fp.grad_views[name], ref.fp.grad_views[name]
        cos = torch.nn.functional.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()
        ratio = a.norm().item() / max(b.norm().item(), 1e-12)
        assert cos > 0.98 and abs(ratio - 1) < 0.05, (S, name, cos, ratio)
    hip.apply_update()
    ref.apply_update()
    torch.cuda.synchronize()
    d = (hip.fp.flat - ref.fp.flat).abs().max().item()
    assert d < 5e-3, d
    # inference through the same trunk kernels: probabilities over S*S points
    from alphago_amd.models.inference import HipTrunkInference
    probs = HipTrunkInference(net, cuda_device, buckets=(B,)).evaluate(planes.cpu().numpy())
    assert probs.shape == (B, S * S)
    assert torch.allclose(probs.float().sum(1), torch.ones(B, device=probs.device), atol=1e-3)


@pytest.mark.parametrize("kind,F,C,B", [("policy", 192, 48, 6), ("value", 152, 49, 5), ("policy", 64, 12, 3)])
def test_fused_sgd_pack_matches_separate_update(cuda_device, monkeypatch, kind, F, C, B):
    """The fused update (ops.sgd_pack: SGD + bf16 forward / transposed packs in one launch)
    leaves the same master weights and the same packed copies as sgd_update followed by pack_weights,
    eager and with the device schedule (graph-mode path)."""
    import copy

    from alphago_amd.models.nets import PolicyNet, ValueNet
    from alphago_amd.train.engine import HipPolicyTrainer, HipValueTrainer

    torch.manual_seed(3)
    net = PolicyNet(C, filters_per_layer=F, layers=3) if kind == "policy" else ValueNet(C, filters_per_layer=F, layers=3)
    cls = HipPolicyTrainer if kind == "policy" else HipValueTrainer
    trs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("ALPHAGO_AMD_FUSED_UPDATE", fused)
        trs.append(cls(copy.deepcopy(net), B, lr=0.05, decay=0.01, device=cuda_device))
    planes = torch.randint(0, 2, (B, C, 19, 19), dtype=torch.uint8, device=cuda_device)
    tgt = (torch.randint(0, 361, (B,), dtype=torch.int32, device=cuda_device) if kind == "policy"
           else torch.rand(B, device=cuda_device) * 2 - 1)
    for t in trs:
        t.step(planes, tgt)
        t.sync_schedule()
        t.compute_grads(planes, tgt)
        t.apply_update(device_schedule=True)
    torch.cuda.synchronize()
    a, b = trs
    assert a._fused_update and not b._fused_update
    assert torch.allclose(a.fp.flat, b.fp.flat, rtol=0, atol=1e-7)
    for l in range(3):
        assert torch.equal(a.wf[l], b.wf[l]), l
        assert torch.equal(a.wd[l], b.wd[l]), l
    assert torch.equal(a._sched_dev, b._sched_dev)


@pytest.mark.parametrize("B,kind", [(4, "policy"), (1, "policy"), (2, "value")])
def test_splitk_small_batch_trainer_matches(cuda_device, monkeypatch, B, kind):
    """Small batches run the forward and the bitmask dgrad on the split-K 32-pixel tile
    (ops.conv_fwd_splitk; the value net's 152 filters on the 160-wide tile with straddled K-steps);
    same loss and gradients as ALPHAGO_AMD_SPLITK=0 up to summation order."""
    import copy

    from alphago_amd.models.nets import PolicyNet, ValueNet
    from alphago_amd.train.engine import HipPolicyTrainer, HipValueTrainer

    torch.manual_seed(6)
    if kind == "policy":
        net, C, cls = PolicyNet(48, filters_per_layer=192, layers=4), 48, HipPolicyTrainer
    else:
        net, C, cls = ValueNet(49, filters_per_layer=152, layers=4), 49, HipValueTrainer
    trs = []
    monkeypatch.setenv("ALPHAGO_AMD_WS", "0")  # the weight-stationary tile would take these batches
    for sk in ("1", "0"):
        monkeypatch.setenv("ALPHAGO_AMD_SPLITK", sk)
        trs.append(cls(copy.deepcopy(net), B, lr=0.05, device=cuda_device))
    def split(plans):
        return [p.kind == "splitk" and p.nsplit > 1 for p in plans if p is not None]

    assert trs[0].dg_plan[0] is None and trs[1].dg_plan[0] is None
    assert any(split(trs[0].fwd_plan)) and any(split(trs[0].dg_plan))
    assert not any(split(trs[1].fwd_plan + trs[1].dg_plan))
    assert all(p.nsplit == 1 for p in trs[1].fwd_plan + trs[1].dg_plan[1:])
    planes = torch.randint(0, 2, (B, C, 19, 19), dtype=torch.uint8, device=cuda_device)
    if kind == "policy":
        tgt = torch.randint(0, 361, (B,), dtype=torch.int32, device=cuda_device)
    else:
        tgt = (torch.randint(0, 2, (B,), device=cuda_device) * 2 - 1).float()
    for t in trs:
        t.compute_grads(planes, tgt)
    torch.cuda.synchronize()
    a, b = trs
    assert abs(a.loss.sum().item() - b.loss.sum().item()) < 1e-2 * abs(b.loss.sum().item())
    for name in a.fp.names:
        ga, gb = a.fp.grad_views[name].double().flatten(), b.fp.grad_views[name].double().flatten()
        if gb.norm() < 1e-6 * b.fp.grad.norm():
            continue
        assert torch.nn.functional.cosine_similarity(ga, gb, dim=0) > 0.999, name


@pytest.mark.parametrize("optimizer,nesterov", [("momentum", False), ("momentum", True), ("adam", False)])
def test_fused_optimizer_matches_torch_update(cuda_device, optimizer, nesterov):
    """Momentum SGD and Adam in the fused update (pack.hip opt_update) vs the same Keras 1.0 update in
    torch fp32 ops (engine.optimizer_update_) over three steps -- two eager, one with the device
    schedule (graph-mode path: the 8-entry schedule computes Adam's bias correction) -- and the bf16
    packs equal a fresh pack of the updated master weights."""
    from alphago_amd import ops
    from alphago_amd.models.nets import ValueNet
    from alphago_amd.train.engine import HipValueTrainer, optimizer_update_

    torch.manual_seed(9)
    B, C = 5, 49
    net = ValueNet(C, filters_per_layer=152, layers=3)
    tr = HipValueTrainer(net, B, lr=0.01, decay=0.01, device=cuda_device, optimizer=optimizer, momentum=0.9,
                         nesterov=nesterov)
    assert len(tr.opt_state) == (2 if optimizer == "adam" else 1)
    p_ref = tr.fp.flat.clone()
    st_ref = [torch.zeros_like(p_ref) for _ in tr.opt_state]
    planes = torch.randint(0, 2, (B, C, 19, 19), dtype=torch.uint8, device=cuda_device)
    z = torch.rand(B, device=cuda_device) * 2 - 1
    for k in range(3):
        tr.compute_grads(planes, z)
        torch.cuda.synchronize()
        g = tr.fp.grad.clone()
        step = tr.sched.current()
        if k == 2:
            tr.sync_schedule()
        tr.apply_update(device_schedule=(k == 2))
        optimizer_update_(p_ref, g, st_ref, tr.sched, step)
        torch.cuda.synchronize()
        torch.testing.assert_close(tr.fp.flat, p_ref, rtol=1e-5, atol=1e-7)
        for a, b in zip(tr.opt_state, st_ref):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-9)
        tr.fp.flat.copy_(p_ref)  # keep the two paths on the same weights
    assert int(tr._sched_dev[2].item()) == tr.sched.iterations == 3
    wf = [torch.zeros_like(w) for w in tr.wf]
    wd = [torch.zeros_like(w) for w in tr.wd]
    tr.fp.flat.copy_(p_ref)
    ops.pack_weights([tr.fp.views["w%d" % l] for l in range(3)], wf, wd)
    tr.compute_grads(planes, z)
    tr.fp.grad.zero_()
    tr.opt_state[0].zero_()  # zero gradient and zero velocity / first moment: the master stays put
    tr.apply_update()
    torch.cuda.synchronize()
    for l in range(3):
        assert torch.equal(tr.wf[l], wf[l]) and torch.equal(tr.wd[l], wd[l]), l


@pytest.mark.parametrize("B,kind", [(1, "policy"), (8, "policy"), (2, "value"), (16, "value")])
def test_weight_stationary_trainer_matches(cuda_device, monkeypatch, B, kind):
    """Small batches run the forward and the bitmask dgrad on the weight-stationary tile (tile 40,
    conv_ws.hip): same loss and gradients as the 32-pixel tiles (ALPHAGO_AMD_WS=0, no split-K) up to
    summation order, and the weights after a step."""
    import copy

    from alphago_amd.models.nets import PolicyNet, ValueNet
    from alphago_amd.train.engine import HipPolicyTrainer, HipValueTrainer

    torch.manual_seed(8)
    if kind == "policy":
        net, C, cls = PolicyNet(48, filters_per_layer=192, layers=4), 48, HipPolicyTrainer
    else:
        net, C, cls = ValueNet(49, filters_per_layer=152, layers=4), 49, HipValueTrainer
    trs = []
    for ws in ("1", "0"):
        monkeypatch.setenv("ALPHAGO_AMD_WS", ws)
        monkeypatch.setenv("ALPHAGO_AMD_SPLITK", ws)
        trs.append(cls(copy.deepcopy(net), B, lr=0.05, device=cuda_device))
    assert all(p.kind == "ws" for p in trs[0].fwd_plan[1:] + trs[0].dg_plan[1:])
    assert not any(p.kind == "ws" for p in trs[1].fwd_plan + trs[1].dg_plan[1:])
    for t in trs:  # the weight-stationary copies exist exactly where the plan reads them
        assert [w is not None for w in t.wf_ws] == [p.kind == "ws" for p in t.fwd_plan]
        assert [w is not None for w in t.wd_ws] == [p is not None and p.kind == "ws" for p in t.dg_plan]
    planes = torch.randint(0, 2, (B, C, 19, 19), dtype=torch.uint8, device=cuda_device)
    if kind == "policy":
        tgt = torch.randint(0, 361, (B,), dtype=torch.int32, device=cuda_device)
    else:
        tgt = (torch.randint(0, 2, (B,), device=cuda_device) * 2 - 1).float()
    for t in trs:
        t.compute_grads(planes, tgt)
    torch.cuda.synchronize()
    a, b = trs
    assert abs(a.loss.sum().item() - b.loss.sum().item()) < 1e-2 * abs(b.loss.sum().item())
    for name in a.fp.names:
        ga, gb = a.fp.grad_views[name].double().flatten(), b.fp.grad_views[name].double().flatten()
        if gb.norm() < 1e-6 * b.fp.grad.norm():
            continue
        assert torch.nn.functional.cosine_similarity(ga, gb, dim=0) > 0.995, name
    for t in trs:
        t.apply_update()
    torch.cuda.synchronize()
    assert (a.fp.flat - b.fp.flat).abs().max().item() < 5e-3


@pytest.mark.parametrize("B,kind,overlap", [(16, "policy", False), (48, "policy", True), (24, "value", False),
                                            (3, "policy", False)])
def test_merged_reduce_bitwise_equal(cuda_device, B, kind, overlap):
    """merged_reduce: every layer's split slab kept and summed by ONE conv_wgrad_reduce_multi launch
    after the backward -- bitwise the gradients of a reduce launch per layer (same summation order),
    with the wgrads on the side stream too, and with the split-free layers (B <= 4) left as they are."""
    import copy

    from alphago_amd.models.nets import PolicyNet, ValueNet
    from alphago_amd.train.engine import HipPolicyTrainer, HipValueTrainer

    torch.manual_seed(9)
    if kind == "policy":
        net, C, cls = PolicyNet(48, filters_per_layer=192, layers=4), 48, HipPolicyTrainer
    else:
        net, C, cls = ValueNet(49, filters_per_layer=152, layers=4), 49, HipValueTrainer
    trs = [cls(copy.deepcopy(net), B, lr=0.05, device=cuda_device, overlap=overlap, merged_reduce=m)
           for m in (True, False)]
    assert trs[0].merged_reduce and not trs[1].merged_reduce
    planes = torch.randint(0, 2, (B, C, 19, 19), dtype=torch.uint8, device=cuda_device)
    if kind == "policy":
        tgt = torch.randint(0, 361, (B,), dtype=torch.int32, device=cuda_device)
    else:
        tgt = (torch.randint(0, 2, (B,), device=cuda_device) * 2 - 1).float()
    for _ in range(2):
        for t in trs:
            t.compute_grads(planes, tgt)
        torch.cuda.synchronize()
        assert torch.equal(trs[0].fp.grad, trs[1].fp.grad)
        for t in trs:
            t.apply_update()
    torch.cuda.synchronize()
    assert torch.equal(trs[0].fp.flat, trs[1].fp.flat)
