"""The dual (policy + value) HIP training step against its autograd twin and against the two
single-head HIP trainers on the split nets."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

S = 19


def _cos_ratio(a, b):
    cos = torch.nn.functional.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()
    return cos, a.norm().item() / max(b.norm().item(), 1e-12)


def _batch(device, B, C=49, seed=0):
    g = torch.Generator().manual_seed(seed)
    planes = torch.randint(0, 2, (B, C, S, S), dtype=torch.uint8, generator=g).to(device)
    moves = torch.randint(0, S * S, (B,), dtype=torch.int32, generator=g).to(device)
    z = (torch.randint(0, 2, (B,), generator=g) * 2 - 1).float().to(device)
    sym = torch.randint(0, 8, (B,), dtype=torch.int32, generator=g).to(device)
    pi = torch.rand(B, S * S + 1, generator=g) ** 8  # peaked like a visit distribution
    pi = pi / pi.sum(1, keepdim=True)
    pi[1] = 0
    pi[1, S * S] = 1.0  # all visits on the pass: no policy loss, the value head still learns
    return planes, moves, pi.to(device), z, sym


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("F,L,C,B", [(64, 3, 49, 6), (192, 3, 49, 5)])
def test_hip_pv_grads_match_torch(cuda_device, F, L, C, B, soft):
    """HipPolicyValueTrainer.compute_grads against TorchPolicyValueTrainer on a deep copy, with
    symmetries, hard targets and a soft (B, S*S + 1) target with one all-pass row: every named
    gradient segment within cosine 0.98 and 5 % in norm, both losses within rtol / atol 2e-2
    (test_hip_grads_match_torch / test_hip_value_grads_match_torch's tolerances).  The first layer
    (192 or 64 filters, 64-channel tile, 49 real planes, K = 5) is new to the trainers."""
    from alphago_amd.models.nets import PolicyValueNet
    from alphago_amd.train.engine import HipPolicyValueTrainer, TorchPolicyValueTrainer

    torch.manual_seed(0)
    net = PolicyValueNet(C, filters_per_layer=F, layers=L)
    net_ref = copy.deepcopy(net)
    planes, moves, pi, z, sym = _batch(cuda_device, B, C)
    tgt = (pi if soft else moves, z)
    hip = HipPolicyValueTrainer(net, B, lr=0.01, device=cuda_device)
    ref = TorchPolicyValueTrainer(net_ref, B, lr=0.01, device=cuda_device)
    assert not hip._top_e5m2_fusable()
    assert hip.fp.names[-8:] == ["head_w", "head_b", "vhead_w", "vhead_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"]
    hip.compute_grads(planes, tgt, sym)
    ref.compute_grads(planes, tgt, sym)
    torch.cuda.synchronize()
    for name in hip.fp.names:
        a, b = hip.fp.grad_views[name], ref.fp.grad_views[name]
        if name == "head_b":  # d(mean CE)/d(scalar logit bias) == 0 exactly (softmax shift invariance)
            assert abs(a.item()) < 1e-5 and abs(b.item()) < 1e-5
            continue
        cos, ratio = _cos_ratio(a, b)
        print(name, round(cos, 5), round(ratio, 4))
        assert cos > 0.98 and abs(ratio - 1) < 0.05, (name, cos, ratio)
    assert torch.allclose(hip.loss, ref._last[0], rtol=2e-2, atol=2e-2)
    assert torch.allclose(hip.vloss, ref._vlast[0], rtol=2e-2, atol=2e-2)
    if soft:
        assert hip.loss[1].item() == 0.0 and hip.vloss[1].item() > 0.0


@pytest.mark.parametrize("value_coef", [0.0, 1.0])
def test_trunk_grads_are_the_sum_of_the_two_heads(cuda_device, value_coef):
    """Hard targets: the dual trainer's trunk-layer gradients against a policy-only HipPolicyTrainer
    (value_coef 0) and against the sum of it and a value-only HipValueTrainer (value_coef 1) on the
    split nets: cosine > 0.999 per trunk tensor."""
    from alphago_amd.models.nets import he_uniform_
    from alphago_amd.models.policy import CNNPolicyValue
    from alphago_amd.train.engine import HipPolicyTrainer, HipPolicyValueTrainer, HipValueTrainer

    B, F, L = 6, 64, 3
    torch.manual_seed(1)
    pv = CNNPolicyValue(device=cuda_device, board=S, filters_per_layer=F, layers=L)
    he_uniform_(pv.model, generator=torch.Generator(device=cuda_device).manual_seed(1))
    pol, val = pv.split()
    planes, moves, _, z, sym = _batch(cuda_device, B, seed=3)
    dual = HipPolicyValueTrainer(pv.model, B, lr=0.01, device=cuda_device, value_coef=value_coef)
    tp = HipPolicyTrainer(pol.model, B, lr=0.01, device=cuda_device)
    tv = HipValueTrainer(val.model, B, lr=0.01, device=cuda_device)
    dual.compute_grads(planes, (moves, z), sym)
    tp.compute_grads(planes, moves, sym)
    tv.compute_grads(planes, z, sym)
    torch.cuda.synchronize()
    for l in range(L):
        for name in ("w%d" % l, "b%d" % l):
            want = tp.fp.grad_views[name] + value_coef * tv.fp.grad_views[name]
            cos, ratio = _cos_ratio(dual.fp.grad_views[name], want)
            print(name, round(cos, 6), round(ratio, 4))
            assert cos > 0.999, (name, cos, ratio)
    # the value head contributes: at value_coef 1 the sum differs from the policy part alone
    if value_coef:
        assert _cos_ratio(tv.fp.grad_views["w0"], tp.fp.grad_views["w0"])[0] < 0.99
    # the heads' own gradients are the single-head trainers'
    assert _cos_ratio(dual.fp.grad_views["head_w"], tp.fp.grad_views["head_w"])[0] > 0.999
    if value_coef:
        for n_dual, n_val in (("vhead_w", "head_w"), ("fc1_w", "fc1_w"), ("fc2_w", "fc2_w")):
            assert _cos_ratio(dual.fp.grad_views[n_dual], tv.fp.grad_views[n_val])[0] > 0.999
    else:
        assert float(dual.fp.grad_views["fc1_w"].abs().max()) == 0.0


def test_twenty_steps_reduce_both_losses(cuda_device):
    """A fixed batch, 20 SGD steps (fan-in init, lr 0.003: the settings at which the autograd twin
    takes the policy CE sum from 39.8 to 8.0 and the squared-error sum from 6.0 to 0.04)."""
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_
    from alphago_amd.train.engine import HipPolicyValueTrainer

    B = 6
    net = he_uniform_(PolicyValueNet(49, S, 64, 3), generator=torch.Generator().manual_seed(1))
    planes, moves, _, z, _ = _batch(cuda_device, B, seed=5)
    tr = HipPolicyValueTrainer(net, B, lr=0.003, device=cuda_device)
    hist = [[float(m) for m in tr.step(planes, (moves, z))] for _ in range(20)]
    print(hist[0], hist[-1])
    assert len(hist[0]) == 4
    assert hist[-1][0] < 0.8 * hist[0][0]
    assert hist[-1][2] < 0.8 * hist[0][2]


def test_refusals(cuda_device):
    """Graph mode and the regularised head options are refused; an e5m2 head output is never fused."""
    from alphago_amd.models.nets import PolicyValueNet
    from alphago_amd.train.engine import HipPolicyValueTrainer

    B = 2
    tr = HipPolicyValueTrainer(PolicyValueNet(49, S, 64, 2), B, lr=0.01, device=cuda_device)
    planes, moves, _, z, _ = _batch(cuda_device, B)
    with pytest.raises(RuntimeError, match="graph mode"):
        tr.enable_graphs()
    for attr in ("ent_coef", "kl_coef"):
        setattr(tr, attr, 0.1)
        with pytest.raises(ValueError, match="dual"):
            tr.step(planes, (moves, z))
        setattr(tr, attr, 0.0)
    tr.collect_stats = True
    with pytest.raises(ValueError, match="dual"):
        tr.compute_grads(planes, (moves, z))
    tr.collect_stats = False
    with pytest.raises(ValueError, match="pair"):
        tr.step(planes, moves)
    assert len(tr.step(planes, (moves, z))) == 4
