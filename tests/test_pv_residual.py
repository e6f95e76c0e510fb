"""A residual trunk through the HIP engines: the dual trainer's gradients against its autograd twin, the
Fixup identity, the inference engine on every plan kind (eager and captured), symmetry ensembling over a
residual trunk, and the fp8 refusals.  Tolerances are tests/test_pv_trainer.py's and
tests/test_pv_inference.py's own."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_pv_trainer import _batch, _cos_ratio

pytestmark = pytest.mark.gpu

S = 19


def _residual_net(Fl, L, seed=0, live_branches=True):
    """he_uniform_ (Fixup: block ends zero), then -- ``live_branches`` -- the block-end convs re-drawn at
    the block-first bound, so that the skip path and the branch both carry signal and gradient."""
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_

    g = torch.Generator().manual_seed(seed)
    net = he_uniform_(PolicyValueNet(49, S, Fl, L, residual=1), generator=g)
    if live_branches:
        bound = (6.0 / (Fl * 9)) ** 0.5 * ((L - 1) // 2) ** -0.5
        with torch.no_grad():
            for l in range(2, L, 2):
                net.trunk.weights[l].uniform_(-bound, bound, generator=g)
    return net


def _planes(n, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 49, S, S)) < 0.4).astype(np.uint8), (rng.random((n, S * S)) < 0.6).astype(np.uint8)


# ----------------------------------------------------------------------------- trainer
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("Fl,L,B,kinds", [(64, 5, 6, {"splitk"}), (192, 5, 5, {"ws"}), (192, 3, 20, {"tile"})])
def test_hip_pv_grads_match_torch(cuda_device, Fl, L, B, kinds, soft):
    """HipPolicyValueTrainer.compute_grads against TorchPolicyValueTrainer on a deep copy: every named
    gradient within cosine 0.98 and 5 % in norm, both losses within rtol / atol 2e-2.  B = 5 / 6: the
    small-batch kernels (split-K at 64 filters, weight-stationary at 192), two blocks; B = 20 (M = 7220, past the weight-stationary and split-K limits of a
    training step): the tile kernels, one block."""
    from alphago_amd.train.engine import HipPolicyValueTrainer, TorchPolicyValueTrainer

    net = _residual_net(Fl, L)
    net_ref = copy.deepcopy(net)
    planes, moves, pi, z, sym = _batch(cuda_device, B)
    tgt = (pi if soft else moves, z)
    hip = HipPolicyValueTrainer(net, B, lr=0.01, device=cuda_device)
    ref = TorchPolicyValueTrainer(net_ref, B, lr=0.01, device=cuda_device)
    assert hip.residual and {p.kind for p in hip.fwd_plan[1:]} == kinds == {p.kind for p in hip.dg_plan[1:]}
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
    # the skips matter: the same weights as a plain stack give another gradient for the stem
    plain = copy.deepcopy(net_ref)
    plain.trunk.residual = False
    other = TorchPolicyValueTrainer(plain, B, lr=0.01, device=cuda_device)
    other.compute_grads(planes, tgt, sym)
    assert _cos_ratio(other.fp.grad_views["w0"], ref.fp.grad_views["w0"])[0] < 0.98


def test_splitk_training_step(cuda_device, monkeypatch):
    """B = 2 with the weight-stationary kernel off: forward and dgrad of the blocks on the split-K tile."""
    from alphago_amd.train.engine import HipPolicyValueTrainer, TorchPolicyValueTrainer

    monkeypatch.setenv("ALPHAGO_AMD_WS", "0")
    B = 2
    net = _residual_net(192, 5, seed=2)
    net_ref = copy.deepcopy(net)
    planes, moves, pi, z, sym = _batch(cuda_device, B)
    hip = HipPolicyValueTrainer(net, B, lr=0.01, device=cuda_device)
    ref = TorchPolicyValueTrainer(net_ref, B, lr=0.01, device=cuda_device)
    assert {p.kind for p in hip.fwd_plan[1:]} == {"splitk"}
    hip.compute_grads(planes, (moves, z), sym)
    ref.compute_grads(planes, (moves, z), sym)
    torch.cuda.synchronize()
    for l in range(5):
        cos, ratio = _cos_ratio(hip.fp.grad_views["w%d" % l], ref.fp.grad_views["w%d" % l])
        assert cos > 0.98 and abs(ratio - 1) < 0.05, (l, cos, ratio)


# ----------------------------------------------------------------------------- Fixup identity
def test_fixup_identity_on_the_gpu(cuda_device):
    """Right after he_uniform_ every block is the identity: trainer.predict and the inference engine give
    what the stem plus the heads give (fp32 torch), within test_pv_inference's atol / rtol 2e-2."""
    from alphago_amd.models.inference import HipPolicyValueInference
    from alphago_amd.train.engine import HipPolicyValueTrainer

    B = 6
    net = _residual_net(64, 5, seed=1, live_branches=False).to(cuda_device)
    x, legal = _planes(B, seed=3)
    xt = torch.from_numpy(x).to(cuda_device)
    with torch.no_grad():
        tr = net.trunk
        stem = torch.relu(F.conv2d(xt.float(), tr.weights[0], tr.biases[0], padding=2))
        z, v_ref = net.heads_torch(stem)
        p_ref = torch.softmax(z, 1)
        assert torch.equal(tr.forward_torch(xt.float()), stem)
    eng = HipPolicyValueInference(net, cuda_device, buckets=(8,))
    probs, values = eng.evaluate(x)
    v_tr = HipPolicyValueTrainer(net, B, lr=0.01, device=cuda_device).predict(xt)
    torch.cuda.synchronize()
    assert float(v_ref.abs().max()) > 1e-3
    torch.testing.assert_close(values.contiguous(), v_ref, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(v_tr, v_ref, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(probs.contiguous(), p_ref, atol=2e-2, rtol=2e-2)
    # the last block's output (layer 4) is its input (layer 2's output) bit for bit: bf16(relu(0 + 0 + Y2)) == Y2
    bk = eng._b[(8, 0)]
    assert torch.equal(bk.Y[4 % 3][:B], bk.Y[2 % 3][:B]) and bool(bk.Y[4 % 3][:B].any())


# ----------------------------------------------------------------------------- inference
@pytest.mark.parametrize("graphs", [False, True])
def test_inference_on_every_plan_kind(cuda_device, monkeypatch, graphs):
    """HipPolicyValueInference on a residual net against net.forward in fp32: buckets on the
    weight-stationary, split-K and tile plans (read from bk.plan), eager and captured."""
    from alphago_amd.models.inference import HipPolicyValueInference

    net = _residual_net(192, 5, seed=4).to(cuda_device)
    plain = copy.deepcopy(net)
    plain.trunk.residual = False
    seen = set()
    for n, bucket, ws in ((7, 8, "1"), (3, 4, "0"), (40, 64, "1")):
        monkeypatch.setenv("ALPHAGO_AMD_WS", ws)
        eng = HipPolicyValueInference(net, cuda_device, buckets=(bucket,), use_graphs=graphs)
        x, legal = _planes(n, seed=n)
        probs, values = [t.clone() for t in eng.evaluate(x, legal)]
        probs2, values2 = eng.evaluate(x, legal)  # a second submission: the captured graph replays
        torch.cuda.synchronize()
        kinds = {p.kind for p in eng._b[(bucket, 0)].plan[1:]}
        assert len(kinds) == 1
        seen |= kinds
        assert torch.equal(probs, probs2) and torch.equal(values, values2)
        xt, lt = torch.from_numpy(x).to(cuda_device), torch.from_numpy(legal).to(cuda_device)
        with torch.no_grad():
            z, v_ref = net.logits_value_torch(xt.float())
            p_ref = torch.softmax(z.masked_fill(lt == 0, float("-inf")), 1)
            z_plain, v_plain = plain.logits_value_torch(xt.float())
            p_plain = torch.softmax(z_plain.masked_fill(lt == 0, float("-inf")), 1)
        print(kinds, "max |dp| %.3g max |dv| %.3g" % ((probs - p_ref).abs().max().item(),
                                                     (values - v_ref).abs().max().item()))
        torch.testing.assert_close(values.contiguous(), v_ref, atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(probs.contiguous(), p_ref, atol=2e-2, rtol=2e-2)
        assert not bool((probs[lt == 0] != 0).any())
        # and not the plain stack's function: the skips are in the engine
        assert not (torch.allclose(v_plain, v_ref, atol=2e-2, rtol=2e-2)
                    and torch.allclose(p_plain, p_ref, atol=2e-2, rtol=2e-2))
    assert seen == {"ws", "splitk", "tile"}


def test_encoded_path(cuda_device):
    """evaluate_encoded (GPU featurizer in the graph) equals evaluate on the host-featurized planes."""
    from alphago_amd._native import engine
    from alphago_amd.features import VALUE_FEATURES, Preprocess
    from alphago_amd.models.inference import HipPolicyValueInference
    from test_engine_state import game_states

    net = _residual_net(64, 5, seed=5).to(cuda_device)
    states = game_states(5, 7, 60, 140)
    eng = HipPolicyValueInference(net, cuda_device, buckets=(8,), feature_list=list(VALUE_FEATURES))
    out, mask, bad = eng.evaluate_encoded(*engine().encode_batch(states, True, 2))
    probs, values = [t.clone() for t in eng.split_outputs(out)]
    x = Preprocess(VALUE_FEATURES).states_to_uint8(states)
    p2, v2 = eng.evaluate(x, mask.cpu().numpy())
    torch.cuda.synchronize()
    assert not bad and torch.equal(probs, p2) and torch.equal(values, v2)


def test_symmetry_ensembling_over_a_residual_trunk(cuda_device, mode="all"):
    """The ensembling engine (HipTrunkInference; the dual engine takes symmetries="none" only) over a
    residual trunk: it acts on inputs and outputs, so it equals the torch engine's ensemble of
    forward_torch within the same tolerance."""
    from alphago_amd.models.inference import HipTrunkInference, TorchPolicyInference
    from alphago_amd.models.nets import ConvStack, PolicyNet

    src = _residual_net(64, 5, seed=6)
    net = PolicyNet(49, S, 64, 5)
    net.trunk = ConvStack(49, 64, 5, [5, 3, 3, 3, 3], residual=True)
    net.trunk.load_state_dict(src.trunk.state_dict())
    with torch.no_grad():
        net.head_w.copy_(src.head_w)
    net = net.to(cuda_device)
    x, legal = _planes(5, seed=9)
    hip = HipTrunkInference(net, cuda_device, buckets=(8,), symmetries=mode, symmetry_seed=3)
    ref = TorchPolicyInference(net, cuda_device, symmetries=mode, symmetry_seed=3)
    assert hip.residual
    p = hip.evaluate(x, legal)
    p_ref = ref.evaluate(x, legal)
    torch.cuda.synchronize()
    torch.testing.assert_close(p.float().contiguous(), p_ref.float().to(cuda_device), atol=2e-2, rtol=2e-2)
    assert torch.allclose(p.float().sum(1), torch.ones(5, device=cuda_device), atol=1e-3)


# ----------------------------------------------------------------------------- refusals
def test_fp8_is_refused(cuda_device, monkeypatch):
    from alphago_amd.models.inference import HipPolicyValueInference
    from alphago_amd.train.engine import HipPolicyValueTrainer

    net = _residual_net(64, 3)
    with pytest.raises(ValueError, match="bf16 only"):
        HipPolicyValueTrainer(copy.deepcopy(net), 2, lr=0.01, device=cuda_device, precision="fp8")
    with pytest.raises(ValueError, match="ALPHAGO_AMD_PRECISION"):
        HipPolicyValueInference(net, cuda_device, precision="fp8")
    monkeypatch.setenv("ALPHAGO_AMD_PRECISION", "fp8")
    with pytest.raises(ValueError, match="ALPHAGO_AMD_PRECISION"):
        HipPolicyValueInference(net, cuda_device)
    monkeypatch.delenv("ALPHAGO_AMD_PRECISION")
    monkeypatch.setenv("ALPHAGO_AMD_LAB_TILE", "5")
    with pytest.raises(ValueError, match="ALPHAGO_AMD_LAB_TILE"):
        HipPolicyValueTrainer(copy.deepcopy(net), 2, lr=0.01, device=cuda_device)
