"""The global pooling branch through the HIP engines: the dual trainer's gradients (the gates' included)
against its autograd twin on every plan kind, the zero-gate identity, two optimizer steps, the inference
engine eager and captured (plan kinds, the encoded path, weight refresh, symmetry ensembling) and the
refusals.  Helpers and tolerances are tests/test_pv_residual.py's (test_pv_trainer.py's and
test_pv_inference.py's own)."""
import copy

import numpy as np
import pytest
import torch

from test_pv_ownership import _own_target
from test_pv_residual import _planes
from test_pv_trainer import _batch, _cos_ratio

pytestmark = pytest.mark.gpu

S = 19


def _gpool_net(Fl, L, k, seed=0, zero_gates=False, ownership=0):
    """he_uniform_, the block ends re-drawn live (test_pv_residual._residual_net), and the gates re-drawn
    uniform with the LeCun bound of their 2F inputs times the Fixup factor n_blocks ** -0.5."""
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_

    g = torch.Generator().manual_seed(seed)
    net = he_uniform_(PolicyValueNet(49, S, Fl, L, residual=1, gpool=k, ownership=ownership), generator=g)
    nb = (L - 1) // 2
    bound = (6.0 / (Fl * 9)) ** 0.5 * nb ** -0.5
    with torch.no_grad():
        for l in range(2, L, 2):
            net.trunk.weights[l].uniform_(-bound, bound, generator=g)
        if not zero_gates:
            gb = (3.0 / (2 * Fl)) ** 0.5 * nb ** -0.5
            for w in net.trunk.gpool_w:
                w.uniform_(-gb, gb, generator=g)
    return net


def _without_branch(net):
    """The same weights in a net without gpool."""
    from alphago_amd.models.nets import PolicyValueNet

    a = {k: v for k, v in net.arch.items() if k != "gpool"}
    plain = PolicyValueNet(**a)
    plain.load_state_dict({k: v for k, v in net.state_dict().items() if "gpool_w" not in k})
    return plain


def _check_grads(hip, ref):
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


# ----------------------------------------------------------------------------- trainer
@pytest.mark.parametrize("Fl,L,B,k,kinds,gates", [(64, 5, 6, 1, {"splitk"}, ["g2", "g4"]),
                                                  (192, 5, 5, 2, {"ws"}, ["g4"]),
                                                  (192, 3, 20, 1, {"tile"}, ["g2"]),
                                                  (48, 3, 6, 1, {"splitk"}, ["g2"])])
def test_hip_pv_grads_match_torch(cuda_device, Fl, L, B, k, kinds, gates):
    """HipPolicyValueTrainer.compute_grads against TorchPolicyValueTrainer on a deep copy: every named
    gradient, the gates' included, within cosine 0.98 and 5 % in norm, both losses within rtol / atol 2e-2.
    The 48-filter case runs on 64-wide tiles: the kernels see zero-padded copies of the gates."""
    from alphago_amd.train.engine import HipPolicyValueTrainer, TorchPolicyValueTrainer

    net = _gpool_net(Fl, L, k)
    net_ref = copy.deepcopy(net)
    planes, moves, pi, z, sym = _batch(cuda_device, B)
    tgt = (moves, z)
    hip = HipPolicyValueTrainer(net, B, lr=0.01, device=cuda_device)
    ref = TorchPolicyValueTrainer(net_ref, B, lr=0.01, device=cuda_device)
    assert hip.residual and {p.kind for p in hip.fwd_plan[1:]} == kinds == {p.kind for p in hip.dg_plan[1:]}
    assert hip.fp.names == ref.fp.names and [n for n in hip.fp.names if n[0] == "g"] == gates
    for g in gates:  # right after the bias of the block's last layer
        assert hip.fp.names[hip.fp.names.index(g) - 1] == "b" + g[1:]
    hip.compute_grads(planes, tgt, sym)
    ref.compute_grads(planes, tgt, sym)
    torch.cuda.synchronize()
    _check_grads(hip, ref)
    for g in gates:
        assert float(hip.fp.grad_views[g].abs().max()) > 0
    # the branch matters: the same weights without it give another gradient for the stem
    other = TorchPolicyValueTrainer(_without_branch(net_ref), B, lr=0.01, device=cuda_device)
    other.compute_grads(planes, tgt, sym)
    cos = _cos_ratio(other.fp.grad_views["w0"], ref.fp.grad_views["w0"])[0]
    print("without the branch: w0 cosine", round(cos, 5))
    assert cos < 0.98


@pytest.mark.parametrize("Fl,L,B,k", [(64, 5, 6, 1), (192, 3, 20, 1)])
def test_zero_gates_give_the_gradients_of_the_net_without(cuda_device, Fl, L, B, k):
    """Wg = 0: R == Y[l-1] and G2 == 0 exactly, so every trunk and head gradient equals that of the same
    weights in a net without gpool (torch.equal: adding a zero can only turn a -0 into a +0); the gates'
    own gradients are not zero."""
    from alphago_amd.train.engine import HipPolicyValueTrainer

    net = _gpool_net(Fl, L, k, seed=1, zero_gates=True)
    plain = _without_branch(net)
    planes, moves, pi, z, sym = _batch(cuda_device, B)
    hip = HipPolicyValueTrainer(net, B, lr=0.01, device=cuda_device)
    base = HipPolicyValueTrainer(plain, B, lr=0.01, device=cuda_device)
    hip.compute_grads(planes, (moves, z), sym)
    base.compute_grads(planes, (moves, z), sym)
    torch.cuda.synchronize()
    for name in base.fp.names:
        assert torch.equal(hip.fp.grad_views[name], base.fp.grad_views[name]), name
    for name in hip.fp.names:
        if name[0] == "g":
            assert float(hip.fp.grad_views[name].abs().max()) > 0, name


def test_ownership_head_and_reduce_stream(cuda_device):
    """A net with the ownership head (the gates follow ohead_* in the module, g<l> follows b<l> in the flat
    parameters), and the same step with the split-K reduce on its side stream: the same gradients."""
    from alphago_amd.train.engine import HipPolicyValueTrainer, TorchPolicyValueTrainer

    Fl, L, B = 64, 5, 6
    net = _gpool_net(Fl, L, 1, seed=2, ownership=1)
    net_ref, net_rs = copy.deepcopy(net), copy.deepcopy(net)
    planes, moves, pi, z, sym = _batch(cuda_device, B)
    tgt = (moves, z, _own_target(cuda_device, B))
    hip = HipPolicyValueTrainer(net, B, lr=0.01, device=cuda_device)
    ref = TorchPolicyValueTrainer(net_ref, B, lr=0.01, device=cuda_device)
    rs = HipPolicyValueTrainer(net_rs, B, lr=0.01, device=cuda_device, reduce_stream=True)
    assert rs.s_r is not None and hip.fp.names == ref.fp.names and hip.fp.names[-2:] == ["ohead_w", "ohead_b"]
    hip.compute_grads(planes, tgt, sym)
    ref.compute_grads(planes, tgt, sym)
    rs.compute_grads(planes, tgt, sym)
    torch.cuda.synchronize()
    _check_grads(hip, ref)
    _check_grads(rs, ref)


def test_two_optimizer_steps(cuda_device):
    """Two steps on two batches: finite losses and every gate moves in both.  Then the stepped trainer and a
    fresh one built from the updated weights give the same gradients for a third batch, bit for bit (the
    kernels are deterministic): a P, an argmax, an R / G2 or a padded gate copy left over from an earlier
    step would show."""
    from alphago_amd.train.engine import HipPolicyValueTrainer

    Fl, L, B = 48, 5, 6  # 48 filters on 64-wide tiles: the padded gate copies are refreshed by every update
    net = _gpool_net(Fl, L, 1, seed=3)
    # lr 1e-3: at 1e-2 two SGD steps drive this He-initialised value head into tanh saturation (v == -1 in
    # fp32 on every board, in the autograd trainer too) and its gradients are exactly zero
    hip = HipPolicyValueTrainer(net, B, lr=0.001, device=cuda_device)
    for step in range(2):
        planes, moves, pi, z, sym = _batch(cuda_device, B, seed=step)
        before = [hip.fp.views[n].clone() for n in ("g2", "g4")]
        m = hip.step(planes, (moves, z), sym)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v)) for v in m)
        assert all(bool((b != hip.fp.views[n]).any()) for b, n in zip(before, ("g2", "g4")))
    fresh_net = _gpool_net(Fl, L, 1, seed=3)
    fresh_net.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    fresh = HipPolicyValueTrainer(fresh_net, B, lr=0.001, device=cuda_device)
    planes, moves, pi, z, sym = _batch(cuda_device, B, seed=2)
    hip.compute_grads(planes, (moves, z), sym)
    fresh.compute_grads(planes, (moves, z), sym)
    torch.cuda.synchronize()
    for name in hip.fp.names:
        assert torch.equal(hip.fp.grad_views[name], fresh.fp.grad_views[name]), name
    assert float(hip.fp.grad_views["g2"].abs().max()) > 0 and float(hip.fp.grad_views["vhead_w"].abs().max()) > 0


# ----------------------------------------------------------------------------- inference
@pytest.mark.parametrize("graphs", [False, True])
def test_inference_on_every_plan_kind(cuda_device, monkeypatch, graphs):
    """HipPolicyValueInference on a gpool net against net.forward in fp32 on the weight-stationary, split-K
    and tile plans, eager and captured; not the function of the net without the branch; and after
    sync_weights with new gates the same bucket gives the new result (the in-place contract)."""
    from alphago_amd.models.inference import HipPolicyValueInference

    net = _gpool_net(192, 5, 1, seed=4).to(cuda_device)
    plain = _without_branch(net).to(cuda_device)
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

        def oracle(m):
            with torch.no_grad():
                z, v = m.logits_value_torch(xt.float())
                return torch.softmax(z.masked_fill(lt == 0, float("-inf")), 1), v

        p_ref, v_ref = oracle(net)
        p_plain, v_plain = oracle(plain)
        print(kinds, "max |dp| %.3g max |dv| %.3g" % ((probs - p_ref).abs().max().item(),
                                                     (values - v_ref).abs().max().item()))
        torch.testing.assert_close(values.contiguous(), v_ref, atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(probs.contiguous(), p_ref, atol=2e-2, rtol=2e-2)
        assert not (torch.allclose(v_plain, v_ref, atol=2e-2, rtol=2e-2)
                    and torch.allclose(p_plain, p_ref, atol=2e-2, rtol=2e-2))
        if bucket == 8:  # new gates into the same (captured) bucket
            saved = [w.detach().clone() for w in net.trunk.gpool_w]
            ptrs = [w.data_ptr() for w in eng.gpool_w]
            with torch.no_grad():
                for w in net.trunk.gpool_w:
                    w.neg_()
            eng.sync_weights()
            assert ptrs == [w.data_ptr() for w in eng.gpool_w]
            p_new, v_new = [t.clone() for t in eng.evaluate(x, legal)]
            p_ref2, v_ref2 = oracle(net)
            torch.testing.assert_close(v_new.contiguous(), v_ref2, atol=2e-2, rtol=2e-2)
            torch.testing.assert_close(p_new.contiguous(), p_ref2, atol=2e-2, rtol=2e-2)
            assert not torch.allclose(v_ref2, v_ref, atol=2e-2, rtol=2e-2)
            with torch.no_grad():
                for w, s in zip(net.trunk.gpool_w, saved):
                    w.copy_(s)
    assert seen == {"ws", "splitk", "tile"}


def test_zero_gates_leave_the_trunk_output_unchanged(cuda_device):
    """Wg = 0: the engine's last Y buffer equals that of the engine of the net without gpool."""
    from alphago_amd.models.inference import HipPolicyValueInference

    net = _gpool_net(64, 5, 1, seed=5, zero_gates=True).to(cuda_device)
    plain = _without_branch(net).to(cuda_device)
    x, legal = _planes(6, seed=1)
    a = HipPolicyValueInference(net, cuda_device, buckets=(8,))
    b = HipPolicyValueInference(plain, cuda_device, buckets=(8,))
    a.evaluate(x, legal)
    b.evaluate(x, legal)
    torch.cuda.synchronize()
    ya, yb = a._b[(8, 0)].Y[4 % 3], b._b[(8, 0)].Y[4 % 3]
    assert torch.equal(ya, yb) and bool(ya.any())


def test_padded_width(cuda_device):
    """48 filters on 64-wide tiles: the engine's zero-padded gates give the net's function."""
    from alphago_amd.models.inference import HipPolicyValueInference

    net = _gpool_net(48, 3, 1, seed=8).to(cuda_device)
    x, legal = _planes(6, seed=2)
    probs, values = HipPolicyValueInference(net, cuda_device, buckets=(8,)).evaluate(x, legal)
    xt, lt = torch.from_numpy(x).to(cuda_device), torch.from_numpy(legal).to(cuda_device)
    with torch.no_grad():
        z, v_ref = net.logits_value_torch(xt.float())
        p_ref = torch.softmax(z.masked_fill(lt == 0, float("-inf")), 1)
    torch.testing.assert_close(values.contiguous(), v_ref, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(probs.contiguous(), p_ref, atol=2e-2, rtol=2e-2)


def test_encoded_path(cuda_device):
    """evaluate_encoded (GPU featurizer in the graph) equals evaluate on the host-featurized planes."""
    from alphago_amd._native import engine
    from alphago_amd.features import VALUE_FEATURES, Preprocess
    from alphago_amd.models.inference import HipPolicyValueInference
    from test_engine_state import game_states

    net = _gpool_net(64, 5, 2, seed=6).to(cuda_device)
    states = game_states(5, 7, 60, 140)
    eng = HipPolicyValueInference(net, cuda_device, buckets=(8,), feature_list=list(VALUE_FEATURES))
    out, mask, bad = eng.evaluate_encoded(*engine().encode_batch(states, True, 2))
    probs, values = [t.clone() for t in eng.split_outputs(out)]
    x = Preprocess(VALUE_FEATURES).states_to_uint8(states)
    p2, v2 = eng.evaluate(x, mask.cpu().numpy())
    torch.cuda.synchronize()
    assert not bad and torch.equal(probs, p2) and torch.equal(values, v2)


def test_symmetry_ensembling_over_a_gpool_trunk(cuda_device):
    """symmetries="all" on the ensembling engine (HipTrunkInference; the dual engine takes "none" only) over
    a gpool trunk: the pooling is per trunk board, so the result is the torch engine's mean of forward over
    the 8 symmetries within the same tolerance."""
    from alphago_amd.models.inference import HipTrunkInference, TorchPolicyInference
    from alphago_amd.models.nets import ConvStack, PolicyNet

    src = _gpool_net(64, 5, 1, seed=7)
    net = PolicyNet(49, S, 64, 5)
    net.trunk = ConvStack(49, 64, 5, [5, 3, 3, 3, 3], residual=True, gpool=1)
    net.trunk.init_gpool()
    net.trunk.load_state_dict(src.trunk.state_dict())
    with torch.no_grad():
        net.head_w.copy_(src.head_w)
    net = net.to(cuda_device)
    x, legal = _planes(5, seed=9)
    hip = HipTrunkInference(net, cuda_device, buckets=(8,), symmetries="all", symmetry_seed=3)
    ref = TorchPolicyInference(net, cuda_device, symmetries="all", symmetry_seed=3)
    assert hip.gpool_blocks == [0, 1]
    p = hip.evaluate(x, legal)
    p_ref = ref.evaluate(x, legal)
    torch.cuda.synchronize()
    torch.testing.assert_close(p.float().contiguous(), p_ref.float().to(cuda_device), atol=2e-2, rtol=2e-2)


# ----------------------------------------------------------------------------- refusals
def test_fp8_and_lab_tile_are_refused(cuda_device, monkeypatch):
    from alphago_amd.models.inference import HipPolicyValueInference
    from alphago_amd.train.engine import HipPolicyValueTrainer

    net = _gpool_net(192, 3, 1)
    with pytest.raises(ValueError, match="gpool=1.*bf16 only"):
        HipPolicyValueTrainer(copy.deepcopy(net), 2, lr=0.01, device=cuda_device, precision="fp8")
    with pytest.raises(ValueError, match="gpool=1.*ALPHAGO_AMD_PRECISION"):
        HipPolicyValueInference(net, cuda_device, precision="fp8")
    monkeypatch.setenv("ALPHAGO_AMD_PRECISION", "fp8")
    with pytest.raises(ValueError, match="gpool=1.*ALPHAGO_AMD_PRECISION"):
        HipPolicyValueInference(net, cuda_device)
    monkeypatch.delenv("ALPHAGO_AMD_PRECISION")
    monkeypatch.setenv("ALPHAGO_AMD_LAB_TILE", "5")
    with pytest.raises(ValueError, match="ALPHAGO_AMD_LAB_TILE"):
        HipPolicyValueTrainer(copy.deepcopy(net), 2, lr=0.01, device=cuda_device)
    monkeypatch.delenv("ALPHAGO_AMD_LAB_TILE")
    with pytest.raises(RuntimeError, match="graph mode"):
        HipPolicyValueTrainer(copy.deepcopy(net), 2, lr=0.01, device=cuda_device).enable_graphs(True)
