"""The ownership head through the HIP engines: the dual trainer's gradients against its autograd twin
(plain and residual trunks, hard and soft policy targets, symmetries, invalid boards), the zero
coefficient, the inference engine on every plan kind (eager, captured, encoded) and an fp8 trunk.
Shapes and tolerances are tests/test_pv_residual.py's."""
import copy

import numpy as np
import pytest
import torch

from test_pv_trainer import _batch, _cos_ratio

pytestmark = pytest.mark.gpu

S = 19
# With random moves the policy CE (about 6 per board) dominates the trunk gradient; at 8 the ownership
# term carries enough of it that another batch's ownership target moves w0 past the limits on every shape
# (computed with the autograd twin alone: cosine 0.47 .. 0.996, norm ratio off by 6 % .. 48 %).
OWN_COEF = 8.0

# vhead_b's gradient is one scalar, (sum_p (W1 w2)_p) * sum_b w_b dv_b with dv_b = 2 (v_b - z_b)(1 - v_b^2): with
# outcomes of both signs the sum over the boards cancels, and what is left carries the bf16 trunk's error in v
# magnified by sum |w_b dv_b| / |sum w_b dv_b|.  The net's seed is chosen per shape so that the autograd twin
# alone keeps that ratio below 1 / 0.3 (seed 0 leaves 0.086 at 64 x 5 plain and 0.19 at 192 x 3 residual).
NET_SEED = {(64, 5, 6, 0): 3, (192, 3, 20, 1): 5}


def _net(Fl, L, residual, ownership=1, seed=0):
    """he_uniform_; on a residual trunk the block-end convs re-drawn at the block-first bound
    (test_pv_residual._residual_net), so that the branches carry signal and gradient."""
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_

    g = torch.Generator().manual_seed(seed)
    net = he_uniform_(PolicyValueNet(49, S, Fl, L, residual=residual, ownership=ownership), generator=g)
    if residual:
        bound = (6.0 / (Fl * 9)) ** 0.5 * ((L - 1) // 2) ** -0.5
        with torch.no_grad():
            for l in range(2, L, 2):
                net.trunk.weights[l].uniform_(-bound, bound, generator=g)
    return net


def _own_target(device, B, seed=0):
    """(own_t (B, S*S) int8, own_valid (B,)) with boards 1 and 3 invalid.  The maps are territory-like: a
    random line through the board with +1 on one side and -1 on the other, and about a tenth of the points
    neutral (a map drawn point by point would average out of the conv gradients, unlike any real one)."""
    g = torch.Generator().manual_seed(1000 + seed)
    xs = torch.arange(S).float().view(1, S, 1) - (S - 1) / 2
    ys = torch.arange(S).float().view(1, 1, S) - (S - 1) / 2
    ang = torch.rand(B, 1, 1, generator=g) * 2 * torch.pi
    off = (torch.rand(B, 1, 1, generator=g) - 0.5) * S / 2
    side = xs * torch.cos(ang) + ys * torch.sin(ang) - off
    t = torch.where(side > 0, 1, -1).to(torch.int8)
    t[torch.rand(B, S, S, generator=g) < 0.1] = 0
    valid = torch.ones(B)
    valid[1] = 0
    valid[3] = 0
    return t.reshape(B, S * S).to(device), valid.to(device)


def _planes(n, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 49, S, S)) < 0.4).astype(np.uint8), (rng.random((n, S * S)) < 0.6).astype(np.uint8)


# ----------------------------------------------------------------------------- trainer
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("residual", [0, 1])
@pytest.mark.parametrize("Fl,L,B", [(64, 5, 6), (192, 3, 20), (192, 5, 5)])
def test_hip_grads_match_torch(cuda_device, Fl, L, B, residual, soft):
    """Every named gradient of HipPolicyValueTrainer, ohead_w and ohead_b included, against
    TorchPolicyValueTrainer on a deep copy: cosine > 0.98, norm within 5 %, the three per-board losses
    within rtol / atol 2e-2; with symmetries, per-board weights and two invalid boards.  A control with
    the ownership target of another batch misses those limits on w0."""
    from alphago_amd.train.engine import HipPolicyValueTrainer, TorchPolicyValueTrainer

    from alphago_amd.train.engine import apply_symmetry

    dev = cuda_device
    net = _net(Fl, L, residual, seed=NET_SEED.get((Fl, L, B, residual), 0))
    net_ref = copy.deepcopy(net)
    planes, moves, pi, z, sym = _batch(dev, B)
    own = _own_target(dev, B)
    weight = (torch.rand(B, generator=torch.Generator().manual_seed(3)) + 0.5).to(dev)
    tgt = (pi if soft else moves, z, own)
    hip = HipPolicyValueTrainer(net, B, lr=0.01, device=dev, own_coef=OWN_COEF)
    ref = TorchPolicyValueTrainer(net_ref, B, lr=0.01, device=dev, own_coef=OWN_COEF)
    assert hip.fp.names[-2:] == ["ohead_w", "ohead_b"] and hip.fp.names == ref.fp.names
    v = ref.predict(apply_symmetry(planes, None, sym, ref.table)[0])
    dv = weight * 2 * (v - z) * (1 - v * v)
    assert float(dv.sum().abs() / dv.abs().sum()) >= 0.3  # the reference alone: vhead_b is well conditioned
    hip.compute_grads(planes, tgt, sym, weight)
    ref.compute_grads(planes, tgt, sym, weight)
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
    assert torch.allclose(hip.oloss * own[1], ref._olast[0], rtol=2e-2, atol=2e-2)
    m = hip._step_metrics()
    assert len(m) == 6
    assert torch.allclose(m[4], ref._olast[0].sum(), rtol=2e-2, atol=2e-2)
    assert torch.allclose(m[5], ref._olast[1].sum(), rtol=0, atol=2e-2 * B)
    assert not bool(hip.dlo[1].any()) and not bool(hip.dlo[3].any()) and bool(hip.dlo[0].any())
    other = TorchPolicyValueTrainer(copy.deepcopy(net_ref), B, lr=0.01, device=dev, own_coef=OWN_COEF)
    other.compute_grads(planes, (tgt[0], z, (_own_target(dev, B, seed=1)[0], own[1])), sym, weight)
    cos, ratio = _cos_ratio(other.fp.grad_views["w0"], ref.fp.grad_views["w0"])
    print("control w0", round(cos, 5), round(ratio, 4))
    assert not (cos > 0.98 and abs(ratio - 1) < 0.05)


@pytest.mark.parametrize("soft", [False, True])
def test_zero_coefficient_is_the_net_without_the_head(cuda_device, soft):
    """own_coef = 0: every gradient except ohead_* equals that of the same weights in a net without the
    head (torch.equal: the two-head pass adds a zero to dZ, which can only turn a -0 into a +0), and a
    pair target on the net with the head gives the same and zero ohead gradients."""
    from alphago_amd.train.engine import HipPolicyValueTrainer

    dev = cuda_device
    Fl, L, B = 64, 5, 6
    net = _net(Fl, L, 0)
    plain = _net(Fl, L, 0, ownership=0)
    for n, p in plain.named_parameters():
        assert torch.equal(p, dict(net.named_parameters())[n]), n
    planes, moves, pi, z, sym = _batch(dev, B)
    own = _own_target(dev, B)
    a = HipPolicyValueTrainer(net, B, lr=0.01, device=dev, own_coef=0.0)
    b = HipPolicyValueTrainer(plain, B, lr=0.01, device=dev)
    a.compute_grads(planes, (pi if soft else moves, z, own), sym)
    b.compute_grads(planes, (pi if soft else moves, z), sym)
    torch.cuda.synchronize()
    assert len(b._step_metrics()) == 4 and b.fp.names == a.fp.names[:-2]
    for name in b.fp.names:
        assert a.fp.segments[name] == b.fp.segments[name]
        assert torch.equal(a.fp.grad_views[name], b.fp.grad_views[name]), name
    ga = {n: a.fp.grad_views[n].clone() for n in a.fp.names}
    assert bool(torch.isfinite(ga["ohead_w"]).all())
    a.compute_grads(planes, (pi if soft else moves, z), sym)
    torch.cuda.synchronize()
    for name in b.fp.names:
        assert torch.equal(a.fp.grad_views[name], ga[name]), name
    assert not bool(a.fp.grad_views["ohead_w"].any()) and not bool(a.fp.grad_views["ohead_b"].any())
    assert float(a._step_metrics()[4]) == 0.0
    with pytest.raises(ValueError, match="ownership head"):
        b.compute_grads(planes, (moves, z, own), sym)


def test_step_and_evaluate_return_six_sums(cuda_device):
    from alphago_amd.train.engine import HipPolicyValueTrainer, TorchPolicyValueTrainer

    dev = cuda_device
    B = 6
    net = _net(64, 3, 0)
    ref = TorchPolicyValueTrainer(copy.deepcopy(net), B, lr=0.01, device=dev)
    hip = HipPolicyValueTrainer(net, B, lr=0.01, device=dev)
    planes, moves, pi, z, sym = _batch(dev, B)
    own = _own_target(dev, B)
    e_hip = torch.stack(hip.evaluate(planes, (pi, z, own)))
    e_ref = torch.stack(ref.evaluate(planes, (pi, z, own)))
    o_hip, o_ref = hip.own.clone(), ref.net.ownership_torch(ref.net.trunk.forward_torch(planes.float())).detach()
    s_hip = torch.stack(hip.step(planes, (pi, z, own), sym))
    torch.cuda.synchronize()
    assert e_hip.shape == (6,) and s_hip.shape == (6,) and bool(torch.isfinite(s_hip).all())
    torch.testing.assert_close(o_hip, o_ref, atol=2e-2, rtol=2e-2)
    for i in (0, 2, 4):  # the three losses; the counts can differ where a value sits at a tie
        assert torch.allclose(e_hip[i], e_ref[i], rtol=2e-2, atol=2e-2), i
    assert abs(float(e_hip[5] - e_ref[5])) <= 2e-2 * B
    after = torch.stack(hip.evaluate(planes, (pi, z, own)))
    assert float(after[4]) != float(e_hip[4])  # the step moved the ownership head


# ----------------------------------------------------------------------------- inference
def _own_ref(net, xt):
    with torch.no_grad():
        return net.ownership_torch(net.trunk.forward_torch(xt.float()))


@pytest.mark.parametrize("graphs", [False, True])
def test_inference_ownership_on_every_plan_kind(cuda_device, monkeypatch, graphs):
    """own against the torch engine within atol / rtol 2e-2 on the weight-stationary, split-K and tile
    plans, eager and captured; the (B, S*S + 1) rows of an engine with the flag on are bit-equal to those
    of one with it off."""
    from alphago_amd.models.inference import HipPolicyValueInference, TorchPolicyValueInference

    dev = cuda_device
    net = _net(192, 5, 1, seed=4).to(dev)
    torch_eng = TorchPolicyValueInference(net, dev, ownership=True)
    seen = set()
    for n, bucket, ws in ((7, 8, "1"), (3, 4, "0"), (40, 64, "1")):
        monkeypatch.setenv("ALPHAGO_AMD_WS", ws)
        eng = HipPolicyValueInference(net, dev, buckets=(bucket,), use_graphs=graphs, ownership=True)
        off = HipPolicyValueInference(net, dev, buckets=(bucket,), use_graphs=graphs)
        x, legal = _planes(n, seed=n)
        probs, values = [t.clone() for t in eng.evaluate(x, legal)]
        own = eng.ownership_view().clone()
        probs2, values2 = eng.evaluate(x, legal)  # a second submission: the captured graph replays
        p_off, v_off = off.evaluate(x, legal)
        torch.cuda.synchronize()
        assert own.shape == (n, S * S) and torch.equal(own, eng.ownership_view())
        assert torch.equal(probs, probs2) and torch.equal(values, values2)
        assert torch.equal(probs, p_off) and torch.equal(values, v_off)
        seen |= {p.kind for p in eng._b[(bucket, 0)].plan[1:]}
        torch_eng.evaluate(x, legal)
        ref = torch_eng.ownership_view()
        print("max |d own| %.3g" % (own - ref).abs().max().item())
        torch.testing.assert_close(own, ref, atol=2e-2, rtol=2e-2)
        assert float(ref.abs().max()) > 0.05
        with pytest.raises(RuntimeError, match="ownership=True"):
            off.ownership_view()
    assert seen == {"ws", "splitk", "tile"}


def test_inference_flag_needs_the_head(cuda_device):
    from alphago_amd.models.inference import HipPolicyValueInference, TorchPolicyValueInference

    plain = _net(64, 3, 0, ownership=0)
    with pytest.raises(ValueError, match="ownership head"):
        HipPolicyValueInference(plain.to(cuda_device), cuda_device, ownership=True)
    with pytest.raises(ValueError, match="ownership head"):
        TorchPolicyValueInference(plain, "cpu", ownership=True)


def test_encoded_path_and_weight_refresh(cuda_device):
    """evaluate_encoded (GPU featurizer in the graph) fills own like evaluate on the host-featurized
    planes, the handle's view is the submission's, and sync_weights refreshes ohead in a captured bucket."""
    from alphago_amd._native import engine
    from alphago_amd.features import VALUE_FEATURES, Preprocess
    from alphago_amd.models.inference import HipPolicyValueInference
    from test_engine_state import game_states

    dev = cuda_device
    net = _net(64, 5, 1, seed=5).to(dev)
    states = game_states(5, 7, 60, 140)
    eng = HipPolicyValueInference(net, dev, buckets=(8,), feature_list=list(VALUE_FEATURES), ownership=True)
    enc = engine().encode_batch(states, True, 2)
    handle = eng.submit_encoded(*enc)
    own_enc = eng.ownership_view(handle).clone()
    out, mask, bad = eng.collect(handle)
    x = Preprocess(VALUE_FEATURES).states_to_uint8(states)
    eng.evaluate(x, mask.cpu().numpy())
    own = eng.ownership_view().clone()
    torch.cuda.synchronize()
    assert not bad and own_enc.shape == (5, S * S) and torch.equal(own_enc, own)
    ref = _own_ref(net, torch.from_numpy(x).to(dev))
    torch.testing.assert_close(own, ref, atol=2e-2, rtol=2e-2)
    with torch.no_grad():
        net.ohead_w.neg_()
        net.ohead_b.neg_()
    eng.sync_weights()
    handle = eng.submit_encoded(*enc)  # the captured graph replays on the refreshed head
    flipped = eng.ownership_view(handle).clone()
    torch.cuda.synchronize()
    assert torch.equal(flipped, -own_enc) and bool(own_enc.any())


def test_model_api_on_the_gpu(cuda_device):
    """CNNPolicyValue.batch_eval_ownership: (S, S) arrays, + = Black, from a second engine; the search
    engine keeps the flag off."""
    from alphago_amd.features import VALUE_FEATURES
    from alphago_amd.models.nets import he_uniform_
    from alphago_amd.models.policy import CNNPolicyValue
    from test_engine_state import game_states

    pv = CNNPolicyValue(list(VALUE_FEATURES), device="cpu", board=S, filters_per_layer=64, layers=3, ownership=1)
    he_uniform_(pv.model, torch.Generator().manual_seed(2))
    pv.device = torch.device(cuda_device)
    pv.model.to(pv.device)
    states = game_states(4, 11, 30, 90)
    maps = pv.batch_eval_ownership(states)
    pv.batch_eval_both(states)
    assert not pv.engine.ownership and pv._own_engine.ownership
    x = torch.from_numpy(pv.preprocessor.states_to_uint8(states)).to(cuda_device)
    ref = _own_ref(pv.model, x).cpu().numpy()
    assert len(maps) == 4 and {st.current_player for st in states} == {1, -1}
    for i, st in enumerate(states):
        assert maps[i].shape == (S, S)
        np.testing.assert_allclose(maps[i], ref[i].reshape(S, S) * st.current_player, atol=2e-2, rtol=2e-2)


# ----------------------------------------------------------------------------- fp8 trunk
def test_fp8_trunk(cuda_device):
    """A plain trunk with precision="fp8": the step runs, and the ownership loss (mean over the valid
    boards) is finite and within 2e-2 of the bf16 trainer's."""
    from alphago_amd.train.engine import HipPolicyValueTrainer

    dev = cuda_device
    Fl, L, B = 192, 3, 20
    net = _net(Fl, L, 0)
    planes, moves, pi, z, sym = _batch(dev, B)
    own = _own_target(dev, B)
    bf = HipPolicyValueTrainer(copy.deepcopy(net), B, lr=0.01, device=dev)
    f8 = HipPolicyValueTrainer(copy.deepcopy(net), B, lr=0.01, device=dev, precision="fp8")
    m_bf = torch.stack(bf.step(planes, (pi, z, own), sym))
    m_f8 = torch.stack(f8.step(planes, (pi, z, own), sym))
    torch.cuda.synchronize()
    n_valid = float(own[1].sum())
    l_bf, l_f8 = float(m_bf[4]) / n_valid, float(m_f8[4]) / n_valid
    print("ownership loss bf16 %.5f fp8 %.5f" % (l_bf, l_f8))
    assert bool(torch.isfinite(m_f8).all()) and bool(torch.isfinite(f8.fp.grad).all())
    assert l_bf > 0.1 and abs(l_f8 - l_bf) <= 2e-2
