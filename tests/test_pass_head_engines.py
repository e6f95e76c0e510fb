"""The pass head through the HIP engines: one training step against its autograd twin (pass_w and pass_b
included; with and without the ownership target, with gpool), run-to-run bits, the inference engine against the
torch engine eager and captured, weight refresh under a captured graph, the untouched engines of nets without the
head, an fp8 engine, and a search that passes.  Nets: a 5-layer residual F = 64 net at B = 6 and a 3-layer
F = 192 net at B = 4.  Tolerances are tests/test_pv_trainer.py's (every named gradient within cosine 0.98 and
5 % in norm, per-board losses within rtol / atol 2e-2) and tests/test_pv_residual.py's / test_gpool_engines.py's
for an engine against torch (atol / rtol 2e-2)."""
import copy

import pytest
import torch

from test_pv_ownership import _own_target
from test_pv_residual import _planes
from test_pv_trainer import _batch, _cos_ratio

pytestmark = pytest.mark.gpu

S = 19
NP = S * S

# (filters, layers, batch, net keywords)
NETS = [(64, 5, 6, dict(residual=1, gpool=1)), (192, 3, 4, dict())]


def _pass_net(Fl, L, seed=0, pass_head=1, **kw):
    """he_uniform_, block ends and gates re-drawn live (test_gpool_engines._gpool_net's way), and the pass head
    re-drawn with the LeCun bound of its 2F inputs and a bias of 1, so that the pass has visible probability."""
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_

    g = torch.Generator().manual_seed(seed)
    net = he_uniform_(PolicyValueNet(49, S, Fl, L, pass_head=pass_head, **kw), generator=g)
    with torch.no_grad():
        if kw.get("residual"):
            nb = (L - 1) // 2
            bound = (6.0 / (Fl * 9)) ** 0.5 * nb ** -0.5
            for l in range(2, L, 2):
                net.trunk.weights[l].uniform_(-bound, bound, generator=g)
            gb = (3.0 / (2 * Fl)) ** 0.5 * nb ** -0.5
            for w in getattr(net.trunk, "gpool_w", ()):
                w.uniform_(-gb, gb, generator=g)
        if pass_head:
            pb = (3.0 / (2 * Fl)) ** 0.5
            net.pass_w.uniform_(-pb, pb, generator=g)
            net.pass_b.fill_(1.0)
    return net


def _without_head(net):
    """The same weights in a net without the pass head."""
    from alphago_amd.models.nets import PolicyValueNet

    plain = PolicyValueNet(**{k: v for k, v in net.arch.items() if k != "pass_head"})
    plain.load_state_dict({k: v for k, v in net.state_dict().items() if not k.startswith("pass_")})
    return plain


def _check_grads(hip, ref):
    """test_pv_trainer.py's comparisons.  head_b is no exception here: with a pass logit beside the board logits a
    shift of the board bias alone changes the softmax, so its gradient is not zero."""
    for name in hip.fp.names:
        a, b = hip.fp.grad_views[name], ref.fp.grad_views[name]
        cos, ratio = _cos_ratio(a, b)
        print(name, round(cos, 5), round(ratio, 4))
        assert cos > 0.98 and abs(ratio - 1) < 0.05, (name, cos, ratio)
    assert torch.allclose(hip.loss, ref._last[0], rtol=2e-2, atol=2e-2)
    assert torch.allclose(hip.vloss, ref._vlast[0], rtol=2e-2, atol=2e-2)


def _targets(device, B, soft, own):
    planes, moves, pi, z, sym = _batch(device, B)
    moves = moves.clone()
    moves[1] = -1  # a played pass; pi[1] is _batch's all-pass row
    tgt = (pi if soft else moves, z) + ((_own_target(device, B),) if own else ())
    return planes, tgt, sym


# ----------------------------------------------------------------------------- trainer
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("own", [0, 1])
@pytest.mark.parametrize("Fl,L,B,kw", NETS)
def test_hip_step_matches_torch(cuda_device, Fl, L, B, kw, own, soft):
    from alphago_amd.train.engine import HipPolicyValueTrainer, TorchPolicyValueTrainer

    net = _pass_net(Fl, L, ownership=own, **kw)
    net_ref = copy.deepcopy(net)
    planes, tgt, sym = _targets(cuda_device, B, soft, own)
    hip = HipPolicyValueTrainer(net, B, lr=0.01, device=cuda_device)
    ref = TorchPolicyValueTrainer(net_ref, B, lr=0.01, device=cuda_device)
    assert hip.fp.names == ref.fp.names and hip.fp.names[-2:] == ["pass_w", "pass_b"]
    if own:
        assert hip.fp.names[-4:-2] == ["ohead_w", "ohead_b"]
    hip.compute_grads(planes, tgt, sym)
    ref.compute_grads(planes, tgt, sym)
    torch.cuda.synchronize()
    _check_grads(hip, ref)
    assert float(hip.fp.grad_views["pass_w"].abs().max()) > 0 and float(hip.fp.grad_views["pass_b"].abs()) > 0
    assert hip.loss[1].item() > 0.0  # the pass row has a loss now
    # the metric sums of evaluate: policy loss and top-1 count the pass row, the value pair as before
    mh, mr = hip.evaluate(planes, tgt), ref.evaluate(planes, tgt)
    assert len(mh) == len(mr) == (6 if own else 4)
    assert torch.allclose(mh[0], mr[0].float(), rtol=2e-2, atol=2e-2) and 0 <= mh[1].item() <= B
    assert torch.allclose(mh[2], mr[2].float(), rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("Fl,L,B,kw", NETS)
def test_two_identical_steps_give_identical_bits(cuda_device, Fl, L, B, kw):
    """The same step on two trainers built from one net, and twice on one of them: equal gradients, equal metric
    sums and, after the update, equal parameters, bit for bit."""
    from alphago_amd.train.engine import HipPolicyValueTrainer

    net = _pass_net(Fl, L, seed=1, ownership=1, **kw)
    planes, tgt, sym = _targets(cuda_device, B, True, 1)
    a = HipPolicyValueTrainer(copy.deepcopy(net), B, lr=0.001, device=cuda_device)
    b = HipPolicyValueTrainer(copy.deepcopy(net), B, lr=0.001, device=cuda_device)
    a.compute_grads(planes, tgt, sym)
    g0 = a.fp.grad.clone()
    a.compute_grads(planes, tgt, sym)
    torch.cuda.synchronize()
    assert torch.equal(a.fp.grad.view(torch.int32), g0.view(torch.int32))
    ma, mb = a.step(planes, tgt, sym), b.step(planes, tgt, sym)
    torch.cuda.synchronize()
    assert torch.equal(a.fp.grad.view(torch.int32), b.fp.grad.view(torch.int32))
    assert torch.equal(a.fp.flat.view(torch.int32), b.fp.flat.view(torch.int32))
    assert all(torch.equal(x, y) for x, y in zip(ma, mb)) and all(bool(torch.isfinite(x)) for x in ma)
    po, pn = a.fp.segments["pass_w"]
    assert float((a.fp.flat[po:po + pn + 1] - torch.cat([net.pass_w.detach().view(-1), net.pass_b.detach()]).to(cuda_device)).abs().max()) > 0


def test_padded_width_and_refusals(cuda_device):
    """48 filters on 64-wide tiles: the kernels read the zero-padded (2, 64) copy of pass_w, refreshed by repack();
    a narrower soft row and graph mode are refused."""
    from alphago_amd.train.engine import HipPolicyValueTrainer, TorchPolicyValueTrainer

    B = 6
    net = _pass_net(48, 3, seed=2)
    net_ref = copy.deepcopy(net)
    planes, tgt, sym = _targets(cuda_device, B, True, 0)
    hip = HipPolicyValueTrainer(net, B, lr=0.01, device=cuda_device)
    ref = TorchPolicyValueTrainer(net_ref, B, lr=0.01, device=cuda_device)
    assert tuple(hip._ps_w.shape) == (2, 64) and not bool(hip._ps_w[:, 48:].any())
    assert torch.equal(hip._ps_w[:, :48], hip.fp.views["pass_w"].view(2, 48))
    hip.compute_grads(planes, tgt, sym)
    ref.compute_grads(planes, tgt, sym)
    torch.cuda.synchronize()
    _check_grads(hip, ref)
    hip.apply_update()
    torch.cuda.synchronize()
    assert torch.equal(hip._ps_w[:, :48], hip.fp.views["pass_w"].view(2, 48)) and not bool(hip._ps_w[:, 48:].any())
    with pytest.raises(ValueError, match="pass last"):
        hip.compute_grads(planes, (tgt[0][:, :NP].contiguous(), tgt[1]), sym)
    with pytest.raises(RuntimeError, match="graph mode"):
        hip.enable_graphs(True)


# ----------------------------------------------------------------------------- inference
def _oracle(net, x, legal, device):
    from alphago_amd.models.inference import TorchPolicyValueInference

    p, v = TorchPolicyValueInference(net, device).evaluate(x, legal)
    return p, v


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("Fl,L,B,kw", NETS)
def test_inference_matches_torch(cuda_device, Fl, L, B, kw, own, graphs):
    """The NP + 1 probabilities and the value against the torch engine, eager and captured (a second submission
    replays the graph); illegal points exactly 0, rows summing to 1; and after sync_weights with a changed pass_b
    the same bucket gives the new pass column out of the same tensors."""
    from alphago_amd.models.inference import HipPolicyValueInference

    net = _pass_net(Fl, L, seed=3, ownership=int(own), **kw).to(cuda_device)
    eng = HipPolicyValueInference(net, cuda_device, buckets=(8,), use_graphs=graphs, ownership=own)
    assert eng.pass_head and eng.NE == NP + 1
    x, legal = _planes(B, seed=B)
    legal[B - 1] = 0  # a board with no legal point
    probs, values = [t.clone() for t in eng.evaluate(x, legal)]
    probs2, values2 = eng.evaluate(x, legal)
    torch.cuda.synchronize()
    assert tuple(probs.shape) == (B, NP + 1) and tuple(values.shape) == (B,)
    assert torch.equal(probs, probs2) and torch.equal(values, values2)
    p_ref, v_ref = _oracle(net, x, legal, cuda_device)
    print("max |dp| %.3g max |dv| %.3g" % ((probs - p_ref).abs().max().item(), (values - v_ref).abs().max().item()))
    torch.testing.assert_close(values.contiguous(), v_ref, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(probs.contiguous(), p_ref, atol=2e-2, rtol=2e-2)
    lt = torch.from_numpy(legal).to(cuda_device)
    assert not bool((probs[:, :NP][lt == 0] != 0).any()) and probs[B - 1, NP].item() == 1.0
    assert float((probs.sum(1) - 1).abs().max()) < 1e-5 and bool((probs[:, NP] > 0).all())
    # the value and the ownership map do not see the pass head: the bits of the engine of the same weights without it
    plain = HipPolicyValueInference(_without_head(net).to(cuda_device), cuda_device, buckets=(8,), use_graphs=False,
                                    ownership=own)
    p0, v0 = plain.evaluate(x, legal)
    torch.cuda.synchronize()
    assert tuple(p0.shape) == (B, NP) and torch.equal(v0, values)
    if own:
        assert torch.equal(eng.ownership_view(), plain.ownership_view()) and bool(eng.ownership_view().any())
    # a changed pass_b into the same (captured) bucket
    ptrs = [t.data_ptr() for t in eng.phead]
    with torch.no_grad():
        net.pass_b.fill_(4.0)
    eng.sync_weights()
    assert ptrs == [t.data_ptr() for t in eng.phead]
    p_new, v_new = [t.clone() for t in eng.evaluate(x, legal)]
    p_ref2, v_ref2 = _oracle(net, x, legal, cuda_device)
    torch.cuda.synchronize()
    torch.testing.assert_close(p_new.contiguous(), p_ref2, atol=2e-2, rtol=2e-2)
    assert torch.equal(v_new, values)  # the value head does not see pass_b
    # the same trunk output and three more in the pass logit: the log-odds of the pass move by 3
    po, pn = probs[:-1, NP].double(), p_new[:-1, NP].double()
    mid = (po > 1e-4) & (pn < 1 - 1e-4)
    assert bool((pn > po).all()) and bool(mid.any())
    shift = (torch.log(pn / (1 - pn)) - torch.log(po / (1 - po)))[mid]
    assert float((shift - 3.0).abs().max()) < 1e-2


@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("Fl,L,B,kw", NETS)
def test_engines_of_nets_without_the_head_are_untouched(cuda_device, Fl, L, B, kw, own):
    """A net without the head: rows of NP + 1 (probabilities, value) as before, and the probabilities are the bits
    of the net's own policy_value_head / policy_value_own_head call on the engine's trunk output.  (A digest of the
    parent commit's output could not be recorded without a GPU, so the comparison is against the op call.)"""
    from alphago_amd import ops
    from alphago_amd.models.inference import HipPolicyValueInference

    net = _pass_net(Fl, L, seed=4, pass_head=0, ownership=int(own), **kw).to(cuda_device)
    eng = HipPolicyValueInference(net, cuda_device, buckets=(8,), use_graphs=False, ownership=own)
    assert not eng.pass_head and eng.phead is None and eng.NE == NP
    seen = []
    head = eng._head
    eng._head = lambda bk, y: (seen.append((bk, y)), head(bk, y))[1]
    x, legal = _planes(B, seed=1)
    probs, values = eng.evaluate(x, legal)
    torch.cuda.synchronize()
    assert tuple(probs.shape) == (B, NP) and not hasattr(seen[-1][0], "ps_P")
    bk, y = seen[-1]
    vw, vb = eng.vhead[:2]
    p = torch.full((bk.B, NP), float("nan"), device=cuda_device)
    zv = torch.full((bk.B, NP), float("nan"), device=cuda_device)
    if own:
        ops.policy_value_own_head(y, eng.head_w, eng.head_b, vw, vb, eng.ohead[0], eng.ohead[1], p, zv,
                                  torch.zeros_like(zv), S, legal=bk.legal)
    else:
        ops.policy_value_head(y, eng.head_w, eng.head_b, vw, vb, p, zv, S, legal=bk.legal)
    torch.cuda.synchronize()
    assert torch.equal(probs.contiguous().view(torch.int32), p[:B].view(torch.int32))


def test_fp8_engine_pass_column(cuda_device):
    """An fp8 engine (F = 192, bucket 256): every arm of the trunk hands the head a bf16 top output, so the pass
    column is the new head op applied to that output: equal bits."""
    from alphago_amd import ops
    from alphago_amd.models.inference import HipPolicyValueInference

    net = _pass_net(192, 3, seed=5).to(cuda_device)
    eng = HipPolicyValueInference(net, cuda_device, buckets=(256,), use_graphs=False, precision="fp8")
    eng.fp8_min_batch = 0
    seen = []
    head = eng._head
    eng._head = lambda bk, y: (seen.append((bk, y.clone())), head(bk, y))[1]
    x, legal = _planes(256, seed=6)
    probs, values = eng.evaluate(x, legal)
    torch.cuda.synchronize()
    assert eng.calibrated and eng.precision == "fp8" and tuple(probs.shape) == (256, NP + 1)
    bk, y = seen[-1]
    assert y.dtype == torch.bfloat16
    P = torch.zeros(256, 2, eng.Fp, device=cuda_device)
    a = torch.zeros(256, eng.Fp, dtype=torch.int32, device=cuda_device)
    ops.gpool_fwd(y, P, a, S)
    p = torch.full((256, NP + 1), float("nan"), device=cuda_device)
    zv = torch.zeros(256, NP, device=cuda_device)
    vw, vb = eng.vhead[:2]
    ops.policy_value_pass_head(y, eng.head_w, eng.head_b, vw, vb, P, eng.phead[0], eng.phead[1], p, zv, S,
                               legal=bk.legal)
    torch.cuda.synchronize()
    assert torch.equal(probs.contiguous().view(torch.int32), p.view(torch.int32))
    assert bool((probs[:, NP] > 0).all()) and float((probs.sum(1) - 1).abs().max()) < 1e-5


# ----------------------------------------------------------------------------- search
def test_search_with_the_real_engine_passes(cuda_device):
    """BatchedMCTS over the HIP engine of a 9 x 9 net whose pass_b is large: the pass column reaches the forest
    (the encoded path) and the root's answer is PASS."""
    from alphago_amd import go
    from alphago_amd.models.nets import he_uniform_
    from alphago_amd.models.policy import CNNPolicyValue
    from alphago_amd.search.mcts import BatchedMCTS

    torch.manual_seed(7)
    pv = CNNPolicyValue(device=cuda_device, board=9, filters_per_layer=64, layers=3, pass_head=1)
    he_uniform_(pv.model, generator=torch.Generator(device=cuda_device).manual_seed(7))
    with torch.no_grad():
        pv.model.pass_b.fill_(20.0)
    pv.refresh()
    assert pv.engine.pass_head
    st = go.GameState(size=9)
    for mv in [(2, 2), (6, 6), (2, 6)]:
        st.do_move(mv)
    mcts = BatchedMCTS(pv, n_trees=1, seed=3, threads=2)
    assert mcts.search([st], 48, leaves_per_tree=4) == [None]
    d = mcts.visit_distribution(0, 9)
    assert d.argmax() == 81 and d[81] > 0.9
    moves, visits, _ = mcts.forest.root_stats(0)
    assert moves[-1] is None and len(moves) > 1  # PASS stored last, beside the sensible moves
