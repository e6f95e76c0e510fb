"""The score head through the HIP engines: the silent fresh head against the same net without it, one training step
against its autograd twin, the inference engine's score and utility column, weight refresh under captured graphs,
the untouched engine with ``score=False`` and the fp8 trainers.

Nets: residual, 5 layers, S = 19, F = 192 and F = 152 (padded tiles), B = 2 and 70, with the score head alone and
with pass + ownership + gpool.  Tolerances are tests/test_pass_head_engines.py's for the HIP trainer against torch
(every named gradient within cosine 0.98 and 5 % in norm, losses and metric sums within rtol / atol 2e-2) and
tests/test_fp8_residual_engines.py's for fp8 against bf16 gradients (cosine >= 0.95 and norm ratio in 0.8-1.25 per
weight, cosine > 0.85 per bias)."""
import copy

import pytest
import torch

import score_head_refs as SR
from test_pv_ownership import _own_target
from test_pv_residual import _planes
from test_pv_trainer import _batch, _cos_ratio

pytestmark = pytest.mark.gpu

S = 19
NP = S * S
L = 5
SCORE_NAMES = ("sc1_w", "sc1_b", "sc2_w", "sc2_b")
FULL = dict(pass_head=1, ownership=1, gpool=1)
NETS = [(192, 2, {}), (152, 70, {}), (192, 70, FULL), (152, 2, FULL)]


def _score_net(Fl, seed=0, live=True, score_head=1, **kw):
    """he_uniform_, the block ends and gates re-drawn live (test_gpool_engines' way), the pass head live
    (test_pass_head_engines' way) and -- ``live`` -- the score head's output layer re-drawn with the LeCun bound of
    its inputs and a bias of 0.25; otherwise it keeps he_uniform_'s zero."""
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_

    g = torch.Generator().manual_seed(seed)
    net = he_uniform_(PolicyValueNet(49, S, Fl, L, residual=1, score_head=score_head, **kw), generator=g)
    nb = (L - 1) // 2
    with torch.no_grad():
        bound = (6.0 / (Fl * 9)) ** 0.5 * nb ** -0.5
        for l in range(2, L, 2):
            net.trunk.weights[l].uniform_(-bound, bound, generator=g)
        gb = (3.0 / (2 * Fl)) ** 0.5 * nb ** -0.5
        for w in getattr(net.trunk, "gpool_w", ()):
            w.uniform_(-gb, gb, generator=g)
        if kw.get("pass_head"):
            pb = (3.0 / (2 * Fl)) ** 0.5
            net.pass_w.uniform_(-pb, pb, generator=g)
            net.pass_b.fill_(1.0)
        if score_head and live:
            sb = (3.0 / net.score_dense) ** 0.5
            net.sc2_w.uniform_(-sb, sb, generator=g)
            net.sc2_b.fill_(0.25)
    return net


def _without_head(net):
    """The same weights in a net without the score head."""
    from alphago_amd.models.nets import PolicyValueNet

    plain = PolicyValueNet(**{k: v for k, v in net.arch.items() if k not in ("score_head", "score_dense")})
    plain.load_state_dict({k: v for k, v in net.state_dict().items() if not k.startswith("sc")})
    return plain


def _targets(device, B, kw, score=True, shift=0.0):
    planes, moves, pi, z, sym = _batch(device, B)
    g = torch.Generator().manual_seed(77)
    sc_t = (torch.randn(B, generator=g) * 12 + shift).to(device)  # points: both arms of the Huber loss at S = 19
    sc_v = torch.ones(B)
    sc_v[1] = 0
    own = None
    if kw.get("ownership"):  # the helper marks boards 1 and 3 invalid: made for four boards at least
        ot, ov = _own_target(device, max(B, 4))
        own = (ot[:B].contiguous(), ov[:B].contiguous())
    base = (pi, z) if own is None else (pi, z, own)
    full = (pi, z, own, (sc_t, sc_v.to(device)))
    wt = (torch.rand(B, generator=g) + 0.5).to(device)
    return planes, (full if score else base), base, sym, wt


# ----------------------------------------------------------------------------- trainer
@pytest.mark.parametrize("Fl,B,kw", NETS)
def test_the_fresh_head_is_silent(cuda_device, Fl, B, kw):
    """sc2_w = 0: DZ[L-1] and every other gradient of a step carry the bits of the same net built without the
    head; so do the policy and the value of the inference engine."""
    from alphago_amd.models.inference import HipPolicyValueInference
    from alphago_amd.train.engine import HipPolicyValueTrainer

    dev = cuda_device
    net = _score_net(Fl, seed=1, live=False, **kw)
    assert not bool(net.sc2_w.any())
    plain = _without_head(net)
    planes, full, base, sym, wt = _targets(dev, B, kw)
    a = HipPolicyValueTrainer(copy.deepcopy(net), B, lr=0.01, device=dev)
    b = HipPolicyValueTrainer(copy.deepcopy(plain), B, lr=0.01, device=dev)
    assert a.fp.names[-4:] == list(SCORE_NAMES) and a.fp.names[:-4] == b.fp.names
    a.compute_grads(planes, full, sym, wt)
    b.compute_grads(planes, base, sym, wt)
    torch.cuda.synchronize()
    assert torch.equal(a.DZ[-1].view(torch.int16), b.DZ[-1].view(torch.int16)) and bool(a.DZ[-1].any())
    for n in b.fp.names:
        assert torch.equal(a.fp.grad_views[n].view(torch.int32), b.fp.grad_views[n].view(torch.int32)), n
    assert bool(a.fp.grad_views["sc2_w"].any()) and bool(a.fp.grad_views["sc2_b"].any())  # the head itself learns
    assert not bool(a.fp.grad_views["sc1_w"].any())
    x, legal = _planes(min(B, 8), seed=B)
    ea = HipPolicyValueInference(net.to(dev), dev, buckets=(8,), use_graphs=False, score=True)
    eb = HipPolicyValueInference(plain.to(dev), dev, buckets=(8,), use_graphs=False)
    pa, va = ea.evaluate(x, legal)
    pb, vb = eb.evaluate(x, legal)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(va, vb)
    assert not bool(ea.score_view().any())


@pytest.mark.parametrize("Fl,B,kw", NETS)
def test_hip_step_matches_torch(cuda_device, Fl, B, kw):
    from alphago_amd.train.engine import HipPolicyValueTrainer, TorchPolicyValueTrainer

    dev = cuda_device
    net = _score_net(Fl, seed=2, **kw)
    net_ref = copy.deepcopy(net)
    planes, full, base, sym, wt = _targets(dev, B, kw)
    hip = HipPolicyValueTrainer(net, B, lr=0.01, device=dev, score_coef=0.8)
    ref = TorchPolicyValueTrainer(net_ref, B, lr=0.01, device=dev, score_coef=0.8)
    assert hip.fp.names == ref.fp.names and hip.fp.names[-4:] == list(SCORE_NAMES)
    if kw.get("pass_head"):
        assert hip.fp.names[-6:-4] == ["pass_w", "pass_b"]
    hip.compute_grads(planes, full, sym, wt)
    ref.compute_grads(planes, full, sym, wt)
    torch.cuda.synchronize()
    for name in hip.fp.names:
        if name == "head_b" and not kw.get("pass_head"):
            continue  # d(mean CE)/d(scalar logit bias) == 0 exactly without a pass logit beside it
        cos, ratio = _cos_ratio(hip.fp.grad_views[name], ref.fp.grad_views[name])
        print(name, round(cos, 5), round(ratio, 4))
        assert cos > 0.98 and abs(ratio - 1) < 0.05, (name, cos, ratio)
    for n in SCORE_NAMES:
        assert float(hip.fp.grad_views[n].abs().max()) > 0, n
    mh, mr = hip._step_metrics(), ref._metrics(*[t.sum() for t in ref._last])
    n = len(mh)
    assert n == len(mr) == (8 if kw.get("ownership") else 6)
    print("score sums", [float(x) for x in mh[-2:]], [float(x) for x in mr[-2:]])
    for i in (n - 2, n - 1):
        assert torch.allclose(mh[i], mr[i].float(), rtol=2e-2, atol=2e-2) and float(mh[i]) > 0
    eh, er = hip.evaluate(planes, full), ref.evaluate(planes, full)
    for i in (n - 2, n - 1):
        assert torch.allclose(eh[i], er[i].float(), rtol=2e-2, atol=2e-2)
    # without the fourth slot: no score term, zero gradients, two zero sums, and the other heads as before
    hip.compute_grads(planes, base, sym, wt)
    torch.cuda.synchronize()
    for nm in SCORE_NAMES:
        assert not bool(hip.fp.grad_views[nm].any()), nm
    m0 = hip._step_metrics()
    assert len(m0) == n and float(m0[-1]) == 0.0 and float(m0[-2]) == 0.0
    with pytest.raises(RuntimeError, match="graph mode"):
        hip.enable_graphs(True)


def test_two_identical_steps_give_identical_bits(cuda_device):
    from alphago_amd.train.engine import HipPolicyValueTrainer

    dev = cuda_device
    Fl, B, kw = 152, 70, FULL
    net = _score_net(Fl, seed=3, **kw)
    planes, full, base, sym, wt = _targets(dev, B, kw)
    a = HipPolicyValueTrainer(copy.deepcopy(net), B, lr=0.001, device=dev)
    b = HipPolicyValueTrainer(copy.deepcopy(net), B, lr=0.001, device=dev)
    assert tuple(a._sc_w1.shape) == (2 * a.Fp, 64) and a.Fp > Fl and not bool(a._sc_w1[Fl:a.Fp].any())
    ma, mb = a.step(planes, full, sym), b.step(planes, full, sym)
    torch.cuda.synchronize()
    assert torch.equal(a.fp.grad.view(torch.int32), b.fp.grad.view(torch.int32))
    assert torch.equal(a.fp.flat.view(torch.int32), b.fp.flat.view(torch.int32))
    assert all(torch.equal(x, y) for x, y in zip(ma, mb)) and all(bool(torch.isfinite(x)) for x in ma)
    # repack refreshed the zero-padded copy of the updated sc1_w
    w = a.fp.views["sc1_w"]
    assert torch.equal(a._sc_w1[:Fl], w[:Fl]) and torch.equal(a._sc_w1[a.Fp:a.Fp + Fl], w[Fl:])
    assert float((w.cpu() - net.sc1_w.detach()).abs().max()) > 0


# ----------------------------------------------------------------------------- inference
@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("Fl,B,kw", NETS[:1] + NETS[3:])
def test_inference_score_and_utility(cuda_device, Fl, B, kw, graphs):
    from alphago_amd import ops
    from alphago_amd.models.inference import HipPolicyValueInference

    dev = cuda_device
    net = _score_net(Fl, seed=4, **kw).to(dev)
    eng = HipPolicyValueInference(net, dev, buckets=(2, 8), use_graphs=graphs, score=True)
    seen = {}
    head = eng._head
    eng._head = lambda bk, y: (seen.__setitem__(bk.B, y.clone()), head(bk, y))[1]
    lam = 0.5
    util = HipPolicyValueInference(net, dev, buckets=(2, 8), use_graphs=graphs, score_utility=lam)
    assert util.score and eng.score and eng.score_utility == 0.0
    ptrs = [t.data_ptr() for t in eng.shead]
    first = {}
    for n in (2, 6):  # both buckets
        x, legal = _planes(n, seed=n)
        probs, values = [t.clone() for t in eng.evaluate(x, legal)]
        score = eng.score_view().clone()
        eng.evaluate(x, legal)  # a second submission replays the graph
        torch.cuda.synchronize()
        assert torch.equal(score, eng.score_view()) and tuple(score.shape) == (n,)
        # against score_torch and the float64 reference on the engine's own bf16 trunk output
        bB = 2 if n == 2 else 8
        h = ops.from_padded(seen[bB], 1, Fl)[:n]
        with torch.no_grad():
            want = net.score_torch(h)
        w1, b1, w2, b2 = (t.detach().double() for t in (net.sc1_w, net.sc1_b, net.sc2_w, net.sc2_b))
        ref = SR.score_ref(h, w1, b1, w2, b2)
        P, _ = SR.pooled_ref(h)
        # fp32 roundings: NP per mean, 2F per hidden unit, D for the output, a few more; magnitudes of the chain
        mag = S * (((P.reshape(n, -1).abs() @ w1.abs() + b1.abs()) @ w2.abs()).squeeze(1) + b2.abs())
        bound = (NP + 2 * Fl + net.score_dense + 4) * SR.U24 * mag
        print("score err / bound: %.3g" % ((score.double() - ref).abs() / bound).max().item())
        assert bool(((score.double() - ref).abs() <= bound).all()) and bool(((want.double() - ref).abs() <= bound).all())
        assert float(score.abs().max()) > 0.5
        # the utility column, and everything else as without it
        pu, vu = util.evaluate(x, legal)
        torch.cuda.synchronize()
        assert torch.equal(pu, probs)
        formula = (values.double() + lam * torch.tanh(score.double() / (2 * S))) / (1 + lam)
        assert float((vu.double() - formula).abs().max()) < 1e-6 and float(vu.abs().max()) <= 1.0
        assert torch.equal(util.score_view(), score)
        first[n] = (x, legal, score, values)
    # a weight refresh reaches every captured bucket through the same tensors: sc2_b + 1 is S more points
    with torch.no_grad():
        net.sc2_b.add_(1.0)
    eng.sync_weights()
    assert ptrs == [t.data_ptr() for t in eng.shead]
    for n, (x, legal, score, values) in first.items():
        p2, v2 = eng.evaluate(x, legal)
        torch.cuda.synchronize()
        assert torch.equal(v2, values)
        assert float((eng.score_view() - score - S).abs().max()) < 1e-3


@pytest.mark.parametrize("Fl,B,kw", NETS[:1] + NETS[3:])
def test_score_false_launches_nothing_new(cuda_device, Fl, B, kw):
    """A net with the head on an engine built without the option (and with ``score_utility=0``): no score buffers,
    and the output rows are the bits of the head op the engine has always called."""
    from alphago_amd import ops
    from alphago_amd.models.inference import HipPolicyValueInference

    dev = cuda_device
    net = _score_net(Fl, seed=5, **kw).to(dev)
    for opts in (dict(), dict(score_utility=0.0)):
        eng = HipPolicyValueInference(net, dev, buckets=(8,), use_graphs=False, **opts)
        assert not eng.score and eng.shead is None
        seen = []
        head = eng._head
        eng._head = lambda bk, y: (seen.append((bk, y.clone())), head(bk, y))[1]
        x, legal = _planes(6, seed=1)
        probs, values = eng.evaluate(x, legal)
        torch.cuda.synchronize()
        bk, y = seen[-1]
        assert not hasattr(bk, "sc_up") and not hasattr(bk, "score")
        with pytest.raises(RuntimeError):
            eng.score_view()
        vw, vb, w1, b1, w2, b2 = eng.vhead
        NE = eng.NE
        p = torch.full((bk.B, NE), float("nan"), device=dev)
        zv = torch.full((bk.B, NP), float("nan"), device=dev)
        if kw.get("pass_head"):
            P = torch.zeros(bk.B, 2, eng.Fp, device=dev)
            a = torch.zeros(bk.B, eng.Fp, dtype=torch.int32, device=dev)
            ops.gpool_fwd(y, P, a, S)
            ops.policy_value_pass_head(y, eng.head_w, eng.head_b, vw, vb, P, eng.phead[0], eng.phead[1], p, zv, S,
                                       legal=bk.legal)
        else:
            ops.policy_value_head(y, eng.head_w, eng.head_b, vw, vb, p, zv, S, legal=bk.legal)
        hh = torch.zeros(bk.B, w1.shape[1], device=dev)
        val = torch.zeros(bk.B, device=dev)
        ops.dense_f32(zv, w1, hh, bias=b1)
        ops.value_out(hh, w2.view(-1), b2, val)
        torch.cuda.synchronize()
        assert torch.equal(probs.contiguous().view(torch.int32), p[:6].view(torch.int32))
        assert torch.equal(values.contiguous().view(torch.int32), val[:6].view(torch.int32))
    with pytest.raises(ValueError, match="score head"):
        HipPolicyValueInference(_without_head(net).to(dev), dev, buckets=(8,), use_graphs=False, score=True)


# ----------------------------------------------------------------------------- fp8
def _is_weight(name):
    return name.startswith("w") or name.endswith("_w")


def _check_arm(got, ref, names, what):
    for n in names:
        cos, ratio = _cos_ratio(got[n], ref[n])
        print(what, n, round(cos, 4), round(ratio, 4))
        if _is_weight(n):
            assert cos >= 0.95 and 0.8 < ratio < 1.25, (what, n, cos, ratio)
        else:
            assert cos > 0.85, (what, n, cos, ratio)


def test_fp8_steps(cuda_device):
    """precision="fp8", F = 192, residual, B = 32 (test_fp8_residual_engines' batch): the default arm after its
    calibrating call against the bf16 trainer, the all-fp8 backward's second call against the default arm's second
    call; finite score gradients in both, the trunk's and the score head's within that file's limits."""
    from alphago_amd.train.engine import HipPolicyValueTrainer

    dev = cuda_device
    B, kw = 32, dict(pass_head=1)
    net = _score_net(192, seed=6, **kw)
    # targets about S points below the prediction: the per-board gradients mostly share a sign, so that their sum
    # is no near-cancellation, which would amplify the fp8 forward's noise in s (asserted on the bf16 step below)
    planes, full, base, sym, wt = _targets(dev, B, kw, shift=-20.0)

    def grads(t):
        return {n: t.fp.grad_views[n].double().flatten().clone() for n in t.fp.names}

    bf = HipPolicyValueTrainer(copy.deepcopy(net), B, lr=0.0, device=dev)
    bf.compute_grads(planes, full, sym)
    g_bf = grads(bf)
    gb = bf._sc_dout[:, -1]
    assert float(gb.sum().abs()) > 0.5 * float(gb.abs().sum()) and float((bf._sc_abs > 1).float().mean()) < 0.9
    d = HipPolicyValueTrainer(copy.deepcopy(net), B, lr=0.0, device=dev, precision="fp8")
    d.compute_grads(planes, full, sym)
    g_first = grads(d)
    d.compute_grads(planes, full, sym)
    g_second = grads(d)
    a = HipPolicyValueTrainer(copy.deepcopy(net), B, lr=0.0, device=dev, precision="fp8", fp8_dgrad=True,
                              fp8_wgrad=True)
    assert a.fp8_dgrad and a.fp8_wgrad
    a.compute_grads(planes, full, sym)
    a.compute_grads(planes, full, sym)
    g_all = grads(a)
    torch.cuda.synchronize()
    for g in (g_first, g_all):
        for n in SCORE_NAMES:
            assert bool(torch.isfinite(g[n]).all()) and float(g[n].abs().max()) > 0, n
    trunk = ["w%d" % l for l in range(L)] + ["b%d" % l for l in range(L)]
    _check_arm(g_first, g_bf, trunk + list(SCORE_NAMES), "fp8 forward vs bf16")
    _check_arm(g_all, g_second, trunk + list(SCORE_NAMES), "all-fp8 vs bf16 backward")
