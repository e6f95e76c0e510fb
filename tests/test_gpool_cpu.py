"""The global pooling branch of the residual trunk on the CPU: refusals, parameters and their draw order, the
Fixup zero, ``forward_torch`` against the fp64 numpy references (tests/gpool_refs.py), the tie rule,
gradcheck, the analytic backward, the spec and weight-file round trips, ``init-model pv --residual --gpool``
and a torch trainer step."""
import json

import numpy as np
import pytest
import torch

import gpool_refs as R

S, F, L, C0 = 5, 8, 5, 6


def _net(gpool=0, seed=0, he=False, live=False, **kw):
    """PolicyValueNet(S = 5, F = 8, L = 5) from ``seed``; ``live``: every parameter re-drawn non-zero."""
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_

    torch.manual_seed(seed)
    kw.setdefault("residual", 1)
    kw.setdefault("layers", L)
    net = PolicyValueNet(C0, S, F, dense=16, gpool=gpool, **kw)
    if he:
        he_uniform_(net, generator=torch.Generator().manual_seed(seed + 1))
    if live:
        g = torch.Generator().manual_seed(seed + 2)
        with torch.no_grad():
            for p in net.parameters():
                p.uniform_(-0.3, 0.3, generator=g)
    return net


def _np(t):
    return t.detach().double().numpy()


def _trunk_ref(net, x):
    tr = net.trunk
    gates = [None] * ((tr.layers - 1) // 2)
    for i, j in enumerate(tr.gpool_blocks):
        gates[j] = _np(tr.gpool_w[i])
    return R.trunk_forward(_np(x), [_np(w) for w in tr.weights], [_np(b) for b in tr.biases], gates)


# ----------------------------------------------------------------------------- refusals, parameters
def test_refusals():
    from alphago_amd.models.nets import PolicyValueNet

    with pytest.raises(ValueError, match="residual=1"):
        PolicyValueNet(C0, S, F, L, gpool=1)
    for k in (-1, 3):
        with pytest.raises(ValueError, match="valid choices: 1, 2"):
            PolicyValueNet(C0, S, F, L, residual=1, gpool=k)
    assert PolicyValueNet(C0, S, F, L, residual=1, gpool=2).trunk.gpool_blocks == [1]
    assert PolicyValueNet(C0, S, F, 7, residual=1, gpool=1).trunk.gpool_blocks == [0, 1, 2]


def test_unknown_gpool_is_no_longer_swallowed():
    """Before the feature ``gpool=`` disappeared into **kwargs: the net had no gates and no arch key."""
    net = _net(gpool=1)
    assert net.arch["gpool"] == 1 and len(net.trunk.gpool_w) == 2


@pytest.mark.parametrize("own", [0, 1])
def test_parameter_names_shapes_and_order(own):
    net = _net(gpool=2, ownership=own)
    names = [n for n, _ in net.named_parameters()]
    base = [n for n, _ in _net(ownership=own).named_parameters()]
    assert names == base + ["trunk.gpool_w.0"]  # created after every other parameter, the ownership head included
    assert tuple(net.trunk.gpool_w[0].shape) == (2 * F, F)
    assert [tuple(g.shape) for g in _net(gpool=1).trunk.gpool_w] == [(2 * F, F)] * 2


@pytest.mark.parametrize("he", [False, True])
@pytest.mark.parametrize("own", [0, 1])
def test_other_tensors_draw_what_they_draw_without_gpool(he, own):
    a, b = _net(seed=3, he=he, ownership=own), _net(gpool=1, seed=3, he=he, ownership=own)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    for n, p in pa.items():
        assert torch.equal(p, pb[n]), n
    drawn = all(bool(g.any()) and float(g.detach().abs().max()) <= 0.05 for g in b.trunk.gpool_w)
    assert drawn != he  # keras_uniform_ by default; he_uniform_ zeroes the gates


def test_he_uniform_zeroes_the_gates_and_the_net_is_the_net_without():
    a, b = _net(seed=4, he=True), _net(gpool=1, seed=4, he=True)
    with torch.no_grad():  # live block ends, so that the blocks compute something
        for l in (2, 4):
            a.trunk.weights[l].uniform_(-0.2, 0.2, generator=torch.Generator().manual_seed(l))
            b.trunk.weights[l].copy_(a.trunk.weights[l])
    assert all(not bool(g.any()) for g in b.trunk.gpool_w)
    x = (torch.rand(4, C0, S, S, generator=torch.Generator().manual_seed(0)) < 0.4).float()
    assert torch.equal(a.trunk.forward_torch(x), b.trunk.forward_torch(x))
    pa, va = a(x)
    pb, vb = b(x)
    assert torch.equal(pa, pb) and torch.equal(va, vb) and bool(a.trunk.forward_torch(x).any())


# ----------------------------------------------------------------------------- the function
@pytest.mark.parametrize("k", [1, 2])
def test_forward_torch_is_the_reference(k):
    net = _net(gpool=k, seed=5, live=True).double()
    x = torch.rand(3, C0, S, S, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        y = net.trunk.forward_torch(x)
    ref = _trunk_ref(net, x)
    err = np.abs(_np(y) - ref).max()
    print("gpool=%d max |forward_torch - ref| = %.3g, max |ref| = %.3g" % (k, err, np.abs(ref).max()))
    # fp64 sums of at most 9 * 8 + 2 * 8 + 2 terms per layer over 5 layers: 1e-12 is ~1e4 ulp of the largest value
    assert err <= 1e-12 * max(1.0, np.abs(ref).max())
    plain = _net(seed=5, live=True).double()
    plain.load_state_dict(net.state_dict(), strict=False)
    with torch.no_grad():
        y0 = plain.trunk.forward_torch(x)
    assert float((y - y0).abs().max()) > 1e-3  # the branch matters


def test_a_planted_tie_takes_the_lowest_index():
    from alphago_amd.models.nets import ConvStack

    tr = ConvStack(C0, F, 3, [5, 3, 3], residual=True, gpool=1)
    tr.init_gpool()
    y = torch.rand(2, F, S, S, dtype=torch.float64, generator=torch.Generator().manual_seed(2)) * 0.5
    y[0, 3, 1, 2] = y[0, 3, 4, 0] = 0.75   # two equal maxima: pixel 7 wins over pixel 20
    y[1, 5] = 0.0                          # an all-zero channel: pixel 0
    y[1, 6, 4, 4] = 0.9                    # the maximum at the last pixel
    y.requires_grad_(True)
    P, a = R.pool(_np(y))
    assert a[0, 3] == 7 and a[1, 5] == 0 and a[1, 6] == S * S - 1
    with torch.no_grad():
        tr.gpool_w[0].copy_(torch.eye(2 * F)[:, F:])  # g = the max half of P
    g = tr.double().gate_torch(y, 0)
    assert np.array_equal(_np(g), P[:, 1])
    g.sum().backward()
    hit = y.grad.reshape(2, F, -1) != 0
    assert bool((hit.sum(2) == 1).all())  # the max gradient lands on exactly one pixel per (b, c)
    assert np.array_equal(hit.double().argmax(2).numpy(), a)


def test_gradcheck():
    net = _net(gpool=1, seed=6, live=True, layers=3).double()
    x = torch.rand(2, C0, S, S, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    names = [n for n, _ in net.trunk.named_parameters()]
    net.trunk.forward = net.trunk.forward_torch  # functional_call goes through forward

    def f(xin, *ps):  # the input too: the pooling's gradient reaches it through the stem
        return torch.func.functional_call(net.trunk, dict(zip(names, ps)), (xin,), strict=True)

    ins = [x.requires_grad_(True)] + [p.detach().clone().requires_grad_(True) for p in net.trunk.parameters()]
    assert torch.autograd.gradcheck(f, ins, eps=1e-6, atol=1e-5, rtol=1e-4)


def test_autograd_is_the_analytic_backward():
    """Autograd of forward_torch on a stem + one block against gpool_refs.block_backward."""
    net = _net(gpool=1, seed=7, live=True, layers=3).double()
    tr = net.trunk
    x = torch.rand(3, C0, S, S, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    up = torch.rand(3, F, S, S, dtype=torch.float64, generator=torch.Generator().manual_seed(5)) - 0.3
    (tr.forward_torch(x) * up).sum().backward()
    y0 = np.maximum(R.conv(_np(x), _np(tr.weights[0]), _np(tr.biases[0])), 0.0)
    ref = R.block_backward(y0, _np(tr.weights[1]), _np(tr.biases[1]), _np(tr.weights[2]), _np(tr.biases[2]),
                           _np(tr.gpool_w[0]), _np(up))
    got = dict(w1=tr.weights[1].grad, b1=tr.biases[1].grad, w2=tr.weights[2].grad, b2=tr.biases[2].grad,
               Wg=tr.gpool_w[0].grad)
    for n, g in got.items():
        err = np.abs(_np(g) - ref[n]).max()
        print(n, "max |autograd - analytic| = %.3g of %.3g" % (err, np.abs(ref[n]).max()))
        assert np.abs(ref[n]).max() > 1e-3 and err <= 1e-11 * max(1.0, np.abs(ref[n]).max()), n


# ----------------------------------------------------------------------------- persistence, CLI
def test_spec_round_trip_and_unchanged_spec_without_gpool():
    from alphago_amd.io import keras_compat

    net = _net(gpool=2)
    spec = keras_compat.pv_spec(net)
    assert spec["gpool"] == 2
    back = keras_compat.pv_from_spec(json.loads(json.dumps(spec)))
    assert back.arch == net.arch and back.trunk.gpool_blocks == [1]
    plain = keras_compat.pv_spec(_net())
    assert "gpool" not in plain and list(plain) == ["input_dim", "board", "filters_per_layer", "layers", "dense",
                                                    "residual"]


@pytest.mark.parametrize("own", [0, 1])
def test_weight_file_round_trip(tmp_path, own):
    from alphago_amd.io import keras_compat
    from alphago_amd.io.h5lite import H5File

    net = _net(gpool=1, seed=8, live=True, ownership=own)
    path = str(tmp_path / "w.hdf5")
    keras_compat.save_weights(net, path)
    with H5File(path) as f:
        names = [n.decode() if isinstance(n, bytes) else str(n) for n in f.attrs["layer_names"]]
    assert names[-2:] == ["gpool_dense_1", "gpool_dense_2"]
    assert ("ownership_convolution2d_1" in names) == bool(own) and (not own or names[-3] == "ownership_convolution2d_1")
    other = _net(gpool=1, seed=9, ownership=own)
    keras_compat.load_weights(other, path)
    for (n, p), (_, q) in zip(net.named_parameters(), other.named_parameters()):
        assert torch.equal(p, q), n
    # a net without gpool writes the entries it always wrote
    keras_compat.save_weights(_net(ownership=own), path)
    with H5File(path) as f:
        assert not any(b"gpool" in (n if isinstance(n, bytes) else str(n).encode()) for n in f.attrs["layer_names"])


def test_init_model_gpool(tmp_path, capsys):
    from alphago_amd.cli import main
    from alphago_amd.models.policy import CNNPolicyValue

    js = str(tmp_path / "m.json")
    assert main(["init-model", "pv", js, "--weights", str(tmp_path / "m.hdf5"), "--board", "9", "--filters", "8",
                 "--layers", "5", "--residual", "--gpool", "2"]) == 0
    with open(js) as f:
        assert json.load(f)["pv_model"]["gpool"] == 2
    m = CNNPolicyValue.load_model(js, device="cpu")
    assert m.model.trunk.gpool == 2 and len(m.model.trunk.gpool_w) == 1
    with pytest.raises(SystemExit):
        main(["init-model", "pv", str(tmp_path / "e.json"), "--board", "9", "--filters", "8", "--layers", "5",
              "--gpool", "2"])
    assert "--residual" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main(["init-model", "pv", str(tmp_path / "e.json"), "--board", "9", "--filters", "8", "--layers", "5",
              "--residual", "--gpool", "3"])
    assert "valid choices" in capsys.readouterr().err
    assert not (tmp_path / "e.json").exists()


def test_flops_add_the_gates():
    assert _net(gpool=1).flops_per_position() - _net().flops_per_position() == 2 * (2 * 2 * F * F)
    assert _net(gpool=2).flops_per_position() - _net().flops_per_position() == 2 * 2 * F * F


# ----------------------------------------------------------------------------- trainer
def test_torch_trainer_step_moves_every_gate():
    from alphago_amd.train.engine import TorchPolicyValueTrainer

    net = _net(gpool=1, seed=10, live=True)
    tr = TorchPolicyValueTrainer(net, 4, lr=0.1, device="cpu")
    assert tr.fp.names[:10] == ["w0", "b0", "w1", "b1", "w2", "b2", "g2", "w3", "b3", "w4"] and tr.fp.names[10:12] == \
        ["b4", "g4"]
    before = [g.detach().clone() for g in net.trunk.gpool_w]
    rng = np.random.default_rng(0)
    planes = torch.from_numpy((rng.random((4, C0, S, S)) < 0.4).astype(np.uint8))
    moves = torch.from_numpy(rng.integers(0, S * S, 4).astype(np.int64))
    z = torch.tensor([1.0, -1.0, 1.0, -1.0])
    tr.step(planes, (moves, z))
    for b, g in zip(before, net.trunk.gpool_w):
        assert bool((b != g).all())
    # a net without gpool keeps its flat layout
    assert TorchPolicyValueTrainer(_net(), 4, lr=0.1, device="cpu").fp.names[:6] == ["w0", "b0", "w1", "b1", "w2", "b2"]
