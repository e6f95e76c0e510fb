"""The residual trunk of the dual net on the CPU: the block definition against a hand-written loop, the
depth rule, the ``pv_model`` spec (absent key by default, round trip when set), ``init-model pv
--residual``, ``split()``, the Fixup init and its identity, ``train-pv`` through the torch backend, and the
conditions of the integer oracles the GPU tests compare against (tests/residual_refs.py)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_refs as R
import residual_refs as RR
from test_pv_cpu import _planes, _pv, _selfplay_file


def _loop_forward(trunk, x):
    """Y[0] = relu(conv_0(x)); odd l: Y[l] = relu(conv_l(Y[l-1])); even l >= 2: Y[l] = relu(conv_l(Y[l-1]) + Y[l-2])."""
    Y = []
    for l in range(trunk.layers):
        z = F.conv2d(x if l == 0 else Y[l - 1], trunk.weights[l], trunk.biases[l], padding=trunk.widths[l] // 2)
        if l >= 2 and l % 2 == 0:
            z = z + Y[l - 2]
        Y.append(torch.relu(z))
    return Y


def _random_trunk(layers=5, filters=6, seed=3):
    from alphago_amd.models.nets import ConvStack

    tr = ConvStack(7, filters, layers, [5] + [3] * (layers - 1), residual=True)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for w, b in zip(tr.weights, tr.biases):
            w.uniform_(-0.4, 0.4, generator=g)
            b.uniform_(-0.2, 0.2, generator=g)
    return tr


def test_forward_torch_is_the_block_definition():
    from alphago_amd.models.nets import ConvStack

    tr = _random_trunk()
    assert tr.residual and [n for n, _ in tr.named_parameters()] == \
        [n for n, _ in ConvStack(7, 6, 5, [5, 3, 3, 3, 3]).named_parameters()]
    x = torch.rand(3, 7, 9, 9, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = _loop_forward(tr, x)[-1]
        got = tr.forward_torch(x)
        assert torch.equal(got, want)
        tr.residual = False  # the same parameters without the skips compute something else
        assert not torch.allclose(tr.forward_torch(x), want)


@pytest.mark.parametrize("layers,near", [(2, ("3",)), (4, ("3", "5")), (12, ("11", "13"))])
def test_even_depth_is_refused(layers, near):
    from alphago_amd.models.nets import ConvStack, PolicyValueNet

    with pytest.raises(ValueError, match="odd") as e:
        ConvStack(7, 6, layers, [5] + [3] * (layers - 1), residual=True)
    assert all(n in str(e.value) for n in near)
    with pytest.raises(ValueError, match="odd"):
        PolicyValueNet(49, 9, 8, layers, dense=16, residual=1)
    ConvStack(7, 6, layers, [5] + [3] * (layers - 1))  # plain stacks keep every depth


def test_arch_key_only_when_set_and_default_spec_bytes(tmp_path):
    from alphago_amd.features import VALUE_FEATURES
    from alphago_amd.models.nets import PolicyNet, PolicyValueNet, ValueNet

    assert "residual" not in PolicyValueNet(49, 9, 8, 3, dense=16).arch
    assert not PolicyValueNet(49, 9, 8, 3, dense=16).trunk.residual
    assert PolicyValueNet(49, 9, 8, 3, dense=16, residual=1).arch["residual"] == 1
    assert "residual" not in PolicyNet(48, 9, 8, 3).arch and "residual" not in ValueNet(49, 9, 8, 3).arch
    plain, res = PolicyValueNet(49, 9, 8, 3, dense=16), PolicyValueNet(49, 9, 8, 3, dense=16, residual=1)
    assert res.flops_per_position() == plain.flops_per_position()  # the adds are not MACs
    assert [(n, tuple(p.shape)) for n, p in res.named_parameters()] == \
        [(n, tuple(p.shape)) for n, p in plain.named_parameters()]
    js = str(tmp_path / "pv.json")
    _pv(layers=3, dense=16).save_model(js)
    with open(js) as f:
        text = f.read()
    assert text == ('{"pv_model": {"input_dim": 49, "board": 9, "filters_per_layer": 8, "layers": 3, "dense": 16}, '
                    '"feature_list": %s}' % json.dumps(list(VALUE_FEATURES)))


def test_json_and_weights_round_trip(tmp_path):
    from alphago_amd.models.policy import CNNPolicyValue

    pv = _pv(layers=5, dense=16, residual=1)
    js, wf = str(tmp_path / "pv.json"), str(tmp_path / "pv.hdf5")
    pv.save_model(js, wf)
    with open(js) as f:
        assert json.load(f)["pv_model"]["residual"] == 1
    back = CNNPolicyValue.load_model(js, device="cpu")
    assert back.model.trunk.residual and back.model.arch == pv.model.arch
    with torch.no_grad():  # the Fixup init zeroes the block ends: give the branches something to carry
        for l in (2, 4):
            pv.model.trunk.weights[l].uniform_(-0.3, 0.3, generator=torch.Generator().manual_seed(l))
    pv.save_weights(wf)
    back.load_weights(wf)
    x = _planes(4)
    p0, v0 = pv.forward(x)
    p1, v1 = back.forward(x)
    assert np.array_equal(p0, p1) and np.array_equal(v0, v1)
    plain = _pv(layers=5, dense=16)
    plain.load_weights(wf)  # same parameter layout; a different function
    assert not np.array_equal(plain.forward(x)[0], p0)


def test_init_model_residual(tmp_path, capsys):
    from alphago_amd.cli import main
    from alphago_amd.models.policy import CNNPolicyValue

    js = str(tmp_path / "m.json")
    assert main(["init-model", "pv", js, "--weights", str(tmp_path / "m.hdf5"), "--board", "9", "--filters", "8",
                 "--layers", "5", "--residual"]) == 0
    m = CNNPolicyValue.load_model(js, device="cpu")
    assert m.model.trunk.residual and m.model.arch["layers"] == 5 and m.model.arch["residual"] == 1
    with pytest.raises(SystemExit):
        main(["init-model", "pv", str(tmp_path / "e.json"), "--board", "9", "--filters", "8", "--layers", "4",
              "--residual"])
    err = capsys.readouterr().err
    assert "odd" in err and "3" in err and "5" in err
    for kind in ("policy", "value"):
        with pytest.raises(SystemExit):
            main(["init-model", kind, str(tmp_path / "p.json"), "--board", "9", "--layers", "5", "--residual"])
        assert "--residual" in capsys.readouterr().err
    assert not (tmp_path / "e.json").exists() and not (tmp_path / "p.json").exists()


def test_split_raises():
    pv = _pv(layers=3, residual=1)
    with pytest.raises(ValueError, match="residual"):
        pv.split()


def test_fixup_init_and_identity():
    """he_uniform_ on a residual trunk: block-first convs at He bound * n_blocks ** -0.5, block-last convs
    zero, stem and heads as on a plain net; every block is then the identity on its non-negative input."""
    from alphago_amd.models.nets import PolicyValueNet, he_uniform_

    L, Fl = 7, 8
    net = he_uniform_(PolicyValueNet(49, 9, Fl, L, dense=16, residual=1), generator=torch.Generator().manual_seed(4))
    plain = he_uniform_(PolicyValueNet(49, 9, Fl, L, dense=16), generator=torch.Generator().manual_seed(4))
    tr = net.trunk
    he3 = (6.0 / (Fl * 9)) ** 0.5
    with torch.no_grad():
        assert torch.equal(tr.weights[0], plain.trunk.weights[0])  # the stem: the plain draw
        for l in range(1, L):
            if l % 2 == 0:
                assert not tr.weights[l].any()
            else:
                m = float(tr.weights[l].abs().max())
                assert he3 * 3 ** -0.5 * 0.8 < m <= he3 * 3 ** -0.5
        assert float(net.head_w.abs().max()) <= (6.0 / Fl) ** 0.5 and net.head_w.abs().max() > 0.05
        assert all(not b.any() for b in tr.biases)
        x = torch.from_numpy(_planes(3)).float()
        stem = torch.relu(F.conv2d(x, tr.weights[0], tr.biases[0], padding=2))
        assert torch.equal(tr.forward_torch(x), stem)
        assert stem.any()


def test_train_pv_torch_backend_runs_an_epoch(tmp_path):
    from alphago_amd.cli import main
    from alphago_amd.models.policy import CNNPolicyValue

    pv = _pv(layers=5, residual=1)
    js = str(tmp_path / "pv.json")
    pv.save_model(js, str(tmp_path / "pv0.hdf5"))
    h5 = str(tmp_path / "selfplay.h5")
    assert _selfplay_file(h5, pv) == 12
    out = tmp_path / "out"
    assert main(["train-pv", js, h5, str(out), "--minibatch", "4", "--epochs", "1", "--backend", "torch",
                 "--train-val-test", "0.7", "0.3", "0", "--learning-rate", "0.01"]) == 0
    trained = CNNPolicyValue.load_model(js, device="cpu", weights_file=str(out / "weights.00000.hdf5"))
    assert trained.model.trunk.residual
    before = CNNPolicyValue.load_model(js, device="cpu")
    # the zero-initialised block ends receive gradient through the skip path and move
    assert not before.model.trunk.weights[2].any() and trained.model.trunk.weights[2].any()
    x = _planes(2)
    assert not np.array_equal(trained.forward(x)[0], before.forward(x)[0])


@pytest.mark.parametrize("case", RR.CASES, ids=R.case_id)
def test_oracle_conditions(case):
    """Every case of the GPU test keeps its sums exact and its sign tests sensitive to the skip."""
    share, flips, top = RR.fwd_conditions(case)
    assert 0.3 <= share <= 0.7 and flips >= RR.MIN_FLIPS and top <= R.MAX_ABS
    c = RR.fwd_case(case)
    assert 0 <= c["res"].min() and c["res"].max() <= RR.RES_MAX
    assert abs((c["res"][..., :R.real_channels(case)[1]] != 0).double().mean().item() - 0.5 * 32 / 33) < 0.02
    assert torch.equal(c["y"].double(), (c["pre"] + c["res"]).clamp_min(0))
    d = RR.dgrad_case(case)
    assert d["dx"].abs().max() <= R.MAX_ABS and set(d["res"].unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert torch.equal(d["dx"], torch.where(d["mask"], d["raw"] + d["res"], torch.zeros_like(d["raw"])))
    assert not torch.equal(d["dx"], R.dgrad_case(case)["dx"])
    buf = RR.res_buffer(c["res"])
    assert torch.isnan(buf[R.border_mask(case[1], case[0], 1, case[3])]).all()
    assert torch.equal(R.interior(buf, 1, case[0]).double(), c["res"])
