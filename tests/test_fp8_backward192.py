"""All-fp8 backward at the policy width (192): the fp8 wgrad's 192 x 96 tile, conv_dgrad_fp8_bits on the
192-wide tile, the bitmask dgrad's e5m2 copy at 192, and the opt-in switch of the trainer.  The kernel
tests are the 160-wide ones of tests/test_conv160.py at 192 with the same tolerances (the maths is
identical); references are torch ops on the dequantised operands, evaluated in fp64."""
import copy
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 3


def _bf(x):
    return x.to(torch.bfloat16).float()


def _rel_err(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


def _wgrad_case(ops, dev, B, S, C, Cp=192, seed=11):
    """Operands as tests/test_conv160.py::test_conv_wgrad_fp8_160 builds them, and the fp64 references."""
    torch.manual_seed(seed)
    x = torch.relu(torch.randn(B, C, S, S, device=dev)) * 2.0
    dz = torch.randn(B, C, S, S, device=dev) * 1e-3
    ex = ops.fp8_exponent(float(x.abs().max()), margin=0)
    eg = ops.fp8_exponent(float(dz.abs().max()), margin=0) + 7
    x8q = (x * 2.0 ** ex).clamp(-448, 448).to(torch.float8_e4m3fn)
    dz8q = (dz * 2.0 ** eg).clamp(-57344, 57344).to(torch.float8_e5m2)
    xq = x8q.double() * 2.0 ** -ex
    dzq = dz8q.double() * 2.0 ** -eg
    x8 = torch.zeros((B, S + 2, S + 2, Cp), dtype=torch.uint8, device=dev)
    x8[:, 1:S + 1, 1:S + 1, :C] = x8q.view(torch.uint8).permute(0, 2, 3, 1)
    dz8 = torch.zeros_like(x8)
    dz8[:, 1:S + 1, 1:S + 1, :C] = dz8q.view(torch.uint8).permute(0, 2, 3, 1)
    ref_w = torch.nn.grad.conv2d_weight(xq, (C, C, K, K), dzq, padding=1)
    ref_b = dzq.sum(dim=(0, 2, 3))
    xs = torch.tensor([127 - ex], dtype=torch.int32, device=dev)
    gs = torch.tensor([127 - eg], dtype=torch.int32, device=dev)
    gm = torch.tensor([2.0 ** eg], device=dev)
    return x8, dz8, xs, gs, gm, ref_w, ref_b, dzq


def _run_wgrad(ops, dev, x8, dz8, xs, gs, gm, S, amax=None):
    B, Cp = x8.shape[0], x8.shape[3]
    ns = ops.wgrad_fp8_nsplit(B * S * S, K, width=Cp)
    slab = torch.full((ns, K * K, Cp, Cp), float("nan"), device=dev)
    dbs = torch.full((ns, Cp), float("nan"), device=dev)
    ops.conv_wgrad_fp8(x8, dz8, slab, dbs, xs, gs, gm, K, S, 1, 1, amax=amax)
    return slab, dbs


# (1, 9): M = 81, less than one 128-pixel step; (5, 9): the step-to-step row / column carry on a small
# board; (3, 19), (7, 19, 176): one step per split, real channels below the padded width; (24, 19): 68
# steps on 28 splits of 3 -- several steps per split (both LDS buffers), a ragged last split, empty splits
@pytest.mark.parametrize("B,S,C", [(1, 9, 192), (5, 9, 192), (3, 19, 192), (7, 19, 176), (24, 19, 192)])
def test_conv_wgrad_fp8_192(ops, cuda_device, B, S, C):
    """fp8 wgrad at 192 vs fp64 conv2d_weight of the dequantised operands; the NaN-filled slabs catch
    any tile a split failed to write; max |dZ| from the e5m2 bytes is exact; two calls agree bitwise."""
    Cp = 192
    x8, dz8, xs, gs, gm, ref_w, ref_b, dzq = _wgrad_case(ops, cuda_device, B, S, C)
    amax = ops.fp8_amax_buffer(1, cuda_device)[0]
    slab, dbs = _run_wgrad(ops, cuda_device, x8, dz8, xs, gs, gm, S, amax=amax)
    slab2, dbs2 = _run_wgrad(ops, cuda_device, x8, dz8, xs, gs, gm, S)
    gw = torch.zeros(Cp, Cp, K, K, device=cuda_device)
    gb = torch.zeros(Cp, device=cuda_device)
    ops.conv_wgrad_reduce(slab, dbs, gw, gb, 1.0, 0.0)
    torch.cuda.synchronize()
    assert torch.isfinite(slab).all() and torch.isfinite(dbs).all()
    assert torch.isfinite(gw).all() and torch.isfinite(gb).all()
    ew, eb = _rel_err(gw[:C, :C].double(), ref_w), _rel_err(gb[:C].double(), ref_b)
    print("wgrad 192 (B, S, C) =", (B, S, C), "rel err w, b:", ew, eb)
    assert ew < 2e-3
    assert eb < 2e-3
    # padded channels: rows / columns C..191 of the gradient are exactly zero
    assert gw[C:].abs().sum() == 0 and gw[:, C:].abs().sum() == 0 and gb[C:].abs().sum() == 0
    # a decoded e5m2 byte divided by a power of two: exact
    assert amax.view(torch.float32).max().item() == dzq.abs().max().item()
    assert torch.equal(slab, slab2) and torch.equal(dbs, dbs2)  # deterministic: no atomics on the gradients


@pytest.mark.parametrize("cout,cin", [(384, 384), (192, 160)])
def test_conv_wgrad_fp8_refuses_other_widths(ops, cuda_device, cout, cin):
    B, S = 1, 9
    x8 = torch.zeros((B, S + 2, S + 2, cin), dtype=torch.uint8, device=cuda_device)
    dz8 = torch.zeros((B, S + 2, S + 2, cout), dtype=torch.uint8, device=cuda_device)
    slab = torch.zeros((1, 9, cout, cin), device=cuda_device)
    dbs = torch.zeros((1, cout), device=cuda_device)
    one = torch.tensor([127], dtype=torch.int32, device=cuda_device)
    with pytest.raises(RuntimeError, match="160 -> 160 and 192 -> 192"):
        ops.conv_wgrad_fp8(x8, dz8, slab, dbs, one, one, torch.ones(1, device=cuda_device), K, S, 1, 1)


def _forward_bits(ops, dev, B, S, C, Cp, bias_scale=0.1):
    """A real bf16 forward's ReLU' bitmask and its output."""
    xin = _bf(torch.randn(B, C, S, S, device=dev))
    w0 = _bf(torch.randn(C, C, K, K, device=dev) * 0.05)
    wp0 = ops.packed_weight_like(w0, Cp, Cp)
    ops.pack_weights([w0.contiguous()], [wp0])
    yprev = ops.padded_empty(B, S, 1, Cp, dev)
    mbits = torch.zeros(B * (S + 2) ** 2 * ops.mbits_words(Cp), dtype=torch.int32, device=dev)
    ops.conv_fwd(ops.to_padded(xin, 1, Cp), wp0, torch.randn(Cp, device=dev) * bias_scale, yprev, K, S, 1, 1,
                 mbits=mbits)
    return yprev, mbits


@pytest.mark.parametrize("B,outs", [(3, "fp8"), (5, "bf16"), (2, "both")])
@pytest.mark.parametrize("C", [192, 176])
def test_conv_dgrad_fp8_bits_192(ops, cuda_device, C, B, outs):
    """conv_dgrad_fp8_bits on the 192-wide tile: e5m2 dZ x transposed e4m3 weights, ReLU' from a real
    forward's bitmask, e5m2 and/or bf16 outputs vs fp64 conv2d_input of the dequantised operands."""
    torch.manual_seed(16)
    S, Cp = 19, 192
    yprev, mbits = _forward_bits(ops, cuda_device, B, S, C, Cp)
    dz = torch.randn(B, C, S, S, device=cuda_device) * 1e-3
    w = torch.randn(C, C, K, K, device=cuda_device) * 0.05
    eg = ops.fp8_exponent(float(dz.abs().max()), margin=0) + 7
    ew = ops.fp8_exponent(float(w.abs().max()), margin=0)
    w8t = torch.zeros(ops.fp8_weight_shape(K, Cp, Cp), dtype=torch.uint8, device=cuda_device)
    ops.pack_weights_fp8_multi([w], [w8t], torch.tensor([2.0 ** ew], device=cuda_device), [0], [1])
    dz8q = (dz * 2.0 ** eg).clamp(-57344, 57344).to(torch.float8_e5m2)
    dz8 = torch.zeros((B, S + 2, S + 2, Cp), dtype=torch.uint8, device=cuda_device)
    dz8[:, 1:S + 1, 1:S + 1, :C] = dz8q.view(torch.uint8).permute(0, 2, 3, 1)
    dzq = dz8q.double() * 2.0 ** -eg
    wq = (w * 2.0 ** ew).clamp(-448, 448).to(torch.float8_e4m3fn).double() * 2.0 ** -ew
    ymask = ops.from_padded(yprev, 1)[:, :C] > 0
    ref = torch.nn.grad.conv2d_input((B, C, S, S), wq, dzq, padding=K // 2) * ymask
    scales = torch.tensor([127 - eg, 127 - ew], dtype=torch.int32, device=cuda_device)
    eo = ops.fp8_exponent(float(ref.abs().max()), margin=0) + 7
    amax = ops.fp8_amax_buffer(1, cuda_device)[0]
    dx = ops.padded_empty(B, S, 1, Cp, cuda_device) if outs in ("bf16", "both") else None
    dx8 = torch.zeros_like(dz8) if outs in ("fp8", "both") else None
    ops.conv_dgrad_fp8_bits(dz8, w8t, mbits, scales, torch.tensor([2.0 ** eo], device=cuda_device), K, S,
                            y_bf16=dx, y_fp8=dx8, amax=amax)
    torch.cuda.synchronize()
    if dx is not None:
        out = ops.from_padded(dx, 1)
        assert _rel_err(out[:, :C].double(), ref) < 1e-2
        assert out[:, C:].abs().sum() == 0
        assert dx[:, 0].abs().sum() == 0  # borders untouched
    if dx8 is not None:
        got = dx8[:, 1:S + 1, 1:S + 1, :C].view(torch.float8_e5m2).double().permute(0, 3, 1, 2) * 2.0 ** -eo
        # e5m2 keeps 2 mantissa bits: at most half a step (12.5 % of the value) from the exact result
        assert _rel_err(got, ref) < 0.13
        assert (got - ref).abs().mean().item() < 0.1 * ref.abs().mean().item()
        assert dx8[:, 0].sum() == 0 and dx8[:, 1:S + 1, 1:S + 1, C:].sum() == 0
    assert abs(amax.view(torch.float32).max().item() - ref.abs().max().item()) <= 1e-2 * ref.abs().max().item()


# tile 0: the engine's default (its choice for this pixel count); 388 / 386: the large-batch default
# (compact-halo 384-pixel tile) and the tile it replaced, forced at this small batch
@pytest.mark.parametrize("tile", [0, 388, 386])
def test_dgrad_bits_bf8_copy_192(ops, cuda_device, tile):
    """The bitmask dgrad's e5m2 copy at 192: the bf16 output is bit-equal to the plain bitmask dgrad,
    the copy is e5m2(dx * scale) of the fp32 result, and the amax slots hold max |dx|."""
    torch.manual_seed(12)
    B, S, C, Cp = 4, 19, 192, 192
    y, mbits = _forward_bits(ops, cuda_device, B, S, C, Cp, bias_scale=0.0)
    w = _bf(torch.randn(C, C, K, K, device=cuda_device) * 0.05)
    wf, wd = ops.packed_weight_like(w, Cp, Cp), ops.packed_weight_like(w, Cp, Cp, transposed=True)
    ops.pack_weights([w], [wf], [wd])
    dz = ops.to_padded(_bf(torch.randn(B, C, S, S, device=cuda_device) * 1e-3), 1, Cp)
    dx = ops.padded_empty(B, S, 1, Cp, cuda_device)
    dx8 = torch.zeros(dx.shape, dtype=torch.uint8, device=cuda_device)
    amax = ops.fp8_amax_buffer(1, cuda_device)[0]
    sc = torch.tensor([2.0 ** 20], device=cuda_device)
    ops.conv_dgrad_bits_bf8(dz, wd, dx, mbits, dx8, sc, K, S, amax=amax, tile=tile)
    ref = ops.padded_empty(B, S, 1, Cp, cuda_device)
    ops.conv_fwd(dz, wd, None, ref, K, S, 1, 1, mode=ops.MODE_MASKBITS, mbits=mbits, tile=tile)
    torch.cuda.synchronize()
    assert torch.equal(dx, ref)  # the bf16 output is unchanged by the extra copy
    assert dx8.any()  # the tile's epilogue wrote the copy
    q = (dx.float() * 2.0 ** 20).clamp(-57344, 57344).to(torch.float8_e5m2).view(torch.uint8)
    assert (q != dx8).float().mean().item() < 0.02  # fp32 vs bf16-rounded source: rare 1-ulp differences
    deq = dx8.view(torch.float8_e5m2).float() * 2.0 ** -20
    assert _rel_err(deq, dx.float()) < 0.13
    mx = dx.float().abs().max().item()
    assert abs(amax.view(torch.float32).max().item() - mx) <= 1e-2 * mx


# ------------------------------------------------------------------ engine
def _planes(n, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2, (n, C, 19, 19), dtype=torch.uint8, generator=g)


ARMS = [(False, False), (False, True), (True, True)]  # (fp8_dgrad, fp8_wgrad)


@pytest.fixture(scope="module")
def policy_arm_grads(cuda_device):
    """Per-arm gradients of the fp8 policy trainer (4 x 192, B = 32) on one batch: the second backward
    (the first calibrates the activation and gradient scales), all arms on the same fp8 forward."""
    from alphago_amd.models.nets import PolicyNet
    from alphago_amd.train.engine import HipPolicyTrainer

    torch.manual_seed(4)
    dev = cuda_device
    B, L = 32, 4
    net = PolicyNet(48, filters_per_layer=192, layers=L)
    planes = _planes(B, 48, seed=11).to(dev)
    tgt = torch.randint(0, 361, (B,), dtype=torch.int32, device=dev)
    out = {}
    for dg, wg in ARMS:
        t = HipPolicyTrainer(copy.deepcopy(net), B, lr=0.0, device=dev, precision="fp8", fp8_dgrad=dg, fp8_wgrad=wg)
        assert (t.fp8_dgrad, t.fp8_wgrad) == (dg, wg)
        t.compute_grads(planes, tgt)
        t.compute_grads(planes, tgt)
        torch.cuda.synchronize()
        out[(dg, wg)] = ({n: t.fp.grad_views[n].double().flatten().clone() for n in t.fp.names},
                         t.gscales8.clone().cpu())
    return L, out


def _cos_ratio(a, b):
    return (round(torch.nn.functional.cosine_similarity(a, b, dim=0).item(), 4), round((a.norm() / b.norm()).item(), 4))


@pytest.mark.parametrize("arm", ARMS[1:])
def test_policy_fp8_backward_matches_bf16_backward(cuda_device, policy_arm_grads, arm):
    """fp8 wgrad, and fp8 wgrad + dgrad, on the 4 x 192 policy trunk vs the bf16 backward of the same fp8
    forward: the project's limits for that comparison (cosine >= 0.95 and norm ratio 0.8-1.25 per weight,
    cosine > 0.85 per bias: sums of e5m2 gradients over 32 boards); gradient exponents calibrated."""
    L, got = policy_arm_grads
    ref, (g8, gsc) = got[(False, False)][0], got[arm]
    res = {n: _cos_ratio(g8[n], ref[n]) for n in ["w%d" % l for l in range(L)] + ["b%d" % l for l in range(L)]}
    print("arm (dgrad, wgrad) =", arm, "per-layer (cosine, norm ratio):", res)
    for l in range(L):
        cos, ratio = res["w%d" % l]
        assert cos >= 0.95 and 0.8 < ratio < 1.25, (arm, l, cos, ratio)
        assert res["b%d" % l][0] > 0.85, (arm, l, res["b%d" % l])
    assert (gsc[1:, 0] != 127).all()


def test_policy_fp8_backward_trains(cuda_device):
    """12 all-fp8 steps at lr 0.05 bring the loss on the memorised batch below 0.9 x its start."""
    from alphago_amd.models.nets import PolicyNet
    from alphago_amd.train.engine import HipPolicyTrainer

    torch.manual_seed(0)
    B = 32
    net = PolicyNet(48, filters_per_layer=192, layers=4)
    planes = _planes(B, 48, seed=5).to(cuda_device)
    tgt = torch.randint(0, 361, (B,), dtype=torch.int32, device=cuda_device)
    t = HipPolicyTrainer(net, B, lr=0.05, device=cuda_device, precision="fp8", fp8_dgrad=True, fp8_wgrad=True)
    assert t.fp8_wgrad and t.fp8_dgrad
    l0 = t.evaluate(planes, tgt)[0].item()
    for _ in range(12):
        t.step(planes, tgt)
    l1 = t.evaluate(planes, tgt)[0].item()
    print("loss", l0, "->", l1)
    assert l1 < 0.9 * l0
    assert (t.gscales8[1:, 0] != 127).all()


def test_policy_fp8_overlap_backward_matches_serial(cuda_device):
    """All-fp8 policy training with the wgrad on its own stream gives the serial backward's weights and
    scale state bit for bit (as test_fp8_overlap_backward_matches_serial at the value width)."""
    from alphago_amd.models.nets import PolicyNet
    from alphago_amd.train.engine import HipPolicyTrainer

    torch.manual_seed(2)
    B = 64
    net = PolicyNet(48, filters_per_layer=192, layers=4)
    nets = [net, copy.deepcopy(net)]
    planes = _planes(B, 48, seed=9).to(cuda_device)
    tgt = torch.randint(0, 361, (B,), dtype=torch.int32, device=cuda_device)
    trs = [HipPolicyTrainer(n, B, lr=0.01, device=cuda_device, precision="fp8", overlap=ov, fp8_dgrad=True,
                            fp8_wgrad=True) for n, ov in zip(nets, (False, True))]
    for _ in range(4):
        for t in trs:
            t.step(planes, tgt)
    torch.cuda.synchronize()
    a, b = trs
    assert torch.equal(a.fp.flat, b.fp.flat)
    assert torch.equal(a.fp.grad, b.fp.grad)
    assert torch.equal(a.gscales8, b.gscales8) and torch.equal(a.gamax8, b.gamax8)


@pytest.mark.parametrize("env", [None, "1"])
def test_policy_fp8_default_keeps_bf16_backward(cuda_device, monkeypatch, env):
    """Without fp8_* arguments a 192-wide fp8 trainer keeps the bf16 backward, whatever the environment."""
    from alphago_amd.models.nets import PolicyNet
    from alphago_amd.train.engine import HipPolicyTrainer

    if env is None:
        monkeypatch.delenv("ALPHAGO_AMD_FP8_WGRAD", raising=False)
    else:
        monkeypatch.setenv("ALPHAGO_AMD_FP8_WGRAD", env)
    t = HipPolicyTrainer(PolicyNet(48, filters_per_layer=192, layers=2), 4, lr=0.0, device=cuda_device,
                         precision="fp8")
    assert t.fp8_wgrad is False and t.fp8_dgrad is False
