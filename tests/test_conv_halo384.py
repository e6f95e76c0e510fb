"""Tile 388: the production 384-pixel forward / bitmask-dgrad loop with the pixel rows staged once per
64-channel chunk (compact halo).  It keeps tile 386's K order, so every check against 386 is bitwise."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = 7.0

# S, B, Cin, Cout, Pin
CASES = [
    (19, 1, 192, 192, 1),   # M = 361 < 384: one partial tile, halo indices clamped at both ends
    (19, 3, 192, 192, 1),   # M = 1083: tile 1 starts mid-row of board 1, halo crosses boards, partial last tile
    (9, 11, 192, 192, 1),   # halo spans five boards, G = 10
    (13, 5, 128, 192, 2),   # two chunks (one halo-buffer swap), input pad larger than the tap radius
    (19, 3, 64, 384, 1),    # a single chunk (no prefetch), blockIdx.y = 1
    (19, 3, 256, 192, 1),   # four chunks (halo-buffer parity wraps)
]


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


def _bf(x):
    return x.to(torch.bfloat16).float()


def _rel_err(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


def _sentinel(ops, B, S, C, dev):
    return torch.full_like(ops.padded_empty(B, S, 1, C, dev), SENTINEL)


def _border_mask(B, S, C, dev):
    m = torch.ones(B, S + 2, S + 2, C, dtype=torch.bool, device=dev)
    m[:, 1:S + 1, 1:S + 1] = False
    return m


def _run_case(ops, dev, S, B, Cin, Cout, Pin):
    """One Cin -> Cout layer geometry on tiles 386 and 388: the forward (bias + ReLU, writing the bitmask)
    and a bitmask dgrad of the same kernel shape -- the transposed pack of a (Cin, Cout, 3, 3) weight,
    Cin-wide gradient in, Cout-wide gradient out, masked by the forward's bits."""
    g = torch.Generator(device="cpu").manual_seed(1000 * S + 10 * B + Cin)
    x = _bf(torch.randn(B, Cin, S, S, generator=g)).to(dev)
    w = _bf(torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).to(dev)
    b = (torch.randn(Cout, generator=g) * 0.1).to(dev)
    dz = _bf(torch.randn(B, Cin, S, S, generator=g)).to(dev)
    w2 = _bf(torch.randn(Cin, Cout, 3, 3, generator=g) * 0.05).to(dev)
    xp = ops.padded_empty(B, S, Pin, Cin, dev)
    xp[:, Pin:Pin + S, Pin:Pin + S] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    dzp = ops.padded_empty(B, S, Pin, Cin, dev)
    dzp[:, Pin:Pin + S, Pin:Pin + S] = dz.permute(0, 2, 3, 1).to(torch.bfloat16)
    wf = ops.packed_weight_like(w, Cin, Cout)
    w2f = ops.packed_weight_like(w2, Cout, Cin)
    w2d = ops.packed_weight_like(w2, Cout, Cin, True)
    ops.pack_weights([w.contiguous()], [wf])
    ops.pack_weights([w2.contiguous()], [w2f], [w2d])
    words = B * (S + 2) ** 2 * ops.mbits_words(Cout)
    out, dx = {}, {}
    for tile in (386, 388):
        y = _sentinel(ops, B, S, Cout, dev)
        mb = torch.full((words,), -1, dtype=torch.int32, device=dev)
        ops.conv_fwd(xp, wf, b, y, 3, S, Pin, 1, mbits=mb, tile=tile)
        d = _sentinel(ops, B, S, Cout, dev)
        ops.conv_fwd(dzp, w2d, None, d, 3, S, Pin, 1, mode=ops.MODE_MASKBITS, mbits=mb, tile=tile)
        out[tile] = (y, mb)
        dx[tile] = d
    torch.cuda.synchronize()
    ref_y = F.relu(F.conv2d(x, w, b, padding=1))
    ref_dx = torch.nn.grad.conv2d_input((B, Cout, S, S), w2, dz, padding=1) * (ops.from_padded(out[386][0], 1) > 0)
    return out, dx, ref_y, ref_dx


_cache = {}


def _case(ops, dev, case):
    if case not in _cache:
        _cache[case] = _run_case(ops, dev, *case)
    return _cache[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%d-B%d-%dto%d-P%d" % c)
def test_halo384_bitwise_equals_tile386(ops, cuda_device, case):
    S, B, Cin, Cout, Pin = case
    out, dx, _, _ = _case(ops, cuda_device, case)
    y6, mb6 = out[386][:2]
    y8, mb8 = out[388][:2]
    assert torch.equal(y8, y6)
    assert torch.equal(mb8, mb6)
    assert torch.equal(dx[388], dx[386])
    # interior written, border untouched
    assert (y8[_border_mask(B, S, Cout, cuda_device)] == SENTINEL).all()
    assert (dx[388][_border_mask(B, S, Cout, cuda_device)] == SENTINEL).all()
    assert (mb8.view(B, S + 2, S + 2, -1)[:, 1:S + 1, 1:S + 1] != -1).any()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%d-B%d-%dto%d-P%d" % c)
def test_halo384_matches_fp32_reference(ops, cuda_device, case):
    out, dx, ref_y, ref_dx = _case(ops, cuda_device, case)
    assert _rel_err(ops.from_padded(out[388][0], 1), ref_y) < 1e-2
    assert _rel_err(ops.from_padded(dx[388], 1), ref_dx) < 1e-2
    assert (ops.from_padded(dx[388], 1) != 0).any()


def _train(dev, tile):
    from alphago_amd.models.nets import PolicyNet
    from alphago_amd.train.engine import HipPolicyTrainer

    torch.manual_seed(0)
    B = 4
    tr = HipPolicyTrainer(PolicyNet(48, filters_per_layer=192, layers=3), B, lr=0.01, device=dev, conv_tile=tile)
    g = torch.Generator().manual_seed(5)
    for _ in range(2):
        planes = torch.randint(0, 2, (B, 48, 19, 19), dtype=torch.uint8, generator=g).to(dev)
        tgt = torch.randint(0, 361, (B,), dtype=torch.int32, generator=g).to(dev)
        tr.step(planes, tgt)
    torch.cuda.synchronize()
    return tr.fp.flat.detach().cpu().clone()


def test_halo384_training_bitwise_equals_tile386(cuda_device):
    p6 = _train(cuda_device, 386)
    p8 = _train(cuda_device, 388)
    assert torch.isfinite(p8).all()
    assert torch.equal(p8, p6)


_DEBUG_CHILD = r"""
import torch
from alphago_amd import ops
ops.load(build_if_missing=False)
assert torch.ops.alphago_amd.is_debug_build()
dev = torch.device("cuda:0")
torch.manual_seed(0)
S, B, Cin, Cout = 19, 3, 192, 192
x = torch.randn(B, Cin, S, S, device=dev)
w = torch.randn(Cout, Cin, 3, 3, device=dev) * 0.05
b = torch.randn(Cout, device=dev) * 0.1
xp = ops.to_padded(x, 1)
wf = ops.packed_weight_like(w, Cin, Cout); wd = ops.packed_weight_like(w, Cin, Cout, True)
ops.pack_weights([w.contiguous()], [wf], [wd])
res = {}
for tile in (386, 388):
    y = ops.padded_empty(B, S, 1, Cout, dev)
    mb = torch.zeros(B * (S + 2) ** 2 * ops.mbits_words(Cout), dtype=torch.int32, device=dev)
    ops.conv_fwd(xp, wf, b, y, 3, S, 1, 1, mbits=mb, tile=tile)      # bounds-checked forward
    d = ops.padded_empty(B, S, 1, Cin, dev)
    ops.conv_fwd(y, wd, None, d, 3, S, 1, 1, mode=ops.MODE_MASKBITS, mbits=mb, tile=tile)  # and dgrad
    res[tile] = (y, mb, d)
torch.cuda.synchronize()
assert all(torch.equal(p, q) for p, q in zip(res[386], res[388]))
assert (res[388][0] != 0).any() and (res[388][2] != 0).any()
print("DEBUG-OK")
"""


def test_halo384_debug_build(cuda_device):
    """The AGK_DEBUG library runs tile 388's forward and bitmask dgrad (M = 1083: clamped halo rows at
    both ends, a partial last tile) without a bounds violation -- every debug op raises on one."""
    from alphago_amd import _build

    assert os.path.exists(_build.hip_path("debug")), "debug library not built"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ALPHAGO_AMD_KERNELS="debug", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _DEBUG_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEBUG-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
