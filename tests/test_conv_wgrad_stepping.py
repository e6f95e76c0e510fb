"""The stepped staging addresses of the split-K wgrad (wgrad_tile): a lane's pixel is split into
(board, row, column) once per workgroup and then advanced 32 pixels per stage by compares and adds.

The cases walk many stages across many row and board wraps inside one split, which the cases of
tests/test_conv_exact.py (M <= 1083) do not.  Integer operands (conv_refs.wgrad_case): every product and
partial sum is exact in fp32, so grad_w and grad_b after conv_wgrad_reduce are compared with
``torch.equal`` against the fp64 oracle, whatever the split count; the oracle asserts its own exactness
bound (M x 16 < 2^24).  Slabs and gradients start as NaN."""
import os
import subprocess
import sys

import pytest
import torch

import conv_refs as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# (S, B, Cin, Cout, K, Pin)
CASES = [
    (9, 40, 192, 192, 3, 1),   # M = 3240; 32 = 3 * 9 + 5: a step crosses 3 or 4 rows, a board wraps every 2.5 steps
    (13, 12, 192, 192, 3, 1),  # M = 2028, 13 x 13 boards
    (19, 6, 192, 192, 3, 1),   # M = 2166, 19 x 19 boards
    (19, 6, 64, 192, 5, 2),    # the 48-plane tap-merged first-layer kernel
    (9, 20, 160, 160, 3, 1),   # value width
    (9, 32, 64, 64, 3, 1),     # M = 2592 = 81 x 32: no tail
    (19, 25, 64, 64, 3, 1),    # M = 9025 = 282 x 32 + 1: a one-pixel tail stage
]
SPLITS = ["1", "3", "7", "auto"]  # 7 starts ranges mid-board and mid-row
SMALL_PLAN_CASES = [c for c in CASES if c[4] == 3 and c[2] % 64 == 0 and c[3] % 64 == 0]
DIRECT_CASES = [CASES[0], CASES[3]]


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


_dev_cache = {}


def _setup(dev, case):
    if case not in _dev_cache:
        c = R.wgrad_case(case)
        Pin = case[5]
        _dev_cache[case] = {"xp": R.place(c["x"], Pin, BF).to(dev), "dzp": R.place(c["dz"], 1, BF).to(dev),
                            "dw": c["dw"].float().to(dev), "db": c["db"].float().to(dev)}
    return _dev_cache[case]


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _thin(case):
    ci = R.real_channels(case)[0]
    return ci if case[2] == 64 and ci < 64 else 0


def _run(ops, dev, case, ns, variant=0):
    S, B, Cin, Cout, K, Pin = case
    s = _setup(dev, case)
    slab, dbs = _nan((ns, K * K, Cout, Cin), dev), _nan((ns, Cout), dev)
    ops.conv_wgrad(s["xp"], s["dzp"], slab, dbs, K, S, Pin, 1, cin_real=_thin(case), variant=variant)
    ci, co = R.real_channels(case)
    gw, gb = _nan((co, ci, K, K), dev), _nan((co,), dev)
    ops.conv_wgrad_reduce(slab, dbs, gw, gb, 1.0, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(gw, s["dw"])
    assert torch.equal(gb, s["db"])
    return slab, dbs


def _nsplit(ops, case, split):
    S, B, K = case[0], case[1], case[4]
    return ops.wgrad_splits(B * S * S, K * K) if split == "auto" else int(split)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_stepping_slab_and_reduce(ops, cuda_device, case, split):
    _run(ops, cuda_device, case, _nsplit(ops, case, split))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", SMALL_PLAN_CASES, ids=R.case_id)
def test_stepping_small_plan(ops, cuda_device, case, split):
    """The small-batch plan (64 x 64 tiles, tap-merged kernel rows)."""
    _run(ops, cuda_device, case, _nsplit(ops, case, split), variant=ops.WGRAD_SMALL)


def test_stepping_empty_splits_write_zeros(ops, cuda_device):
    """M = 361 is 12 stages: with 16 splits the last four have none and must write zeros."""
    case = (19, 1, 192, 192, 3, 1)
    slab, dbs = _run(ops, cuda_device, case, 16)
    assert (slab[12:] == 0).all() and (dbs[12:] == 0).all()
    assert (slab[:12] != 0).any()


@pytest.mark.parametrize("split", ["3", "plan"])
def test_division_path_160_filters_48_planes(ops, cuda_device, split):
    """160 filters over 48 real planes of 64 (5x5 tap-merged rows, 48-wide c tile): the instantiation
    that keeps the per-stage division (no register room for the walk at its two workgroups per CU).
    Own integer data (conv_refs has no such case), same exactness argument: M x 16 = 23104 < 2^24."""
    dev = cuda_device
    S, B, K, Pin, ci, co = 19, 4, 5, 2, 48, 152
    g = torch.Generator(device="cpu").manual_seed(160048)
    x = torch.randint(-4, 5, (B, ci, S, S), generator=g).double()
    dz = torch.randint(-4, 5, (B, co, S, S), generator=g).double()
    dw = torch.nn.grad.conv2d_weight(x, (co, ci, K, K), dz, padding=K // 2)
    db = dz.sum(dim=(0, 2, 3))
    xp = R.place(R.nhwc(x, 64), Pin, BF).to(dev)
    dzp = R.place(R.nhwc(dz, 160), 1, BF).to(dev)
    ns = ops.wgrad_nsplit(B * S * S, 160, 64, K, ci) if split == "plan" else int(split)
    slab, dbs = _nan((ns, K * K, 160, 64), dev), _nan((ns, 160), dev)
    ops.conv_wgrad(xp, dzp, slab, dbs, K, S, Pin, 1, cin_real=ci)
    gw, gb = _nan((co, ci, K, K), dev), _nan((co,), dev)
    ops.conv_wgrad_reduce(slab, dbs, gw, gb, 1.0, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(gw.cpu().double(), dw) and torch.equal(gb.cpu().double(), db)


@pytest.mark.parametrize("ksub", [1, 2, 4, 8])
@pytest.mark.parametrize("case", DIRECT_CASES, ids=R.case_id)
def test_stepping_direct(ops, cuda_device, case, ksub):
    """The split-free kernel: KSUB sub-steps per stage share the stepping."""
    S, B, Cin, Cout, K, Pin = case
    ci, co = R.real_channels(case)
    assert ops.wgrad_direct_supported(Cout, Cin, ci, K)
    s = _setup(cuda_device, case)
    gw, gb = _nan((co, ci, K, K), cuda_device), _nan((co,), cuda_device)
    ops.conv_wgrad_direct(s["xp"], s["dzp"], gw, gb, K, S, Pin, 1, ksub=ksub)
    torch.cuda.synchronize()
    assert torch.equal(gw, s["dw"]) and torch.equal(gb, s["db"])


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=R.case_id)
def test_stepping_deterministic(ops, cuda_device, case):
    """Two launches on float data write the same slab bytes."""
    dev = cuda_device
    S, B, Cin, Cout, K, Pin = case
    g = torch.Generator(device="cpu").manual_seed(1234 + S + B)
    x = torch.zeros(B, S + 2 * Pin, S + 2 * Pin, Cin, dtype=BF)
    x[:, Pin:Pin + S, Pin:Pin + S, :R.real_channels(case)[0]] = torch.randn(
        B, S, S, R.real_channels(case)[0], generator=g).to(BF)
    dz = torch.zeros(B, S + 2, S + 2, Cout, dtype=BF)
    dz[:, 1:1 + S, 1:1 + S] = torch.randn(B, S, S, Cout, generator=g).to(BF)
    x, dz = x.to(dev), dz.to(dev)
    ns = 7
    outs = []
    for _ in range(2):
        slab, dbs = _nan((ns, K * K, Cout, Cin), dev), _nan((ns, Cout), dev)
        ops.conv_wgrad(x, dz, slab, dbs, K, S, Pin, 1, cin_real=_thin(case))
        torch.cuda.synchronize()
        outs.append((slab, dbs))
    cols = _thin(case) or Cin  # the thin kernel leaves the slab columns above cin_real unwritten
    a, b = outs
    assert torch.equal(a[0][..., :cols].view(torch.int32), b[0][..., :cols].view(torch.int32))
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.isfinite(a[0][..., :cols]).all() and torch.isfinite(a[1]).all()


_DEBUG_CHILD = r"""
import torch
import conv_refs as R
from alphago_amd import ops
ops.load(build_if_missing=False)
assert torch.ops.alphago_amd.is_debug_build()
dev = torch.device("cuda:0")
BF = torch.bfloat16
for case, ns in (((9, 40, 192, 192, 3, 1), 7), ((19, 6, 64, 192, 5, 2), 3)):
    S, B, Cin, Cout, K, Pin = case
    c = R.wgrad_case(case)
    ci, co = R.real_channels(case)
    xp, dzp = R.place(c["x"], Pin, BF).to(dev), R.place(c["dz"], 1, BF).to(dev)
    slab = torch.full((ns, K * K, Cout, Cin), float("nan"), device=dev)
    dbs = torch.full((ns, Cout), float("nan"), device=dev)
    ops.conv_wgrad(xp, dzp, slab, dbs, K, S, Pin, 1, cin_real=ci if ci < Cin and Cin == 64 else 0)
    gw = torch.full((co, ci, K, K), float("nan"), device=dev)
    gb = torch.full((co,), float("nan"), device=dev)
    ops.conv_wgrad_reduce(slab, dbs, gw, gb, 1.0, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(gw.cpu().double(), c["dw"]) and torch.equal(gb.cpu().double(), c["db"])
print("DEBUG-OK")
"""


def test_stepping_debug_build(cuda_device):
    """The AGK_DEBUG library checks every staged piece's element range: two of the cases run without a
    bounds violation (every debug op raises on one) and give the oracle's gradients."""
    from alphago_amd import _build

    assert os.path.exists(_build.hip_path("debug")), "debug library not built"
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, ALPHAGO_AMD_KERNELS="debug", PYTHONPATH=root + os.pathsep + here)
    r = subprocess.run([sys.executable, "-c", _DEBUG_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEBUG-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
