"""The skip operand (``res``) of the conv epilogues -- the forward of a residual block's last layer and the
bitmask dgrad of its first -- on every kernel ``ops.plan_conv`` can pick for an F -> F 3x3 layer, against
the integer oracles of tests/residual_refs.py with ``torch.equal``.

Outputs start as sentinels (bf16 7.0, -1 in bitmask words): the interior must equal the oracle, all four
borders keep the sentinel, padded output channels are exactly 0 with bits 0.  The skip buffer's own
border is NaN, so a read of a border pixel would show in the interior.  The forward checks the value and
the decoded ReLU' bits (the oracle's skip flips > 10 % of the sign tests); the dgrad reads bits encoded in
Python from the written layout."""
import pytest
import torch

import conv_refs as R
import residual_refs as RR
from test_conv_exact import PROD_TILES, SPLITS, _nsplit, _tile_ok, _ws_pack

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TILE_PARAMS = [pytest.param(c, t, id="%s-tile%d" % (R.case_id(c), t)) for c in RR.CASES for t in PROD_TILES
               if _tile_ok(c[3], t)]
_dev_cache = {}


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


def _cached(key, fn):
    if key not in _dev_cache:
        _dev_cache[key] = fn()
    return _dev_cache[key]


def _conv(ops, dev, how, x, w, bias, y, K, S, mode, mbits, res):
    """One launch with a skip operand: a production tile code, "ws" (tile 40) or "sk-<n>"."""
    if how == "ws":
        ops.conv_fwd(x, _ws_pack(ops, w), bias, y, K, S, 1, 1, mode=mode, mbits=mbits, tile=40, res=res)
    elif isinstance(how, str):
        M, Cout, Cin = y.shape[0] * S * S, y.shape[3], x.shape[3]
        ns = _nsplit(ops, how[3:], M, Cout, Cin, K)
        ws = torch.full((ns * M * Cout,), float("nan"), device=dev)
        ops.conv_fwd_splitk(x, w, bias, y, K, S, 1, 1, mode, mbits, ws, ns, res=res)
    else:
        ops.conv_fwd(x, w, bias, y, K, S, 1, 1, mode=mode, mbits=mbits, tile=how, res=res)


# ----------------------------------------------------------------------------- forward
def _fwd_setup(dev, case):
    def build():
        c = RR.fwd_case(case)
        S, B, Cin, Cout, K, Pin = case
        return {"xp": R.place(c["x"], Pin, BF).to(dev), "wf": R.packed(c["w"], Cin, Cout).to(dev),
                "bias": c["bias"].to(dev), "y": c["y"].to(dev), "mask": c["mask"].to(dev),
                "res": RR.res_buffer(c["res"]).to(dev)}

    return _cached(("fwd", case), build)


def _run_forward(ops, dev, case, how):
    S, B, Cin, Cout, K, Pin = case
    s = _fwd_setup(dev, case)
    y = torch.full((B, S + 2, S + 2, Cout), R.BF16_SENTINEL, dtype=BF, device=dev)
    mb = torch.full((B * (S + 2) ** 2 * ops.mbits_words(Cout),), R.MBITS_SENTINEL, dtype=torch.int32, device=dev)
    _conv(ops, dev, how, s["xp"], s["wf"], s["bias"], y, K, S, ops.MODE_BIAS_RELU, mb, s["res"])
    torch.cuda.synchronize()
    co = R.real_channels(case)[1]
    assert R.check_padded(y, s["y"], 1, R.BF16_SENTINEL) == []
    assert R.check_mbits(mb, s["mask"], Cout) == []
    assert not R.interior(y, 1, S)[..., co:].any()
    assert not R.decode_mbits(mb.view(B, S + 2, S + 2, -1), Cout)[..., co:].any()


@pytest.mark.parametrize("case,tile", TILE_PARAMS)
def test_forward_tiles(ops, cuda_device, case, tile):
    _run_forward(ops, cuda_device, case, tile)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", RR.CASES, ids=R.case_id)
def test_forward_splitk(ops, cuda_device, case, split):
    _run_forward(ops, cuda_device, case, "sk-" + split)


@pytest.mark.parametrize("case", RR.CASES, ids=R.case_id)
def test_forward_weight_stationary(ops, cuda_device, case):
    assert ops.conv_ws_supported(case[3], case[2], case[4])
    _run_forward(ops, cuda_device, case, "ws")


# ----------------------------------------------------------------------------- dgrad
def _dgrad_setup(dev, case):
    def build():
        c = RR.dgrad_case(case)
        S, B, Cin, Cout, K, Pin = case
        return {"dzp": R.place(c["dz"], Pin, BF).to(dev), "wd": R.packed(c["w"], Cin, Cout, transposed=True).to(dev),
                "mbits": R.encode_mbits(c["mask"], Cin).flatten().to(dev), "dx": c["dx"].to(BF).to(dev),
                "res": RR.res_buffer(c["res"]).to(dev)}

    return _cached(("dgrad", case), build)


def _run_dgrad(ops, dev, case, how):
    S, B, Cin, Cout, K, Pin = case
    s = _dgrad_setup(dev, case)
    dx = torch.full((B, S + 2, S + 2, Cin), R.BF16_SENTINEL, dtype=BF, device=dev)
    _conv(ops, dev, how, s["dzp"], s["wd"], None, dx, K, S, ops.MODE_MASKBITS, s["mbits"], s["res"])
    torch.cuda.synchronize()
    ci = R.real_channels(case)[0]
    assert R.check_padded(dx, s["dx"], 1, R.BF16_SENTINEL) == []
    assert not R.interior(dx, 1, S)[..., ci:].any()


@pytest.mark.parametrize("case,tile", TILE_PARAMS)
def test_dgrad_tiles(ops, cuda_device, case, tile):
    _run_dgrad(ops, cuda_device, case, tile)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", RR.CASES, ids=R.case_id)
def test_dgrad_splitk(ops, cuda_device, case, split):
    _run_dgrad(ops, cuda_device, case, "sk-" + split)


@pytest.mark.parametrize("case", RR.CASES, ids=R.case_id)
def test_dgrad_weight_stationary(ops, cuda_device, case):
    assert ops.conv_ws_supported(case[2], case[3], case[4])
    _run_dgrad(ops, cuda_device, case, "ws")


# ----------------------------------------------------------------------------- host checks
@pytest.mark.parametrize("how", [0, 40, "sk"])
def test_host_checks_raise_before_any_launch(ops, cuda_device, how):
    """A skip operand that aliases y, has the wrong shape, dtype or device, or comes with mode 1 / 2 is
    refused on the host: the sentinel-filled output is untouched."""
    dev = cuda_device
    case = RR.CASES[0]
    S, B, Cin, Cout, K, Pin = case
    s = _fwd_setup(dev, case)
    w = _ws_pack(ops, s["wf"]) if how == 40 else s["wf"]
    y = torch.full((B, S + 2, S + 2, Cout), R.BF16_SENTINEL, dtype=BF, device=dev)
    ws = torch.zeros(2 * B * S * S * Cout, device=dev)

    def run(res, mode=ops.MODE_BIAS_RELU, out=y, mask=None):
        if how == "sk":
            ops.conv_fwd_splitk(s["xp"], w, s["bias"], out, K, S, 1, 1, mode, None, ws, 2, res=res)
        else:
            ops.conv_fwd(s["xp"], w, s["bias"], out, K, S, 1, 1, mode=mode, mask=mask, tile=how, res=res)

    good = s["res"]
    bad = {
        "alias": y,
        "shape": torch.zeros((B, S + 2, S + 2, Cout + 64), dtype=BF, device=dev),
        "pad": torch.zeros((B, S + 4, S + 4, Cout), dtype=BF, device=dev),
        "dtype": torch.zeros(good.shape, dtype=torch.float32, device=dev),
        "device": good.cpu(),
        "strided": torch.zeros((B, S + 2, S + 2, 2 * Cout), dtype=BF, device=dev)[..., ::2],
    }
    for name, res in bad.items():
        with pytest.raises(RuntimeError):
            run(res)
    # a view into y's memory that overlaps it
    big = torch.full((2 * y.numel(),), R.BF16_SENTINEL, dtype=BF, device=dev)
    y2, r2 = big[:y.numel()].view(y.shape), big[64:64 + y.numel()].view(y.shape)
    with pytest.raises(RuntimeError):
        run(r2, out=y2)
    for mode in (ops.MODE_MASK, ops.MODE_NONE):
        with pytest.raises(RuntimeError):
            run(good, mode=mode, mask=torch.ones_like(y) if mode == ops.MODE_MASK and how != "sk" else None)
    torch.cuda.synchronize()
    assert (y == R.BF16_SENTINEL).all() and (big == R.BF16_SENTINEL).all()
    run(good)  # and the well-formed call runs
    torch.cuda.synchronize()
    assert R.check_padded(y, s["y"], 1, R.BF16_SENTINEL) == []
