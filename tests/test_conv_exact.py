"""The conv forward, dgrad and wgrad kernels (bf16 and fp8), the split-K finish, the weight-stationary
kernel, the wgrad reduce and pack_weights against the fp64 oracles of tests/conv_refs.py on integer data.

The operands are small integers, so every product and every partial sum is exact in fp32 and the
result does not depend on tiling, K order, split count or reduce order: every comparison below is
``torch.equal`` against the oracle.  Outputs start as sentinels (bf16 7.0, NaN in fp32 slabs and
gradients, -1 in bitmask words, 0x5a in byte outputs), the interior must equal the oracle and all four
borders must keep the sentinel.  The dgrad consumers read ReLU' bits encoded in Python from the layout
comment at ConvEpilogue (conv_refs.encode_mbits), the forward producers are decoded with its inverse:
each kernel is pinned to the written layout, not to a partner kernel.

A case skips only where ops.conv_ws_supported / ops.wgrad_direct_supported / ops.wgrad_fp8_supported
says the shape has no instantiation."""
import pytest
import torch
import torch.nn.functional as F

import conv_refs as R
import fp8_ref
from _marks import lab_params

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PROD_TILES = (0, 36, 37, 64, 128, 256, 384, 385, 386, 387, 388)
# kernel-lab tile codes: the LDS-ring tiles (every width); re-cuts of the production loop for the 64 / 128 /
# 192-wide N tiles -- 7 / 8 run the 32x32x16 MFMA and write / read the bitmask through ConvEpilogue32; and the
# kernels of conv_fwd_variants.hip (halo staging, the L2 pixel operand), run at the geometries they were
# written for (19 x 19, the 192-wide 3x3 trunk layer and the 5x5 first layer)
LAB_RING_TILES = (65, 130)
LAB_LOOP_TILES = (7, 8, 9, 10, 2568)
LAB_VARIANT_TILES = (-1, 2, 4, 5, 6, 11, 32)
LAB_VARIANT_FWD_CASES = [(19, 3, 192, 192, 3, 1), (19, 2, 64, 192, 5, 2)]
LAB_VARIANT_DGRAD_CASES = [(19, 3, 192, 192, 3, 1)]
BYTE_SENTINEL = 0x5A


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


def _tile_ok(width, tile, case=None, variant_cases=()):
    """The 160-wide launcher has no 2-wave 32-pixel tile (code 37) and none of the lab re-cuts: not cases,
    by construction."""
    if tile in LAB_VARIANT_TILES:
        return case in variant_cases
    return not (width == 160 and (tile == 37 or tile in LAB_LOOP_TILES))


def _params(cases, width_of, variant_cases):
    """(case, tile) for every tile code that has the case's shape; lab codes marked by ``lab_params``."""
    out = []
    for case in cases:
        for t in lab_params(PROD_TILES + LAB_RING_TILES + LAB_LOOP_TILES + LAB_VARIANT_TILES, PROD_TILES):
            tile, marks = (t, ()) if isinstance(t, int) else (t.values[0], t.marks)
            if _tile_ok(width_of(case), tile, case, variant_cases):
                out.append(pytest.param(case, tile, marks=marks, id="%s-tile%d" % (R.case_id(case), tile)))
    return out


FWD_TILE_PARAMS = _params(R.CASES, lambda c: c[3], LAB_VARIANT_FWD_CASES)
DGRAD_TILE_PARAMS = _params(R.DGRAD_CASES, lambda c: c[2], LAB_VARIANT_DGRAD_CASES)
BF8_TILES = (0, 64, 128, 256, 384, 385, 386, 387, 388)  # the tile codes conv_dgrad_bits_bf8 takes
BF8_CASES = [c for c in R.DGRAD_CASES if c[5] == 1]       # the op fixes the input pad at 1
SPLITS = ("1", "2", "auto")

_dev_cache = {}


def _cached(key, fn):
    if key not in _dev_cache:
        _dev_cache[key] = fn()
    return _dev_cache[key]


# ----------------------------------------------------------------------------- forward
def _fwd_setup(dev, case, impulse=False):
    def build():
        c = (R.impulse_fwd_case if impulse else R.fwd_case)(case)
        S, B, Cin, Cout, K, Pin = case
        return {"xp": R.place(c["x"], Pin, BF).to(dev), "wf": R.packed(c["w"], Cin, Cout).to(dev),
                "bias": c["bias"].to(dev), "y": c["y"].to(dev), "mask": c["mask"].to(dev)}

    return _cached(("fwd", case, impulse), build)


def _fwd_outputs(ops, dev, case):
    S, B, Cin, Cout, K, Pin = case
    y = torch.full((B, S + 2, S + 2, Cout), R.BF16_SENTINEL, dtype=BF, device=dev)
    mb = torch.full((B * (S + 2) ** 2 * ops.mbits_words(Cout),), R.MBITS_SENTINEL, dtype=torch.int32, device=dev)
    return y, mb


def _check_fwd(s, case, y, mb):
    torch.cuda.synchronize()
    Cout = case[3]
    co = R.real_channels(case)[1]
    assert R.check_padded(y, s["y"], 1, R.BF16_SENTINEL) == []
    assert R.check_mbits(mb, s["mask"], Cout) == []
    # padded output channels: exactly 0 and their bits 0 (part of the oracle; stated on its own)
    S = case[0]
    assert not R.interior(y, 1, S)[..., co:].any()
    assert not R.decode_mbits(mb.view(case[1], S + 2, S + 2, -1), Cout)[..., co:].any()


def _ws_pack(ops, w):
    wws = torch.full_like(w, R.BF16_SENTINEL)  # ws_pack fills every element tile 40 reads
    ops.ws_pack([w], [wws])
    return wws


def _nsplit(ops, split, M, cout_p, cin_p, K):
    return ops.splitk_nsplit(M, cout_p, cin_p, K) if split == "auto" else int(split)


def _conv(ops, dev, how, x, w, bias, y, K, S, Pin, mode, mask=None, mbits=None):
    """One conv launch.  ``how``: a tile code (production codes through ops.conv_fwd, kernel-lab codes
    through the lab library), "ws" (tile 40 on the weight-stationary copy of the pack) or "sk-<n>"
    (split-K with n splits or the automatic count; the partials workspace starts as NaN)."""
    if how == "ws":
        ops.conv_fwd(x, _ws_pack(ops, w), bias, y, K, S, Pin, 1, mode=mode, mbits=mbits, tile=40)
    elif isinstance(how, str):
        M, Cout, Cin = y.shape[0] * S * S, y.shape[3], x.shape[3]
        ns = _nsplit(ops, how[3:], M, Cout, Cin, K)
        ws = torch.full((ns * M * Cout,), float("nan"), device=dev)
        ops.conv_fwd_splitk(x, w, bias, y, K, S, Pin, 1, mode, mbits, ws, ns)
    elif how in PROD_TILES:
        ops.conv_fwd(x, w, bias, y, K, S, Pin, 1, mode=mode, mask=mask, mbits=mbits, tile=how)
    else:
        ops.lab().conv_fwd(x, w, bias, mask, y, K, S, Pin, 1, mode, mbits, how)


def _run_forward(ops, dev, case, how, impulse=False):
    S, B, Cin, Cout, K, Pin = case
    s = _fwd_setup(dev, case, impulse)
    y, mb = _fwd_outputs(ops, dev, case)
    _conv(ops, dev, how, s["xp"], s["wf"], s["bias"], y, K, S, Pin, ops.MODE_BIAS_RELU, mbits=mb)
    _check_fwd(s, case, y, mb)


@pytest.mark.parametrize("case,tile", FWD_TILE_PARAMS)
def test_forward_tiles(ops, cuda_device, case, tile):
    """Bias + ReLU + bitmask on every tile code: y bitwise, decode_mbits(mb) == (y_ref > 0) everywhere."""
    _run_forward(ops, cuda_device, case, tile)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_forward_splitk(ops, cuda_device, case, split):
    """Split-K 32-pixel tile and its finishing pass with 1, 2 and ops.splitk_nsplit(...) splits."""
    _run_forward(ops, cuda_device, case, "sk-" + split)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_forward_weight_stationary(ops, cuda_device, case):
    """Tile 40 after ws_pack."""
    if not ops.conv_ws_supported(case[3], case[2], case[4]):
        pytest.skip("conv_ws_supported: no weight-stationary instantiation for this shape")
    _run_forward(ops, cuda_device, case, "ws")


@pytest.mark.parametrize("how", PROD_TILES + ("sk-auto", "ws"))
@pytest.mark.parametrize("case", R.IMPULSE_CASES, ids=R.case_id)
def test_forward_impulses(ops, cuda_device, case, how):
    """Unit impulses at the corners and the centre through w = 1 + kh K + kw: tap placement."""
    if how == "ws":
        assert ops.conv_ws_supported(case[3], case[2], case[4])
    _run_forward(ops, cuda_device, case, how, impulse=True)


# ----------------------------------------------------------------------------- dgrad
def _dgrad_setup(dev, case, impulse=False):
    def build():
        c = (R.impulse_dgrad_case if impulse else R.dgrad_case)(case)
        S, B, Cin, Cout, K, Pin = case
        return {"dzp": R.place(c["dz"], Pin, BF).to(dev), "wd": R.packed(c["w"], Cin, Cout, transposed=True).to(dev),
                "mbits": R.encode_mbits(c["mask"], Cin).flatten().to(dev),
                "act": R.place(R.mask_activation(c["mask"]), 1, BF).to(dev), "dx": c["dx"].to(BF).to(dev),
                "dx64": c["dx"]}

    return _cached(("dgrad", case, impulse), build)


def _dx_output(dev, case):
    S, B, Cin = case[0], case[1], case[2]
    return torch.full((B, S + 2, S + 2, Cin), R.BF16_SENTINEL, dtype=BF, device=dev)


def _check_dx(s, case, dx):
    torch.cuda.synchronize()
    S, ci = case[0], R.real_channels(case)[0]
    assert R.check_padded(dx, s["dx"], 1, R.BF16_SENTINEL) == []
    assert not R.interior(dx, 1, S)[..., ci:].any()


def _run_dgrad(ops, dev, case, how, mode="bits", impulse=False):
    S, B, Cin, Cout, K, Pin = case
    s = _dgrad_setup(dev, case, impulse)
    dx = _dx_output(dev, case)
    if mode == "bits":
        _conv(ops, dev, how, s["dzp"], s["wd"], None, dx, K, S, Pin, ops.MODE_MASKBITS, mbits=s["mbits"])
    else:
        _conv(ops, dev, how, s["dzp"], s["wd"], None, dx, K, S, Pin, ops.MODE_MASK, mask=s["act"])
    _check_dx(s, case, dx)


@pytest.mark.parametrize("mode", ["bits", "mask"])
@pytest.mark.parametrize("case,tile", DGRAD_TILE_PARAMS)
def test_dgrad_tiles(ops, cuda_device, case, tile, mode):
    """Each dgrad consumer on its own: MODE_MASKBITS reads bits encoded in Python from the written layout,
    MODE_MASK a bf16 activation with negative values, +0.0 and -0.0 where the mask is off."""
    _run_dgrad(ops, cuda_device, case, tile, mode)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", R.DGRAD_CASES, ids=R.case_id)
def test_dgrad_splitk(ops, cuda_device, case, split):
    _run_dgrad(ops, cuda_device, case, "sk-" + split)


@pytest.mark.parametrize("case", R.DGRAD_CASES, ids=R.case_id)
def test_dgrad_weight_stationary(ops, cuda_device, case):
    if not ops.conv_ws_supported(case[2], case[3], case[4]):
        pytest.skip("conv_ws_supported: no weight-stationary instantiation for the transposed shape")
    _run_dgrad(ops, cuda_device, case, "ws")


@pytest.mark.parametrize("how", PROD_TILES + ("sk-auto", "ws"))
@pytest.mark.parametrize("case", R.IMPULSE_CASES[:1], ids=R.case_id)
def test_dgrad_impulses(ops, cuda_device, case, how):
    """Impulse gradients through the asymmetric weights: the flipped taps of the dgrad pack (the 3x3
    geometry; the 5x5 one below runs the tiles, its transposed shape having no weight-stationary kernel)."""
    _run_dgrad(ops, cuda_device, case, how, impulse=True)


@pytest.mark.parametrize("how", PROD_TILES + ("sk-auto",))
@pytest.mark.parametrize("case", R.IMPULSE_CASES[1:], ids=R.case_id)
def test_dgrad_impulses_5x5(ops, cuda_device, case, how):
    _run_dgrad(ops, cuda_device, case, how, impulse=True)


def _amax(slots):
    return slots.view(torch.float32).max().item()


@pytest.mark.parametrize("tile", BF8_TILES)
@pytest.mark.parametrize("case", BF8_CASES, ids=R.case_id)
def test_dgrad_bits_bf8_copy(ops, cuda_device, case, tile):
    """conv_dgrad_bits_bf8: dx bitwise, its e5m2 copy == fp8_ref.quantize(dx * 2^-4) (ties occur), the 64
    amax slots fold to exactly max |dx|."""
    S, B, Cin, Cout, K, Pin = case
    s = _dgrad_setup(cuda_device, case)
    dx = _dx_output(cuda_device, case)
    dx8 = torch.full(dx.shape, BYTE_SENTINEL, dtype=torch.uint8, device=cuda_device)
    amax = ops.fp8_amax_buffer(1, cuda_device)[0]
    sc = torch.tensor([2.0 ** -4], device=cuda_device)
    ops.conv_dgrad_bits_bf8(s["dzp"], s["wd"], dx, s["mbits"], dx8, sc, K, S, amax=amax, tile=tile)
    _check_dx(s, case, dx)
    want8 = torch.from_numpy(fp8_ref.quantize((s["dx64"] * 2.0 ** -4).float().numpy(), "e5m2"))
    assert R.check_padded(dx8.cpu(), want8, 1, BYTE_SENTINEL) == []
    assert _amax(amax) == s["dx64"].abs().max().item()


# ----------------------------------------------------------------------------- wgrad
def _wgrad_setup(dev, case):
    def build():
        c = R.wgrad_case(case)
        S, B, Cin, Cout, K, Pin = case
        return {"xp": R.place(c["x"], Pin, BF).to(dev), "dzp": R.place(c["dz"], 1, BF).to(dev),
                "dw": c["dw"].float().to(dev), "db": c["db"].float().to(dev), "dw64": c["dw"], "db64": c["db"]}

    return _cached(("wgrad", case), build)


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _thin(case):
    """cin_real as the trainers pass it: the real plane count of a 64-channel first-layer input, else 0."""
    ci = R.real_channels(case)[0]
    return ci if case[2] == 64 and ci < 64 else 0


def _reduce_and_check(ops, dev, case, s, slab, dbs, mult=1.0):
    ci, co = R.real_channels(case)
    K = case[4]
    gw, gb = _nan((co, ci, K, K), dev), _nan((co,), dev)
    ops.conv_wgrad_reduce(slab, dbs, gw, gb, 1.0, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(gw, s["dw"] * mult)
    if slab.shape[3] == case[2] and not _thin(case):
        # every slab column written: the gradient at the padded widths is the oracle with zero rows and columns
        gwp = _nan((slab.shape[2], slab.shape[3], K, K), dev)
        ops.conv_wgrad_reduce(slab, dbs, gwp, None, 1.0, 0.0)
        torch.cuda.synchronize()
        assert torch.equal(gwp, F.pad(s["dw"] * mult, (0, 0, 0, 0, 0, gwp.shape[1] - ci, 0, gwp.shape[0] - co)))
    return gb


SMALL_PLAN_CASES = [c for c in R.CASES if c[4] == 3 and 160 not in (c[2], c[3])]  # what ops.wgrad_config gives it
WGRAD_PARAMS = ([pytest.param(c, 0, id=R.case_id(c) + "-v0") for c in R.CASES] +
                [pytest.param(c, 14, id=R.case_id(c) + "-v14") for c in SMALL_PLAN_CASES] +
                [pytest.param(c, p.values[0], marks=p.marks, id="%s-v%d" % (R.case_id(c), p.values[0]))
                 for c in R.CASES[:3] for p in lab_params((5, 6, 7, 9), ())])


@pytest.mark.parametrize("split", ["1", "3", "auto"])
@pytest.mark.parametrize("case,variant", WGRAD_PARAMS)
def test_wgrad_slab_and_reduce(ops, cuda_device, case, variant, split):
    """conv_wgrad (0: per-tap kernel, 14: the small-batch plan; lab: the row, tap-pair, line and ring
    kernels) into NaN slabs, then conv_wgrad_reduce into NaN gradients: grad_w and grad_b bitwise."""
    S, B, Cin, Cout, K, Pin = case
    s = _wgrad_setup(cuda_device, case)
    ns = ops.wgrad_splits(B * S * S, K * K) if split == "auto" else int(split)
    slab, dbs = _nan((ns, K * K, Cout, Cin), cuda_device), _nan((ns, Cout), cuda_device)
    ops.conv_wgrad(s["xp"], s["dzp"], slab, dbs, K, S, Pin, 1, cin_real=_thin(case), variant=variant)
    gb = _reduce_and_check(ops, cuda_device, case, s, slab, dbs)
    assert torch.equal(gb, s["db"])


@pytest.mark.parametrize("ksub", [1, 2, 4, 8])
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_wgrad_direct(ops, cuda_device, case, ksub):
    """Split-free wgrad into NaN gradients (beta 0 never reads them), then scale 0.5 / beta 2.0 on an
    integer gradient: both bitwise."""
    S, B, Cin, Cout, K, Pin = case
    ci, co = R.real_channels(case)
    if not ops.wgrad_direct_supported(Cout, Cin, ci, K):
        pytest.skip("wgrad_direct_supported: no instantiation for this shape")
    s = _wgrad_setup(cuda_device, case)
    gw, gb = _nan((co, ci, K, K), cuda_device), _nan((co,), cuda_device)
    ops.conv_wgrad_direct(s["xp"], s["dzp"], gw, gb, K, S, Pin, 1, ksub=ksub)
    torch.cuda.synchronize()
    assert torch.equal(gw, s["dw"]) and torch.equal(gb, s["db"])
    g0w, g0b = R.wgrad_g0(case, "w"), R.wgrad_g0(case, "b")
    gw2, gb2 = g0w.float().to(cuda_device), g0b.float().to(cuda_device)
    ops.conv_wgrad_direct(s["xp"], s["dzp"], gw2, gb2, K, S, Pin, 1, scale=0.5, beta=2.0, ksub=ksub)
    torch.cuda.synchronize()
    assert torch.equal(gw2.cpu(), R.combine(g0w, s["dw64"], 0.5, 2.0))
    assert torch.equal(gb2.cpu(), R.combine(g0b, s["db64"], 0.5, 2.0))


def _int_slabs(ns, T, Cout, Cin, cin_real, seed):
    g = torch.Generator().manual_seed(seed)
    slab = torch.randint(-1000, 1001, (ns, T, Cout, Cin), generator=g).double()
    dbs = torch.randint(-1000, 1001, (ns, Cout), generator=g).double()
    K = int(round(T ** 0.5))
    g0w = torch.randint(-64, 65, (Cout, Cin, K, K), generator=g).double()
    g0b = torch.randint(-64, 65, (Cout,), generator=g).double()
    slab_nan = slab.float()
    slab_nan[..., cin_real:] = float("nan")  # unused slab columns must never be read
    return slab, dbs, g0w, g0b, slab_nan


REDUCE_SHAPES = [(1, 9, 192, 192, 192, 192), (3, 9, 64, 64, 64, 64), (7, 25, 192, 64, 48, 192),
                 (56, 9, 192, 192, 192, 192), (21, 9, 160, 160, 152, 152), (5, 25, 160, 64, 49, 152)]


def _reduce_expect(slab, dbs, g0w, g0b, cin_real, cout_real, scale, beta):
    K = g0w.shape[2]
    dw = slab.sum(0)[:, :cout_real, :cin_real].permute(1, 2, 0).reshape(cout_real, cin_real, K, K)
    return (R.combine(g0w[:cout_real, :cin_real], dw, scale, beta),
            R.combine(g0b[:cout_real], dbs.sum(0)[:cout_real], scale, beta))


@pytest.mark.parametrize("ns,T,Cout,Cin,cin_real,cout_real", REDUCE_SHAPES)
def test_wgrad_reduce(ops, cuda_device, ns, T, Cout, Cin, cin_real, cout_real):
    """conv_wgrad_reduce alone on integer slabs: any split count, NaN in the unused columns, real channel
    counts below the padded ones, scale 0.5 / beta 2.0 and scale 1 / beta 0 into NaN."""
    dev = cuda_device
    slab, dbs, g0w, g0b, slab_nan = _int_slabs(ns, T, Cout, Cin, cin_real, 100 + ns)
    gw = g0w[:cout_real, :cin_real].float().contiguous().to(dev)
    gb = g0b[:cout_real].float().to(dev)
    ops.conv_wgrad_reduce(slab_nan.to(dev), dbs.float().to(dev), gw, gb, 0.5, 2.0)
    ew, eb = _reduce_expect(slab, dbs, g0w, g0b, cin_real, cout_real, 0.5, 2.0)
    torch.cuda.synchronize()
    assert torch.equal(gw.cpu(), ew) and torch.equal(gb.cpu(), eb)
    gw, gb = _nan(gw.shape, dev), _nan(gb.shape, dev)
    ops.conv_wgrad_reduce(slab_nan.to(dev), dbs.float().to(dev), gw, gb, 1.0, 0.0)
    ew, eb = _reduce_expect(slab, dbs, 0 * g0w, 0 * g0b, cin_real, cout_real, 1.0, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(gw.cpu(), ew) and torch.equal(gb.cpu(), eb)


def test_wgrad_reduce_multi(ops, cuda_device):
    """Every shape above in one conv_wgrad_reduce_multi launch."""
    dev = cuda_device
    slabs, dbss, gws, gbs, want = [], [], [], [], []
    for ns, T, Cout, Cin, cin_real, cout_real in REDUCE_SHAPES:
        slab, dbs, g0w, g0b, slab_nan = _int_slabs(ns, T, Cout, Cin, cin_real, 200 + ns)
        slabs.append(slab_nan.to(dev))
        dbss.append(dbs.float().to(dev))
        gws.append(g0w[:cout_real, :cin_real].float().contiguous().to(dev))
        gbs.append(g0b[:cout_real].float().to(dev))
        want.append(_reduce_expect(slab, dbs, g0w, g0b, cin_real, cout_real, 0.5, 2.0))
    ops.conv_wgrad_reduce_multi(slabs, dbss, gws, gbs, 0.5, 2.0)
    torch.cuda.synchronize()
    for gw, gb, (ew, eb) in zip(gws, gbs, want):
        assert torch.equal(gw.cpu(), ew) and torch.equal(gb.cpu(), eb)


# ----------------------------------------------------------------------------- fp8
# E8M0 scale bytes (127 = 2^0): all ones, and activations / gradients 2^2 with weights 2^-1 (product 2)
FP8_EXPONENTS = [(127, 127), (129, 126)]
OUT_SCALE = 2.0 ** -4  # byte outputs of integers / 16: ties to even occur


def _mult(exps):
    return 2.0 ** (exps[0] - 127 + exps[1] - 127)


def _bytes(t_nhwc, P, dtype, dev):
    """Integer values as e4m3 / e5m2 bytes in a zero-bordered padded buffer (exact: |v| <= 4)."""
    b = R.place(t_nhwc, P, torch.float32).to(dtype)
    assert torch.equal(b.float().double(), R.place(t_nhwc, P, torch.float64))
    return b.view(torch.uint8).to(dev)


def _quant(t64, fmt):
    return torch.from_numpy(fp8_ref.quantize(t64.float().numpy(), fmt))


def _i32(vals, dev):
    return torch.tensor(list(vals), dtype=torch.int32, device=dev)


def _w8(ops, dev, w, rows_p, red_p, transposed):
    """Ternary weights as packed e4m3 at scale 1 (ALPHAGO_AMD_FP8_CW32 picks the chunk width)."""
    K = w.shape[2]
    out = torch.zeros(ops.fp8_weight_shape(K, red_p, rows_p), dtype=torch.uint8, device=dev)
    ops.pack_weights_fp8_multi([w.float().to(dev)], [out], torch.ones(1, device=dev), [0], [int(transposed)])
    return out


FP8_FWD_PARAMS = [(c, cw) for c in R.FP8_FWD_CASES for cw in ((32, 64) if c[2] == 160 else (64,))]


@pytest.mark.parametrize("outs", ["both", "fp8"])
@pytest.mark.parametrize("exps", FP8_EXPONENTS, ids=["e127", "e129-126"])
@pytest.mark.parametrize("case,cw", FP8_FWD_PARAMS, ids=lambda v: R.case_id(v) if isinstance(v, tuple) else "cw%d" % v)
def test_fp8_forward(ops, cuda_device, monkeypatch, case, cw, exps, outs):
    """conv_fwd_fp8 (production variant) on ternary bytes: bf16 output, e4m3 output ==
    fp8_ref.quantize(exact * 2^-4), amax == the exact max, ReLU' bitmask; no stochastic rounding."""
    monkeypatch.setenv("ALPHAGO_AMD_FP8_CW32", "1" if cw == 32 else "0")
    dev = cuda_device
    S, B, Cin, Cout, K, Pin = case
    c = R.fwd_case(case)
    m = _mult(exps)
    x8 = _bytes(c["x"], Pin, torch.float8_e4m3fn, dev)
    w8 = _w8(ops, dev, c["w"], Cout, Cin, False)
    assert w8.shape[2] == (cw if Cin == 160 else 64)
    y, mb = _fwd_outputs(ops, dev, case)
    y8 = torch.full(y.shape, BYTE_SENTINEL, dtype=torch.uint8, device=dev)
    amax = ops.fp8_amax_buffer(1, dev)[0]
    ops.conv_fwd_fp8(x8, w8, (c["bias"] * m).to(dev), _i32(exps, dev), torch.tensor([OUT_SCALE], device=dev), K, S,
                     Pin, 1, y_bf16=y if outs == "both" else None, y_fp8=y8, amax=amax, mbits=mb)
    torch.cuda.synchronize()
    want = c["y"].double() * m
    if outs == "both":
        assert R.check_padded(y.cpu(), want.to(BF), 1, R.BF16_SENTINEL) == []
    assert R.check_padded(y8.cpu(), _quant(want * OUT_SCALE, "e4m3"), 1, BYTE_SENTINEL) == []
    assert R.check_mbits(mb.cpu(), c["mask"], Cout) == []
    assert _amax(amax) == want.max().item()


def _fp8_dgrad_common(ops, dev, case, cw, monkeypatch):
    monkeypatch.setenv("ALPHAGO_AMD_FP8_CW32", "1" if cw == 32 else "0")
    S, B, C, _, K, Pin = case
    c = R.dgrad_case(case)
    w8t = _w8(ops, dev, c["w"], C, C, True)
    dx = _dx_output(dev, case)
    dx8 = torch.full(dx.shape, BYTE_SENTINEL, dtype=torch.uint8, device=dev)
    return c, w8t, dx, dx8, ops.fp8_amax_buffer(1, dev)[0]


def _check_fp8_dx(c, m, dx, dx8, amax):
    torch.cuda.synchronize()
    want = c["dx"] * m
    if dx is not None:
        assert R.check_padded(dx.cpu(), want.to(BF), 1, R.BF16_SENTINEL) == []
    if dx8 is not None:
        assert R.check_padded(dx8.cpu(), _quant(want * OUT_SCALE, "e5m2"), 1, BYTE_SENTINEL) == []
    assert _amax(amax) == want.abs().max().item()


FP8_SQ_PARAMS = [(c, cw) for c in R.FP8_SQUARE_CASES for cw in ((32, 64) if c[2] == 160 else (64,))]
_sq_ids = lambda v: R.case_id(v) if isinstance(v, tuple) else "cw%d" % v  # noqa: E731


@pytest.mark.parametrize("exps", FP8_EXPONENTS, ids=["e127", "e129-126"])
@pytest.mark.parametrize("case,cw", FP8_SQ_PARAMS, ids=_sq_ids)
def test_fp8_dgrad_mask(ops, cuda_device, monkeypatch, case, cw, exps):
    """conv_dgrad_fp8: e5m2 gradient bytes x transposed e4m3 weights, masked by a bf16 activation."""
    dev = cuda_device
    S, K = case[0], case[4]
    c, w8t, dx, dx8, amax = _fp8_dgrad_common(ops, dev, case, cw, monkeypatch)
    dz8 = _bytes(c["dz"], 1, torch.float8_e5m2, dev)
    act = R.place(R.mask_activation(c["mask"]), 1, BF).to(dev)
    ops.conv_dgrad_fp8(dz8, w8t, act, _i32(exps, dev), torch.tensor([OUT_SCALE], device=dev), K, S, dx, y_fp8=dx8,
                       amax=amax)
    _check_fp8_dx(c, _mult(exps), dx, dx8, amax)


@pytest.mark.parametrize("outs", ["both", "fp8", "bf16"])
@pytest.mark.parametrize("exps", FP8_EXPONENTS, ids=["e127", "e129-126"])
@pytest.mark.parametrize("case,cw", FP8_SQ_PARAMS, ids=_sq_ids)
def test_fp8_dgrad_bits(ops, cuda_device, monkeypatch, case, cw, exps, outs):
    """conv_dgrad_fp8_bits: ReLU' from oracle-encoded bits; e5m2 and / or bf16 outputs."""
    dev = cuda_device
    S, K, C = case[0], case[4], case[2]
    c, w8t, dx, dx8, amax = _fp8_dgrad_common(ops, dev, case, cw, monkeypatch)
    dz8 = _bytes(c["dz"], 1, torch.float8_e5m2, dev)
    mbits = R.encode_mbits(c["mask"], C).flatten().to(dev)
    dx = dx if outs in ("both", "bf16") else None
    dx8 = dx8 if outs in ("both", "fp8") else None
    ops.conv_dgrad_fp8_bits(dz8, w8t, mbits, _i32(exps, dev), torch.tensor([OUT_SCALE], device=dev), K, S, y_bf16=dx,
                            y_fp8=dx8, amax=amax)
    _check_fp8_dx(c, _mult(exps), dx, dx8, amax)


@pytest.mark.parametrize("exps", FP8_EXPONENTS, ids=["e127", "e129-126"])
@pytest.mark.parametrize("case,cw", FP8_SQ_PARAMS, ids=_sq_ids)
def test_fp8_dgrad_from_bf16(ops, cuda_device, monkeypatch, case, cw, exps):
    """conv_dgrad_fp8_bf16: the bf16 gradient times in_scale = 2^3 becomes e5m2 in registers (+-8: exact);
    the E8M0 byte undoes the 2^3 on top of the pair's own exponent."""
    dev = cuda_device
    S, K, C = case[0], case[4], case[2]
    c, w8t, dx, _, amax = _fp8_dgrad_common(ops, dev, case, cw, monkeypatch)
    dzp = R.place(c["dz"], 1, BF).to(dev)
    mbits = R.encode_mbits(c["mask"], C).flatten().to(dev)
    ops.conv_dgrad_fp8_bf16(dzp, w8t, mbits, _i32((exps[0] - 3, exps[1]), dev), torch.tensor([8.0], device=dev), K, S,
                            dx, amax=amax)
    _check_fp8_dx(c, _mult(exps), dx, None, amax)


@pytest.mark.parametrize("exps", FP8_EXPONENTS, ids=["e127", "e129-126"])
@pytest.mark.parametrize("case", R.FP8_SQUARE_CASES, ids=R.case_id)
def test_fp8_wgrad(ops, cuda_device, case, exps):
    """conv_wgrad_fp8 at 160 and 192 on integer bytes in [-4, 4] into NaN slabs, reduced into NaN
    gradients: grad_w, grad_b and the gradient amax bitwise."""
    dev = cuda_device
    S, B, C, _, K, Pin = case
    if not ops.wgrad_fp8_supported(C, C, K):
        pytest.skip("wgrad_fp8_supported: no instantiation for this shape")
    c = R.wgrad_case(case)
    s = _wgrad_setup(dev, case)
    x8 = _bytes(c["x"], 1, torch.float8_e4m3fn, dev)
    dz8 = _bytes(c["dz"], 1, torch.float8_e5m2, dev)
    gmul = 2.0 ** (127 - exps[1])  # the multiplier the gradient bytes carry, undone by their E8M0 byte
    ns = ops.wgrad_fp8_nsplit(B * S * S, K, width=C)
    slab, dbs = _nan((ns, K * K, C, C), dev), _nan((ns, C), dev)
    amax = ops.fp8_amax_buffer(1, dev)[0]
    ops.conv_wgrad_fp8(x8, dz8, slab, dbs, _i32(exps[:1], dev), _i32(exps[1:], dev), torch.tensor([gmul], device=dev),
                       K, S, 1, 1, amax=amax)
    gb = _reduce_and_check(ops, dev, case, s, slab, dbs, mult=_mult(exps))
    assert torch.equal(gb, s["db"] / gmul)
    assert _amax(amax) == c["dz"].abs().max().item() / gmul


# ----------------------------------------------------------------------------- pack_weights
@pytest.mark.parametrize("co,ci,cout_p,cin_p,K", [(192, 48, 192, 64, 5), (152, 152, 160, 160, 3),
                                                  (192, 192, 192, 192, 3)])
def test_pack_weights(ops, cuda_device, co, ci, cout_p, cin_p, K):
    """wf[t][n][c] = bf16(w[n][c][kh][kw]), wd[tf][c][n] at the flipped tap, zeros in every padded row and
    column, into destinations that start as sentinels.  Contract: the extra tap of
    ops.packed_weight_like (reduction width an odd multiple of 32) is not the pack's to write -- it keeps
    what the allocation put there (zeros in production)."""
    g = torch.Generator().manual_seed(co + ci + K)
    w = torch.randint(-100, 101, (co, ci, K, K), generator=g).double()  # integers: exact in bf16
    ewf, ewd = R.expected_pack(w, cin_p, cout_p)
    wdev = w.float().to(cuda_device)
    wf = torch.full_like(ops.packed_weight_like(wdev, cin_p, cout_p), R.BF16_SENTINEL)
    wd = torch.full_like(ops.packed_weight_like(wdev, cin_p, cout_p, transposed=True), R.BF16_SENTINEL)
    ops.pack_weights([wdev], [wf], [wd])
    torch.cuda.synchronize()
    T = K * K
    assert torch.equal(wf[:T].cpu(), ewf) and torch.equal(wd[:T].cpu(), ewd)
    assert wf.shape[0] == T + (1 if cin_p % 64 == 32 else 0) and wd.shape[0] == T + (1 if cout_p % 64 == 32 else 0)
    assert (wf[T:] == R.BF16_SENTINEL).all() and (wd[T:] == R.BF16_SENTINEL).all()
    # and the packs the conv tests feed the kernels are these
    assert torch.equal(R.packed(w, cin_p, cout_p)[:T], ewf)


# ----------------------------------------------------------------------------- coverage of the lists
def test_every_kernel_reached(ops, cuda_device):
    """Walk the parameter lists with the support predicates and ops.plan_conv: every production kernel
    family is run by at least two (direction, case) pairs.  A tile code counts for the kernel the launcher
    really runs: code 0 resolves to the 32-pixel tile 36 at every committed size (M < 8192), so it never
    reaches a large tile here -- those are forced by their codes; code 388 is the compact-halo kernel only
    where it covers the layer (3x3, 192-wide N tile, S <= 19, bias + ReLU or the bitmask dgrad) and runs
    386 elsewhere, as it does for the dgrad's MODE_MASK runs."""
    hits = {}

    def hit(name, what):
        hits.setdefault(name, set()).add(what)

    runs = [("fwd", c, c[3], c[2]) for c in R.CASES] + [("dgrad", c, c[2], c[3]) for c in R.DGRAD_CASES]
    for kind, case, wout, wred in runs:  # output width, reduction width
        S, B, K = case[0], case[1], case[4]
        M = B * S * S
        assert M < 8192
        for tile in PROD_TILES:
            if _tile_ok(wout, tile):
                runs_as = ops.conv_fwd_tile_info(M, S, K, wred, wout, 0 if kind == "fwd" else 3, tile=tile).code
                hit("tile %d" % runs_as, (kind, case))
        hit("N tile %d" % ops.conv_n_tile(wout), (kind, case))
        if wred % 64 == 32:
            hit("straddled K-steps", (kind, case))
        if ops.conv_ws_supported(wout, wred, K):  # test_*_weight_stationary run exactly these
            hit("weight-stationary", (kind, case))
        hit("split-K", (kind, case))
        if ops.splitk_nsplit(M, wout, wred, K) > 2:  # "auto" differs from the fixed counts 1 and 2
            hit("split-K, automatic count", (kind, case))
        plan = ops.plan_conv(M, wout, wred, K)  # what the trainers and inference would launch
        hit("plan " + plan.kind, (kind, case))
        assert plan.kind != "ws" or ops.conv_ws_supported(wout, wred, K)
        assert plan.kind != "splitk" or plan.nsplit == ops.splitk_nsplit(M, wout, wred, K)
    for case in R.CASES:
        S, B, Cin, Cout, K, Pin = case
        hit("wgrad per tap, %d taps per workgroup" % ops.wgrad_tap_group(Cout, Cin, K), case)
        if ops.wgrad_direct_supported(Cout, Cin, R.real_channels(case)[0], K):
            hit("wgrad direct", case)
        if _thin(case):
            hit("wgrad thin input", case)
        if 160 in (Cin, Cout):
            hit("wgrad 160-wide", case)
    for case in SMALL_PLAN_CASES:
        hit("wgrad small plan", case)
    for case in R.FP8_SQUARE_CASES:
        if ops.wgrad_fp8_supported(case[3], case[2], case[4]):
            hit("fp8 wgrad %d" % case[2], case)
        hit("fp8 dgrad %d" % case[2], case)
    for case, cw in FP8_FWD_PARAMS:
        hit("fp8 forward, chunk width %d" % cw, case)
    expected = (["tile %d" % t for t in PROD_TILES if t != 0] + ["N tile %d" % n for n in (64, 128, 160, 192)] +
                ["straddled K-steps", "weight-stationary", "split-K", "split-K, automatic count", "plan ws",
                 "plan splitk", "wgrad direct", "wgrad thin input", "wgrad 160-wide", "wgrad small plan",
                 "fp8 wgrad 160", "fp8 wgrad 192", "fp8 dgrad 160", "fp8 dgrad 192", "fp8 forward, chunk width 32",
                 "fp8 forward, chunk width 64"])
    assert {k: len(v) for k, v in hits.items() if k in expected and len(v) < 2} == {}
    assert [k for k in expected if k not in hits] == []
    assert sum(1 for k in hits if k.startswith("wgrad per tap")) >= 2  # tap-merged and one-tap workgroups
