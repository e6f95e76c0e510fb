"""How the conv epilogue's values reach memory: the paired 16-byte stores of ConvEpilogue (two channel
blocks of a pixel exchanged between lanes l and l ^ 16, one 64-byte run per pixel and instruction), the
unpaired last block of an odd block count, the paired e5m2 copy and the residual epilogue, which stays
unpaired.

Every check is ``torch.equal`` against the integer oracles of tests/conv_refs.py (tests/residual_refs.py
for the skip operand), which know nothing of the kernels; comparing one tile with another would prove
nothing, since all of them share the epilogue.  The shapes are the smallest where a paired store can go
wrong: partial tiles whose rows past M fall inside a 16-pixel block (both lanes of a pair must agree on
the pixel), every block count (NB = 6, 5, 4, 2), a second tile column (blockIdx.y = 1) and the 5x5
first-layer geometry.

Every output lives in a larger allocation: ``FRONT`` elements in front of it and ``GUARD`` behind it hold
the sentinel, as do the tensor's own borders, and all of them must still hold it afterwards -- a store
displaced by the pairing offset (+12 elements in the odd lane rows) would land there or in a neighbour
pixel.  ``shift`` moves the tensor 8 bytes off its 16-byte boundary (4 bytes for the e5m2 bytes): the
16-byte stores then straddle 16-byte lines and the result must not change."""
import pytest
import torch

import conv_refs as R
import fp8_ref
import residual_refs as RR

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
BYTE_SENTINEL = 0x5A
FRONT = 64    # elements in front of an output (a multiple of 16 bytes for every dtype used)
GUARD = 4096  # elements behind it
PARTIAL_CASES = [(19, 1, 192, 192, 3, 1), (9, 5, 192, 192, 3, 1)]  # M = 361, M = 405 (a tile spans five boards)
PARTIAL_TILES = (36, 64, 128, 256, 386, 388)
# 192 -> 384 (blockIdx.y = 1), 128 and 64 wide (NB 4 and 2), 160 wide (NB 5: a narrow last block), 5x5 first layer
WIDTH_CASES = [(19, 2, 192, 384, 3, 1), (13, 3, 128, 128, 3, 1), (19, 2, 64, 64, 3, 1), (19, 2, 160, 160, 3, 1),
               (19, 2, 64, 192, 5, 2)]
WIDTH_TILES = (64, 386)  # a 32-pixel-per-wave loop with load() inside the K loop, and the 96-pixel-per-wave tile
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


class Guarded:
    """A sentinel-filled tensor of ``shape`` inside a sentinel-filled allocation; ``shift`` elements off
    the aligned position."""

    def __init__(self, shape, sentinel, dtype, dev, shift=0):
        n = 1
        for s in shape:
            n *= s
        self.sentinel, self.n, self.start = sentinel, n, FRONT + shift
        self.buf = torch.full((FRONT + shift + n + GUARD,), sentinel, dtype=dtype, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[self.start:self.start + n].view(shape)
        assert self.t.data_ptr() == self.buf.data_ptr() + self.start * self.buf.element_size()

    def outside_untouched(self):
        return bool((self.buf[:self.start] == self.sentinel).all()) and \
            bool((self.buf[self.start + self.n:] == self.sentinel).all())


def _fwd_setup(dev, case, refs=R):
    def build():
        c = refs.fwd_case(case)
        S, B, Cin, Cout, K, Pin = case
        s = {"xp": R.place(c["x"], Pin, BF).to(dev), "wf": R.packed(c["w"], Cin, Cout).to(dev),
             "bias": c["bias"].to(dev), "y": c["y"].to(dev), "mask": c["mask"].to(dev)}
        if refs is RR:
            s["res"] = RR.res_buffer(c["res"]).to(dev)
        return s

    return _cached(("fwd", case, refs is RR), build)


def _dgrad_setup(dev, case, refs=R):
    def build():
        c = refs.dgrad_case(case)
        S, B, Cin, Cout, K, Pin = case
        s = {"dzp": R.place(c["dz"], Pin, BF).to(dev), "wd": R.packed(c["w"], Cin, Cout, transposed=True).to(dev),
             "mbits": R.encode_mbits(c["mask"], Cin).flatten().to(dev), "dx": c["dx"].to(BF).to(dev), "dx64": c["dx"]}
        if refs is RR:
            s["res"] = RR.res_buffer(c["res"]).to(dev)
        return s

    return _cached(("dgrad", case, refs is RR), build)


def _forward(ops, dev, case, tile, shift=0, refs=R):
    """Bias + ReLU (+ skip operand) with the ReLU' bits written; returns (y, bits) after every check."""
    S, B, Cin, Cout, K, Pin = case
    s = _fwd_setup(dev, case, refs)
    y = Guarded((B, S + 2, S + 2, Cout), R.BF16_SENTINEL, BF, dev, shift)
    mb = Guarded((B * (S + 2) ** 2 * ops.mbits_words(Cout),), R.MBITS_SENTINEL, torch.int32, dev)
    ops.conv_fwd(s["xp"], s["wf"], s["bias"], y.t, K, S, Pin, 1, mode=ops.MODE_BIAS_RELU, mbits=mb.t, tile=tile,
                 res=s.get("res"))
    torch.cuda.synchronize()
    co = R.real_channels(case)[1]
    assert R.check_padded(y.t, s["y"], 1, R.BF16_SENTINEL) == []
    assert R.check_mbits(mb.t, s["mask"], Cout) == []
    assert not R.interior(y.t, 1, S)[..., co:].any()
    assert y.outside_untouched() and mb.outside_untouched()
    return y.t, mb.t


def _dgrad(ops, dev, case, tile, shift=0, refs=R):
    """Bitmask dgrad (+ skip operand) of the case's layer: Cout_p channels in, Cin_p out."""
    S, B, Cin, Cout, K, Pin = case
    s = _dgrad_setup(dev, case, refs)
    dx = Guarded((B, S + 2, S + 2, Cin), R.BF16_SENTINEL, BF, dev, shift)
    ops.conv_fwd(s["dzp"], s["wd"], None, dx.t, K, S, Pin, 1, mode=ops.MODE_MASKBITS, mbits=s["mbits"], tile=tile,
                 res=s.get("res"))
    torch.cuda.synchronize()
    ci = R.real_channels(case)[0]
    assert R.check_padded(dx.t, s["dx"], 1, R.BF16_SENTINEL) == []
    assert not R.interior(dx.t, 1, S)[..., ci:].any()
    assert dx.outside_untouched()
    return dx.t


def _dgrad_bf8(ops, dev, case, tile, shift=0, shift8=0):
    """conv_dgrad_bits_bf8: dx, its e5m2 copy (dx * 2^-4, ties occur) and the folded amax."""
    S, B, Cin, Cout, K, Pin = case
    s = _dgrad_setup(dev, case)
    dx = Guarded((B, S + 2, S + 2, Cin), R.BF16_SENTINEL, BF, dev, shift)
    dx8 = Guarded((B, S + 2, S + 2, Cin), BYTE_SENTINEL, torch.uint8, dev, shift8)
    amax = ops.fp8_amax_buffer(1, dev)[0]
    sc = torch.tensor([2.0 ** -4], device=dev)
    ops.conv_dgrad_bits_bf8(s["dzp"], s["wd"], dx.t, s["mbits"], dx8.t, sc, K, S, amax=amax, tile=tile)
    torch.cuda.synchronize()
    assert R.check_padded(dx.t, s["dx"], 1, R.BF16_SENTINEL) == []
    want8 = _cached(("want8", case), lambda: torch.from_numpy(
        fp8_ref.quantize((s["dx64"] * 2.0 ** -4).float().numpy(), "e5m2")))
    assert R.check_padded(dx8.t.cpu(), want8, 1, BYTE_SENTINEL) == []
    assert amax.view(torch.float32).max().item() == s["dx64"].abs().max().item()
    assert dx.outside_untouched() and dx8.outside_untouched()
    return dx.t, dx8.t


# ----------------------------------------------------------------------------- partial tiles
@pytest.mark.parametrize("tile", PARTIAL_TILES)
@pytest.mark.parametrize("case", PARTIAL_CASES, ids=R.case_id)
def test_partial_tile_forward(ops, cuda_device, case, tile):
    _forward(ops, cuda_device, case, tile)


@pytest.mark.parametrize("tile", PARTIAL_TILES)
@pytest.mark.parametrize("case", PARTIAL_CASES, ids=R.case_id)
def test_partial_tile_dgrad(ops, cuda_device, case, tile):
    _dgrad(ops, cuda_device, case, tile)


# the e5m2 copy's op takes the tile codes from 64 up
@pytest.mark.parametrize("tile", [t for t in PARTIAL_TILES if t >= 64])
@pytest.mark.parametrize("case", PARTIAL_CASES, ids=R.case_id)
def test_partial_tile_dgrad_bf8(ops, cuda_device, case, tile):
    _dgrad_bf8(ops, cuda_device, case, tile)


# ----------------------------------------------------------------------------- widths
@pytest.mark.parametrize("tile", WIDTH_TILES)
@pytest.mark.parametrize("case", WIDTH_CASES, ids=R.case_id)
def test_widths_forward(ops, cuda_device, case, tile):
    _forward(ops, cuda_device, case, tile)


@pytest.mark.parametrize("tile", WIDTH_TILES)
@pytest.mark.parametrize("case", [c for c in WIDTH_CASES if c in R.DGRAD_CASES], ids=R.case_id)
def test_widths_dgrad(ops, cuda_device, case, tile):
    _dgrad(ops, cuda_device, case, tile)


@pytest.mark.parametrize("case", [(19, 2, 160, 160, 3, 1), (13, 3, 128, 128, 3, 1), (19, 2, 64, 64, 3, 1)],
                         ids=R.case_id)
def test_widths_dgrad_bf8(ops, cuda_device, case):
    """The paired e5m2 words at NB = 5 (the narrow last block keeps its 4-byte store), 4 and 2."""
    _dgrad_bf8(ops, cuda_device, case, 386)


# ----------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("tile", (64, 388))
def test_output_8_bytes_off_a_16_byte_boundary(ops, cuda_device, tile):
    """y / dx as views 4 elements (8 bytes) into a 16-byte aligned allocation, the e5m2 bytes 4 bytes in:
    every result equals the oracle and so the aligned run, bit for bit."""
    case = PARTIAL_CASES[0]
    y0, mb0 = _forward(ops, cuda_device, case, tile)
    y1, mb1 = _forward(ops, cuda_device, case, tile, shift=4)
    assert y1.data_ptr() % 16 == 8 and y0.data_ptr() % 16 == 0
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16)) and torch.equal(mb0, mb1)
    dx0 = _dgrad(ops, cuda_device, case, tile)
    dx1 = _dgrad(ops, cuda_device, case, tile, shift=4)
    assert torch.equal(dx0.view(torch.int16), dx1.view(torch.int16))
    a0, b0 = _dgrad_bf8(ops, cuda_device, case, tile)
    a1, b1 = _dgrad_bf8(ops, cuda_device, case, tile, shift=4, shift8=4)
    assert b1.data_ptr() % 8 == 4
    assert torch.equal(a0.view(torch.int16), a1.view(torch.int16)) and torch.equal(b0, b1)


# ----------------------------------------------------------------------------- residual epilogue
def test_residual_tile_388(ops, cuda_device):
    """The skip-operand epilogue (unpaired stores, its row groups as before) on the compact-halo tile."""
    case = (19, 3, 192, 192, 3, 1)
    assert case in RR.CASES
    _forward(ops, cuda_device, case, 388, refs=RR)
    _dgrad(ops, cuda_device, case, 388, refs=RR)
