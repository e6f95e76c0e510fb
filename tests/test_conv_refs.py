"""CPU checks of tests/conv_refs.py: the fp64 oracles against nested-loop convolutions, the bitmask
encoder against hand-worked words, the value ranges of every case the GPU tests run, and the detection
power of the comparisons they make."""
import pytest
import torch
import torch.nn.functional as F

import conv_refs as R
import fp8_ref


# ----------------------------------------------------------------------------- oracles vs nested loops
def _tiny(seed, B=2, C=3, N=2, S=4, K=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (B, C, S, S), generator=g).double()
    w = torch.randint(-3, 4, (N, C, K, K), generator=g).double()  # asymmetric taps
    b = torch.randint(-8, 9, (N,), generator=g).double()
    dz = torch.randint(-3, 4, (B, N, S, S), generator=g).double()
    return x, w, b, dz


@pytest.mark.parametrize("K", [3, 5])
def test_oracles_match_nested_loops(K):
    x, w, b, dz = _tiny(K, K=K)
    assert not torch.equal(w, w.flip(2, 3))
    assert torch.equal(F.conv2d(x, w, b, padding=K // 2), R.naive_conv2d(x, w, b, K // 2))
    assert torch.equal(torch.nn.grad.conv2d_input(x.shape, w, dz, padding=K // 2), R.naive_dgrad(dz, w, K // 2))
    assert torch.equal(torch.nn.grad.conv2d_weight(x, w.shape, dz, padding=K // 2), R.naive_wgrad(x, dz, K, K // 2))


def test_single_tap_orientation():
    """One asymmetric tap: forward reads x at (i + kh - P, j + kw - P); dgrad scatters to the mirrored side."""
    x = torch.zeros(1, 1, 5, 5, dtype=torch.float64)
    x[0, 0, 2, 2] = 1.0
    w = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    w[0, 0, 0, 2] = 2.0  # kh = 0, kw = 2
    y = F.conv2d(x, w, None, padding=1)
    assert y[0, 0, 3, 1] == 2.0 and y.sum() == 2.0  # output (i, j) with i + 0 - 1 = 2, j + 2 - 1 = 2
    dx = torch.nn.grad.conv2d_input(x.shape, w, x, padding=1)
    assert dx[0, 0, 1, 3] == 2.0 and dx.sum() == 2.0
    assert torch.equal(dx, R.naive_dgrad(x, w, 1)) and torch.equal(y, R.naive_conv2d(x, w, None, 1))


def test_dgrad_equals_forward_with_expected_dgrad_pack():
    """The dgrad pack of ``expected_pack`` (flipped taps, transposed) turns the forward into the dgrad."""
    x, w, b, dz = _tiny(7)
    N, C, K, _ = w.shape
    _, wd = R.expected_pack(w, C, N)
    w_t = wd.double().view(K, K, C, N).permute(2, 3, 0, 1).contiguous()  # (C, N, kh, kw): a forward weight
    assert torch.equal(F.conv2d(dz, w_t, None, padding=1), torch.nn.grad.conv2d_input(x.shape, w, dz, padding=1))


def test_expected_pack_layout_and_padding():
    g = torch.Generator().manual_seed(3)
    w = torch.randint(-5, 6, (5, 3, 3, 3), generator=g).double()
    wf, wd = R.expected_pack(w, 64, 64)
    assert wf.shape == (9, 64, 64) and wd.shape == (9, 64, 64)
    assert wf[1 * 3 + 2, 4, 2] == w[4, 2, 1, 2]
    assert wd[(2 - 1) * 3 + (2 - 2), 2, 4] == w[4, 2, 1, 2]
    assert not wf[:, 5:].any() and not wf[:, :, 3:].any() and not wd[:, 3:].any() and not wd[:, :, 5:].any()
    assert R.packed(w, 160, 160).shape == (10, 160, 160) and not R.packed(w, 160, 160)[9].any()


# ----------------------------------------------------------------------------- bitmask layout
@pytest.mark.parametrize("C", [64, 128, 160, 192, 384])
def test_mbits_round_trip(C):
    g = torch.Generator().manual_seed(C)
    mask = torch.randint(0, 2, (2, 5, 5, C), generator=g).bool()
    words = R.encode_mbits(mask, C)
    assert words.dtype == torch.int32 and words.shape == (2, 7, 7, R.mbits_words(C))
    assert torch.equal(R.decode_mbits(words, C), mask)
    assert not words[R.border_mask(2, 5, 1, words.shape[3])].any()
    # every channel owns exactly one bit
    word, bit = R._bit_position(C)
    assert len({(int(a), int(b)) for a, b in zip(word, bit)}) == C
    full = R.encode_mbits(torch.ones(1, 1, 1, C, dtype=torch.bool), C)[0, 1, 1].long() & 0xFFFFFFFF
    assert torch.equal(full & R.mbits_unused(C), torch.zeros_like(full))
    assert torch.equal(full | R.mbits_unused(C), torch.full_like(full, 0xFFFFFFFF))


def test_mbits_hand_worked_words():
    """From the comment at ConvEpilogue: word by*8 + wn*4 + lane/16, bit 4i + r for channel
    nbase + 16i + r, nbase = by*BN + wn*BN/2 + 4*(lane/16)."""
    def words_of(C, channels):
        m = torch.zeros(1, 1, 1, C, dtype=torch.bool)
        m[..., channels] = True
        return R.encode_mbits(m, C)[0, 1, 1].tolist()

    # BN = 192: channel 0 -> word 0 bit 0; 17 = 0 + 16*1 + 1 -> word 0 bit 5; 95 = 12 + 16*5 + 3 -> word 3
    # bit 23; 100 = 96 + 4*1 + 0 -> wave half 1, lane group 1: word 5 bit 0
    assert words_of(192, [0, 17]) == [1 | 1 << 5, 0, 0, 0, 0, 0, 0, 0]
    assert words_of(192, [95, 100]) == [0, 0, 0, 1 << 23, 0, 1, 0, 0]
    # 384 channels: channel 192 + 100 sits in the second workgroup column's words 8..15
    assert words_of(384, [292])[13] == 1 and sum(words_of(384, [292])) == 1
    # BN = 160: halves of 80 channels, 20 bits per word; channel 151 = 80 + 4*1 + 16*4 + 3 -> word 5 bit 19
    assert words_of(160, [151]) == [0, 0, 0, 0, 0, 1 << 19, 0, 0]
    # BN = 128: channel 127 = 64 + 12 + 16*3 + 3 -> word 7 bit 15; BN = 64: channel 63 -> word 7 bit 7
    assert words_of(128, [127])[7] == 1 << 15
    assert words_of(64, [63])[7] == 1 << 7 and words_of(64, [31])[3] == 1 << 7


@pytest.mark.parametrize("C", [64, 128, 192, 384])
def test_mbits_32x32_epilogue_formula_is_the_layout(C):
    """ConvEpilogue32's comment (conv_common.h): its lane holds channel nbase + 32 i + 8 g + 4 h + r in bit
    8 i + 4 (g / 2) + r of word by*8 + wn*4 + h + 2 (g % 2) -- the same (word, bit) as the written layout."""
    bn = R.n_tile(C)
    word, bit = R._bit_position(C)
    seen = set()
    for by in range(C // bn):
        for wn in range(2):
            for i in range(bn // 64):
                for g in range(4):
                    for h in range(2):
                        for r in range(4):
                            c = by * bn + wn * (bn // 2) + 32 * i + 8 * g + 4 * h + r
                            assert (int(word[c]), int(bit[c])) == (by * 8 + wn * 4 + h + 2 * (g % 2),
                                                                  8 * i + 4 * (g // 2) + r)
                            seen.add(c)
    assert seen == set(range(C))


def test_mbits_word_counts_match_ops():
    from alphago_amd import ops

    for C in (64, 128, 160, 192, 256, 384):
        assert R.mbits_words(C) == ops.mbits_words(C) and R.n_tile(C) == ops.conv_n_tile(C)
    assert R.mbits_words(160) == 8 and R.mbits_words(384) == 16


# ----------------------------------------------------------------------------- conditions of every GPU case
@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_forward_case_in_range(case):
    c = R.fwd_case(case)  # asserts the conditions itself; stated again here
    S, B, Cin, Cout, K, Pin = case
    ci, co = R.real_channels(case)
    assert c["pre"].abs().max().item() <= R.MAX_ABS
    assert 0.3 <= (c["pre"][..., :co] > 0).double().mean().item() <= 0.7
    assert set(c["x"].unique().tolist()) <= {-1.0, 0.0, 1.0} and set(c["w"].unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert c["bias"].abs().max().item() <= 8 and c["bias"].dtype == torch.float32
    assert not c["x"][..., ci:].any() and not c["y"][..., co:].any() and not c["bias"][co:].any()
    assert torch.equal(c["y"].double(), c["pre"].clamp_min(0))
    # twice the values (the fp8 runs with a non-trivial exponent pair) are still exact in bf16
    assert torch.equal((2 * c["pre"]).to(torch.bfloat16).double(), 2 * c["pre"])


@pytest.mark.parametrize("case", R.DGRAD_CASES + [c for c in R.FP8_SQUARE_CASES if c not in R.DGRAD_CASES],
                         ids=R.case_id)
def test_dgrad_case_in_range(case):
    c = R.dgrad_case(case)
    ci, co = R.real_channels(case)
    assert c["raw"].abs().max().item() <= R.MAX_ABS
    assert 0.3 <= c["mask"][..., :ci].double().mean().item() <= 0.7
    assert not c["dx"][..., ci:].any() and not c["mask"][..., ci:].any()
    assert not torch.signbit(c["dx"][~c["mask"]]).any()  # masked elements are +0
    assert torch.equal(c["dx"].to(torch.bfloat16).double(), c["dx"])
    act = R.mask_activation(c["mask"])
    assert (act == 0).any() and torch.signbit(act[act == 0]).any() and (act < 0).any()


@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_wgrad_case_in_range(case):
    c = R.wgrad_case(case)
    S, B = case[0], case[1]
    assert c["x"].abs().max().item() <= 4 and c["dz"].abs().max().item() <= 4
    assert B * S * S * 16 < R.MAX_WGRAD and c["dw"].abs().max().item() < R.MAX_WGRAD
    for fmt, dt in (("e4m3", torch.float8_e4m3fn), ("e5m2", torch.float8_e5m2)):  # exact in both byte formats
        v = torch.arange(-4, 5).float()
        assert torch.equal(v.to(dt).float(), v)
        assert [fp8_ref.decode(fmt, b) for b in fp8_ref.quantize(v.numpy(), fmt)] == v.tolist()
    g0 = R.wgrad_g0(case, "w")
    assert torch.equal(R.combine(g0, c["dw"], 0.5, 2.0).double(), 2.0 * g0 + 0.5 * c["dw"])


@pytest.mark.parametrize("case", R.IMPULSE_CASES, ids=R.case_id)
def test_impulse_cases(case):
    S, B, Cin, Cout, K, Pin = case
    f, d = R.impulse_fwd_case(case), R.impulse_dgrad_case(case)
    P = K // 2
    # the centre impulse of board 0: output pixel (c + P - kh, c + P - kw) sees weight 1 + kh K + kw, twice
    # (channels 0 and cin_real - 1); the dgrad sees the mirrored tap
    c = S // 2
    for kh in range(K):
        for kw in range(K):
            assert f["pre"][0, c + P - kh, c + P - kw, 0] == 2 * (1 + kh * K + kw)
            assert d["dx"][0, c - P + kh, c - P + kw, 0] == 2 * (1 + kh * K + kw)
    assert f["pre"][0, 0, 0, 0] == 2 * (1 + P * K + P)  # corner: only the taps inside the board


# ----------------------------------------------------------------------------- detection power
CASE = (9, 5, 192, 192, 3, 1)


def _padded_oracle():
    f = R.fwd_case(CASE)
    return f, R.place(f["y"], 1, torch.bfloat16, R.BF16_SENTINEL)


def test_comparison_passes_on_the_oracle():
    f, got = _padded_oracle()
    assert R.check_padded(got, f["y"], 1, R.BF16_SENTINEL) == []
    mb = R.encode_mbits(f["mask"], 192)
    mb[R.border_mask(5, 9, 1, 8)] = R.MBITS_SENTINEL
    assert R.check_mbits(mb.flatten(), f["mask"], 192) == []


def test_detects_one_dropped_tap_at_one_pixel():
    f, got = _padded_oracle()
    S, B, Cin, Cout, K, Pin = CASE
    xp = R.place(f["x"], 1, torch.float64)
    # a pixel / channel / tap whose product is nonzero and whose output is positive with and without it
    w = f["w"]
    for b, i, j, n in ((b, i, j, n) for b in range(B) for i in range(S) for j in range(S) for n in range(Cout)):
        prod = xp[b, i + 2, j + 1, 0] * w[n, 0, 2, 1]  # tap (kh, kw) = (2, 1), input channel 0
        if prod != 0 and f["pre"][b, i, j, n] > 1:
            got[b, i + 1, j + 1, n] = float(f["pre"][b, i, j, n] - prod)
            break
    assert R.check_padded(got, f["y"], 1, R.BF16_SENTINEL) == ["interior"]


def test_detects_one_dropped_channel_group():
    f, got = _padded_oracle()
    S, B, Cin, Cout, K, Pin = CASE
    x = f["x"].permute(0, 3, 1, 2).clone()
    x[1, 8:16, 4, 4] = 0  # one 8-channel group of one input pixel
    assert f["x"][1, 4, 4, 8:16].any()
    y2 = F.conv2d(x, f["w"], f["bias"].double(), padding=1).clamp_min(0)
    got = R.place(R.nhwc(y2, Cout), 1, torch.bfloat16, R.BF16_SENTINEL)
    assert R.check_padded(got, f["y"], 1, R.BF16_SENTINEL) == ["interior"]


def test_detects_unwritten_last_pixel():
    f, got = _padded_oracle()
    got[-1, 9, 9] = R.BF16_SENTINEL  # the last pixel of the batch left as it was
    assert R.check_padded(got, f["y"], 1, R.BF16_SENTINEL) == ["interior"]
    mb = R.encode_mbits(f["mask"], 192)
    mb[R.border_mask(5, 9, 1, 8)] = R.MBITS_SENTINEL
    mb[-1, 9, 9] = R.MBITS_SENTINEL
    assert "bits" in R.check_mbits(mb.flatten(), f["mask"], 192)


def test_detects_bitmask_shifted_by_one_word():
    f, _ = _padded_oracle()
    mb = R.encode_mbits(f["mask"], 192)
    mb[R.border_mask(5, 9, 1, 8)] = R.MBITS_SENTINEL
    shifted = torch.roll(mb.flatten(), 1)
    assert "bits" in R.check_mbits(shifted, f["mask"], 192)
    # and one wrong bit of one word
    one = mb.clone()
    one[2, 3, 4, 5] ^= 1 << 7
    assert R.check_mbits(one.flatten(), f["mask"], 192) == ["bits"]
    # a bit no channel owns
    stray = mb.clone()
    stray[2, 3, 4, 5] |= 1 << 30
    assert R.check_mbits(stray.flatten(), f["mask"], 192) == ["unused bits"]


@pytest.mark.parametrize("where", [(0, 0, 3), (2, 10, 5), (4, 6, 0), (1, 4, 10)])
def test_detects_border_element_overwritten(where):
    f, got = _padded_oracle()
    b, i, j = where  # one element on each of the four borders
    got[b, i, j, 17] = 0.0
    assert R.check_padded(got, f["y"], 1, R.BF16_SENTINEL) == ["border"]
    mb = R.encode_mbits(f["mask"], 192)
    mb[R.border_mask(5, 9, 1, 8)] = R.MBITS_SENTINEL
    mb[b, i, j, 3] = 0
    assert R.check_mbits(mb.flatten(), f["mask"], 192) == ["border words"]


def test_detects_one_dropped_wgrad_pixel():
    """One pixel of one split missing from dW: an exact comparison sees the single product."""
    c = R.wgrad_case(CASE)
    S, B, Cin, Cout, K, Pin = CASE
    x, dz = c["x"].permute(0, 3, 1, 2).clone(), c["dz"].permute(0, 3, 1, 2)
    assert dz[B - 1, :, S - 1, S - 1].any() and x[B - 1, :, S - 1, S - 1].any()
    x2 = x.clone()
    x2[B - 1, :, S - 1, S - 1] = 0
    dw2 = torch.nn.grad.conv2d_weight(x2, c["dw"].shape, dz.contiguous(), padding=1)
    assert not torch.equal(dw2.float(), c["dw"].float())
