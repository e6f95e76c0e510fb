"""Integer oracles for the two skip-operand epilogues of the conv kernels (residual blocks), in the style
of tests/conv_refs.py, whose operands they reuse.

Forward (MODE_BIAS_RELU with ``res``): y = bf16(relu(conv + bias + res)), ReLU' bit = (y > 0).
Bitmask dgrad (MODE_MASKBITS with ``res``): dx = (conv_input + res) where the mask is set, +0 elsewhere.

The conv operands are ``conv_refs.fwd_case`` / ``dgrad_case`` (ternary activations and weights, small
integer bias).  The forward skip holds integers in [0, 32] on a random half of the elements and 0
elsewhere (a block input is a ReLU output: non-negative), the dgrad skip is ternary; padded channels are
zero.  Every sum stays an exact integer with |.| <= conv_refs.MAX_ABS, so the kernels must match with
``torch.equal`` whatever their tiling, K order or split count.

Two more conditions keep the forward cases meaningful and are asserted per case:
  * the positive share of pre + res lies in [0.3, 0.7];
  * at least 5 % of the elements have (pre > 0) != (pre + res > 0): a kernel that adds the skip to the
    value but not to the ReLU' bit, or the other way round, cannot pass.
Everything runs on the CPU from seeded generators."""
import functools

import torch

import conv_refs as R

# (S, B, Cin_p, Cout_p, K, Pin): F -> F 3x3 layers, the shapes a residual block's last layer has
CASES = [
    (19, 1, 192, 192, 3, 1),   # M = 361: one partial tile of every large tile
    (19, 3, 192, 192, 3, 1),   # M = 1083: partial last tiles, tiles that start mid-row
    (9, 5, 192, 192, 3, 1),    # a tile spans five boards
    (19, 2, 160, 160, 3, 1),   # 152 real channels in 160, straddled K-steps
    (19, 2, 64, 64, 3, 1),     # the 64-wide N tile
]
MIN_FLIPS = 0.05
RES_MAX = 32


def _real(t_nhwc, c_real):
    return t_nhwc[..., :c_real]


def fwd_conditions(case):
    """(positive share of pre + res, share of elements whose sign test the skip flips, max |pre + res|)
    over the real output channels."""
    c = fwd_case(case)
    co = R.real_channels(case)[1]
    pre, tot = _real(c["pre"], co), _real(c["pre"] + c["res"], co)
    return ((tot > 0).double().mean().item(), ((pre > 0) != (tot > 0)).double().mean().item(),
            tot.abs().max().item())


@functools.lru_cache(maxsize=None)
def fwd_case(case):
    """conv_refs.fwd_case plus ``res`` (fp64 NHWC, Cout_p channels) and the oracle of the skip epilogue:
    ``y`` (bf16) = relu(pre + res), ``mask`` = y > 0.  ``pre`` stays the conv's own pre-activation."""
    S, B, Cin, Cout, K, Pin = case
    co = R.real_channels(case)[1]
    base = R.fwd_case(case)
    g = R._gen(case, 6)
    vals = R._ints((B, S, S, co), 0, RES_MAX, g)
    on = torch.randint(0, 2, (B, S, S, co), generator=g).bool()
    res = R._pad_last(torch.where(on, vals, torch.zeros_like(vals)), Cout)
    tot = base["pre"] + res
    R._check_range("pre + res " + R.case_id(case), tot)
    y = tot.clamp_min(0)
    y_bf = y.to(torch.bfloat16)
    assert torch.equal(y_bf.double(), y)
    out = dict(base)
    out.update(res=res, y=y_bf, mask=y > 0)
    share = (_real(tot, co) > 0).double().mean().item()
    flips = ((_real(base["pre"], co) > 0) != (_real(tot, co) > 0)).double().mean().item()
    assert 0.3 <= share <= 0.7, "%s: positive share %.3f of pre + res outside [0.3, 0.7]" % (R.case_id(case), share)
    assert flips >= MIN_FLIPS, "%s: the skip flips %.3f of the sign tests, below %.2f" % (R.case_id(case), flips,
                                                                                       MIN_FLIPS)
    assert not out["y"][..., co:].any() and not out["res"][..., co:].any()
    return out


@functools.lru_cache(maxsize=None)
def dgrad_case(case):
    """conv_refs.dgrad_case plus a ternary ``res`` (fp64 NHWC, Cin_p channels: the dgrad's output width)
    and ``dx`` = (raw + res) under the mask, +0 where it is off."""
    S, B, Cin, Cout, K, Pin = case
    ci = R.real_channels(case)[0]
    base = R.dgrad_case(case)
    g = R._gen(case, 7)
    res = R._pad_last(R._ternary((B, S, S, ci), g), Cin)
    tot = base["raw"] + res
    R._check_range("dx + res " + R.case_id(case), tot)
    dx = torch.where(base["mask"], tot, torch.zeros_like(tot))
    assert torch.equal(dx.to(torch.bfloat16).double(), dx)
    # the skip must show: a kernel that drops it, or adds it after the mask, differs on many elements
    seen = (base["mask"] & (res != 0)).double().mean().item()
    leak = (~base["mask"] & (res != 0))[..., :ci].double().mean().item()
    assert seen >= MIN_FLIPS and leak >= MIN_FLIPS
    out = dict(base)
    out.update(res=res, dx=dx)
    return out


def res_buffer(res_nhwc, dtype=torch.bfloat16):
    """The skip operand as the kernels read it: padded NHWC with border 1 whose border pixels are NaN, so
    a read of a border pixel shows in the interior of the output."""
    return R.place(res_nhwc, 1, dtype, fill=float("nan"))
