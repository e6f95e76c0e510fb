"""The kernels of the global pooling branch (csrc/kernels/gpool.hip) against torch expressions of their
definitions: gpool_fwd (exact on integer data, the derived fp32 bound on random data, run-to-run bits, both
modes), gpool_bias_add, gpool_bwd_fill, and the host checks.  Shapes: B in {1, 3}, S in {9, 19}, C in
{64, 192} -- one and several boards, two board sizes, 8 and 24 16-byte channel groups (64 and 21 pixel
groups per workgroup, the second one not dividing the thread count)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 9, 64), (3, 19, 192), (3, 9, 192), (1, 19, 64)]


def _padded(B, S, C, device, interior):
    """Zero-bordered NHWC bf16 (B, S + 2, S + 2, C) with the given (B, S, S, C) interior."""
    y = torch.zeros(B, S + 2, S + 2, C, dtype=torch.bfloat16, device=device)
    y[:, 1:S + 1, 1:S + 1] = interior.to(device=device, dtype=torch.bfloat16)
    return y


def _interior(y, S):
    return y[:, 1:S + 1, 1:S + 1].reshape(y.shape[0], S * S, y.shape[3])


def _inv(S):
    return torch.tensor(1.0 / (S * S), dtype=torch.float32)


def _first_argmax(flat):
    """(B, C) lowest pixel index among each column's maxima of a (B, NP, C) tensor."""
    NP = flat.shape[1]
    idx = torch.arange(NP, device=flat.device)[None, :, None].expand_as(flat)
    return torch.where(flat == flat.max(1, keepdim=True).values, idx, torch.full_like(idx, NP)).min(1).values


def _pool(y, S, full=True):
    from alphago_amd import ops

    B, C = y.shape[0], y.shape[3]
    if not full:
        return ops.gpool_fwd(y, torch.full((B, C), -7.0, device=y.device), None, S), None
    P = torch.full((B, 2, C), -7.0, device=y.device)
    a = torch.full((B, C), -7, dtype=torch.int32, device=y.device)
    ops.gpool_fwd(y, P, a, S)
    return P, a


@pytest.mark.parametrize("B,S,C", SHAPES)
def test_gpool_fwd_exact_on_integers(cuda_device, B, S, C):
    """Integer-valued bf16 data in [-16, 16]: every partial sum is an integer below 2^24, so the fp32 sum is
    exact in any order and must EQUAL torch's; so must sum * inv, the max and the lowest-index argmax."""
    g = torch.Generator().manual_seed(B * 100 + S)
    x = torch.randint(-16, 17, (B, S, S, C), generator=g).float()
    b = B - 1
    x[b, :, :, 0] = -3.0
    x[b, 2, 3, 0] = x[b, 7, 1, 0] = 16.0     # planted double maximum: pixel 2 S + 3 wins over 7 S + 1
    x[b, :, :, 1] = 0.0                      # an all-zero channel: max 0, argmax 0
    x[b, :, :, 2] = -16.0
    x[b, S - 1, S - 1, 2] = 5.0              # the maximum at the last pixel
    x[0, :, :, C - 1] = 4.0                  # all equal: pixel 0
    y = _padded(B, S, C, cuda_device, x)
    P, a = _pool(y, S)
    s, _ = _pool(y, S, full=False)
    torch.cuda.synchronize()
    flat = _interior(y, S).float()
    assert torch.equal(s, flat.sum(1))
    assert torch.equal(P[:, 0], flat.sum(1) * _inv(S).to(cuda_device))
    assert torch.equal(P[:, 1], flat.max(1).values)
    assert torch.equal(a.long(), _first_argmax(flat))
    assert a[b, 0].item() == 2 * S + 3 and a[b, 1].item() == 0 and P[b, 1, 1].item() == 0.0
    assert a[b, 2].item() == S * S - 1 and a[0, C - 1].item() == 0


@pytest.mark.parametrize("B,S,C", SHAPES)
def test_gpool_fwd_random_within_the_fp32_bound(cuda_device, B, S, C):
    """|sum - fp64 sum| <= 361 * 2^-24 * sum |x| per (b, c): (n - 1) u sum |x| bounds an fp32 sum of n <= 361
    terms in any order (u = 2^-24); max and argmax are exact whatever the data."""
    g = torch.Generator().manual_seed(7 + S + C)
    y = _padded(B, S, C, cuda_device, torch.randn(B, S, S, C, generator=g) * 3)
    P, a = _pool(y, S)
    s, _ = _pool(y, S, full=False)
    torch.cuda.synchronize()
    flat = _interior(y, S).double()
    err = (s.double() - flat.sum(1)).abs()
    bound = 361 * 2.0 ** -24 * flat.abs().sum(1)
    print("max |sum - fp64| / bound = %.3g" % (err / bound).max().item())
    assert bool((err <= bound).all())
    assert torch.equal(P[:, 1].double(), flat.max(1).values) and torch.equal(a.long(), _first_argmax(flat))
    # the two arms are one summation: the full mode's mean is the sum mode's sum times inv, and runs repeat
    assert torch.equal(P[:, 0], s * _inv(S).to(cuda_device))
    P2, a2 = _pool(y, S)
    s2, _ = _pool(y, S, full=False)
    torch.cuda.synchronize()
    assert torch.equal(P, P2) and torch.equal(a, a2) and torch.equal(s, s2)


@pytest.mark.parametrize("B,S,C", SHAPES)
def test_gpool_bias_add(cuda_device, B, S, C):
    from alphago_amd import ops

    g = torch.Generator().manual_seed(11 + S)
    skip = _padded(B, S, C, cuda_device, torch.randn(B, S, S, C, generator=g).abs())
    gate = (torch.randn(B, C, generator=g) * 0.7).to(cuda_device)
    out = torch.zeros_like(skip)
    ops.gpool_bias_add(skip, gate, out, S)
    ref = (skip.float() + gate[:, None, None, :]).bfloat16()
    assert torch.equal(out[:, 1:S + 1, 1:S + 1], ref[:, 1:S + 1, 1:S + 1])
    border = out.clone()
    border[:, 1:S + 1, 1:S + 1] = 0
    assert not bool(border.any())  # the borders of out are still all zero
    inplace = skip.clone()
    ops.gpool_bias_add(inplace, gate, inplace, S)
    torch.cuda.synchronize()
    assert torch.equal(inplace, out)


@pytest.mark.parametrize("B,S,C", SHAPES)
def test_gpool_bwd_fill(cuda_device, B, S, C):
    from alphago_amd import ops

    g = torch.Generator().manual_seed(13 + C)
    dp = torch.randn(B, 2, C, generator=g).to(cuda_device)
    dp[:, 1].masked_fill_(dp[:, 1] == 0, 1.0)
    a = torch.randint(0, S * S, (B, C), generator=g, dtype=torch.int32).to(cuda_device)
    a[0, 0], a[0, 1] = 0, S * S - 1
    out = torch.full((B, S + 2, S + 2, C), 9.0, dtype=torch.bfloat16, device=cuda_device)
    ops.gpool_bwd_fill(dp, a, out, S)
    torch.cuda.synchronize()
    hit = torch.arange(S * S, device=cuda_device)[None, :, None] == a[:, None, :].long()
    # two roundings: the fp32 product, then the fp32 sum (torch does not contract them)
    ref = (dp[:, 0][:, None, :] * _inv(S).to(cuda_device) + torch.where(hit, dp[:, 1][:, None, :], 0.0)).bfloat16()
    assert torch.equal(_interior(out, S), ref)
    border = out.clone()
    border[:, 1:S + 1, 1:S + 1] = 9.0
    assert bool((border == 9.0).all())  # borders untouched
    # the max gradient lands on exactly one pixel per (b, c)
    base = (dp[:, 0] * _inv(S).to(cuda_device)).bfloat16()
    differs = _interior(out, S) != base[:, None, :]
    assert bool((differs.sum(1) <= 1).all()) and not bool((differs & ~hit).any())


def test_host_checks(cuda_device):
    from alphago_amd import ops

    B, S, C = 2, 9, 64
    y = torch.zeros(B, S + 2, S + 2, C, dtype=torch.bfloat16, device=cuda_device)
    P = torch.zeros(B, 2, C, device=cuda_device)
    a = torch.zeros(B, C, dtype=torch.int32, device=cuda_device)
    gate = torch.zeros(B, C, device=cuda_device)
    bad = [
        lambda: ops.gpool_fwd(y.cpu(), P, a, S),
        lambda: ops.gpool_fwd(y, P.cpu(), a, S),
        lambda: ops.gpool_fwd(y.float(), P, a, S),
        lambda: ops.gpool_fwd(y, P.double(), a, S),
        lambda: ops.gpool_fwd(y, P, a.long(), S),
        lambda: ops.gpool_fwd(y, P[:, :1].contiguous(), a, S),
        lambda: ops.gpool_fwd(y, P, None, S),             # the sum mode writes (B, C)
        lambda: ops.gpool_fwd(y, gate, a, S),             # the full mode writes (B, 2, C)
        lambda: ops.gpool_fwd(y, P, a, S + 1),
        lambda: ops.gpool_fwd(y[:, :, :, :60].contiguous(), P[:, :, :60].contiguous(), a[:, :60].contiguous(), S),
        lambda: ops.gpool_bias_add(y.cpu(), gate, y, S),
        lambda: ops.gpool_bias_add(y, gate.half(), y, S),
        lambda: ops.gpool_bias_add(y, gate[:1], y, S),
        lambda: ops.gpool_bias_add(y, gate, y[:1], S),
        lambda: ops.gpool_bwd_fill(P.cpu(), a, y, S),
        lambda: ops.gpool_bwd_fill(P, a.float(), y, S),
        lambda: ops.gpool_bwd_fill(gate, a, y, S),
        lambda: ops.gpool_bwd_fill(P, a, y.float(), S),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail("case %d did not raise" % i)
    torch.cuda.synchronize()
