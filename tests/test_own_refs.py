"""CPU checks of the float64 oracles in own_refs.py, the references test_own_head_kernels.py holds the
ownership-head kernels to."""
import pytest
import torch

import head_refs as R
import own_refs as O

SMALL = [(8, 8, 3, 9), (192, 192, 7, 13), (160, 152, 7, 19)]


@pytest.mark.parametrize("C,C_real,B,S", SMALL)
def test_gradient_equals_autograd(C, C_real, B, S):
    """dlo is the gradient, with respect to the ownership logits, of
    grad_scale * sum_b valid_b w_b (1 / SS) sum_p (tanh(o) - t)^2."""
    c = O.own_case(C, C_real, B, S)
    gs = 1.0 / 48
    ref = O.own_ref(c.y, c.wo, c.bo, c.target, c.sym, c.valid, c.weight, gs)
    o = R.logits64(c.y, c.wo, c.bo).requires_grad_(True)
    t = O.move_rows(c.target.double(), c.sym, S)
    per = ((torch.tanh(o) - t) ** 2).mean(1)
    (gs * (per * c.valid.double() * c.weight.double()).sum()).backward()
    assert torch.allclose(o.grad, ref.dlo, rtol=1e-12, atol=1e-15)
    assert torch.allclose(per.detach(), ref.loss, rtol=1e-12, atol=0)
    assert bool((ref.dlo[c.valid == 0] == 0).all())


@pytest.mark.parametrize("s", range(8))
def test_loss_moves_with_the_board(s):
    """A target moved by a symmetry together with its board gives the same loss, and (t, sym = s) is
    the pre-moved target with sym = 0."""
    C, C_real, B, S = 8, 8, 3, 9
    c = O.own_case(C, C_real, B, S)
    sym = torch.full((B,), s, dtype=torch.int32)
    base = O.own_ref(c.y, c.wo, c.bo, c.target, None, None, None, 1.0)
    ym = O.move_board(c.y, sym)
    moved = O.own_ref(ym, c.wo, c.bo, c.target, sym, None, None, 1.0)
    assert torch.allclose(moved.loss, base.loss, rtol=1e-12, atol=0)
    assert torch.equal(moved.agree, base.agree)
    pre = O.own_ref(ym, c.wo, c.bo, O.move_rows(c.target, sym, S), None, None, None, 1.0)
    assert torch.equal(pre.dlo, moved.dlo)
    # the convention is pack_input's: a one-hot row lands on fwd[s][p]
    p = 2 * S + 5
    one = torch.zeros(1, S * S)
    one[0, p] = 1
    assert int(O.move_rows(one, sym[:1], S).argmax()) == int(O.symmetry_tables(S)[s, p])


def test_symmetry_tables_match_the_trainers():
    from alphago_amd.train.engine import apply_symmetry_dist, symmetry_tables

    for S in (9, 19):
        assert torch.equal(O.symmetry_tables(S), symmetry_tables(S))
    g = torch.Generator().manual_seed(3)
    d = torch.rand(8, 81, generator=g)
    sym = torch.arange(8, dtype=torch.int32)
    assert torch.equal(O.move_rows(d, sym, 9), apply_symmetry_dist(d, sym, symmetry_tables(9)))


@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
def test_sign_is_decided_in_the_reference(C, C_real, B, S):
    """Fewer than 1 % of a case's points have a float64 ownership within the ``own`` bound of 0: the
    agreement count of the kernel may differ from the reference only there."""
    c = O.own_case(C, C_real, B, S)
    ref = O.own_ref(c.y, c.wo, c.bo, c.target, c.sym, c.valid, c.weight, 1.0)
    near = O.near_zero_points(ref, O.own_bound(c.y, c.wo, c.bo))
    assert int(near.sum()) < 0.01 * near.numel()
    assert set(c.target.unique().tolist()) == {-1, 0, 1}


@pytest.mark.parametrize("C,C_real,B,S", SMALL)
def test_backward_add2_reference(C, C_real, B, S):
    """x - dz_in is the gradient of sum_p g1 (y . w1) + g2 (y . w2) with respect to y where y > 0, the
    dhead blocks the gradients with respect to (w, b)."""
    c = O.own_case(C, C_real, B, S)
    g = torch.Generator().manual_seed(C + S)
    g1 = torch.randn(B, S * S, generator=g)
    g2 = torch.randn(B, S * S, generator=g)
    dz_in = torch.randn(B, S, S, C, generator=g).to(torch.bfloat16)
    ref = O.backward_add2_ref(c.y, dz_in, g1, c.wv, g2, c.wo)
    y = c.y.double().requires_grad_(True)
    w1 = c.wv.double().requires_grad_(True)
    w2 = c.wo.double().requires_grad_(True)
    b1 = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    z1 = (torch.relu(y)[..., :C_real] * w1).sum(-1).flatten(1) + b1
    z2 = (torch.relu(y)[..., :C_real] * w2).sum(-1).flatten(1)
    ((z1 * g1.double()).sum() + (z2 * g2.double()).sum()).backward()
    assert torch.allclose(ref.x - dz_in.double(), y.grad, rtol=1e-12, atol=1e-15)
    assert torch.allclose(ref.dh1[:, :C_real].sum(0), w1.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(ref.dh2[:, :C_real].sum(0), w2.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(ref.dh1[:, C_real].sum(), b1.grad[0], rtol=1e-10, atol=1e-12)
