"""The soft-target policy head (head_soft.hip, op policy_head_soft) against a float64 autograd oracle
of its objective (soft_head_refs.py), and against the plain head on one-hot targets.

Tolerances are the project's own for this kernel family (_check_policy_train in
tests/test_head_kernels.py): loss rtol 1e-3 / atol 1e-4; dz max error under 1e-2 of the reference
max; dhead weight part under 1e-3 of the reference max, per board and summed; bias part 1e-4;
``correct`` equal; the dz border and the padded channels exactly 0.
"""
import pytest
import torch

import head_refs as R
import soft_head_refs as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


_DEV = {}


def _dev(c, dev):
    """A head case's tensors on the device, made once per case and written by no test."""
    if id(c) not in _DEV:
        y = c.y.to(dev)
        _DEV[id(c)] = (R.pad_nhwc(y), y, c.w.to(dev), c.b.to(dev), c.weight.to(dev))
    return _DEV[id(c)]


def _max_err(a, ref):
    return (a.double() - ref.double()).abs().max().item()


def _outputs(yp, B, Cr):
    """NaN-filled outputs; the dz border, which no head kernel writes, is zero as in the trainers."""
    dev = yp.device
    dz = torch.zeros_like(yp)
    dz[:, 1:-1, 1:-1] = float("nan")
    nan = float("nan")
    return (dz, torch.full((B,), nan, device=dev), torch.full((B,), nan, device=dev),
            torch.full((B, Cr + 1), nan, device=dev))


def _check(Cr, dz, loss, corr, dhead, ref):
    """_check_policy_train's comparisons; ``ref`` has loss, correct, dz (interior) and dhead."""
    assert bool(torch.isfinite(loss).all() and torch.isfinite(dhead).all() and torch.isfinite(dz.float()).all())
    err = _max_err(loss, ref.loss)
    print("loss max err %.3g" % err)
    assert torch.allclose(loss.double(), ref.loss.double(), rtol=1e-3, atol=1e-4), err
    assert torch.equal(corr.double(), ref.correct.double())
    dzi = dz[:, 1:-1, 1:-1]
    dzmax = max(ref.dz.abs().max().item(), 1e-6)
    print("dz max err / ref max %.3g" % (_max_err(dzi, ref.dz) / dzmax))
    assert _max_err(dzi, ref.dz) < 1e-2 * dzmax
    assert R.border_is_zero(dz)
    assert not bool((dzi[..., Cr:] != 0).any())
    wmax = max(ref.dhead[:, :Cr].abs().max().item(), 1e-6)
    print("dhead max err / ref max %.3g" % (_max_err(dhead[:, :Cr], ref.dhead[:, :Cr]) / wmax))
    assert _max_err(dhead[:, :Cr], ref.dhead[:, :Cr]) < 1e-3 * wmax
    smax = max(ref.dhead[:, :Cr].double().sum(0).abs().max().item(), 1e-6)
    assert _max_err(dhead[:, :Cr].double().sum(0), ref.dhead[:, :Cr].double().sum(0)) < 1e-3 * smax
    assert _max_err(dhead[:, Cr], ref.dhead[:, Cr]) < 1e-4
    assert abs(dhead[:, Cr].double().sum().item() - ref.dhead[:, Cr].double().sum().item()) < 1e-4


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("with_sym", [False, True])
@pytest.mark.parametrize("pass_col", [False, True])
@pytest.mark.parametrize("C,C_real,B,S", SR.SOFT_SHAPES)
def test_policy_head_soft_vs_fp64(ops, cuda_device, C, C_real, B, S, pass_col, with_sym, weighted):
    """Loss, top-1, dz and dhead of every launch variant against the fp64 oracle: dense, visit-count,
    one-hot, negative-entry, all-zero and (with the pass column) pass-only rows, with and without
    the per-board symmetry and the signed per-board weights.  Boards without board mass give
    loss == correct == dz == dhead == 0 exactly, out of NaN-filled outputs."""
    c = R.head_case(C, C_real, B, S, "uniform")
    yp, y, w, b, wt = _dev(c, cuda_device)
    T = S * S + (1 if pass_col else 0)
    td, sym, kind = SR.soft_targets(C, C_real, B, S, T, with_sym)
    td = td.to(cuda_device)
    sym = None if sym is None else sym.to(cuda_device)
    weight = wt if weighted else None
    gs = 1.0 / B
    dz, loss, corr, dhead = _outputs(yp, B, C_real)
    ops.policy_head_train_soft(yp, w, b, td, dz, loss, corr, dhead, S, gs, weight=weight, sym=sym)
    torch.cuda.synchronize()
    ref = SR.soft_policy_ref(y, w, b, td, sym, weight, gs)
    assert R.argmax_is_decided(ref.logits, R.logits_bound(y, w, b))
    # the targets' maxima are unique by construction, so fp32 keeps their place too
    qs = ref.q[ref.has].sort(1, descending=True).values
    assert bool((qs[:, 0] - qs[:, 1] > 1e-3).all())
    _check(C_real, dz, loss, corr, dhead, ref)
    none = ~ref.has
    expect = (kind == SR.ZERO) | ((kind == SR.PASS_ONLY) if pass_col else torch.zeros_like(kind, dtype=torch.bool))
    assert torch.equal(none.cpu(), expect) and bool(none.any())
    assert bool((loss[none] == 0).all()) and bool((corr[none] == 0).all())
    assert bool((dz[none].float() == 0).all()) and bool((dhead[none] == 0).all())
    if B > 3:
        assert 0 < corr.sum().item() < B  # both outcomes of the top-1 flag occur


@pytest.mark.parametrize("C,C_real,B,S", SR.SOFT_SHAPES)
def test_one_hot_soft_equals_plain_head(ops, cuda_device, C, C_real, B, S):
    """A one-hot distribution under ``sym`` against the plain head on pack_input's transformed
    target: the soft path's D4 convention is pack_input's.  The plain kernel's outputs are the
    reference (same tolerances; p_target is far from the plain loss's clip here)."""
    c = R.head_case(C, C_real, B, S, "uniform")
    yp, y, w, b, wt = _dev(c, cuda_device)
    SS = S * S
    g = torch.Generator().manual_seed(B + S)
    t = torch.randint(0, SS, (B,), generator=g, dtype=torch.int32).to(cuda_device)
    sym = SR.cycling_sym(B).to(cuda_device)
    tout = torch.full((B,), -7, dtype=torch.int32, device=cuda_device)
    planes = torch.zeros(B, 1, S, S, dtype=torch.uint8, device=cuda_device)
    x0 = torch.zeros(B, S + 2, S + 2, 8, dtype=torch.bfloat16, device=cuda_device)
    ops.pack_input(planes, x0, 1, sym=sym, target=t, target_out=tout)
    td = torch.zeros(B, SS, device=cuda_device)
    td[torch.arange(B, device=cuda_device), t.long()] = 1.0
    gs = 1.0 / B
    dz, loss, corr, dhead = _outputs(yp, B, C_real)
    ops.policy_head_train_soft(yp, w, b, td, dz, loss, corr, dhead, S, gs, weight=wt, sym=sym)
    dz0, loss0, corr0, dhead0 = _outputs(yp, B, C_real)
    ops.policy_head_train(yp, w, b, tout, dz0, loss0, corr0, dhead0, S, gs, weight=wt)
    torch.cuda.synchronize()
    # the transformed one-hot sits on the point target_out names
    q = SR.transformed(td, sym, S)
    assert torch.equal(q.argmax(1).to(torch.int32), tout) and bool((q.sum(1) == 1).all())
    from types import SimpleNamespace

    _check(C_real, dz, loss, corr, dhead,
           SimpleNamespace(loss=loss0, correct=corr0, dz=dz0[:, 1:-1, 1:-1], dhead=dhead0))


def test_policy_head_soft_refuses_bad_arguments(ops, cuda_device):
    """A distribution of the wrong width, dtype or device and a symmetry of the wrong dtype are
    refused on the host."""
    C, Cr, B, S = 8, 8, 3, 9
    c = R.head_case(C, Cr, B, S, "uniform")
    yp, y, w, b, wt = _dev(c, cuda_device)
    good = torch.full((B, S * S), 1.0 / (S * S), device=cuda_device)

    def run(td, sym=None):
        dz, loss, corr, dhead = _outputs(yp, B, Cr)
        ops.policy_head_train_soft(yp, w, b, td, dz, loss, corr, dhead, S, 1.0 / B, sym=sym)
        torch.cuda.synchronize()

    run(good, torch.zeros(B, dtype=torch.int32, device=cuda_device))  # the well-formed call passes
    for bad in (torch.zeros(B, S * S + 2, device=cuda_device), torch.zeros(B, S * S - 1, device=cuda_device),
                torch.zeros(B + 1, S * S, device=cuda_device), good.double(), good.cpu()):
        with pytest.raises(RuntimeError):
            run(bad)
    with pytest.raises(RuntimeError):
        run(good, torch.zeros(B, dtype=torch.int64, device=cuda_device))


@pytest.mark.parametrize("C,C_real,B,S", [(192, 192, 7, 19), (64, 64, 257, 9)])
def test_non_finite_targets_leave_finite_outputs(ops, cuda_device, C, C_real, B, S):
    """NaN entries count as 0 like negatives (the same bits as the row with zeros in their place); a
    row with an infinite entry has no loss: exact zeros.  No output is non-finite."""
    c = R.head_case(C, C_real, B, S, "uniform")
    yp, y, w, b, wt = _dev(c, cuda_device)
    td, _, _ = SR.soft_targets(C, C_real, B, S, S * S + 1, False)
    clean = td.to(cuda_device).clone()
    dirty = clean.clone()
    holes = torch.tensor([3, 40, S * S - 1], device=cuda_device)  # board 0: a dense row
    clean[0, holes] = 0.0
    dirty[0, holes] = float("nan")
    clean[1] = 0.0                     # board 1 (a visit-count row): an infinite entry -> no loss
    dirty[1, 5] = float("inf")
    outs = []
    for t in (clean, dirty):
        dz, loss, corr, dhead = _outputs(yp, B, C_real)
        ops.policy_head_train_soft(yp, w, b, t, dz, loss, corr, dhead, S, 1.0 / B, weight=wt)
        torch.cuda.synchronize()
        outs.append((dz, loss, corr, dhead))
    for a_, b_ in zip(*outs):
        assert bool(torch.isfinite(b_.float()).all())
        assert torch.equal(a_.view(torch.int16) if a_.dtype == torch.bfloat16 else a_.view(torch.int32),
                           b_.view(torch.int16) if b_.dtype == torch.bfloat16 else b_.view(torch.int32))
    dz, loss, corr, dhead = outs[1]
    assert loss[1].item() == 0 and corr[1].item() == 0 and not bool(dz[1].float().any()) and not bool(dhead[1].any())
    assert loss[0].item() > 0
