"""D4 symmetry ensembling on the GPU: the kernels of csrc/kernels/symmetry.hip (d4_expand,
policy_head_d4, group_mean) and the HIP engines' symmetries="random" / "all" modes.

Definition (models/inference.py): symmetry s is pack_input's, fwd_s = symmetry_tables(S)[s];
policy = 1/G sum_g P_s[fwd_s(p)], value = 1/G sum_g V(board under s), G = 8 ("all", s_g = g) or 1.

Bounds: ``head_bound(G) = 1e-5 + G * 2^-24`` -- 1e-5 is the bound of policy_head_probs against float64
(test_head_kernels.test_policy_head_probs_temperature); a mean of G such terms cannot exceed it, and
the fp32 sum over g adds at most G * 2^-24.  Engine tests compare with the plain engine run on the
explicitly transformed boards in the same batch positions (same kernels, same plans, same inputs),
mapped back and averaged in float64, under the same bound.
"""
import numpy as np
import pytest
import torch

import head_refs as R
from alphago_amd.train.engine import symmetry_tables

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
_TABLES = {}


def head_bound(G):
    return 1e-5 + G * U24


def table(S):
    if S not in _TABLES:
        _TABLES[S] = symmetry_tables(S)
    return _TABLES[S]  # (8, S*S) long, fwd[s][p]


def transform(a, s, S):
    """(..., S*S) numpy array, original frame -> frame of symmetry s: out[fwd[p]] = a[p]."""
    out = np.empty_like(a)
    out[..., table(S)[s].numpy()] = a
    return out


def back(a, s, S):
    return a[..., table(S)[s].numpy()]


def t_planes(planes, s, S):
    n, c = planes.shape[:2]
    return transform(planes.reshape(n, c, S * S), s, S).reshape(planes.shape)


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


def roughen(net, std):
    """Weights large enough for the outputs to depend visibly on the orientation."""
    with torch.no_grad():
        for p in net.parameters():
            p.normal_(0.0, std)
    return net


# ------------------------------------------------------------------------------------ 1. d4_expand
def _expand_ref(src, sym, S, P):
    """Torch index gather: dst[k] interior, flat point q <- src[k % B] interior, flat point inv_s[q]."""
    B, Cp = src.shape[0], src.shape[3]
    fwd = table(S).to(src.device)[sym.long()]
    inv = torch.argsort(fwd, dim=1)
    inter = src[:, P:P + S, P:P + S].reshape(B, S * S, Cp)
    rows = torch.arange(sym.numel(), device=src.device) % B
    return torch.gather(inter[rows], 1, inv.unsqueeze(2).expand(-1, -1, Cp)).reshape(-1, S, S, Cp)


@pytest.mark.parametrize("S,P,Cp,B", [(19, 2, 64, 3), (19, 1, 64, 2), (13, 2, 64, 2), (9, 1, 64, 3), (9, 1, 128, 2)])
def test_d4_expand_bit_exact(ops, cuda_device, S, P, Cp, B):
    dev = cuda_device
    g = torch.Generator().manual_seed(S * 100 + P * 10 + B)
    cases = [(B, torch.arange(8, dtype=torch.int32).repeat_interleave(B)),  # G = 8, sym = g
             (8, torch.tensor([5, 0, 3, 7, 1, 6, 2, 4], dtype=torch.int32))]  # G = 1, every symmetry
    for Bs, sym in cases:
        sym = sym.to(dev)
        GB = sym.numel()
        src = ops.padded_empty(Bs, S, P, Cp, dev)
        src[:, P:P + S, P:P + S] = torch.randn(Bs, S, S, Cp, generator=g).to(torch.bfloat16).to(dev)
        dst = ops.padded_empty(GB, S, P, Cp, dev)
        ops.d4_expand(src, dst, sym, S, P)
        torch.cuda.synchronize()
        assert torch.equal(dst[:, P:P + S, P:P + S], _expand_ref(src, sym, S, P))
        border = dst.clone()
        border[:, P:P + S, P:P + S] = 0
        assert not bool(border.view(torch.int16).any())
        if Cp == 64:  # the training augmentation's convention: pack_input with the same sym
            planes = torch.randint(0, 2, (Bs, 48, S, S), dtype=torch.uint8, generator=g).to(dev)
            one = ops.pack_input(planes, ops.padded_empty(Bs, S, P, Cp, dev), P)
            rows = (torch.arange(GB, device=dev) % Bs).long()
            want = ops.pack_input(planes, ops.padded_empty(GB, S, P, Cp, dev), P, sym=sym, rows=rows)
            got = ops.d4_expand(one, ops.padded_empty(GB, S, P, Cp, dev), sym, S, P)
            torch.cuda.synchronize()
            assert torch.equal(got, want)


def test_d4_expand_refuses_bad_arguments(ops, cuda_device):
    dev = cuda_device
    src = ops.padded_empty(2, 9, 1, 64, dev)
    sym = torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):  # dst not a multiple of src's boards
        ops.d4_expand(src, ops.padded_empty(3, 9, 1, 64, dev), sym[:3], 9, 1)
    with pytest.raises(RuntimeError):  # sym length
        ops.d4_expand(src, ops.padded_empty(4, 9, 1, 64, dev), sym[:3], 9, 1)
    with pytest.raises(RuntimeError):  # geometry
        ops.d4_expand(src, ops.padded_empty(4, 9, 2, 64, dev), sym, 9, 1)
    with pytest.raises(RuntimeError):  # host tensor
        ops.d4_expand(src, ops.padded_empty(4, 9, 1, 64, dev), sym.cpu(), 9, 1)
    with pytest.raises(RuntimeError):  # sym dtype
        ops.d4_expand(src, ops.padded_empty(4, 9, 1, 64, dev), sym.long(), 9, 1)


# ------------------------------------------------------------------------- 2. policy_head_probs_d4
def _legal(kind, B, SS, seed):
    if kind == "none":
        return None
    legal = (torch.rand(B, SS, generator=torch.Generator().manual_seed(seed)) > 0.5).to(torch.uint8)
    if kind == "edges":
        legal[1] = 0  # no legal point: the row is exactly 0
        legal[0] = 0
        legal[0, SS // 3] = 1  # one legal point: exactly 1.0 there
    return legal


@pytest.mark.parametrize("kind", ["none", "half", "edges"])
@pytest.mark.parametrize("T", [1.0, 0.5])
@pytest.mark.parametrize("G,scratch", [(1, False), (8, False), (8, True)])
@pytest.mark.parametrize("C,C_real,B,S", [(192, 192, 3, 19), (160, 152, 3, 19), (192, 192, 3, 13), (8, 8, 2, 9),
                                          (64, 64, 33, 9)])
def test_policy_head_probs_d4_vs_fp64(ops, cuda_device, C, C_real, B, S, G, scratch, T, kind):
    """``scratch``: with the (G*B, S*S) buffer these batches (B < 128) take the small-batch path, one
    workgroup per orientation and a group_mean pass; without it, one workgroup per position."""
    dev = cuda_device
    SS = S * S
    c = R.head_case(C, C_real, max(G * B, 3), S, "uniform")  # head_case builds at least 3 boards
    y = c.y[:G * B]
    sym = torch.arange(G * B) // B if G == 8 else (torch.arange(B) * 3 + 1) % 8  # G = 1: mixed symmetries
    legal = _legal(kind, B, SS, 7 * B + S)
    # float64 reference from the definition
    z = R.logits64(y, c.w, c.b) / T  # (G*B, SS), each row in its transformed frame
    zo = torch.gather(z, 1, table(S)[sym])  # original frame: z_s[fwd_s(p)]
    if legal is not None:
        zo = zo.masked_fill(legal.repeat(G, 1) == 0, float("-inf"))
    p = torch.nan_to_num(torch.softmax(zo, 1), nan=0.0)  # an all-illegal row is 0
    ref = p.view(G, B, SS).sum(0) / G

    probs = torch.full((B, SS), float("nan"), device=dev)
    ops.policy_head_probs_d4(R.pad_nhwc(y.to(dev)), c.w.to(dev), c.b.to(dev), probs, S, sym.to(torch.int32).to(dev), G,
                             legal=legal.to(dev) if legal is not None else None, temperature=T,
                             scratch=torch.full((G * B, SS), float("nan"), device=dev) if scratch else None)
    torch.cuda.synchronize()
    out = probs.cpu()
    assert bool(torch.isfinite(out).all())
    err = (out.double() - ref).abs().max().item()
    print("policy_head_probs_d4 %s G=%d scratch=%s T=%g %s: max err %.3g (bound %.3g)"
          % ((C, C_real, B, S), G, scratch, T, kind, err, head_bound(G)))
    assert err <= head_bound(G)
    live = torch.ones(B, dtype=torch.bool)
    if legal is not None:
        assert not bool((out * (legal == 0)).abs().max() > 0)  # illegal points are exactly 0
        live = legal.sum(1) > 0
    assert ((out.double().sum(1) - 1.0).abs()[live] <= SS * U24 + 1e-5).all()
    if kind == "edges":
        assert out[1].abs().max().item() == 0
        assert out[0, SS // 3].item() == 1.0


def test_policy_head_probs_d4_many_positions(ops, cuda_device):
    """B = 130 >= 128 positions: the per-position kernel runs with or without scratch (same bits), on
    the 512-thread row mapping (G * B >= 256)."""
    dev = cuda_device
    C, B, S, G = 64, 130, 9, 8
    SS = S * S
    c = R.head_case(C, C, G * B, S, "uniform")
    sym = torch.arange(G * B) // B
    legal = _legal("edges", B, SS, 11)
    zo = torch.gather(R.logits64(c.y, c.w, c.b), 1, table(S)[sym]).masked_fill(legal.repeat(G, 1) == 0, float("-inf"))
    ref = torch.nan_to_num(torch.softmax(zo, 1), nan=0.0).view(G, B, SS).sum(0) / G
    yp, w, b, symd, ld = R.pad_nhwc(c.y.to(dev)), c.w.to(dev), c.b.to(dev), sym.to(torch.int32).to(dev), legal.to(dev)
    a = ops.policy_head_probs_d4(yp, w, b, torch.full((B, SS), float("nan"), device=dev), S, symd, G, legal=ld)
    a2 = ops.policy_head_probs_d4(yp, w, b, torch.full((B, SS), float("nan"), device=dev), S, symd, G, legal=ld,
                                  scratch=torch.empty(G * B, SS, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(a, a2)
    assert (a.cpu().double() - ref).abs().max().item() <= head_bound(G)
    assert a[1].abs().max().item() == 0 and a[0, SS // 3].item() == 1.0
    with pytest.raises(RuntimeError):  # scratch too small
        ops.policy_head_probs_d4(yp, w, b, torch.empty(B, SS, device=dev), S, symd, G, scratch=torch.empty(B, SS, device=dev))


def test_policy_head_probs_d4_is_deterministic_and_checks(ops, cuda_device):
    dev = cuda_device
    C, B, S, G = 64, 33, 9, 8
    c = R.head_case(C, C, G * B, S, "uniform")
    yp, w, b = R.pad_nhwc(c.y.to(dev)), c.w.to(dev), c.b.to(dev)
    sym = (torch.arange(G * B) // B).to(torch.int32).to(dev)
    a = ops.policy_head_probs_d4(yp, w, b, torch.empty(B, S * S, device=dev), S, sym, G)
    a2 = ops.policy_head_probs_d4(yp, w, b, torch.empty(B, S * S, device=dev), S, sym, G)
    torch.cuda.synchronize()
    assert torch.equal(a, a2)
    with pytest.raises(RuntimeError):  # sym length != G * B
        ops.policy_head_probs_d4(yp, w, b, torch.empty(B, S * S, device=dev), S, sym[:B], G)
    with pytest.raises(RuntimeError):  # y does not hold G * B boards
        ops.policy_head_probs_d4(yp, w, b, torch.empty(B + 1, S * S, device=dev), S, sym, G)
    with pytest.raises(RuntimeError):  # more weights than channels
        ops.policy_head_probs_d4(yp, torch.zeros(C + 8, device=dev), b, torch.empty(B, S * S, device=dev), S, sym, G)
    with pytest.raises(RuntimeError):  # host tensor
        ops.policy_head_probs_d4(yp, w, b, torch.empty(B, S * S, device=dev), S, sym.cpu(), G)


# ----------------------------------------------------------------------------------- 3. group_mean
@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("B", [1, 5, 257])
def test_group_mean_bit_exact(ops, cuda_device, B, G):
    v = (torch.rand(G * B, generator=torch.Generator().manual_seed(B + G)) * 2 - 1).to(cuda_device)
    out = torch.full((B,), float("nan"), device=cuda_device)
    ops.group_mean(v, out, G)
    ref = torch.zeros(B, device=cuda_device)
    for g in range(G):
        ref = ref + v[g * B:(g + 1) * B]
    ref = ref * torch.tensor(np.float32(1.0 / G), device=cuda_device)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    with pytest.raises(RuntimeError):
        ops.group_mean(v, torch.empty(B + 1, device=cuda_device), G)


# ------------------------------------------------------------------------- 4. engine, planes path
NB, SB, CB = 4, 9, 12  # positions, board, planes of the small engine tests


def _boards(seed, n=NB, S=SB, C=CB):
    rng = np.random.default_rng(seed)
    return (rng.random((n, C, S, S)) < 0.4).astype(np.uint8), (rng.random((n, S * S)) < 0.6).astype(np.uint8)


def _fanned(planes, legal, syms, S):
    """The G * n explicitly transformed boards and masks in trunk order k = g * n + b."""
    xs = [t_planes(planes[b:b + 1], int(s), S) for row in syms for b, s in enumerate(row)]
    ls = [transform(legal[b:b + 1], int(s), S) for row in syms for b, s in enumerate(row)]
    return np.concatenate(xs), np.concatenate(ls)


def _policy_oracle(plain, planes, legal, syms, S, pad_to=None):
    """float64 mean over g of the plain engine's rows (boards in trunk order), mapped back."""
    G, n = syms.shape
    x, l = _fanned(planes, legal, syms, S)
    p = plain.evaluate(x, l).double().cpu().numpy()
    acc = np.zeros((n, S * S))
    for g in range(G):
        for b in range(n):
            acc[b] += back(p[g * n + b], int(syms[g, b]), S)
    return acc / G


ALL4 = np.repeat(np.arange(8)[:, None], NB, 1)


@pytest.mark.parametrize("precision,use_graphs", [("bf16", True), ("bf16", False), ("fp8", True)])
def test_engine_all_planes_path(cuda_device, monkeypatch, precision, use_graphs):
    from alphago_amd.models.inference import HipTrunkInference
    from alphago_amd.models.nets import PolicyNet

    monkeypatch.setenv("ALPHAGO_AMD_FP8_MIN_BATCH", "8")
    torch.manual_seed(5)
    net = roughen(PolicyNet(CB, board=SB, filters_per_layer=32, layers=3), 0.1).to(cuda_device)
    eng = HipTrunkInference(net, cuda_device, buckets=(NB,), use_graphs=use_graphs, precision=precision,
                            symmetries="all")
    plain = HipTrunkInference(net, cuda_device, buckets=(8 * NB,), use_graphs=use_graphs, precision=precision)
    for seed in (1, 2):  # the second submission: nothing from the capture is stale
        planes, legal = _boards(seed)
        out = eng.evaluate(planes, legal).clone()
        again = eng.evaluate(planes, legal).clone()
        assert torch.equal(out, again)
        ref = _policy_oracle(plain, planes, legal, ALL4, SB)
        err = np.abs(out.double().cpu().numpy() - ref).max()
        print("engine all %s graphs=%s submission %d: max err %.3g" % (precision, use_graphs, seed, err))
        assert err <= head_bound(8)
        assert np.all(out.cpu().numpy()[legal == 0] == 0)
        assert eng.last_symmetries().shape == (8, NB)
        if precision == "fp8":  # both engines calibrated on the same 32 boards: same scales
            assert eng.ex == plain.ex
    one = plain.evaluate(planes, legal)[:NB].double().cpu().numpy()
    assert np.abs(one - ref).max() > 1e-3  # the ensemble differs from the single orientation


@pytest.mark.parametrize("t", [1, 4, 6, 7])
def test_engine_all_is_equivariant(cuda_device, t):
    """"all" on the board moved by t is the "all" output moved by t, within 2 G 2^-24: the G trunk rows
    are the same boards in another order, so only the order of the fp32 sum over g differs."""
    from alphago_amd.models.inference import HipTrunkInference
    from alphago_amd.models.nets import PolicyNet

    torch.manual_seed(5)
    net = roughen(PolicyNet(CB, board=SB, filters_per_layer=32, layers=3), 0.1).to(cuda_device)
    eng = HipTrunkInference(net, cuda_device, buckets=(NB,), symmetries="all")
    planes, legal = _boards(3)
    base = eng.evaluate(planes, legal).double().cpu().numpy()
    moved = eng.evaluate(t_planes(planes, t, SB), transform(legal, t, SB)).double().cpu().numpy()
    err = np.abs(moved - transform(base, t, SB)).max()
    print("engine equivariance t=%d: max err %.3g (bound %.3g)" % (t, err, 2 * 8 * U24))
    assert err <= 2 * 8 * U24


# ------------------------------------------------------------------------ 5. engine, encoded path
def _random_states(n, size, seed, max_len):
    from alphago_amd import go

    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        gs = go.GameState(size)
        for _ in range(int(rng.integers(5, max_len))):
            moves = gs.get_legal_moves(include_eyes=False)
            if not moves:
                break
            gs.do_move(moves[int(rng.integers(len(moves)))])
        out.append(gs)
    return out


def test_engine_all_encoded_path(cuda_device):
    from alphago_amd.features import DEFAULT_FEATURES
    from alphago_amd.models.inference import HipTrunkInference
    from alphago_amd.models.nets import PolicyNet

    torch.manual_seed(6)
    net = roughen(PolicyNet(48, board=19, filters_per_layer=32, layers=3), 0.1).to(cuda_device)
    kw = dict(buckets=(8,), feature_list=DEFAULT_FEATURES)
    eng = HipTrunkInference(net, cuda_device, symmetries="all", **kw)
    plain = HipTrunkInference(net, cuda_device, **kw)
    eng.set_encoded_planes(True)
    plain.set_encoded_planes(True)
    states = _random_states(5, 19, 4, 90)
    n = len(states)
    b, a, m, l = eng.fz.encode(states)
    probs, sens, bad = eng.evaluate_encoded(b, a, m, l)
    probs, sens = probs.clone(), sens.clone()
    planes = eng.encoded_planes_view(n).clone()
    _, sens0, bad0 = plain.evaluate_encoded(b, a, m, l)
    assert bad == bad0
    assert torch.equal(sens, sens0)  # the mask stays in the original frame
    assert torch.equal(planes, plain.encoded_planes_view(n))
    assert int(planes.sum()) > 0 and int(sens.sum()) > 0
    ref = eng.evaluate(planes, sens).double()
    err = (probs.double() - ref).abs().max().item()
    print("engine all encoded vs planes: max err %.3g" % err)
    assert err <= head_bound(8)
    assert not bool((probs * (sens == 0)).abs().max() > 0)
    one = plain.evaluate(planes, sens).double()
    assert (one - ref).abs().max().item() > 1e-4


# ------------------------------------------------------------------------------- 6. value engine
def test_value_engine_all(cuda_device):
    from alphago_amd.models.inference import HipValueInference
    from alphago_amd.models.nets import ValueNet

    torch.manual_seed(7)
    net = roughen(ValueNet(CB, board=SB, filters_per_layer=32, layers=3, dense=64), 0.1).to(cuda_device)
    eng = HipValueInference(net, cuda_device, buckets=(NB,), symmetries="all")
    plain = HipValueInference(net, cuda_device, buckets=(8 * NB,))
    for seed in (1, 2):
        planes, legal = _boards(seed)
        out = eng.evaluate(planes).clone()
        assert torch.equal(out, eng.evaluate(planes))
        x, _ = _fanned(planes, legal, ALL4, SB)
        v = plain.evaluate(x).double().cpu().numpy().reshape(8, NB)
        err = np.abs(out.double().cpu().numpy() - v.mean(0)).max()
        print("value engine all, submission %d: max err %.3g; spread over orientations %.3g" % (seed, err,
                                                                                             np.ptp(v, 0).max()))
        assert err <= 1e-6 + 8 * U24
        assert np.ptp(v, 0).max() > 1e-3  # the orientations do differ


# -------------------------------------------------------------------------------------- 7. random
def test_engines_random(cuda_device):
    from alphago_amd.models.inference import HipTrunkInference, HipValueInference
    from alphago_amd.models.nets import PolicyNet, ValueNet

    torch.manual_seed(8)
    n = 6
    pnet = roughen(PolicyNet(CB, board=SB, filters_per_layer=32, layers=3), 0.1).to(cuda_device)
    vnet = roughen(ValueNet(CB, board=SB, filters_per_layer=32, layers=3, dense=64), 0.1).to(cuda_device)
    e1 = HipTrunkInference(pnet, cuda_device, buckets=(8,), symmetries="random", symmetry_seed=3)
    e2 = HipTrunkInference(pnet, cuda_device, buckets=(8,), symmetries="random", symmetry_seed=3)
    plain = HipTrunkInference(pnet, cuda_device, buckets=(8,))
    seen = set()
    for seed in (1, 2, 3):
        planes, legal = _boards(seed, n=n)
        o1 = e1.evaluate(planes, legal).clone()
        o2 = e2.evaluate(planes, legal).clone()
        s = e1.last_symmetries()
        assert s.shape == (n,) and s.min() >= 0 and s.max() <= 7
        assert np.array_equal(s, e2.last_symmetries())  # same seed, same draw
        assert torch.equal(o1, o2)
        seen |= set(s.tolist())
        ref = _policy_oracle(plain, planes, legal, s[None], SB)
        assert np.abs(o1.double().cpu().numpy() - ref).max() <= head_bound(1)
    assert len(seen) > 1
    ev = HipValueInference(vnet, cuda_device, buckets=(8,), symmetries="random", symmetry_seed=3)
    vplain = HipValueInference(vnet, cuda_device, buckets=(8,))
    planes, legal = _boards(4, n=n)
    out = ev.evaluate(planes).clone()
    x, _ = _fanned(planes, legal, ev.last_symmetries()[None], SB)
    assert np.abs((out - vplain.evaluate(x)).double().cpu().numpy()).max() <= 1e-6 + U24


def test_engine_bad_mode_raises(cuda_device):
    from alphago_amd.models.inference import HipTrunkInference, make_policy_inference
    from alphago_amd.models.nets import PolicyNet

    net = PolicyNet(CB, board=SB, filters_per_layer=32, layers=2).to(cuda_device)
    with pytest.raises(ValueError):
        HipTrunkInference(net, cuda_device, symmetries="8")
    with pytest.raises(ValueError):
        make_policy_inference(net, cuda_device, symmetries="All")
