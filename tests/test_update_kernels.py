"""The kernels that write the weights -- ops.sgd_update, sgd_update_sched, sgd_pack, pack_weights,
pack_input (pack.hip) and dense_f32 (dense.hip) -- against the fp64 oracles of tests/update_refs.py.

Updates on dyadic data must equal the fp64 oracle bit for bit; on normal data every element must be
within twice the first-order fp32 bound that update_refs derives (tests/test_update_refs.py shows on the
CPU that this comparison rejects a list of wrong updates and accepts the fp32 evaluation).  Packs, the
input pack and the dense layer on integer operands are compared with ``torch.equal``.  Outputs start as
sentinels and everything a kernel must not write has to keep them.  Every test prints the figures it
asserts (``pytest -s``)."""
import numpy as np
import pytest
import torch

import update_refs as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U53 = 2.0 ** -53
BYTE_SENTINEL = 0x5A


@pytest.fixture(scope="module")
def ops(cuda_device):
    from alphago_amd import ops as _ops

    _ops.load()
    return _ops


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _report(what, value):
    print("update-kernels: %s = %s" % (what, value))


# ============================================================================= sgd_update, sgd_update_sched
# every n % 4 tail; 2^21 + 3 fills the 2048-block grid exactly (2048 * 256 float4 lanes, one pass each),
# 2^21 + 1027 is the first size class that needs 2049 blocks: the grid is capped and the stride loop wraps
SGD_SIZES = [1, 2, 3, 4, 5, 1003, 2 ** 21 + 3, 2 ** 21 + 1027]
GUARD = 4  # floats around the updated span (keeps the span 16-byte aligned)


def _guarded(p, dev):
    buf = torch.full((p.size + 2 * GUARD,), R.P_SENTINEL, dtype=torch.float32)
    buf[GUARD:GUARD + p.size] = torch.from_numpy(p)
    buf = buf.to(dev)
    return buf, buf[GUARD:GUARD + p.size]


def _run_sgd(ops, dev, n, dyadic, sched_mode):
    hp = R.hyper(R.OPT_SGD, lr=2.0 ** -3, gscale=0.5) if dyadic else R.hyper(R.OPT_SGD, lr=0.01, gscale=0.25)
    p, g = R.update_inputs(n, 100 + n % 1000, dyadic, hp["gscale"])[:2]
    buf, pd = _guarded(p, dev)
    gd = _dev(g, dev)
    lr = None
    if sched_mode:
        k0, decay = 7.0, 0.0 if dyadic else 0.01
        sched = torch.tensor([hp["lr"], decay, k0, 0.0], dtype=torch.float64, device=dev)
        ops.sgd_update_sched(pd, gd, sched, hp["gscale"])
        s = sched.cpu().tolist()
        assert s[:3] == [hp["lr"], decay, k0 + 1]
        lr = s[3]
        assert abs(lr - R.host_schedule(hp["lr"], decay, k0)) <= 4 * U53 * lr
    else:
        ops.sgd_update(pd, gd, hp["lr"], hp["gscale"])
    out, err = R.update_oracle(hp, p, g, lr=lr)
    got = buf.cpu()
    assert torch.equal(_bits(gd), _bits(torch.from_numpy(g)))  # the gradient is read only
    guard = torch.cat([got[:GUARD], got[GUARD + n:]])
    assert (guard == R.P_SENTINEL).all() and guard.numel() == 2 * GUARD
    return got[GUARD:GUARD + n].numpy(), out["p"], err["p"]


@pytest.mark.parametrize("sched_mode", [False, True], ids=["lr", "sched"])
@pytest.mark.parametrize("n", SGD_SIZES)
def test_sgd_update_exact_on_dyadic_data(ops, cuda_device, n, sched_mode):
    """p, g multiples of 2^-8 in [-4, 4], step 2^-3, gscale 0.5: every product and sum is exact, so the
    result is the fp64 oracle bit for bit, contracted or not; the guards around the span keep their
    sentinel and g is untouched."""
    got, ref, _ = _run_sgd(ops, cuda_device, n, True, sched_mode)
    assert R.bit_equal(got, ref)


@pytest.mark.parametrize("sched_mode", [False, True], ids=["lr", "sched"])
@pytest.mark.parametrize("n", SGD_SIZES)
def test_sgd_update_within_bound(ops, cuda_device, n, sched_mode):
    """Normal data, lr 0.01 (or the schedule at decay 0.01), gscale 0.25: |got - ref| <= 2 bound everywhere."""
    got, ref, bound = _run_sgd(ops, cuda_device, n, False, sched_mode)
    _report("sgd_update%s n=%d max |got - ref| / bound" % ("_sched" if sched_mode else "", n),
            R.worst_ratio(got, ref, bound))
    bad = R.mismatches(got, ref, bound)
    assert bad.size == 0, (bad[:8], got[bad[:8]], ref[bad[:8]])


@pytest.mark.parametrize("decay", [2.0 ** -7, 0.01], ids=["decay2^-7", "decay0.01"])
def test_sgd_update_sched_schedule(ops, cuda_device, decay):
    """After k calls sched[2] = k0 + k, sched[0] and sched[1] unchanged, and sched[3] is the host's
    lr0 / (1 + decay t): bit for bit where decay t is exact (decay 2^-7), within 4 * 2^-53 relative at
    decay 0.01 (the host rounds three times, a contracting device twice); float32(sched[3]), the step the
    update kernel uses, is within one fp32 ulp of the exact value.

    Observed on MI355X at decay 0.01, t = 0..11, 999, 12345 (lr0 0.003): sched[3] was bit-equal to the host's
    value at all 14 (the test prints the count and the largest deviation)."""
    dev = cuda_device
    lr0 = 0.003
    p, g = torch.zeros(8, device=dev), torch.ones(8, device=dev)
    equal, worst, total = 0, 0.0, 0
    for k0, calls in ((0, 12), (999, 1), (12345, 1)):
        sched = torch.tensor([lr0, decay, float(k0), -1.0], dtype=torch.float64, device=dev)
        for k in range(calls):
            ops.sgd_update_sched(p, g, sched, 1.0)
            s = sched.cpu().tolist()
            t = k0 + k
            assert s[0] == lr0 and s[1] == decay and s[2] == t + 1
            host = R.host_schedule(lr0, decay, t)
            exact = R.schedule_exact(lr0, decay, t)
            equal += s[3] == host
            total += 1
            worst = max(worst, abs(s[3] - host) / host / U53)
            if decay == 2.0 ** -7:
                assert s[3] == host == float(exact)
            assert abs(s[3] - host) <= 4 * U53 * host
            assert R.rel_dev(s[3], exact) <= 4 * U53
            assert R.within_one_ulp32(np.float32(s[3]), exact)
    _report("sched decay=%g: device == host bit for bit in %d of %d, max |dev - host| / host in 2^-53"
            % (decay, equal, total), worst)


def test_sgd_update_refuses_unaligned_views(ops, cuda_device):
    """sgd_kernel reads p and g as float4: a contiguous view that starts inside a buffer is refused on the
    host (nothing is launched)."""
    p, g = torch.ones(16, device=cuda_device), torch.ones(16, device=cuda_device)
    sched = torch.tensor([0.1, 0.0, 0.0, 0.0], dtype=torch.float64, device=cuda_device)
    for pp, gg in ((p[1:], g[1:]), (p[:15], g[1:]), (p[1:], g[:15])):
        with pytest.raises(RuntimeError):
            ops.sgd_update(pp, gg, 0.5, 1.0)
        with pytest.raises(RuntimeError):
            ops.sgd_update_sched(pp, gg, sched, 1.0)
    assert (p == 1).all() and sched.cpu().tolist() == [0.1, 0.0, 0.0, 0.0]
    ops.sgd_update(p[4:], g[4:], 0.5, 1.0)  # 16 bytes in: aligned, accepted
    assert (p[:4] == 1).all() and (p[4:] == 0.5).all()


# ============================================================================= sgd_pack
def _pack_buffers(ops, dev, layers):
    """Sentinel-filled wf / wd of ops.packed_weight_like / packed_weight_pk's shapes (an empty wd for the
    packed-tap layer)."""
    wfs, wds = [], []
    for (co, ci, K, cout_p, cin_p, pk) in layers:
        shape = torch.empty((co, ci, K, K), device="meta")
        if pk:
            wfs.append(torch.full_like(ops.packed_weight_pk(shape, cout_p, device=dev), R.BF16_SENTINEL))
            wds.append(torch.empty(0, dtype=BF, device=dev))
        else:
            wfs.append(torch.full_like(ops.packed_weight_like(shape, cin_p, cout_p, device=dev), R.BF16_SENTINEL))
            wds.append(torch.full_like(ops.packed_weight_like(shape, cin_p, cout_p, transposed=True, device=dev),
                                       R.BF16_SENTINEL))
    return wfs, wds


def _check_packs(layers, ws, wfs, wds, what, sgd_pack):
    """Every pack equals the oracle's pack of the OIHW weights ``ws`` bit for bit.  Not written, so still
    the sentinel: the extra tap of packed_weight_like; and by sgd_pack (``sgd_pack`` True) the slots of the
    packed-tap layout's last step with t >= T, which pack_weights fills with zeros."""
    for i, (layer, w, wf, wd) in enumerate(zip(layers, ws, wfs, wds)):
        co, ci, K, cout_p, cin_p, pk = layer
        T = K * K
        ewf, ewd = R.pack_oracle(w, layer)
        wf = wf.cpu()
        if pk:
            un = R.pk_unwritten(T, ci, cout_p)
            assert un.any()
            if sgd_pack:
                assert torch.equal(wf[~un], ewf[~un]), (what, i)
                assert (wf[un] == R.BF16_SENTINEL).all(), (what, i)
            else:
                assert torch.equal(wf, ewf), (what, i)
            continue
        wd = wd.cpu()
        assert torch.equal(wf[:T], ewf) and torch.equal(wd[:T], ewd), (what, i)
        assert wf.shape[0] == T + (cin_p % 64 == 32) and wd.shape[0] == T + (cout_p % 64 == 32)
        assert (wf[T:] == R.BF16_SENTINEL).all() and (wd[T:] == R.BF16_SENTINEL).all(), (what, i)


def _meta(layers, lo):
    return [(o, co, ci, K) for (co, ci, K, _, _, _), o in zip(layers, lo)]


def _sgd_pack_steps(ops, dev, hp, dyadic, sched_mode, layers=R.PACK_LAYERS, range_lens=R.RANGE_LENS, steps=2, k0=3,
                    seed=21):
    """``steps`` consecutive ops.sgd_pack calls on the flat buffer of update_refs.flat_layout, each checked
    against the oracle applied to the state the step started from.  Returns the largest |got - ref| / bound
    per output."""
    lo, rg, total = R.flat_layout(layers, range_lens)
    cov = R.covered_mask(total, layers, lo, rg)
    state = dict(zip(("p", "g", "m1", "m2"), R.flat_inputs(seed, dyadic, layers, range_lens, hp["gscale"])))
    opt = hp["opt"]
    pd, gd = _dev(state["p"], dev), _dev(state["g"], dev)
    m1d = _dev(state["m1"], dev) if opt >= 1 else None
    m2d = _dev(state["m2"], dev) if opt == 2 else None
    wfs, wds = _pack_buffers(ops, dev, layers)
    sched = None
    if sched_mode:
        decay = 0.0 if dyadic or opt == 2 else 0.01
        if opt == 2:
            k0 = 0  # t = 0 and 1: where the bias correction is largest
        s = [hp["lr"], decay, float(k0), -1.0] + ([hp["b1"], hp["b2"], 2.0, 0.0] if opt == 2 else [])
        sched = torch.tensor(s, dtype=torch.float64, device=dev)
    worst = dict(p=0.0, m1=0.0, m2=0.0)
    for step in range(steps):
        ops.sgd_pack(pd, gd, hp["lr"], _meta(layers, lo), wfs, wds, rg, sched=sched, gscale=hp["gscale"], opt=opt,
                     m1=m1d, m2=m2d, momentum=hp["mom"], beta_1=hp["b1"], beta_2=hp["b2"], epsilon=hp["eps"],
                     nesterov=hp["nesterov"])
        lr = None
        if sched_mode:
            s = sched.cpu().tolist()
            t = k0 + step
            assert s[0] == hp["lr"] and s[1] == decay and s[2] == t + 1
            lr = s[3]
            if opt == 2:
                assert s[4:] == [hp["b1"], hp["b2"], 2.0, 0.0]
                exact = R.schedule_exact(hp["lr"], decay, t, adam=(hp["b1"], hp["b2"]))
                _report("sgd_pack adam schedule t=%d fp64 relative deviation in 2^-53" % t, R.rel_dev(lr, exact) / U53)
                assert R.within_one_ulp32(np.float32(lr), exact)
            else:
                host = R.host_schedule(hp["lr"], decay, t)
                assert abs(lr - host) <= 4 * U53 * host
                assert dyadic is False or lr == host
                assert R.within_one_ulp32(np.float32(lr), R.schedule_exact(hp["lr"], decay, t))
        ref, bnd = R.flat_oracle(hp, state["p"], state["g"], state["m1"], state["m2"], layers, range_lens, lr=lr)
        got = dict(p=pd.cpu().numpy().copy(), m1=m1d.cpu().numpy().copy() if opt >= 1 else state["m1"],
                   m2=m2d.cpu().numpy().copy() if opt == 2 else state["m2"])
        assert torch.equal(_bits(gd), _bits(torch.from_numpy(state["g"])))  # g wholly unchanged, NaNs included
        for key in ("p", "m1", "m2"):
            # the gaps and the tail: bit-unchanged
            assert np.array_equal(got[key][~cov].view(np.int32), state[key][~cov].view(np.int32)), (key, step)
            worst[key] = max(worst[key], R.worst_ratio(got[key][cov], ref[key][cov], bnd[key][cov]))
            bad = R.mismatches(got[key], ref[key], bnd[key])
            assert bad.size == 0, (key, step, bad[:8], got[key][bad[:8]], ref[key][bad[:8]], bnd[key][bad[:8]])
            if dyadic:
                assert R.bit_equal(got[key], ref[key]), (key, step)
        # packs: bf16 of the master the kernel left, zeros in every padded row and column
        _check_packs(layers, R.layer_weights(got["p"], layers, lo), wfs, wds, "step %d" % step, True)
        if dyadic:  # and of the oracle's master
            _check_packs(layers, R.layer_weights(ref["p"].astype(np.float32), layers, lo), wfs, wds, "oracle", True)
        state.update(p=got["p"], m1=got["m1"], m2=got["m2"])
    # the same weights through ops.pack_weights: identical where both write
    if layers:
        wf2, wd2 = _pack_buffers(ops, dev, layers)
        wdev = [pd[o:o + co * ci * K * K].view(co, ci, K, K) for (co, ci, K, _, _, _), o in zip(layers, lo)]
        ops.pack_weights(wdev, wf2, wd2)
        for layer, a, b, c, d in zip(layers, wfs, wf2, wds, wd2):
            T = layer[2] * layer[2]
            if layer[5]:
                un = R.pk_unwritten(T, layer[1], layer[3]).to(dev)
                assert torch.equal(a[~un], b[~un]) and not b[un].any() and (a[un] == R.BF16_SENTINEL).all()
            else:
                assert torch.equal(a, b) and torch.equal(c, d)
    return worst


_OPT_CASES = {
    "sgd": dict(opt=R.OPT_SGD, lr=0.01),
    "momentum": dict(opt=R.OPT_MOMENTUM, lr=0.01, mom=0.9),
    "nesterov": dict(opt=R.OPT_MOMENTUM, lr=0.01, mom=0.9, nesterov=True),
    "adam": dict(opt=R.OPT_ADAM, lr=1e-3),
}


@pytest.mark.parametrize("sched_mode", [False, True], ids=["lr", "sched"])
@pytest.mark.parametrize("gscale", [1.0, 0.25])
@pytest.mark.parametrize("name", list(_OPT_CASES))
def test_sgd_pack_within_bound(ops, cuda_device, name, gscale, sched_mode):
    """Six layers (5x5 with 49 of 64 channels, 152 of 160 with the extra tap, 192, 3 input channels with an
    empty second n-tile, 1x1, packed-tap) and five ranges (0, 1, 7, 256, 16389 elements, unaligned) in one
    launch, twice: masters and moments within the bound, gaps and g untouched, packs = bf16(master).

    Not written by sgd_pack (asserted to keep the sentinel): the extra tap of wf / wd, and in the
    packed-tap layout the slots with t >= T of the last step (ops.pack_weights zeroes those; production
    allocates them zeroed)."""
    hp = R.hyper(gscale=gscale, **_OPT_CASES[name])
    worst = _sgd_pack_steps(ops, cuda_device, hp, False, sched_mode)
    _report("sgd_pack %s gscale=%g %s max |got - ref| / bound" % (name, gscale, "sched" if sched_mode else "lr"), worst)


@pytest.mark.parametrize("gscale,sched_mode", [(1.0, True), (0.25, False)], ids=["g1-sched", "g0.25-lr"])
@pytest.mark.parametrize("name", ["sgd", "momentum", "nesterov"])
def test_sgd_pack_exact_on_dyadic_data(ops, cuda_device, name, gscale, sched_mode):
    """Dyadic data, momentum 0.5, step 2^-3: masters and velocity equal the fp64 oracle bit for bit over two
    steps, and every pack equals the pack of the oracle's master."""
    hp = R.hyper(gscale=gscale, **dict(_OPT_CASES[name], lr=2.0 ** -3, **({"mom": 0.5} if name != "sgd" else {})))
    _sgd_pack_steps(ops, cuda_device, hp, True, sched_mode)


@pytest.mark.parametrize("name", list(_OPT_CASES))
@pytest.mark.parametrize("what", ["no-layers", "no-ranges", "nothing"])
def test_sgd_pack_degenerate_calls(ops, cuda_device, name, what):
    """A call with no layers (ranges only), with no ranges (the two small layers only), and with neither."""
    hp = R.hyper(gscale=0.25, **_OPT_CASES[name])
    layers = [] if what != "no-ranges" else [R.PACK_LAYERS[3], R.PACK_LAYERS[4]]
    lens = [] if what != "no-layers" else R.RANGE_LENS
    _sgd_pack_steps(ops, cuda_device, hp, False, name == "adam", layers, lens, steps=1)


@pytest.mark.parametrize("t", [0, 1, 999])
def test_sgd_pack_adam_schedule(ops, cuda_device, t):
    """The 8-entry schedule at (0.9, 0.999): float32(sched[3]), the step Adam uses, is within one fp32 ulp of
    the exact lr_t = lr sqrt(1 - b2^(t+1)) / (1 - b1^(t+1)).  No fp64 assertion is made for the device pow
    path; the deviation is printed.  Observed on MI355X, |sched[3] - exact| / exact in units of 2^-53:
    0.14 at t = 0, 63.6 at t = 1 (1 - 0.999^2 loses three digits of pow's result), 1.16 at t = 999."""
    dev = cuda_device
    hp = R.hyper(R.OPT_ADAM, lr=3e-4, gscale=0.25)
    p, g, m1, m2 = R.update_inputs(260, 5, False, 0.25)
    pd, gd, m1d, m2d = (_dev(a, dev) for a in (p, g, m1, m2))
    sched = torch.tensor([3e-4, 0.0, float(t), -1.0, 0.9, 0.999, 2.0, 0.0], dtype=torch.float64, device=dev)
    ops.sgd_pack(pd, gd, 123.0, [], [], [], [(1, 258)], sched=sched, gscale=0.25, opt=R.OPT_ADAM, m1=m1d, m2=m2d)
    s = sched.cpu().tolist()
    exact = R.schedule_exact(3e-4, 0.0, t, adam=(0.9, 0.999))
    _report("adam schedule t=%d fp64 relative deviation in 2^-53" % t, R.rel_dev(s[3], exact) / U53)
    assert s[2] == t + 1 and s[:2] == [3e-4, 0.0] and s[4:] == [0.9, 0.999, 2.0, 0.0]
    assert R.within_one_ulp32(np.float32(s[3]), exact)
    out, err = R.update_oracle(hp, p, g, m1, m2, lr=s[3])
    got = dict(p=pd.cpu().numpy(), m1=m1d.cpu().numpy(), m2=m2d.cpu().numpy())
    for key, old in (("p", p), ("m1", m1), ("m2", m2)):
        assert R.accepted(got[key][1:259], out[key][1:259], err[key][1:259]), key
        assert got[key][0] == old[0] and got[key][259] == old[259]


def test_sgd_pack_refusals(ops, cuda_device):
    """Host checks only: nothing is launched, p keeps its values."""
    dev = cuda_device
    n = 4096
    p, g = torch.ones(n, device=dev), torch.ones(n, device=dev)
    m = torch.zeros(n, device=dev)
    wf = torch.zeros(9, 64, 8, dtype=BF, device=dev)
    sched4 = torch.tensor([0.1, 0.0, 0.0, 0.0], dtype=torch.float64, device=dev)
    ok = dict(w_meta=[(0, 8, 3, 3)], wf=[wf], wd=[], ranges=[(300, 10)])

    def refused(**kw):
        a = dict(ok, **kw)
        with pytest.raises(RuntimeError):
            ops.sgd_pack(p, g, 0.5, a.pop("w_meta"), a.pop("wf"), a.pop("wd"), a.pop("ranges"), **a)

    refused(w_meta=[(0, 8, 3, 3)] * 25, wf=[wf] * 25)                       # 25 layers
    refused(ranges=[(i, 1) for i in range(65)])                            # 65 ranges
    refused(ranges=[(n - 1, 2)])                                           # a range past the end
    refused(w_meta=[(n - 8 * 3 * 9 + 1, 8, 3, 3)])                         # a layer past the end
    refused(opt=R.OPT_ADAM, m1=m, m2=m.clone(), sched=sched4)              # Adam with a 4-entry schedule
    refused(opt=R.OPT_MOMENTUM, m1=m[:n - 1])                              # m1 of the wrong size
    refused(opt=R.OPT_ADAM, m1=m, m2=m[:n - 4])
    refused(opt=R.OPT_MOMENTUM)                                            # no m1 at all
    refused(w_meta=[(0, 1, 1, 7)], wf=[torch.zeros(49, 64, 64, dtype=BF, device=dev)])  # K = 7
    assert (p == 1).all() and not m.any() and not wf.any() and sched4.cpu().tolist() == [0.1, 0.0, 0.0, 0.0]


# ============================================================================= pack_weights
def _int_weights(co, ci, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-100, 101, (co, ci, K, K), generator=g).float()  # integers: exact in bf16


@pytest.mark.parametrize("co,ci,K,cout_p", [(192, 48, 5, 192), (152, 49, 5, 160)])
def test_pack_weights_packed_tap_layout(ops, cuda_device, co, ci, K, cout_p):
    """The packed-tap layout into sentinels: bit-equal to the oracle, the zero tail of the last step
    (t >= T), which this kernel writes, included."""
    layer = (co, ci, K, cout_p, 64, True)
    w = _int_weights(co, ci, K, co + ci)
    wfs, wds = _pack_buffers(ops, cuda_device, [layer])
    ops.pack_weights([w.to(cuda_device)], wfs, wds)
    _check_packs([layer], [w], wfs, wds, "pk", False)
    assert not wfs[0].cpu()[R.pk_unwritten(K * K, ci, cout_p)].any()


@pytest.mark.parametrize("co,ci,cout_p,cin_p", [(1, 192, 64, 192), (33, 40, 64, 64), (152, 152, 160, 160)])
def test_pack_weights_1x1(ops, cuda_device, co, ci, cout_p, cin_p):
    layer = (co, ci, 1, cout_p, cin_p, False)
    w = _int_weights(co, ci, 1, co * 7 + ci)
    wfs, wds = _pack_buffers(ops, cuda_device, [layer])
    ops.pack_weights([w.to(cuda_device)], wfs, wds)
    _check_packs([layer], [w], wfs, wds, "1x1", False)


def test_pack_weights_25_layers(ops, cuda_device):
    """25 layers of mixed shapes in one call: two launches (24 + 1).  Every layer, the 25th included, is
    correct, the extra taps keep their sentinel, the weights and a bystander tensor are undisturbed."""
    kinds = [(8, 3, 3, 64, 8, False), (1, 192, 1, 64, 192, False), (33, 20, 3, 64, 32, False), (16, 48, 5, 64, 64, True),
             (5, 7, 5, 32, 32, False), (152, 49, 5, 160, 64, False), (40, 33, 3, 64, 64, True)]
    layers = [kinds[i % len(kinds)] for i in range(24)] + [(70, 35, 3, 96, 64, False)]
    assert len(layers) == 25 and layers[24] not in kinds
    ws = [_int_weights(co, ci, K, 1000 + i) for i, (co, ci, K, _, _, _) in enumerate(layers)]
    wdev = [w.to(cuda_device) for w in ws]
    by = torch.full((1024,), R.BF16_SENTINEL, dtype=BF, device=cuda_device)
    wfs, wds = _pack_buffers(ops, cuda_device, layers)
    ops.pack_weights(wdev, wfs, wds)
    _check_packs(layers, ws, wfs, wds, "25 layers", False)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(wdev, ws)) and (by == R.BF16_SENTINEL).all()


@pytest.mark.parametrize("layer", [(64, 33, 3, 64, 64, False), (40, 33, 3, 64, 64, True)], ids=["taps", "packed-tap"])
def test_pack_weights_rounds_to_nearest_even(ops, cuda_device, layer):
    """Non-integer weights, a third of them exactly halfway between two bf16 numbers: the pack is
    w.to(bfloat16)."""
    co, ci, K = layer[:3]
    w = R.halfway_weights((co, ci, K, K), 9)
    wfs, wds = _pack_buffers(ops, cuda_device, [layer])
    ops.pack_weights([w.to(cuda_device)], wfs, wds)
    _check_packs([layer], [w], wfs, wds, "halfway", False)
    if not layer[5]:
        assert torch.equal(wfs[0].cpu()[4, :co, :ci], w[:, :, 1, 1].to(BF))


# ============================================================================= pack_input
def _pack_input_case(ops, dev, C, S, Cp, P, B, npool, binary, with_out8, bad_rows=True):
    g = torch.Generator().manual_seed(C * 100 + S + P)
    planes = torch.randint(0, 2 if binary else 256, (npool, C, S, S), dtype=torch.uint8, generator=g)
    sym = (torch.arange(B) % 8).to(torch.int32)
    rows = torch.randint(0, npool, (B,), generator=g)
    if bad_rows:
        rows[B // 2], rows[B - 1] = npool, -1  # out of the pool: all-zero boards
    tgt = torch.randint(0, S * S, (B,), generator=g).to(torch.int32)
    tgt[1], tgt[B - 2] = -1, -1
    ref, tref = R.pack_input_ref(planes, sym, tgt, P, Cp, R.BF16_SENTINEL, rows=rows)
    out = torch.full((B, S + 2 * P, S + 2 * P, Cp), R.BF16_SENTINEL, dtype=BF, device=dev)
    out8 = torch.full(out.shape, BYTE_SENTINEL, dtype=torch.uint8, device=dev) if with_out8 else None
    tout = torch.full((B,), -7, dtype=torch.int32, device=dev)
    ops.pack_input(planes.to(dev), out, P, sym=sym.to(dev), target=tgt.to(dev), target_out=tout, rows=rows.to(dev),
                   out8=out8)
    got = out.cpu().float()
    # interior fully written (no sentinel survives unless the oracle says 7), padded channels zero, all four
    # borders keep the sentinel: one comparison with the sentinel-bordered oracle
    assert torch.equal(got, ref)
    assert (got[:, :P] == R.BF16_SENTINEL).all() and (got[:, -P:] == R.BF16_SENTINEL).all()
    assert (got[:, :, :P] == R.BF16_SENTINEL).all() and (got[:, :, -P:] == R.BF16_SENTINEL).all()
    assert not got[:, P:-P, P:-P, C:].any() and not (bad_rows and got[B // 2, P:-P, P:-P].any())
    assert torch.equal(tout.cpu().long(), tref) and tout[1].item() == -1 and tout[B - 2].item() == -1
    if with_out8:
        b8 = out8.cpu()
        inner = torch.zeros(out.shape[1:3], dtype=torch.bool)
        inner[P:-P, P:-P] = True
        assert (b8[:, ~inner] == BYTE_SENTINEL).all()
        assert torch.equal(b8[:, inner].view(torch.float8_e4m3fn).float(), ref[:, inner])  # 0 / 1: exact in e4m3


@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("C,S,Cp", [(48, 19, 64), (3, 9, 8), (137, 19, 144)])
def test_pack_input_borders_and_symmetries(ops, cuda_device, C, S, Cp, P):
    """Boards gathered from a pool through ``rows`` into a sentinel-filled buffer: (48, 19, 64) and (3, 9, 8)
    run the per-board kernel (4-byte and byte loads) on sixteen boards, all eight symmetries twice, two rows
    outside the pool; (137, 19, 144) is 49 457 bytes a board, the grid-stride kernel, on eight boards, one per
    symmetry (its out-of-pool rows are in test_pack_input_grid_wrap)."""
    B = 8 if C == 137 else 16
    _pack_input_case(ops, cuda_device, C, S, Cp, P, B, 11, False, False, bad_rows=B == 16)


@pytest.mark.parametrize("C,S,Cp", [(48, 19, 64), (3, 9, 8)])
def test_pack_input_e4m3_borders(ops, cuda_device, C, S, Cp):
    """out8 as well: its borders keep their bytes, its interior holds the same 0 / 1 planes."""
    _pack_input_case(ops, cuda_device, C, S, Cp, 2, 16, 11, True, True)


def test_pack_input_grid_wrap(ops, cuda_device):
    """B = 324 boards of (137, 19, 144): 324 * 361 * 18 = 2 105 352 chunks > 8192 * 256, so the grid-stride
    kernel wraps.  0 / 1 planes from a pool of four keep it small."""
    B = 324
    assert B * 361 * 18 > 8192 * 256 and 137 * 361 > 48 * 1024
    _pack_input_case(ops, cuda_device, 137, 19, 144, 1, B, 4, True, False)


# ============================================================================= dense_f32
@pytest.mark.parametrize("M,N,K,ta,tb,bias,beta", R.DENSE_CASES)
def test_dense_f32_exact_on_integers(ops, cuda_device, M, N, K, ta, tb, bias, beta):
    """Integer operands: every partial sum is an integer below 2^24, so the result equals fp64 for any
    summation order and split count.  C is a column slice of a wider tensor whose other columns keep a
    sentinel; with beta == 0 it starts as NaN and must be overwritten."""
    dev = cuda_device
    A, B, b, C0 = R.dense_inputs(M, N, K, ta, tb, M * 1000 + N * 10 + K)
    ref = R.dense_oracle(A, B, b if bias else None, C0, ta, tb, beta)
    assert ref.abs().max() < 2 ** 24
    wide = torch.full((M, N + 5), R.P_SENTINEL, device=dev)
    C = wide[:, 2:2 + N]
    C.copy_(C0 if beta != 0 else torch.full_like(C0, float("nan")))
    ops.dense_f32(A.to(dev), B.to(dev), C, bias=b.to(dev) if bias else None, trans_a=ta, trans_b=tb, beta=beta)
    got = wide.cpu()
    assert not torch.isnan(got).any()
    assert torch.equal(got[:, 2:2 + N].double(), ref)
    assert (got[:, :2] == R.P_SENTINEL).all() and (got[:, 2 + N:] == R.P_SENTINEL).all()
