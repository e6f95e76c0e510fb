"""CPU checks of the oracles in update_refs.py that test_update_kernels.py holds the optimizer, pack and
dense kernels to: the oracles against train/engine.py, hand-computed values and nested loops; the
comparison rejects every mutant on the committed inputs and accepts the fp32 evaluation in the kernel's
order, contracted or not, with no element left out."""
import decimal
import math

import numpy as np
import pytest
import torch

import update_refs as R
from alphago_amd.train.engine import KerasSGDSchedule, optimizer_update_

U53 = 2.0 ** -53
# (name, hyper-parameters): the optimizers of the GPU tests at the scale that matters
OPTS = [
    ("sgd", R.hyper(R.OPT_SGD, lr=0.01, gscale=0.25)),
    ("momentum", R.hyper(R.OPT_MOMENTUM, lr=0.01, gscale=0.25, mom=0.9)),
    ("nesterov", R.hyper(R.OPT_MOMENTUM, lr=0.01, gscale=0.25, mom=0.9, nesterov=True)),
    ("adam", R.hyper(R.OPT_ADAM, lr=1e-3, gscale=0.25)),
]
N, SEED = 4099, 11


def _inputs(hp, n=N, seed=SEED):
    return R.update_inputs(n, seed, False, hp["gscale"], hp)


# ----------------------------------------------------------------------------- the update oracles
@pytest.mark.parametrize("name,hp", OPTS, ids=[o[0] for o in OPTS])
def test_oracle_equals_optimizer_update_in_fp64(name, hp):
    """train/engine.py optimizer_update_ on fp64 CPU tensors, with the kernel's fp32 constants and the
    gradient scale folded the way SgdPackArgs documents it (into the step; for Adam into the gradient)."""
    p, g, m1, m2 = _inputs(hp)
    k = R.kernel_constants(hp)
    optimizer = ("sgd", "momentum", "adam")[hp["opt"]]
    sched = KerasSGDSchedule(hp["lr"], optimizer=optimizer,
                             momentum=k["mom"], nesterov=hp["nesterov"], beta_1=k["b1"], beta_2=k["b2"], epsilon=k["eps"])
    tp, tg, t1, t2 = (torch.from_numpy(a).double() for a in (p, g, m1, m2))
    if hp["opt"] == R.OPT_ADAM:
        tg = tg * k["gs"]
    state = [t1, t2][:hp["opt"]]
    optimizer_update_(tp, tg, state, sched, k["s"])
    out, err = R.update_oracle(hp, p, g, m1, m2)
    # the same real-number expression: agreement to fp64 rounding of differently ordered operations
    # (1 - b formed in fp64 there, in fp32 here: engine's 1.0 - float32 value is exact, so identical)
    tol = 64 * U53
    for name_, t in (("p", tp), ("m1", t1 if hp["opt"] >= 1 else None), ("m2", t2 if hp["opt"] == 2 else None)):
        if t is None:
            assert out[name_] is None
            continue
        ref = out[name_]
        scale = np.maximum(np.abs(ref), err[name_] / R.U24)  # the magnitudes that were rounded
        assert np.all(np.abs(t.numpy() - ref) <= tol * scale), name_


def test_adam_two_steps_by_hand():
    """p = 1, g = 2 then 4, gscale 0.5, b1 = 0.5, b2 = 0.75, eps = 0.5, step 0.25, moments from zero:
    step 1: ge = 1, m = 0.5, v = 0.25, p = 1 - 0.25 * 0.5 / (0.5 + 0.5) = 0.875
    step 2: ge = 2, m = 0.25 + 1 = 1.25, v = 0.1875 + 1 = 1.1875, p = 0.875 - 0.3125 / (sqrt(1.1875) + 0.5)."""
    hp = R.hyper(R.OPT_ADAM, lr=0.25, gscale=0.5, b1=0.5, b2=0.75, eps=0.5)
    o1, e1 = R.update_oracle(hp, [1.0], [2.0], [0.0], [0.0])
    assert (o1["m1"][0], o1["m2"][0], o1["p"][0]) == (0.5, 0.25, 0.875)
    o2, _ = R.update_oracle(hp, o1["p"], [4.0], o1["m1"], o1["m2"])
    assert (o2["m1"][0], o2["m2"][0]) == (1.25, 1.1875)
    assert o2["p"][0] == 0.875 - 0.3125 / (math.sqrt(1.1875) + 0.5)
    # step 1 rounds only exactly representable values: every error term is U24 |value|
    assert e1["m1"][0] == R.U24 * (0.0 + 0.5 * 1.0 + 0.5 + 0.5) and e1["p"][0] > 0


def test_momentum_by_hand():
    hp = R.hyper(R.OPT_MOMENTUM, lr=0.125, gscale=0.5, mom=0.5)
    o, e = R.update_oracle(hp, [1.0], [4.0], [2.0])
    assert (o["m1"][0], o["p"][0]) == (0.75, 1.75)  # v' = 1 - 0.25, p' = 1 + 0.75
    assert e["m1"][0] == R.U24 * (1.0 + 0.25 + 0.75) and e["p"][0] == e["m1"][0] + R.U24 * 1.75
    hp["nesterov"] = True
    o, _ = R.update_oracle(hp, [1.0], [4.0], [2.0])
    assert o["p"][0] == 1.0 + 0.5 * 0.75 - 0.25


@pytest.mark.parametrize("name,hp", OPTS, ids=[o[0] for o in OPTS])
@pytest.mark.parametrize("contract", [False, True])
def test_fp32_update_is_within_the_bound(name, hp, contract):
    """The true update -- numpy float32 in the kernel's order, contracted and not -- passes the very
    comparison the GPU tests make, every element of it, over two consecutive steps."""
    p, g, m1, m2 = _inputs(hp)
    for step in range(2):
        out, err = R.update_oracle(hp, p, g, m1, m2)
        got = R.update_fp32(hp, p, g, m1, m2, contract=contract)
        for key in ("p", "m1", "m2"):
            if out[key] is None:
                continue
            bad = R.mismatches(got[key], out[key], err[key])
            assert bad.size == 0, (key, step, bad[:8], R.worst_ratio(got[key], out[key], err[key]))
            assert R.worst_ratio(got[key], out[key], err[key]) <= 1.0  # first order alone already holds it
        p = got["p"]
        m1 = got["m1"] if got["m1"] is not None else m1
        m2 = got["m2"] if got["m2"] is not None else m2


def test_fp32_update_on_dyadic_data_is_exact():
    """Dyadic inputs, step 2^-3, gscale 0.5, momentum 0.5: two SGD / momentum / Nesterov steps are exact in
    fp32, contracted or not -- the fp64 oracle is the one possible fp32 result."""
    for hp in (R.hyper(R.OPT_SGD, gscale=0.5), R.hyper(R.OPT_MOMENTUM, gscale=0.5, mom=0.5),
               R.hyper(R.OPT_MOMENTUM, gscale=0.5, mom=0.5, nesterov=True)):
        p, g, m1, m2 = R.update_inputs(N, SEED, dyadic=True)
        for step in range(2):
            out, err = R.update_oracle(hp, p, g, m1)
            for contract in (False, True):
                got = R.update_fp32(hp, p, g, m1, contract=contract)
                assert R.bit_equal(got["p"], out["p"])
                assert got["m1"] is None or R.bit_equal(got["m1"], out["m1"])
            p, m1 = got["p"], got["m1"] if got["m1"] is not None else m1


def _rejected(hp, mutant, inputs=None, **kw):
    p, g, m1, m2 = inputs or _inputs(hp)
    out, err = R.update_oracle(hp, p, g, m1, m2)
    mut, _ = R.update_oracle(hp, p, g, m1, m2, mutant=mutant, **kw)
    return {k: R.mismatches(mut[k], out[k], err[k]).size for k in ("p", "m1", "m2") if out[k] is not None}


def test_mutants_are_rejected():
    """Each wrong update, fed to the comparison in place of the kernel's output, fails it on the committed
    inputs (in the output named; the others may be unaffected)."""
    hp = dict(OPTS)
    assert _rejected(hp["adam"], "eps_in_sqrt")["p"] > 0
    bad = _rejected(hp["adam"], "adam_no_gscale")
    assert bad["p"] > 0 and bad["m1"] > N // 2 and bad["m2"] > N // 2
    bad = _rejected(hp["momentum"], "momentum_gscale_twice")
    assert bad["p"] > N // 2 and bad["m1"] > N // 2
    bad = _rejected(hp["nesterov"], "nesterov_plain")
    assert bad["p"] > N // 2 and bad["m1"] == 0
    bad = _rejected(hp["adam"], "v_linear")
    assert bad["m2"] > N // 2 and bad["m1"] == 0
    bad = _rejected(hp["adam"], "swap_m1_m2")
    assert bad["m1"] > N // 2 and bad["m2"] > N // 2
    for name in ("sgd", "momentum", "nesterov", "adam"):
        assert _rejected(hp[name], "step_64ulp")["p"] > 0, name


def test_eps_placement_shows_at_the_edge_elements():
    """Why update_inputs carries elements with sqrt(v') around eps: that is where the placement of eps
    moves p' by more than the bound; and the other edges are what their comments say."""
    hp = dict(OPTS)["adam"]
    p, g, m1, m2 = _inputs(hp)
    out, err = R.update_oracle(hp, p, g, m1, m2)
    mut, _ = R.update_oracle(hp, p, g, m1, m2, mutant="eps_in_sqrt")
    bad = R.mismatches(mut["p"], out["p"], err["p"])
    assert bad.size > 0 and set(bad.tolist()) & set(range(9))  # g = 0 / m2 = 0 and |g gscale| ~ eps
    k = R.kernel_constants(hp)
    assert np.sqrt(out["m2"][3:9]).min() < k["eps"] < np.sqrt(out["m2"][3:9]).max() * 10
    assert out["m2"][0] == 0.0 and abs(out["m1"][11]) < 1e-3 * abs(m1[11])  # the sum cancels


# ----------------------------------------------------------------------------- the flat buffer
def test_flat_layout_has_gaps_and_unaligned_offsets():
    lo, rg, total = R.flat_layout()
    cov = R.covered_mask(total, R.PACK_LAYERS, lo, rg)
    assert not cov[0] and not cov[-1] and [n for _, n in rg] == R.RANGE_LENS
    spans = [(o, co * ci * K * K) for (co, ci, K, _, _, _), o in zip(R.PACK_LAYERS, lo)] + rg
    for (o, n), (o2, _) in zip(spans, spans[1:]):
        assert o + n < o2  # a gap before every layer and range
    assert all(o % 4 for o, _ in rg)
    assert cov.sum() == sum(n for _, n in spans)
    p, g, m1, m2 = R.flat_inputs(3, False)
    assert np.isnan(g[~cov]).all() and (p[~cov] == R.P_SENTINEL).all() and (m1[~cov] == R.M_SENTINEL).all()
    assert not np.isnan(g[cov]).any() and (m2[cov] >= 0).all()


@pytest.mark.parametrize("name,hp", OPTS, ids=[o[0] for o in OPTS])
def test_shifted_layer_offset_is_rejected(name, hp):
    """A layer updated one element further on: its first element keeps the old value, the gap element
    behind it takes a NaN gradient; both fail the comparison, which is bit equality in the gaps."""
    p, g, m1, m2 = R.flat_inputs(5, False, gscale=hp["gscale"])
    ref, bnd = R.flat_oracle(hp, p, g, m1, m2)
    lo, rg, total = R.flat_layout()
    cov = R.covered_mask(total, R.PACK_LAYERS, lo, rg)
    assert (bnd["p"][~cov] == 0).all() and np.array_equal(ref["p"][~cov], p[~cov].astype(np.float64))
    for layer in (0, 3, 5):
        mut, _ = R.flat_oracle(hp, p, g, m1, m2, shift_layer=layer)
        bad = R.mismatches(mut["p"], ref["p"], bnd["p"])
        co, ci, K = R.PACK_LAYERS[layer][:3]
        assert set(bad.tolist()) == {lo[layer], lo[layer] + co * ci * K * K}
    # a sentinel overwritten with its own value plus one ulp in a gap is a mismatch too
    touched = ref["p"].copy()
    touched[0] = np.nextafter(np.float32(R.P_SENTINEL), np.float32(np.inf))
    assert R.mismatches(touched, ref["p"], bnd["p"]).tolist() == [0]


# ----------------------------------------------------------------------------- the schedule
@pytest.mark.parametrize("decay", [0.0, 2.0 ** -7, 0.01, 1e-4])
def test_schedule_oracle_equals_keras_schedule_sgd(decay):
    """KerasSGDSchedule.current() rounds three times (product, sum, quotient): within 4 * 2^-53 relative
    of the exact value; where decay * t is exact and the sum representable it is the rounded exact value."""
    for t in (0, 1, 2, 3, 10, 999, 12345, 10 ** 6):
        host = KerasSGDSchedule(0.003, decay, iterations=t).current()
        assert host == R.host_schedule(0.003, decay, t)
        exact = R.schedule_exact(0.003, decay, t)
        assert R.rel_dev(host, exact) <= 4 * U53
        if decay in (0.0, 2.0 ** -7):
            assert host == float(exact)


@pytest.mark.parametrize("t", [0, 1, 999])
def test_schedule_oracle_equals_keras_schedule_adam(t):
    """Adam's bias correction: the bound follows from the conditioning of 1 - b^n at the tested t
    (update_refs.adam_schedule_bound): about 1000 units of 2^-53 at t = 0 with beta_2 = 0.999, where
    1 - 0.999 loses three digits, and a handful at t = 999."""
    s = KerasSGDSchedule(3e-4, 0.0, iterations=t, optimizer="adam", beta_1=0.9, beta_2=0.999)
    exact = R.schedule_exact(3e-4, 0.0, t, adam=(0.9, 0.999))
    bound = R.adam_schedule_bound(0.9, 0.999, t)
    assert R.rel_dev(s.current(), exact) <= bound * U53
    assert bound < (1100 if t == 0 else 600 if t == 1 else 12)
    assert R.within_one_ulp32(np.float32(s.current()), exact)
    assert not R.within_one_ulp32(np.float32(s.current()) * np.float32(1 + 2.0 ** -21), exact)


def test_schedule_exact_values():
    assert R.schedule_exact(0.5, 0.25, 4) == decimal.Decimal("0.25")
    # t = 0, b1 = 0.5, b2 = 0.75: lr sqrt(0.25) / 0.5 = lr
    assert R.schedule_exact(0.125, 0.0, 0, adam=(0.5, 0.75)) == decimal.Decimal("0.125")


# ----------------------------------------------------------------------------- packs
@pytest.mark.parametrize("co,ci,K,cout_p", [(192, 48, 5, 192), (152, 49, 5, 160), (3, 33, 3, 32)])
def test_packed_tap_oracle_against_nested_loops(co, ci, K, cout_p):
    """Slot by slot: a permutation of expected_pack's wf entries plus zeros."""
    g = torch.Generator().manual_seed(co + ci)
    w = torch.randint(-100, 101, (co, ci, K, K), generator=g).double()
    got = R.expected_pack_pk(w, cout_p)
    wf, _ = R.expected_pack(w, 64, cout_p)
    T, cpt = K * K, (ci + 7) // 8
    ref = torch.zeros_like(got)
    seen = torch.zeros(got.shape, dtype=torch.bool)
    for t in range(T):
        for c in range(ci):
            q = t * cpt + (c >> 3)
            slot = (q & 7) * 8 + (c & 7)
            assert not seen[q >> 3, 0, slot]
            seen[q >> 3, :, slot] = True
            ref[q >> 3, :, slot] = wf[t, :, c]
    assert got.shape == (R.pk_steps(T, ci), cout_p, 64) and torch.equal(got, ref)
    assert not got[~seen].any() and not got[:, co:].any()
    assert sorted(got[seen].flatten().tolist()) == sorted(wf[:, :, :ci].flatten().tolist())
    un = R.pk_unwritten(T, ci, cout_p)
    assert un.sum().item() == (got.shape[0] * 8 - T * cpt) * 8 * cout_p and not (un & seen).any()
    assert not un[:-1].any()  # only the last step has a tail


def test_pack_mutants_are_rejected():
    """The pack comparison is torch.equal: an unflipped wd and a non-zero padded row both fail it."""
    lo, rg, total = R.flat_layout()
    p = R.flat_inputs(7, True)[0]
    ws = R.layer_weights(p)
    for layer, w in zip(R.PACK_LAYERS, ws):
        wf, wd = R.pack_oracle(w, layer)
        if wd is not None and layer[2] > 1:
            assert not torch.equal(R.pack_oracle(w, layer, mutant="no_flip")[1], wd)
        if layer[3] > layer[0]:
            assert not torch.equal(R.pack_oracle(w, layer, mutant="padded_row")[0], wf)
            assert not wf[:, layer[0]:].any()
    # K = 1 has a single tap: the flip is the identity there and only there
    one = R.PACK_LAYERS[4]
    assert torch.equal(R.pack_oracle(ws[4], one, mutant="no_flip")[1], R.pack_oracle(ws[4], one)[1])


def test_halfway_weights_hit_both_rounding_directions():
    w = R.halfway_weights((64, 33, 3, 3), 1)
    b = w.view(torch.int32)
    tie = (b & 0xFFFF) == 0x8000
    assert 0.25 < tie.float().mean().item() < 0.4
    up = w.to(torch.bfloat16).float().abs() > w.abs()
    assert (tie & up).any() and (tie & ~up).any()
    odd = ((b >> 16) & 1) == 1
    assert torch.equal((tie & up), (tie & odd))  # ties go to the even neighbour
    assert not torch.equal(w.to(torch.bfloat16).float(), w)


# ----------------------------------------------------------------------------- pack_input
def test_pack_input_ref_borders_and_rows():
    g = torch.Generator().manual_seed(2)
    planes = torch.randint(0, 256, (5, 3, 9, 9), dtype=torch.uint8, generator=g)
    sym = torch.arange(8, dtype=torch.int32)
    rows = torch.tensor([0, 4, 5, -1, 2, 1, 3, 0])
    tgt = torch.tensor([0, 80, -1, 40, 8, 72, -1, 9], dtype=torch.int32)
    for P in (1, 2):
        ref, tout = R.pack_input_ref(planes, sym, tgt, P, 8, 7.0, rows=rows)
        assert ref.shape == (8, 9 + 2 * P, 9 + 2 * P, 8)
        border = torch.ones(ref.shape[1:3], dtype=torch.bool)
        border[P:-P, P:-P] = False
        assert (ref[:, border] == 7.0).all() and not ref[:, ~border][..., 3:].any()
        assert not ref[2, ~border].any() and not ref[3, ~border].any()  # rows outside the pool
        assert torch.equal(ref[0, P:-P, P:-P, :3], planes[0].permute(1, 2, 0).float())  # identity
        assert torch.equal(ref[1, P:-P, P:-P, 0], torch.rot90(planes[4, 0], 1).float())
        assert tout.tolist()[2] == -1 and tout.tolist()[6] == -1 and tout.tolist()[0] == 0


# ----------------------------------------------------------------------------- dense
def test_dense_oracle_and_split_edges():
    A, B, bias, C0 = R.dense_inputs(5, 7, 33, True, False, 0)
    ref = R.dense_oracle(A, B, bias, C0, True, False, 0.5)
    loop = torch.zeros(5, 7, dtype=torch.float64)
    for m in range(5):
        for n in range(7):
            dot = sum(float(A[k, m]) * float(B[k, n]) for k in range(33))
            loop[m, n] = dot + float(bias[n]) + 0.5 * float(C0[m, n])
    assert torch.equal(ref, loop) and torch.equal(ref, ref.round())
    assert (C0 % 2 == 0).all() and A.abs().max() <= 8 and B.abs().max() <= 8
    # the split edges the GPU test runs: a last split of a single k, and a recomputed split count
    assert R.dense_launch_splits(33, 33, 385) == (4, 128, 4) and 385 - 3 * 128 == 1
    assert R.dense_launch_splits(1, 1, 129) == (2, 96, 2)
    assert R.dense_launch_splits(64, 64, 128) == (1, 128, 1)
    K = R.dense_recomputed_k(65, 65)
    s, kchunk, launched = R.dense_launch_splits(65, 65, K)
    assert K == 8193 and launched < s and K * 64 + 8 + 64 < 2 ** 24


def test_dense_cases_cover_the_edges():
    """Walks the list: M, N in {1, 31, 32, 33, 63, 64, 65}, every listed K, all four transposes, bias on and
    off, every beta, each on both paths ."""
    assert {c[0] for c in R.DENSE_CASES} == {c[1] for c in R.DENSE_CASES} == {1, 31, 32, 33, 63, 64, 65}
    assert {c[2] for c in R.DENSE_CASES} == {1, 2, 31, 32, 33, 128, 129, 385, R.DENSE_K_RECOMPUTED}
    assert R.dense_recomputed_k(65, 65) == R.DENSE_K_RECOMPUTED
    for split in (False, True):
        sub = [c for c in R.DENSE_CASES if (R.dense_launch_splits(*c[:3])[2] > 1) == split]
        assert {(c[3], c[4]) for c in sub} == {(a, b) for a in (False, True) for b in (False, True)}
        assert {c[5] for c in sub} == {False, True} and {c[6] for c in sub} == {0.0, 1.0, 0.5}
    s, kchunk, launched = R.dense_launch_splits(65, 65, R.DENSE_K_RECOMPUTED)
    assert launched < s
    assert R.dense_launch_splits(33, 33, 385)[1:] == (128, 4)  # the last split holds a single k
