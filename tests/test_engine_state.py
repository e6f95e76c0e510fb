"""The inference engines' state over time (models/inference.py): a bucket is allocated once, captured
once into a HIP graph and then replayed for the life of the process -- across weight refreshes, smaller
batches, several slots in flight and alternating planes / encoded submissions.

Comparison principle: an engine that has been through the state under test is compared with a fresh
engine that never was, built on the same net with the same buckets, precision and ``use_graphs`` and
given the same inputs in the same rows.  Same bucket means same conv plan, same kernels and the same
per-pixel accumulation order, so every comparison is ``torch.equal`` / ``np.array_equal``.  The one
inequality is the float64 anchor of ``test_refresh_after_capture`` (``ANCHOR``).

1. ``sync_weights`` after a capture: no device tensor moves (a), and the engine computes the new
   network (b) -- per parameter group, through the CNNPolicy / CNNValue wrappers, and after a trainer step.
2. A reused bucket forgets its previous batch: padding rows, masks, encoded inputs (c).
3. Two slots in flight (d); ``set_encoded_planes`` after a capture (e).
"""
import copy

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

SB, CB, NB = 9, 12, 8  # board, planes, bucket of the small engines (those of test_symmetry_inference.py)
FEATS = ["board", "ones", "turns_since"]  # 12 planes: the wrappers' feature list at these shapes

# Float64 anchor of the all-parameters refresh (bf16 arms): with d_new / d_old the engine's largest
# distance from the module's own float64 forward with the new / the old weights, ANCHOR * d_new <= d_old.
# A condition, not a precision claim: an engine holding any stale group sits near the old reference or
# between the two.  The references alone, measured on the CPU (weights of seed 11 at std 0.1 re-drawn
# with seed 12 at PERTURB_STD, boards of seed 1): max |ref64(new) - ref64(old)| = 0.327 (policy),
# 1.449 (value); the fp32 torch engines on the new weights give d_new 2.6e-7 / 1.1e-6 and d_old equal to
# those margins.  test_reference_margin_cpu keeps both margins above REF_MARGIN.
ANCHOR = 4
REF_MARGIN = 0.05


def roughen(net, std, seed):
    """Weights large enough for the outputs to depend visibly on every one of them; drawn on the host
    and written in place (the parameters stay where they are, on either device)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * std)
    return net


GROUPS = {
    "all": lambda name: True,
    "trunk_w": lambda name: name.startswith("trunk.weights"),
    "trunk_b": lambda name: name.startswith("trunk.biases"),
    "head_w": lambda name: name == "head_w",
    "head_b": lambda name: name == "head_b",
    "fc1_w": lambda name: name == "fc1_w",
    "fc1_b": lambda name: name == "fc1_b",
    "fc2_w": lambda name: name == "fc2_w",
    "fc2_b": lambda name: name == "fc2_b",
}
POLICY_GROUPS = ["all", "trunk_w", "trunk_b", "head_w", "head_b"]
VALUE_GROUPS = POLICY_GROUPS + ["fc1_w", "fc1_b", "fc2_w", "fc2_b"]


# 0.15, not the 0.1 of the first draw: at 0.1 the policy's two references are only 0.031 apart (81 points
# share the mass); at 0.15 the new policy is peaked (largest probability 0.35) and they are 0.327 apart
PERTURB_STD = 0.15


def perturb(net, group, seed):
    """Re-draw the parameters of one group in place (another seed); returns how many."""
    g = torch.Generator().manual_seed(seed)
    hit = 0
    with torch.no_grad():
        for name, p in net.named_parameters():
            fresh = torch.randn(p.shape, generator=g) * PERTURB_STD  # drawn for every parameter: one stream per seed
            if GROUPS[group](name):
                p.copy_(fresh)
                hit += 1
    assert hit > 0
    return hit


def make_net(kind, device, seed):
    from alphago_amd.models.nets import PolicyNet, ValueNet

    if kind == "policy":
        net = PolicyNet(CB, board=SB, filters_per_layer=32, layers=3)
    else:
        net = ValueNet(CB, board=SB, filters_per_layer=32, layers=3, dense=64)
    return roughen(net, 0.1, seed).to(device)


def make_engine(kind, net, device, **kw):
    from alphago_amd.models.inference import HipTrunkInference, HipValueInference

    kw.setdefault("buckets", (NB,))
    return (HipTrunkInference if kind == "policy" else HipValueInference)(net, device, **kw)


def boards(seed, n=NB, S=SB, C=CB):
    rng = np.random.default_rng(seed)
    return (rng.random((n, C, S, S)) < 0.4).astype(np.uint8), (rng.random((n, S * S)) < 0.6).astype(np.uint8)


def run(eng, kind, planes, legal=None, slot=0):
    """One evaluation, copied out of the bucket (``evaluate`` returns views of bucket memory)."""
    out = eng.evaluate(planes, legal, slot=slot) if kind == "policy" else eng.evaluate(planes, slot=slot)
    return out.clone()


def ref64(net, kind, planes, legal):
    """The module's own forward in float64 on the CPU: ``logits_torch`` with the mask applied as
    TorchPolicyInference._plain does, or ``forward_torch`` -- written out from the module's trunk and
    parameters, because both methods cast the head's output to fp32 (``.float()``), which a float64
    ValueNet then cannot multiply with its float64 dense weights."""
    n64 = copy.deepcopy(net).double().cpu()
    x = torch.from_numpy(planes).double()
    with torch.no_grad():
        h = n64.trunk.forward_torch(x)
        z = torch.nn.functional.conv2d(h, n64.head_w, n64.head_b).flatten(1)
        assert z.dtype == torch.float64
        if kind == "value":
            z = z @ n64.fc1_w + n64.fc1_b
            return torch.tanh(z @ n64.fc2_w + n64.fc2_b).squeeze(1)
        z = z.masked_fill(torch.from_numpy(legal) == 0, float("-inf"))
        return torch.nan_to_num(torch.softmax(z, 1), nan=0.0)


def assert_fp8_ran(eng):
    """The e4m3 trunk really ran: the engine is calibrated and every bucket is at or above the threshold."""
    assert eng.calibrated
    assert eng._b and all(bk.Bt >= eng.fp8_min_batch for bk in eng._b.values())


ENGINE_ARMS = [(k, p, g) for k in ("policy", "value") for p in ("bf16", "fp8") for g in (True, False)]


# ------------------------------------------------------------- (a) addresses survive a refresh
def device_tensors(engine):
    """{path: (data_ptr, shape, dtype)} of every device tensor the engine owns: its attributes, through
    lists, tuples and dicts, and the attributes of every bucket."""
    from alphago_amd.models.inference import _Bucket

    found = {}

    def visit(path, v):
        if isinstance(v, torch.Tensor):
            if v.is_cuda:
                found[path] = (v.data_ptr(), tuple(v.shape), v.dtype)
        elif isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                visit("%s[%d]" % (path, i), e)
        elif isinstance(v, dict):
            for k, e in v.items():
                visit("%s[%r]" % (path, k), e)
        elif isinstance(v, _Bucket):
            for k, e in vars(v).items():
                visit("%s.%s" % (path, k), e)

    for k, v in vars(engine).items():
        visit(k, v)
    return found


@gpu
@pytest.mark.parametrize("kind,precision,use_graphs", ENGINE_ARMS)
def test_refresh_keeps_addresses(cuda_device, monkeypatch, kind, precision, use_graphs):
    """A captured graph holds the addresses of everything it reads, so ``sync_weights`` may rebind no
    device tensor of the engine or of a bucket: the set of (path, address, shape, dtype) is the same
    before and after a refresh.  Whoever adds a tensor to the engine gets this check for it."""
    monkeypatch.setenv("ALPHAGO_AMD_FP8_MIN_BATCH", str(NB))
    net = make_net(kind, cuda_device, 11)
    eng = make_engine(kind, net, cuda_device, precision=precision, use_graphs=use_graphs)
    planes, legal = boards(1)
    run(eng, kind, planes, legal)  # a graph exists (use_graphs) and every lazy buffer is allocated
    torch.cuda.synchronize()
    before = device_tensors(eng)
    bucket = "_b[(%d, 0)]." % NB
    must = ["wf[0]", "wf[2]", "bias_p[0]", "head_w", "head_b", bucket + "X0", bucket + "legal"]
    must += ["wf_ws[%d]" % l for l, w in enumerate(eng.wf_ws) if w is not None]
    if precision == "fp8":
        assert_fp8_ran(eng)
        must += ["w8[0]", "w8[2]", "scales8", "osc8", "amax8", bucket + "X08"]
    must += ["fc[0]", "fc[1]", "fc[2]", "fc[3]", bucket + "values"] if kind == "value" else [bucket + "probs"]
    assert not [m for m in must if m not in before], "the walk misses %s" % [m for m in must if m not in before]
    perturb(net, "all", 12)
    eng.sync_weights()
    torch.cuda.synchronize()
    after = device_tensors(eng)
    moved = sorted(k for k in before if after.get(k) != before[k])
    assert not moved, "rebound by sync_weights: %s" % moved
    assert sorted(after) == sorted(before)


# ------------------------------------------------------- (b) refresh after capture: the new network
def _refresh_cases():
    for kind, precision, use_graphs in ENGINE_ARMS:
        for group in (POLICY_GROUPS if kind == "policy" else VALUE_GROUPS):
            yield pytest.param(kind, precision, use_graphs, group,
                               id="%s-%s-%s-%s" % (kind, precision, "graph" if use_graphs else "eager", group))


@gpu
@pytest.mark.parametrize("kind,precision,use_graphs,group", list(_refresh_cases()))
def test_refresh_after_capture(cuda_device, monkeypatch, kind, precision, use_graphs, group):
    """Evaluate, re-draw one parameter group (or all) in place, ``sync_weights``, evaluate again: bitwise
    the output of a fresh engine built after the change, and not the output from before it (but for the
    policy's head bias alone: softmax is shift-invariant).  fp8: both engines recalibrate on the same
    boards, so weight and activation exponents agree too."""
    monkeypatch.setenv("ALPHAGO_AMD_FP8_MIN_BATCH", str(NB))
    net = make_net(kind, cuda_device, 11)
    kw = dict(precision=precision, use_graphs=use_graphs)
    eng = make_engine(kind, net, cuda_device, **kw)
    planes, legal = boards(1)
    before = run(eng, kind, planes, legal)
    if precision == "fp8":
        assert_fp8_ran(eng)
    anchor = precision == "bf16" and group == "all"
    old64 = ref64(net, kind, planes, legal) if anchor else None
    perturb(net, group, 12)
    eng.sync_weights()
    out = run(eng, kind, planes, legal)
    fresh = make_engine(kind, net, cuda_device, **kw)
    want = run(fresh, kind, planes, legal)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert bool(torch.isfinite(out).all())
    if precision == "fp8":
        assert_fp8_ran(eng)
        assert_fp8_ran(fresh)
        assert eng.ew == fresh.ew and eng.ex == fresh.ex
    if not (kind == "policy" and group == "head_b"):
        assert not torch.equal(out, before)
    if anchor:
        new64 = ref64(net, kind, planes, legal)
        margin = (new64 - old64).abs().max().item()
        d_new = (out.double().cpu() - new64).abs().max().item()
        d_old = (out.double().cpu() - old64).abs().max().item()
        print("refresh anchor %s graphs=%s: d_new %.3g d_old %.3g (references apart by %.3g)"
              % (kind, use_graphs, d_new, d_old, margin))
        assert ANCHOR * d_new <= d_old


def test_reference_margin_cpu():
    """The anchor's precondition, on the references alone: the float64 forwards of the two weight sets
    of test_refresh_after_capture differ by at least REF_MARGIN on its boards, for both nets."""
    planes, legal = boards(1)
    for kind in ("policy", "value"):
        net = make_net(kind, "cpu", 11)
        old64 = ref64(net, kind, planes, legal)
        perturb(net, "all", 12)
        margin = (ref64(net, kind, planes, legal) - old64).abs().max().item()
        print("reference margin %s: %.3g" % (kind, margin))
        assert margin >= REF_MARGIN


def _wrapper(kind, device, seed):
    from alphago_amd.models.policy import CNNPolicy, CNNValue

    if kind == "policy":
        w = CNNPolicy(FEATS, device=device, board=SB, filters_per_layer=32, layers=3)
    else:
        w = CNNValue(FEATS, device=device, board=SB, filters_per_layer=32, layers=3, dense=64)
    roughen(w.model, 0.1, seed)
    return w


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=gpu)])
@pytest.mark.parametrize("kind", ["policy", "value"])
def test_load_weights_refreshes_wrapper(request, tmp_path, kind, device):
    """The RL loop's path: a wrapper that has already evaluated loads another network's weights file and
    from then on computes that network (``load_weights`` -> ``refresh`` -> ``sync_weights``)."""
    if device == "cuda":
        device = request.getfixturevalue("cuda_device")
    first, second = _wrapper(kind, device, 21), _wrapper(kind, device, 22)
    x = boards(3)[0]
    before = np.array(first.forward(x))
    path = str(tmp_path / "second.hdf5")
    second.save_weights(path)
    first.load_weights(path)
    got, want = np.array(first.forward(x)), np.array(second.forward(x))
    assert np.array_equal(got, want)
    assert not np.array_equal(got, before)


@gpu
def test_trainer_step_reaches_engine(cuda_device):
    """An engine on the net a trainer owns: FlatParams rebinds every ``p.data`` to a view of its flat
    buffer, and after a step ``sync_weights`` reads the stepped weights from there."""
    from alphago_amd.train.engine import HipPolicyTrainer

    net = make_net("policy", cuda_device, 31)
    eng = make_engine("policy", net, cuda_device)  # before the trainer takes the parameters over
    planes, legal = boards(1)
    before = run(eng, "policy", planes, legal)
    trainer = HipPolicyTrainer(net, NB, lr=0.1, device=cuda_device)
    g = torch.Generator().manual_seed(5)
    targets = torch.randint(0, SB * SB, (NB,), dtype=torch.int32, generator=g).to(cuda_device)
    trainer.step(torch.from_numpy(planes).to(cuda_device), targets)
    torch.cuda.synchronize()
    eng.sync_weights()
    out = run(eng, "policy", planes, legal)
    want = run(make_engine("policy", net, cuda_device), "policy", planes, legal)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert not torch.equal(out, before)


# ------------------------------------------------ (c) a reused bucket forgets its previous batch
@gpu
@pytest.mark.parametrize("kind,precision,symmetries", [("policy", "bf16", "none"), ("policy", "bf16", "all"),
                                                       ("value", "bf16", "none"), ("policy", "fp8", "none")])
def test_bucket_forgets_previous_batch(cuda_device, monkeypatch, kind, precision, symmetries):
    """A full batch of dense boards under a random mask, then fewer boards without a mask, then the same
    with one: the rows equal a fresh engine's, whose padding rows never held anything.  The fp8 fresh
    engine is given the first engine's activation scales (it would calibrate on other boards)."""
    monkeypatch.setenv("ALPHAGO_AMD_FP8_MIN_BATCH", str(NB))
    B, n = (4, 2) if symmetries == "all" else (NB, 3)
    net = make_net(kind, cuda_device, 11)
    kw = dict(precision=precision, symmetries=symmetries, buckets=(B,))
    eng = make_engine(kind, net, cuda_device, **kw)
    full, full_legal = boards(1, n=B)
    first = run(eng, kind, full, full_legal)
    few, few_legal = boards(2, n=n)
    for legal in (None, few_legal):
        out = run(eng, kind, few, legal)
        fresh = make_engine(kind, net, cuda_device, **kw)
        if precision == "fp8":
            assert_fp8_ran(eng)
            fresh._set_act_exponents(eng.ex[1:])
            fresh.calibrated = True
        want = run(fresh, kind, few, legal)
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        assert not torch.equal(out, first[:n])
        if legal is None:  # the mask of the batch before is gone from every row
            assert torch.equal(eng._b[(B, 0)].legal, torch.ones_like(eng._b[(B, 0)].legal))
        elif kind == "policy":
            illegal = torch.from_numpy(legal == 0)
            assert torch.equal(out.cpu()[illegal], torch.zeros(int(illegal.sum())))


@gpu
def test_batch_larger_than_every_bucket(cuda_device):
    """6 boards on an engine whose largest bucket is 4: ``bucket_for`` rounds up to 8, and the result is
    that of an engine that has the bucket of 8."""
    net = make_net("policy", cuda_device, 11)
    small = make_engine("policy", net, cuda_device, buckets=(4,))
    assert small.bucket_for(6) == 8
    planes, legal = boards(4, n=6)
    out = run(small, "policy", planes, legal)
    want = run(make_engine("policy", net, cuda_device, buckets=(8,)), "policy", planes, legal)
    torch.cuda.synchronize()
    assert out.shape == (6, SB * SB)
    assert torch.equal(out, want)
    assert list(small._b) == [(8, 0)]


# ----------------------------------------------------------------------------- encoded path
def game_states(n, seed, lo, hi, ko_last=0, size=19):
    """n positions of random games lo .. hi - 1 moves long; the last ``ko_last`` of them are played on
    from ``lo`` moves until a ko point stands."""
    from alphago_amd import go

    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        gs = go.GameState(size)
        length = int(rng.integers(lo, hi))
        played = 0
        while True:
            moves = gs.get_legal_moves(include_eyes=False)
            if not moves:
                break
            gs.do_move(moves[int(rng.integers(len(moves)))])
            played += 1
            if i >= n - ko_last:
                if played >= lo and gs.ko is not None:
                    break
            elif played >= length:
                break
        out.append(gs)
    return out


class Encoded:
    """19 x 19 positions for the encoded path: 8 late ones (ko points in the last rows, ladder bits,
    non-trivial sensible masks), 3 early ones and 5 from the middle game, with their encodings."""

    def __init__(self):
        from alphago_amd._native import engine
        from alphago_amd.features import DEFAULT_FEATURES, Preprocess

        self.features = DEFAULT_FEATURES
        self.late = game_states(8, 3, 200, 320, ko_last=2)
        self.early = game_states(3, 101, 5, 30)
        self.mid = game_states(5, 7, 60, 140)
        self.enc = {name: engine().encode_batch(getattr(self, name), True, 2) for name in ("late", "early", "mid")}
        self.planes = {name: Preprocess(DEFAULT_FEATURES).states_to_uint8(getattr(self, name))
                       for name in ("late", "early", "mid")}
        meta, lad = self.enc["late"][2], self.enc["late"][3]
        assert int(meta[:, 0].max()) >= 0 and int(meta[-1, 0]) >= 0  # a ko point, in a row that becomes padding
        assert lad.any()


@pytest.fixture(scope="module")
def encoded():
    return Encoded()


@pytest.fixture(scope="module")
def net19(cuda_device):
    from alphago_amd.models.nets import PolicyNet

    return roughen(PolicyNet(48, board=19, filters_per_layer=32, layers=3), 0.1, 6).to(cuda_device)


def engine19(net, device, features):
    from alphago_amd.models.inference import HipTrunkInference

    return HipTrunkInference(net, device, buckets=(NB,), feature_list=features)


def run_encoded(eng, enc, slot=0):
    probs, sens, bad = eng.evaluate_encoded(*enc, slot=slot)
    return probs.clone(), sens.clone(), list(bad)


def assert_same_encoded(got, want):
    assert torch.equal(got[0], want[0])  # probabilities
    assert torch.equal(got[1], want[1])  # sensible mask
    assert got[2] == want[2]  # overflow list


def test_encoded_positions_cpu(encoded):
    """The positions are what the encoded tests need them to be (host encoder only)."""
    for name, n in (("late", 8), ("early", 3), ("mid", 5)):
        b, a, m, l = encoded.enc[name]
        assert b.shape == (n, 361) and m.shape == (n, 2) and l.shape == (n, 361)
    assert (encoded.enc["late"][2][-2:, 0] >= 0).all()
    assert (encoded.enc["early"][2][:, 0] < 0).all()


@gpu
def test_encoded_bucket_forgets_previous_batch(cuda_device, encoded, net19):
    """8 late positions, then 3 early ones in the same bucket: ``e_meta`` (ko), ``e_ladder`` and the
    sensible mask of the padding rows are left over from the late batch and must not reach the rows."""
    eng = engine19(net19, cuda_device, encoded.features)
    late = run_encoded(eng, encoded.enc["late"])
    assert int(late[1].sum()) > 0 and not bool(late[1].all())  # a non-trivial sensible mask
    got = run_encoded(eng, encoded.enc["early"])
    want = run_encoded(engine19(net19, cuda_device, encoded.features), encoded.enc["early"])
    torch.cuda.synchronize()
    assert_same_encoded(got, want)
    assert not torch.equal(got[0], late[0][:3])


@gpu
def test_encoded_and_planes_interleave(cuda_device, encoded, net19):
    """Encoded, planes without a mask, encoded again on one bucket: each result is a fresh engine's, and
    the planes submission in the middle ran under an all-ones mask, not the sensible mask before it."""
    eng = engine19(net19, cuda_device, encoded.features)
    fresh = lambda: engine19(net19, cuda_device, encoded.features)  # noqa: E731
    planes = encoded.planes["mid"]
    a = run_encoded(eng, encoded.enc["late"])
    mid = run(eng, "policy", planes, None)
    mask = eng._b[(NB, 0)].legal.clone()
    b = run_encoded(eng, encoded.enc["early"])
    torch.cuda.synchronize()
    assert_same_encoded(a, run_encoded(fresh(), encoded.enc["late"]))
    assert torch.equal(mid, run(fresh(), "policy", planes, None))
    assert torch.equal(mask, torch.ones_like(mask)) and not bool(a[1].all())
    assert_same_encoded(b, run_encoded(fresh(), encoded.enc["early"]))


# -------------------------------------------------------------------- (d) two slots in flight
def _host_copy(collected):
    """``collect`` of a to_host submission returns views of the slot's pinned buffers."""
    out, mask, bad = collected
    return np.array(out), np.array(mask), list(bad)


@gpu
@pytest.mark.parametrize("fallback", [False, True])
def test_two_slots_in_flight(cuda_device, encoded, net19, fallback):
    """Two encoded batches submitted to slots 0 and 1 before either is collected (``fallback``: with a
    planes evaluation on slot 2 between them, the search's overflow fallback): each equals its serial
    evaluation on a fresh engine, and slot 0's device outputs are untouched by what ran after it."""
    eng = engine19(net19, cuda_device, encoded.features)
    A, B = encoded.enc["late"], encoded.enc["mid"]
    ha = eng.submit_encoded(*A, slot=0, to_host=True)
    dev_a = [t.clone() for t in eng.outputs(ha)]
    if fallback:
        fb = run(eng, "policy", encoded.planes["early"], None, slot=2)
    hb = eng.submit_encoded(*B, slot=1, to_host=True)
    got_b = _host_copy(eng.collect(hb))
    now_a = eng.outputs(ha)
    assert torch.equal(now_a[0], dev_a[0]) and torch.equal(now_a[1], dev_a[1])
    got_a = _host_copy(eng.collect(ha))
    for got, enc in ((got_a, A), (got_b, B)):
        want = run_encoded(engine19(net19, cuda_device, encoded.features), enc)
        assert np.array_equal(got[0], want[0].cpu().numpy())
        assert np.array_equal(got[1], want[1].cpu().numpy())
        assert got[2] == want[2]
    assert not np.array_equal(got_a[0][:5], got_b[0])
    if fallback:
        assert torch.equal(fb, run(engine19(net19, cuda_device, encoded.features), "policy", encoded.planes["early"],
                                   None))
        assert sorted(eng._b) == [(NB, 0), (NB, 1), (NB, 2)]


# ------------------------------------------------------ (e) set_encoded_planes after a capture
@gpu
def test_set_encoded_planes_after_capture(cuda_device, encoded, net19):
    """Toggling the uint8 plane output drops the captured encoded graph; the re-captured one writes the
    planes of ``Preprocess`` and the same probabilities, and toggling back takes the view away again."""
    eng = engine19(net19, cuda_device, encoded.features)
    enc, n = encoded.enc["late"], len(encoded.late)
    first = run_encoded(eng, enc)
    assert first[2] == []  # no overflow board: every board's planes come from the kernel
    with pytest.raises(RuntimeError):
        eng.encoded_planes_view(n)
    eng.set_encoded_planes(True)
    second = run_encoded(eng, enc)
    planes = eng.encoded_planes_view(n).clone()
    torch.cuda.synchronize()
    assert torch.equal(planes.cpu(), torch.from_numpy(encoded.planes["late"]))
    assert_same_encoded(second, first)
    eng.set_encoded_planes(False)
    third = run_encoded(eng, enc)
    torch.cuda.synchronize()
    assert_same_encoded(third, first)
    with pytest.raises(RuntimeError):
        eng.encoded_planes_view(n)
