"""fp64 oracles, first-order fp32 error bounds and seeded CPU inputs for the kernels that write the
weights: ops.sgd_update / sgd_update_sched / sgd_pack (pack.hip), ops.pack_weights and ops.pack_input
(pack.hip) and ops.dense_f32 (dense.hip).

tests/test_update_refs.py checks the oracles on the CPU (against train/engine.py, hand-computed values,
nested loops, and a list of mutants that the comparison must reject); tests/test_update_kernels.py holds
the HIP kernels to them.  Everything here runs on the CPU from seeded generators, so both files see the
same tensors.

Error bound of an update (``U24`` = 2^-24, the fp32 unit roundoff)
-----------------------------------------------------------------
Every fp32 rounding the kernel performs (pack.hip ``opt_update``) is counted once, at ``U24`` times the
magnitude of the exact value that is rounded, and propagated linearly to the outputs.  ``s`` is the fp32
step the kernel holds, ``gs`` = float32(gscale); the constants ``mom``, ``b1``, ``b2``, ``eps``,
``1.f - b1``, ``1.f - b2`` are the fp32 values the kernel holds (input preparation, no error).

SGD        p' = p - s g
           roundings: s g, the difference            e(p') = U (|s g| + |p'|)
momentum   v' = mom v - s g
           roundings: mom v, s g, the difference     e(v') = U (|mom v| + |s g| + |v'|)
           p' = p + v'                               e(p') = e(v') + U |p'|
nesterov   p' = (p + mom v') - s g
           roundings: mom v', p + mom v', s g, p'    e(p') = |mom| e(v') + U (|mom v'| + |p + mom v'| + |s g| + |p'|)
Adam       ge = g gs                                 e(ge) = U |ge|
           m' = b1 m + (1 - b1) ge
           roundings: b1 m, (1 - b1) ge, the sum     e(m') = U |b1 m| + (1 - b1) e(ge) + U |(1 - b1) ge| + U |m'|
           v' = b2 v + ((1 - b2) ge) ge
           t1 = (1 - b2) ge                          e(t1) = (1 - b2) e(ge) + U |t1|
           t2 = t1 ge                                e(t2) = |ge| e(t1) + |t1| e(ge) + U |t2|
           roundings: b2 v, the sum                  e(v') = U |b2 v| + e(t2) + U |v'|
           p' = p - (s m') / (sqrt(v') + eps)
           num = s m'                                e(num) = s e(m') + U |num|
           sq = sqrt(v')                             e(sq) = e(v') / (2 sq) + U sq      (0 where v' = 0: then e(v') = 0)
           den = sq + eps                            e(den) = e(sq) + U den
           q = num / den                             e(q) = e(num) / den + |num| e(den) / den^2 + U |q|
           the difference                            e(p') = e(q) + U |p'|
A contracted evaluation (an fma for a product and the following sum) performs fewer roundings, so the same
bound covers it.  The assertion is |got - ref| <= 2 * bound: the factor 2 covers the second-order terms,
a sqrtf or a division that is not correctly rounded, and the freedom to contract; there is no other slack.
Where the bound is 0 (dyadic data, untouched gaps) that is bit equality.
"""
import decimal
import fractions

import numpy as np
import torch

from conv_refs import BF16_SENTINEL, expected_pack  # noqa: F401  (re-exported for the two test files)

U24 = 2.0 ** -24
OPT_SGD, OPT_MOMENTUM, OPT_ADAM = 0, 1, 2
f32 = np.float32


def _d(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


# ----------------------------------------------------------------------------- hyper-parameters
def hyper(opt, lr=2.0 ** -3, gscale=1.0, mom=0.0, b1=0.9, b2=0.999, eps=1e-8, nesterov=False):
    return dict(opt=opt, lr=lr, gscale=gscale, mom=mom, b1=b1, b2=b2, eps=eps, nesterov=nesterov)


def kernel_constants(hp, lr=None):
    """The fp32 values the kernel computes with (as float64 numbers): the step ``s`` =
    float32(float32(lr) * float32(gscale)) for SGD and momentum, float32(lr) for Adam; ``lr`` overrides
    hp['lr'] (the device schedule's sched[3])."""
    lr = f32(hp["lr"] if lr is None else lr)
    gs = f32(hp["gscale"])
    b1, b2 = f32(hp["b1"]), f32(hp["b2"])
    s = lr if hp["opt"] == OPT_ADAM else f32(lr * gs)
    return dict(s=float(s), gs=float(gs), mom=float(f32(hp["mom"])), b1=float(b1), b2=float(b2),
                eps=float(f32(hp["eps"])), omb1=float(f32(1.0) - b1), omb2=float(f32(1.0) - b2))


MUTANTS = ("eps_in_sqrt", "adam_no_gscale", "momentum_gscale_twice", "nesterov_plain", "v_linear", "swap_m1_m2",
           "step_64ulp")


# ----------------------------------------------------------------------------- the update oracle
def update_oracle(hp, p, g, m1=None, m2=None, lr=None, mutant=None):
    """One Keras 1.0 step in fp64.  Returns {'p','m1','m2'} and {'p','m1','m2'} bounds (the module
    docstring's e(.)); entries the optimizer does not keep are None.  ``mutant``: one of MUTANTS, a wrong
    update for tests of the comparison's discriminating power."""
    k = kernel_constants(hp, lr)
    p, g = _d(p), _d(g)
    s, U = k["s"], U24
    if mutant == "step_64ulp":
        s = s * (1.0 + 64 * 2.0 ** -23)
    out = dict(p=None, m1=None, m2=None)
    err = dict(p=None, m1=None, m2=None)
    with np.errstate(invalid="ignore", divide="ignore"):
        if hp["opt"] == OPT_SGD:
            sg = s * g
            out["p"] = p - sg
            err["p"] = U * (np.abs(sg) + np.abs(out["p"]))
        elif hp["opt"] == OPT_MOMENTUM:
            v = _d(m1)
            if mutant == "momentum_gscale_twice":
                s = s * k["gs"]
            sg, mv = s * g, k["mom"] * v
            v1 = mv - sg
            ev = U * (np.abs(mv) + np.abs(sg) + np.abs(v1))
            out["m1"], err["m1"] = v1, ev
            if hp["nesterov"] and mutant != "nesterov_plain":
                mv1 = k["mom"] * v1
                t = p + mv1
                out["p"] = t - sg
                err["p"] = abs(k["mom"]) * ev + U * (np.abs(mv1) + np.abs(t) + np.abs(sg) + np.abs(out["p"]))
            else:
                out["p"] = p + v1
                err["p"] = ev + U * np.abs(out["p"])
        else:
            m, v = _d(m1), _d(m2)
            if mutant == "swap_m1_m2":
                m, v = v, m
            ge = g if mutant == "adam_no_gscale" else g * k["gs"]
            ege = U * np.abs(ge)
            bm, og = k["b1"] * m, k["omb1"] * ge
            mn = bm + og
            em = U * np.abs(bm) + k["omb1"] * ege + U * np.abs(og) + U * np.abs(mn)
            t1 = k["omb2"] * ge
            et1 = k["omb2"] * ege + U * np.abs(t1)
            t2 = t1 if mutant == "v_linear" else t1 * ge
            et2 = np.abs(ge) * et1 + np.abs(t1) * ege + U * np.abs(t2)
            bv = k["b2"] * v
            vn = bv + t2
            evn = U * np.abs(bv) + et2 + U * np.abs(vn)
            num = s * mn
            enum = s * em + U * np.abs(num)
            if mutant == "eps_in_sqrt":
                sq = np.sqrt(vn + k["eps"])
                den = sq
            else:
                sq = np.sqrt(vn)
                den = sq + k["eps"]
            esq = np.where(vn > 0, evn / (2 * np.where(sq > 0, sq, 1.0)), 0.0) + U * sq
            eden = esq + U * den
            q = num / den
            eq = enum / den + np.abs(num) * eden / den ** 2 + U * np.abs(q)
            out["p"] = p - q
            err["p"] = eq + U * np.abs(out["p"])
            out["m1"], out["m2"], err["m1"], err["m2"] = mn, vn, em, evn
    return out, err


def fma32(a, b, c):
    """float32 fma emulated through fp64 (the product of two fp32 numbers is exact in fp64)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def update_fp32(hp, p, g, m1=None, m2=None, lr=None, contract=False):
    """pack.hip opt_update in numpy float32, in the kernel's order; ``contract``: every product that feeds
    a sum goes into an fma, as a compiler that contracts would do."""
    k = {n: f32(v) for n, v in kernel_constants(hp, lr).items()}
    p, g = _d(p).astype(f32), _d(g).astype(f32)
    s = k["s"]
    out = dict(p=None, m1=None, m2=None)
    with np.errstate(invalid="ignore", divide="ignore"):
        if hp["opt"] == OPT_SGD:
            out["p"] = fma32(-s, g, p) if contract else p - s * g
        elif hp["opt"] == OPT_MOMENTUM:
            v = _d(m1).astype(f32)
            v1 = fma32(-s, g, k["mom"] * v) if contract else k["mom"] * v - s * g
            out["m1"] = v1
            if hp["nesterov"]:
                out["p"] = fma32(-s, g, fma32(k["mom"], v1, p)) if contract else p + k["mom"] * v1 - s * g
            else:
                out["p"] = p + v1
        else:
            m, v = _d(m1).astype(f32), _d(m2).astype(f32)
            ge = g * k["gs"]
            if contract:
                mn = fma32(k["omb1"], ge, k["b1"] * m)
                vn = fma32(k["omb2"] * ge, ge, k["b2"] * v)
            else:
                mn = k["b1"] * m + k["omb1"] * ge
                vn = k["b2"] * v + k["omb2"] * ge * ge
            out["m1"], out["m2"] = mn, vn
            out["p"] = p - s * mn / (np.sqrt(vn) + k["eps"])
    return out


# ----------------------------------------------------------------------------- the comparison
def mismatches(got, ref, bound):
    """Indices where not |got - ref| <= 2 bound (a NaN in ``got`` is a mismatch; where ``ref`` is NaN,
    an untouched NaN gradient for instance, ``got`` must be NaN too)."""
    got, ref, bound = _d(got), _d(ref), _d(bound)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - ref) <= 2.0 * bound
    ok |= np.isnan(got) & np.isnan(ref)
    return np.flatnonzero(~ok)


def accepted(got, ref, bound):
    return mismatches(got, ref, bound).size == 0


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements with a non-zero bound (the figure the summary reports)."""
    got, ref, bound = _d(got), _d(ref), _d(bound)
    m = bound > 0
    return float((np.abs(got - ref)[m] / bound[m]).max()) if m.any() else 0.0


def bit_equal(got, ref):
    """``got`` (fp32) equals the fp64 oracle exactly: the oracle value is an fp32 number and got is it."""
    got, ref = _d(got), _d(ref)
    return bool(np.array_equal(got, ref))


# ----------------------------------------------------------------------------- element inputs
def update_inputs(n, seed, dyadic=False, gscale=0.25, hp=None):
    """p, g, m1, m2 (float32 numpy, m2 >= 0) of ``n`` elements.

    dyadic: multiples of 2^-8 in [-4, 4]; with a power-of-two step and momentum every product and sum of an
    SGD / momentum step is exact (two steps from here stay below 24 bits).
    otherwise: normal draws, and from n >= 64 on the first 16 elements are the edges the bound must be tight
    at (``gscale`` and ``hp``'s b1 / eps place them): g = 0 with m2 = 0, |g gscale| around eps, a large |p|
    with a tiny step, cancelling b1 m and (1 - b1) ge, a small |p| under a large gradient."""
    r = np.random.default_rng(seed)
    if dyadic:
        p, g, m1 = (r.integers(-1024, 1025, n).astype(np.float64) / 256 for _ in range(3))
        m2 = np.abs(r.integers(-1024, 1025, n).astype(np.float64) / 256)
        return tuple(a.astype(f32) for a in (p, g, m1, m2))
    p = r.standard_normal(n)
    g = r.standard_normal(n) * 0.5
    m1 = r.standard_normal(n) * 0.1
    m2 = (r.standard_normal(n) * 0.1) ** 2
    if n >= 64:
        hp = hp or hyper(OPT_ADAM)
        eps, b1 = hp["eps"], hp["b1"]
        e = eps / gscale
        # g = 0 and m2 = 0: v' = 0, the quotient is s m' / eps
        g[0:3], m2[0:3], m1[0:3] = 0.0, 0.0, (0.0, 1e-9, -3e-10)
        # |g gscale| around eps (sqrt(v') of the order of eps and far below it)
        g[3:9] = (0.5 * e, e, 2 * e, -e, 30 * e, -40 * e)
        m2[3:9] = (0.0, 0.0, eps * eps, 4 * eps * eps, 0.0, 0.0)
        m1[3:9] = (0.0, 1e-9, -1e-9, 2e-9, 0.0, 1e-8)
        # a large |p| with a tiny step
        p[9:11], g[9:11] = (1000.0, -4096.5), (1e-3, -2e-3)
        # b1 m and (1 - b1) ge of opposite sign, nearly cancelling
        m1[11:13] = (0.3, -0.07)
        g[11:13] = -b1 * m1[11:13] / ((1.0 - b1) * gscale) * (1.0 + 1e-4)
        # a small |p| under a large gradient (the step's own error shows)
        p[13:16], g[13:16], m1[13:16] = (1e-3, -2e-4, 0.0), (1.0, -1.5, 2.0), (0.0, 0.0, 0.0)
    return tuple(a.astype(f32) for a in (p, g, m1, m2))


# ----------------------------------------------------------------------------- the schedule
def schedule_exact(lr0, decay, t, adam=None, prec=60):
    """lr_t of the Keras schedule at ``iterations`` = t as a Decimal of ``prec`` digits, from the exact
    rational values of the fp64 inputs: lr0 / (1 + decay t), times sqrt(1 - b2^(t+1)) / (1 - b1^(t+1)) with
    ``adam`` = (b1, b2)."""
    F = fractions.Fraction
    lr = F(lr0) / (1 + F(decay) * int(t))
    with decimal.localcontext() as ctx:
        ctx.prec = prec
        D = lambda fr: decimal.Decimal(fr.numerator) / decimal.Decimal(fr.denominator)  # noqa: E731
        if adam is None:
            return +D(lr)
        b1, b2 = F(adam[0]), F(adam[1])
        n = int(t) + 1
        return D(lr) * D(1 - b2 ** n).sqrt() / D(1 - b1 ** n)


def ulp32(x):
    return float(np.spacing(f32(abs(float(x)))))


def within_one_ulp32(got, exact):
    """float32 ``got`` within one fp32 ulp of the exact Decimal value."""
    return abs(decimal.Decimal(float(got)) - exact) <= decimal.Decimal(ulp32(float(exact)))


def rel_dev(got, exact):
    """|got - exact| / |exact| of an fp64 ``got`` against the exact Decimal, as a float."""
    return float(abs(decimal.Decimal(float(got)) - exact) / abs(exact))


def host_schedule(lr0, decay, t):
    """KerasSGDSchedule.current()'s SGD expression: three fp64 roundings."""
    return lr0 / (1.0 + decay * t)


def adam_schedule_bound(b1, b2, t):
    """Relative bound, in units of 2^-53, of KerasSGDSchedule.current() for Adam at ``iterations`` = t
    against the exact value, for a pow within one ulp: lr0 / (1 + decay t) contributes 4 (three roundings
    and the exactness of the inputs); pow's relative error 2 is amplified by the conditioning c(b) =
    b^n / (1 - b^n) of 1 - b^n, n = t + 1, plus that subtraction's own rounding; the square root halves its
    operand's error and rounds once; the product and the quotient round once each."""
    n = t + 1
    c1, c2 = b1 ** n / (1 - b1 ** n), b2 ** n / (1 - b2 ** n)
    return 4 + (2 * c2 + 1) / 2 + 1 + (2 * c1 + 1) + 2


# ----------------------------------------------------------------------------- the flat buffer of sgd_pack
# (Cout_real, Cin_real, K, Cout_p, Cin_p, packed-tap layout)
PACK_LAYERS = [
    (152, 49, 5, 160, 64, False),    # Cin_real not a multiple of 8 in a 64-wide pack; wd has the extra tap
    (152, 152, 3, 160, 160, False),  # extra tap in wf and wd
    (192, 192, 3, 192, 192, False),
    (8, 3, 3, 64, 8, False),         # Cin_real < 32; the second n-tile has no real rows
    (1, 192, 1, 64, 192, False),     # K = 1
    (192, 48, 5, 192, 64, True),     # packed-tap layout, no wd
]
RANGE_LENS = [0, 1, 7, 256, 16384 + 5]
GAPS = [3, 5, 1, 7, 2, 9, 1, 6, 3, 1, 2, 5]  # before each layer / range; the last is the tail


def flat_layout(layers=PACK_LAYERS, range_lens=RANGE_LENS):
    """Offsets of the layers and ranges in one flat buffer with gaps between them and a tail: returns
    (layer_offsets, ranges [(off, len)], total)."""
    off, lo, rg, gi = 0, [], [], 0
    for (co, ci, K, _, _, _) in layers:
        off += GAPS[gi % len(GAPS)]
        off += off % 4 == 0  # no layer and no range starts 16-byte aligned
        gi += 1
        lo.append(off)
        off += co * ci * K * K
    for n in range_lens:
        off += GAPS[gi % len(GAPS)]
        off += off % 4 == 0
        gi += 1
        rg.append((off, n))
        off += n
    return lo, rg, off + GAPS[gi % len(GAPS)]


def covered_mask(total, layers, layer_offsets, ranges):
    m = np.zeros(total, dtype=bool)
    for (co, ci, K, _, _, _), o in zip(layers, layer_offsets):
        m[o:o + co * ci * K * K] = True
    for o, n in ranges:
        m[o:o + n] = True
    return m


P_SENTINEL, M_SENTINEL = 12345.0, -777.0


def flat_inputs(seed, dyadic, layers=PACK_LAYERS, range_lens=RANGE_LENS, gscale=0.25):
    """p, g, m1, m2 (float32 numpy) over the flat layout: ``update_inputs`` everywhere, then in every gap
    and the tail a NaN gradient and a sentinel parameter / moment."""
    lo, rg, total = flat_layout(layers, range_lens)
    p, g, m1, m2 = (a[64:] for a in update_inputs(total + 64, seed, dyadic, gscale))  # without the edge elements
    cov = covered_mask(total, layers, lo, rg)
    # the edge elements go inside the first layer
    if not dyadic and lo:
        e = update_inputs(64, seed + 1, False, gscale)
        for a, b in zip((p, g, m1, m2), e):
            a[lo[0] + 8:lo[0] + 72] = b
    p[~cov], g[~cov], m1[~cov], m2[~cov] = P_SENTINEL, np.nan, M_SENTINEL, M_SENTINEL
    return p, g, m1, m2


def flat_oracle(hp, p, g, m1, m2, layers=PACK_LAYERS, range_lens=RANGE_LENS, lr=None, mutant=None, shift_layer=None):
    """update_oracle over the covered elements of the flat buffer; everything else unchanged with bound 0.
    ``shift_layer``: that layer's offset moved by one element (a mutant)."""
    lo, rg, total = flat_layout(layers, range_lens)
    if shift_layer is not None:
        lo = list(lo)
        lo[shift_layer] += 1
    cov = covered_mask(total, layers, lo, rg)
    out, err = update_oracle(hp, p, g, m1, m2, lr=lr, mutant=mutant)
    res, bnd = {}, {}
    for name, old in (("p", p), ("m1", m1), ("m2", m2)):
        if out[name] is None:
            res[name], bnd[name] = _d(old), np.zeros(total)
        else:
            res[name] = np.where(cov, out[name], _d(old))
            bnd[name] = np.where(cov, err[name], 0.0)
    return res, bnd


def layer_weights(flat, layers=PACK_LAYERS, layer_offsets=None):
    """The OIHW weights of every layer as views of a flat (numpy or torch) buffer, as torch tensors."""
    if layer_offsets is None:
        layer_offsets = flat_layout(layers)[0]
    t = flat if isinstance(flat, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(flat))
    return [t[o:o + co * ci * K * K].reshape(co, ci, K, K) for (co, ci, K, _, _, _), o in zip(layers, layer_offsets)]


# ----------------------------------------------------------------------------- packs
def pk_steps(T, cin_real):
    cpt = (cin_real + 7) // 8
    return (T * cpt + 7) // 8


def expected_pack_pk(w, cout_p):
    """The packed-tap first-layer layout of OIHW ``w`` (ops.packed_weight_pk's docstring, pack.hip
    wf_index): (steps, cout_p, 64) bf16 with w[n][c][t] at step q >> 3, slot (q & 7) * 8 + (c & 7),
    q = t cpt + (c >> 3), cpt = ceil(Cin_real / 8); zeros where t >= T, n >= Cout_real or c >= Cin_real."""
    co, ci, K, _ = w.shape
    T, cpt = K * K, (ci + 7) // 8
    out = torch.zeros(pk_steps(T, ci), cout_p, 64, dtype=torch.bfloat16)
    wb = w.to(torch.bfloat16).reshape(co, ci, T)
    t = torch.arange(T).view(T, 1).expand(T, ci)
    c = torch.arange(ci).view(1, ci).expand(T, ci)
    q = t * cpt + (c >> 3)
    out[q >> 3, :co, (q & 7) * 8 + (c & 7)] = wb.permute(2, 1, 0)  # indexed dims first: (T, ci, co)
    return out


def pk_unwritten(T, cin_real, cout_p):
    """Slots of the packed-tap layout with t >= T (the zero tail of the last step): ops.pack_weights
    writes zeros there, ops.sgd_pack does not write them."""
    cpt = (cin_real + 7) // 8
    m = torch.zeros(pk_steps(T, cin_real), cout_p, 64, dtype=torch.bool)
    for q in range(T * cpt, m.shape[0] * 8):
        m[q >> 3, :, (q & 7) * 8:(q & 7) * 8 + 8] = True
    return m


def pack_oracle(w, layer, mutant=None):
    """(wf, wd) of a PACK_LAYERS entry for OIHW ``w``, without the extra tap; wd is None in the packed-tap
    layout.  Mutants: 'no_flip' leaves wd's taps unflipped, 'padded_row' puts a 1 into a padded row."""
    co, ci, K, cout_p, cin_p, pk = layer
    if pk:
        wf, wd = expected_pack_pk(w, cout_p), None
    else:
        wf, wd = expected_pack(w, cin_p, cout_p)
        if mutant == "no_flip":
            wd = wf.transpose(1, 2).contiguous()
    if mutant == "padded_row" and cout_p > co:
        wf = wf.clone()
        wf[0, cout_p - 1, 0] = 1.0
    return wf, wd


def halfway_weights(shape, seed):
    """Non-integer fp32 weights, a third of them exactly halfway between two neighbouring bf16 numbers
    (both parities of the lower neighbour, so that round-to-nearest-even goes both ways)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g)
    b = w.to(torch.bfloat16).float().view(torch.int32)
    half = (b | 0x8000).view(torch.float32)  # the bf16 number with one more mantissa bit set: a tie
    pick = torch.rand(shape, generator=g) < 1 / 3
    return torch.where(pick, half, w)


# ----------------------------------------------------------------------------- pack_input
def pack_input_ref(planes, sym, targets, P, Cp, sentinel, rows=None):
    """(padded NHWC float (B, S + 2P, S + 2P, Cp), targets) that ops.pack_input must leave in a buffer that
    held ``sentinel``: train/engine.py apply_symmetry in the interior, zeros in the padded channels, the
    sentinel on all four borders; a row outside the pool is an all-zero board."""
    from alphago_amd.train.engine import apply_symmetry, symmetry_tables

    if rows is not None:
        npool = planes.shape[0]
        valid = (rows >= 0) & (rows < npool)
        planes = planes[rows.clamp(0, npool - 1)] * valid.view(-1, 1, 1, 1).to(planes.dtype)
    B, C, S, _ = planes.shape
    out, tout = apply_symmetry(planes, targets, sym, symmetry_tables(S))
    ref = torch.full((B, S + 2 * P, S + 2 * P, Cp), float(sentinel))
    ref[:, P:P + S, P:P + S, :] = 0.0
    ref[:, P:P + S, P:P + S, :C] = out.permute(0, 2, 3, 1).float()
    return ref, tout


# ----------------------------------------------------------------------------- dense
DENSE_BM, DENSE_BK = 64, 32


def dense_splits(M, N, K):
    """dense.hip dense_splits: the requested split count."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    s = min((256 + tiles - 1) // tiles, (K + 4 * DENSE_BK - 1) // (4 * DENSE_BK))
    return max(s, 1)


def dense_launch_splits(M, N, K):
    """(requested, kchunk, launched) as launch_dense_f32 computes them."""
    s = dense_splits(M, N, K)
    kchunk = ((K + s - 1) // s + DENSE_BK - 1) // DENSE_BK * DENSE_BK
    return s, kchunk, (K + kchunk - 1) // kchunk


def dense_recomputed_k(M, N, kmax=1 << 15):
    """The smallest K at which the launcher's recomputed split count is below the requested one (the
    rounding of kchunk up to a multiple of 32 empties the last splits)."""
    for K in range(1, kmax):
        s, _, launched = dense_launch_splits(M, N, K)
        if launched < s:
            return K
    raise AssertionError("no such K below %d" % kmax)


def dense_inputs(M, N, K, ta, tb, seed):
    """Integer operands |a|, |b| <= 8, an integer bias and an even-integer C0: every partial sum is an
    integer below 2^24 (K 64 + 8 + 64 at most for the K used here), so fp32 is exact in any order."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-8, 9, (K, M) if ta else (M, K), generator=g).float()
    B = torch.randint(-8, 9, (N, K) if tb else (K, N), generator=g).float()
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    C0 = (torch.randint(-32, 33, (M, N), generator=g) * 2).float()
    return A, B, bias, C0


def dense_oracle(A, B, bias, C0, ta, tb, beta):
    """C = beta C0 + op(A) op(B) + bias in fp64 (C0 is not read when beta == 0)."""
    a = A.double().t() if ta else A.double()
    b = B.double().t() if tb else B.double()
    c = a @ b
    if bias is not None:
        c = c + bias.double()
    if beta != 0:
        c = c + beta * C0.double()
    return c


# (M, N, K, transA, transB, bias, beta) of the GPU test: pairs, not the full product
DENSE_K_RECOMPUTED = 8193  # dense_recomputed_k(65, 65): 64 splits requested, kchunk 160, 52 launched
DENSE_SHAPES = [(1, 1, 1), (31, 65, 2), (32, 64, 31), (33, 63, 32), (63, 33, 33), (64, 32, 128), (65, 31, 129),
                 (1, 65, 385), (65, 1, 385), (33, 33, 385), (64, 64, 129), (32, 32, 128), (65, 65, DENSE_K_RECOMPUTED),
                 (31, 31, DENSE_K_RECOMPUTED), (63, 64, 2), (64, 65, 129)]
DENSE_CASES = [(M, N, K, bool(i & 1), bool(i & 2), i % 3 != 1, (0.0, 1.0, 0.5)[(i // 2) % 3])
                for i, (M, N, K) in enumerate(DENSE_SHAPES)]
# every transpose pair and every beta on the single-pass path and on the split path, with and without bias
DENSE_CASES += [(33, 65, 33, True, True, True, 0.5), (33, 65, 385, False, False, False, 1.0),
                 (65, 33, 385, True, True, True, 0.0), (33, 65, 385, False, True, True, 0.5),
                 (63, 31, 129, True, False, False, 0.0), (1, 1, 385, True, True, False, 1.0)]
