"""CPU checks of the oracles in head_refs.py that test_head_kernels.py holds the HIP kernels to."""
import math

import pytest
import torch

import head_refs as R


def test_mix64_is_splitmix64():
    """First outputs of splitmix64 from state 0 (the published test vector of the generator)."""
    assert R.mix64(0) == 0xE220A8397B1DCDAF
    assert R.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4  # its second output
    assert R.u01(0, 0) == (0xE220A8397B1DCDAF >> 40) / 2.0 ** 24
    assert all(0.0 <= R.u01(s, b) < 1.0 for s in (0, 1, 2 ** 63 - 1) for b in range(64))


def test_clip_constants_are_fp32():
    assert R.EPS_LO != 1e-7 and abs(R.EPS_LO - 1e-7) < 1e-14
    assert R.EPS_HI == 1.0 - 2.0 ** -23  # fp32(1) - fp32(1e-7) rounds to the next fp32 below 1 but one


@pytest.mark.parametrize("C,C_real,B,S", R.HEAD_SHAPES)
@pytest.mark.parametrize("regime", ["uniform", "clip"])
def test_head_cases_avoid_the_discontinuities(C, C_real, B, S, regime):
    """The GPU tests' inputs, on the fp64 reference alone: no probability within a factor 2 of a clip
    threshold, no argmax that fp32 could reorder, and the clip regime reaches every branch."""
    c = R.head_case(C, C_real, B, S, regime)
    z = R.logits64(c.y, c.w, c.b)
    p = torch.softmax(z, 1)
    assert R.clip_band_clear(p)
    assert R.argmax_is_decided(z, R.logits_bound(c.y, c.w, c.b))
    assert c.target[2].item() == -1 and not bool(c.y[..., C_real:].any())
    if regime == "clip":
        pt = p.gather(1, c.target.long().clamp_min(0).unsqueeze(1)).squeeze(1)
        assert pt[0].item() > R.EPS_HI and (p[0] < R.EPS_LO).sum().item() == S * S - 1
        assert pt[1].item() < R.EPS_LO
        inside = (p > R.EPS_LO) & (p < R.EPS_HI)
        assert bool(inside[1:].any(1).all()) and bool((p[1:] < R.EPS_LO).any(1).all())
        if B > 3:
            assert R.EPS_LO < pt[3].item() < R.EPS_HI
    else:
        assert torch.allclose(p[0], torch.full_like(p[0], 1.0 / (S * S)), rtol=1e-12, atol=0)
        assert R.first_argmax(z)[:2].tolist() == [0, 0]


def test_policy_ref_bce_matches_closed_form():
    """The autograd oracle against the formula in policy_head.h: dz_i = p_i (g_i - sum_j p_j g_j) with
    g = 0 outside the clip range; a board above the upper threshold has no gradient at all, a target
    below the lower one has g = 0 while the rest of the board still moves."""
    c = R.head_case(8, 8, 3, 9, "clip")
    gs = 1.0 / 3
    t = c.target.clone()
    t[2] = 4  # the third board gets a target here
    r = R.policy_ref(c.y, c.w, c.b, t, c.weight, gs, "bce")
    SS = 81
    p = r.probs
    oh = torch.nn.functional.one_hot(t.long(), SS).double()
    inside = (p >= R.EPS_LO) & (p <= R.EPS_HI)
    g = torch.where(inside, -(oh / p - (1 - oh) / (1 - p)) / SS, torch.zeros_like(p))
    dl = p * (g - (p * g).sum(1, keepdim=True)) * c.weight.double().unsqueeze(1) * gs
    assert torch.allclose(r.dlogits, dl, rtol=1e-9, atol=1e-18)
    assert r.dlogits[0].abs().max().item() == 0 and r.dz[0].abs().max().item() == 0
    assert g[1, c.target[1]].item() == 0 and r.dlogits[1].abs().max().item() > 0
    assert abs(r.loss[0].item() + (math.log(R.EPS_HI) + 80 * math.log1p(-R.EPS_LO)) / SS) < 1e-12


def test_policy_ref_ce_clips_the_loss_only():
    c = R.head_case(8, 8, 3, 9, "clip")
    r = R.policy_ref(c.y, c.w, c.b, c.target, c.weight, 1.0, "ce")
    assert abs(r.loss[1].item() + math.log(R.EPS_LO)) < 1e-12 and r.loss[2].item() == 0
    oh = torch.nn.functional.one_hot(c.target.long().clamp_min(0), 81).double()
    dl = (r.probs - oh) * c.weight.double().unsqueeze(1)
    dl[2] = 0
    assert torch.allclose(r.dlogits, dl, rtol=1e-9, atol=1e-18)
    assert r.correct.tolist() == [1.0, 0.0, 0.0]


@pytest.mark.parametrize("beta", [1.0, 0.5, 2.0])
@pytest.mark.parametrize("NP", [81, 362])
def test_sample_oracle_separates_neighbours(NP, beta):
    """The interval check accepts the exact inverse-CDF index with no miss and rejects the next
    positive entry on either side by far more than any tolerance the GPU test uses (1e-4)."""
    p, has = R.sample_case(NP, 512)
    seed = 1
    idx = R.sample_exact(p, beta, seed)
    assert idx[R.ROW_ONE_HOT].item() == NP // 3 and idx[R.ROW_LAST_ONLY].item() == NP - 1
    assert idx[R.ROW_ALL_ZERO].item() == -1
    miss, pos = R.sample_miss(p, beta, seed, idx)
    assert miss.max().item() == 0 and bool(pos.all())
    w, _ = R.sample_cdf(p, beta)
    for step in (1, -1):
        out = idx.clone()
        for b in range(4, 512):
            j = idx[b].item() + step
            while 0 <= j < NP and not w[b, j] > 1e-6:
                j += step
            if 0 <= j < NP:
                out[b] = j
        moved = out != idx
        m, _ = R.sample_miss(p, beta, seed, out)
        assert bool((m[moved] > 0).all())
        # nearly every off-by-one lands well outside; the rest sit close to an edge of their interval
        assert (m[moved] > 1e-4).sum().item() > 0.9 * moved.sum().item() > 400
