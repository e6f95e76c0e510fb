"""The dual (policy + value) inference engine against the pair of engines built from
``CNNPolicyValue.split()``: the same trunk weights in the same buckets run the same conv plan, so the
policy outputs are bit-equal and the values are bit-equal wherever the head takes head_logits' order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = 19


def _wrapper(device, F, L=2, seed=3):
    from alphago_amd.models.nets import he_uniform_
    from alphago_amd.models.policy import CNNPolicyValue

    torch.manual_seed(seed)
    pv = CNNPolicyValue(device=device, board=S, filters_per_layer=F, layers=L)
    he_uniform_(pv.model, generator=torch.Generator(device=device).manual_seed(seed))
    return pv


_NETS = {}


def _nets(device, F):
    """(dual wrapper, policy wrapper, value wrapper) of one width, made once."""
    if F not in _NETS:
        pv = _wrapper(device, F)
        _NETS[F] = (pv,) + tuple(pv.split())
    return _NETS[F]


def _engines(device, F, **kw):
    from alphago_amd.models.inference import HipPolicyValueInference, HipTrunkInference, HipValueInference

    pv, pol, val = _nets(device, F)
    return (HipPolicyValueInference(pv.model, device, **kw), HipTrunkInference(pol.model, device, **kw),
            HipValueInference(val.model, device, **kw))


def _planes(n, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 49, S, S)) < 0.4).astype(np.uint8), (rng.random((n, S * S)) < 0.6).astype(np.uint8)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("F", [64, 192])
def test_small_batch_equals_the_pair(cuda_device, F):
    """n = 7 (bucket 8, the 1024-thread head): probs and values bit-equal to the pair's."""
    dual, pe, ve = _engines(cuda_device, F)
    x, legal = _planes(7)
    probs, values = dual.evaluate(x, legal)
    p_ref = pe.evaluate(x, legal)
    v_ref = ve.evaluate(x)
    torch.cuda.synchronize()
    assert probs.shape == (7, S * S) and values.shape == (7,)
    assert torch.equal(_bits(probs), _bits(p_ref))
    assert torch.equal(_bits(values), _bits(v_ref))
    assert float(values.abs().max()) > 1e-3 and float(probs.max()) > 2.0 / (S * S)  # not a trivial net
    assert not bool((probs[torch.from_numpy(legal).to(cuda_device) == 0] != 0).any())


@pytest.mark.parametrize("F", [64, 192])
def test_large_batch_equals_the_pair(cuda_device, F):
    """n = 300 (bucket 512, the 512-thread row-mapped head): probs bit-equal; the value head's dot
    products take BoardRows' summation order there, so values agree within atol / rtol 2e-2
    (test_hip_value_grads_match_torch's tolerance)."""
    dual, pe, ve = _engines(cuda_device, F, buckets=(512,))
    x, legal = _planes(300, seed=1)
    probs, values = dual.evaluate(x, legal)
    p_ref = pe.evaluate(x, legal)
    v_ref = ve.evaluate(x)
    torch.cuda.synchronize()
    assert torch.equal(_bits(probs), _bits(p_ref))
    print("max |dv|: %.3g" % (values - v_ref).abs().max().item())
    torch.testing.assert_close(values.contiguous(), v_ref, atol=2e-2, rtol=2e-2)


def test_encoded_path_equals_the_pair(cuda_device):
    """evaluate_encoded (GPU featurizer in the graph) on game positions: one row of S*S probabilities
    and the value per position, equal to the pair's encoded outputs, masks and overflow lists; the
    to_host submission brings both home behind one event."""
    from alphago_amd._native import engine
    from alphago_amd.features import VALUE_FEATURES
    from test_engine_state import game_states

    states = game_states(5, 7, 60, 140)
    dual, pe, ve = _engines(cuda_device, 64, buckets=(8,), feature_list=list(VALUE_FEATURES))
    enc = engine().encode_batch(states, True, 2)
    out, mask, bad = dual.evaluate_encoded(*enc)
    probs, values = dual.split_outputs(out)
    p_ref, m_ref, b_ref = pe.evaluate_encoded(*enc)
    v_ref, _, vb_ref = ve.evaluate_encoded(*enc)
    torch.cuda.synchronize()
    assert out.shape == (5, S * S + 1)
    assert torch.equal(_bits(probs), _bits(p_ref)) and torch.equal(_bits(values), _bits(v_ref))
    assert torch.equal(mask, m_ref) and list(bad) == list(b_ref) == list(vb_ref)
    h = dual.submit_encoded(*enc, slot=1, to_host=True)
    hout, hmask, hbad = dual.collect(h)
    assert isinstance(hout, np.ndarray) and hout.shape == (5, S * S + 1)
    assert np.array_equal(hout, out.cpu().numpy()) and np.array_equal(hmask, mask.cpu().numpy()) and hbad == list(bad)


def test_weight_refresh_under_graphs(cuda_device):
    """A captured engine whose module weights then change in place computes, after refresh(), what a
    fresh engine computes (both heads' tensors are refreshed in place, never rebound)."""
    from alphago_amd.models.inference import HipPolicyValueInference

    pv = _wrapper(cuda_device, 64, seed=8)
    x, legal = _planes(7, seed=2)
    eng = pv.engine
    assert isinstance(eng, HipPolicyValueInference) and eng.use_graphs
    p0, v0 = [t.clone() for t in eng.evaluate(x, legal)]
    ptrs = [t.data_ptr() for t in eng.vhead + [eng.head_w, eng.head_b]]
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for p in pv.model.parameters():
            p.copy_(p + 0.5 * p.abs().mean() * torch.randn(p.shape, generator=g).to(p.device))
    pv.refresh()
    assert ptrs == [t.data_ptr() for t in eng.vhead + [eng.head_w, eng.head_b]]
    p1, v1 = [t.clone() for t in eng.evaluate(x, legal)]
    fresh = HipPolicyValueInference(pv.model, cuda_device)
    p2, v2 = fresh.evaluate(x, legal)
    torch.cuda.synchronize()
    assert torch.equal(_bits(p1), _bits(p2)) and torch.equal(_bits(v1), _bits(v2))
    assert not torch.equal(p0, p1) and not torch.equal(v0, v1)


def test_fp8_trunk(cuda_device):
    """precision="fp8" (the base trunk's) runs and stays within tests/test_fp8_inference.py's own
    tolerances of the bf16 engine: total variation < 0.15 per board, |dv| < 0.05 + 0.1 max |v|."""
    from alphago_amd.models.inference import HipPolicyValueInference

    pv = _nets(cuda_device, 192)[0]
    e16 = HipPolicyValueInference(pv.model, cuda_device, precision="bf16")
    e8 = HipPolicyValueInference(pv.model, cuda_device, precision="fp8")
    e8.fp8_min_batch = 0  # the fp8 trunk at this batch too
    x, _ = _planes(64, seed=4)
    p16, v16 = [t.float().cpu() for t in e16.evaluate(x)]
    p8, v8 = [t.float().cpu() for t in e8.evaluate(x)]
    assert e8.calibrated
    assert torch.allclose(p8.sum(1), torch.ones(64), atol=1e-3)
    tv = 0.5 * (p8 - p16).abs().sum(1)
    print("max TV %.3g, max |dv| %.3g" % (tv.max().item(), (v8 - v16).abs().max().item()))
    assert tv.max().item() < 0.15
    assert (v8 - v16).abs().max().item() < 0.05 + 0.1 * v16.abs().max().item()


def test_symmetries_are_refused(cuda_device):
    from alphago_amd.models.inference import HipPolicyValueInference, make_policy_value_inference

    pv = _nets(cuda_device, 64)[0]
    with pytest.raises(ValueError, match="does not ensemble"):
        HipPolicyValueInference(pv.model, cuda_device, symmetries="all")
    with pytest.raises(ValueError, match="does not ensemble"):
        make_policy_value_inference(pv.model, cuda_device, symmetries="random")
