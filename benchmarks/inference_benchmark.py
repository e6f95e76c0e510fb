"""Batched network evaluation throughput (policy 12x192 / 48 planes, value
12x152 / 49 planes) on the HIP engines: bf16 vs fp8 (e4m3 block-scaled MFMA),
uint8-plane input vs the encoded-board input with the GPU featurizer in the
graph.  Replaces the reference's batch-1 Theano forward per state
(policy.py:26-42).  Prints JSON: evaluations/s per configuration.

``--symmetries none,random,all`` times the symmetry-ensembled engines too (positions/s at the user
batch: an "all" engine runs an 8x trunk batch).  The arms of one batch alternate within every round
(``--rounds``); with more than one round the JSON holds the median and [min, max] over rounds."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from alphago_amd import go  # noqa: E402
from alphago_amd._native import engine  # noqa: E402
from alphago_amd.features import DEFAULT_FEATURES, VALUE_FEATURES  # noqa: E402
from alphago_amd.models.inference import HipTrunkInference, HipValueInference  # noqa: E402
from alphago_amd.models.nets import PolicyNet, ValueNet  # noqa: E402


def states(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        gs = go.GameState()
        for _ in range(int(rng.integers(10, 200))):
            mv = gs.get_legal_moves(include_eyes=False)
            if not mv:
                break
            gs.do_move(mv[int(rng.integers(len(mv)))])
        out.append(gs)
    return out


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--symmetries", default="none", help="comma-separated arms out of none, random, all")
    ap.add_argument("--batches", default="256,1024", help="comma-separated user batch sizes")
    ap.add_argument("--precisions", default="bf16,fp8")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--positions", type=int, default=256, help="distinct random positions (tiled up to the batch)")
    a = ap.parse_args()
    arms = a.symmetries.split(",")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    pnet = PolicyNet(48, filters_per_layer=192, layers=12).to(dev)
    vnet = ValueNet(49, filters_per_layer=152, layers=12).to(dev)
    base = states(a.positions)
    runs = {}
    for B in [int(b) for b in a.batches.split(",")]:
        st = (base * (B // len(base) + 1))[:B]
        enc = engine().encode_batch(st, True, 8)
        planes = torch.from_numpy(engine().featurize_batch(st, DEFAULT_FEATURES, 8)).to(dev)
        vplanes = torch.from_numpy(engine().featurize_batch(st, VALUE_FEATURES, 8)).to(dev)
        for prec in a.precisions.split(","):
            eng = {}
            for sym in arms:
                kw = {} if sym == "none" else {"symmetries": sym}  # "none": the plain engines' constructor
                eng[sym] = (HipTrunkInference(pnet, dev, feature_list=DEFAULT_FEATURES, precision=prec, **kw),
                            HipValueInference(vnet, dev, feature_list=VALUE_FEATURES, precision=prec, **kw))
            for _ in range(a.rounds):
                for sym in arms:
                    pe, ve = eng[sym]
                    tag = "" if sym == "none" else "_sym-" + sym
                    dt = timeit(lambda: pe.evaluate(planes), a.iters)
                    runs.setdefault("policy_%s_B%d_planes%s" % (prec, B, tag), []).append(B / dt)
                    dt = timeit(lambda: pe.evaluate_encoded(*enc), a.iters)
                    runs.setdefault("policy_%s_B%d_encoded%s" % (prec, B, tag), []).append(B / dt)
                    dt = timeit(lambda: ve.evaluate(vplanes), a.iters)
                    runs.setdefault("value_%s_B%d_planes%s" % (prec, B, tag), []).append(B / dt)
            del eng
            torch.cuda.empty_cache()
    out = {"evals_per_s": {k: round(statistics.median(v)) for k, v in runs.items()},
           "note": "encoded = GPU featurizer inside the HIP graph (incl. H2D of the "
                   "2-byte/point encoding; host ladder reading excluded)"}
    if a.rounds > 1:
        out["min_max"] = {k: [round(min(v)), round(max(v))] for k, v in runs.items()}
        out["rounds"] = a.rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
