"""Dual (policy + value) net against the policy / value pair on the GPU (random-init weights).

  leaf   one leaf-batch evaluation as the search runs it (encoded submission, results on the host):
         the 12 x 192 policy + 12 x 152 value pair (value net on a side stream up to 64 leaves) against
         one 12 x 192 dual net, at B = 32 and B = 1024, in the engines' precision
         (ALPHAGO_AMD_PRECISION=fp8 for the e4m3 trunk)
  genmove  single-tree genmove latency (1600 playouts, 32 leaves per batch) on seeded mid-game
         positions, pair against dual
  train  training step time at B = 2176: HipPolicyValueTrainer (49 planes) against HipPolicyTrainer
         (48 planes), both 12 x 192

Every timed window is warmed up first and ends in a device synchronise (or the batch's own event);
the two sides alternate inside one process and every figure is the median of ``--repeats`` windows,
printed with their min and max.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from alphago_amd import go  # noqa: E402
from alphago_amd._native import engine as native  # noqa: E402
from alphago_amd.features import DEFAULT_FEATURES, VALUE_FEATURES  # noqa: E402
from alphago_amd.models.policy import CNNPolicy, CNNPolicyValue, CNNValue  # noqa: E402


def positions(n, seed, lo=40, hi=160):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        st = go.GameState()
        for _ in range(int(rng.integers(lo, hi))):
            moves = st.get_legal_moves(include_eyes=False)
            if not moves:
                break
            st.do_move(moves[int(rng.integers(len(moves)))])
        out.append(st)
    return out


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def bench_leaf(dev, pol, val, pv, B, iters, repeats):
    base = positions(min(B, 64), 1)
    states = [base[i % len(base)] for i in range(B)]
    pe, ve, de = pol.engine, val.engine, pv.engine
    ladder = pe.needs_ladder or ve.needs_ladder or de.needs_ladder
    enc = native().encode_batch(states, ladder, 16)
    enc = [torch.as_tensor(np.ascontiguousarray(e)).pin_memory() if e is not None else None for e in enc]
    side = torch.cuda.Stream(device=dev) if B <= 64 else None  # BatchedMCTS.VALUE_STREAM_MAX

    def pair():
        hp = pe.submit_encoded(*enc, to_host=True)
        if side is not None:
            with torch.cuda.stream(side):
                hv = ve.submit_encoded(*enc, to_host=True)
        else:
            hv = ve.submit_encoded(*enc, to_host=True)
        pe.collect(hp)
        ve.collect(hv)

    def dual():
        de.collect(de.submit_encoded(*enc, to_host=True))

    res = {"pair": [], "dual": []}
    for fn in (pair, dual):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for name, fn in (("pair", pair), ("dual", dual)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t) / iters * 1e3)
    return {"B": B, "pair_ms": spread(res["pair"]), "dual_ms": spread(res["dual"])}


def bench_genmove(pol, val, pv, n_pos, playouts, leaves):
    from alphago_amd.search.players import MCTSPlayer

    pos = positions(n_pos, 7)
    players = {"pair": MCTSPlayer(pol, val, n_playout=playouts, leaves_per_batch=leaves),
               "dual": MCTSPlayer(pv, None, n_playout=playouts, leaves_per_batch=leaves)}
    lat = {"pair": [], "dual": []}
    for p in players.values():  # warm-up: the buckets' graphs
        p.get_move(pos[0])
    for st in pos:
        for name, p in players.items():
            t = time.perf_counter()
            p.get_move(st)
            lat[name].append((time.perf_counter() - t) * 1e3)
    return {k + "_ms": {"p50": round(float(np.percentile(v, 50)), 2), "p95": round(float(np.percentile(v, 95)), 2)}
            for k, v in lat.items()} | {"positions": n_pos, "playouts": playouts, "leaves": leaves}


def bench_train(dev, B, steps, repeats, only=None):
    from alphago_amd.models.nets import PolicyNet, PolicyValueNet
    from alphago_amd.train.engine import HipPolicyTrainer, HipPolicyValueTrainer

    g = torch.Generator().manual_seed(0)
    moves = torch.randint(0, 361, (B,), dtype=torch.int32, generator=g).to(dev)
    z = (torch.randint(0, 2, (B,), generator=g) * 2 - 1).float().to(dev)
    sym = torch.randint(0, 8, (B,), dtype=torch.int32, generator=g).to(dev)
    sides = {}
    if only in (None, "policy"):
        x48 = torch.randint(0, 2, (B, 48, 19, 19), dtype=torch.uint8, generator=g).to(dev)
        tp = HipPolicyTrainer(PolicyNet(48, filters_per_layer=192, layers=12), B, lr=0.003, device=dev)
        sides["policy"] = lambda: tp.step(x48, moves, sym)
    if only in (None, "dual"):
        x49 = torch.randint(0, 2, (B, 49, 19, 19), dtype=torch.uint8, generator=g).to(dev)
        td = HipPolicyValueTrainer(PolicyValueNet(), B, lr=0.003, device=dev)
        sides["dual"] = lambda: td.step(x49, (moves, z), sym)
    res = {k: [] for k in sides}
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t) / steps * 1e3)
    return {"B": B} | {k + "_step_ms": spread(v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["leaf", "genmove", "train"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--positions", type=int, default=30)
    ap.add_argument("--train-batch", type=int, default=2176)
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--train-only", choices=["policy", "dual"], default=None, help="one trainer only (kernel traces)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pv_benchmark measures on a GPU")
    dev = torch.device("cuda")
    out = {"precision": os.environ.get("ALPHAGO_AMD_PRECISION", "bf16")}
    if "leaf" in a.what or "genmove" in a.what:
        torch.manual_seed(0)
        pol = CNNPolicy(DEFAULT_FEATURES, filters_per_layer=192, layers=12, device=dev)
        val = CNNValue(VALUE_FEATURES, filters_per_layer=152, layers=12, device=dev)
        pv = CNNPolicyValue(VALUE_FEATURES, filters_per_layer=192, layers=12, device=dev)
        fp, fv, fd = (m.model.flops_per_position() for m in (pol, val, pv))
        out["flops_per_position"] = {"policy": fp, "value": fv, "dual": fd, "dual_over_pair": round(fd / (fp + fv), 4)}
        if "leaf" in a.what:
            out["leaf"] = [bench_leaf(dev, pol, val, pv, B, 200 if B <= 64 else 30, a.repeats) for B in (32, 1024)]
        if "genmove" in a.what:
            out["genmove"] = bench_genmove(pol, val, pv, a.positions, 1600, 32)
    if "train" in a.what:
        out["train"] = bench_train(dev, a.train_batch, a.train_steps, a.repeats, a.train_only)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
