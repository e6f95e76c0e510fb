"""Dual (policy + value) net against the policy / value pair on the GPU (random-init weights).

  leaf   one leaf-batch evaluation as the search runs it (encoded submission, results on the host):
         the 12 x 192 policy + 12 x 152 value pair (value net on a side stream up to 64 leaves) against
         one 12 x 192 dual net, at B = 32 and B = 1024, in the engines' precision
         (ALPHAGO_AMD_PRECISION=fp8 for the e4m3 trunk)
  genmove  single-tree genmove latency (1600 playouts, 32 leaves per batch) on seeded mid-game
         positions, pair against dual
  train  training step time at B = 2176: HipPolicyValueTrainer (49 planes) against HipPolicyTrainer
         (48 planes), both 12 x 192
  own    (not in the default set) the ownership head at B = 2176, 12 x 192: (a) the head alone, the fused
         pair value_own_head + head_backward_add2 against the composition of the older kernels that
         computes the same (head_logits twice, tanh / MSE elementwise in torch, head_backward_add
         twice); (b) the whole training step of the dual net with the head against the same net
         without it.  Prints the byte counts of one pass over the trunk output next to the times.

  --precision A[,B...] with train / leaf: the dual net alone in each named arm (bf16, fp8, and for train
         fp8-backward = the all-fp8 step), the arms alternating inside the process; --layers and --residual
         pick its trunk (e.g. train --layers 21 --residual --precision bf16,fp8,fp8-backward)

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


ARM_KW = {"bf16": {}, "fp8": {"precision": "fp8"},
          "fp8-backward": {"precision": "fp8", "fp8_dgrad": True, "fp8_wgrad": True}}


def bench_train_arms(dev, B, steps, repeats, arms, layers, residual):
    """The dual trainer's step in each arm of ARM_KW, alternating."""
    from alphago_amd.models.nets import PolicyValueNet
    from alphago_amd.train.engine import HipPolicyValueTrainer

    g = torch.Generator().manual_seed(0)
    moves = torch.randint(0, 361, (B,), dtype=torch.int32, generator=g).to(dev)
    z = (torch.randint(0, 2, (B,), generator=g) * 2 - 1).float().to(dev)
    sym = torch.randint(0, 8, (B,), dtype=torch.int32, generator=g).to(dev)
    x49 = torch.randint(0, 2, (B, 49, 19, 19), dtype=torch.uint8, generator=g).to(dev)
    sides = {}
    for arm in arms:
        torch.manual_seed(0)
        t = HipPolicyValueTrainer(PolicyValueNet(49, 19, 192, layers, residual=int(residual)), B, lr=0.003,
                                  device=dev, **ARM_KW[arm])
        sides[arm] = lambda t=t: t.step(x49, (moves, z), sym)
    res = _alternate(sides, 3, steps, repeats)
    return {"B": B, "layers": layers, "residual": bool(residual)} | {k + "_step_ms": spread(v) for k, v in res.items()}


def bench_leaf_arms(dev, B, iters, repeats, arms, layers, residual):
    """One encoded leaf-batch evaluation of the dual engine in each precision, alternating."""
    base = positions(min(B, 64), 1)
    states = [base[i % len(base)] for i in range(B)]
    engines = {}
    for arm in arms:
        torch.manual_seed(0)
        os.environ["ALPHAGO_AMD_PRECISION"] = arm  # read when the engine is made
        engines[arm] = CNNPolicyValue(VALUE_FEATURES, filters_per_layer=192, layers=layers, device=dev,
                                      **({"residual": 1} if residual else {})).engine
    enc = native().encode_batch(states, any(e.needs_ladder for e in engines.values()), 16)
    enc = [torch.as_tensor(np.ascontiguousarray(e)).pin_memory() if e is not None else None for e in enc]
    sides = {arm: (lambda e=e: e.collect(e.submit_encoded(*enc, to_host=True))) for arm, e in engines.items()}
    res = _alternate(sides, 10, iters, repeats)
    out = {"B": B, "layers": layers, "residual": bool(residual)}
    for k, v in res.items():
        out[k + "_ms"] = spread(v)
        out[k + "_evals_per_s"] = round(B / (float(np.median(v)) * 1e-3), 1)
    return out


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


def _alternate(sides, warm, iters, repeats):
    res = {k: [] for k in sides}
    for fn in sides.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t) / iters * 1e3)
    return res


def bench_own(dev, B, steps, repeats, only=None):
    from alphago_amd import ops
    from alphago_amd.models.nets import PolicyValueNet
    from alphago_amd.train.engine import HipPolicyValueTrainer

    ops.load()
    S, C, SS = 19, 192, 361
    g = torch.Generator().manual_seed(0)
    out = {"B": B, "bytes": {"pass_over_trunk_output": B * SS * C * 2}}
    pas = out["bytes"]["pass_over_trunk_output"]
    # reads of y, reads + writes of dz (the (B, S*S) rows and the weights are three orders smaller)
    out["bytes"].update(value_own_head=pas, head_backward_add2=3 * pas, fused_pair=4 * pas,
                        head_logits_x2=2 * pas, head_backward_add_x2=6 * pas, unfused_composition=8 * pas)
    if only in (None, "fused", "unfused"):
        y = torch.zeros(B, S + 2, S + 2, C, dtype=torch.bfloat16, device=dev)
        y[:, 1:-1, 1:-1] = torch.randn(B, S, S, C, generator=g).to(torch.bfloat16).clamp_min(0).to(dev)
        dz0 = torch.zeros_like(y)
        dz0[:, 1:-1, 1:-1] = (torch.randn(B, S, S, C, generator=g) * 1e-3).to(torch.bfloat16).to(dev)
        dz = dz0.clone()
        wv, wo = [(torch.randn(C, generator=g) * 0.05).to(dev) for _ in range(2)]
        bv, bo = [torch.randn(1, generator=g).to(dev) for _ in range(2)]
        t8 = torch.randint(-1, 2, (B, SS), generator=g).to(torch.int8).to(dev)
        tf = t8.float()
        sym = torch.zeros(B, dtype=torch.int32, device=dev)
        valid = torch.ones(B, device=dev)
        dzl = (torch.randn(B, SS, generator=g) / B).to(dev)  # the value head's dlogits, as the dense backward leaves them
        zv, own, olog, dlo = [torch.zeros(B, SS, device=dev) for _ in range(4)]
        oloss, oagree = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
        dh1, dh2 = torch.zeros(B, C + 1, device=dev), torch.zeros(B, C + 1, device=dev)
        gs = 1.0 / B

        def fused():
            ops.value_own_head(y, wv, bv, wo, bo, zv, S, own=own, target=t8, sym=sym, valid=valid, oloss=oloss,
                               oagree=oagree, dlo=dlo, grad_scale=gs)
            ops.head_backward_add2(y, wv, dzl, wo, dlo, dz, dh1, dh2, S)

        def unfused():
            ops.head_logits(y, wv, bv, zv, S)
            ops.head_logits(y, wo, bo, olog, S)
            torch.tanh(olog, out=own)
            e = own - tf
            oloss.copy_((e * e).mean(1))
            oagree.copy_(((torch.sign(own) == tf) & (tf != 0)).float().sum(1))
            dlo.copy_((valid * (gs * 2.0 / SS)).unsqueeze(1) * e * (1 - own * own))
            ops.head_backward_add(y, wv, dzl, dz, dh1, S)
            ops.head_backward_add(y, wo, dlo, dz, dh2, S)

        arms = {k: v for k, v in (("fused", fused), ("unfused", unfused)) if only in (None, k)}
        res = _alternate(arms, 3, 20 * steps, repeats)  # a call is a fraction of a millisecond: 20 x the step count per window
        out["head"] = {k + "_ms": spread(v) for k, v in res.items()}
        if len(res) == 2:
            f, u = res["fused"], res["unfused"]
            out["head"]["fused_faster_by_ms"] = round(float(np.median(u) - np.median(f)), 4)
            out["head"]["min_max_spread_ms"] = round(float(max(max(f) - min(f), max(u) - min(u))), 4)
        del y, dz, dz0
    if only in (None, "step"):
        moves = torch.randint(0, 361, (B,), dtype=torch.int32, generator=g).to(dev)
        z = (torch.randint(0, 2, (B,), generator=g) * 2 - 1).float().to(dev)
        sym = torch.randint(0, 8, (B,), dtype=torch.int32, generator=g).to(dev)
        x49 = torch.randint(0, 2, (B, 49, 19, 19), dtype=torch.uint8, generator=g).to(dev)
        ot = torch.randint(-1, 2, (B, SS), generator=g).to(torch.int8).to(dev)
        ov = torch.ones(B, device=dev)
        th = HipPolicyValueTrainer(PolicyValueNet(ownership=1), B, lr=0.003, device=dev)
        tn = HipPolicyValueTrainer(PolicyValueNet(), B, lr=0.003, device=dev)
        res = _alternate({"with_head": lambda: th.step(x49, (moves, z, (ot, ov)), sym),
                          "without_head": lambda: tn.step(x49, (moves, z), sym)}, 3, steps, repeats)
        out["step"] = {k + "_step_ms": spread(v) for k, v in res.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["leaf", "genmove", "train"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--positions", type=int, default=30)
    ap.add_argument("--train-batch", type=int, default=2176)
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--train-only", choices=["policy", "dual"], default=None, help="one trainer only (kernel traces)")
    ap.add_argument("--own-only", choices=["fused", "unfused", "step"], default=None,
                    help="own: one arm only (kernel traces)")
    ap.add_argument("--precision", default=None,
                    help="train / leaf: the dual net alone in these arms, joined with commas: bf16, fp8, "
                         "fp8-backward (train only)")
    ap.add_argument("--layers", type=int, default=12, help="with --precision: trunk layers of the dual net")
    ap.add_argument("--residual", action="store_true", help="with --precision: a residual trunk (odd --layers)")
    ap.add_argument("--leaf-batch", type=int, default=1024, help="with --precision: boards per leaf batch")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pv_benchmark measures on a GPU")
    dev = torch.device("cuda")
    if a.precision is not None:
        arms = a.precision.split(",")
        if any(x not in ARM_KW for x in arms):
            ap.error("--precision arms: " + ", ".join(ARM_KW))
        out = {"arms": arms}
        if "train" in a.what:
            out["train"] = bench_train_arms(dev, a.train_batch, a.train_steps, a.repeats, arms, a.layers, a.residual)
        if "leaf" in a.what:
            out["leaf"] = bench_leaf_arms(dev, a.leaf_batch, 200 if a.leaf_batch <= 64 else 30, a.repeats,
                                          [x for x in arms if x != "fp8-backward"], a.layers, a.residual)
        print(json.dumps(out))
        return
    if a.residual or a.layers != 12:
        ap.error("--layers / --residual go with --precision")
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
    if "own" in a.what:
        out["own"] = bench_own(dev, a.train_batch, a.train_steps, a.repeats, a.own_only)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
