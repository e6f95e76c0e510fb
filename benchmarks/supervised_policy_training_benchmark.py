"""SL training on the reference fixture dataset (the reference's version of this
benchmark was broken: benchmarks/supervised_policy_training_benchmark.py passed 6
positional args to run_training).  Runs a few epochs of the real CLI on the
1033-position fixture with the reference minimodel architecture and reports
positions/s from the metrics log.  Prints JSON.

    python benchmarks/supervised_policy_training_benchmark.py [backend] [--precision fp8 [--fp8-backward]]
                                                              [-B N] [-E N] [--epoch-length N]

``--precision fp8`` alone is the e4m3 forward with the bf16 backward; ``--fp8-backward`` adds the
all-fp8 trunk backward (its own configuration: never reported as the bf16 or fp8-forward figure)."""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from alphago_amd.models.policy import CNNPolicy  # noqa: E402
from alphago_amd.train.sl import run_training  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                       "reference_data", "hdf5", "alphago-vs-lee-sedol-features.hdf5")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("backend", nargs="?", default="hip" if torch.cuda.is_available() else "torch")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--fp8-backward", action="store_true", help="with --precision fp8: all-fp8 trunk backward")
    ap.add_argument("--minibatch", "-B", type=int, default=64)
    ap.add_argument("--epochs", "-E", type=int, default=3)
    ap.add_argument("--epoch-length", "-l", type=int, default=None, help="positions per epoch (default: the fixture)")
    args = ap.parse_args()
    if args.fp8_backward and args.precision != "fp8":
        ap.error("--fp8-backward requires --precision fp8")
    backend = args.backend
    extra = []
    if args.precision != "bf16":
        extra += ["--precision", args.precision]
    if args.fp8_backward:
        extra.append("--fp8-backward")
    if args.epoch_length:
        extra += ["--epoch-length", str(args.epoch_length)]
    with tempfile.TemporaryDirectory() as d:
        data = FIXTURE
        if not os.path.exists(data):  # no reference checkout: same schema, synthetic content
            import numpy as np
            from alphago_amd.io.h5lite import H5Writer
            data = os.path.join(d, "synthetic.h5")
            rng = np.random.default_rng(0)
            with H5Writer(data) as f:
                f["states"] = rng.integers(0, 2, (1033, 12, 19, 19), dtype=np.uint8)
                f["actions"] = rng.integers(0, 19, (1033, 2), dtype=np.uint8)
        pol = CNNPolicy(["board", "ones", "turns_since"], filters_per_layer=192, layers=12, device="cpu")
        j = os.path.join(d, "model.json")
        pol.save_model(j)
        metrics = os.path.join(d, "m.jsonl")
        meta = run_training([j, data, os.path.join(d, "out"), "-E", str(args.epochs), "-B", str(args.minibatch),
                             "-r", "0.003", "--backend", backend, "--metrics", metrics] + extra)
        rows = [json.loads(l) for l in open(metrics)]
        cfg = "bf16" if args.precision == "bf16" else ("fp8-fwd/fp8-bwd" if args.fp8_backward else "fp8-fwd/bf16-bwd")
        print(json.dumps({"backend": backend, "config": cfg, "minibatch": args.minibatch, "epochs": meta["epochs"],
                          "positions_per_s_last_epoch": rows[-1]["positions_per_s"]}))


if __name__ == "__main__":
    main()
