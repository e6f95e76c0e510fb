#!/usr/bin/env python
"""Record the reference traces replayed by tests/test_differential_reference.py.

    ALPHAGO_REFERENCE=/path/to/reference/checkout python scripts/make_reference_traces.py

Plays the tests' seeded random games on the reference rules engine and featurizer (tests/refshim.py
loads them from the checkout) and writes the moves and the state / feature-plane digests
(tests/reftrace.py) to tests/golden/reference_traces/*.npz.  The native engine is not involved: the
files hold the reference's behaviour only.  Re-run it only when the recorded cases change.
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import refshim  # noqa: E402
import reftrace  # noqa: E402
from alphago_amd.features import ALL_NO_LADDER_FEATURES  # noqa: E402  (a list of feature names)

RULES_CASES = [(7, 0), (9, 1), (9, 2), (13, 3), (19, 4)]
RULES_MOVES = {7: 120, 9: 200, 13: 300, 19: 350}
FEATURE_CASES = [(9, 5), (19, 6)]
SWEEP_CASES = ((9, 6000, 101), (13, 2500, 102), (19, 1500, 103))
PROPERTY_EXAMPLES, PROPERTY_SEED = 60, 2024


def _mv(mv):
    return reftrace.PASS if mv is None else mv


def _random_game(rg, size, n_moves, seed):
    """The reference game of one (size, seed) case: yields (move, state) after every move that does not
    end the game."""
    rnd = random.Random(seed)
    ref = rg.GameState(size)
    for _ in range(n_moves):
        legal = ref.get_legal_moves()
        mv = None if (not legal or rnd.random() < 0.03) else rnd.choice(legal)
        ref.do_move(mv)
        yield mv, ref
        if ref.is_end_of_game:
            break


def _save(name, **arrays):
    os.makedirs(reftrace.TRACES, exist_ok=True)
    path = os.path.join(reftrace.TRACES, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d bytes" % (path, os.path.getsize(path)), flush=True)


def rules(rg):
    for size, seed in RULES_CASES:
        moves, state, eyes = [], [], []
        for mv, ref in _random_game(rg, size, RULES_MOVES[size], seed):
            moves.append(_mv(mv))
            if ref.is_end_of_game:
                break
            state.append(reftrace.state_digest(ref))
            if (len(state) - 1) % 7 == 0:
                eyes.append(reftrace.eye_digest(ref))
        _save("rules_%d_%d" % (size, seed), moves=np.array(moves, np.int16), state=np.array(state, np.uint64),
              eyes=np.array(eyes, np.uint64))


def features(rg, rpp):
    for size, seed in FEATURE_CASES:
        moves, planes = [], []
        for i, (mv, ref) in enumerate(_random_game(rg, size, 260, seed)):
            moves.append(_mv(mv))
            if ref.is_end_of_game:
                break
            if i % 5 == 0:
                planes.append(reftrace.plane_digests(rpp.state_to_tensor(ref)[0]))
        _save("features_%d_%d" % (size, seed), moves=np.array(moves, np.int16), planes=np.array(planes, np.uint64))


def sweep(rg, rpp):
    for size, n, seed in SWEEP_CASES:
        rnd = random.Random(seed)
        ref = rg.GameState(size)
        moves, state, planes, restart = [], [], [], []
        while len(moves) < n:
            legal = ref.get_legal_moves()
            mv = None if (not legal or rnd.random() < 0.03) else rnd.choice(legal)
            ref.do_move(mv)
            moves.append(_mv(mv))
            state.append(reftrace.state_digest(ref))
            planes.append(reftrace.planes_digest(rpp.state_to_tensor(ref)[0]))
            new = bool(ref.is_end_of_game or len(ref.history) > 3 * size * size)
            restart.append(new)
            if new:
                ref = rg.GameState(size)
        _save("sweep_%d_%d" % (size, seed), moves=np.array(moves, np.int16), state=np.array(state, np.uint64),
              planes=np.array(planes, np.uint64), restart=np.array(restart, np.bool_))


def property_sequences(rg):
    """Seeded stand-ins for the property test's examples: board size from (5, 7, 9), 1 .. 150 picks in
    [0, 2^20], pick % (n_legal + 1) == n_legal meaning pass."""
    rnd = random.Random(PROPERTY_SEED)
    sizes, starts, moves, state = [], [0], [], []
    for _ in range(PROPERTY_EXAMPLES):
        size = rnd.choice([5, 7, 9])
        ref = rg.GameState(size)
        for _ in range(rnd.randint(1, 150)):
            legal = ref.get_legal_moves()
            k = rnd.randint(0, 1 << 20) % (len(legal) + 1)
            mv = None if k == len(legal) else legal[k]
            ref.do_move(mv)
            moves.append(_mv(mv))
            state.append(reftrace.state_digest(ref))
            if ref.is_end_of_game:
                break
        sizes.append(size)
        starts.append(len(moves))
    _save("property_sequences", sizes=np.array(sizes, np.int16), starts=np.array(starts, np.int32),
          moves=np.array(moves, np.int16), state=np.array(state, np.uint64))


def main():
    if not refshim.available():
        raise SystemExit("set ALPHAGO_REFERENCE to a checkout of the reference implementation")
    rg = refshim.ref_go()
    rpp = refshim.ref_preprocessing().Preprocess(ALL_NO_LADDER_FEATURES)
    rules(rg)
    features(rg, rpp)
    property_sequences(rg)
    sweep(rg, rpp)


if __name__ == "__main__":
    main()
