"""Recorded traces of the reference implementation (differential tests without the reference).

``scripts/make_reference_traces.py`` plays seeded random games on the reference rules engine and
featurizer (loaded through refshim.py from a reference checkout) and records, per position, the move
played and 64-bit digests of the reference's state and feature planes into
``tests/golden/reference_traces/*.npz``.  The tests replay the moves on the native engine and
compare digests computed by the same functions, so a digest match means what the array comparison
against the live reference meant.  Only moves and digests are stored, nothing of the reference's
program text.
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRACES = os.path.join(GOLDEN, "reference_traces")
PASS = (-1, -1)  # a pass in a recorded move list


def _i16(a) -> bytes:
    return np.ascontiguousarray(np.asarray(a, dtype=np.int16)).tobytes()


def _digest(*parts) -> np.uint64:
    h = hashlib.blake2b(digest_size=8)
    for p in parts:
        h.update(len(p).to_bytes(4, "little"))
        h.update(p)
    return np.uint64(int.from_bytes(h.digest(), "little"))


def state_digest(gs) -> np.uint64:
    """Board, liberty counts, ko, side to move, prisoners, winner, end of game and the legal-move list
    (in order) of a GameState, the reference's or ours."""
    ko = PASS if gs.ko is None else tuple(gs.ko)
    scalars = [gs.current_player, gs.num_black_prisoners, gs.num_white_prisoners, gs.get_winner(),
               int(bool(gs.is_end_of_game))]
    legal = np.asarray(gs.get_legal_moves(), dtype=np.int16).reshape(-1, 2)
    return _digest(_i16(gs.board), _i16(gs.liberty_counts), _i16(ko), _i16(scalars), _i16(legal))


def eye_digest(gs) -> np.uint64:
    """is_eye of every empty point for both colours (row-major, black then white)."""
    size = gs.size
    out = [int(bool(gs.is_eye((x, y), c))) for x in range(size) for y in range(size) if gs.board[x, y] == 0
           for c in (1, -1)]
    return _digest(_i16(out))


def plane_digests(planes) -> np.ndarray:
    """One digest per feature plane of a (F, S, S) 0/1 array (the shape goes into each)."""
    p = np.asarray(planes)
    shape = _i16(p.shape)
    return np.array([_digest(shape, np.ascontiguousarray(p[i].astype(np.uint8)).tobytes())
                     for i in range(p.shape[0])], dtype=np.uint64)


def planes_digest(planes) -> np.uint64:
    """One digest of a whole (F, S, S) 0/1 array."""
    p = np.asarray(planes)
    return _digest(_i16(p.shape), np.ascontiguousarray(p.astype(np.uint8)).tobytes())


def to_move(row):
    """Recorded (x, y) row -> move (None = pass)."""
    x, y = int(row[0]), int(row[1])
    return None if (x, y) == PASS else (x, y)


def load(name):
    with np.load(os.path.join(TRACES, name + ".npz")) as z:
        return {k: z[k] for k in z.files}
