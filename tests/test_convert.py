"""SGF parsing and SGF->HDF5 conversion; bit-exact parity with the reference fixture."""
import glob
import os

import numpy as np
import pytest

from alphago_amd import go
from alphago_amd.data.convert import GameConverter, run_game_converter
from alphago_amd.io.h5lite import H5File
from alphago_amd.io.sgf import SGFParseError, parse
from alphago_amd.utils.gorecords import flatten_idx, gamestate_to_sgf, sgf_iter_states, sgf_to_gamestate, unflatten_idx

# the reference's test data (SGF records, its converter's HDF5 output), stored with the suite
REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_data")


def test_sgf_parser_basics():
    t = parse("(;GM[1]SZ[9]C[a \\] b]AB[aa][bb];B[cc];W[](;B[dd])(;B[ee]))")
    g = t[0]
    assert g.root.properties["AB"] == ["aa", "bb"]
    assert g.root.properties["C"] == ["a ] b"]
    assert [n.properties for n in g.rest] == [{"B": ["cc"]}, {"W": [""]}, {"B": ["dd"]}]
    with pytest.raises(SGFParseError):
        parse("(;B[aa]")


def test_idx_helpers():
    for p in [(0, 0), (3, 17), (18, 18)]:
        assert unflatten_idx(flatten_idx(p, 19), 19) == p


def test_sgf_roundtrip():
    gs = go.GameState(9)
    for m in [(2, 2), (6, 6), None, (4, 4)]:
        gs.do_move(m)
    gs2 = sgf_to_gamestate(gamestate_to_sgf(gs))
    assert np.array_equal(gs.board, gs2.board) and gs2.history == gs.history


def test_ab_aw_setup():
    with open(os.path.join(REF, "sgf", "ab_aw.sgf")) as f:
        gs = sgf_to_gamestate(f.read())
    assert gs.size == 19 and np.count_nonzero(gs.board) > 0


def test_conversion_matches_reference_fixture(tmp_path):
    """The reference fixture was produced by the reference converter with
    features board, ones, turns_since (12 planes); ours must be bit-identical."""
    conv = GameConverter(["board", "ones", "turns_since"])
    with H5File(os.path.join(REF, "hdf5", "alphago-vs-lee-sedol-features.hdf5")) as f:
        states, actions = f["states"].read(), f["actions"].read()
        offs = {k: tuple(f["file_offsets"][k].read()) for k in f["file_offsets"].keys()}
    for key, (start, n) in offs.items():
        path = os.path.join(REF, "sgf", key.split("::")[-1])
        planes, acts, err = conv.game_arrays(path, 19)
        assert err is None
        assert planes.shape[0] == n
        assert np.array_equal(acts, actions[start:start + n])
        assert np.array_equal(planes, states[start:start + n]), key


def test_converter_cli(tmp_path):
    out = str(tmp_path / "out.h5")
    n = run_game_converter(["--features", "board,ones,turns_since,liberties,sensibleness", "-o", out,
                            "-d", os.path.join(REF, "sgf")])
    assert n > 1000
    with H5File(out) as f:
        assert f["states"].shape == (n, 3 + 1 + 8 + 8 + 1, 19, 19)
        assert f["actions"].shape == (n, 2)
        assert list(f.attrs["features"])[0] == b"board"
        assert sum(int(f["file_offsets"][k].read()[1]) for k in f["file_offsets"].keys()) == n
    assert not os.path.exists(str(tmp_path / ".tmp.out.h5"))
    out2 = str(tmp_path / "rec.h5")
    assert run_game_converter(["-o", out2, "-d", REF, "-R"]) == n * 1 or os.path.exists(out2)


def test_converter_writes_reference_layout_and_matches_fixture(tmp_path):
    """Converter output uses the reference's storage layout (states chunked
    (64,F,S,S) + LZF, actions chunked (1024,2) + LZF, game_converter.py:71-86),
    round-trips through h5lite (whole reads and chunk-sliced row reads), and its
    contents equal the reference fixture's."""
    out = str(tmp_path / "lee.h5")
    sgfs = sorted(os.path.join(REF, "sgf", f) for f in os.listdir(os.path.join(REF, "sgf")) if "Lee" in f)
    conv = GameConverter(["board", "ones", "turns_since"])
    n = conv.sgfs_to_hdf5(sgfs, out, 19)
    with H5File(os.path.join(REF, "hdf5", "alphago-vs-lee-sedol-features.hdf5")) as f:
        ref_states, ref_actions = f["states"].read(), f["actions"].read()
        ref_offs = {k.split("::")[-1]: tuple(f["file_offsets"][k].read()) for k in f["file_offsets"].keys()}
    with H5File(out) as f:
        st, ac = f["states"], f["actions"]
        assert st.chunked and st._layout[2][:4] == (64, 12, 19, 19) and [x for x, _ in st._filters] == [32000]
        assert ac.chunked and ac._layout[2][:2] == (1024, 2) and [x for x, _ in ac._filters] == [32000]
        assert n == st.shape[0] == len(ref_states)
        got_offs = {k.split(":")[-1]: tuple(f["file_offsets"][k].read()) for k in f["file_offsets"].keys()}
        states, actions = st.read(), ac.read()
        for name, (s0, cnt) in ref_offs.items():
            g0, gcnt = got_offs[name]
            assert gcnt == cnt
            assert np.array_equal(states[g0:g0 + cnt], ref_states[s0:s0 + cnt]), name
            assert np.array_equal(actions[g0:g0 + cnt], ref_actions[s0:s0 + cnt]), name
        rng = np.random.default_rng(0)
        idx = rng.integers(0, n, 300)
        assert np.array_equal(st.rows(idx), states[idx])
        assert np.array_equal(st.read_rows(70, 200), states[70:200])
    assert os.path.getsize(out) < ref_states.nbytes // 4  # compressed
