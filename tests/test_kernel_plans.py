"""Host-side kernel planning of the production library (no GPU needed: the HIP library's planning
functions run on the host): which layers and batches take the weight-stationary conv (tile 40), the
small-batch wgrad plan and the automatic wgrad / dgrad overlap."""
import pytest

from alphago_amd import ops

S2 = 361


@pytest.fixture(scope="module", autouse=True)
def _lib():
    try:
        ops.load()
    except Exception as e:  # noqa: BLE001 - no HIP runtime / library in this environment
        pytest.skip("production library not loadable here: %s" % e)


def test_weight_stationary_shapes():
    # the trunk layers of both nets and the policy's 5x5 first layer; not the value net's first layer
    assert ops.conv_ws_supported(192, 192, 3) and ops.conv_ws_supported(192, 64, 5)
    assert ops.conv_ws_supported(160, 160, 3) and ops.conv_ws_supported(128, 128, 3)
    assert ops.conv_ws_supported(64, 64, 3)
    assert not ops.conv_ws_supported(160, 64, 5)


def test_weight_stationary_batch_limits(monkeypatch):
    assert ops.ws_applies(1 * S2, 192, 192, 3) and ops.ws_applies(32 * S2, 192, 192, 3)
    assert not ops.ws_applies(33 * S2, 192, 192, 3)
    # inside training steps it stops at B = 16 (the side-stream wgrad shares the GPU there)
    assert ops.ws_applies(16 * S2, 192, 192, 3, training=True)
    assert not ops.ws_applies(17 * S2, 192, 192, 3, training=True)
    assert ops.ws_applies(32 * S2, 160, 160, 3) and not ops.ws_applies(17 * S2, 160, 160, 3, training=True)
    monkeypatch.setenv("ALPHAGO_AMD_WS", "0")
    assert not ops.ws_applies(1 * S2, 192, 192, 3)


POLICY_TRUNK, POLICY_FIRST, VALUE_TRUNK, VALUE_FIRST = (192, 192, 3), (192, 64, 5), (160, 160, 3), (160, 64, 5)
PLAN_BATCHES = (1, 2, 4, 8, 9, 16, 17, 32, 33, 64, 256, 2176)
WS, TILE = ("ws", 1, 40), ("tile", 1, 0)


def _split(n):
    return ("splitk", n, 38)


def _plans(shape, **kw):
    return {B: tuple(ops.plan_conv(B * S2, *shape, **kw)) for B in PLAN_BATCHES}


@pytest.mark.parametrize("training,last_ws", [(True, 16), (False, 32)])
def test_plan_conv_table(monkeypatch, training, last_ws):
    """ops.plan_conv at M = B * 361 against the values of ops.ws_applies / ops.splitk_nsplit the
    trainers and the inference buckets combined themselves before it existed."""
    monkeypatch.delenv("ALPHAGO_AMD_WS", raising=False)
    monkeypatch.delenv("ALPHAGO_AMD_SPLITK", raising=False)
    for shape in (POLICY_TRUNK, POLICY_FIRST, VALUE_TRUNK):
        assert _plans(shape, training=training) == {B: WS if B <= last_ws else TILE for B in PLAN_BATCHES}, shape
    # the value net's first layer has no weight-stationary instantiation: split-K, for both uses
    first = {1: _split(8), 2: _split(7), 4: _split(4), 8: _split(2)}
    assert _plans(VALUE_FIRST, training=training) == {B: first.get(B, TILE) for B in PLAN_BATCHES}
    # an explicit tile or small=False: the plain tile at every batch
    for shape in (POLICY_TRUNK, POLICY_FIRST, VALUE_TRUNK, VALUE_FIRST):
        assert set(_plans(shape, training=training, tile=386).values()) == {("tile", 1, 386)}
        assert set(_plans(shape, training=training, small=False).values()) == {TILE}
        assert set(_plans(shape, training=training, tile=386, small=False).values()) == {("tile", 1, 386)}
    monkeypatch.setenv("ALPHAGO_AMD_WS", "0")
    table = {POLICY_FIRST: (8, 7, 4, 2), POLICY_TRUNK: (9, 7, 4, 2), VALUE_TRUNK: (7, 7, 4, 2),
             VALUE_FIRST: (8, 7, 4, 2)}
    for shape, ns in table.items():
        want = dict(zip((1, 2, 4, 8), map(_split, ns)))
        assert _plans(shape, training=training) == {B: want.get(B, TILE) for B in PLAN_BATCHES}, shape
    monkeypatch.setenv("ALPHAGO_AMD_SPLITK", "0")
    for shape in table:
        assert set(_plans(shape, training=training).values()) == {TILE}, shape


def test_splitk_workspace_numel():
    M = 4 * S2
    plans = [ops.ConvPlan("ws", 1, 40), None, ops.ConvPlan("splitk", 4, 38), ops.ConvPlan("splitk", 7, 38),
             ops.ConvPlan("tile", 1, 0)]
    assert ops.splitk_workspace_numel(plans, M, 192) == 7 * M * 192
    assert ops.splitk_workspace_numel([plans[0], None, plans[4]], M, 192) == 0
    assert ops.splitk_workspace_numel([], M, 192) == 0


@pytest.mark.parametrize("B,small", [(1, False), (16, False), (17, True), (32, True), (64, True), (65, False),
                                     (2176, False)])
def test_small_batch_wgrad_plan(B, small):
    var, ns = ops.wgrad_config(B * S2, 192, 192, 3)
    assert (var == ops.WGRAD_SMALL) == small
    assert ns >= 1
    if small:
        taps, per_split, per_cu, threads = ops.wgrad_plan(192, 192, 3, 0, ops.WGRAD_SMALL)
        assert (taps, per_split, per_cu) == (3, 27, 2)
        assert ns * per_split <= 256 * per_cu  # one resident round
    # the first layer (48 real planes) and the value net's 160-wide layers keep their own plans
    assert ops.wgrad_config(B * S2, 192, 64, 5, cin_real=48)[0] == 0
    assert ops.wgrad_config(B * S2, 160, 160, 3)[0] == 0


# ----------------------------------------------------------------------------- forward / dgrad tile table
# code: (pixels per workgroup, waves, threads, K loop, chunk-outer K order, LDS slots), as the launch sites
# spelled them before the tile descriptions existed; LDS = slots x (BM + BN) x 128 bytes
FWD_TILES = {
    36: (32, 4, 256, "pipelined", False, 2), 37: (32, 2, 128, "pipelined", False, 2),
    38: (32, 4, 256, "pipelined", False, 2), 64: (64, 4, 256, "pipelined", False, 2),
    128: (128, 4, 256, "pipelined", False, 2), 256: (256, 8, 512, "pipelined", False, 2),
    384: (384, 8, 512, "plain", False, 2), 385: (384, 8, 512, "dma-spread", False, 2),
    386: (384, 8, 512, "dma-spread", True, 2), 387: (384, 8, 512, "plain", True, 2),
}
HALO388 = (388, 384, 8, 512, 2 * 432 * 128 + 2 * 192 * 128, "compact-halo", True, 2)  # 159744 B
LAB_TILES = (7, 8, 9, 10, 65, 130, 2560, 2568)
MODE_MASK, MODE_MASKBITS = 1, 3


def _row(code, bn):
    bm, waves, threads, loop, co, slots = FWD_TILES[code]
    return (code, bm, waves, threads, slots * (bm + bn) * 128, loop, co, slots)


@pytest.mark.parametrize("cout,bn", [(64, 64), (128, 128), (160, 160), (192, 192), (384, 192), (256, 128), (320, 64)])
def test_conv_fwd_tile_table(cout, bn):
    """Every production code on every width: the resolved code, BM, waves, threads, LDS bytes, loop, K order
    and ring depth of the tile that runs.  160-wide has no 37; the kernel-lab codes raise here."""
    for cin, K in ((cout if cout == 160 else 192, 3), (64, 5)):
        for code in FWD_TILES:
            if bn == 160 and code == 37:
                with pytest.raises(ValueError, match="160-wide tiles support tile codes"):
                    ops.conv_fwd_tile_info(S2, 19, K, cin, cout, tile=code)
                continue
            assert tuple(ops.conv_fwd_tile_info(S2, 19, K, cin, cout, tile=code)) == _row(code, bn), (code, cin, K)
        for code in LAB_TILES + (1, 39, 389):
            with pytest.raises(ValueError, match="160-wide tiles support" if bn == 160 else "unknown tile code %d" % code):
                ops.conv_fwd_tile_info(S2, 19, K, cin, cout, tile=code)


def test_conv_fwd_tile_388():
    """388 is the compact-halo kernel where it covers the layer and 386 everywhere else."""
    for mode in (0, MODE_MASKBITS):
        for res in (False, True):
            for S in (9, 13, 19):
                for cin in (64, 128, 192, 256):
                    assert tuple(ops.conv_fwd_tile_info(S2, S, 3, cin, 192, mode, res, 388)) == HALO388
            assert tuple(ops.conv_fwd_tile_info(S2, 19, 3, 192, 384, mode, res, 388)) == HALO388
    not_covered = [dict(S=19, K=3, cin_p=160, cout_p=160), dict(S=19, K=5, cin_p=64, cout_p=192),
                   dict(S=21, K=3, cin_p=192, cout_p=192), dict(S=19, K=3, cin_p=192, cout_p=192, mode=MODE_MASK),
                   dict(S=19, K=3, cin_p=192, cout_p=192, mode=2), dict(S=19, K=3, cin_p=128, cout_p=128),
                   dict(S=19, K=3, cin_p=64, cout_p=64), dict(S=19, K=3, cin_p=192, cout_p=192, Pin=0)]
    for kw in not_covered:
        got = ops.conv_fwd_tile_info(S2, tile=388, **kw)
        assert tuple(got) == _row(386, ops.conv_n_tile(kw["cout_p"])), kw


@pytest.mark.parametrize("cout,K,cin,edges", [
    # 192-wide, a layer the compact-halo kernel covers: 36 / 64 / 128 / 256 / 388
    (192, 3, 192, [(64 * 256 - 1, 36), (64 * 256, 64), (128 * 256 - 1, 64), (128 * 256, 128), (256 * 512 - 1, 128),
                   (256 * 512, 256), (384 * 512 - 1, 256), (384 * 512, 388), (2176 * S2, 388), (1, 36)]),
    # ... and one it does not cover (5x5): 386 at the top
    (192, 5, 64, [(64 * 256 - 1, 36), (64 * 256, 64), (128 * 256 - 1, 64), (128 * 256, 128), (256 * 512 - 1, 128),
                  (256 * 512, 256), (384 * 512 - 1, 256), (384 * 512, 386), (2176 * S2, 386)]),
    # 160-wide: the 32-pixel tile below 8192 pixels, then the same ladder; never the compact halo
    (160, 3, 160, [(8191, 36), (8192, 64), (64 * 256, 64), (128 * 256 - 1, 64), (128 * 256, 128), (256 * 512 - 1, 128),
                   (256 * 512, 256), (384 * 512 - 1, 256), (384 * 512, 386)]),
    (160, 5, 64, [(8191, 36), (8192, 64), (384 * 512, 386)]),
    (128, 3, 128, [(64 * 256 - 1, 36), (64 * 256, 64), (384 * 512 - 1, 256), (384 * 512, 386)]),
])
def test_conv_fwd_automatic_tile_edges(cout, K, cin, edges):
    """tile 0 one below and at each threshold of the automatic rule, for the forward and the bitmask dgrad, with
    and without a skip.  The build before fwd_resolve_tile had no host function to ask, so the expected codes are
    written out from the five ifs its launcher held (M >= 384*512 -> 386, >= 256*512 -> 256, >= 128*256 -> 128,
    else 64; 386 -> 388 where the compact halo covers; 36 below 64*256 pixels, below 8192 on 160-wide)."""
    for M, want in edges:
        for mode in (0, MODE_MASKBITS):
            for res in (False, True):
                assert ops.conv_fwd_tile_info(M, 19, K, cin, cout, mode, res).code == want, (M, mode, res)
        # the plain-mask dgrad and the epilogue-free mode have no compact-halo kernel
        for mode in (MODE_MASK, 2):
            assert ops.conv_fwd_tile_info(M, 19, K, cin, cout, mode).code == (386 if want == 388 else want)


# ----------------------------------------------------------------------------- wgrad plan = launch
def test_wgrad_plan_grid():
    """wgrad_plan and wgrad_tap_group over widths x real planes x kernel sizes x variants reproduce what the
    hand-kept plan answered (tests/wgrad_plan_golden.py), now that they read the launcher's own choice."""
    from wgrad_plan_golden import ROWS, VARIANTS

    assert VARIANTS[1] == ops.WGRAD_SMALL and len(ROWS) == 99
    widths = (64, 128, 160, 192)
    legal = [(co, ci) for co in widths for ci in widths if (co == 160) == (ci == 160) or (co == 160 and ci == 64)]
    assert sorted({k[:2] for k in ROWS}) == sorted(legal)
    bad = {}
    for (co, ci, cr, K), (group, plans) in ROWS.items():
        if ops.wgrad_tap_group(co, ci, K) != group:
            bad[(co, ci, cr, K, "tap group")] = ops.wgrad_tap_group(co, ci, K)
        for v, want in zip(VARIANTS, plans):
            got = tuple(ops.wgrad_plan(co, ci, K, cr, v))
            if got != want:
                bad[(co, ci, cr, K, v)] = (got, want)
    assert bad == {}


def test_wgrad_choice_tiles_and_lds():
    """The tile behind a plan: n x c widths and dynamic LDS bytes, 2 buffers x (WN + WC x taps) x 64 bytes x 32
    pixels as the launch sites computed them: the per-tap 192 x 192 tile, the value net's 160 x 160 on 4 waves, the
    tap-merged rows, the thin first layer's 48-wide rows (96-wide halves at 5x5) and the small-batch plan."""
    want = {(192, 192, 3, 0, 0): (1, 9, 2, 512, 192, 192, 49152), (160, 160, 3, 0, 0): (1, 9, 2, 256, 160, 160, 40960),
            (192, 64, 3, 0, 0): (3, 3, 2, 512, 192, 64, 49152), (160, 64, 5, 49, 0): (5, 5, 1, 512, 160, 64, 61440),
            (192, 64, 5, 48, 0): (5, 10, 2, 384, 96, 48, 43008), (192, 64, 3, 48, 0): (3, 3, 2, 384, 192, 48, 43008),
            (128, 192, 1, 0, 0): (1, 1, 2, 512, 128, 192, 40960), (64, 128, 3, 0, 0): (1, 9, 2, 512, 64, 128, 24576),
            (192, 192, 3, 0, ops.WGRAD_SMALL): (3, 27, 2, 512, 64, 64, 32768)}
    for (co, ci, K, cr, v), row in want.items():
        assert ops.wgrad_choice(co, ci, K, cr, v) == row, (co, ci, K, cr, v)
        assert ops.wgrad_choice(co, ci, K, cr, v)[:4] == tuple(ops.wgrad_plan(co, ci, K, cr, v))
    for co, ci in ((160, 128), (64, 160)):  # no tile for these width pairs: the plan raises as the launch does
        with pytest.raises(ValueError, match="conv_wgrad: C(out|in) 160"):
            ops.wgrad_plan(co, ci, 3)


def test_automatic_overlap_range():
    from alphago_amd.train.engine import OVERLAP_AUTO_MAX_PIXELS, OVERLAP_AUTO_MIN_PIXELS

    assert OVERLAP_AUTO_MIN_PIXELS == 17 * S2 and OVERLAP_AUTO_MAX_PIXELS == 256 * S2
