"""Host side of the fp8 backward at the policy width: supported shapes, split counts, train-sl's flag."""
import pytest

from alphago_amd import ops
from alphago_amd.train import sl


def test_wgrad_fp8_supported_widths():
    assert ops.wgrad_fp8_supported(192, 192, 3) is True
    assert ops.wgrad_fp8_supported(160, 160, 3) is True
    assert ops.wgrad_fp8_supported(384, 384, 3) is False
    assert ops.wgrad_fp8_supported(192, 192, 5) is False
    assert ops.wgrad_fp8_supported(192, 160, 3) is False


@pytest.mark.parametrize("M,ns", [(81, 1), (1083, 9), (8664, 56), (2176 * 361, 56)])
def test_wgrad_fp8_nsplit_160_unchanged(M, ns):
    """The 160 call sites (positional K, default width) keep their split counts."""
    assert ops.wgrad_fp8_nsplit(M) == ns
    assert ops.wgrad_fp8_nsplit(M, 3) == ns
    assert ops.wgrad_fp8_nsplit(M, 3, width=160) == ns


@pytest.mark.parametrize("M", [81, 405, 1083, 2527, 8664, 32 * 361, 2176 * 361])
def test_wgrad_fp8_nsplit_192_one_resident_round(M):
    """192 x 96 tiles, 73,728 B of LDS each: two workgroups on each of the 256 CUs, and the grid
    nsplit x 9 taps x 2 tiles never exceeds that round; no more splits than 128-pixel steps."""
    ns = ops.wgrad_fp8_nsplit(M, 3, width=192)
    tiles = ops.wgrad_fp8_tiles(192)
    assert tiles == 2 and ops.wgrad_fp8_tiles(160) == 1
    assert 2 * 73728 <= 160 * 1024
    assert 1 <= ns <= (M + 127) // 128
    assert ns * 9 * tiles <= 2 * 256
    # ... and it fills the round when there is enough work
    assert ns == min((M + 127) // 128, 28)


def test_train_sl_parser_fp8_backward_flag():
    args = sl._parser().parse_args(["m.json", "d.h5", "out", "--precision", "fp8", "--fp8-backward"])
    assert args.precision == "fp8" and args.fp8_backward is True
    args = sl._parser().parse_args(["m.json", "d.h5", "out", "--precision", "fp8"])
    assert args.fp8_backward is False


@pytest.mark.parametrize("extra", [[], ["--precision", "bf16"]])
def test_train_sl_parser_rejects_fp8_backward_without_fp8(extra, capsys):
    with pytest.raises(SystemExit):
        sl._parser().parse_args(["m.json", "d.h5", "out", "--fp8-backward"] + extra)
    assert "--fp8-backward requires --precision fp8" in capsys.readouterr().err
