"""The parts of the fp8 residual trunk that need no GPU: the per-layer plan of the fp8 inference trunk
(models.inference.fp8_trunk_plan) and train-pv's --fp8-backward argument handling."""
import pytest

from alphago_amd.models.inference import fp8_trunk_plan
from alphago_amd.train import pv

DEPTHS = list(range(3, 22, 2))  # a stem plus (L - 1) / 2 two-layer blocks


@pytest.mark.parametrize("L", DEPTHS)
def test_residual_plan(L):
    plan = fp8_trunk_plan(L, True)
    assert len(plan) == L
    bf16_written = {}  # bf16 buffer -> the layer that wrote it last
    for l, p in enumerate(plan):
        last, end = l == L - 1, l >= 2 and l % 2 == 0
        if end:  # the skip is the stream written exactly two layers earlier, and no output of this launch
            assert p.res is not None and bf16_written[p.res] == l - 2
            assert p.res != p.y_bf16
        else:
            assert p.res is None
        if l % 2 == 1:
            assert p.y_bf16 is None and p.y_fp8 is not None  # odd layers write no bf16
        else:
            assert p.y_bf16 is not None
        if last:
            assert p.y_bf16 is not None and p.y_fp8 is None  # the top writes bf16 only
        else:
            assert p.y_fp8 == l % 2  # layer l + 1 reads what layer l wrote, not what it writes itself
        assert p.y_bf16 is None or 0 <= p.y_bf16 < 3  # a residual bucket owns three bf16 buffers
        assert p.y_fp8 is None or 0 <= p.y_fp8 < 2    # and two e4m3 buffers
        if p.y_bf16 is not None:
            bf16_written[p.y_bf16] = l


@pytest.mark.parametrize("L", [1, 2, 4, 12, 13])
def test_plain_plan_is_the_old_one(L):
    """A plain trunk: e4m3 ping-pong, bf16 only from the top layer into buffer 0, no skip."""
    plan = fp8_trunk_plan(L, False)
    for l, p in enumerate(plan):
        last = l == L - 1
        assert p == ((0, None, None) if last else (None, l % 2, None))


ARGS = ["model.json", "data.h5", "out"]


def test_fp8_backward_needs_fp8_precision(capsys):
    with pytest.raises(SystemExit):
        pv._parser().parse_args(ARGS + ["--fp8-backward"])
    assert "--fp8-backward requires --precision fp8" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        pv._parser().parse_args(ARGS + ["--fp8-backward", "--precision", "bf16"])


def test_trainer_keywords():
    p = pv._parser()
    kw = pv.trainer_kwargs(p.parse_args(ARGS + ["--precision", "fp8", "--fp8-backward"]), False)
    assert kw["precision"] == "fp8" and kw["fp8_dgrad"] is True and kw["fp8_wgrad"] is True
    kw = pv.trainer_kwargs(p.parse_args(ARGS + ["--precision", "fp8"]), True)
    assert kw["precision"] == "fp8" and "fp8_dgrad" not in kw and "fp8_wgrad" not in kw and "own_coef" in kw
    kw = pv.trainer_kwargs(p.parse_args(ARGS), False)
    assert kw == {"value_coef": 1.0}
