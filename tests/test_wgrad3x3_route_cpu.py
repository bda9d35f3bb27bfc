"""Which backward-weight calls wg_route (csrc/conv.hip) gives to the streaming 3x3 kernel (SPRK_STAGE_WGRAD3X3), asked
through sprk_conv2d_variant, which needs no GPU (the plans are those of a 256-CU device): with the switch on the admitted
shapes of tests/wgrad3x3_cases.py report stage 8 with the MFMA plan's record, with it off stage 5 and the same record;
the refusals, and the shapes whose plan is another one, report the same with the switch on and off."""
import pytest

import wgrad3x3_cases as w3


@pytest.fixture(autouse=True)
def _switch_back_on():
    yield
    w3.switch(1)


def _both(g, **kw):
    w3.switch(1)
    on = w3.query(g, **kw)
    w3.switch(0)
    off = w3.query(g, **kw)
    return on, off


@pytest.mark.parametrize("case", list(w3.TAKEN))
def test_taken(case):
    N, C1, C2, Cout, H, W, pad, tiles = w3.TAKEN[case]
    on, off = _both(w3.geom_of(N, C1, C2, Cout, H, W, pad), has_x2=C2 > 0)
    assert (on["stage"], off["stage"]) == (w3.WGRAD3X3, w3.MFMA), (on, off)
    assert {k: v for k, v in on.items() if k != "stage"} == {k: v for k, v in off.items() if k != "stage"}
    assert (on["IT"], on["MODE"], on["WJ"], on["tiles"]) == (7, 2, 2 if on["NT"] == 6 else 1, tiles), on
    assert on["NT"] == (3 if Cout <= 48 else 6) and on["c2"] == (C2 > 0) and on["chunks"] == (C1 + C2 > 48), on


@pytest.mark.parametrize("case", list(w3.PLANNED_ELSEWHERE))
def test_planned_elsewhere(case):
    on, off = _both(w3.geom_of(*w3.PLANNED_ELSEWHERE[case]))
    assert on == off and on["stage"] == w3.MFMA and on["MODE"] == 2 and on["IT"] < 7, (on, off)


# name -> stage and MODE with the switch on and off
REFUSED_AS = {"stride2": (5, 0), "dilation2": (5, 2), "5x5": (5, 2), "1x1": (5, 1), "up1": (5, 0), "60x44": (5, 2),
              "unaligned-x": (5, 0), "Cin40": (5, 2), "bf16": (5, 2), "storage16": (-1, 0)}


@pytest.mark.parametrize("case", list(w3.REFUSED))
def test_refused(case):
    what = w3.REFUSED[case][6]
    on, off = _both(w3.refused_geom(case), xoff=what.get("xoff", 0))
    assert on == off and (on["stage"], on["MODE"]) == REFUSED_AS[case], (on, off)


def test_pads_beyond_the_halo_are_refused():
    """a same-size 3x3 output needs pad_top + pad_bottom = 2: pads of 0 .. 2 are taken, and nothing else is same-size"""
    for pad in ((0, 2, 1, 1), (1, 1, 0, 2), (1, 1, 2, 0), (2, 0, 2, 0)):
        on, off = _both(w3.geom_of(16, 48, 0, 48, 32, 32, pad))
        assert (on["stage"], off["stage"]) == (w3.WGRAD3X3, w3.MFMA), (pad, on, off)
    on, off = _both(w3.geom_of(16, 48, 0, 48, 32, 32, (1, 1, 1, 0)))     # 32 x 31 outputs
    assert on == off and on["stage"] == w3.MFMA, (on, off)
