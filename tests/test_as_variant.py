"""Which instantiation of the active-set sweeps a launch takes (pmpc_amd/csrc/as_variant.h) against a table recorded from the launchers
as they stood before the selection had a place of its own (tests/golden/as_sweep_variants.json), and: whatever the solver can ask for
is compiled.  No GPU: the selection is read from the built library on the host."""
import json
import string
from pathlib import Path

import pytest

GOLDEN = json.loads((Path(__file__).parent / "golden" / "as_sweep_variants.json").read_text())
BIT = {name: 1 << k for k, name in enumerate(GOLDEN["flag_bits"])}


def _grid():
    for fl in range(1 << len(GOLDEN["flag_bits"])):
        for Nc in GOLDEN["Nc"]:
            for M in GOLDEN["M"]:
                yield fl, Nc, M


def _solver_can_ask(fl, dims):
    """solver_qp.hip sets mat32 / cone_H and as_uraw / xb_D only behind f32_ / cone_ / xbox_as_dims_supported."""
    f32_ok, cone_ok, xbox_ok = dims
    return (f32_ok or not fl & BIT["mat32"]) and (cone_ok or not fl & (BIT["cone_H"] | BIT["as_uraw"])) and (xbox_ok or not fl & BIT["xb_D"])


def test_the_table_covers_the_grid_it_claims():
    from pmpc_amd import _lib

    assert tuple(GOLDEN["flag_bits"]) == _lib.AS_SWEEP_FLAGS
    assert GOLDEN["Nc"] == [0, 1, 2] and GOLDEN["M"] == [1, 1024, 1025, 3072, 3073, 4096]
    assert GOLDEN["pairs"] == [[12, 4], [4, 2], [4, 1], [1, 1]]
    assert GOLDEN["knobs"] == {"default": None, "deep2_maxm=0": [0, 3072, 1 << 30], "fwd_pf2_maxm=0": [1024, 3072, 0]}
    n = sum(1 for _ in _grid())
    for sweep in ("bwd", "fwd"):
        for knobs in GOLDEN["knobs"]:
            assert all(len(GOLDEN["cells"][sweep][knobs]["%d,%d" % tuple(p)]) == n for p in GOLDEN["pairs"])


@pytest.mark.parametrize("knobs", list(GOLDEN["knobs"]))
@pytest.mark.parametrize("x,u", [tuple(p) for p in GOLDEN["pairs"]])
@pytest.mark.parametrize("sweep", ["bwd", "fwd"])
def test_selection_is_the_recorded_one_and_what_the_solver_can_ask_for_is_compiled(sweep, x, u, knobs):
    from pmpc_amd import _lib

    variants = [tuple(int(t) for t in v.split(",")) for v in GOLDEN["variants"][sweep]]
    cells = GOLDEN["cells"][sweep][knobs]["%d,%d" % (x, u)]
    wrong, missing, extra = [], [], []
    for cell, (fl, Nc, M) in zip(cells, _grid()):
        got, compiled, dims = _lib.as_sweep_variant(sweep, x, u, M, Nc, fl, GOLDEN["knobs"][knobs])
        recorded = None if cell == "-" else variants[string.ascii_letters.index(cell)]
        if recorded is None:  # the old launcher had no such instantiation and refused: there is none now either
            if compiled:
                extra.append((fl, Nc, M, got))
        elif got != recorded or not compiled:
            wrong.append((fl, Nc, M, got, compiled, recorded))
        if _solver_can_ask(fl, dims) and not compiled:
            missing.append((fl, Nc, M, got))
    assert not wrong, wrong[:5]
    assert not extra, extra[:5]
    assert not missing, missing[:5]


def test_pairs_without_cone_and_fp32_kernels():
    from pmpc_amd import _lib

    dims = {(x, u): _lib.as_sweep_variant("bwd", x, u, 1, 1, 0)[2] for x, u in [(12, 4), (4, 2), (4, 1), (1, 1)]}
    assert dims == {(12, 4): (True, True, True), (4, 2): (True, True, True), (4, 1): (False, False, True), (1, 1): (False, False, True)}
    with pytest.raises(ValueError):
        _lib.as_sweep_variant("bwd", 11, 4, 1, 1, 0)
