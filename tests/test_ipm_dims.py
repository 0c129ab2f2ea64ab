"""The inputs of tests/test_ipm_dims_gpu.py without a device: the seed tables of tests/support/ipm_dims.py still give problems the
oracle answers with its certificate and whose optimum meets the conditions the GPU tests rely on (a control on its box and one free,
a shared control on its bound, a state entry on its box) — a table gone stale after a change of a generator shows here.
Cost: about 27 s of the CPU suite (24 s small, 3 s tiled) — the oracle solves every case of every pair, 12-state problems included."""
import pytest

from tests.support import ipm_dims
from tests.support.as_variants import PAIRS


@pytest.mark.parametrize("family", ["small", "tiled"])
def test_seed_tables_meet_the_conditions_on_every_pair(family, capsys):
    cases, _ = ipm_dims.FAMILIES[family]
    assert len(ipm_dims.SEEDS[family]) == len(PAIRS) and all(len(row) == len(cases) for row in ipm_dims.SEEDS[family])
    ipm_dims.run(family, dry=True)  # asserts the conditions case by case
    out = capsys.readouterr().out
    assert out.count("case (") == len(PAIRS) * len(cases) and "worst error" in out


def test_cases_cover_what_they_are_there_for():
    shapes = {shape: (modes, twice) for shape, modes, twice in ipm_dims.SMALL_SHAPES}
    assert set(shapes) == {(3, 1, 1), (3, 2, 0), (11, 6, 6), (9, 7, 1)}
    assert all(set(twice) <= set(modes) for modes, twice in shapes.values())
    # every sweep instantiation the GPU test asserts has a case that asks for it: boxes u, x and both
    assert {"none", "u", "x", "ux"} == {mode for _, mode, _ in ipm_dims.SMALL_CASES} == {mode for _, mode, _ in ipm_dims.TILED_CASES}
    M = ipm_dims.TILED_BASE * ipm_dims.TILED_COPIES
    assert M == 3087 > 3 * 1024  # (launch_bwd_t: DEEP up to 3072 particles)
    assert (M + 7) // 8 == 386 and M % 8 == 7 and (M + 3) // 4 > 64  # condensing groups, live waves of the last, reduction slices capped
