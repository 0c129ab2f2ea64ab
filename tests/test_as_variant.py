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
    assert GOLDEN["knobs"] == {"default": None, "deep2_maxm=0": [0, 3072, 1 << 30], "fwd_pf2_maxm=0": [1024, 3072, 0], "all_maxm=0": [0, 0, 0]}
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


# ---- launch counts (pmpc_as_sweep_launches) and what tests/test_as_variants_gpu.py builds on them ----------------------------------
CODES = {"bwd": 72, "fwd": 32}


def test_launch_count_codes_round_trip_every_variant():
    """The code layout of include/pmpc_abi.h gives every variant the selectors can return an index of its own, inside the table,
    and the fields come back out of it."""
    from pmpc_amd import _lib

    radix = {"bwd": (3, 2, 2, 3, 2), "fwd": (2, 2, 2, 2, 2)}
    for sweep in ("bwd", "fwd"):
        variants = [tuple(int(t) for t in v.split(",")) for v in GOLDEN["variants"][sweep]]
        codes = [_lib.as_sweep_code(sweep, v) for v in variants]
        assert len(set(codes)) == len(variants) and min(codes) >= 0 and max(codes) < CODES[sweep], (sweep, codes)
        for v, c in zip(variants, codes):
            back = []
            for r in radix[sweep]:
                back.append(c % r)
                c //= r
            assert tuple(back) == v and c == 0, (sweep, v)


def test_a_process_that_launched_nothing_reads_zero_counts_and_its_own_knobs():
    """Own process: in a run of the whole suite this one may have launched sweeps already, and the knobs are read once."""
    import os
    import subprocess
    import sys

    from tests.support.as_variants import KNOB_ENV

    prog = ("from pmpc_amd import _lib; b, f = _lib.as_sweep_launches('bwd'), _lib.as_sweep_launches('fwd', reset=True); "
            "print(len(b), len(f), sum(b), sum(f), *_lib.as_sweep_knobs())")
    root = str(Path(__file__).resolve().parents[1])
    for values, want in (((7, 11, 13), (7, 11, 13)), ((None, None, None), (1024, 3072, 1 << 30))):
        env = {k: v for k, v in os.environ.items() if k not in KNOB_ENV}
        env.update({k: str(v) for k, v in zip(KNOB_ENV, values) if v is not None})
        r = subprocess.run([sys.executable, "-c", prog], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert [int(t) for t in r.stdout.split()] == [CODES["bwd"], CODES["fwd"], 0, 0, *want], r.stdout
    from pmpc_amd import _lib

    assert _lib.load().pmpc_as_sweep_launches(2, None, 0, 0) == -1


def test_every_pair_of_the_gpu_test_is_a_compiled_pair():
    """tests/support/as_variants.py keeps PMPC_FAST_DIMS (pmpc_amd/csrc/fast_common.h) as a literal list."""
    from pmpc_amd import _lib
    from tests.support.as_variants import CONE_PAIRS, F32_PAIRS, PAIRS, XBOX_PAIRS

    assert len(PAIRS) == len(set(PAIRS)) == 25
    header = (Path(__file__).resolve().parents[1] / "pmpc_amd" / "csrc" / "fast_common.h").read_text()
    listed = header[header.index("#else", header.index("#define PMPC_FAST_DIMS(X) X(12, 4)")):]
    listed = listed[:listed.index("#endif")]
    assert [tuple(int(t) for t in m) for m in __import__("re").findall(r"X\((\d+), (\d+)\)", listed)] == PAIRS
    for x, u in PAIRS:
        _, compiled, (f32_ok, cone_ok, xbox_ok) = _lib.as_sweep_variant("bwd", x, u, 8, 1, 0)
        assert compiled
        assert f32_ok == ((x, u) in F32_PAIRS) and (cone_ok or (x, u) not in CONE_PAIRS) and (xbox_ok or (x, u) not in XBOX_PAIRS)


@pytest.mark.parametrize("setting,row", [("lean", "all_maxm=0"), ("deep", "deep2_maxm=0")])
def test_expected_set_of_the_gpu_test_agrees_with_the_recorded_table(setting, row):
    """The set of variants the GPU test requires to have been launched, computed from the library's selectors, is the set the recorded
    table gives for the same launches.  The table's grid has M = 1 where the cases have 6 .. 16 particles and Nc <= 2: under both
    settings these lie on the same side of every threshold (asserted), and Nc enters the selection only as Nc == 1."""
    from pmpc_amd import _lib
    from tests.support.as_variants import SETTINGS, expected_variants, family_cases

    knobs = SETTINGS[setting]
    assert GOLDEN["knobs"][row] == list(knobs)
    assert all((1 <= k) == (16 <= k) for k in knobs)
    grid = {key: n for n, key in enumerate(_grid())}

    def recorded(sweep, x, u, M, Nc, fl, kn):
        assert list(kn) == list(knobs) and 1 <= M <= 16
        cell = GOLDEN["cells"][sweep][row]["%d,%d" % (x, u)][grid[(fl, Nc if Nc in (0, 1) else 2, 1)]]
        if cell == "-":
            return (0,) * 5, False, None
        return tuple(int(t) for t in GOLDEN["variants"][sweep][string.ascii_letters.index(cell)].split(",")), True, None

    checked = 0
    for family in ("plain", "cone", "xbox", "f32", "ragged"):
        for (x, u), cases in family_cases(family):
            if [x, u] not in GOLDEN["pairs"]:
                continue
            want = expected_variants(family, knobs, x, u, cases)
            assert want == expected_variants(family, knobs, x, u, cases, select=recorded), (family, x, u)
            assert len({_lib.as_sweep_code(sw, v) for sw, v in want if sw == "bwd"}) == len([1 for sw, _ in want if sw == "bwd"])
            checked += 1
    assert checked >= 6
    from tests.support.as_variants import UNREACHED

    assert not [k for k in UNREACHED if k[0] == "plain"]  # the plain family's sweeps are all reached: nothing may be excused there
    # the plain family's expected set under each setting, spelled out: these are the variants the issue is about
    plain = expected_variants("plain", knobs, 12, 4, [dict(M=8, Nc=1)])
    if setting == "lean":
        assert plain == {("bwd", (0, 0, 0, 0, 0)), ("bwd", (1, 1, 0, 0, 0)), ("bwd", (1, 0, 1, 0, 0)), ("fwd", (0, 0, 0, 0, 0)), ("fwd", (1, 0, 0, 0, 0))}
    else:
        assert plain == {("bwd", (1, 0, 0, 0, 0)), ("bwd", (1, 1, 0, 0, 0)), ("bwd", (1, 0, 1, 0, 0)), ("fwd", (0, 1, 0, 0, 0)), ("fwd", (1, 1, 0, 0, 0))}
