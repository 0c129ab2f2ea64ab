"""The ledger of the cone objective (tools/cone_ledger.py) against tests/golden/cone_ledger.json.  Per configuration every integer of
`last_info` (status, fast_path, interior-point iterations, structured solves, outer solves, active-set rounds) is the one the code produced
BEFORE its bodies became per-solve objects; each part of the fixture was recorded at the commit before that change, twice, in separate
processes.  What the tests of the optima cannot see: a dispatch that takes the wrong body, or one solve or Newton step too many, reaches
the same optimum.

Hard boxes (`lcone_body` before `ConeSolve`): four tied problems through every `cone_path` twice on one context, one particle, particle
weights on one and on two ranks, a worst-k case, fp32 storage, ties sharded over two and four in-process ranks, the log barrier and the
one-particle squareplus dispatch.

Smoothed boxes (`lcone_smooth_body` before `SmoothSolve`), one configuration per branch of the Newton iteration: two solves on one context
(warm start and remembered multipliers; `cone_rank_memory` 0; `cold_start`), consensus horizons with the Newton system on the device (Nc 2),
on the host (Nc = N) and without a shared control (Nc 0), barrier weights 1 and 100 (damped steps, width changes), squareplus (seven
particles, ties, one particle with and without a weight), the log barrier declined (weights, slew), phase 1 reached and ending with status 0,
phase 1 failing, and the sharded gathers (two and four ranks at Nc 1, two ranks at Nc 2, two ranks at Nc = N: the host system's table;
squareplus on two ranks)."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = json.loads((ROOT / "tests" / "golden" / "cone_ledger.json").read_text())


@pytest.fixture(scope="module")
def ledger():
    spec = importlib.util.spec_from_file_location("cone_ledger", ROOT / "tools" / "cone_ledger.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_holds_every_configuration_and_every_integer(ledger):
    assert sorted(GOLDEN["configs"]) == sorted(ledger.CONFIGS)
    assert GOLDEN["dropped"] == []  # (an integer that differed between the two recordings would be named here and left out of the fixture)


@pytest.mark.parametrize("name", sorted(GOLDEN["configs"]))
def test_cone_ledger_equals_the_recorded_one(ledger, name):
    got, digest = ledger.run_config(name)
    print(f"{name}: {json.dumps(got)} sha256(X, U) {digest}")
    assert got == GOLDEN["configs"][name]
