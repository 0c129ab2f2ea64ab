"""The ledger of the cone objective's hard-box half (tools/cone_ledger.py) against tests/golden/cone_ledger.json: per configuration — four
tied problems through every `cone_path` twice on one context, one particle, particle weights on one and on two ranks, a worst-k case, fp32
storage, ties sharded over two and four in-process ranks, the log barrier and the one-particle squareplus dispatch — every integer of
`last_info` (status, fast_path, interior-point iterations, structured solves, outer solves, active-set rounds) is the one `lcone_body`
produced before it became `ConeSolve` (the fixture was recorded at that commit, twice, in separate processes).  What the tests of the
optima cannot see: a dispatch that takes the wrong body, or one weighted solve too many, reaches the same optimum."""
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
