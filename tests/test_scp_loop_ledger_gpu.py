"""The launch ledger of the library's SCP loop (tools/scp_loop_ledger.py) against tests/golden/scp_loop_ledger.json: per configuration —
compact / dense / fused linearisation, one step, a cost, a keep-out constraint, both, a runtime-compiled model, the cone objective, two
in-process ranks, a refused model — every recorded integer is the one the loop produced before it became `ScpLoop` (the fixture was
recorded at that commit, twice, in separate processes): iterations done, where the final iterate is, per-iteration status / rounds /
interior-point iterations, follow-ups taken as enqueued behind the rounds or enqueued again after the solve, and how many linearisation and
residual scopes ran.  What the tests of the iterates cannot see: a loop that linearises twice, or runs the separate residual where the
fused launch belonged, walks the same iterates."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = json.loads((ROOT / "tests" / "golden" / "scp_loop_ledger.json").read_text())
STARRED = ("boxes_nc1_cold", "boxes_nc3", "keepout")  # each the only cover of one case of ScpLoop::follow_up


@pytest.fixture(scope="module")
def ledger():
    spec = importlib.util.spec_from_file_location("scp_loop_ledger", ROOT / "tools" / "scp_loop_ledger.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_holds_every_configuration_or_says_why_not(ledger):
    dropped = [d["config"] for d in GOLDEN["dropped"]]
    assert sorted(list(GOLDEN["configs"]) + dropped) == sorted(ledger.CONFIGS)
    assert len(dropped) <= 2 and not set(dropped) & set(STARRED)


@pytest.mark.parametrize("name", sorted(GOLDEN["configs"]))
def test_loop_ledger_equals_the_recorded_one(ledger, name):
    got, digest = ledger.run_config(name)
    print(f"{name}: {json.dumps(got)} sha256(X, U, res) {digest}")
    assert got == GOLDEN["configs"][name]
    if name == "unknown_model":  # nothing ran
        assert got["done"] == 0 and got["status"] == [2] and got["linearize"] == 0 and got["scp_residual"] == 0
