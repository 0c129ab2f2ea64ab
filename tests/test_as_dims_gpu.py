"""Every (xdim, udim) pair of the active-set sweeps, at the smallest shapes that reach each body of the sweeps, against the exact
oracle: M = 3, N in {2, 9}, Nc in {1, 2}, a cold solve and a warm one under prev_is_last_solution between which controls are held
and released, with and without the SENS forward sweeps (tests/support/as_dims.py holds the cases and the assertions).  What a cut
of the sweeps' vector instructions can break shows here: the row masks of pairs with udim < 4, the padding selects of pairs with
xdim % 4 != 0, the MAIN body next to the general body, restarts at the checkpoint rungs 4 and 8.

One child process, one time limit, no retry; a child that ends by a signal, at its time limit or with a HIP error fails the test
and nothing else is started (tests/support/child.py)."""
import pytest

from tests.support.as_dims import OK_TOKEN
from tests.support.child import run_child

pytestmark = pytest.mark.gpu

# seconds: the oracle's share is 4 s on the CPU (python -m tests.support.as_dims --dry) + one more oracle solve per warm solve, start-up,
# and 400 device solves of 3 particles by <= 9 stages, milliseconds each — times a generous allowance for a slower or busier host
TIMEOUT = 300


def test_every_pair_cold_and_warm_matches_the_oracle():
    run_child("tests.support.as_dims", [], OK_TOKEN, TIMEOUT)
