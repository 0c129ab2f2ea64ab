"""Every (xdim, udim) pair of the register-resident kernels through the equality solve and the interior-point iteration alone
(options polish_mu = 0 and xbox_as = 0: no active-set rounds), against the exact oracle — the kernels that answer whenever the rounds
do not (pmpc_amd/csrc/kernels_fast.hip: k_bwd_fast in its 16 instantiations per pair, k_fwd_fast, k_cond_fast_grouped; the consensus
reductions and dense solves of kernels_generic.hip behind them).  tests/support/ipm_dims.py holds the cases and the assertions; the
launch counts of pmpc_fast_launches say per pair that FACTOR ran with every (HXB, HUB), the vector-only sweep with every box, and
the grouped condensing kernel — so no case passes vacuously, and a heuristic that moves an instantiation out of reach fails here.

One child process per test function, one time limit, no retry; a child that ends by a signal, at its time limit or with a HIP error
fails the test and nothing else is started (tests/support/child.py)."""
import pytest

from tests.support.child import run_child
from tests.support.ipm_dims import OK_TOKEN

pytestmark = pytest.mark.gpu


def _child(family, timeout):
    run_child("tests.support.ipm_dims", [family], OK_TOKEN, timeout)


def test_every_pair_through_the_equality_and_interior_point_path_alone():
    """Per pair: (M, N, Nc) = (3, 1, 1), (3, 2, 0), (11, 6, 6), (9, 7, 1) under the box modes none / u / x / ux, a second (perturbed)
    solve for the u and ux modes of the last two shapes that must take the interior-point warm start (no equality phase in the counts), and the third shape again with cond_grouped = 0.
    Time limit 300 s: the oracle's share is 24 s on the CPU (python -m tests.support.ipm_dims small --dry), start-up, and
    400 device solves of at most 11 particles by 7 stages, milliseconds each — times a generous allowance for a slower or busier host."""
    _child("small", 300)


def test_every_pair_above_the_deep_threshold_as_tiled_copies():
    """Per pair: 441 copies of a 7-particle problem (N = 6, Nc = 6), M = 3087 > 3072 — every DEEP = false instantiation, 386 condensing
    workgroups with 7 live waves in the last, the reductions with 64 slices and their second stage; every copy against the oracle's answer
    for the 7, and the copies against each other.
    Time limit 300 s: the oracle's share is 3 s on the CPU (python -m tests.support.ipm_dims tiled --dry), start-up, and 100
    device solves whose largest array is 21 MB — times the same allowance."""
    _child("tiled", 300)
