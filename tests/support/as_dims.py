"""Every (xdim, udim) pair of the active-set sweeps through the bodies a cut of their vector instructions can break — the child
process of tests/test_as_dims_gpu.py.

    python -m tests.support.as_dims            on the device
    python -m tests.support.as_dims --dry      no device: the oracle's answer stands in for the device's — checks the conditions
                                               on the inputs and times the oracle's share
    python -m tests.support.as_dims --search   no device: prints a SEEDS table whose cases meet the conditions

Per pair of PMPC_FAST_DIMS: M = 3, N in {2, 9}, Nc in {1, 2}, control boxes tight enough that between two consecutive solves some
controls stay held and some are released.  N = 2 is the smallest horizon that reaches "only the general body", N = 9 the smallest
that reaches the MAIN body with the checkpoint rungs 4 and 8 and a remainder in the three-stage ring.  The first solve is cold, the
second warm under prev_is_last_solution (DEFECT sweeps, SKIP sweeps of the later rounds restarted at a rung, the stage-0 and consensus
bodies); the pair of solves runs twice, the second time with option as_sens_min_m = 1 (the SENS forward sweeps, which the default
starts at 3072 particles).  Pairs with udim < 4 and xdim % 4 != 0 are where row masks and padding selects can go wrong.
Tolerance, oracle and helpers are those of the plain family of tests/support/as_variants.py."""
from __future__ import annotations

import sys
import time

import numpy as np

from tests.support.as_variants import PAIRS, _device, _next_problem, _oracle, _rel, case_tolerance
from tests.support.problems import rand_problem

OK_TOKEN = "AS_DIMS_OK"
M = 3
SHAPES = [(2, 1), (2, 2), (9, 1), (9, 2)]  # (N, Nc)
BU = 0.25  # half-width of the control boxes (the plain family's)
# seed of case (pair k, shape c) = 36000 + 4000 k + 1000 c + SEEDS[k][c]: the first offset at which the oracle's two answers hold some
# controls on their boxes in both solves and release some between them (python -m tests.support.as_dims --search)
SEEDS = None  # filled below


def _seed(k, c):
    return 36000 + 4000 * k + 1000 * c + SEEDS[k][c]


def _on_box(U, kw):
    return (U <= kw["u_l"] + 1e-9) | (U >= kw["u_u"] - 1e-9)


def case_problems(orc, x, u, N, Nc, seed):
    """The two problems of a case from the ORACLE's trajectory (the second is linearised about the first one's answer, as an SCP loop
    would), the oracle's answers, and (held in both, released between them)."""
    rng = np.random.default_rng(seed)
    case = dict(M=M, N=N, Nc=Nc)
    args0, kw = rand_problem(rng, M, N, x, u, BU)
    X0, U0 = _oracle(orc, "plain", case, args0, kw, u)
    args1 = _next_problem("plain", rng, args0, 2, X0, U0)
    X1, U1 = _oracle(orc, "plain", case, args1, kw, u)
    b0, b1 = _on_box(U0, kw), _on_box(U1, kw)
    return (args0, args1), kw, ((X0, U0), (X1, U1)), (int(np.sum(b0 & b1)), int(np.sum(b0 & ~b1)))


def search(orc):
    rows = []
    for k, (x, u) in enumerate(PAIRS):
        row = []
        for c, (N, Nc) in enumerate(SHAPES):
            for off in range(400):
                held, released = case_problems(orc, x, u, N, Nc, 36000 + 4000 * k + 1000 * c + off)[3]
                if held > 0 and released > 0:
                    break
            else:
                raise SystemExit(f"no seed for {(x, u, N, Nc)}")
            row.append(off)
        rows.append(row)
        print(f"    {row},  # {(x, u)}", flush=True)
    return rows


def run(dry):
    from oracle import lqp_oracle as orc

    if not dry:
        from pmpc_amd import _lib
        from pmpc_amd.device import DeviceSolver
    worst, t0, t_orc = 0.0, time.time(), 0.0
    for k, (x, u) in enumerate(PAIRS):
        if not dry:
            _lib.as_sweep_launches("bwd", reset=True)
            _lib.as_sweep_launches("fwd", reset=True)
        for c, (N, Nc) in enumerate(SHAPES):
            case = dict(M=M, N=N, Nc=Nc, seed=_seed(k, c))
            tc = time.time()
            problems, kw, answers, (held, released) = case_problems(orc, x, u, N, Nc, case["seed"])
            t_orc += time.time() - tc
            assert all(np.all(np.isfinite(a)) for XU in answers for a in XU), (x, u, case)
            assert held > 0 and released > 0, ("the boxes do not hold and release controls between the two solves", x, u, case, held, released)
            print(f"case ({x}, {u}) {case} held {held} released {released}", flush=True)
            if dry:
                continue
            for sens in (False, True):
                s = DeviceSolver(0)
                if sens:
                    s.set_option("as_sens_min_m", 1)
                for t, (args, (Xo, Uo)) in enumerate(zip(problems, answers)):
                    if t == 1:  # the promise holds for the DEVICE's last answer: linearise about it (it is the oracle's to the tolerance)
                        args = tuple(Xl if i == 4 else (Ul if i == 5 else a) for i, a in enumerate(args))
                        tc = time.time()
                        Xo, Uo = _oracle(orc, "plain", case, args, kw, u)
                        t_orc += time.time() - tc
                    X, U, status, info = _device(s, "plain", case, args, kw, u, promise=t == 1)
                    ex, eu = _rel(X, Xo), _rel(U, Uo)
                    tol = case_tolerance("plain", case, info)
                    print(f"  sens {int(sens)} t{t} status {status} fast_path {info['fast_path']} ipm {info['ipm_iters']} rounds {info['active_set_rounds']} "
                          f"errX {ex:.2e} errU {eu:.2e} tol {tol:.0e}", flush=True)
                    assert status == 0, (x, u, case, sens, t, info)
                    assert ex < tol and eu < tol, ("parity", x, u, case, sens, t, ex, eu, tol, info)
                    worst = max(worst, ex, eu)
                    Xl, Ul = X, U
                s.close()
        if dry:
            continue
        # the instantiations the cases are there for were launched for this pair: DEFECT and SKIP factor sweeps, DEFECT and SENS forward sweeps
        bwd, fwd = _lib.as_sweep_launches("bwd"), _lib.as_sweep_launches("fwd")
        n_defect = sum(n for code, n in enumerate(bwd) if (code // 6) % 2)
        n_skip = sum(n for code, n in enumerate(bwd) if (code // 3) % 2)
        n_fdefect = sum(n for code, n in enumerate(fwd) if code % 2)
        n_sens = sum(n for code, n in enumerate(fwd) if code // 16)
        print(f"pair ({x}, {u}) launches: factor DEFECT {n_defect} SKIP {n_skip}; forward DEFECT {n_fdefect} SENS {n_sens}", flush=True)
        assert n_defect > 0 and n_skip > 0 and n_fdefect > 0 and n_sens > 0, (x, u, bwd, fwd)
    print(f"worst error {worst:.3e}; oracle {t_orc:.1f} s of {time.time() - t0:.1f} s", flush=True)


SEEDS = [
    [0, 0, 0, 0],  # (12, 4)
    [0, 5, 0, 0],  # (12, 3)
    [0, 3, 0, 0],  # (12, 2)
    [1, 2, 0, 0],  # (10, 4)
    [0, 0, 0, 0],  # (10, 2)
    [0, 2, 0, 0],  # (9, 4)
    [0, 0, 0, 0],  # (9, 3)
    [0, 0, 0, 0],  # (8, 4)
    [0, 1, 0, 0],  # (8, 2)
    [0, 0, 0, 0],  # (7, 3)
    [0, 1, 0, 0],  # (6, 4)
    [0, 2, 0, 0],  # (6, 3)
    [0, 4, 0, 0],  # (6, 2)
    [0, 1, 0, 0],  # (5, 3)
    [0, 4, 0, 0],  # (5, 2)
    [0, 2, 0, 0],  # (4, 4)
    [0, 4, 0, 0],  # (4, 3)
    [0, 1, 0, 0],  # (4, 2)
    [0, 45, 0, 0],  # (4, 1)
    [0, 1, 0, 0],  # (3, 3)
    [2, 5, 0, 0],  # (3, 2)
    [4, 8, 0, 0],  # (3, 1)
    [3, 1, 0, 0],  # (2, 2)
    [2, 16, 0, 0],  # (2, 1)
    [5, 3, 0, 0],  # (1, 1)
]


def main(argv):
    global SEEDS
    if "--search" in argv[1:]:
        from oracle import lqp_oracle as orc

        print("SEEDS = [")
        SEEDS = search(orc)
        print("]")
        return
    run("--dry" in argv[1:])
    print(OK_TOKEN, flush=True)


if __name__ == "__main__":
    main(sys.argv)
