"""Every (xdim, udim) pair of the register-resident kernels through the equality solve and the interior-point iteration ALONE
(pmpc_amd/csrc/kernels_fast.hip: k_bwd_fast / k_fwd_fast / k_cond_fast_grouped, and the consensus reductions and dense solves behind
them) — the child process of tests/test_ipm_dims_gpu.py, and what tests/test_ipm_dims.py runs in-process without a device.

    python -m tests.support.ipm_dims FAMILY            on the device (FAMILY: small | tiled)
    python -m tests.support.ipm_dims FAMILY --dry      no device: the oracle's answer stands in for the device's — checks the conditions
                                                       on the inputs and times the oracle's share
    python -m tests.support.ipm_dims FAMILY --search   no device: prints the family's seed table

Every context sets polish_mu = 0 (no active-set rounds at all: no cold start, no warm start, no finish of the interior-point
iteration) and xbox_as = 0 before its first solve, so these kernels answer alone — the active-set sweeps normally answer most of
these problems, and a wrong kernel here would hide behind them until the rounds hand over.

small: per pair the smallest shapes that reach each body (SMALL_CASES), box modes none / u / x / ux (control boxes of
rand_problem(bu = 0.25), state boxes of xbox_problem(pull = 0.7)); the u and ux modes of the last two shapes solve a second,
perturbed problem on the same context (_next_problem, step 0.03): the interior-point warm start from the remembered iterate, its
multipliers of the state boxes included — the second problem's state boxes are the first's widened by what the step can move a
rollout, so the remembered iterate fits them, and the launch counts must show that the second solve ran no equality phase.
tiled: the kernels above 3072 particles (DEEP = false, 386 condensing workgroups with a ragged last one, the reductions with their
second stage) — TILED_COPIES identical copies of a base problem of TILED_BASE particles: the objective is the sum of the copies', the
boxes are equal and the consensus bounds are particle 0's, so the optimum is the base problem's optimum in every copy, and the oracle
solves 7 particles where the device solves 3087.

Tolerances are the project's own: 1e-10 without boxes (one Newton step: tests/test_slew_gpu.py), 1e-7 behind interior-point
iterations on control boxes (tests/test_parity_gpu.py), 1e-6 where the interior-point iteration alone answers state boxes
(tests/test_xbox_gpu.py::test_state_box_rounds_can_be_switched_off_per_context)."""
from __future__ import annotations

import sys
import time

import numpy as np

from tests.support.as_variants import PAIRS, _next_problem, _rel
from tests.support.problems import rand_problem, xbox_problem

OK_TOKEN = "IPM_DIMS_OK"
MODES = ("none", "u", "x", "ux")
TOL = {"none": 1e-10, "u": 1e-7, "x": 1e-6, "ux": 1e-6}
BU, PULL, STEP = 0.25, 0.7, 0.03
# (M, N, Nc), modes, modes that solve a second problem.  (3, 1, 1): a single stage (no "one stage ahead" prefetch target), k_cons_small;
# (3, 2, 0): two stages, no consensus — the smallest horizon whose state boxes bind (with N = 1 and the one control shared no row does);
# (11, 6, 6): nc = 6 udim in {6, 12, 18, 24} — always the grouped condensing kernel, two workgroups of 8 + 3 live waves, tiles that
# straddle stages at udim 3, two tiles at udim 4, the lds / register-resident dense solve from udim 3; (9, 7, 1): one shared stage, odd M
SMALL_SHAPES = [((3, 1, 1), ("none", "u"), ()), ((3, 2, 0), ("none", "u", "ux"), ()), ((11, 6, 6), ("none", "u", "x", "ux"), ("u", "ux")),
                ((9, 7, 1), ("u", "x"), ("u",))]
SMALL_CASES = [(shape, mode, mode in twice) for shape, modes, twice in SMALL_SHAPES for mode in modes]
GROUPED_OFF = [((11, 6, 6), "none"), ((11, 6, 6), "u")]  # repeated with option cond_grouped = 0: k_cond_fast on this path
TILED_BASE, TILED_COPIES, TILED_N, TILED_NC = 7, 441, 6, 6  # M = 3087 > 3072: DEEP = false
TILED_CASES = [((TILED_BASE, TILED_N, TILED_NC), mode, False) for mode in MODES]
FAMILIES = {"small": (SMALL_CASES, 41000), "tiled": (TILED_CASES, 95000)}
# seed of case (pair k, case j) = base + 2000 k + 100 j + SEEDS[family][k][j]: the first offset at which the oracle answers every solve
# of the case with its certificate and the conditions on the inputs hold (python -m tests.support.ipm_dims FAMILY --search)
SEEDS = {}  # filled below
SEARCH_RANGE, SEARCH_SECONDS = 100, 3  # (offsets tried per case; seconds after which the search gives a seed up)
# (the sweep instantiations a pair must have launched: FACTOR with every (HXB, HUB), the vector-only corrector sweep with every box)
WANT_SWEEPS = [(1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (0, 0, 1), (0, 1, 0), (0, 1, 1)]  # (factor, hxb, hub)


def _seed(family, k, j):
    return FAMILIES[family][1] + 2000 * k + 100 * j + SEEDS[family][k][j]


def conditions(mode, Nc, Xo, Uo, kw):
    """What of the oracle's optimum sits on its boxes, and whether the case tests what it is there for: u modes — a control on its box,
    one free and (Nc >= 1) a shared control on its bound; x modes — a state entry on its box."""
    note, ok = [], True
    if "u" in mode:
        on = (Uo <= kw["u_l"] + 1e-9) | (Uo >= kw["u_u"] - 1e-9)
        shared = int(np.sum(on[0, :Nc])) if Nc > 0 else None
        note.append(f"ubox {int(on.sum())} of {on.size}" + (f" shared {shared}" if Nc > 0 else ""))
        # (udim 1 with the one stage shared is ONE control for all particles: it is held, and there is no other to be free)
        one_control = Nc > 0 and Uo[0, :Nc].size == Uo[0].size == 1
        ok = ok and 0 < on.sum() and (on.sum() < on.size or one_control) and (Nc <= 0 or shared > 0)
    if "x" in mode:
        rows = int(np.sum((Xo <= kw["x_l"] + 1e-9) | (Xo >= kw["x_u"] - 1e-9)))
        note.append(f"xrows {rows}")
        ok = ok and rows > 0
    return ok, " ".join(note)


def _rollout(args, U):
    """States the controls U roll out to: x_j = f_j + fx_j (x_{j-1} - X_prev_{j-1}) + fu_j (u_j - U_prev_j), no fx term at stage 0."""
    x0, f, fx, fu, X_prev, U_prev = args[:6]
    X = np.empty_like(f)
    for j in range(f.shape[1]):
        X[:, j] = f[:, j] + np.einsum("mrt,mt->mr", fu[:, j], U[:, j] - U_prev[:, j])
        if j:
            X[:, j] += np.einsum("mrt,mt->mr", fx[:, j], X[:, j - 1] - X_prev[:, j - 1])
    return X


def _rollout_shift_bound(args0, args1, u_l, u_u):
    """Per state entry, a bound on |rollout under args1 - rollout under args0| over all controls inside [u_l, u_u]: the shift is
    affine in a particle's controls, s(U) = s(mid) + L (U - mid), so |s| <= |s(mid)| + sum_k |L_k| half_k."""
    mid, half = 0.5 * (u_l + u_u), 0.5 * (u_u - u_l)
    shift = lambda U: _rollout(args1, U) - _rollout(args0, U)
    s0 = shift(mid)
    bound = np.abs(s0)
    for j in range(mid.shape[1]):
        for b in range(mid.shape[2]):
            U = mid.copy()
            U[:, j, b] += 1.0
            bound += np.abs(shift(U) - s0) * half[:, j, b][:, None, None]
    return bound


def case_solves(orc, x, u, shape, mode, twice, seed):
    """[(args, kw, (Xo, Uo), ok, note)] of the one or two solves of a case; the second problem does not depend on the first answer."""
    M, N, Nc = shape
    rng = np.random.default_rng(seed)
    bu = BU if "u" in mode else None
    if "x" in mode:
        args, kw = xbox_problem(rng, orc, M, N, x, u, Nc, bu, pull=PULL)
    else:
        args, kw = rand_problem(rng, M, N, x, u, bu)
    out = []
    for t in range(2 if twice else 1):
        if t:
            args = _next_problem("plain", rng, args, t, None, None, step=STEP)
            if "x" in mode:
                # The first problem's state boxes are empty for dynamics moved by 3 % (the oracle diverges on every seed tried at
                # (11, 6, 6)), so the second problem's are the first's, widened entry by entry by the most the step can move the state
                # that ANY controls inside the control boxes roll out to (_rollout_shift_bound).  The iterate the context remembers lies
                # strictly inside the first boxes, so it lies inside these under the new dynamics: the warm start must take it.
                w = _rollout_shift_bound(first_args, args, kw["u_l"], kw["u_u"])
                kw = dict(kw, x_l=kw["x_l"] - w, x_u=kw["x_u"] + w)
        first_args = args
        Xo, Uo = orc.lqp_solve_py(*args, Nc=Nc, **kw)
        assert np.all(np.isfinite(Xo)) and np.all(np.isfinite(Uo)), (x, u, shape, mode, seed, t)
        out.append((args, kw, (Xo, Uo)) + conditions(mode, Nc, Xo, Uo, kw))
    return out


def search(orc, family, first_pair=0):
    """The seed table: a seed whose oracle solve fails its own certificate (or finds the perturbed problem's boxes empty) is skipped
    HERE — the tests run the table's seeds and catch nothing."""
    import signal

    def too_long(*_):  # (an oracle that grinds on a perturbed problem whose boxes are empty: not a seed for a quick test)
        raise TimeoutError

    signal.signal(signal.SIGALRM, too_long)
    cases, base = FAMILIES[family]
    rows = []
    for k, (x, u) in enumerate(PAIRS):
        if k < first_pair:
            continue
        row = []
        for j, (shape, mode, twice) in enumerate(cases):
            for off in range(SEARCH_RANGE):
                signal.alarm(SEARCH_SECONDS)
                try:
                    solves = case_solves(orc, x, u, shape, mode, twice, base + 2000 * k + 100 * j + off)
                except (AssertionError, FloatingPointError, RuntimeError, TimeoutError, np.linalg.LinAlgError):
                    continue
                finally:
                    signal.alarm(0)
                if all(s[3] for s in solves):
                    break
            else:
                raise SystemExit(f"no seed for {(x, u, shape, mode)}")
            row.append(off)
        rows.append(row)
        print(f"    {row},  # {(x, u)}", flush=True)
    return rows


def _tile(a, copies):
    return np.tile(a, (copies,) + (1,) * (a.ndim - 1))


def _check(s, x, u, shape, mode, t, args, kw, Xo, Uo, copies=1, label=""):
    """One device solve against the oracle's answer (of the base problem, tiled `copies` times for the device); returns the worst error."""
    from tests.test_slew_gpu import _solve

    M, N, Nc = shape
    if copies > 1:
        args = tuple(_tile(a, copies) for a in args)
        kw = {key: (_tile(v, copies) if isinstance(v, np.ndarray) else v) for key, v in kw.items()}
    X, U, status, info = _solve(s, args, kw, Nc)
    tol = TOL[mode]
    where = (x, u, shape, mode, t, label, info)
    if copies == 1:
        ex, eu, spread = _rel(X, Xo), _rel(U, Uo), 0.0
    else:  # every copy against the base answer, and the copies of one base particle against each other
        Xc, Uc = X.reshape(copies, -1), U.reshape(copies, -1)
        nx, nu = max(np.linalg.norm(Xo), 1.0), max(np.linalg.norm(Uo), 1.0)
        ex = float(np.max(np.linalg.norm(Xc - Xo.reshape(1, -1), axis=1)) / nx)
        eu = float(np.max(np.linalg.norm(Uc - Uo.reshape(1, -1), axis=1)) / nu)
        spread = max(float(np.linalg.norm(Xc.max(0) - Xc.min(0)) / nx), float(np.linalg.norm(Uc.max(0) - Uc.min(0)) / nu))
    print(f"  {mode:4s} {label}t{t} status {status} fast_path {info['fast_path']} ipm {info['ipm_iters']} rounds {info['active_set_rounds']} "
          f"errX {ex:.2e} errU {eu:.2e}" + (f" spread {spread:.2e}" if copies > 1 else "") + f" tol {tol:.0e}", flush=True)
    assert status == 0 and info["fast_path"] == 1 and info["active_set_rounds"] == 0, where
    assert (info["ipm_iters"] == 0) if mode == "none" else (info["ipm_iters"] > 0), where
    assert ex <= tol and eu <= tol and spread <= tol, ("parity", ex, eu, spread, tol) + where
    if Nc != 0:  # the shared controls are one value, bitwise
        assert np.all(U[:, :Nc] == U[0:1, :Nc]), where
    if "x" in mode:
        assert np.all(X >= kw["x_l"] - 1e-8) and np.all(X <= kw["x_u"] + 1e-8), where
    return max(ex, eu, spread)


def _context(**options):
    from pmpc_amd.device import DeviceSolver

    s = DeviceSolver(0)
    for key, val in dict(polish_mu=0, xbox_as=0, **options).items():
        s.set_option(key, val)
    return s


def run(family, dry):
    from oracle import lqp_oracle as orc

    if not dry:
        from pmpc_amd import _lib
    cases, _ = FAMILIES[family]
    copies = TILED_COPIES if family == "tiled" else 1
    worst, t0, t_orc = {m: 0.0 for m in MODES}, time.time(), 0.0
    for k, (x, u) in enumerate(PAIRS):
        if not dry:
            for kind in _lib.FAST_LAUNCH_KINDS:
                _lib.fast_launches(kind, reset=True)
        ungrouped = 0
        for j, (shape, mode, twice) in enumerate(cases):
            tc = time.time()
            solves = case_solves(orc, x, u, shape, mode, twice, _seed(family, k, j))
            t_orc += time.time() - tc
            print(f"case ({x}, {u}) {shape} {mode} seed {_seed(family, k, j)}: " + "; ".join(s[4] for s in solves), flush=True)
            assert all(s[3] for s in solves), ("the oracle's optimum does not meet the conditions on the inputs", x, u, shape, mode, [s[4] for s in solves])
            if dry:
                continue
            s = _context()
            eq_code = _lib.fast_sweep_code(1, 0, 0, family == "small")  # the factor sweep of the equality-only solve
            for t, (args, kw, (Xo, Uo), _, _) in enumerate(solves):
                eq_before = _lib.fast_launches("sweep")[eq_code]
                worst[mode] = max(worst[mode], _check(s, x, u, shape, mode, t, args, kw, Xo, Uo, copies))
                eq_sweeps = _lib.fast_launches("sweep")[eq_code] - eq_before
                # a second solve starts from the remembered iterate (controls and multipliers, the state boxes' included): no equality
                # phase — a rejected or failed warm attempt would run one (run_box_dispatch); a first solve runs exactly one
                assert eq_sweeps == (0 if t else 1), ("warm start from the remembered iterate not taken" if t else "equality phase", x, u, shape, mode, t, eq_sweeps)
                if t:
                    print(f"       t{t} warm: no equality phase", flush=True)
            s.close()
            if family == "small" and (shape, mode) in GROUPED_OFF:
                before = _lib.fast_launches("cond")
                s = _context(cond_grouped=0)
                args, kw, (Xo, Uo), _, _ = solves[0]
                worst[mode] = max(worst[mode], _check(s, x, u, shape, mode, 0, args, kw, Xo, Uo, label="cond_grouped=0 "))
                s.close()
                after = _lib.fast_launches("cond")
                assert after[0] > before[0] and after[1] == before[1], ("cond_grouped = 0 did not run k_cond_fast alone", x, u, shape, mode, before, after)
                ungrouped += after[0] - before[0]
        if dry:
            continue
        # the instantiations the cases are there for were launched for this pair
        sweeps, cond, cons = (_lib.fast_launches(kind) for kind in ("sweep", "cond", "cons"))
        deep = family == "small"  # launch_bwd_t: DEEP up to 3072 particles
        print(f"pair ({x}, {u}) launches (code: count): sweep {dict((c, n) for c, n in enumerate(sweeps) if n)} cond {cond} "
              f"cons {dict((c, n) for c, n in enumerate(cons) if n)}", flush=True)
        missing = [v for v in WANT_SWEEPS if sweeps[_lib.fast_sweep_code(*v, deep)] == 0]
        assert not missing, ("sweep instantiations (factor, hxb, hub) never launched", x, u, deep, missing, sweeps)
        assert not any(sweeps[_lib.fast_sweep_code(f, xb, ub, not deep)] for f in (0, 1) for xb in (0, 1) for ub in (0, 1)), ("DEEP on the wrong side of its threshold", x, u, sweeps)
        assert cond[1] > 0 and (family == "tiled" or ungrouped > 0), ("condensing kernels", x, u, cond, ungrouped)
        if family == "tiled":
            assert cond[0] == 0, ("k_cond_fast answered a solve the grouped kernel is there for", x, u, cond)
    print("worst error " + " ".join(f"{m} {worst[m]:.3e}" for m in MODES) + f"; oracle {t_orc:.1f} s of {time.time() - t0:.1f} s", flush=True)


SEEDS["small"] = [
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 0],  # (12, 4)
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0],  # (12, 3)
    [0, 10, 0, 0, 0, 0, 0, 0, 0, 0, 0],  # (12, 2)
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0],  # (10, 4)
    [0, 1, 0, 0, 0, 0, 0, 0, 0, 2, 0],  # (10, 2)
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0],  # (9, 4)
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],  # (9, 3)
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0],  # (8, 4)
    [0, 5, 0, 0, 0, 0, 0, 0, 1, 2, 0],  # (8, 2)
    [0, 1, 0, 0, 0, 0, 0, 0, 0, 3, 0],  # (7, 3)
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0],  # (6, 4)
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],  # (6, 3)
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 0],  # (6, 2)
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0],  # (5, 3)
    [0, 1, 0, 0, 0, 0, 0, 0, 0, 2, 0],  # (5, 2)
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],  # (4, 4)
    [0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0],  # (4, 3)
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0],  # (4, 2)
    [0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0],  # (4, 1)
    [0, 1, 0, 0, 0, 0, 0, 0, 0, 2, 0],  # (3, 3)
    [0, 2, 0, 0, 0, 0, 0, 0, 0, 1, 0],  # (3, 2)
    [0, 7, 0, 0, 0, 0, 0, 0, 0, 1, 0],  # (3, 1)
    [0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0],  # (2, 2)
    [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0],  # (2, 1)
    [0, 2, 0, 0, 0, 0, 0, 0, 0, 3, 0],  # (1, 1)
]
SEEDS["tiled"] = [[0, 0, 0, 0]] * 23 + [
    [0, 0, 0, 1],  # (2, 1)
    [0, 0, 0, 0],  # (1, 1)
]


def main(argv):
    family = argv[1]
    if "--search" in argv[2:]:
        from oracle import lqp_oracle as orc

        print(f'SEEDS["{family}"] = [')
        SEEDS[family] = search(orc, family, int(argv[3]) if len(argv) > 3 else 0)  # (a pair number to start at)
        print("]")
        return
    run(family, "--dry" in argv[2:])
    print(OK_TOKEN, flush=True)


if __name__ == "__main__":
    main(sys.argv)
