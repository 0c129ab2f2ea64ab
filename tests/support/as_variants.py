"""Every selectable instantiation of the active-set sweeps (pmpc_amd/csrc/kernels_as.hip: k_bwd_as / k_fwd_as) at small shapes
against the exact oracles — the child process of tests/test_as_variants_gpu.py, and what that test and tests/test_as_variant.py
share with it (pairs, knob settings, cases, the expected set of variants).

    python -m tests.support.as_variants FAMILY          with PMPC_AS_DEEP2_MAXM / PMPC_AS_DEEP_MAXM / PMPC_AS_FWD_PF2_MAXM set
    python -m tests.support.as_variants FAMILY --dry    no device: the oracle's answer stands in for the device's — checks the
                                                        conditions on the inputs and times the oracle's share of the child

The three knobs are read once per process, so each setting is a process of its own.  A child prints one line per case, one per
(pair) with the launched and the expected variants, the worst error of the family and, last, OK_TOKEN."""
from __future__ import annotations

import os
import sys
import time

import numpy as np

from tests.support.problems import rand_problem, xbox_problem

OK_TOKEN = "AS_VARIANTS_OK"
KNOB_ENV = ("PMPC_AS_DEEP2_MAXM", "PMPC_AS_DEEP_MAXM", "PMPC_AS_FWD_PF2_MAXM")
# (deep2_maxm, deep_maxm, fwd_pf2_maxm); "deep" leaves the last two at the library's defaults
SETTINGS = {"lean": (0, 0, 0), "deep": (0, 3072, 1 << 30)}
CHILDREN = [("plain", "lean"), ("plain", "deep"), ("cone", "lean"), ("xbox", "lean"), ("f32", "lean"), ("ragged", "lean"), ("ragged", "deep")]

# PMPC_FAST_DIMS of pmpc_amd/csrc/fast_common.h (tests/test_as_variant.py asserts that the library accepts each pair)
PAIRS = [(12, 4), (12, 3), (12, 2), (10, 4), (10, 2), (9, 4), (9, 3), (8, 4), (8, 2), (7, 3), (6, 4), (6, 3), (6, 2), (5, 3),
         (5, 2), (4, 4), (4, 3), (4, 2), (4, 1), (3, 3), (3, 2), (3, 1), (2, 2), (2, 1), (1, 1)]
F32_PAIRS = [(12, 4), (6, 3), (4, 2)]  # as_f32_dims of as_variant.h
CONE_PAIRS = [(12, 4), (4, 2), (5, 3), (3, 3), (6, 2)]
XBOX_PAIRS = [(12, 4), (4, 2), (6, 3), (2, 1), (9, 3), (8, 4)]

# the family's own bits of `flags` (pmpc_amd/_lib.py: AS_SWEEP_FLAGS) next to defect (1) and as_settled_in (2); as_T stays off: the
# sensitivity records start at as_sens_min_m particles, far above these
FAMILY_FLAGS = {"plain": [0], "cone": [8 | 32], "xbox": [16], "f32": [4, 4 | 8 | 32], "ragged": [0]}

# Variants of the expected set that no input of these sizes reaches, by name: (family, setting, pair, sweep, variant) -> reason.
# Must stay empty for the plain family's full sweeps (MODE 0, MODE 1 with and without DEFECT, both forward rings).
UNREACHED = {
    ("f32", "lean", (12, 4), "bwd", (1, 0, 0, 1, 1)):
        "fp32 storage + cone, MODE 1 without DEFECT and without SKIP: the fp32 rounds only start from a DEFECT sweep and their later rounds are "
        "SKIP sweeps unless option as_skip is 0; with as_skip = 0 the cones' rounds of (12, 4) did not settle within their limit on any input tried "
        "(M = 5, N = 6, steps of 0.005; the fp64 rounds of the same context neither), so the widened fp64 solve answers and the "
        "parity check says nothing about this instantiation; the case marked probe= fails if that ever changes.  On (4, 2) the same case "
        "settles and the variant is reached; its fp64 twin (1, 0, 0, 1, 0) and its box twin (1, 0, 0, 0, 1) are reached on every pair.",
}

# Solves of the plain family that interior-point iterations answer, by name: (pair, seed of the case, solve) -> reason.  Every other
# solve of the family must be finished by the rounds alone (ipm_iters == 0, active_set_rounds >= 1), cold ones included: a sweep
# that is wrong in a way that keeps the active set from settling would otherwise hide behind the interior-point path's answer.
NEEDS_IPM = {
    ((12, 4), 31002, 3): "warm rounds at their limit of 8 (9 counted) with 266 of 360 controls on their boxes; the same under lean and deep",
    ((6, 4), 31102, 2): "warm rounds at their limit, then the finish of the interior-point iteration (15 rounds in all); the same under lean and deep",
}

# The same for the ragged family (boxes of tests/support/ragged_boxes.py: every instantiation reads lo / hi in its own code).  More than
# 5 % of the family's 300 solves here would be a finding of its own, to be reported and not written down.
NEEDS_IPM_RAGGED = {
    ((10, 4), 35030, 2): "offset boxes, 421 of 540 controls on a side: warm rounds at their limit, then 12 interior-point iterations; the same under lean and deep",
    ((10, 4), 35030, 3): "the same case one step on (423 on a side): 26 interior-point iterations, 7 rounds",
    ((8, 4), 35071, 3): "all nine stages shared under +-0.02 boxes, 245 of 252 on a side: warm rounds at their limit (10 counted with the finish)",
    ((6, 4), 35100, 3): "pinned boxes, 537 sides held among 504 controls (a pinned entry counts on both): warm rounds at their limit, finish of the interior-point iteration",
    ((6, 3), 35110, 2): "offset boxes, 128 of 162 on a side: warm rounds at their limit, 9 interior-point iterations",
    ((4, 4), 35150, 0): "offset boxes, 215 of 252 on a side: the cold rounds hand over (10 interior-point iterations, 6 rounds)",
    ((4, 4), 35150, 2): "the same case, warm: 13 interior-point iterations, 7 rounds",
    ((4, 4), 35150, 3): "the same case, warm: 12 interior-point iterations, 6 rounds",
    ((4, 3), 35160, 2): "per-entry boxes, 200 of 270 on a side: warm rounds at their limit (15 counted), 9 interior-point iterations",
}  # 9 of 300 solves (3 %), the same nine under both settings
RAGGED_KINDS = ("per_entry", "one_sided", "pinned", "offset")


def plain_cases(k):
    """(M, N, Nc) of pair number k: every Nc of {0, 1, 3, N}, N in {1, 2, 9} and one of {3, 5} — N = 1: no MAIN stage, 2: jmin on the
    first trip, 3 and 5: first checkpoint at stage 4 not reached / reached with one restart rung, 9: two rungs.  Even and odd k both
    hold padded (x = 5, 6, 7, 9, 10) and unpadded pairs, so each N meets both."""
    shapes = [(1, 0), (2, 2), (9, 1), (9, 3), (3, 0)] if k % 2 == 0 else [(1, 1), (2, 0), (9, 9), (9, 3), (5, 1)]
    return [(6 + (3 * k + 2 * c) % 11, N, Nc) for c, (N, Nc) in enumerate(shapes)]


def family_cases(family):
    """[(pair, [case, ..])]: case = dict(M, N, Nc, seed, + what the family adds)."""
    out = []
    if family == "plain":
        for k, (x, u) in enumerate(PAIRS):
            out.append(((x, u), [dict(M=M, N=N, Nc=Nc, seed=31000 + 10 * k + c, bu=0.02 if Nc == N else 0.25) for c, (M, N, Nc) in enumerate(plain_cases(k))]))
    elif family == "ragged":
        # three of the plain family's shape classes per pair — N = 9 with one shared stage, N = 9 with three or all shared, N = 2 without —
        # with M as in plain_cases; the kind of box rotates with pair + case, so that every kind meets every shape class
        for k, (x, u) in enumerate(PAIRS):
            shapes = [(9, 1), (9, 3 if k % 2 == 0 else 9), (2, 0)]
            out.append(((x, u), [dict(M=6 + (3 * k + 2 * c) % 11, N=N, Nc=Nc, seed=35000 + 10 * k + c, bu=0.02 if Nc == N else 0.25, kind=RAGGED_KINDS[(k + c) % 4])
                                 for c, (N, Nc) in enumerate(shapes)]))
    elif family == "cone":  # sized like SOC_CASES of tests/test_cone_gpu.py
        for k, (x, u) in enumerate(CONE_PAIRS):
            shapes = [(4, 6, 0), (5, 8, 1), (6, 5, 2), (4, 6, 6)]
            out.append(((x, u), [dict(M=M, N=N, Nc=Nc, seed=32000 + 10 * k + c, bu=0.3 if Nc == N else 0.6, cone=True) for c, (M, N, Nc) in enumerate(shapes)]))
    elif family == "xbox":  # sized like XBOX_CASES of tests/test_xbox_gpu.py
        for k, (x, u) in enumerate(XBOX_PAIRS):
            # (the boxes are built around trajectories of THESE dynamics: keep_map, and f disturbed by a hundredth of the boxes' margin, so
            #  that they stay feasible.  One stage: Nc = 0 — with the one control shared, the two trajectories the boxes are built from coincide and no row binds;
            #  short horizons get tighter control boxes, so that one still binds)
            shapes = [(6, 1, 0, 0.4), (3, 2, (0, 1, 2)[k % 3], 0.6), (5, 10, (1, 10, 2, 0)[k % 4], 0.8), (6, 9, 1, 0.9)]
            out.append(((x, u), [dict(M=M, N=N, Nc=Nc, seed=33005 + 10 * k + c, bu={1: 0.2, 2: 0.1}.get(N, 0.4), pull=pull, margin=0.05, step=0.0005, scp_from=1, keep_map=True)
                                 for c, (M, N, Nc, pull) in enumerate(shapes)]))
    elif family == "f32":
        # fp32 storage runs the rounds with Nc <= 1 only (solver_qp.hip), and only from a warm start under prev_is_last_solution, whose
        # first round is a DEFECT sweep and whose later ones are SKIP sweeps: option as_skip = 0 makes them full sweeps without DEFECT.
        # Rounds that do not settle end in a widened fp64 solve (fast_path 1): the cone cases move as an SCP loop near its fixed point
        # does (keep_map, steps of 0.005), where the cones' Newton rounds do settle
        for k, (x, u) in enumerate(F32_PAIRS):
            cs = [dict(M=7, N=9, Nc=1, seed=34000 + 10 * k, bu=0.25), dict(M=6, N=2, Nc=0, seed=34001 + 10 * k, bu=0.25),
                  dict(M=8, N=5, Nc=1, seed=34002 + 10 * k, bu=0.25, options={"as_skip": 0})]
            if u >= 4 or (x, u) == (4, 2):
                cs += [dict(M=5, N=8, Nc=1, seed=34003 + 10 * k, bu=0.6, cone=True, step=0.005, scp_from=1, keep_map=True),
                       dict(M=4, N=6, Nc=0, seed=34004 + 10 * k, bu=0.6, cone=True, step=0.005, scp_from=1, keep_map=True),
                       dict(M=5, N=6, Nc=1, seed=34005 + 10 * k, bu=0.6, cone=True, step=0.005, scp_from=1, keep_map=True, options={"as_skip": 0})]
                if (x, u) == (12, 4):  # probe of the UNREACHED entry: were these rounds to settle on the float arrays, the entry would be stale
                    cs[-1]["probe"] = ("bwd", (1, 0, 0, 1, 1))
            out.append(((x, u), cs))
    else:
        raise ValueError(family)
    return out


def case_flags(family, case):
    if family == "f32":
        return [4 | 8 | 32] if case.get("cone") else [4]
    return FAMILY_FLAGS[family]


def expected_variants(family, knobs, x, u, cases, select=None):
    """{(sweep, variant)}: what the selectors return for the pair's (M, Nc), defect and as_settled_in on and off, the family's flags."""
    if select is None:
        from pmpc_amd import _lib

        select = _lib.as_sweep_variant
    want = set()
    for case in cases:
        for fam in case_flags(family, case):
            for fl in range(4):
                for sweep in ("bwd", "fwd"):
                    v, compiled, _ = select(sweep, x, u, case["M"], case["Nc"], fl | fam, list(knobs))
                    assert compiled, (sweep, x, u, case, fl | fam, v)
                    want.add((sweep, tuple(v)))
    return want


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1.0)


def _soc(u):
    """The stage cone of tests/test_cone_gpu.py::test_stage_cones_match_cone_oracle: || (u_1, ..) || <= 0.5 u_0 + 0.05."""
    W = np.zeros((u - 1, u))
    W[np.arange(u - 1), np.arange(1, u)] = 1.0
    return dict(W=W, w0=np.zeros(u - 1), v=np.eye(u)[0] * 0.5, v0=0.05, u_int=np.eye(u)[0] * 0.2)


def _round32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _oracle(orc, family, case, args, kw, u):
    if case.get("cone"):
        c = _soc(u)
        return orc.lsoc_solve_py(*args, Nc=case["Nc"], reg_x=kw["reg_x"], reg_u=kw["reg_u"], u_l=kw["u_l"], u_u=kw["u_u"], soc_W=c["W"],
                                 soc_w0=c["w0"], soc_v=c["v"], soc_v0=c["v0"], u_interior=c["u_int"])
    return orc.lqp_solve_py(*args, Nc=case["Nc"], **kw)


def _device(s, family, case, args, kw, u, promise):
    import torch

    f32 = family == "f32"
    dev = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    md = torch.float32 if f32 else torch.float64
    T = lambda a: dev(np.swapaxes(a, -1, -2), md)
    x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref = args
    opt = dict(f=dev(f), fx=T(fx), fu=T(fu), X_prev=dev(X_prev), U_prev=dev(U_prev), Q=T(Q), R=T(R), X_ref=dev(X_ref), U_ref=dev(U_ref),
               reg_x=kw["reg_x"], reg_u=kw["reg_u"], Nc=case["Nc"], symmetric_cost=True, lu=dev(kw["u_l"]), uu=dev(kw["u_u"]),
               prev_is_last_solution=promise)
    if "x_l" in kw:
        opt.update(lx=dev(kw["x_l"]), ux=dev(kw["x_u"]))
    if case.get("cone"):
        c = _soc(u)
        X, U, status = s.lsoc_solve(soc_W=dev(c["W"]), soc_w0=dev(c["w0"]), soc_v=dev(c["v"]), soc_v0=c["v0"], soc_u_interior=dev(c["u_int"]), **opt)
    else:
        X, U, status = s.lqp_solve(**opt)
    s.sync()
    return X.cpu().numpy(), U.cpu().numpy(), status, dict(s.last_info)


def _next_problem(family, rng, args, t, Xl, Ul, step=0.03, scp_from=2, keep_map=False):
    """Problem of solve t = 1, 2, 3 from the one before: a perturbed problem, from t = scp_from on linearised about the last outputs
    (from t = 2 on the solves carry the promise prev_is_last_solution, so scp_from <= 2; with scp_from = 1 the step that moves X_prev and
    U_prev from random points onto a solution, which moves the optimum a long way, is taken by the solve WITHOUT the promise).
    step: size of the change (0.03 relative: tests/test_device_gpu.py::test_scp_like_sequence_without_rollout).
    keep_map: the affine dynamics stay what they are — f is moved to the new linearisation point and disturbed by step, fx and fu stay —,
    so only the proximal terms move from solve to solve and the sequence settles like an SCP loop near its fixed point."""
    relin = t >= scp_from
    x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref = args
    if keep_map:
        if relin:
            f = f + np.einsum("mnrt,mnt->mnr", fu, Ul - U_prev)
            f[:, 1:] += np.einsum("mnrt,mnt->mnr", fx[:, 1:], Xl[:, :-1] - X_prev[:, :-1])
            X_prev, U_prev = Xl, Ul
        f = f + step * rng.standard_normal(f.shape)
    else:
        f = f + step * rng.standard_normal(f.shape)
        fx = fx * (1 + step * rng.standard_normal(fx.shape))
        fu = fu * (1 + step * rng.standard_normal(fu.shape))
        if relin:
            X_prev, U_prev = Xl, Ul
        else:
            X_prev, U_prev = X_prev + step * rng.standard_normal(X_prev.shape), U_prev + step * rng.standard_normal(U_prev.shape)
    if family == "f32":
        fx, fu = _round32(fx), _round32(fu)
    return (x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref)


def case_tolerance(family, case, info):
    """The project's own values: 1e-9 for a solve of the active-set rounds alone (tests/test_device_gpu.py), 1e-7 behind interior-point
    iterations; the module TOL of tests/test_cone_gpu.py (1e-6) and tests/test_xbox_gpu.py (1e-7); 1e-6 for fp32 storage."""
    if family == "f32" or case.get("cone"):
        return 1e-6
    if family == "xbox":
        return 1e-7
    return 1e-9 if info["ipm_iters"] == 0 else 1e-7


def run_case(orc, family, x, u, case, dry):
    """The four solves of one context; returns (worst error, most rounds of a solve, DEFECT solves the rounds alone finished,
    [line per solve])."""
    rng = np.random.default_rng(case["seed"])
    M, N, Nc = case["M"], case["N"], case["Nc"]
    if family == "xbox":
        args, kw = xbox_problem(rng, orc, M, N, x, u, Nc, case["bu"], pull=case["pull"], margin=case.get("margin", 0.02))
    elif family == "ragged":
        from tests.support.ragged_boxes import ragged_boxes

        args, kw = rand_problem(rng, M, N, x, u, None)
        kw["u_l"], kw["u_u"] = ragged_boxes(rng, M, N, u, case["kind"], case["bu"])[:2]
    else:
        args, kw = rand_problem(rng, M, N, x, u, case["bu"])
    if family == "f32":  # the oracle solves the float-rounded data widened to double: the problem the device solves
        args = tuple(_round32(a) if k in (2, 3, 6, 7) else a for k, a in enumerate(args))
    s = None
    if not dry:
        from pmpc_amd.device import DeviceSolver

        s = DeviceSolver(0)
        for key, val in case.get("options", {}).items():
            s.set_option(key, val)
    worst, rounds, by_defect, lines = 0.0, 0, 0, []
    Xl = Ul = None
    for t in range(4):
        if t:
            args = _next_problem(family, rng, args, t, Xl, Ul, case.get("step", 0.03), case.get("scp_from", 2), case.get("keep_map", False))
        Xo, Uo = _oracle(orc, family, case, args, kw, u)
        # conditions on the inputs (a test must not pass vacuously): a control on its box; a cone active; a state row binding
        assert np.all(np.isfinite(Xo)) and np.all(np.isfinite(Uo)), (family, x, u, case, t)
        if family == "ragged":  # on a FINITE side of the boxes the joint program sees (particle 0's on the consensus stages)
            from tests.support.ragged_boxes import effective_boxes, on_side_counts

            on_box = sum(on_side_counts(Uo, *effective_boxes(kw["u_l"], kw["u_u"], Nc))[:2])
        else:
            on_box = int(np.sum((Uo <= kw["u_l"] + 1e-9) | (Uo >= kw["u_u"] - 1e-9)))
        assert on_box > 0, ("no control on its box", family, x, u, case, t)
        note = f"ubox {on_box}"
        if case.get("cone"):
            slack = 0.5 * Uo[..., 0] + 0.05 - np.linalg.norm(Uo[..., 1:], axis=-1)
            assert slack.min() > -1e-7 and (slack < 1e-6).sum() > 0, ("no cone active", family, x, u, case, t, slack.min())
            note += f" cones {(slack < 1e-6).sum()}"
        if family == "xbox":
            rows = int(np.sum((Xo <= kw["x_l"] + 1e-9) | (Xo >= kw["x_u"] - 1e-9)))
            assert rows > 0, ("no state row binds", family, x, u, case, t)
            note += f" xrows {rows}"
        if dry:
            Xl, Ul = Xo, Uo
            lines.append(f"  t{t} {note}")
            continue
        X, U, status, info = _device(s, family, case, args, kw, u, promise=t >= 2)
        ex, eu = _rel(X, Xo), _rel(U, Uo)
        tol = case_tolerance(family, case, info)
        lines.append(f"  t{t} {note} status {status} fast_path {info['fast_path']} ipm {info['ipm_iters']} rounds {info['active_set_rounds']} "
                     f"errX {ex:.2e} errU {eu:.2e} tol {tol:.0e}")
        print(lines[-1], flush=True)
        assert status == 0, (family, x, u, case, t, info)
        assert ex < tol and eu < tol, ("parity", family, x, u, case, t, ex, eu, tol, info)
        if case.get("probe"):
            assert ("f32", "lean", (x, u)) + case["probe"] in UNREACHED
            assert not (t >= 2 and info["fast_path"] == 2 and info["ipm_iters"] == 0 and info["active_set_rounds"] >= 2), (
                "the rounds of this case settled: its variant is reached after all — drop the UNREACHED entry and the probe mark", x, u, case, t, info)
        elif family == "f32" and t >= 2:  # the warm solves of an SCP loop: the rounds read the float arrays
            assert info["fast_path"] == 2 and info["ipm_iters"] == 0 and info["active_set_rounds"] >= 1, (family, x, u, case, t, info)
        else:
            assert info["fast_path"] == 1, (family, x, u, case, t, info)
        if family in ("plain", "ragged") and ((x, u), case["seed"], t) not in (NEEDS_IPM if family == "plain" else NEEDS_IPM_RAGGED):
            assert info["ipm_iters"] == 0 and info["active_set_rounds"] >= 1, ("not finished by the rounds alone", family, x, u, case, t, info)
        if t >= 2 and info["ipm_iters"] == 0 and info["active_set_rounds"] >= 1:
            by_defect += 1
        worst, rounds = max(worst, ex, eu), max(rounds, info["active_set_rounds"])
        Xl, Ul = X, U
    if s is not None:
        s.close()
    return worst, rounds, by_defect, lines


def run_family(family, setting, dry=False, pairs=None):
    from oracle import lqp_oracle as orc

    knobs = SETTINGS[setting]
    if not dry:
        from pmpc_amd import _lib

        got = _lib.as_sweep_knobs()
        print(f"family {family} setting {setting} knobs {got}", flush=True)
        assert tuple(got) == tuple(knobs), (got, knobs)
        assert tuple(int(os.environ[k]) for k in KNOB_ENV) == tuple(knobs)
    worst_family, t0 = 0.0, time.time()
    for (x, u), cases in family_cases(family):
        if pairs is not None and (x, u) not in pairs:
            continue
        if not dry:
            _lib.as_sweep_launches("bwd", reset=True)
            _lib.as_sweep_launches("fwd", reset=True)
        most_rounds = by_defect = 0
        for case in cases:
            print(f"case {family} {setting} ({x}, {u}) {case}", flush=True)
            tc = time.time()
            worst, rounds, nd, lines = run_case(orc, family, x, u, case, dry)
            if dry:
                print("\n".join(lines) + f"\n  oracle {time.time() - tc:.2f} s", flush=True)
            worst_family, most_rounds, by_defect = max(worst_family, worst), max(most_rounds, rounds), by_defect + nd
        if dry:
            continue
        # SKIP sweeps have work in later rounds only, and a launch behind the round that ended the solve returns at once
        assert most_rounds >= 2, ("no solve of the pair went to a second round", family, setting, x, u)
        # a warm start whose rounds do not settle hands over to the interior-point iteration (same answer, to its tolerance): the DEFECT
        # sweeps must have produced the accepted answer of some solve
        assert by_defect >= 1, ("no solve under prev_is_last_solution was finished by the rounds alone", family, setting, x, u)
        want = expected_variants(family, knobs, x, u, cases)
        launched = {(sw, v) for sw, v in want if _lib.as_sweep_launches(sw)[_lib.as_sweep_code(sw, v)] > 0}
        counts = {sw: {c: n for c, n in enumerate(_lib.as_sweep_launches(sw)) if n} for sw in ("bwd", "fwd")}
        excused = {(sw, v) for (fam, st, pair, sw, v) in UNREACHED if (fam, st, pair) == (family, setting, (x, u))}
        print(f"pair ({x}, {u}) rounds {most_rounds} by_defect {by_defect} expected {sorted(want)} launched(code: count) {counts}", flush=True)
        missing = want - launched - excused
        assert not missing, ("expected variants never launched", family, setting, x, u, sorted(missing))
    print(f"worst error {family} {setting}: {worst_family:.3e}; {time.time() - t0:.1f} s", flush=True)
    return worst_family


def main(argv):
    family = argv[1]
    dry = "--dry" in argv[2:]
    if dry:
        setting = "lean"
    else:
        env = tuple(int(os.environ[k]) for k in KNOB_ENV)
        setting = {v: k for k, v in SETTINGS.items()}[env]
    run_family(family, setting, dry)
    print(OK_TOKEN, flush=True)


if __name__ == "__main__":
    main(sys.argv)
