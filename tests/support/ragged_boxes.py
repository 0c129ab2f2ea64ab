"""Control boxes that are NOT one number: per entry, one-sided, pinned (lo == hi), excluding zero — the generator, the conditions a case
must meet to tell a wrong kernel from a right one, and the case tables that tests/test_ragged_boxes.py certifies on the CPU (oracle
alone) before tests/test_ragged_boxes_gpu.py hands them to the device.

    python -m tests.support.ragged_boxes ipm_only      child of the interior-point-only test (PMPC_POLISH_MU=0, read once per process)

Semantics under test (limits): +-inf removes one side of one entry; lo == hi pins the entry; the consensus stages read
GLOBAL particle 0's box (PMPC.jl/src/lqp_utils.jl:329-330) whatever the other particles carry there."""
from __future__ import annotations

import functools
import sys

import numpy as np

from tests.support.problems import rand_problem

KINDS = ("per_entry", "one_sided", "upper_only", "pinned", "offset")
ON, FREE, BEYOND = 1e-9, 1e-6, 1e-3  # on a side / strictly free / detectably different


def ragged_boxes(rng, M, N, u, kind, b):
    """(lo, hi, parent_lo, parent_hi), all (M, N, u) float64.  per_entry: lo = -b U(0.5, 1.5), hi = b U(0.5, 1.5) drawn per particle, stage
    and control — the parent of one_sided (per entry one of: lower side removed, upper side removed, both kept), upper_only (all of lo at
    -inf: what backend.aff_solve builds from single-variable rows) and pinned (a quarter of the entries lo = hi = a point of the parent
    box).  offset: centre U(-1, 1), half-width U(0.05, 0.5) — its own parent.  mixed: one of the five per entry."""
    shape = (M, N, u)
    plo, phi = -b * rng.uniform(0.5, 1.5, shape), b * rng.uniform(0.5, 1.5, shape)
    if kind == "per_entry":
        return plo.copy(), phi.copy(), plo, phi
    if kind == "one_sided":
        side = rng.integers(0, 3, shape)
        return np.where(side == 0, -np.inf, plo), np.where(side == 1, np.inf, phi), plo, phi
    if kind == "upper_only":
        return np.full(shape, -np.inf), phi.copy(), plo, phi
    if kind in ("pinned", "pins_only"):
        pin = rng.random(shape) < 0.25
        v = plo + rng.random(shape) * (phi - plo)
        if kind == "pins_only":  # the pins are the only finite sides (the tie rule's case: every boxed entry has both sides active)
            return np.where(pin, v, -np.inf), np.where(pin, v, np.inf), plo, phi
        return np.where(pin, v, plo), np.where(pin, v, phi), plo, phi
    if kind == "offset":
        c, w = rng.uniform(-1.0, 1.0, shape), rng.uniform(0.05, 0.5, shape)
        return c - w, c + w, c - w, c + w
    if kind == "mixed":
        which = rng.integers(0, len(KINDS), shape)
        lo, hi = np.empty(shape), np.empty(shape)
        for k, name in enumerate(KINDS):
            l, h, _, _ = ragged_boxes(rng, M, N, u, name, b)
            lo, hi = np.where(which == k, l, lo), np.where(which == k, h, hi)
        return lo, hi, plo, phi
    raise ValueError(kind)


def shared_stages(N, Nc):
    return N if Nc < 0 else min(Nc, N)


def effective_boxes(lo, hi, Nc):
    """The boxes the joint program sees: particle 0's written onto the consensus stages."""
    lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    k = shared_stages(lo.shape[1], Nc)
    lo[:, :k], hi[:, :k] = lo[:1, :k], hi[:1, :k]
    return lo, hi


def on_side_counts(U, lo, hi):
    """(entries on a finite lower side, on a finite upper side, strictly free) — pinned entries count on both sides."""
    on_lo, on_hi = np.isfinite(lo) & (U <= lo + ON), np.isfinite(hi) & (U >= hi - ON)
    free = (U > lo + FREE) & (U < hi - FREE)
    return int(on_lo.sum()), int(on_hi.sum()), int(free.sum())


def check_conditions(kind, Uo, lo, hi, parent, Nc, U_prev, U_parent=None, any_side=False):
    """Asserts that the case can tell a wrong kernel from a right one; `Uo` is the oracle's optimum under the caller's boxes (lo, hi),
    `parent` = (parent_lo, parent_hi), `U_parent` the oracle's optimum under the parent boxes (pinned only).  Everything but the consensus
    condition is evaluated on the effective boxes.  `any_side`: one entry on either side will do (the stage-cone cases: their cone keeps u_0 above
    -0.1 and the other controls within 0.5 u_0 + 0.05 of zero, so hardly any lower side can be reached).  Returns the counts, for the log."""
    M, N, _ = Uo.shape
    k = shared_stages(N, Nc)
    elo, ehi = effective_boxes(lo, hi, Nc)
    plo, phi = effective_boxes(*parent, Nc)
    assert np.all(Uo >= elo - 1e-8) and np.all(Uo <= ehi + 1e-8), "the oracle's optimum leaves the effective boxes"
    n_lo, n_hi, n_free = on_side_counts(Uo, elo, ehi)
    out = dict(on_lo=n_lo, on_hi=n_hi, free=n_free)
    if any_side:
        assert n_lo + n_hi > 0, ("no entry on a finite side", kind)
    else:
        if np.isfinite(elo).any():  # (upper_only has no finite lower side to sit on)
            assert n_lo > 0, ("no entry on a finite lower side", kind)
        assert n_hi > 0, ("no entry on a finite upper side", kind)
    assert n_free > 0, ("no strictly free entry", kind)
    if kind in ("one_sided", "upper_only"):
        out["beyond"] = int(np.sum((~np.isfinite(elo) & (Uo < plo - BEYOND)) | (~np.isfinite(ehi) & (Uo > phi + BEYOND))))
        assert out["beyond"] > 0, ("no entry beyond the side that was removed", kind)
    if kind == "pinned":
        pin = elo == ehi
        assert U_parent is not None
        out["pinned"], out["pin_moves"] = int(pin.sum()), int(np.sum(pin & (np.abs(U_parent - elo) > BEYOND)))
        assert out["pin_moves"] > 0, ("no pinned entry that the parent's optimum is away from", kind)
    if kind == "offset":
        out["excl_0"], out["excl_prev"] = int(np.sum((elo > 0) | (ehi < 0))), int(np.sum((elo > U_prev) | (ehi < U_prev)))
        assert out["excl_0"] > 0 and out["excl_prev"] > 0, ("no box that excludes 0 / U_prev", kind)
    if k and M > 1:
        out["cons"] = consensus_violations(Uo, lo, hi, Nc)[1:].sum()
        assert out["cons"] > 0, ("the shared optimum is inside every particle's own box on the consensus stages", kind)
    return out


def consensus_violations(Uo, lo, hi, Nc):
    """Per particle: entries of the consensus stages where the shared optimum is outside the particle's OWN box by more than 1e-3."""
    k = shared_stages(Uo.shape[1], Nc)
    return np.sum((Uo[:, :k] < lo[:, :k] - BEYOND) | (Uo[:, :k] > hi[:, :k] + BEYOND), axis=(1, 2))


# -------------------------------------------------------------------------------------------------------------------------------
# case tables.  A case is a tuple (path, M, N, x, u, Nc, kind, b, extra) with `extra` a hashable tuple of (key, value) pairs; its seed
# is derived from its place in the table unless RESEEDED names another: seeds whose draw missed a condition of check_conditions were
# replaced here, on the CPU (tests/test_ragged_boxes.py fails on a case that misses one; no case is skipped at run time).
# -------------------------------------------------------------------------------------------------------------------------------
B = 0.4
FOUR = ("per_entry", "one_sided", "upper_only", "offset")  # the kinds with an interior

# a. QP path through the C ABI: register-resident padded (5, 3), (12, 4) and unpadded, generic (13, 2), (9, 5); Nc in {0, 1, 2, N};
#    M = 1, N = 1 (Nc = 0: with the one stage shared only u entries are left), M = 65 (more than one wave, no multiple of 64)
QP_SHAPES = [(5, 9, 12, 4, 1), (5, 9, 12, 4, -1), (7, 12, 5, 3, 1), (3, 6, 3, 2, 0), (3, 6, 3, 2, 2), (4, 7, 13, 2, 1), (4, 6, 9, 5, 0),
             (4, 8, 4, 2, -1), (1, 6, 3, 2, 0), (6, 1, 4, 2, 0), (65, 5, 4, 2, 1)]
# b. interior-point path alone
IPM_SHAPES = [(5, 9, 12, 4, 1), (4, 7, 13, 2, 1), (4, 8, 4, 2, -1), (3, 6, 3, 2, 0)]
# c. slew, increment form
SLEW_SHAPES = [(3, 6, 3, 2, 2), (3, 6, 3, 2, -1), (3, 6, 3, 2, 0)]
# d. dense consensus system (two of DENSE_CONS of tests/test_parity_gpu.py, with their boxes' sizes)
DENSE_SHAPES = [(3, 17, 4, 2, -1, 0.3), (2, 27, 5, 3, -1, 0.4)]
# e. cone objective
CONE_SHAPES = [(4, 8, 3, 2, 2), (12, 6, 2, 1, -1), (25, 7, 12, 4, 3)]
# f. stage cone, g. state boxes with one-sided sides
SOC_SHAPES = [(4, 6, 4, 2, 0), (5, 8, 12, 4, 1)]
XBOX_SHAPES = [(6, 10, 4, 2, 1, 0.8), (4, 9, 6, 3, 2, 0.8)]  # (.., pull)
# h. sharded: M = 3 world
SHARD = [(world, Nc, kind) for world in (2, 3) for Nc in (1, -1) for kind in ("per_entry", "pinned")]


def _table():
    t = {}
    t["qp"] = [("qp", *s, kind, B, ()) for s in QP_SHAPES for kind in KINDS]
    t["ipm"] = [("qp", *s, kind, B, ()) for s in IPM_SHAPES for kind in FOUR]
    t["ipm_pinned"] = [("qp", *s, "pinned", B, ()) for s in IPM_SHAPES[:2]]
    t["slew"] = [("qp", *s, kind, B, (("slew", 0.5),) + ((("slew0", 0.3),) if s0 else ())) for s in SLEW_SHAPES for s0 in (False, True) for kind in KINDS]
    t["dense"] = [("qp", *s[:5], kind, s[5], ()) for s in DENSE_SHAPES for kind in ("per_entry", "pinned")]
    t["cone"] = [("cone", *s, kind, B, ()) for s in CONE_SHAPES for kind in KINDS]
    t["barrier"] = [("cone", *s, kind, B, (("alpha", 10.0),)) for s in CONE_SHAPES for kind in FOUR]
    t["soc"] = [("soc", *s, kind, B, ()) for s in SOC_SHAPES for kind in ("per_entry", "one_sided")]
    t["xbox"] = [("xbox", *s[:5], kind, B, (("pull", s[5]),)) for s in XBOX_SHAPES for kind in ("per_entry", "one_sided")]
    # the finish of the interior-point iteration on entries that have BOTH sides active (k_as_setup's tie rule): register-resident and generic
    t["tie"] = [("qp", *s, "pins_only", B, ()) for s in IPM_SHAPES[:2]]
    t["shard"] = [("qp", 3 * w, 8, 5, 3, Nc, kind, B, (("world", w),)) for w, Nc, kind in SHARD]
    t["shard_cone"] = [("cone", 6, 6, 4, 2, 1, "per_entry", B, (("world", 2),))]
    return t


TABLES = _table()
# (spelled out, so that a table added later moves no other table's draws)
_BASE = dict(qp=52000, ipm=53000, ipm_pinned=54000, slew=55000, dense=56000, cone=57000, barrier=58000, soc=59000, xbox=60000, shard=61000,
             shard_cone=62000, tie=63000)
assert set(_BASE) == set(TABLES)
RESEEDED = {('barrier', 4): 148004, ('barrier', 5): 138005, ('barrier', 9): 68009, ('barrier', 10): 138010, ('cone', 1): 67001,
            ('cone', 5): 97005, ('cone', 6): 617006, ('cone', 7): 77007, ('cone', 11): 77011, ('ipm', 2): 63002, ('ipm', 4): 83004,
            ('ipm', 5): 113005, ('ipm', 6): 113006, ('qp', 0): 62000, ('qp', 6): 62006, ('qp', 11): 62011, ('qp', 12): 72012,
            ('qp', 26): 112026, ('qp', 27): 102027, ('qp', 36): 62036, ('qp', 46): 62046, ('qp', 50): 392050, ('qp', 51): 482051,
            ('qp', 52): 1082052, ('shard', 4): 71004, ('slew', 0): 65000, ('slew', 6): 65006, ('slew', 10): 65010, ('slew', 11): 65011,
            ('slew', 16): 115016, ('slew', 17): 65017, ('soc', 0): 79000, ('soc', 1): 69001, ('soc', 2): 119002, ('soc', 3): 199003,
            ('xbox', 0): 70000, ('xbox', 1): 70001}
# (the three seeds far from their base are M = 65, Nc = 1: with 65 particles pulling, the shared control rarely leaves the narrowest own box)


def case_seed(table, case):
    i = TABLES[table].index(case)
    return RESEEDED.get((table, i), _BASE[table] + i)


def case_id(case):
    path, M, N, x, u, Nc, kind, b, extra = case
    return f"{path}-M{M}N{N}x{x}u{u}Nc{Nc}-{kind}" + "".join(f"-{k}{v}" for k, v in extra)


def soc_cone(u, b):
    """The stage cone of tests/support/as_variants.py::_soc with an interior point that is inside every per_entry / one_sided box:
    (0.1 b, 0, ..) — lo <= -0.5 b < 0.1 b < 0.5 b <= hi, and 0 <= 0.5 * 0.1 b + 0.05."""
    W = np.zeros((u - 1, u))
    W[np.arange(u - 1), np.arange(1, u)] = 1.0
    return dict(W=W, w0=np.zeros(u - 1), v=np.eye(u)[0] * 0.5, v0=0.05, u_interior=np.eye(u)[0] * 0.1 * b)


def build_problem(table, case, orc=None):
    """(args, kw, parent): the seeded problem of a case, boxes in kw["u_l"], kw["u_u"] (caller's, not effective)."""
    path, M, N, x, u, Nc, kind, b, extra = case
    ex = dict(extra)
    rng = np.random.default_rng(case_seed(table, case))
    args, kw = rand_problem(rng, M, N, x, u, None, None, ex.get("slew"), ex.get("slew0"))
    lo, hi, plo, phi = ragged_boxes(rng, M, N, u, kind, b)
    kw["u_l"], kw["u_u"] = lo, hi
    if path == "xbox":
        # the construction of tests/support/problems.py::xbox_problem (margin 0.02) with the ragged control boxes in both of its solves, so
        # that X_f stays feasible; then one side removed per state entry as in one_sided, which keeps it feasible
        if orc is None:
            from oracle import lqp_oracle as orc
        Xs, _ = orc.lqp_solve_py(*args, Nc=Nc, **kw)
        other = list(args)
        other[8] = rng.standard_normal((M, N, x))
        Xf, _ = orc.lqp_solve_py(*other, Nc=Nc, **kw)
        P = Xf + ex["pull"] * (Xs - Xf)
        side = rng.integers(0, 3, (M, N, x))
        kw["x_l"], kw["x_u"] = np.where(side == 0, -np.inf, np.minimum(Xf, P) - 0.02), np.where(side == 1, np.inf, np.maximum(Xf, P) + 0.02)
    return args, kw, (plo, phi)


def oracle_solve(orc, case, args, kw):
    """(Xo, Uo, info) by the oracle of the case's path; info carries the KKT certificate where the oracle returns one."""
    path, M, N, x, u, Nc, kind, b, extra = case
    ex = dict(extra)
    if path == "cone":
        return orc.lcone_solve_py(*args, Nc=Nc, return_info=True, smooth_alpha=ex.get("alpha", float("nan")), **kw)
    if path == "soc":
        c = soc_cone(u, b)
        X, U = orc.lsoc_solve_py(*args, Nc=Nc, reg_x=kw["reg_x"], reg_u=kw["reg_u"], u_l=kw["u_l"], u_u=kw["u_u"], soc_W=c["W"], soc_w0=c["w0"],
                                 soc_v=c["v"], soc_v0=c["v0"], u_interior=c["u_interior"])
        return X, U, {}
    return orc.lqp_solve_py(*args, Nc=Nc, return_info=True, **kw)


@functools.lru_cache(maxsize=None)
def reference(table, case):
    """The case's problem and the oracle's answer, computed once per process and shared (callers must not write into the arrays)."""
    from oracle import lqp_oracle as orc

    orc.build()
    args, kw, parent = build_problem(table, case, orc)
    Xo, Uo, info = oracle_solve(orc, case, args, kw)
    return dict(args=args, kw=kw, parent=parent, Xo=Xo, Uo=Uo, info=info)


def case_conditions(table, case, ref=None):
    """check_conditions on a case of the tables (+ the path's own: a cone active, a state row on a finite side, a shared control held by
    particle 0's box, a violating particle on a rank other than 0).  The barrier cases have no entry ON a side: they are checked on the hard
    problem of the same draw."""
    from oracle import lqp_oracle as orc

    path, M, N, x, u, Nc, kind, b, extra = case
    ex = dict(extra)
    ref = ref or reference(table, case)
    args, kw, parent = ref["args"], ref["kw"], ref["parent"]
    Uo, Xo = ref["Uo"], ref["Xo"]
    hard = case
    if "alpha" in ex:
        hard = case[:8] + (tuple(p for p in extra if p[0] != "alpha"),)
        Xo, Uo, _ = oracle_solve(orc, hard, args, kw)
    U_parent = None
    if kind in ("pinned", "pins_only"):
        _, U_parent, _ = oracle_solve(orc, hard, args, dict(kw, u_l=parent[0], u_u=parent[1]))
    out = check_conditions("pinned" if kind == "pins_only" else kind, Uo, kw["u_l"], kw["u_u"], parent, Nc, args[5], U_parent, any_side=path == "soc")
    if path == "soc":
        slack = 0.5 * Uo[..., 0] + 0.05 - np.linalg.norm(Uo[..., 1:], axis=-1)
        out["cones"] = int((slack < 1e-6).sum())
        assert slack.min() > -1e-7 and out["cones"] > 0, "no cone active"
    if path == "xbox":
        out["xrows"] = int(np.sum((np.isfinite(kw["x_l"]) & (Xo <= kw["x_l"] + ON)) | (np.isfinite(kw["x_u"]) & (Xo >= kw["x_u"] - ON))))
        assert out["xrows"] > 0, "no state row on a finite side"
    if table == "dense":
        k = shared_stages(N, Nc)
        out["held"] = int(np.sum((Uo[0, :k] <= kw["u_l"][0, :k] + ON) | (Uo[0, :k] >= kw["u_u"][0, :k] - ON)))
        assert out["held"] > 0, "particle 0's box holds no shared control"
    if "world" in ex:  # the violating particle must live on another rank than 0: that is what the broadcast of rank 0's boxes is for
        out["cons_off_rank0"] = int(consensus_violations(Uo, kw["u_l"], kw["u_u"], Nc)[M // ex["world"]:].sum())
        assert out["cons_off_rank0"] > 0, "no particle of another rank whose own box the shared optimum violates"
    return out


def rel(a, b, floor=1.0):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), floor))


def errors(X, U, Xo, Uo):
    """The relative measures of tests/test_parity_gpu.py."""
    return rel(X, Xo, 1e-300), rel(U, Uo, 1.0)


def assert_shared_exactly(U, N, Nc):
    k = shared_stages(N, Nc)
    if k and U.shape[0] > 1:
        assert np.all(U[:, :k] == U[0:1, :k]), "the shared controls differ between particles"


# -------------------------------------------------------------------------------------------------------------------------------
# i. one context, the kinds in sequence: the same problem under boxes that change from call to call, so that the statuses and
# multipliers a call stored per side meet a side that is gone, a box that became a point, no boxes at all, an empty box
# -------------------------------------------------------------------------------------------------------------------------------
SEQ = dict(M=4, N=8, x=4, u=2, Nc=2, b=0.4, seed=58000)
SEQ_STEPS = ("uniform", "one_sided", "pinned", "none", "offset", "empty", "per_entry", "static_1", "static_2", "particle_0_moved")


@functools.lru_cache(maxsize=None)
def sequence():
    """[dict(name, lo, hi, Xo, Uo)] + the problem: lo / hi None = no boxes; Xo None = no feasible point (NaN outputs expected).  The
    last three steps are section i's static_cons_bounds part: the per_entry boxes unchanged twice, then particle 0's box on consensus
    stage 0 moved so that it excludes the shared optimum of before."""
    from oracle import lqp_oracle as orc

    orc.build()
    M, N, x, u, Nc, b = (SEQ[k] for k in ("M", "N", "x", "u", "Nc", "b"))
    rng = np.random.default_rng(SEQ["seed"])
    args, kw = rand_problem(rng, M, N, x, u, b)
    base = dict(reg_x=kw["reg_x"], reg_u=kw["reg_u"])
    steps = []

    def add(name, lo, hi, feasible=True):
        boxes = {} if lo is None else dict(u_l=lo, u_u=hi)
        Xo, Uo = orc.lqp_solve_py(*args, Nc=Nc, **base, **boxes) if feasible else (None, None)
        steps.append(dict(name=name, lo=lo, hi=hi, Xo=Xo, Uo=Uo))
        return Uo

    U1 = add("uniform", kw["u_l"], kw["u_u"])
    lo, hi, _, _ = ragged_boxes(rng, M, N, u, "one_sided", b)
    held = np.argwhere(U1[:, Nc:] >= b - ON)  # a free-stage control the previous answer holds on its upper side: that side goes
    assert len(held), "the uniform step holds no free-stage control on its upper side"
    i, j, c = held[0]
    lo[i, Nc + j, c], hi[i, Nc + j, c] = -b, np.inf
    U2 = add("one_sided", lo, hi)
    assert U2[i, Nc + j, c] > b + BEYOND, "the control whose side was removed does not move beyond it"
    lo, hi, _, _ = ragged_boxes(rng, M, N, u, "pinned", b)
    add("pinned", lo, hi)
    add("none", None, None)
    lo, hi, _, _ = ragged_boxes(rng, M, N, u, "offset", b)
    add("offset", lo, hi)
    lo, hi, _, _ = ragged_boxes(rng, M, N, u, "per_entry", b)
    elo = lo.copy()
    elo[M - 1, N // 2, u - 1] = hi[M - 1, N // 2, u - 1] + 0.25
    add("empty", elo, hi, feasible=False)
    U7 = add("per_entry", lo, hi)
    add("static_1", lo, hi)
    add("static_2", lo, hi)
    lo2, hi2 = lo.copy(), hi.copy()
    hi2[0, 0] = U7[0, 0] - 0.05
    lo2[0, 0] = np.minimum(lo[0, 0], hi2[0, 0] - 0.2)
    U10 = add("particle_0_moved", lo2, hi2)
    assert np.abs(U10[0, 0] - U7[0, 0]).min() >= 0.05 - 1e-9
    for st in steps:  # every boxed step holds some control on a side and leaves some free
        if st["lo"] is not None and st["Uo"] is not None:
            n_lo, n_hi, n_free = on_side_counts(st["Uo"], *effective_boxes(st["lo"], st["hi"], Nc))
            assert n_lo + n_hi > 0 and n_free > 0, (st["name"], n_lo, n_hi, n_free)
            if st["name"] not in ("uniform",):
                assert consensus_violations(st["Uo"], st["lo"], st["hi"], Nc)[1:].sum() > 0, ("consensus condition", st["name"])
    assert tuple(st["name"] for st in steps) == SEQ_STEPS
    return args, base, steps


# -------------------------------------------------------------------------------------------------------------------------------
# child process of tests/test_ragged_boxes_gpu.py::test_interior_point_path_alone (PMPC_POLISH_MU=0: every active-set use is off)
# -------------------------------------------------------------------------------------------------------------------------------
IPM_OK = "RAGGED_IPM_ONLY_OK"


def _ipm_only_child():
    import os

    from pmpc_amd import backend
    from tests.support.problems import abi_args

    assert os.environ.get("PMPC_POLISH_MU") == "0"
    worst = 0.0
    for case in TABLES["ipm"]:
        ref = reference("ipm", case)
        N, Nc = case[2], case[5]
        for rep in range(2):  # the second call starts from the interior-point iterate of the first
            X, U = backend.lqp_solve(*abi_args(ref["args"], ref["kw"], Nc))
            e = max(errors(X, U, ref["Xo"], ref["Uo"]))
            worst = max(worst, e)
            print(case_id(case), rep, f"{e:.2e}", flush=True)
            assert e < 1e-7, (case, rep, e)
            assert_shared_exactly(U, N, Nc)
    print(f"worst error interior-point path alone: {worst:.3e}", flush=True)
    # a pinned entry has no interior.  What the library does there, established on the device: the iteration still closes in on the point
    # and its answer has the oracle's parity (5.9e-15 and 2.5e-15 on these two cases) — asserted, as is the next call on the same context.
    for case in TABLES["ipm_pinned"]:
        ref = reference("ipm_pinned", case)
        Nc = case[5]
        X, U = backend.lqp_solve(*abi_args(ref["args"], ref["kw"], Nc))
        e = max(errors(X, U, ref["Xo"], ref["Uo"]))
        print(case_id(case), f"{e:.2e}", flush=True)
        assert e < 1e-7, ("a pinned entry on the interior-point path alone", case, e)
        assert_shared_exactly(U, case[2], Nc)
        free = next(c for c in TABLES["ipm"] if c[1:6] == case[1:6] and c[6] == "per_entry")  # same shape: the same context
        r2 = reference("ipm", free)
        X, U = backend.lqp_solve(*abi_args(r2["args"], r2["kw"], free[5]))
        e = max(errors(X, U, r2["Xo"], r2["Uo"]))
        print("  next call on the same context", f"{e:.2e}", flush=True)
        assert e < 1e-7, ("the context did not recover", e)
    print(IPM_OK, flush=True)


if __name__ == "__main__":
    if sys.argv[1:] == ["ipm_only"]:
        _ipm_only_child()
    else:
        raise SystemExit("usage: python -m tests.support.ragged_boxes ipm_only")
