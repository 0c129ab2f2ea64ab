"""The ledger of the cone objective (`ConeSolve` and its bodies, csrc/solver_cone.hip; the smoothed boxes' `SmoothSolve`,
csrc/solver_cone_smooth.hip): which body answered a call and how many solves it took, as integers, on the smallest shape an existing test
uses per dispatch — and, for the smoothed half, per branch of its Newton iteration: warm and cold second solves, remembered multipliers,
consensus horizons on the device and on the host system, barrier weights that damp steps and move the hinge width, squareplus, the
declined calls, phase 1 and the sharded gathers.  Optima alone do not pin that: a dispatch that takes the wrong body, or one weighted
solve too many, reaches the same optimum.

Per solve, from `DeviceSolver.last_info`: `status`, `fast_path`, `ipm_iters`, `structured_solves`, `outer_solves`, `active_set_rounds`.
tests/golden/cone_ledger.json holds these (tests/test_cone_ledger_gpu.py compares them exactly); the SHA-256 of the X and U bytes of
every solve of a configuration is printed only — a kernel change may move it, a host-side change must not.

    python tools/cone_ledger.py [--out ledger.json] [--verbose] [config ...]

--verbose passes `verbose=True` to every solve: the library's trace of its iterations on stdout (the smoothed body prints every Newton step).
"""
import argparse
import hashlib
import json
import sys
import threading
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FIELDS = ("status", "fast_path", "ipm_iters", "structured_solves", "outer_solves", "active_set_rounds")
_verbose = [False]  # main(): --verbose
_group = [7300]  # ids of the in-process communicators (tests/test_multirank_gpu.py counts from 1000, tools/scp_loop_ledger.py from 7100)


def _tied(copies, others, Nc, bu, seed):
    from tests.test_cone_ties_gpu import tied_problem

    return tied_problem(np.random.default_rng(seed), copies, others, 6, 4, 2, bu, Nc)


def _rand(seed, M, *rest, N=6, bu=0.4):
    from tests.support.problems import rand_problem

    return rand_problem(np.random.default_rng(seed), M, N, 4, 2, bu, *rest)


def _forced(copies, others, Nc, bu, seed):
    """tests/test_cone_ties_gpu.py, every body forced on the same problem: two solves on one context per `cone_path` (the second one
    meets what the first left in `fp_key`, `cone_lam` and `cone_rw`)."""
    args, kw = _tied(copies, others, Nc, bu, seed)
    return [dict(name=f"cone_path{path}", args=args, kw=kw, Nc=Nc, options={"cone_path": path}, repeats=2) for path in (0, 1, 2, 3)]


def _weighted(world=1):
    args, kw = _rand(105, 6)
    wts = 0.2 + np.random.default_rng(106).random(6)
    if world > 1:
        return [dict(name="weights", args=args, kw=kw, Nc=1, weights=wts, world=world, repeats=2)]
    return [dict(name=f"cone_path{path}", args=args, kw=kw, Nc=1, weights=wts, options={"cone_path": path}, repeats=2) for path in (0, 3)]


def _worst_k(case):
    g = np.load(ROOT / "tests" / "golden" / "worstk_ties.npz")
    names = ["x0", "f", "fx", "fu", "X_prev", "U_prev", "Q", "R", "X_ref", "U_ref"]
    args = tuple(g[f"c{case}_{n}"] for n in names)
    kw = {k_[len(f"c{case}_kw_"):]: (float(g[k_]) if g[k_].ndim == 0 else g[k_]) for k_ in g.files if k_.startswith(f"c{case}_kw_")}
    Nc, k = (int(v) for v in g[f"c{case}_meta"])
    return [dict(name="k", args=args, kw=kw, Nc=Nc, solve=dict(cone_k=k), repeats=2)]


def _one(name, args_kw, Nc=1, **run):
    return [dict(name=name, args=args_kw[0], kw=args_kw[1], Nc=Nc, **run)]


_LOG10 = dict(smooth_alpha=10.0)  # the log barrier at the weight most tests use
_PHASE1 = (1, 6, 2.0)  # rand_problem: seed, M, state bound (control bound 0.4); phase 1 ends with status 0, so does the solve


def _squareplus(beta):
    return dict(smooth_alpha=10.0, smooth_cstr="squareplus", smooth_beta=beta)


# name -> the runs of the configuration: each one context (or `world` in-process ranks), `repeats` solves of one problem
CONFIGS = {
    "tied_2_4_nc1": lambda: _forced(2, 4, 1, 0.4, 1231),
    "tied_5_3_nc1": lambda: _forced(5, 3, 1, 0.4, 507),
    "tied_4_3_nc2": lambda: _forced(4, 3, 2, 0.4, 407),
    "tied_4_3_ncN": lambda: _forced(4, 3, -1, 5.0, 1250),
    "one_particle": lambda: _one("solve", _rand(31, 1)),  # a single solve at weight 1 - eps
    "weights": _weighted,  # the `user` scaling of the costs: epigraph path (cone_path 0), rank-based iteration (3) ...
    "weights_two_ranks": lambda: _weighted(2),  # ... and the sharded check
    "worst_k": lambda: _worst_k(41),  # tests/golden/worstk_ties.npz, case 41: four costs on the threshold
    "fp32_storage": lambda: _one("solve", _rand(77, 12, N=8, bu=0.5), f32=True, solve=dict(cold_start=True)),  # tests/test_cone_gpu.py: the widened copy
    "tied_5_3_two_ranks": lambda: _one("solve", _tied(5, 3, 1, 0.4, 708), world=2, repeats=2),  # tests/test_multirank_gpu.py: host check, all-gathered quadratics
    "tied_5_3_four_ranks": lambda: _one("solve", _tied(5, 3, 1, 0.4, 710), world=4, repeats=2),
    "logbarrier_3_3": lambda: _one("solve", _tied(3, 3, 1, 0.4, 907), solve=dict(smooth_alpha=10.0)),  # the dispatch into lcone_smooth_body
    "squareplus_one_particle_slew": lambda: _one("solve", _rand(74, 1, None, 0.5, None), solve=dict(smooth_alpha=10.0, smooth_cstr="squareplus", smooth_beta=2.0)),
    # ---- the smoothed boxes' Newton iteration (SmoothSolve), branch by branch ----
    # two solves on one context: warm start from the last solution, multipliers and hinge width remembered / not remembered / cold
    "smooth_5_3_twice": lambda: _one("solve", _tied(5, 3, 1, 0.4, 1507), solve=_LOG10, repeats=2),
    "smooth_5_3_twice_no_rank_memory": lambda: _one("solve", _tied(5, 3, 1, 0.4, 1507), solve=_LOG10, options={"cone_rank_memory": 0}, repeats=2),
    "smooth_5_3_twice_cold": lambda: _one("solve", _tied(5, 3, 1, 0.4, 1507), solve=dict(_LOG10, cold_start=True), repeats=2),
    # consensus horizons: Newton system on the device (Nc u = 4, off-diagonal blocks condensed), on the host (Nc u = 12), no shared control
    "smooth_3_3_nc2": lambda: _one("solve", _tied(3, 3, 2, 0.4, 506), Nc=2, solve=_LOG10),
    "smooth_4_2_ncN": lambda: _one("solve", _tied(4, 2, -1, 0.4, 506), Nc=-1, solve=_LOG10),
    "smooth_nc0": lambda: _one("solve", _rand(501, 6), Nc=0, solve=_LOG10),
    # barrier weights (tests/test_cone_ties_gpu.py, test_logbarrier_smoothing_with_ties): damped steps, width changes
    "smooth_9_4_alpha1": lambda: _one("solve", _tied(9, 4, 1, 0.4, 2708), solve=dict(smooth_alpha=1.0)),
    "smooth_3_3_alpha100": lambda: _one("solve", _tied(3, 3, 1, 0.4, 907), solve=dict(smooth_alpha=100.0)),
    "squareplus_7": lambda: _one("solve", _rand(40, 7), solve=_squareplus(1.0)),
    "squareplus_tied_3_3": lambda: _one("solve", _tied(3, 3, 1, 0.4, 41), solve=_squareplus(5.0)),
    "squareplus_one_particle": lambda: _one("solve", _rand(71, 1), solve=_squareplus(2.0)),
    "squareplus_one_weighted_particle": lambda: _one("solve", _rand(85, 1), weights=np.array([2.5]), solve=_squareplus(2.0)),
    # declined by the smoothed body (-1): which body answers instead
    "logbarrier_weights_declined": lambda: _one("solve", _rand(105, 6), weights=0.2 + np.random.default_rng(106).random(6), solve=_LOG10),
    "logbarrier_slew_declined": lambda: _one("solve", _rand(75, 6, None, 0.5, None), solve=_LOG10),
    # state boxes the rollout of the caller's controls leaves: phase 1 (the barrier QP), then the iteration from its controls
    "smooth_phase1": lambda: _one("solve", _rand(*_PHASE1), solve=_LOG10),
    "smooth_phase1_fails": lambda: _one("solve", _rand(0, 6, 1.0), solve=_LOG10),  # boxes the barrier QP cannot enter either: status 1, NaN outputs
    # sharded (tests/test_multirank_gpu.py): the gathers of the costs, of the read-back after the direction, of the host system's table
    "smooth_3_3_two_ranks": lambda: _one("solve", _tied(3, 3, 1, 0.4, 906), world=2, solve=_LOG10, repeats=2),
    "smooth_5_3_four_ranks": lambda: _one("solve", _tied(5, 3, 1, 0.4, 910), world=4, solve=_LOG10, repeats=2),
    "smooth_3_3_nc2_two_ranks": lambda: _one("solve", _tied(3, 3, 2, 0.4, 506), Nc=2, world=2, solve=_LOG10, repeats=2),
    "smooth_4_2_ncN_two_ranks": lambda: _one("solve", _tied(4, 2, -1, 0.4, 506), Nc=-1, world=2, solve=_LOG10, repeats=2),
    "squareplus_two_ranks": lambda: _one("solve", _tied(3, 5, 1, 0.4, 932), world=2, solve=_squareplus(5.0)),
}


def _solves(s, args, kw, Nc, sl=slice(None), options=None, repeats=1, weights=None, f32=False, solve=None, sharded=False):
    """`repeats` solves of one problem (particles `sl` of it) on the context `s`: [(integers of last_info, X, U)]."""
    import torch

    x0, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref = args
    dev = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(np.asarray(a)[sl]), dtype=dt, device="cuda")
    md = torch.float32 if f32 else torch.float64
    T = lambda a: dev(np.swapaxes(a, -1, -2), md)
    for key, val in (options or {}).items():
        s.set_option(key, val)
    opt = dict(solve or {})
    for name, lo, hi in (("u", "lu", "uu"), ("x", "lx", "ux")):
        if f"{name}_l" in kw:
            opt.update({lo: dev(kw[f"{name}_l"]), hi: dev(kw[f"{name}_u"])})
    if "slew_reg" in kw:
        opt.update(slew_reg=dev(kw["slew_reg"]))
    if "slew_reg0" in kw:
        opt.update(slew_reg0=dev(kw["slew_reg0"]), slew_um1=dev(kw["slew_um1"]))
    if weights is not None:
        opt.update(weights=dev(weights))
    out = []
    for rep in range(repeats):
        if sharded:
            opt["static_cons_bounds"] = rep > 0
        X, U, status = s.lcone_solve(f=dev(f), fx=T(fx), fu=T(fu), X_prev=dev(X_prev), U_prev=dev(U_prev), Q=T(Q), R=T(R), X_ref=dev(X_ref), U_ref=dev(U_ref),
                                     reg_x=kw["reg_x"], reg_u=kw["reg_u"], Nc=Nc, symmetric_cost=True, verbose=_verbose[0], **opt)
        s.sync()
        info = {k: int(s.last_info[k]) for k in FIELDS}
        assert info["status"] == status
        out.append((info, X.cpu().numpy(), U.cpu().numpy()))
    return out


def _sharded(world, args, **run):
    """The solves on `world` in-process ranks (one thread and one context each, particles in contiguous blocks, as
    tests/test_multirank_gpu.py drives them)."""
    from pmpc_amd.device import DeviceSolver

    M = args[1].shape[0]
    assert M % world == 0
    Ml = M // world
    _group[0] += 1
    group, out, errs = _group[0], [None] * world, []

    def rank_fn(rank):
        try:
            s = DeviceSolver(0)
            try:
                assert s.lib.pmpc_comm_init_mock(s.h, rank, world, group) == 0
                s.rank, s.world = rank, world
                out[rank] = _solves(s, args, sl=slice(rank * Ml, (rank + 1) * Ml), sharded=True, **run)
            finally:
                s.close()
        except Exception as e:  # surface failures of a rank thread in the main thread
            errs.append(e)

    threads = [threading.Thread(target=rank_fn, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errs, errs
    assert all(o is not None for o in out), "a rank did not finish (deadlock in a collective?)"
    return out


def run_config(name):
    """(ledger, SHA-256 of the X and U bytes of every solve) of one configuration, on fresh contexts."""
    from pmpc_amd.device import DeviceSolver

    led, h = {}, hashlib.sha256()
    for run in CONFIGS[name]():
        run = dict(run)
        key, world = run.pop("name"), run.pop("world", 1)
        if world > 1:
            ranks = _sharded(world, run.pop("args"), **run)
            led[key] = {f"rank{r}": [o[0] for o in outs] for r, outs in enumerate(ranks)}
            arrays = [a for outs in ranks for o in outs for a in o[1:]]
        else:
            s = DeviceSolver(0)
            try:
                outs = _solves(s, **run)
            finally:
                s.close()
            led[key] = [o[0] for o in outs]
            arrays = [a for o in outs for a in o[1:]]
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
    return led, h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("configs", nargs="*", default=list(CONFIGS), help="default: all")
    ap.add_argument("--out", help="write {config: ledger} as JSON")
    ap.add_argument("--verbose", action="store_true", help="verbose=True for every solve: the library prints its iterations")
    a = ap.parse_args()
    _verbose[0] = a.verbose
    ledgers = {}
    for name in a.configs:
        ledgers[name], digest = run_config(name)
        print(f"{name}: {json.dumps(ledgers[name])}\n{name}: sha256(X, U) {digest}", flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(ledgers, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
