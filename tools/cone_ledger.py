"""The ledger of the cone objective's hard-box half (`lcone_body`, csrc/solver_cone.hip): which body answered a call and how many solves it
took, as integers, on the smallest shape an existing test uses per dispatch.  Optima alone do not pin that: a dispatch that takes the
wrong body, or one weighted solve too many, reaches the same optimum.

Per solve, from `DeviceSolver.last_info`: `status`, `fast_path`, `ipm_iters`, `structured_solves`, `outer_solves`, `active_set_rounds`.
tests/golden/cone_ledger.json holds these (tests/test_cone_ledger_gpu.py compares them exactly); the SHA-256 of the X and U bytes of
every solve of a configuration is printed only — a kernel change may move it, a host-side change must not.

    python tools/cone_ledger.py [--out ledger.json] [config ...]
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
                                     reg_x=kw["reg_x"], reg_u=kw["reg_u"], Nc=Nc, symmetric_cost=True, **opt)
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
    a = ap.parse_args()
    ledgers = {}
    for name in a.configs:
        ledgers[name], digest = run_config(name)
        print(f"{name}: {json.dumps(ledgers[name])}\n{name}: sha256(X, U) {digest}", flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(ledgers, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
