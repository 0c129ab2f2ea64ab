"""The launch ledger of the library's SCP loop (`pmpc_scp_loop_device*`, csrc/solver_scp.hip): what a loop DID, as integers, on one small
configuration per dispatch of its follow-up.  Iterates alone do not pin that: a loop that linearises twice, or runs the separate residual
where the fused launch belonged, still walks the right iterates.

Per configuration, with `profile(2)`: `done`, `last_in_out`, per iteration `status` / `active_set_rounds` / `ipm_iters`, the two follow-up
counters (`pmpc_scp_loop_follow_ups`: taken as enqueued behind the rounds, enqueued after the solve) and the `linearize` / `scp_residual`
scope counts of `profile_read()`.  tests/golden/scp_loop_ledger.json holds these (tests/test_scp_loop_ledger_gpu.py compares them exactly);
the SHA-256 of the final X, U and residual bytes is printed only — a kernel change may move it, a host-side change must not.

    python tools/scp_loop_ledger.py [--out ledger.json] [config ...]
"""
import argparse
import hashlib
import json
import math
import sys
import threading
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

BUMPS = dict(kind="obstacles", pos_idx=(0, 1), centres=np.array([[1.5, 0.2], [3.5, 2.5]]), sigma=np.array([1.0, 1.0]), w=np.array([3.0, 3.0]))
BUMP_AT_THE_BALL = dict(kind="obstacles", pos_idx=(0, 1), centres=np.array([[2.0, 0.9]]), sigma=np.array([0.5]), w=np.array([2.0]))
LOOP_KEYS = ("Q", "R", "x0", "X_ref", "U_ref", "X_prev", "U_prev", "u_l", "u_u", "reg_x", "reg_u", "params")


def _unicycle(Nc=1, model="unicycle", **args):
    from pmpc_amd import dynamics as dyn

    return dyn.make_unicycle_problem(M=40, N=12, Nc=Nc), model, dict(Nc=Nc, **args)  # the shape of tests/test_device_gpu.py's loop test


def _bicycle(**args):
    from pmpc_amd import dynamics as dyn

    return dyn.make_bicycle_problem(M=40, N=12, Nc=1), "bicycle", args  # tests/test_lin_cost_gpu.py


def _keepout(**args):
    from tests.support.keepout_problems import bicycle_keepout_problem  # tests/test_keepout_loop_gpu.py: M 3, N 12

    kw, cstr = bicycle_keepout_problem()
    return kw, "bicycle", dict(cstr=cstr, **args)


def _pendulum(**args):
    from tests.support import custom_models as cm  # tests/test_custom_model_gpu.py: the custom pendulum, M 8, N 6

    M, N, rng = 8, 6, np.random.default_rng(11)
    P = np.stack([rng.uniform(8.0, 12.0, M), rng.uniform(0.1, 0.3, M), np.full(M, 0.05)], -1)
    x0 = np.stack([0.6 + 0.1 * rng.standard_normal(M), 0.2 * rng.standard_normal(M)], -1)
    kw = dict(x0=x0, Q=np.tile(np.diag([4.0, 1.0]), (M, N, 1, 1)), R=np.tile(0.1 * np.eye(1), (M, N, 1, 1)), X_ref=np.zeros((M, N, 2)), U_ref=np.zeros((M, N, 1)),
              X_prev=np.tile(x0[:, None], (1, N, 1)), U_prev=np.zeros((M, N, 1)), u_l=-3.0 * np.ones((M, N, 1)), u_u=3.0 * np.ones((M, N, 1)), reg_x=1.0, reg_u=1.0,
              params=P)
    return kw, cm.make("pendulum"), args


def _cone_quadrotor(**args):
    from pmpc_amd import dynamics as dyn

    return dyn.make_quadrotor_problem(M=96, N=20, Nc=1), "quadrotor", dict(solver="ecos", **args)  # tests/test_cone_ties_gpu.py's loop test


# name -> (problem, model, loop arguments).  prime: one cold iteration first, the recorded loop continues from it with first_cold = False.
CONFIGS = {
    "boxes_nc1_cold": lambda: _unicycle(steps=4),  # compact records from iteration 1
    "boxes_nc1_primed": lambda: _unicycle(steps=4, prime=True),  # compact from iteration 0
    "boxes_nc3": lambda: _unicycle(3, steps=4),  # dense, fused linearisation + residual
    "one_step": lambda: _unicycle(steps=1),  # no next linearisation
    "obstacle_cost": lambda: _bicycle(steps=4, cost=BUMPS),
    "keepout": lambda: _keepout(steps=4),  # strip, then the dense linearisation
    "keepout_and_cost": lambda: _keepout(steps=4, cost=BUMP_AT_THE_BALL),
    "custom_model": lambda: _pendulum(steps=3),
    "cone_objective": lambda: _cone_quadrotor(steps=4),
    "two_mock_ranks": lambda: _unicycle(steps=4, world=2),  # separate residual + all-reduce
    "unknown_model": lambda: _unicycle(model=999, steps=3),  # refused: nothing runs
}
_group = [7100]  # ids of the in-process communicators (tests/test_multirank_gpu.py counts from 1000)


def _loop(s, kw, model, steps, Nc=1, prime=False, cost=None, cstr=None, solver="osqp", count_follow_ups=True):
    """One recorded loop on the context `s`: (ledger, [X, U, res] as numpy)."""
    import torch

    from pmpc_amd import _lib
    from pmpc_amd.device_problem import build_problem, keepout_buffers

    unknown = isinstance(model, int)
    p = build_problem(kw["Q"], kw["R"], kw["x0"], kw["X_ref"], kw["U_ref"], kw["X_prev"], kw["U_prev"], None, None, kw["u_l"], kw["u_u"], kw["reg_x"], kw["reg_u"],
                      None, None, dict(solver=solver, Nc=Nc), None, "unicycle" if unknown else model, kw["params"], "cuda")
    M, N, x, u = p.M, p.N, p.xdim, p.udim
    mid = model if unknown else (s.load_model(p.model) if not isinstance(p.model, int) else p.model)
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    handle = aug = None
    if cstr is not None:
        handle = s.prepare_cstr(cstr, M, N, x)
        aug = keepout_buffers(p, handle[0].K)
    bufs = dict(f=zeros(M, N, x), fx=zeros(M, N, x, x), fu=zeros(M, N, u, x), f2=zeros(M, N, x), fx2=zeros(M, N, x, x), fu2=zeros(M, N, u, x))
    extra = dict(cone_objective=True, barrier_mu=0.0 if math.isnan(p.smooth_alpha) else 1.0 / p.smooth_alpha) if p.cone else {}
    pairs = [(p.X_prev, p.U_prev), (zeros(M, N, x), zeros(M, N, u))]
    call = lambda n, cold, res: s.scp_loop(mid, p.params, n, X_prev=pairs[0][0], U_prev=pairs[0][1], X_out=pairs[1][0], U_out=pairs[1][1], X_ref=p.X_ref,
                                           U_ref=p.U_ref, first_cold=cold, res=res, cost=cost, cstr=handle, aug=aug, **bufs, **p.solve_kw(), **extra)
    torch.cuda.synchronize()
    if prime:
        _, _, last, done = call(1, True, zeros(1))
        s.sync()
        assert done == 1
        if last:
            pairs.reverse()
    s.profile(2)
    s.profile_read()
    if count_follow_ups:
        _lib.scp_loop_follow_ups(reset=True)
    res, infos, last, done = call(steps, not prime, zeros(steps))
    s.sync()
    prof = s.profile_read()
    led = dict(done=int(done), last_in_out=int(last), status=[int(i["status"]) for i in infos], active_set_rounds=[int(i["active_set_rounds"]) for i in infos],
               ipm_iters=[int(i["ipm_iters"]) for i in infos], linearize=int(prof["linearize"][1]), scp_residual=int(prof["scp_residual"][1]))
    if count_follow_ups:
        led["follow_ups"] = [int(v) for v in _lib.scp_loop_follow_ups()]
    X, U = pairs[1] if last else pairs[0]
    return led, [X.cpu().numpy(), U.cpu().numpy(), res.cpu().numpy()]


def _sharded(kw, model, world, **args):
    """The loop on `world` in-process ranks (one thread and one context each, particles in contiguous blocks, as tests/test_multirank_gpu.py
    drives them): every rank's ledger, the follow-up counters of all ranks together."""
    from pmpc_amd import _lib
    from pmpc_amd.device import DeviceSolver

    M = kw["Q"].shape[0]
    Ml = M // world
    _group[0] += 1
    group, out, errs = _group[0], [None] * world, []

    def rank_fn(rank):
        try:
            sl = slice(rank * Ml, (rank + 1) * Ml)
            shard = {k: (v[sl] if isinstance(v, np.ndarray) and v.shape[:1] == (M,) else v) for k, v in kw.items()}
            s = DeviceSolver(0)
            try:
                assert s.lib.pmpc_comm_init_mock(s.h, rank, world, group) == 0
                s.rank, s.world = rank, world
                out[rank] = _loop(s, shard, model, count_follow_ups=False, **args)
            finally:
                s.close()
        except Exception as e:  # surface failures of a rank thread in the main thread
            errs.append(e)

    _lib.scp_loop_follow_ups(reset=True)
    threads = [threading.Thread(target=rank_fn, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errs, errs
    assert all(o is not None for o in out), "a rank did not finish (deadlock in a collective?)"
    led = {f"rank{r}": o[0] for r, o in enumerate(out)}
    led["follow_ups"] = [int(v) for v in _lib.scp_loop_follow_ups()]
    return led, [np.concatenate([o[1][k] for o in out]) for k in range(2)] + [out[0][1][2]]


def run_config(name):
    """(ledger, SHA-256 of the final X, U and residuals) of one configuration, on fresh contexts."""
    from pmpc_amd.device import DeviceSolver

    prob, model, args = CONFIGS[name]()
    kw = {k: prob[k] for k in LOOP_KEYS}
    world = args.pop("world", 1)
    if world > 1:
        led, arrays = _sharded(kw, model, world, **args)
    else:
        s = DeviceSolver(0)
        try:
            led, arrays = _loop(s, kw, model, **args)
        finally:
            s.close()
    h = hashlib.sha256()
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
        print(f"{name}: {json.dumps(ledgers[name])}\n{name}: sha256(X, U, res) {digest}", flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(ledgers, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
