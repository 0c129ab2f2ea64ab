#!/usr/bin/env python
"""What a closed-loop MPC step costs: `MPCController.step` against repeated `pmpc_amd.solve(..., device="cuda")` calls with a warm start
shifted on the host, and the launch times of the rollout / plan-shift kernels next to one linearisation launch.  Not a benchmark of the
solver (bench.py is); the numbers of CHANGELOG.md's MPCController entry come from here.

    python tools/mpc_step_time.py --model quadrotor --M 4096 --N 50 --steps 50 --iterations 3
    python tools/mpc_step_time.py --model bicycle --keepout 2        # both versions with a keep-out constraint of 2 balls per particle
    python tools/mpc_step_time.py --model bicycle --iterations 1 --warm-shift --no-solve   # MPCController(warm_shift=True): the same episode
    python tools/mpc_step_time.py --custom-model --no-solve      # the bicycle written as a pmpc_amd.CustomModel (compiled at run time)

Kernel times: HIP events on the solver's stream around single launches, all shapes warmed first, the kernels alternating in one loop.
Step times: host clock around calls that end with a device->host read (both are synchronous), the two versions alternating step by step
on the same sequence of measured states.  Prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def _stats(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)))


def kernel_times(solver, mid, d, reps=30, also=None):
    """Median / spread in microseconds of one launch of rollout, shift_plan (s = 1), linearize and shift_active_set (s = 1).
    `also`: a second model id of the same dimensions, whose three kernels take turns with the first one's ("<kernel>_also")."""
    import torch

    X, U = d["X_prev"], d["U_prev"]
    Xo, Uo, um1 = torch.empty_like(X), torch.empty_like(U), torch.empty((U.shape[0], U.shape[2]), dtype=torch.float64, device=U.device)
    f, fx, fu = solver.linearize(mid, d["x0"], X, U, d["params"])
    jobs = {}
    for m, tag in [(mid, "")] + ([(also, "_also")] if also is not None else []):
        jobs["rollout" + tag] = lambda m=m: solver.rollout(m, d["x0"], U, d["params"], out=Xo, wait_current_stream=False)
        jobs["shift_plan" + tag] = lambda m=m: solver.shift_plan(m, X, U, d["params"], s=1, X_out=Xo, U_out=Uo, um1_out=um1, wait_current_stream=False)
        jobs["linearize" + tag] = lambda m=m: solver.linearize(m, d["x0"], X, U, d["params"], f, fx, fu, wait_current_stream=False)
    if hasattr(solver.lib, "pmpc_shift_active_set_device") and d.get("lu") is not None:  # (an older library under A/B has none)
        act, act_o = torch.zeros(U.shape, dtype=torch.int32, device=U.device), torch.empty(U.shape, dtype=torch.int32, device=U.device)
        jobs["shift_active_set"] = lambda: solver.shift_active_set(act, U, d["lu"], d["uu"], 1, s=1, U_out=Uo, act_out=act_o, wait_current_stream=False)
    out = {k: [] for k in jobs}
    with torch.cuda.stream(solver.stream):
        for rep in range(reps + 5):
            for k, job in jobs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                job()
                e1.record()
                e1.synchronize()
                if rep >= 5:  # (the first five rounds warm every kernel)
                    out[k].append(1e3 * e0.elapsed_time(e1))
    return {k: _stats(v) for k, v in out.items()}


def solver_arch(solver):
    import torch

    return torch.cuda.get_device_properties(solver.device).gcnArchName.split(":")[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="bicycle", choices=["unicycle", "quadrotor", "bicycle"])
    ap.add_argument("--M", type=int, default=256)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--steps", type=int, default=50, help="timed MPC steps per version (after --warmup)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--keepout", type=int, default=0, metavar="K", help="K balls per particle beside the start plan (tools/keepout_time.py make_cstr): "
                    "MPCController(keepout=...) against solve(builtin_cstr=...)")
    ap.add_argument("--warm-shift", action="store_true", help="MPCController(warm_shift=True): the active set is moved along with the plan and the first "
                    "iteration of a shifted step starts warm; the same episode otherwise")
    ap.add_argument("--custom-model", action="store_true", help="the bicycle written as a pmpc_amd.CustomModel (tests/support/custom_models.py): compiled at "
                    "run time, linearised by automatic differentiation; kernel times next to the built-in bicycle's (\"_also\")")
    ap.add_argument("--no-solve", action="store_true", help="leave the pmpc_amd.solve version out (kernel times and the controller only)")
    args = ap.parse_args()

    import pmpc_amd
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver, to_device_problem

    prob = getattr(dyn, f"make_{args.model}_problem")(M=args.M, N=args.N, Nc=1)
    mid = dyn.model_id(args.model)
    F = getattr(dyn, args.model)
    solver = DeviceSolver(0)
    result = dict(model=args.model, M=args.M, N=args.N, iterations=args.iterations, steps=args.steps)
    if args.custom_model:
        if args.model != "bicycle":
            raise SystemExit("--custom-model is the bicycle: --model bicycle")
        from tests.support import custom_models

        model = custom_models.make("bicycle")
        t0 = time.perf_counter()
        model.compile(arch=solver_arch(solver))
        result["custom_model"], result["compile_ms"] = True, 1e3 * (time.perf_counter() - t0)
        result["kernel_us"] = kernel_times(solver, solver.load_model(model), to_device_problem(prob), also=mid)  # ("_also": the built-in id)
    else:
        model = args.model
        result["kernel_us"] = kernel_times(solver, mid, to_device_problem(prob))

    common = dict(X_ref=prob["X_ref"], U_ref=prob["U_ref"], u_l=prob["u_l"], u_u=prob["u_u"], reg_x=prob["reg_x"], reg_u=prob["reg_u"],
                  solver_settings=dict(solver="osqp", Nc=1))
    ctl_kw, solve_kw = {}, {}
    if args.keepout:
        from keepout_time import make_cstr  # (tools/ is the script's directory)

        cstr = make_cstr(prob, args.keepout, 3 if args.model == "quadrotor" else 2)
        ctl_kw, solve_kw = dict(keepout={k: cstr[k] for k in ("pos_idx", "centres", "radius")}), dict(builtin_cstr=cstr)
        result["keepout"] = args.keepout
    if args.warm_shift:
        ctl_kw["warm_shift"] = True
    result["warm_shift"] = bool(args.warm_shift)
    ctl = pmpc_amd.MPCController(builtin_model=model, params=prob["params"], Q=prob["Q"], R=prob["R"], solver=solver, **ctl_kw, **common)
    ctl.reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
    Xs, Us = prob["X_prev"], prob["U_prev"]  # the solve version's warm start
    rng = np.random.default_rng(0)
    x0 = prob["x0"][0]
    t_ctl, t_solve, first, later, started_warm = [], [], [], [], []
    fresh, restarts = True, 0  # (fresh: the solve version has no plan to shift)
    for k in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        u0, info = ctl.step(x0, iterations=args.iterations)
        t1 = time.perf_counter()
        X = 0
        if u0 is not None and not args.no_solve:
            t2 = time.perf_counter()
            if not fresh:
                Xs, Us, _ = dyn.shift_plan(mid, Xs, Us, prob["params"], s=1)
            X, U, data = pmpc_amd.solve(None, prob["Q"], prob["R"], np.tile(x0, (args.M, 1)), device="cuda", builtin_model=model, params=prob["params"],
                                        X_prev=Xs, U_prev=Us, max_it=args.iterations, res_tol=0.0, verbose=False, **solve_kw, **common)  # (on the package's own context)
            t3 = time.perf_counter()
        if u0 is None or X is None:
            # a hard constraint can leave a shifted plan no feasible step (the particles share particle 0's measured state, not their
            # balls): the episode starts over from the problem's start plan, the failed step is not timed
            if not args.keepout or fresh:
                raise SystemExit(f"step {k} failed: {info}")
            restarts += 1
            ctl.reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
            Xs, Us, x0, fresh = prob["X_prev"], prob["U_prev"], prob["x0"][0], True
            continue
        fresh = False
        if not args.no_solve:
            Xs, Us = X[:, 1:], U
        if k >= args.warmup:
            t_ctl.append(1e3 * (t1 - t0))
            if not args.no_solve:
                t_solve.append(1e3 * (t3 - t2))
            first.append((info["infos"][0]["active_set_rounds"], info["infos"][0]["ipm_iters"]))
            started_warm.append(bool(info.get("warm_shift", False)))  # (.get: an older package under A/B has no such entry)
            later += [(i["active_set_rounds"], i["ipm_iters"]) for i in info["infos"][1:]]
        # (with a keep-out constraint the plant is the model: a disturbed state can sit where the linearised rows leave no feasible first stage)
        x0 = F(x0, u0[0], prob["params"][0])[0] + (0.0 if args.keepout else 0.01) * rng.standard_normal(x0.shape)
    if args.keepout:
        result["episode_restarts"] = restarts
    result["controller_step_ms"] = _stats(t_ctl)
    if t_solve:
        result["solve_step_ms"] = _stats(t_solve)
    mean = lambda rows, c: float(np.mean([r[c] for r in rows])) if rows else float("nan")
    result["first_iteration"] = dict(active_set_rounds=mean(first, 0), ipm_iters=mean(first, 1))
    result["later_iterations"] = dict(active_set_rounds=mean(later, 0), ipm_iters=mean(later, 1))
    # per timed step: (ipm_iters, active_set_rounds) of the first iteration; the share of the timed steps whose first iteration the rounds
    # finished without the interior-point iteration (every timed step follows a shift: the warm-up steps took the one without)
    result["first_iteration_per_step"] = [(int(r[1]), int(r[0])) for r in first]
    result["first_iteration_started_warm"] = float(np.mean(started_warm)) if started_warm else float("nan")
    result["first_iteration_without_ipm"] = float(np.mean([r[1] == 0 for r in first])) if first else float("nan")
    solver.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
