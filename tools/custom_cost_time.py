#!/usr/bin/env python
"""What a custom stage cost costs next to the built-in obstacle cost it can restate: the price of NOT fusing the gradient into the
Cholesky shift (the built-in cost's `k_ref_shift<.., OBS>` forms cx in registers; a `pmpc_amd.CustomCost` writes (cx | cu) to a
scratch that `launch_ref_shift` reads back).  The numbers of CHANGELOG.md's custom-cost entry come from here.

    python tools/custom_cost_time.py --what loop --model quadrotor --M 4096 --N 50      # config D's size: library loop, time per iteration
    python tools/custom_cost_time.py --what mpc --model bicycle --M 256 --N 30          # MPCController, 3 iterations per step

Both versions carry the same K = 2 Gaussian obstacles in the position entries (the custom one compiled with uses_u=False, parameters per
particle) and are checked to agree before anything is timed.  They alternate repeat by repeat (loop) / step by step on the same measured
states (mpc); times are a host clock around calls that end with a device->host read; reported: median, min, max per version and the
median of the paired differences.  `kernel_us`: HIP events around single launches of the fused built-in shift, the custom gradient
kernel and the plain shift, alternating in one loop, all warmed first.  Prints one JSON line."""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

# K = 2 Gaussian bumps in x[0 .. PD-1] (PD = 2 or 3, a macro in front); p = [centres (2 PD) | sigma (2) | w (2)]
OBSTACLE_SRC = """
template <class T>
__device__ T stage_cost(const T *x, const T *u, const double *p, int j, int N) {
  T c = 0.0;
  for (int k = 0; k < 2; k++) {
    T r2 = 0.0;
    for (int d = 0; d < PD; d++) r2 += (x[d] - p[k * PD + d]) * (x[d] - p[k * PD + d]);
    c += p[2 * PD + 2 + k] * exp(-0.5 * r2 / (p[2 * PD + k] * p[2 * PD + k]));
  }
  return c;
}
"""


def _stats(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def costs(model, prob, M):
    """(built-in dict, custom dict) of the same two obstacles beside the start plan."""
    import pmpc_amd

    pd, x, u = (3, 12, 4) if model == "quadrotor" else (2, 4, 2)
    P0 = prob["X_prev"][..., :pd]
    lo, hi = P0.reshape(-1, pd).min(0), P0.reshape(-1, pd).max(0)
    centres = np.stack([lo + 0.35 * (hi - lo), lo + 0.7 * (hi - lo)]) + 0.3
    sigma, w = np.array([1.0, 1.5]), np.array([2.0, 1.0])
    builtin = dict(kind="obstacles", pos_idx=tuple(range(pd)), centres=centres, sigma=sigma, w=w)
    cost = pmpc_amd.CustomCost(f"#define PD {pd}\n" + OBSTACLE_SRC, x, u, 2 * pd + 4, uses_u=False, name=f"obstacles_{pd}d")
    params = np.tile(np.concatenate([centres.reshape(-1), sigma, w])[None], (M, 1))
    return builtin, dict(kind="custom", cost=cost, params=params)


def kernel_times(solver, d, builtin, custom, reps=30):
    import torch

    X, U = d["X_prev"], d["U_prev"]
    M, N, x = X.shape
    hb = solver.prepare_cost(builtin, N, x, X.device)
    hc = solver.prepare_cost(custom, N, x, X.device, M=M, u=U.shape[-1])
    out_b, out_c, cx = torch.empty_like(X), torch.empty_like(X), torch.empty_like(X)
    jobs = {
        # (the ABI entry itself: the Python method synchronises after an asynchronous call)
        "builtin_fused_shift": lambda: solver.lib.pmpc_obstacle_ref_shift_device(solver.h, ctypes.byref(hb[0]), x, N, M, X.data_ptr(), d["Q"].data_ptr(),
                                                                                 d["X_ref"].data_ptr(), out_b.data_ptr()),
        "custom_grad": lambda: solver.custom_cost_grad(hc[0].id, X, U, hc[1][0], cx=cx, wait_current_stream=False),
        "plain_shift_Q": lambda: solver.ref_shift(d["Q"], cx, d["X_ref"], out=out_c, wait_current_stream=False, check=False),
    }
    t = {k: [] for k in jobs}
    with torch.cuda.stream(solver.stream):
        for rep in range(reps + 5):
            for k, job in jobs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                job()
                e1.record()
                e1.synchronize()
                if rep >= 5:
                    t[k].append(1e3 * e0.elapsed_time(e1))
    agree = float((out_b - out_c).abs().max())
    return {k: _stats(v) for k, v in t.items()}, agree


def time_loops(args, prob, mid, builtin, custom):
    """The library loop from the problem's start iterate, `--iterations` iterations per call, a context per version, alternating."""
    import torch

    from pmpc_amd.device import DeviceSolver, to_device_problem

    d = to_device_problem(prob)
    M, N, x = d["X_prev"].shape
    u = d["U_prev"].shape[-1]
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    common = dict(Q=d["Q"], R=d["R"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=1, x0=d["x0"], lu=d["lu"], uu=d["uu"], symmetric_cost=True,
                  X_ref=d["X_ref"], U_ref=d["U_ref"])
    legs = {}
    for name, cost in (("builtin", builtin), ("custom", custom)):
        s = DeviceSolver(0)
        handle = s.prepare_cost(cost, N, x, "cuda", M=M, u=u)
        legs[name] = dict(s=s, handle=handle, bufs=[mk(M, N, x), mk(M, N, x, x), mk(M, N, u, x), mk(M, N, x), mk(M, N, x, x), mk(M, N, u, x)],
                          pair=[mk(M, N, x), mk(M, N, u), mk(M, N, x), mk(M, N, u)], t=[], res=None)
    result = {}
    result["kernel_us"], result["kernel_agree_max_abs"] = kernel_times(legs["custom"]["s"], d, builtin, custom)

    def run(leg):
        s, b, (Xa, Ua, Xb, Ub) = leg["s"], leg["bufs"], leg["pair"]
        Xa.copy_(d["X_prev"])
        Ua.copy_(d["U_prev"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res, infos, last, done = s.scp_loop(mid, d["params"], args.iterations, f=b[0], fx=b[1], fu=b[2], f2=b[3], fx2=b[4], fu2=b[5], X_prev=Xa, U_prev=Ua,
                                            X_out=Xb, U_out=Ub, first_cold=True, cost=leg["handle"], wait_current_stream=False, **common)
        r = res.cpu().numpy()  # (synchronises)
        dt = time.perf_counter() - t0
        assert done == args.iterations and all(i["status"] == 0 for i in infos), infos
        return 1e3 * dt / args.iterations, r, ((Xb, Ub) if last else (Xa, Ua))

    for rep in range(args.warmup + args.repeats):
        outs = {}
        for name in (("builtin", "custom") if rep % 2 == 0 else ("custom", "builtin")):
            ms, r, (X, U) = run(legs[name])
            outs[name] = (r, X.clone())
            if rep >= args.warmup:
                legs[name]["t"].append(ms)
        result["agree_max_abs_X"] = float((outs["builtin"][1] - outs["custom"][1]).abs().max())
        result["agree_max_abs_resid"] = float(np.abs(outs["builtin"][0] - outs["custom"][0]).max())
    result["iteration_ms"] = {k: _stats(v["t"]) for k, v in legs.items()}
    result["paired_difference_ms"] = _stats(np.array(legs["custom"]["t"]) - np.array(legs["builtin"]["t"]))
    for leg in legs.values():
        leg["s"].close()
    return result


def time_mpc(args, prob, model, builtin, custom):
    """Two controllers, a context each, alternating step by step on the same measured states (the built-in controller's control drives
    the plant)."""
    import pmpc_amd
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver

    F = getattr(dyn, model)
    common = dict(builtin_model=model, params=prob["params"], Q=prob["Q"], R=prob["R"], X_ref=prob["X_ref"], U_ref=prob["U_ref"], u_l=prob["u_l"],
                  u_u=prob["u_u"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], solver_settings=dict(solver="osqp", Nc=1))
    ctl = {}
    for name, cost in (("builtin", builtin), ("custom", custom)):
        ctl[name] = pmpc_amd.MPCController(builtin_cost=cost, solver=DeviceSolver(0), **common)
        ctl[name].reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
    rng = np.random.default_rng(0)
    x0 = prob["x0"][0]
    t = dict(builtin=[], custom=[])
    worst = 0.0
    for k in range(args.warmup + args.repeats):
        u0 = {}
        for name in (("builtin", "custom") if k % 2 == 0 else ("custom", "builtin")):
            t0 = time.perf_counter()
            u0[name], info = ctl[name].step(x0, iterations=args.iterations)
            dt = time.perf_counter() - t0
            if u0[name] is None:
                raise SystemExit(f"step {k} of the {name} controller failed: {info}")
            if k >= args.warmup:
                t[name].append(1e3 * dt)
        worst = max(worst, float(np.abs(u0["builtin"] - u0["custom"]).max()))
        x0 = F(x0, u0["builtin"][0], prob["params"][0])[0] + 0.01 * rng.standard_normal(x0.shape)
    out = dict(step_ms={k: _stats(v) for k, v in t.items()}, paired_difference_ms=_stats(np.array(t["custom"]) - np.array(t["builtin"])), agree_max_abs_u0=worst)
    for c in ctl.values():
        c.solver.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", default="loop", choices=["loop", "mpc"])
    ap.add_argument("--model", default="quadrotor", choices=["quadrotor", "bicycle"])
    ap.add_argument("--M", type=int, default=4096)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--iterations", type=int, default=None, help="SCP iterations per loop call (default 10) / per MPC step (default 3)")
    ap.add_argument("--repeats", type=int, default=None, help="timed loop calls (default 7) / MPC steps (default 50) per version")
    ap.add_argument("--warmup", type=int, default=None, help="untimed repeats first (default 2 / 5)")
    args = ap.parse_args()
    loop = args.what == "loop"
    args.iterations = args.iterations or (10 if loop else 3)
    args.repeats = args.repeats or (7 if loop else 50)
    args.warmup = args.warmup if args.warmup is not None else (2 if loop else 5)

    from pmpc_amd import dynamics as dyn

    prob = getattr(dyn, f"make_{args.model}_problem")(M=args.M, N=args.N, Nc=1)
    builtin, custom = costs(args.model, prob, args.M)
    t0 = time.perf_counter()
    custom["cost"].compile()
    result = dict(what=args.what, model=args.model, M=args.M, N=args.N, iterations=args.iterations, repeats=args.repeats,
                  compile_ms=1e3 * (time.perf_counter() - t0))
    result.update(time_loops(args, prob, dyn.model_id(args.model), builtin, custom) if loop else time_mpc(args, prob, args.model, builtin, custom))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
