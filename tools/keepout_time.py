#!/usr/bin/env python
"""What the keep-out constraint costs: one launch of `k_keepout_augment` next to one linearisation launch at the same shape, against the
time its bytes alone would take at a given streaming rate, one launch of the strip-and-residual kernel next to the plain residual
launch, and the per-iteration time of `pmpc_amd.solve(..., device="cuda")` with and without `builtin_cstr` and of the library loop
(`DeviceSolver.scp_loop(cstr=, aug=)`, buffers allocated once as `MPCController` does) with the constraint.  Not a benchmark of the solver (bench.py is); the numbers of CHANGELOG.md's keep-out entry come from here.

    python tools/keepout_time.py --model quadrotor --M 4096 --N 50 --K 2

Kernel times: HIP events on the solver's stream around single launches, both kernels warmed first and alternating in one loop.
Iteration times: host clock around calls of --iterations iterations (res_tol = 0; each ends with a device->host read), the
versions alternating.  Prints one JSON line."""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def _stats(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)))


def make_cstr(prob, K, pos_dim):
    """K balls of radius 0.3 per particle (the per-particle form of the centres): ball k sits 0.6 to the left of the particle's start plan
    at a stage of its own, so every plan is clear of its balls and a plan that moves left there has to go round them."""
    X = prob["X_prev"]
    M, N = X.shape[:2]
    side = np.zeros(pos_dim)
    side[1] = 0.6
    stages = [(k + 1) * N // (K + 1) for k in range(K)]
    centres = np.stack([X[:, j, :pos_dim] + side for j in stages], 1)  # (M, K, pos_dim)
    return dict(kind="keepout", pos_idx=tuple(range(pos_dim)), centres=np.ascontiguousarray(np.broadcast_to(centres[:, None], (M, N, K, pos_dim))), radius=np.full(K, 0.3))


def kernel_times(solver, mid, d, cstr, reps=30):
    import torch

    X, U = d["X_prev"], d["U_prev"]
    M, N, x = X.shape
    f, fx, fu = solver.linearize(mid, d["x0"], X, U, d["params"])
    handle = solver.prepare_cstr(cstr, M, N, x, X.device)
    out = solver.keepout_augment(handle, X, f, fx, fu, X_ref=d["X_ref"])
    jobs = {"linearize": lambda: solver.linearize(mid, d["x0"], X, U, d["params"], f, fx, fu, wait_current_stream=False),
            "keepout_augment": lambda: solver.lib.pmpc_keepout_augment_device(
                solver.h, ctypes.byref(handle[0]), x, U.shape[-1], N, M,
                *[ctypes.c_void_p(t.data_ptr()) for t in (X, f, fx, fu, d["X_ref"], out["f"], out["fx"], out["fu"], out["X_prev"], out["X_ref"], out["xu"])])}
    Xs, Us, res = torch.empty_like(X), U + 0.5, torch.empty((1,), dtype=torch.float64, device=X.device)
    jobs["scp_residual"] = lambda: solver.scp_residual(Xs, X, Us, U, out=res, wait_current_stream=False)
    jobs["strip_residual"] = lambda: solver.strip_residual(out["X_prev"], Xs, X, Us, U, out=res, wait_current_stream=False)
    times = {k: [] for k in jobs}
    with torch.cuda.stream(solver.stream):
        for rep in range(reps + 5):
            for k, job in jobs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                job()
                e1.record()
                e1.synchronize()
                if rep >= 5:  # (the first five rounds warm both kernels)
                    times[k].append(1e3 * e0.elapsed_time(e1))
    return {k: _stats(v) for k, v in times.items()}


def library_leg(prob, model, cstr, iterations):
    """A callable that runs `iterations` iterations of the library loop with the constraint from the problem's start iterate and returns
    (X (M, N, x) numpy or None, infos): every buffer allocated here, once; a call copies the start iterate in and reads the residuals back."""
    import torch

    from pmpc_amd.device import DeviceSolver
    from pmpc_amd.device_problem import build_problem, keepout_buffers

    s = DeviceSolver(0)
    p = build_problem(prob["Q"], prob["R"], prob["x0"], prob["X_ref"], prob["U_ref"], prob["X_prev"], prob["U_prev"], None, None, prob["u_l"], prob["u_u"],
                      prob["reg_x"], prob["reg_u"], None, None, dict(solver="osqp", Nc=1), None, model, prob["params"], "cuda")
    M, N, x, u = p.M, p.N, p.xdim, p.udim
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    handle = s.prepare_cstr(cstr, M, N, x)
    aug = keepout_buffers(p, handle[0].K)
    lin = dict(f=mk(M, N, x), fx=mk(M, N, x, x), fu=mk(M, N, u, x), f2=mk(M, N, x), fx2=mk(M, N, x, x), fu2=mk(M, N, u, x))
    Xa, Ua, Xb, Ub, res = mk(M, N, x), mk(M, N, u), mk(M, N, x), mk(M, N, u), mk(iterations)
    torch.cuda.synchronize()

    def run():
        Xa.copy_(p.X_prev)
        Ua.copy_(p.U_prev)
        _, infos, last, done = s.scp_loop(p.model, p.params, iterations, X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, X_ref=p.X_ref, U_ref=p.U_ref, first_cold=True,
                                          res=res, cstr=handle, aug=aug, **lin, **p.solve_kw())
        r = res.cpu()  # (the device->host read that ends the call, as solve's `hist` row does)
        if done != iterations or not bool(torch.isfinite(r).all()):
            return None, infos
        return (Xb if last else Xa).cpu().numpy(), infos

    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="bicycle", choices=["quadrotor", "bicycle"])
    ap.add_argument("--M", type=int, default=4096)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--K", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--solves", type=int, default=8, help="timed solve calls per version (after two warm-up calls)")
    ap.add_argument("--copy-rate", type=float, default=6.29e12, help="bytes / s of a plain streaming copy, for the bytes-only time")
    ap.add_argument("--no-solve", action="store_true", help="kernel times only")
    args = ap.parse_args()

    import pmpc_amd
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver, to_device_problem

    prob = getattr(dyn, f"make_{args.model}_problem")(M=args.M, N=args.N, Nc=1)
    mid = dyn.model_id(args.model)
    x, u = prob["Q"].shape[-1], prob["R"].shape[-1]
    pos_dim = 3 if args.model == "quadrotor" else 2
    cstr = make_cstr(prob, args.K, pos_dim)
    xd = x + args.K
    solver = DeviceSolver(0)
    result = dict(model=args.model, M=args.M, N=args.N, K=args.K, x=x, u=u, iterations=args.iterations)
    result["kernel_us"] = kernel_times(solver, mid, to_device_problem(prob), cstr)
    units = args.M * args.N
    bytes_in, bytes_out = 8 * (x * x + u * x + 3 * x), 8 * (xd * xd + u * xd + 3 * xd + args.K)
    result["bytes_per_unit"] = dict(read=bytes_in, written=bytes_out)
    result["bytes_only_us"] = 1e6 * units * (bytes_in + bytes_out) / args.copy_rate
    result["kernel_over_bytes_only"] = result["kernel_us"]["keepout_augment"]["median"] / result["bytes_only_us"]
    result["achieved_TBps"] = 1e-12 * units * (bytes_in + bytes_out) / (1e-6 * result["kernel_us"]["keepout_augment"]["median"])
    solver.close()

    if not args.no_solve:
        common = dict(X_ref=prob["X_ref"], U_ref=prob["U_ref"], X_prev=prob["X_prev"], U_prev=prob["U_prev"], u_l=prob["u_l"], u_u=prob["u_u"], reg_x=prob["reg_x"],
                      reg_u=prob["reg_u"], solver_settings=dict(solver="osqp", Nc=1), max_it=args.iterations, res_tol=0.0, verbose=False)
        versions = {"without": {}, "with": dict(builtin_cstr=cstr), "library": None}
        lib_run = library_leg(prob, args.model, cstr, args.iterations)
        t = {k: [] for k in versions}
        info = {}
        for rep in range(args.solves + 2):
            for k, extra in versions.items():
                if k == "library":
                    t0 = time.perf_counter()
                    Xl, infos = lib_run()
                    t1 = time.perf_counter()
                    if Xl is None:
                        info[k] = dict(failed=True)
                        continue
                    if rep >= 2:
                        t[k].append(1e3 * (t1 - t0) / args.iterations)
                    c, r = cstr["centres"], cstr["radius"]
                    info[k] = dict(fast_path=[int(i["fast_path"]) for i in infos], active_set_rounds=[int(i["active_set_rounds"]) for i in infos],
                                   ipm_iters=[int(i["ipm_iters"]) for i in infos], clearance=float((np.linalg.norm(Xl[:, :, None, :pos_dim] - c, axis=-1) - r).min()))
                    continue
                t0 = time.perf_counter()
                X, U, data = pmpc_amd.solve(None, prob["Q"], prob["R"], prob["x0"], device="cuda", builtin_model=args.model, params=prob["params"], **extra, **common)
                t1 = time.perf_counter()
                if X is None:  # (a sub-problem failed: say so, keep the kernel numbers)
                    info[k] = dict(failed=True)
                    continue
                if rep >= 2:
                    t[k].append(1e3 * (t1 - t0) / len(data["hist"]))
                info[k] = dict(fast_path=[int(s["fast_path"]) for s in data["solver_data"]], active_set_rounds=[int(s["active_set_rounds"]) for s in data["solver_data"]],
                               ipm_iters=[int(s["ipm_iters"]) for s in data["solver_data"]], t_aff_solve_ms=[1e3 * v for v in data["t_aff_solve"]])
                if k == "with":
                    c, r = cstr["centres"], cstr["radius"]
                    info[k]["clearance"] = float((np.linalg.norm(X[:, 1:, None, :pos_dim] - c, axis=-1) - r).min())
        result["iteration_ms"] = {k: _stats(v) for k, v in t.items() if v}
        if "with" in result["iteration_ms"] and "without" in result["iteration_ms"]:
            result["slowdown"] = result["iteration_ms"]["with"]["median"] / result["iteration_ms"]["without"]["median"]
        if "with" in result["iteration_ms"] and "library" in result["iteration_ms"]:
            result["library_over_python_driven"] = result["iteration_ms"]["library"]["median"] / result["iteration_ms"]["with"]["median"]
        result["solver_info"] = info
    print(json.dumps(result))


if __name__ == "__main__":
    main()
