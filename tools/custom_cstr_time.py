#!/usr/bin/env python
"""What a custom state constraint costs next to the built-in keep-out constraint it can restate: the price of NOT fusing the rows into the
augmentation (the built-in `k_keepout_augment` forms the K directions in LDS; a `pmpc_amd.CustomConstraint` writes K (x + 1) doubles per
(particle, stage) — a and h — to a scratch that `k_rows_augment` reads back: two launches where keep-out has one).  The numbers of
CHANGELOG.md's custom-constraint entry come from here.

    python tools/custom_cstr_time.py --model bicycle --M 256 --N 30 --K 2
    python tools/custom_cstr_time.py --model quadrotor --M 4096 --N 50 --K 1      # config D's size

Both versions carry the same K balls per particle beside the start plan (the rollout of the problem's start controls), the custom one as
g_k = r_k - |x[pos] - c_k| with the centres and radii as parameters, and are checked to agree before the figures are reported.  A context
per version; the versions alternate repeat by repeat; times are a host clock around library-loop calls that end with a device->host read;
reported: median, min, max per version (3 timed repeats by default, after one untimed) and the median of the paired differences.
`kernel_us`: HIP events around single launches of the keep-out augmentation, the custom rows kernel and the dense-row augmentation,
alternating in one loop, all warmed first.  Prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

# K balls in x[0 .. BALL_PD-1] (a macro in front); p = [centres (K BALL_PD) | radii (K)]
BALLS_SRC = """
template <class T>
__device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g) {
  for (int k = 0; k < KD; k++) {
    T s = 0.0;
    for (int q = 0; q < BALL_PD; q++) {
      const T d = x[q] - p[k * BALL_PD + q];
      s += d * d;
    }
    g[k] = p[KD * BALL_PD + k] - sqrt(s);
  }
}
"""


def _stats(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def constraints(model, prob, K):
    """(keep-out dict, custom dict, clearance of the start plan) of the same K balls of radius 0.2 per particle, 0.3 from the start plan's
    position at K stages spread over the horizon (to the side of the path in the plane, above it in space)."""
    import pmpc_amd

    pd, x = (3, 12) if model == "quadrotor" else (2, 4)
    M, N = prob["X_prev"].shape[:2]
    P = prob["X_prev"][..., :pd]
    cen = np.zeros((M, K, pd))
    for k in range(K):
        j = min(N - 2, max(1, (k + 1) * N // (K + 1)))
        off = np.zeros((M, pd))
        if pd == 3:
            off[:, 2] = 0.3
        else:
            t = P[:, j + 1] - P[:, j - 1]
            nrm = np.linalg.norm(t, axis=-1, keepdims=True)
            t = np.where(nrm > 1e-9, t / np.maximum(nrm, 1e-9), np.array([1.0, 0.0]))
            off = 0.3 * (1 - 2 * (k % 2)) * np.stack([-t[:, 1], t[:, 0]], -1)
        cen[:, k] = P[:, j] + off
    rad = np.full(K, 0.2)
    clear = float((np.linalg.norm(P[:, :, None, :] - cen[:, None], axis=-1) - rad).min())
    keepout = dict(kind="keepout", pos_idx=tuple(range(pd)), centres=np.ascontiguousarray(np.broadcast_to(cen[:, None], (M, N, K, pd))), radius=rad)
    cc = pmpc_amd.CustomConstraint(f"#define BALL_PD {pd}\n" + BALLS_SRC, x, K, K * pd + K, name=f"balls_{pd}d_K{K}")
    params = np.concatenate([cen.reshape(M, K * pd), np.broadcast_to(rad[None], (M, K))], -1)
    return keepout, dict(kind="custom", cstr=cc, params=params), clear


def kernel_times(s, p, lin, hk, hc, reps=30):
    """HIP events around single launches, on the solver's stream: the keep-out augmentation; the rows kernel; the dense-row augmentation."""
    import torch

    from pmpc_amd.device_problem import keepout_buffers

    K = hk[0].K
    M, N, x = p.X_prev.shape
    dev = p.X_prev.device
    out_k, out_c = keepout_buffers(p, K, sets=1)["sets"][0], keepout_buffers(p, K, sets=1)["sets"][0]
    a, h = torch.empty((M, N, K, x), dtype=torch.float64, device=dev), torch.empty((M, N, K), dtype=torch.float64, device=dev)
    f, fx, fu = lin
    jobs = {
        "keepout_augment": lambda: s.keepout_augment(hk, p.X_prev, f, fx, fu, X_ref=p.X_ref, out=out_k, wait_current_stream=False),
        "custom_rows": lambda: s.custom_cstr_rows(hc[0].id, p.X_prev, hc[1][0], a=a, h=h, wait_current_stream=False),
        "rows_augment": lambda: s.rows_augment(a, h, p.X_prev, f, fx, fu, X_ref=p.X_ref, out=out_c, wait_current_stream=False),
    }
    t = {k: [] for k in jobs}
    torch.cuda.synchronize()
    with torch.cuda.stream(s.stream):
        for rep in range(reps + 5):
            for k, job in jobs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                job()
                e1.record()
                e1.synchronize()
                if rep >= 5:
                    t[k].append(1e3 * e0.elapsed_time(e1))
    agree = max(float((out_k[k] - out_c[k]).abs().max()) for k in ("f", "fx", "fu", "X_prev", "X_ref"))
    agree = max(agree, float((out_k["xu"][..., x:] - out_c["xu"][..., x:]).abs().max()))
    return {k: _stats(v) for k, v in t.items()}, agree


def time_loops(args, prob, keepout, custom):
    """The library loop from the problem's start iterate, `--iterations` iterations per call, a context per version, alternating."""
    import torch

    from pmpc_amd.device import DeviceSolver
    from pmpc_amd.device_problem import build_problem, keepout_buffers

    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    legs = {}
    for name, cstr in (("keepout", keepout), ("custom", custom)):
        s = DeviceSolver(0)
        p = build_problem(prob["Q"], prob["R"], prob["x0"], prob["X_ref"], prob["U_ref"], prob["X_prev"], prob["U_prev"], None, None, prob["u_l"], prob["u_u"],
                          prob["reg_x"], prob["reg_u"], None, None, dict(solver="osqp", Nc=1), None, args.model, prob["params"], "cuda")
        M, N, x, u = p.M, p.N, p.xdim, p.udim
        handle = s.prepare_cstr(cstr, M, N, x)
        legs[name] = dict(s=s, p=p, handle=handle, aug=keepout_buffers(p, handle[0].K), X0=p.X_prev.clone(), U0=p.U_prev.clone(), t=[],
                          bufs=[mk(M, N, x), mk(M, N, x, x), mk(M, N, u, x), mk(M, N, x), mk(M, N, x, x), mk(M, N, u, x)], out=[mk(M, N, x), mk(M, N, u)])
    result = {}
    lc = legs["custom"]
    lin = lc["s"].linearize(lc["p"].model, lc["p"].x0, lc["p"].X_prev, lc["p"].U_prev, lc["p"].params)
    hk = lc["s"].prepare_cstr(keepout, lc["p"].M, lc["p"].N, lc["p"].xdim)
    result["kernel_us"], result["kernel_agree_max_abs"] = kernel_times(lc["s"], lc["p"], lin, hk, lc["handle"])

    def run(leg):
        s, p, b, (Xb, Ub) = leg["s"], leg["p"], leg["bufs"], leg["out"]
        p.X_prev.copy_(leg["X0"])
        p.U_prev.copy_(leg["U0"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res, infos, last, done = s.scp_loop(p.model, p.params, args.iterations, f=b[0], fx=b[1], fu=b[2], f2=b[3], fx2=b[4], fu2=b[5], X_prev=p.X_prev,
                                            U_prev=p.U_prev, X_out=Xb, U_out=Ub, X_ref=p.X_ref, U_ref=p.U_ref, first_cold=True, cstr=leg["handle"],
                                            aug=leg["aug"], wait_current_stream=False, **p.solve_kw())
        r = res.cpu().numpy()  # (synchronises)
        dt = time.perf_counter() - t0
        if done != args.iterations or any(i["status"] != 0 for i in infos):
            raise SystemExit(f"the loop stopped after {done} of {args.iterations} iterations: {infos[-1]}")
        return 1e3 * dt / args.iterations, r, (Xb if last else p.X_prev)

    for rep in range(args.warmup + args.repeats):
        outs = {}
        for name in (("keepout", "custom") if rep % 2 == 0 else ("custom", "keepout")):
            ms, r, X = run(legs[name])
            outs[name] = (r, X.clone())
            if rep >= args.warmup:
                legs[name]["t"].append(ms)
        result["agree_max_abs_X"] = float((outs["keepout"][1] - outs["custom"][1]).abs().max())
        result["agree_max_abs_resid"] = float(np.abs(outs["keepout"][0] - outs["custom"][0]).max())
    result["iteration_ms"] = {k: _stats(v["t"]) for k, v in legs.items()}
    result["paired_difference_ms"] = _stats(np.array(legs["custom"]["t"]) - np.array(legs["keepout"]["t"]))
    result["ratio_of_medians"] = result["iteration_ms"]["custom"]["median"] / result["iteration_ms"]["keepout"]["median"]
    for leg in legs.values():
        leg["s"].close()
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="bicycle", choices=["quadrotor", "bicycle"])
    ap.add_argument("--M", type=int, default=256)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--K", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=10, help="SCP iterations per loop call")
    ap.add_argument("--repeats", type=int, default=3, help="timed loop calls per version")
    ap.add_argument("--warmup", type=int, default=1, help="untimed repeats first")
    args = ap.parse_args()

    from pmpc_amd import dynamics as dyn

    prob = getattr(dyn, f"make_{args.model}_problem")(M=args.M, N=args.N, Nc=1)
    prob["X_prev"] = dyn.rollout(args.model, prob["x0"], prob["U_prev"], prob["params"])  # a dynamically feasible start plan
    keepout, custom, clear = constraints(args.model, prob, args.K)
    if clear <= 0.0:
        raise SystemExit(f"the start plan is inside a ball (clearance {clear}): the first sub-problem would not be feasible by construction")
    t0 = time.perf_counter()
    custom["cstr"].compile()
    result = dict(model=args.model, M=args.M, N=args.N, K=args.K, iterations=args.iterations, repeats=args.repeats, start_clearance=clear,
                  compile_ms=1e3 * (time.perf_counter() - t0))
    result.update(time_loops(args, prob, keepout, custom))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
