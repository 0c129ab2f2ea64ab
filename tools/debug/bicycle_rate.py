"""SCP iterations/s of the library's loop on the kinematic bicycle (built-in model 2), lane-change problem of
pmpc_amd.dynamics.make_bicycle_problem.  Run it twice, with PMPC_LIN_COMPACT=1 (default) and =0, to see what the compact Jacobian
records are worth for this model:  python tools/debug/bicycle_rate.py [--M 4096] [--N 50] [--Nc 1] [--steps 20] [--warmup 3] [--windows 5]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import torch  # noqa: E402

from pmpc_amd import dynamics as dyn  # noqa: E402
from pmpc_amd.device import MODEL_BICYCLE, DeviceSolver, to_device_problem  # noqa: E402

ap = argparse.ArgumentParser()
for k, v in (("M", 4096), ("N", 50), ("Nc", 1), ("steps", 20), ("warmup", 3), ("windows", 5)):
    ap.add_argument("--" + k, type=int, default=v)
a = ap.parse_args()
prob = dyn.make_bicycle_problem(M=a.M, N=a.N, Nc=a.Nc)
d = to_device_problem(prob)
M, N, x = d["X_prev"].shape
u = d["U_prev"].shape[-1]
mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
bufs = dict(f=mk(M, N, x), fx=mk(M, N, x, x), fu=mk(M, N, u, x), f2=mk(M, N, x), fx2=mk(M, N, x, x), fu2=mk(M, N, u, x))
common = dict(Q=d["Q"], R=d["R"], X_ref=d["X_ref"], U_ref=d["U_ref"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=a.Nc, x0=d["x0"], lu=d["lu"], uu=d["uu"],
              symmetric_cost=True)
s = DeviceSolver(0)
rates, infos = [], []
for w in range(a.windows):  # every window: the same loop from the same start iterate (warm-up iterations untimed)
    Xa, Ua, Xb, Ub = d["X_prev"].clone(), d["U_prev"].clone(), mk(M, N, x), mk(M, N, u)
    _, _, last, done = s.scp_loop(MODEL_BICYCLE, d["params"], a.warmup, X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, first_cold=True, **bufs, **common)
    assert done == a.warmup
    if last:
        Xa, Ua, Xb, Ub = Xb, Ub, Xa, Ua
    s.sync()
    t0 = time.perf_counter()
    res, infos, last, done = s.scp_loop(MODEL_BICYCLE, d["params"], a.steps, X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, first_cold=False, **bufs, **common)
    s.sync()
    dt = time.perf_counter() - t0
    assert done == a.steps and all(i["status"] == 0 for i in infos), infos
    rates.append(a.steps / dt)
rates.sort()
print(json.dumps(dict(model="bicycle", M=M, N=N, Nc=a.Nc, steps=a.steps, lin_compact=os.environ.get("PMPC_LIN_COMPACT", "1"),
                      it_per_s_median=rates[len(rates) // 2], it_per_s_min=rates[0], it_per_s_max=rates[-1],
                      last_window=[(i["ipm_iters"], i["active_set_rounds"]) for i in infos], final_residual=float(res[-1]))))
s.close()
