"""Compact Jacobian records inside the library's SCP loop (pmpc_amd/csrc/jac_compact.h): they hold exactly the dense
linearisation, and a loop that uses them walks exactly the iterates of a loop that does not."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("model", ["unicycle", "quadrotor"])
@pytest.mark.parametrize("M,N", [(37, 11), (3, 1), (130, 50)])
def test_expanded_compact_records_equal_the_dense_linearisation(model, M, N):
    """Both orientations of the records (the factor sweep's column triples, the forward sweep's row triples) and the per-particle
    constant pool, expanded by k_expand_jac, against pmpc_linearize_device: exact equality, random states, every particle with
    parameters of its own."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import MODEL_QUADROTOR, MODEL_UNICYCLE, DeviceSolver, to_device_problem

    rng = np.random.default_rng(3)
    prob = dyn.make_unicycle_problem(M=M, N=N) if model == "unicycle" else dyn.make_quadrotor_problem(M=M, N=N)
    mid = MODEL_UNICYCLE if model == "unicycle" else MODEL_QUADROTOR
    prob["X_prev"] = prob["X_prev"] + 0.3 * rng.standard_normal(prob["X_prev"].shape)
    dU = 0.3 * rng.standard_normal(prob["U_prev"].shape)
    if model == "unicycle":
        dU = np.sign(dU) * (0.1 + np.abs(dU))
    prob["U_prev"] = prob["U_prev"] + dU
    d = to_device_problem(prob)
    x, u = d["X_prev"].shape[-1], d["U_prev"].shape[-1]
    s = DeviceSolver(0)
    try:
        f, fx, fu = s.linearize(mid, d["x0"], d["X_prev"], d["U_prev"], d["params"])
        fc, jc = s.linearize_compact(mid, d["x0"], d["X_prev"], d["U_prev"], d["params"])
        s.sync()
        assert jc.numel() < fx.numel() + fu.numel()
        assert torch.equal(f, fc)
        for orient in (0, 1):
            ex, eu = s.expand_jac(mid, jc, M, N, x, u, orient)
            s.sync()
            assert torch.equal(ex, fx), (orient, (ex != fx).nonzero()[:5])
            assert torch.equal(eu, fu), (orient, (eu != fu).nonzero()[:5])
    finally:
        s.close()


_CHILD = r"""
import json, sys
import numpy as np
import torch
from pmpc_amd import dynamics as dyn
from pmpc_amd.device import MODEL_QUADROTOR, MODEL_UNICYCLE, DeviceSolver, to_device_problem

case, out = sys.argv[1], sys.argv[2]
kw = {}
if case == "unicycle":
    prob, mid = dyn.make_unicycle_problem(M=48, N=20, Nc=1), MODEL_UNICYCLE
elif case == "quadrotor":
    prob, mid = dyn.make_quadrotor_problem(M=96, N=30, Nc=1), MODEL_QUADROTOR
else:  # tight boxes: torques that saturate around a jump of the position reference, and velocity limits that bind
    prob, mid = dyn.make_quadrotor_problem(M=96, N=30, Nc=1), MODEL_QUADROTOR
    prob["X_ref"][:, 20:, 0] += 1.5
    prob["u_u"][..., 1:] = 0.05
    prob["u_l"][..., 1:] = -0.05
d = to_device_problem(prob)
M, N, x = d["X_prev"].shape
u = d["U_prev"].shape[-1]
if case == "tight":
    lx = torch.full((M, N, x), -float("inf"), dtype=torch.float64, device="cuda")
    lx[..., 3:6] = -0.6
    kw = dict(lx=lx, ux=-lx)
mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
Xa, Ua, Xb, Ub = d["X_prev"].clone(), d["U_prev"].clone(), mk(M, N, x), mk(M, N, u)
s = DeviceSolver(0)
steps = 8
res, infos, last, done = s.scp_loop(mid, d["params"], steps, f=mk(M, N, x), fx=mk(M, N, x, x), fu=mk(M, N, u, x), f2=mk(M, N, x), fx2=mk(M, N, x, x),
                                    fu2=mk(M, N, u, x), X_prev=Xa, U_prev=Ua, X_out=Xb, U_out=Ub, first_cold=True, Q=d["Q"], R=d["R"], X_ref=d["X_ref"],
                                    U_ref=d["U_ref"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], Nc=1, x0=d["x0"], lu=d["lu"], uu=d["uu"],
                                    symmetric_cost=True, **kw)
s.sync()
X, U = (Xb, Ub) if last else (Xa, Ua)
np.savez(out, X=X.cpu().numpy(), U=U.cpu().numpy(), res=res.cpu().numpy(), done=done, infos=json.dumps(infos))
s.close()
"""


def _loop_in_child(case, compact, tmp_path):
    out = tmp_path / f"{case}_{compact}.npz"
    env = dict(os.environ, PMPC_LIN_COMPACT=str(compact))
    r = subprocess.run([sys.executable, "-c", _CHILD, case, str(out)], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    return z["X"], z["U"], z["res"], int(z["done"]), json.loads(str(z["infos"]))


@pytest.mark.parametrize("case", ["unicycle", "quadrotor", "tight"])
def test_scp_loop_with_and_without_compact_records_walks_the_same_iterates(case, tmp_path):
    """PMPC_LIN_COMPACT=0 / 1 in two fresh processes: identical iterates, residuals and per-iteration infos.  `tight`: boxes tight enough
    that warm solves leave the active-set rounds for the interior-point iteration, so the records are expanded on the way
    (QpSolve::densify, k_expand_jac)."""
    X0, U0, r0, d0, i0 = _loop_in_child(case, 0, tmp_path)
    X1, U1, r1, d1, i1 = _loop_in_child(case, 1, tmp_path)
    print(case, [(i["ipm_iters"], i["active_set_rounds"], i["structured_solves"]) for i in i1])
    assert d0 == d1 == 8 and all(i["status"] == 0 for i in i1)
    assert i0 == i1
    np.testing.assert_array_equal(r0, r1)
    np.testing.assert_array_equal(X0, X1)
    np.testing.assert_array_equal(U0, U1)
    assert sum(i["active_set_rounds"] for i in i1[1:]) > 0  # the warm solves did run the rounds whose sweeps read the records
    if case == "tight":
        assert any(i["ipm_iters"] > 0 for i in i1[1:]), i1  # ... and at least one of them handed over to the interior-point iteration
