"""Device-resident SCP loop: `scp_solve` (pmpc/scp_mpc.py:205-442) with every array kept in HBM.

    X, U, data = pmpc_amd.solve(f_fx_fu_fn, Q, R, x0, ..., device="cuda")

`f_fx_fu_fn(X_, U_prev)` receives float64 torch tensors on the GPU (`X_ = [x0, X_prev[:-1]]`, the reference's
contract, README.md:136-145 / scp_mpc.py:338-342) and returns `f (M,N,x)`, `fx (M,N,x,x)`, `fu (M,N,x,u)` as torch GPU
tensors in the usual (row, col) layout — or already in the ABI layout `(M,N,col,row)` with `jacobians_abi_layout=True`,
which saves one transposing copy of the Jacobian stacks per iteration.  A built-in model (`builtin_model="unicycle" |
"quadrotor" | "bicycle"`, `params=...`) is linearised by the HIP kernel of csrc/dynamics.hip instead of a Python callable, and a
`pmpc_amd.CustomModel` given there by the kernel compiled at run time from the user's device code (csrc/model_jit.hip).
Nothing crosses PCIe inside the loop except the scalars of the `hist` row (one small read per SCP iteration); a built-in cost's
descriptor is uploaded once before the loop, and the shifts' counter of refused blocks is read once after it.

`solver_settings["extra_cstrs"]` in the reference's tuple format is accepted for that case (pmpc_amd/extra_cstrs.py).
`soc=dict(W=(q,u), w0=(q,), v=(u,), v0=float, u_interior=(u,))` adds the stage-wise second-order cone
`||W u + w0|| <= v'u + v0` on every stage's controls (thrust cones; `DeviceSolver.lsoc_solve`).

`lin_cost_fn(X_prev, U_prev, problems)` (pmpc/scp_mpc.py:171-185) receives float64 GPU tensors and returns the cost gradients
`(cx, cu)`, each a GPU tensor or None; the iteration then tracks `X_ref - Q^-1 cx`, `U_ref - R^-1 cu` (`DeviceSolver.ref_shift`, a HIP
kernel; `Q` / `R` must be symmetric), while the `obj` column keeps the caller's references, as upstream (:404).
`builtin_cost=dict(kind="obstacles", pos_idx=..., centres=..., sigma=..., w=...)` is the built-in obstacle cost
(`pmpc_amd.dynamics.obstacle_cost`), evaluated and applied in one launch.  `builtin_cost=dict(kind="custom", cost=pmpc_amd.CustomCost,
params=(M, pdim))` is the user's own stage cost, compiled at run time (csrc/cost_jit.hip): `DeviceSolver.custom_cost_grad` gives
`(cx, cu)`, then `ref_shift` on `Q` and — unless the cost has `uses_u=False` — on `R`.

`builtin_cstr=dict(kind="keepout", pos_idx=..., centres=..., radius=...)` is the built-in keep-out constraint: every stage of every
particle stays outside 1 to 4 balls in the position sub-space `pos_idx` (centres `(K, pos_dim)`, `(N, K, pos_dim)` moving, or
`(M, N, K, pos_dim)` per particle).  Every iteration convexifies it about X_prev into half-spaces (`pmpc_amd.extra_cstrs.keepout_rows`)
and restates them as upper bounds on K auxiliary states (`DeviceSolver.keepout_augment`, a HIP kernel): the sub-problem runs at
`xdim + K` states, the loop sees `xdim`.  The host loop's equivalent is `extra_cstrs_fns=make_keepout_extra_cstrs_fn(...)`.  Refused
next to it: a stage cone (`soc=` / `extra_cstrs`), slew penalties, `smooth_cstr="squareplus"`, a sharded context, fp32 Jacobians.
`builtin_cstr=dict(kind="custom", cstr=pmpc_amd.CustomConstraint, params=(M, pdim))` is the user's own state constraint g(x) <= 0, compiled
at run time (csrc/cstr_jit.hip): `DeviceSolver.custom_cstr_rows` gives the rows about X_prev, `DeviceSolver.rows_augment` (a HIP kernel)
restates them the same way; the same refusals hold, and a row whose value or gradient is not finite at an iterate is a `ValueError`.
The host loop's equivalent is `extra_cstrs_fns=make_rows_extra_cstrs_fn(g_fn, jac_fn)`.

Host-only features of the reference loop that need the sub-problem on the host (`extra_cstrs_fns`, filters, `solver_state`) are
not offered here; `pmpc_amd.scp_mpc.scp_solve` (the default) has them.

The arguments become a `DeviceProblem` (pmpc_amd/device_problem.py `build_problem`, shared with `MPCController`) before the loop.
"""
from __future__ import annotations

import math
import time
from typing import Any, Callable, Dict, Optional

import numpy as np
import torch

from .custom_constraint import check_cstr_dict, is_custom as is_custom_cstr
from .custom_cost import is_custom
from .custom_model import CustomModel
from .device import DeviceSolver
from .device_problem import build_problem, keepout_buffers
from .utils import TablePrinter

_solvers: Dict[int, DeviceSolver] = {}


def _solver_for(device: torch.device) -> DeviceSolver:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _solvers:
        _solvers[idx] = DeviceSolver(idx)
    return _solvers[idx]


def _refuse_with_cstr(settings=None, soc=None, slew_rate=None, u0_slew=None, solver=None, jac_dtype=None):
    """The combinations `builtin_cstr` is refused in, each with its reason.  The first three are the cases `backend.aff_solve` refuses for
    rows on the states (the keep-out rows are such rows), for the same reasons."""
    settings = settings or {}
    if soc is not None or settings.get("extra_cstrs"):
        raise ValueError("builtin_cstr: rows on the states together with cones on the controls (soc= / extra_cstrs) are not supported in one solve")
    if (slew_rate is not None and float(slew_rate) != 0.0) or u0_slew is not None or "slew_reg" in settings:
        raise ValueError("builtin_cstr: rows on the states are not supported together with slew penalties")
    if str(settings.get("smooth_cstr", "")).lower() == "squareplus":
        raise ValueError('builtin_cstr: rows on the states together with smooth_cstr="squareplus" are not supported (the reference keeps '
                         "extra_cstrs rows hard there; restated as state boxes they would be softened with the boxes)")
    if solver is not None and getattr(solver, "world", 1) > 1:
        raise ValueError("builtin_cstr: a sharded context (comm_world > 1) is not supported")
    if jac_dtype is not None and jac_dtype != torch.float64:
        raise ValueError(f"builtin_cstr: fp32 storage of the Jacobians ({jac_dtype}) is not supported (the augmentation kernel is fp64)")


def scp_solve_device(f_fx_fu_fn: Optional[Callable], Q, R, x0, X_ref=None, U_ref=None, X_prev=None, U_prev=None, x_l=None,
                     x_u=None, u_l=None, u_u=None, verbose: bool = False, max_it: int = 100, time_limit: float = 1000.0,
                     res_tol: float = 1e-5, reg_x: float = 1e0, reg_u: float = 1e-2, slew_rate: Optional[float] = None,
                     u0_slew=None, solver_settings: Optional[Dict[str, Any]] = None, device="cuda",
                     jacobians_abi_layout: bool = False, builtin_model=None, params=None,
                     return_torch: bool = False, solver: Optional[DeviceSolver] = None, soc: Optional[Dict[str, Any]] = None,
                     lin_cost_fn=None, builtin_cost: Optional[Dict[str, Any]] = None, cost_fn=None,
                     extra_cstrs_fns=None, solver_state=None, filter_method: str = "", debug: bool = False,
                     return_min_viol: bool = False, builtin_cstr: Optional[Dict[str, Any]] = None, **ignored):
    host_only = dict(cost_fn=cost_fn, extra_cstrs_fns=extra_cstrs_fns, solver_state=solver_state,
                     filter_method=filter_method or None, debug=debug or None, return_min_viol=return_min_viol or None)
    bad = [k for k, v in host_only.items() if v is not None]
    if bad:
        raise ValueError(f"scp_solve(device=...) does not support {bad}; use the host loop (device=None)")
    if builtin_cstr is not None:
        _refuse_with_cstr(solver_settings, soc, slew_rate, u0_slew, solver)
        if is_custom_cstr(builtin_cstr):  # dimensions and params that are not the problem's: before any device is touched
            qs = tuple(Q.shape) if hasattr(Q, "shape") else np.shape(Q)
            check_cstr_dict(builtin_cstr, qs[0] if len(qs) == 4 else 1, qs[-1])
    dev = torch.device(device)
    t_start = time.time()
    with_costs = lin_cost_fn is not None or builtin_cost is not None
    p = build_problem(Q, R, x0, X_ref, U_ref, X_prev, U_prev, x_l, x_u, u_l, u_u, reg_x, reg_u, slew_rate, u0_slew, solver_settings, soc,
                      builtin_model, params, dev, need_sym="lin_cost_fn / builtin_cost need" if with_costs else None, builtin_cost=builtin_cost)
    M, N, xdim, udim, single = p.M, p.N, p.xdim, p.udim, p.single
    X_prev, U_prev = p.X_prev, p.U_prev
    T = lambda z: torch.as_tensor(z, dtype=torch.float64, device=dev)  # (lin_cost_fn's gradients)
    s = solver or _solver_for(dev)
    model = s.load_model(p.model) if isinstance(p.model, CustomModel) else p.model  # (a custom model: compiled and loaded once per solver)
    Xs = torch.empty((M, N, xdim), dtype=torch.float64, device=dev)
    Us = torch.empty((M, N, udim), dtype=torch.float64, device=dev)
    static_kw = dict(p.solve_kw(), slew_reg0=p.slew0, slew_um1=p.um1, X_out=Xs, U_out=Us, verbose=p.solver_verbose)

    data: Dict[str, Any] = dict(solver_data=[], hist=[], t_aff_solve=[])
    fields = ["it", "elaps", "obj", "resid", "reg_x", "reg_u"]
    tp = TablePrinter(fields, fmts=["%04d"] + ["%8.3e"] * 5)
    if verbose:
        print(tp.make_header())
    # the built-in cost's descriptor and device arrays: made once, before the loop (nothing of it is uploaded inside)
    cost_handle = s.prepare_cost(builtin_cost, N, xdim, dev, M=M, u=udim) if builtin_cost is not None else None
    custom_cost = is_custom(builtin_cost)
    # the built-in constraint: descriptor, the augmented buffers and the parts of the augmented problem that do not change with the
    # iterate (Q~, x0~, the lower bounds, the first xdim upper bounds) — made once, before the loop
    if builtin_cstr is not None:
        _refuse_with_cstr(solver=s)
        cstr_handle = s.prepare_cstr(builtin_cstr, M, N, xdim, dev)
        custom_cstr = cstr_handle[0].kind == 2
        static = keepout_buffers(p, cstr_handle[0].K, sets=1)  # (one set: nothing of the next iteration is enqueued behind this loop's solves)
        aug, Xs_aug = static["sets"][0], static["X_out"]
    it, max_res = 0, math.inf
    s.stream.wait_stream(torch.cuda.current_stream(dev))  # the set-up above ran on the caller's stream
    while it < max_it:
        if model is not None:
            f, fxa, fua = s.linearize(model, p.x0, X_prev, U_prev, p.params)
        else:
            X_lin = torch.cat([p.x0[:, None, :], X_prev[:, :-1, :]], 1)
            f, fx, fu = f_fx_fu_fn(X_lin if not single else X_lin[0], U_prev if not single else U_prev[0])
            f = f.reshape(M, N, xdim).contiguous()
            if jacobians_abi_layout:
                fxa, fua = fx.reshape(M, N, xdim, xdim).contiguous(), fu.reshape(M, N, udim, xdim).contiguous()
            else:
                fxa = fx.reshape(M, N, xdim, xdim).transpose(-1, -2).contiguous()
                fua = fu.reshape(M, N, xdim, udim).transpose(-1, -2).contiguous()
        # linearised costs (scp_mpc.py:171-185, 352): this iteration's references; X_ref / U_ref stay as they are for the `obj` column
        X_ref_, U_ref_ = p.X_ref, p.U_ref
        if custom_cost:
            cx, cu = s.custom_cost_grad(cost_handle[0].id, X_prev, U_prev, cost_handle[1][0])
            X_ref_ = s.ref_shift(p.Qa, cx, X_ref_, check=False)
            if cu is not None:
                U_ref_ = s.ref_shift(p.Ra, cu, U_ref_, check=False)
        elif builtin_cost is not None:
            X_ref_ = s.obstacle_cost_grad(X_prev, cost_handle, Q=p.Qa, X_ref=X_ref_, check=False)
        if lin_cost_fn is not None:
            problems = dict(ignored, f=f, fx=fxa, fu=fua, x0=p.x0, X_prev=X_prev, U_prev=U_prev, Q=p.Q, R=p.R, X_ref=p.X_ref, U_ref=p.U_ref,
                            x_l=p.lx, x_u=p.ux, u_l=p.lu, u_u=p.uu, slew_rate=slew_rate, u0_slew=u0_slew, jacobians_abi_layout=True)
            cx, cu = lin_cost_fn(X_prev if not single else X_prev[0], U_prev if not single else U_prev[0], problems)
            if cx is not None:
                X_ref_ = s.ref_shift(p.Qa, T(cx).reshape(M, N, xdim).contiguous(), X_ref_, check=False)
            if cu is not None:
                U_ref_ = s.ref_shift(p.Ra, T(cu).reshape(M, N, udim).contiguous(), U_ref_, check=False)
        t_aff = time.time()
        kw = dict(static_kw, f=f, fx=fxa, fu=fua, X_prev=X_prev, U_prev=U_prev, X_ref=X_ref_, U_ref=U_ref_,
                  static_cons_bounds=it > 0,  # the boxes are the same in every iteration of this loop (scp_mpc.py:338-376)
                  prev_is_last_solution=it > 0)  # and X_prev, U_prev are the previous iteration's X, U (scp_mpc.py:430)
        if builtin_cstr is not None:
            _refuse_with_cstr(jac_dtype=fxa.dtype)
            # the keep-out rows about X_prev as bounds on K auxiliary states; the solve runs at xdim + K states.  prev_is_last_solution
            # stays off: X_prev~ holds zeros where the previous output holds the rows' values, so the flag's promise (X_prev is the
            # previous solve's output) does not hold for the augmented arrays
            if custom_cstr:
                rows_a, rows_h = s.custom_cstr_rows(cstr_handle[0].id, X_prev, cstr_handle[1][0])
                s.rows_augment(rows_a, rows_h, X_prev, f, fxa, fua, X_ref=X_ref_, out=aug)
            else:
                s.keepout_augment(cstr_handle, X_prev, f, fxa, fua, X_ref=X_ref_, out=aug)
            kw.update(f=aug["f"], fx=aug["fx"], fu=aug["fu"], X_prev=aug["X_prev"], X_ref=aug["X_ref"], Q=static["Qa"], x0=static["x0"], lx=static["lx"],
                      ux=aug["xu"], X_out=Xs_aug, prev_is_last_solution=False)
        if p.soc_kw:
            _, _, status = s.lsoc_solve(**p.soc_kw, **kw)
        elif p.cone:
            _, _, status = s.lcone_solve(smooth_alpha=p.smooth_alpha, **kw)
        else:
            _, _, status = s.lqp_solve(**kw)
        with torch.cuda.stream(s.stream):  # residual / objective row of scp_mpc.py:397-405 on the solver's stream
            if builtin_cstr is not None:
                Xs.copy_(Xs_aug[..., :xdim])  # strip the auxiliary states
            res = s.scp_residual(Xs, X_prev, Us, U_prev)[0]
            eX, eU = Xs - p.X_ref, Us - p.U_ref
            obj = (torch.sum(eX * torch.einsum("mnrt,mnt->mnr", p.Q, eX)) + torch.sum(eU * torch.einsum("mnrt,mnt->mnr", p.R, eU))) / N / M
            row = torch.stack([res, obj]).cpu()  # the only device->host read of the iteration (synchronises the stream)
            X_prev, U_prev = Xs.clone(), Us.clone()
        torch.cuda.current_stream(dev).wait_stream(s.stream)
        t_aff = time.time() - t_aff
        if status != 0 or not bool(torch.isfinite(row).all()):  # solver failure (:391-394)
            if with_costs:  # ... which a Q / R block that is not positive definite causes (NaN references): say so
                s.check_bad_pivots("lin_cost_fn / builtin_cost: Q or R")
            if builtin_cstr is not None and custom_cstr:
                s.check_bad_rows("builtin_cstr")
            if verbose:
                print("Solver failed...")
            return None, None, None
        max_res, obj_v = float(row[0]), float(row[1])
        vals = (it + 1, time.time() - t_start, obj_v, max_res, float(reg_x), float(reg_u))
        if verbose:
            print(tp.make_values(vals))
        data["hist"].append(dict(zip(fields, vals)))
        data["solver_data"].append(dict(s.last_info))
        data["t_aff_solve"].append(t_aff)
        if max_res < res_tol:
            break
        it += 1
        if (time.time() - t_start) * (it + 1) / it > time_limit:
            break
    if verbose:
        print(tp.make_footer())
    if with_costs:  # the shifts' device-side counter of refused blocks: read once, after the loop
        s.check_bad_pivots("lin_cost_fn / builtin_cost: Q or R")
    if builtin_cstr is not None and custom_cstr:  # likewise the rows kernel's counter of rows it had to drop
        s.check_bad_rows("builtin_cstr")
    X = torch.cat([p.x0[:, None, :], X_prev], 1)
    U = U_prev
    if single:
        X, U = X[0], U[0]
    if return_torch:
        return X, U, data
    return X.cpu().numpy(), U.cpu().numpy(), data
