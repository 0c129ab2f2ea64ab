"""Receding-horizon MPC with the problem resident in HBM: `MPCController`.

    ctl = pmpc_amd.MPCController(builtin_model="bicycle", params=P, Q=Q, R=R, X_ref=Xr, U_ref=Ur, u_l=ul, u_u=uu,
                                 reg_x=1.0, reg_u=1e-2, solver_settings=dict(solver="osqp", Nc=1))
    while running:
        u0, info = ctl.step(x0, iterations=3)      # measure x0, shift the plan one stage on, 3 SCP iterations, first control

The constructor uploads the problem once and allocates every buffer of the library's SCP loop (`DeviceSolver.scp_loop`, the loop
bench.py times); a step is one copy of `x0`, one launch of the plan shift (`DeviceSolver.shift_plan`) and one call of the loop — the
host reads the per-iteration statuses, the residuals and the first control, nothing else crosses PCIe.

By default every step's first SCP iteration runs with `first_cold=True`: after a shift the start iterate is not the previous solve's
output, so the no-rollout warm start and the compact Jacobian records begin at the second iteration of each step.

`warm_shift=True` moves the solver's active-set memory along with the plan: behind the plan shift one more launch
(`DeviceSolver.warm_shift`, specification `pmpc_amd.dynamics.shift_active_set`) moves the control-box statuses the previous step's last
solve settled on `shift` stages on, clamps the shifted controls into the boxes of the stages they arrive at (`u_l` / `u_u` do not move
with the horizon) and drops the statuses the new boxes no longer support.  The step's first iteration then runs with `first_cold=False`
and takes the path of the later ones (warm active-set rounds without a rollout, compact Jacobian records, the follow-up enqueued
ahead); `info["warm_shift"]` says whether it did — not on the first step after `reset`, and not after a step whose last solve ended
without an accepted active set (nothing is stored then).  One semantic difference to the default: on the consensus stages (`j < Nc`) the
start iterate, and with it the linearisation point, holds particle 0's shifted control in every particle, clamped into stage j's box
(the solver's shared control has one base value); everywhere else the start controls are the shifted plan's, clamped.  Shifted are the
control-box statuses and the plan's controls only.  The multiplier memories of the stage cones (`cone_z`), the state rows (`xb_z` /
`xb_st`) and the cone objective's epigraph rows are not, so `warm_shift=True` is refused next to the cone objective (`solver` other than
the QP path, `smooth_alpha`), `soc=` / `extra_cstrs`, state boxes `x_l` / `x_u`, slew (`slew_rate`, `slew_reg`; their increment form
restates the controls as states) and `keepout=` (its loop clears the promise the warm start rests on anyway).  `builtin_cost=` (the obstacle
cost, or `dict(kind="custom", cost=pmpc_amd.CustomCost, params=)`, whose parameters `set_cost_params` rewrites in place) is allowed;
without control boxes nothing is stored and every step stays cold.

`constraint=dict(cstr=pmpc_amd.CustomConstraint, params=(M, pdim))` is the user's own state constraint g(x) <= 0 carried the same way
(`set_constraint_params` rewrites its parameters in place); refused next to `keepout=` (the loop carries one constraint) and with what
`keepout=` is refused with, `warm_shift=True` included.  A row whose value or gradient is not finite at an iterate is a `ValueError`.

`keepout=dict(pos_idx=, centres=, radius=)` is the hard keep-out constraint of `solve(..., device=..., builtin_cstr=...)` (1 to 4 balls in the
position sub-space `pos_idx`; centres `(K, pos_dim)`, `(N, K, pos_dim)` per stage or `(M, N, K, pos_dim)` per particle and stage) carried
through the library loop: every sub-problem runs at `xdim + K` states on augmented buffers the constructor allocates once, the plan
stays at `xdim`.  `set_keepout` writes new centres / radii into the resident arrays.  Refused next to it, before a device is touched: a
stage cone (`soc=` / `extra_cstrs`), slew penalties, a sharded context, `xdim + K > 16`.

`builtin_model=` also takes a `pmpc_amd.CustomModel`: the user's own x+ = F(x, u; p) as a short piece of device code, compiled at run
time with automatic differentiation for its Jacobians and loaded on the controller's solver (`DeviceSolver.load_model`); `params` is
then (M, pdim).  Cost, keep-out and `warm_shift` work as with a built-in name; the loop runs on dense Jacobians (no compact records).

Refused with a ValueError (the library loop has no place for them): a Python `f_fx_fu_fn` / `lin_cost_fn` / `cost_fn`, `extra_cstrs_fns`,
filters, `solver_state`, a sharded context, and `solver_settings` keys other than `solver`, `Nc`, `smooth_alpha`, `slew_reg`,
`extra_cstrs`, `soc_u_interior`.  `soc=` / `solver_settings["extra_cstrs"]` (one stage-wise second-order cone) are taken as in
`solve(..., device=...)`; with a stage cone the sub-problem is `lsoc_solve`'s, whatever `solver` says.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Optional

import numpy as np
import torch

from .device import DeviceSolver
from .device_problem import build_problem, keepout_buffers
from .custom_constraint import check_cstr_dict
from .custom_cost import check_cost_dict, is_custom
from .custom_model import CustomModel
from .dynamics import model_id

_SETTINGS = ("solver", "Nc", "smooth_alpha", "slew_reg", "extra_cstrs", "soc_u_interior")


def _refuse_with_warm_shift(settings, soc, x_l, x_u, slew_rate, keepout, constraint=None):
    """`warm_shift=True` moves the control-box statuses and the plan's controls and nothing else: refused next to every feature whose
    solve carries a warm-start memory of its own that stays at the old stages (or that ends the warm first iteration anyway)."""
    from .device_problem import _CONE_SOLVERS

    has = lambda z: z is not None and (z.numel() if torch.is_tensor(z) else np.size(z)) > 0
    why = None
    if str(settings.get("solver", "ecos")).lower() in _CONE_SOLVERS or "smooth_alpha" in settings or "smooth_cstr" in settings:
        why = ("the cone objective (solver_settings['solver'] is not the QP path's, e.g. 'osqp', or smooth_alpha is set): the multipliers of "
               "its epigraph rows are not shifted")
    elif soc is not None or settings.get("extra_cstrs"):
        why = "a stage cone (soc= / extra_cstrs): the cones' multiplier memory (cone_z) is not shifted"
    elif has(x_l) and has(x_u):
        why = "state boxes x_l / x_u: the state rows' statuses and multipliers (xb_st, xb_z) are not shifted"
    elif (slew_rate is not None and float(slew_rate) != 0.0) or "slew_reg" in settings:
        why = "slew penalties (slew_rate, slew_reg): their increment form restates the controls as states, whose rows are not shifted"
    elif keepout is not None:
        why = "keepout=: its rows are state rows (not shifted), and the keep-out loop runs no sub-problem as a no-rollout warm start"
    elif constraint is not None:
        why = "constraint=: its rows are state rows (not shifted), and the constrained loop runs no sub-problem as a no-rollout warm start"
    if why is not None:
        raise ValueError(f"MPCController: warm_shift=True is not supported next to {why}")


class MPCController:
    def __init__(self, builtin_model=None, params=None, Q=None, R=None, X_ref=None, U_ref=None, u_l=None, u_u=None, x_l=None, x_u=None,
                 reg_x: float = 1e0, reg_u: float = 1e-2, solver_settings: Optional[Dict[str, Any]] = None, builtin_cost: Optional[Dict[str, Any]] = None,
                 slew_rate: Optional[float] = None, u0_slew=None, soc: Optional[Dict[str, Any]] = None, device="cuda",
                 solver: Optional[DeviceSolver] = None, keepout: Optional[Dict[str, Any]] = None, warm_shift: bool = False,
                 constraint: Optional[Dict[str, Any]] = None, **unsupported):
        if builtin_model is None:
            raise ValueError("MPCController needs builtin_model=: a Python f_fx_fu_fn cannot enter the library's SCP loop")
        if unsupported.get("builtin_cstr") is not None:
            raise ValueError("MPCController: builtin_cstr is not supported (the controller takes the keep-out constraint as "
                             "keepout=dict(pos_idx=, centres=, radius=); pmpc_amd.solve(..., device=..., builtin_cstr=...) carries it in one solve)")
        bad = [k for k, v in unsupported.items() if v is not None and v != ""]
        if bad:
            raise ValueError(f"MPCController does not support {sorted(bad)}; the host loop pmpc_amd.solve(...) has the host-only features")
        settings = dict(solver_settings or {})
        if warm_shift:  # what the shifted memory does not cover: before any device is touched
            _refuse_with_warm_shift(settings, soc, x_l, x_u, slew_rate, keepout, constraint)
        self.warm_shift = bool(warm_shift)
        if constraint is not None and keepout is not None:
            raise ValueError("MPCController: constraint= is not supported next to keepout= (the loop carries one constraint: a keep-out ball is "
                             "g = r - |x[pos] - c| in a pmpc_amd.CustomConstraint)")
        if keepout is not None or constraint is not None:  # what the constraint is refused with, for scp_device.py's reasons: before any device is touched
            from .scp_device import _refuse_with_cstr

            _refuse_with_cstr(settings, soc, slew_rate, u0_slew, solver)
        bad = [k for k in settings if k not in _SETTINGS]
        if bad:
            raise ValueError(f"MPCController: solver_settings {sorted(bad)} are not taken by the library's SCP loop (taken: {_SETTINGS})")
        if params is None or Q is None or R is None:
            raise ValueError("MPCController needs params=, Q= and R=")
        custom = isinstance(builtin_model, CustomModel)
        self.model = None if custom else model_id(builtin_model)  # (a custom model: the id the solver loads it under, below)
        dev = torch.device(device)
        self.device = dev
        if np.ndim(Q) != 4 or np.ndim(R) != 4:
            raise ValueError("MPCController: Q (M, N, x, x) and R (M, N, u, u)")
        if custom:  # dimensions and params that are not the model's: likewise before any device is touched
            builtin_model.check_problem(np.shape(Q)[0], np.shape(Q)[-1], np.shape(R)[-1], params)
        check_cost_dict(builtin_cost, np.shape(Q)[0], np.shape(Q)[-1], np.shape(R)[-1])  # (a custom cost: likewise)
        if constraint is not None:  # (a custom constraint: likewise)
            constraint = dict(constraint, kind="custom")
            check_cstr_dict(constraint, np.shape(Q)[0], np.shape(Q)[-1])
        if keepout is not None:  # a description the kernels cannot run: likewise before any device is touched
            from .extra_cstrs import _keepout_arrays

            keepout = dict(keepout, kind=keepout.get("kind", "keepout"))
            host = {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in keepout.items()}
            _, _, rad = _keepout_arrays(host, np.shape(Q)[0], np.shape(Q)[1], np.shape(Q)[-1])
            if np.shape(Q)[-1] + len(rad) > 16:
                raise ValueError(f"keep-out constraint: {np.shape(Q)[-1]} states + {len(rad)} auxiliary states exceed the solver's 16")
        if solver is None:
            from .scp_device import _solver_for

            solver = _solver_for(dev)
        if solver.world > 1:
            raise ValueError("MPCController: a sharded context (comm_world > 1) is not supported")
        self.solver = s = solver
        if custom:
            self.model = s.load_model(builtin_model)
        # the problem as the library takes it (device_problem.py), with copies of the references, boxes and params of its own:
        # `set_reference` and `reset` write the references in place
        p = build_problem(Q, R, None, X_ref, U_ref, None, None, x_l, x_u, u_l, u_u, reg_x, reg_u, slew_rate, u0_slew, settings, soc, builtin_model,
                          params, dev, own_copies=True, need_sym="builtin_cost needs" if builtin_cost is not None else None)
        M, N, x, u = p.M, p.N, p.xdim, p.udim
        self.M, self.N, self.xdim, self.udim = M, N, x, u
        self.X_ref, self.U_ref, self.params = p.X_ref, p.U_ref, p.params
        mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        # slew_reg: the penalty on U[0] - (the control applied last); that control is u0_slew before the first step (None: the first
        # step has no such term, as solve(..., u0_slew=None)) and the shift's um1' from then on
        self._slew0 = p.slew_reg0
        self._um1 = mk(M, u) if self._slew0 is not None else None
        self._u0_slew = p.um1
        soc_kw = p.soc_kw
        if not soc_kw and p.cone:  # as bench.py drives the cone objective through the loop (smoothing: barrier_mu = 1 / alpha)
            soc_kw = dict(cone_objective=True, barrier_mu=0.0 if math.isnan(p.smooth_alpha) else 1.0 / p.smooth_alpha)
        self._x0 = mk(M, x)
        self._pairs = [(p.X_prev, p.U_prev), (mk(M, N, x), mk(M, N, u))]  # the two trajectory pairs of the loop (`reset` fills the first)
        self._lin = [mk(M, N, x), mk(M, N, x, x), mk(M, N, u, x), mk(M, N, x), mk(M, N, x, x), mk(M, N, u, x)]  # f, fx, fu; f2, fx2, fu2
        self._res = mk(64)
        self._cost = s.prepare_cost(builtin_cost, N, x, dev, M=M, u=u) if builtin_cost is not None else None
        self._custom_cost = is_custom(builtin_cost)
        self._kw = dict(p.solve_kw(), x0=self._x0, X_ref=self.X_ref, U_ref=self.U_ref, **soc_kw)
        # the keep-out constraint: the descriptor with its device arrays (`set_keepout` writes them in place) and the augmented buffers
        # of the library loop, both made once; x0~ = [x0 | 0] is refreshed from x0 every step
        self._cstr = self._aug = None
        self._custom_cstr = constraint is not None
        if keepout is not None or constraint is not None:
            self._cstr = s.prepare_cstr(keepout if keepout is not None else constraint, M, N, x, dev)
            p.x0 = self._x0
            self._aug = keepout_buffers(p, self._cstr[0].K, sets=2)
        torch.cuda.current_stream(dev).synchronize()  # (the uploads above ran on the caller's stream; the kernels read them on the solver's)
        self.reset()

    # ---- the plan -------------------------------------------------------------------------------------------
    @property
    def X(self):
        """The current plan's states (M, N, x): stage j is the state after j + 1 steps (a GPU tensor, overwritten by the next step)."""
        return self._pairs[self._cur][0]

    @property
    def U(self):
        return self._pairs[self._cur][1]

    def _load(self, dst, src):
        src = torch.as_tensor(np.asarray(src) if not torch.is_tensor(src) else src, dtype=torch.float64)
        dst.copy_(src.to(self.device).reshape(dst.shape))

    def reset(self, X_prev=None, U_prev=None, rollout: bool = False):
        """Start over from the iterate (X_prev, U_prev) — None: X_ref / U_ref, the defaults of `solve` — with no plan to shift: the
        next `step` solves from it as it is.  `rollout=True`: the next step replaces X_prev by the rollout of its x0 under U_prev, a
        dynamically feasible start.  Clears a failure."""
        s = self.solver
        s._before()
        with torch.cuda.stream(s.stream):
            self._cur = 0
            self._load(self._pairs[0][0], self.X_ref if X_prev is None else X_prev)
            self._load(self._pairs[0][1], self.U_ref if U_prev is None else U_prev)
            if self._u0_slew is not None:
                self._um1.copy_(self._u0_slew)
        s._after()
        self._um1_valid = self._u0_slew is not None
        self._fresh, self._rollout, self.failed = True, bool(rollout), False

    def set_reference(self, X_ref=None, U_ref=None):
        """New references (M, N, x) / (M, N, u), copied into the resident buffers (None: unchanged)."""
        s = self.solver
        s._before()
        with torch.cuda.stream(s.stream):
            if X_ref is not None:
                self._load(self.X_ref, X_ref)
            if U_ref is not None:
                self._load(self.U_ref, U_ref)
        s._after()

    def set_keepout(self, centres=None, radius=None):
        """New centres and / or radii of the keep-out balls, copied into the resident arrays on the solver's stream (None: unchanged).
        Shapes as at construction: a controller built with static centres (K, pos_dim) keeps static ones.  Per-stage or per-particle
        centres are NOT moved along with the plan by `step`'s shift: stage j of the array is stage j of the next plan as it is, so a
        caller with moving obstacles sets them before every step."""
        if self._cstr is None or self._custom_cstr:
            raise ValueError("MPCController.set_keepout: the controller was built without keepout=")
        cen, rad = self._cstr[1]
        if radius is not None and not bool((torch.as_tensor(radius) > 0).all()):
            raise ValueError("keep-out constraint: every radius must be positive")
        s = self.solver
        s._before()
        with torch.cuda.stream(s.stream):
            if centres is not None:
                self._load(cen, centres)
            if radius is not None:
                self._load(rad, radius)
        s._after()

    def set_cost_params(self, cparams):
        """New parameters (M, pdim) of the custom cost (`builtin_cost=dict(kind="custom", ...)`), copied into the resident array on the
        solver's stream: the next step's linearisations read them."""
        if not self._custom_cost:
            raise ValueError('MPCController.set_cost_params: the controller was built without builtin_cost=dict(kind="custom", ...)')
        resident, cc = self._cost[1]
        shape = tuple(cparams.shape) if hasattr(cparams, "shape") else np.shape(cparams)
        if shape != tuple(resident.shape):
            raise ValueError(f"{cc!r}: params must be (M, pdim) = {tuple(resident.shape)}, got {shape}")
        s = self.solver
        s._before()
        with torch.cuda.stream(s.stream):
            self._load(resident, cparams)
        s._after()

    def set_constraint_params(self, gparams):
        """New parameters (M, pdim) of the custom constraint (`constraint=dict(cstr=, params=)`), copied into the resident array on the
        solver's stream: the next step's linearisations read them."""
        if not self._custom_cstr:
            raise ValueError("MPCController.set_constraint_params: the controller was built without constraint=dict(cstr=, params=)")
        resident, cc = self._cstr[1]
        shape = tuple(gparams.shape) if hasattr(gparams, "shape") else np.shape(gparams)
        if shape != tuple(resident.shape):
            raise ValueError(f"{cc!r}: params must be (M, pdim) = {tuple(resident.shape)}, got {shape}")
        s = self.solver
        s._before()
        with torch.cuda.stream(s.stream):
            self._load(resident, gparams)
        s._after()

    # ---- one MPC step ----------------------------------------------------------------------------------------
    def step(self, x0, iterations: int = 3, shift: int = 1, U_tail=None, return_torch: bool = False):
        """x0 (x,) or (M, x), numpy or GPU tensor -> (u0, info): u0 = U[:, 0, :] of the new plan, a copy (M, u) (numpy unless
        `return_torch`); info = dict(resid=per-iteration SCP residuals, infos=per-iteration solver infos, status=, iterations_done=,
        warm_shift=whether the first iteration was started warm from the shifted active set).
        On every call but the first after `reset` the previous plan is first moved `shift` stages on (`U_tail` (M, shift, u): the new
        last controls, None: hold).  A failed sub-problem returns (None, info); the controller then refuses `step` until `reset()`."""
        if self.failed:
            raise RuntimeError("MPCController.step: the previous step failed (info['status'] != 0); call reset() first")
        iterations = int(iterations)
        if not 1 <= iterations <= self._res.numel():
            raise ValueError(f"MPCController.step: iterations = {iterations} is outside 1 .. {self._res.numel()}")
        s = self.solver
        s._before()  # x0 (and U_tail) may come from the caller's stream; everything below is on the solver's
        with torch.cuda.stream(s.stream):
            x0 = torch.as_tensor(np.asarray(x0) if not torch.is_tensor(x0) else x0, dtype=torch.float64)
            self._x0.copy_(x0.to(self.device).reshape(-1, self.xdim).expand(self.M, self.xdim))
            if self._aug is not None:
                self._aug["x0"][:, :self.xdim].copy_(self._x0)
            if U_tail is not None:
                U_tail = torch.as_tensor(np.asarray(U_tail) if not torch.is_tensor(U_tail) else U_tail, dtype=torch.float64).to(self.device).contiguous()
        warm = False
        if self._fresh:
            if self._rollout:
                s.rollout(self.model, self._x0, self.U, self.params, out=self.X, wait_current_stream=False)
        else:
            Xn, Un = self._pairs[self._cur ^ 1]
            s.shift_plan(self.model, self.X, self.U, self.params, s=shift, U_tail=U_tail, X_out=Xn, U_out=Un, um1_out=self._um1,
                         wait_current_stream=False)
            if self.warm_shift:  # the stored statuses follow the plan; the new pair's controls become their base point
                warm = s.warm_shift(self.U, self._kw["lu"], self._kw["uu"], self._kw["Nc"], s=shift, U_tail=U_tail, U_out=Un, wait_current_stream=False)
            self._cur ^= 1
            self._um1_valid = self._um1 is not None
        self._fresh = False
        slew0 = dict(slew_reg0=self._slew0, slew_um1=self._um1) if self._um1_valid else {}
        (Xa, Ua), (Xb, Ub) = self._pairs[self._cur], self._pairs[self._cur ^ 1]
        f, fx, fu, f2, fx2, fu2 = self._lin
        res, infos, last_in_out, done = s.scp_loop(self.model, self.params, iterations, f=f, fx=fx, fu=fu, f2=f2, fx2=fx2, fu2=fu2, X_prev=Xa, U_prev=Ua,
                                                   X_out=Xb, U_out=Ub, first_cold=not warm, res=self._res[:iterations], cost=self._cost,
                                                   cstr=self._cstr, aug=self._aug, wait_current_stream=False, **slew0, **self._kw)
        if last_in_out:
            self._cur ^= 1
        ok = done == iterations
        with torch.cuda.stream(s.stream):
            resid = res[:done].cpu().numpy()  # (synchronises the solver's stream)
            u0 = self.U[:, 0, :].clone() if ok else None
        s._after()
        info = dict(resid=resid, infos=infos, status=0 if ok else int(infos[-1]["status"]), iterations_done=int(done), warm_shift=warm)
        if not ok:
            self.failed = True
            return None, info
        return (u0 if return_torch else u0.cpu().numpy()), info
