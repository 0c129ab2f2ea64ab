"""The resident problem of the device SCP front ends: the caller's arguments as float64 tensors in the layouts the library takes.

`build_problem` is what `solve(..., device=...)` (pmpc_amd/scp_device.py) and `MPCController` (pmpc_amd/mpc.py) share: argument
conversion, the ABI transposes, the reading of `solver_settings`, slew tensors, the `extra_cstrs` -> stage-cone parse.  It is plain
tensor work: no `DeviceSolver`, no library call, no stream — with `device="cpu"` it builds the same object out of CPU tensors.
`keepout_static` is the part of the keep-out augmentation (pmpc_amd.extra_cstrs.keepout_augment) that does not change with the iterate;
`keepout_buffers` adds the arrays that do, once (the Python-driven loop) or twice (the library loop, `DeviceSolver.scp_loop(cstr=, aug=)`).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict, Optional

import numpy as np
import torch

from .custom_model import CustomModel
from .dynamics import model_id

_CONE_SOLVERS = ("ecos", "gurobi", "mosek", "cosmo")  # static_backend.py:242-253


@dataclass
class DeviceProblem:
    M: int
    N: int
    xdim: int
    udim: int
    single: bool  # the caller's arrays had no particle axis (x0.ndim == 1); everything here has one
    Q: torch.Tensor  # py layout (M, N, row, col): the `obj` column and lin_cost_fn's `problems` dict
    R: torch.Tensor
    Qa: torch.Tensor  # ABI layout: column-major blocks
    Ra: torch.Tensor
    sym: bool
    x0: Optional[torch.Tensor]
    X_ref: torch.Tensor
    U_ref: torch.Tensor
    X_prev: torch.Tensor  # the start iterate: always storage of its own
    U_prev: torch.Tensor
    lx: Optional[torch.Tensor]  # a pair of bounds is None unless both are given and non-empty
    ux: Optional[torch.Tensor]
    lu: Optional[torch.Tensor]
    uu: Optional[torch.Tensor]
    reg_x: float
    reg_u: float
    Nc: int
    cone: bool  # the sub-problem has the cone objective (the reference's default path)
    smooth_alpha: float  # NaN: not set
    solver_verbose: bool
    slew: Optional[torch.Tensor]  # (M,) slew_rate, None if 0 / not given
    slew_reg0: Optional[torch.Tensor]  # (M,) solver_settings["slew_reg"], None if not set
    slew0: Optional[torch.Tensor]  # slew_reg0 if there is a u0_slew to apply it to, else None (static_backend.py:263-272)
    um1: Optional[torch.Tensor]  # (M, u) u0_slew, None without slew_reg
    soc_kw: Dict[str, Any]  # the stage cone's keywords of `lsoc_solve` / `scp_loop`; {} if there is none
    model: Any  # the id of a built-in model, a CustomModel (the solver that runs it gives it an id: DeviceSolver.load_model), or None
    params: Optional[torch.Tensor]

    def solve_kw(self) -> Dict[str, Any]:
        """The keywords of `lqp_solve` / `lcone_solve` / `lsoc_solve` / `scp_loop` that no SCP iteration changes."""
        return dict(Q=self.Qa, R=self.Ra, reg_x=self.reg_x, reg_u=self.reg_u, Nc=self.Nc, x0=self.x0, lx=self.lx, ux=self.ux, lu=self.lu,
                    uu=self.uu, slew_reg=self.slew, symmetric_cost=self.sym)


def _stage_cone(soc, settings, T, M, N, xdim, udim, Nc) -> Dict[str, Any]:
    if soc is None and settings.get("extra_cstrs"):  # the reference's tuple format, stage-wise SOC case only
        from .extra_cstrs import stage_soc_from_extra_cstrs

        tuples = list(settings["extra_cstrs"])
        if len(tuples) != 1:
            raise ValueError("one extra_cstrs tuple (the stage-wise second-order cone) is supported")
        soc = stage_soc_from_extra_cstrs(tuples[0], M, N, xdim, udim, Nc)
        if "soc_u_interior" not in settings:
            raise ValueError("solver_settings['soc_u_interior'] (a control strictly inside the boxes and the cone) is required")
        soc["u_interior"] = settings["soc_u_interior"]
    if soc is None:
        return {}
    return dict(soc_W=T(soc["W"]).reshape(-1, udim).contiguous(), soc_w0=T(soc["w0"]).reshape(-1).contiguous(),
                soc_v=T(soc["v"]).reshape(udim).contiguous(), soc_v0=float(soc.get("v0", 0.0)),
                soc_u_interior=T(soc["u_interior"]).reshape(udim).contiguous())


def build_problem(Q, R, x0=None, X_ref=None, U_ref=None, X_prev=None, U_prev=None, x_l=None, x_u=None, u_l=None, u_u=None,
                  reg_x: float = 1e0, reg_u: float = 1e-2, slew_rate: Optional[float] = None, u0_slew=None,
                  solver_settings: Optional[Dict[str, Any]] = None, soc: Optional[Dict[str, Any]] = None, builtin_model=None, params=None,
                  device="cuda", own_copies: bool = False, need_sym: Optional[str] = None, builtin_cost=None) -> DeviceProblem:
    """`own_copies`: the references, boxes and params are clones (a caller that writes them in place later, as `MPCController` does);
    otherwise they alias the caller's tensors wherever no conversion is needed.  `need_sym`: the subject of the refusal of Q / R blocks
    that are not symmetric ("builtin_cost needs"); None: they are allowed.  `builtin_cost`: a dict(kind="custom", cost=, params=) is checked
    against the problem's dimensions here (pmpc_amd.custom_cost.check_cost_dict); any other cost passes."""
    dev = torch.device(device)
    T = lambda z: None if z is None else torch.as_tensor(np.asarray(z) if not torch.is_tensor(z) else z, dtype=torch.float64, device=dev)
    Q, R, x0 = T(Q), T(R), T(x0)
    single = x0 is not None and x0.ndim == 1  # pmpc/scp_mpc.py:297-309
    if single:
        assert Q.ndim == 3 and R.ndim == 3
        Q, R, x0 = Q[None], R[None], x0[None]
    M, N, xdim, udim = Q.shape[0], Q.shape[1], Q.shape[-1], R.shape[-1]
    if builtin_cost is not None:
        from .custom_cost import check_cost_dict

        check_cost_dict(builtin_cost, M, xdim, udim)
    own = (lambda t: t.clone()) if own_copies else (lambda t: t)
    vec = lambda z, d: own(T(z).reshape(M, N, d).contiguous())
    X_ref = torch.zeros((M, N, xdim), dtype=torch.float64, device=dev) if X_ref is None else vec(X_ref, xdim)
    U_ref = torch.zeros((M, N, udim), dtype=torch.float64, device=dev) if U_ref is None else vec(U_ref, udim)
    X_prev = X_ref.clone() if X_prev is None else T(X_prev).reshape(M, N, xdim).contiguous().clone()  # default: X_ref (:313)
    U_prev = U_ref.clone() if U_prev is None else T(U_prev).reshape(M, N, udim).contiguous().clone()
    has = lambda z: z is not None and (z.numel() if torch.is_tensor(z) else np.size(z)) > 0
    lx, ux = (vec(x_l, xdim), vec(x_u, xdim)) if has(x_l) and has(x_u) else (None, None)
    lu, uu = (vec(u_l, udim), vec(u_u, udim)) if has(u_l) and has(u_u) else (None, None)
    Qa, Ra = Q.transpose(-1, -2).contiguous(), R.transpose(-1, -2).contiguous()
    sym = bool(torch.equal(Qa, Q) and torch.equal(Ra, R))
    if need_sym is not None and not sym:
        raise ValueError(f"{need_sym} symmetric Q and R blocks (the reference shift is a Cholesky solve with them)")
    settings = dict(solver_settings or {})
    cone = str(settings.get("solver", "ecos")).lower() in _CONE_SOLVERS or "smooth_cstr" in settings or "smooth_alpha" in settings
    Nc = int(settings.get("Nc", -1))
    full = lambda v: torch.full((M,), float(v), dtype=torch.float64, device=dev)
    slew = full(slew_rate) if slew_rate is not None and float(slew_rate) != 0.0 else None
    slew_reg0 = full(settings["slew_reg"]) if "slew_reg" in settings else None
    um1 = T(u0_slew).reshape(-1, udim).expand(M, udim).contiguous() if slew_reg0 is not None and u0_slew is not None else None
    custom = isinstance(builtin_model, CustomModel)
    model = builtin_model if custom else (model_id(builtin_model) if builtin_model is not None else None)
    if model is not None:
        assert params is not None, "builtin_model needs `params` (M, 3) unicycle / (M, 4) quadrotor / (M, 2) bicycle / (M, pdim) CustomModel"
        if custom:
            model.check_problem(M, xdim, udim, params)
        params = own(T(params).reshape(M, -1).contiguous())
    return DeviceProblem(M=M, N=N, xdim=xdim, udim=udim, single=single, Q=Q, R=R, Qa=Qa, Ra=Ra, sym=sym,
                         x0=None if x0 is None else x0.contiguous(), X_ref=X_ref, U_ref=U_ref, X_prev=X_prev, U_prev=U_prev, lx=lx, ux=ux,
                         lu=lu, uu=uu, reg_x=float(reg_x), reg_u=float(reg_u), Nc=Nc, cone=cone,
                         smooth_alpha=float(settings.get("smooth_alpha", math.nan)), solver_verbose=bool(settings.get("verbose", False)),
                         slew=slew, slew_reg0=slew_reg0, slew0=slew_reg0 if um1 is not None else None, um1=um1,
                         soc_kw=_stage_cone(soc, settings, T, M, N, xdim, udim, Nc), model=model, params=params if model is not None else None)


def keepout_static(p: DeviceProblem, K: int) -> Dict[str, torch.Tensor]:
    """What `extra_cstrs.keepout_augment` makes of the problem alone, at xd = xdim + K states: `Qa` (ABI layout; the auxiliary block
    -reg_x cancels the proximal term on the auxiliary states exactly), `x0` (zeros there), `lx` (-inf there) and `xu`, the upper bounds,
    of which the first xdim entries are final (the K others are every iteration's rows' right-hand sides).  NaN in a box: no bound."""
    M, N, xdim, xd = p.M, p.N, p.xdim, p.xdim + K
    mk = lambda *shape, fill: torch.full(shape, fill, dtype=torch.float64, device=p.Qa.device)
    lx, xu = mk(M, N, xd, fill=-math.inf), mk(M, N, xd, fill=math.inf)
    if p.lx is not None:
        lx[..., :xdim] = torch.where(torch.isnan(p.lx), torch.full_like(p.lx, -math.inf), p.lx)
        xu[..., :xdim] = torch.where(torch.isnan(p.ux), torch.full_like(p.ux, math.inf), p.ux)
    Qa = mk(M, N, xd, xd, fill=0.0)
    Qa[..., :xdim, :xdim] = p.Qa
    Qa[..., torch.arange(xdim, xd), torch.arange(xdim, xd)] = -p.reg_x
    x0 = mk(M, xd, fill=0.0)
    x0[:, :xdim] = p.x0
    return dict(Qa=Qa, x0=x0, lx=lx, xu=xu)


def keepout_buffers(p: DeviceProblem, K: int, sets: int = 2) -> Dict[str, Any]:
    """Every array of the problem at xd = xdim + K states, allocated once: `keepout_static`'s `Qa`, `x0`, `lx`; `sets`: that many
    dicts of the iterate-dependent arrays `f`, `fx`, `fu`, `X_prev`, `X_ref` (uninitialised: the augmentation kernel writes them) and
    `xu` (each set a copy of its own of the static upper bounds: the kernel writes the K auxiliary entries of every row); `X_out`
    (M, N, xd), the sub-problem's output.  The library loop takes two sets (include/pmpc_abi.h pmpc_scp_aug): the augmentation it
    enqueues behind a sub-problem's rounds must not touch what a continued solve still reads."""
    M, N, u, xd = p.M, p.N, p.udim, p.xdim + K
    static = keepout_static(p, K)
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=p.Qa.device)
    one = lambda k: dict(f=mk(M, N, xd), fx=mk(M, N, xd, xd), fu=mk(M, N, u, xd), X_prev=mk(M, N, xd), X_ref=mk(M, N, xd),
                         xu=static["xu"] if k == 0 else static["xu"].clone())
    return dict(Qa=static["Qa"], x0=static["x0"], lx=static["lx"], sets=[one(k) for k in range(int(sets))], X_out=mk(M, N, xd), K=int(K))
