"""Device-resident API: the same solve with every buffer already in HBM (torch ROCm tensors are
used purely as device-memory handles), the on-device linearisation of the built-in models and
particle sharding over RCCL (one process per GPU, torch.distributed only bootstraps the
communicator).  This is the path bench.py times; it has no reference counterpart — the reference
copies the Jacobian stacks host<->Julia every SCP iteration (pmpc/static_backend.py:71-74)."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib

MODEL_UNICYCLE, MODEL_QUADROTOR, MODEL_BICYCLE = 0, 1, 2

# The kinds of runtime-compiled code a solver loads, by the word the messages use: the solver's dict of loaded objects, the prefix of the
# library's _load / _unload entry points, the int arguments of _load taken from the object, the first id.
_JIT_KINDS = {
    "model": ("_custom", "pmpc_model", lambda o: (o.xdim, o.udim, o.pdim), _lib.MODEL_CUSTOM0),
    "cost": ("_costs", "pmpc_cost", lambda o: (o.xdim, o.udim, o.pdim, int(o.uses_u)), _lib.COST_CUSTOM0),
    "constraint": ("_cstrs", "pmpc_cstr", lambda o: (o.xdim, o.kdim, o.pdim), _lib.CSTR_CUSTOM0),
}


def _p(t: Optional[torch.Tensor], dtype=torch.float64):
    if t is None:
        return None
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), (t.device, t.dtype, t.is_contiguous())
    return ctypes.c_void_p(t.data_ptr())


class _TorchF64:
    """The `xp` the array helpers of dynamics.py / extra_cstrs.py take (they call `xp.asarray` only): float64 tensors on `device`."""

    def __init__(self, device):
        self.device = device

    def asarray(self, a):
        return torch.as_tensor(a, dtype=torch.float64, device=self.device)


class DeviceSolver:
    """Owns a pmpc_ctx (HIP stream + workspace cache + optional RCCL communicator)."""

    def __init__(self, device: Optional[int] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("pmpc_amd.DeviceSolver needs a HIP device: there is no CPU path")
        self.lib = _lib.load()
        self.device = torch.cuda.current_device() if device is None else int(device)
        h = ctypes.c_void_p()
        rc = self.lib.pmpc_create(ctypes.byref(h), self.device)
        if rc != 0:
            raise RuntimeError(f"pmpc_create failed ({rc})")
        self.h = h
        self.stream = torch.cuda.ExternalStream(self.lib.pmpc_stream(h), device=self.device)
        self.rank, self.world = 0, 1
        self.last_info: Dict[str, float] = {}
        self._custom: Dict[int, object] = {}  # model id -> the CustomModel loaded under it (load_model)
        self._costs: Dict[int, object] = {}  # cost id -> the CustomCost loaded under it (load_cost); a table apart from the models'
        self._cstrs: Dict[int, object] = {}  # constraint id -> the CustomConstraint loaded under it (load_cstr); likewise

    # ---- runtime-compiled code: one load and one unload for the three kinds (_JIT_KINDS) ---------------
    def _load_custom(self, kind, obj) -> int:
        attr, prefix, ints, first_id = _JIT_KINDS[kind]
        self._need(prefix + "_load")
        loaded = getattr(self, attr)
        for i, o in loaded.items():
            if o is obj:
                return i
        arch = torch.cuda.get_device_properties(self.device).gcnArchName.split(":")[0]  # the target id alone, never a feature suffix
        code = obj.compile(arch)
        i = getattr(self.lib, prefix + "_load")(self.h, code, len(code), *ints(obj))
        if i < first_id:
            raise RuntimeError(f"{prefix}_load failed ({i}) for {obj!r}")
        loaded[i] = obj
        return i

    def _unload_custom(self, kind, i) -> None:
        attr, prefix, _, _ = _JIT_KINDS[kind]
        getattr(self, attr).pop(int(i), None)
        if getattr(self.lib, prefix + "_unload")(self.h, int(i)) != 0:
            raise ValueError(f"{kind} {i} is not a custom {kind} loaded on this solver")

    # ---- runtime-compiled dynamics models (pmpc_amd/custom_model.py) -----------------------------------
    def load_model(self, cm) -> int:
        """The model id (>= 1000) of a `pmpc_amd.CustomModel` on this solver: compiled for the device's architecture and loaded on
        first use, the same id from then on.  `linearize`, `rollout`, `shift_plan` and `scp_loop` take it as they take 0 - 2; it is
        known to this solver only and goes with `unload_model` or `close`."""
        return self._load_custom("model", cm)

    def unload_model(self, model: int) -> None:
        self._unload_custom("model", model)

    def _check_custom(self, model, M, x=None, u=None, params=None):
        """A loaded custom model reads x, u and pdim values per unit whatever the tensors hold: shapes that are not its own are
        refused here (the library takes no dimensions with these calls).  Other ids pass: the library knows or refuses them."""
        cm = self._custom.get(int(model))
        if cm is None:
            return
        if (x is not None and x != cm.xdim) or (u is not None and u != cm.udim):
            raise ValueError(f"{cm!r} (model {model}) was given states of {x} and controls of {u} entries")
        if params is not None and tuple(params.shape) != (M, cm.pdim):
            raise ValueError(f"{cm!r} (model {model}): params must be (M, pdim) = ({M}, {cm.pdim}), got {tuple(params.shape)}")

    # ---- runtime-compiled stage costs (pmpc_amd/custom_cost.py) ---------------------------------------
    def load_cost(self, cc) -> int:
        """The cost id (>= 1000, in a table of its own: it means a cost only where a cost is asked for) of a `pmpc_amd.CustomCost` on
        this solver: compiled for the device's architecture and loaded on first use, the same id from then on.  It is known to this
        solver only and goes with `unload_cost` or `close`."""
        return self._load_custom("cost", cc)

    def unload_cost(self, cost: int) -> None:
        self._unload_custom("cost", cost)

    def custom_cost_grad(self, cost, X_prev, U_prev, cparams, value=False, cx=None, cu=None, wait_current_stream=True):
        """(cx (M, N, x), cu (M, N, u)) — with `value` also val (M, N), the stage values — of a custom cost at (X_prev, U_prev) with the
        parameters cparams (M, pdim): one launch of the kernel compiled from the user's `stage_cost`.  `cost`: a `pmpc_amd.CustomCost`
        (loaded on first use) or the id of `load_cost`.  cu is None for a cost with uses_u=False.  `cx` / `cu`, and a tensor given as `value`: preallocated outputs."""
        self._need("pmpc_custom_cost_grad_device")
        cid = self.load_cost(cost) if not isinstance(cost, int) else int(cost)
        cc = self._costs.get(cid)
        if cc is None:
            raise ValueError(f"cost {cid} is not a custom cost loaded on this solver")
        M, N, x = X_prev.shape
        u = U_prev.shape[-1]
        assert U_prev.shape == (M, N, u), (X_prev.shape, U_prev.shape)
        cc.check_problem(M, x, u, cparams)
        dev = X_prev.device
        cx = torch.empty((M, N, x), dtype=torch.float64, device=dev) if cx is None else cx
        if cc.uses_u:
            cu = torch.empty((M, N, u), dtype=torch.float64, device=dev) if cu is None else cu
        else:
            cu = None
        val = value if torch.is_tensor(value) else (torch.empty((M, N), dtype=torch.float64, device=dev) if value else None)
        assert cx.shape == (M, N, x) and (cu is None or cu.shape == (M, N, u))
        self._before(wait_current_stream)
        st = self.lib.pmpc_custom_cost_grad_device(self.h, cid, N, M, _p(X_prev), _p(U_prev), _p(cparams), _p(cx), _p(cu), _p(val))
        self._after(wait_current_stream)
        if st != 0:
            raise RuntimeError(f"pmpc_custom_cost_grad_device failed ({st})")
        return (cx, cu, val) if val is not None else (cx, cu)

    # ---- runtime-compiled state constraints (pmpc_amd/custom_constraint.py) ---------------------------
    def load_cstr(self, cc) -> int:
        """The constraint id (>= 1000, in a table of its own) of a `pmpc_amd.CustomConstraint` on this solver: compiled for the device's
        architecture and loaded on first use, the same id from then on.  It is known to this solver only and goes with `unload_cstr` or
        `close`."""
        return self._load_custom("constraint", cc)

    def unload_cstr(self, cstr: int) -> None:
        self._unload_custom("constraint", cstr)

    def check_bad_rows(self, what):
        """Raise ValueError if the rows kernel of a custom constraint since the last check met a row whose value or gradient is not finite
        (reads and clears the device-side counter; synchronises the solver's stream)."""
        self._need("pmpc_cstr_bad_rows")
        n = self.lib.pmpc_cstr_bad_rows(self.h, 1)
        if n:
            raise ValueError(f"{what}: {n} constraint row(s) had a non-finite value or gradient at the iterate (they were dropped: h = +inf, a = 0)")

    def custom_cstr_rows(self, cstr, X_prev, gparams, value=False, a=None, h=None, wait_current_stream=True, check=False):
        """(a (M, N, K, x), h (M, N, K)) — with `value` also g (M, N, K), the constraint's values — of a custom constraint about X_prev with
        the parameters gparams (M, pdim): the rows a_k'x <= h_k, one launch of the kernel compiled from the user's `stage_cstr`.  `cstr`: a
        `pmpc_amd.CustomConstraint` (loaded on first use) or the id of `load_cstr`.  `a` / `h`, and a tensor given as `value`: preallocated
        outputs.  A row with a non-finite value or gradient comes back as h = +inf, a = 0 and counts for `check_bad_rows` (`check`: read it now)."""
        self._need("pmpc_custom_cstr_rows_device")
        gid = self.load_cstr(cstr) if not isinstance(cstr, int) else int(cstr)
        cc = self._cstrs.get(gid)
        if cc is None:
            raise ValueError(f"constraint {gid} is not a custom constraint loaded on this solver")
        M, N, x = X_prev.shape
        cc.check_problem(M, x, gparams)
        K, dev = cc.kdim, X_prev.device
        a = torch.empty((M, N, K, x), dtype=torch.float64, device=dev) if a is None else a
        h = torch.empty((M, N, K), dtype=torch.float64, device=dev) if h is None else h
        g = value if torch.is_tensor(value) else (torch.empty((M, N, K), dtype=torch.float64, device=dev) if value else None)
        assert a.shape == (M, N, K, x) and h.shape == (M, N, K) and (g is None or g.shape == (M, N, K))
        self._before(wait_current_stream)
        st = self.lib.pmpc_custom_cstr_rows_device(self.h, gid, N, M, _p(X_prev), _p(gparams), _p(a), _p(h), _p(g))
        self._after(wait_current_stream)
        if st != 0:
            raise RuntimeError(f"pmpc_custom_cstr_rows_device failed ({st})")
        if check:
            self.check_bad_rows("custom_cstr_rows")
        return (a, h, g) if g is not None else (a, h)

    def rows_augment(self, a, h, X_prev, f, fx, fu, X_ref=None, out=None, wait_current_stream=True):
        """`keepout_augment` for K dense rows a (M, N, K, x), h (M, N, K) per (particle, stage) instead of the ball geometry
        (pmpc_amd.extra_cstrs.rows_augment is the specification), one launch: the same dict in the same layouts."""
        self._need("pmpc_rows_augment_device")
        M, N, x = X_prev.shape
        u, K = fu.shape[-2], h.shape[-1]
        xd = x + K
        assert a.shape == (M, N, K, x) and h.shape == (M, N, K), (a.shape, h.shape)
        assert f.shape == (M, N, x) and fx.shape == (M, N, x, x) and fu.shape == (M, N, u, x) and (X_ref is None or X_ref.shape == (M, N, x))
        if not 1 <= K <= 4 or xd > 16:
            raise ValueError(f"rows_augment: {K} rows on {x} states are outside 1 .. 4 rows, 16 states in all")
        if out is None:
            mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=X_prev.device)
            out = dict(f=mk(M, N, xd), fx=mk(M, N, xd, xd), fu=mk(M, N, u, xd), X_prev=mk(M, N, xd), X_ref=mk(M, N, xd), xu=mk(M, N, xd))
        for k, shape in (("f", (M, N, xd)), ("fx", (M, N, xd, xd)), ("fu", (M, N, u, xd)), ("X_prev", (M, N, xd)), ("X_ref", (M, N, xd)), ("xu", (M, N, xd))):
            assert out[k].shape == shape, (k, out[k].shape, shape)
        self._before(wait_current_stream)
        st = self.lib.pmpc_rows_augment_device(self.h, K, x, u, N, M, _p(a), _p(h), _p(X_prev), _p(f), _p(fx), _p(fu), _p(X_ref), _p(out["f"]),
                                               _p(out["fx"]), _p(out["fu"]), _p(out["X_prev"]), _p(out["X_ref"]), _p(out["xu"]))
        self._after(wait_current_stream)
        if st != 0:
            raise RuntimeError(f"pmpc_rows_augment_device failed ({st})")
        return out

    def set_option(self, key: str, value: float) -> None:
        """Per-context algorithm switch (include/pmpc_abi.h, pmpc_set_option): e.g. ``set_option("xbox_as", 0)``."""
        if self.lib.pmpc_set_option(self.h, key.encode(), float(value)) != 0:
            raise KeyError(f"pmpc_set_option: unknown option {key!r}")

    def get_option(self, key: str) -> float:
        v = ctypes.c_double()
        if self.lib.pmpc_get_option(self.h, key.encode(), ctypes.byref(v)) != 0:
            raise KeyError(f"pmpc_get_option: unknown option {key!r}")
        return v.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.pmpc_destroy(self.h)  # (unloads the custom models with everything else)
            self.h = None
            self._custom, self._costs, self._cstrs = {}, {}, {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- RCCL bootstrap over an existing torch.distributed group ------------------------------------
    def init_comm(self):
        import torch.distributed as dist

        if not dist.is_initialized() or dist.get_world_size() == 1:
            return
        rank, world = dist.get_rank(), dist.get_world_size()
        uid = [None]
        if rank == 0:
            buf = ctypes.create_string_buffer(128)
            rc = self.lib.pmpc_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p))
            if rc != 0:
                raise RuntimeError(f"pmpc_comm_unique_id failed ({rc})")
            uid[0] = bytes(buf.raw)
        dist.broadcast_object_list(uid, src=0)
        buf = ctypes.create_string_buffer(uid[0], 128)
        rc = self.lib.pmpc_comm_init(self.h, rank, world, ctypes.cast(buf, ctypes.c_void_p))
        if rc != 0:
            raise RuntimeError(f"pmpc_comm_init failed ({rc})")
        self.rank, self.world = rank, world

    # ---- stream contract -----------------------------------------------------------------------------
    # The solver runs on its own non-blocking HIP stream.  By default every entry point orders that stream BEHIND the
    # caller's current torch stream before it enqueues (inputs produced by torch ops are complete when read) and orders the
    # caller's current stream behind the solver stream when it returns (outputs can be consumed by torch ops / .cpu()
    # straight away).  `wait_current_stream=False` drops both edges for callers that stay on `self.stream` themselves
    # (bench.py's loop: every producer and consumer is a library call on the solver's stream) and `sync()` at the end.
    def _before(self, on=True):
        if on:
            self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def _after(self, on=True):
        if on:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)

    # ---- solve -----------------------------------------------------------------------------------------
    def _problem(self, *, f, fx, fu, X_prev, U_prev, Q, R, X_ref, U_ref, reg_x, reg_u, Nc=-1, x0=None, lx=None, ux=None,
                 lu=None, uu=None, slew_reg=None, slew_reg0=None, slew_um1=None, X_out=None, U_out=None, weights=None,
                 barrier_mu=0.0, force_generic=False, symmetric_cost=False, cold_start=False, static_cons_bounds=False, prev_is_last_solution=False, soc_W=None, soc_w0=None,
                 soc_v=None, soc_v0=0.0, soc_u_interior=None, cone_k=0, cones=None, cone_objective=False, smooth_cstr="logbarrier", smooth_beta=1.0):
        M, N, x = f.shape
        u = U_prev.shape[-1]
        assert fx.shape == (M, N, x, x) and fu.shape == (M, N, u, x) and Q.shape == (M, N, x, x) and R.shape == (M, N, u, u)
        assert weights is None or weights.shape == (M,)
        if X_out is None:
            X_out = torch.empty((M, N, x), dtype=torch.float64, device=f.device)
        if U_out is None:
            U_out = torch.empty((M, N, u), dtype=torch.float64, device=f.device)
        flags = 0
        if lx is not None and ux is not None:
            flags |= _lib.HAS_XBOUNDS
        if lu is not None and uu is not None:
            flags |= _lib.HAS_UBOUNDS
        if slew_reg is not None:
            flags |= _lib.HAS_SLEW
        if slew_reg0 is not None and slew_um1 is not None:
            flags |= _lib.HAS_SLEW0
        if force_generic:
            flags |= _lib.FORCE_GENERIC
        if cold_start:  # ignore the interior-point iterate remembered from the previous solve of this shape
            flags |= _lib.COLD_START
        if static_cons_bounds:  # sharded SCP loops: the consensus controls' bounds are those of the previous solve (no re-broadcast)
            flags |= _lib.STATIC_CONS_BOUNDS
        if prev_is_last_solution:  # SCP loops: X_prev / U_prev are the previous solve's outputs, boxes unchanged (no rollout)
            flags |= _lib.PREV_IS_LAST_SOLUTION
        if symmetric_cost:  # Q_j, R_j exactly symmetric (enables the register-resident MFMA path)
            flags |= _lib.SYMMETRIC_COST
        if cone_objective:  # scp_loop: the sub-problem is the reference's default path (c_lcone_solve semantics; barrier_mu = 1 / smooth_alpha)
            flags |= _lib.CONE_OBJECTIVE
        # fp32-STORAGE mode (include/pmpc_abi.h PMPC_F32_MATRICES): fx, fu, Q, R as float32 tensors — all four or none
        md = torch.float32 if fx.dtype == torch.float32 else torch.float64
        assert fx.dtype == fu.dtype == Q.dtype == R.dtype == md, "fx, fu, Q, R must share one dtype (float64, or float32 for the fp32-storage mode)"
        if md == torch.float32:
            flags |= _lib.F32_MATRICES
        prob = _lib.PmpcProblem(
            xdim=x, udim=u, N=N, M=M, Nc=int(Nc), flags=flags, reg_x=float(reg_x), reg_u=float(reg_u),
            x0=_p(x0), f=_p(f), fx=_p(fx, md), fu=_p(fu, md), X_prev=_p(X_prev), U_prev=_p(U_prev), Q=_p(Q, md), R=_p(R, md),
            X_ref=_p(X_ref), U_ref=_p(U_ref), lx=_p(lx), ux=_p(ux), lu=_p(lu), uu=_p(uu), slew_reg=_p(slew_reg),
            slew_reg0=_p(slew_reg0), slew_um1=_p(slew_um1), X_out=_p(X_out), U_out=_p(U_out), weights=_p(weights), barrier_mu=float(barrier_mu),
            soc_q=0 if soc_W is None else int(soc_W.shape[0]), soc_W=_p(soc_W), soc_w0=_p(soc_w0), soc_v=_p(soc_v), soc_v0=float(soc_v0),
            soc_u_interior=_p(soc_u_interior), cone_k=int(cone_k), smooth_cstr={"logbarrier": 0, "squareplus": 1}[smooth_cstr], smooth_beta=float(smooth_beta))
        if cones is not None:  # general form of the stage cones: dict(sizes=[q_k], A=tensor, c=tensor); per-stage data if A is (M, N, rows, udim)
            sizes = [int(v) for v in cones["sizes"]]
            rows = sum(sizes) + len(sizes)
            A, cvec = cones["A"], cones["c"]
            per_stage = A.dim() == 4
            assert A.shape == ((M, N, rows, u) if per_stage else (rows, u)) and cvec.shape == ((M, N, rows) if per_stage else (rows,)), (A.shape, cvec.shape)
            self._cone_sizes = (ctypes.c_int * len(sizes))(*sizes)  # (kept alive: the struct holds a bare pointer)
            prob.cone_count, prob.cone_sizes = len(sizes), ctypes.cast(self._cone_sizes, ctypes.POINTER(ctypes.c_int))
            prob.cone_A, prob.cone_c, prob.cone_per_stage = _p(A), _p(cvec), int(per_stage)
        return prob, X_out, U_out

    def _solve(self, entry, kw, verbose, wait_current_stream, *args):
        """The part the three sub-problem solves share: the problem struct, one call of `entry` (`args` go between the problem and the
        info struct) inside the stream contract, `last_info`."""
        prob, X_out, U_out = self._problem(**kw)
        info = _lib.PmpcInfo()
        self._before(wait_current_stream)
        status = entry(self.h, ctypes.byref(prob), *args, ctypes.byref(info), int(verbose))
        self.last_info = {k: getattr(info, k) for k, _ in _lib.PmpcInfo._fields_}
        self._after(wait_current_stream)
        return X_out, U_out, status

    def lqp_solve(self, *, verbose=False, wait_current_stream=True, **kw):
        """All tensors float64 CUDA, ABI layout: vectors (M,N,d); matrices (M,N,col,row) i.e. the
        transpose of the py layout.  Returns X (M,N,x), U (M,N,u) (steps 1..N, no x0).  `weights` (M,): per-particle
        cost weights (the reference's `weights` setting, PMPC.jl/src/main.jl:96-112)."""
        return self._solve(self.lib.pmpc_lqp_solve_device, kw, verbose, wait_current_stream)

    def lcone_solve(self, *, smooth_alpha=float("nan"), verbose=False, wait_current_stream=True, **kw):
        """The cone-path objective of `c_lcone_solve` (epsilon-anchored epigraph, PMPC.jl/src/main.jl:194-354) with
        every buffer in HBM; same tensor conventions as `lqp_solve`.  `cone_k` = the reference's `k` setting (worst-k
        objective for k < M; not reachable through its C ABI)."""
        return self._solve(self.lib.pmpc_lcone_solve_device, kw, verbose, wait_current_stream, float(smooth_alpha))

    def lsoc_solve(self, *, verbose=False, wait_current_stream=True, **kw):
        """`lqp_solve` plus one second-order cone ||W u + w0||_2 <= v'u + v0 on the controls of every (particle, stage) —
        `soc_W (q, udim)`, `soc_w0 (q)`, `soc_v (udim)`, `soc_v0`, and `soc_u_interior (udim)`, a control strictly inside
        the boxes and the cone (all float64 CUDA tensors).  Config E's thrust cones; the structured case of the reference's
        pyjulia-only `extra_cstrs` (README.md:219-239).  General form: `cones=dict(sizes=[q_k, ...], A=..., c=...)` — several
        cones per stage, cone k with q_k + 1 rows of `s = A u + c` (q_k = 0: a linear row s >= 0; q_k >= 1: |s[1:]| <= s[0]),
        `A (rows, udim)` / `c (rows,)` shared by all stages or `A (M, N, rows, udim)` / `c (M, N, rows)` per stage; `weights` allowed."""
        return self._solve(self.lib.pmpc_lsoc_solve_device, kw, verbose, wait_current_stream)

    def particle_costs(self, X, U, **kw):
        """J_i(X, U) of PMPC.jl/src/qp_utils.jl:60-162 for every particle (device tensor, (M,))."""
        prob, _, _ = self._problem(X_out=X, U_out=U, **kw)
        J = torch.empty((X.shape[0],), dtype=torch.float64, device=X.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        self.lib.pmpc_particle_costs_device(self.h, ctypes.byref(prob), _p(X), _p(U), _p(J))
        self.sync()
        return J

    def linearize(self, model: int, x0, X_prev, U_prev, params, f=None, fx=None, fu=None, wait_current_stream=True):
        """f, fx, fu (ABI layout) at X_ = [x0, X_prev[:-1]], U_prev for a built-in model or a loaded custom one (`load_model`)."""
        M, N, x = X_prev.shape
        u = U_prev.shape[-1]
        self._check_custom(model, M, x, u, params)
        dev = X_prev.device
        f = torch.empty((M, N, x), dtype=torch.float64, device=dev) if f is None else f
        fx = torch.empty((M, N, x, x), dtype=torch.float64, device=dev) if fx is None else fx
        fu = torch.empty((M, N, u, x), dtype=torch.float64, device=dev) if fu is None else fu
        self._before(wait_current_stream)
        if fx.dtype == torch.float32:  # fp32-storage mode: the Jacobian stacks are written as float32
            st = self.lib.pmpc_linearize_device_f32(self.h, int(model), N, M, _p(x0), _p(X_prev), _p(U_prev), _p(params), _p(f), _p(fx, torch.float32),
                                               _p(fu, torch.float32))
        else:
            st = self.lib.pmpc_linearize_device(self.h, int(model), N, M, _p(x0), _p(X_prev), _p(U_prev), _p(params), _p(f), _p(fx),
                                           _p(fu))
        self._after(wait_current_stream)
        if st != 0:
            raise RuntimeError(f"pmpc_linearize_device failed ({st}): model {model} is not a built-in model, or a HIP error")
        return f, fx, fu

    def rollout(self, model: int, x0, U, params, out=None, wait_current_stream=True):
        """X (M, N, x) = the nonlinear rollout of a built-in model from x0 (M, x) under U (M, N, u) (pmpc_amd.dynamics.rollout is the
        specification): X[:, j] = F(X[:, j - 1], U[:, j]; params), the `f` of `linearize` evaluated alone.  `out` must not be `x0`."""
        self._need("pmpc_rollout_device")
        M, N, _ = U.shape
        x = x0.shape[-1]
        assert x0.shape == (M, x), (x0.shape, U.shape)
        self._check_custom(model, M, x, U.shape[-1], params)
        out = torch.empty((M, N, x), dtype=torch.float64, device=U.device) if out is None else out
        assert out.shape == (M, N, x)
        self._before(wait_current_stream)
        st = self.lib.pmpc_rollout_device(self.h, int(model), N, M, _p(x0), _p(U), _p(params), _p(out))
        self._after(wait_current_stream)
        if st != 0:
            raise RuntimeError(f"pmpc_rollout_device failed ({st}): model {model} is not a built-in model, an empty horizon, or a HIP error")
        return out

    def shift_plan(self, model: int, X, U, params, s=1, U_tail=None, X_out=None, U_out=None, um1_out=None, wait_current_stream=True):
        """The receding-horizon shift of a plan by `s` stages, 1 <= s < N (pmpc_amd.dynamics.shift_plan is the specification), in one
        launch: returns (X', U', um1').  Never in place: `X_out` / `U_out` are other tensors than `X` / `U` (the second trajectory pair
        of `scp_loop`).  `U_tail` (M, s, u): the controls of the new last s stages, None: the last control is held; their states are
        rolled out.  um1' = U[:, s - 1] (the control that was applied) is what `slew_um1` of the next solve takes."""
        self._need("pmpc_shift_plan_device")
        M, N, x = X.shape
        u = U.shape[-1]
        assert U.shape == (M, N, u) and (U_tail is None or U_tail.shape == (M, int(s), u)), (X.shape, U.shape)
        self._check_custom(model, M, x, u, params)
        X_out = torch.empty_like(X) if X_out is None else X_out
        U_out = torch.empty_like(U) if U_out is None else U_out
        um1_out = torch.empty((M, u), dtype=torch.float64, device=U.device) if um1_out is None else um1_out
        assert X_out.shape == X.shape and U_out.shape == U.shape and um1_out.shape == (M, u)
        if not 1 <= int(s) < N or X_out.data_ptr() == X.data_ptr() or U_out.data_ptr() == U.data_ptr():
            raise ValueError(f"shift_plan: s = {s} must be in 1 .. N - 1 = {N - 1}, and the shift is not done in place")
        self._before(wait_current_stream)
        st = self.lib.pmpc_shift_plan_device(self.h, int(model), N, M, int(s), _p(X), _p(U), _p(params), _p(U_tail), _p(X_out), _p(U_out), _p(um1_out))
        self._after(wait_current_stream)
        if st != 0:
            raise RuntimeError(f"pmpc_shift_plan_device failed ({st}): model {model} is not a built-in model, or a HIP error")
        return X_out, U_out, um1_out

    def _shift_set_args(self, what, U, s, U_tail, lo, hi, U_out):
        M, N, u = U.shape
        assert (U_tail is None or U_tail.shape == (M, int(s), u)) and (lo is None or lo.shape == U.shape) and (hi is None or hi.shape == U.shape), U.shape
        U_out = torch.empty_like(U) if U_out is None else U_out
        assert U_out.shape == U.shape
        if not 1 <= int(s) < N or U_out.data_ptr() == U.data_ptr():
            raise ValueError(f"{what}: s = {s} must be in 1 .. N - 1 = {N - 1}, and the shift is not done in place")
        return M, N, u, U_out

    def shift_active_set(self, act, U, lo, hi, Nc, s=1, U_tail=None, U_out=None, act_out=None, wait_current_stream=True):
        """Control-box statuses `act` (M, N, u) int32 (0 free, 1 lower, 2 upper bound) moved `s` stages on together with the controls U
        into the boxes lo / hi (M, N, u; None: unbounded) of the stages they arrive at (pmpc_amd.dynamics.shift_active_set is the
        specification), one launch on the caller's tensors: returns (act', U').  Never in place."""
        self._need("pmpc_shift_active_set_device")
        M, N, u, U_out = self._shift_set_args("shift_active_set", U, s, U_tail, lo, hi, U_out)
        act_out = torch.empty_like(act) if act_out is None else act_out
        assert act.shape == U.shape and act_out.shape == U.shape
        if act_out.data_ptr() == act.data_ptr():
            raise ValueError("shift_active_set: the shift is not done in place")
        self._before(wait_current_stream)
        st = self.lib.pmpc_shift_active_set_device(self.h, N, M, u, int(Nc), int(s), _p(U), _p(U_tail), _p(act, torch.int32), _p(lo), _p(hi), _p(U_out),
                                                   _p(act_out, torch.int32))
        self._after(wait_current_stream)
        if st != 0:
            raise RuntimeError(f"pmpc_shift_active_set_device failed ({st})")
        return act_out, U_out

    def warm_shift(self, U, lo, hi, Nc, s=1, U_tail=None, U_out=None, wait_current_stream=True) -> bool:
        """`shift_active_set` applied to the set this context's last accepted solve stored: U (M, N, u) is the plan BEFORE its shift,
        `U_out` the shifted plan's controls (written behind `shift_plan` on the solver's stream), lo / hi the problem's lu / uu.  True: the
        stored statuses now belong to `U_out` and the next `scp_loop` of this shape may run with `first_cold=False`.  False: nothing was
        stored (no accepted active-set solve of this shape since; a sharded context), nothing ran and `U_out` is untouched.  Stage-cone,
        state-row and epigraph multipliers are not moved: a problem with those keeps `first_cold=True`."""
        self._need("pmpc_warm_shift_device")
        M, N, u, U_out = self._shift_set_args("warm_shift", U, s, U_tail, lo, hi, U_out)
        shifted = ctypes.c_int(0)
        self._before(wait_current_stream)
        st = self.lib.pmpc_warm_shift_device(self.h, N, M, u, int(Nc), int(s), _p(U), _p(U_tail), _p(lo), _p(hi), _p(U_out), ctypes.byref(shifted))
        self._after(wait_current_stream)
        if st != 0:
            raise RuntimeError(f"pmpc_warm_shift_device failed ({st})")
        return bool(shifted.value)

    def warm_set(self, M, N, u, device=None):
        """The control-box statuses the last accepted solve stored, an (M, N, u) int32 tensor (a copy), or None if nothing of that size is
        stored.  For tests and tools."""
        self._need("pmpc_warm_set_read_device")
        out = torch.empty((M, N, u), dtype=torch.int32, device=torch.device("cuda", self.device) if device is None else device)
        self._before()
        st = self.lib.pmpc_warm_set_read_device(self.h, _p(out, torch.int32), M * N * u)
        self._after()
        if st == 2:
            return None
        if st != 0:
            raise RuntimeError(f"pmpc_warm_set_read_device failed ({st})")
        return out

    def linearize_compact(self, model: int, x0, X_prev, U_prev, params, wait_current_stream=True):
        """f (dense) and the compact Jacobian records (one flat tensor) the SCP loop writes for its warm solves."""
        M, N, x = X_prev.shape
        f = torch.empty((M, N, x), dtype=torch.float64, device=X_prev.device)
        n = self.lib.pmpc_jac_compact_doubles(int(model), N, M)
        if n < 0:
            raise RuntimeError(f"model {model} is not a built-in model")
        jc = torch.empty((n,), dtype=torch.float64, device=X_prev.device)
        self._before(wait_current_stream)
        st = self.lib.pmpc_linearize_compact_device(self.h, int(model), N, M, _p(x0), _p(X_prev), _p(U_prev), _p(params), _p(f), _p(jc))
        self._after(wait_current_stream)
        assert st == 0, st
        return f, jc

    def expand_jac(self, model: int, jc, M: int, N: int, x: int, u: int, orient: int = 0, wait_current_stream=True):
        """Dense (fx, fu) in ABI layout from compact records, read through their column- (0) or row-oriented (1) part."""
        fx = torch.empty((M, N, x, x), dtype=torch.float64, device=jc.device)
        fu = torch.empty((M, N, u, x), dtype=torch.float64, device=jc.device)
        self._before(wait_current_stream)
        st = self.lib.pmpc_expand_jac_device(self.h, int(model), N, M, _p(jc), _p(fx), _p(fu), int(orient))
        self._after(wait_current_stream)
        assert st == 0, st
        return fx, fu

    # ---- linearised nonlinear costs (csrc/cost_lin.hip) ------------------------------------------------------
    def _need(self, symbol):
        if not hasattr(self.lib, symbol):  # (an older library loaded through PMPC_HIP_LIB: _lib.load leaves the cost prototypes out)
            raise RuntimeError(f"{_lib.LIB_PATH} has no {symbol}: it predates this entry point, rebuild it (make -C pmpc_amd/csrc)")

    def check_bad_pivots(self, what):
        """Raise ValueError if a reference shift since the last check met a block that is not positive definite (reads and clears the
        device-side counter; synchronises the solver's stream)."""
        self._need("pmpc_ref_shift_bad_pivots")
        n = self.lib.pmpc_ref_shift_bad_pivots(self.h, 1)  # (synchronises the solver's stream; the one read of the call)
        if n:
            raise ValueError(f"{what}: {n} cost block(s) are not symmetric positive definite (their rows of the result are NaN)")

    def ref_shift(self, A, c, ref, out=None, wait_current_stream=True, check=True):
        """out = ref - A^-1 c block by block — the reference shift of a linearised cost (pmpc/scp_mpc.py:171-185): A (..., d, d)
        symmetric positive definite blocks (Q or R; ABI layout, which is immaterial for symmetric blocks), c, ref (..., d), d <= 16;
        `out` may be `ref`.  A block that is not positive definite gives NaN in its row and (`check`) a ValueError for the whole call
        after one read of the device-side counter; `check=False` skips that read (and the synchronisation it costs)."""
        self._need("pmpc_ref_shift_device")
        d = A.shape[-1]
        rows = A.numel() // (d * d) if d else 0
        if not 1 <= d <= 16:
            raise ValueError(f"ref_shift: block dimension {d} is outside 1 .. 16")
        assert A.shape[-2] == d and c.shape == ref.shape and c.shape[-1] == d and c.numel() == rows * d, (A.shape, c.shape, ref.shape)
        out = torch.empty_like(ref) if out is None else out
        assert out.shape == ref.shape
        self._before(wait_current_stream)
        st = self.lib.pmpc_ref_shift_device(self.h, d, rows, _p(A), _p(c), _p(ref), _p(out))
        self._after(wait_current_stream)
        if st != 0:
            raise RuntimeError(f"pmpc_ref_shift_device failed ({st})")
        if check:
            self.check_bad_pivots("ref_shift")
        return out

    def prepare_cost(self, cost, N, x, device="cuda", M=None, u=None):
        """A handle of a built-in cost for repeated `obstacle_cost_grad` / `scp_loop` calls on (N stages, x states): the descriptor
        and its device arrays, uploaded once.  Both methods take the handle wherever they take the dict.  dict(kind="custom", cost=,
        params=) (pmpc_amd.CustomCost; needs M and u): the cost is loaded on this solver and params (M, pdim) uploaded; the handle's
        second entry is [params on the device, the CustomCost]."""
        return self._scp_cost(cost, N, x, device, M, u)

    def _scp_cost(self, cost, N, x, device, M=None, u=None):
        """dict(kind="obstacles", pos_idx=, centres=, sigma=, w=) -> pmpc_scp_cost (+ the tensors it points to, to be kept alive);
        dict(kind="custom", cost=, params=) -> a kind-2 descriptor; a handle of `prepare_cost` passes through."""
        self._need("pmpc_scp_loop_device_cost")
        if isinstance(cost, tuple):
            return cost
        from .custom_cost import check_cost_dict, is_custom

        if is_custom(cost):
            self._need("pmpc_cost_load")
            if M is None or u is None:
                raise ValueError('a dict(kind="custom") cost needs the problem\'s M and udim (prepare_cost(cost, N, x, device, M=, u=))')
            check_cost_dict(cost, M, x, u)  # (host side, before anything is loaded)
            cc = cost["cost"]
            cid = self.load_cost(cc)
            cparams = torch.as_tensor(cost["params"], dtype=torch.float64).to(device).reshape(M, cc.pdim).contiguous()
            if torch.is_tensor(cost["params"]) and cparams.data_ptr() == cost["params"].data_ptr():
                cparams = cparams.clone()  # (the handle's array is its own: MPCController.set_cost_params writes it in place)
            torch.cuda.current_stream(self.device).synchronize()  # (uploaded on the caller's stream; the kernels read it on the solver's)
            return _lib.PmpcScpCost(kind=2, id=cid, uses_u=int(cc.uses_u), cparams=cparams.data_ptr()), [cparams, cc]
        from .dynamics import _obstacle_arrays

        pos_idx, cen, sigma, w = _obstacle_arrays(cost, N, _TorchF64(device))
        if max(pos_idx) >= x or min(pos_idx) < 0:
            raise ValueError(f"obstacle cost: pos_idx {pos_idx} outside the {x} states")
        keep = [cen.contiguous(), sigma.contiguous(), w.contiguous()]
        torch.cuda.current_stream(self.device).synchronize()  # (they were just uploaded on the caller's stream; the kernels read them on the solver's)
        sc = _lib.PmpcScpCost(kind=1, K=int(sigma.shape[0]), pos_dim=len(pos_idx), pos_idx=(ctypes.c_int * 3)(*pos_idx), per_stage=int(cen.shape[0] != 1),
                              centres=keep[0].data_ptr(), sigma=keep[1].data_ptr(), w=keep[2].data_ptr())
        return sc, keep

    def obstacle_cost_grad(self, X_prev, cost, *, Q=None, X_ref=None, out=None, wait_current_stream=True, check=True):
        """Gradient cx (M, N, x) of the built-in obstacle cost (pmpc_amd.dynamics.obstacle_cost is the specification) at X_prev.
        With `Q` and `X_ref`: the fused form the loops use — returns X_ref - Q^-1 cx from one launch, cx is never stored."""
        M, N, x = X_prev.shape
        sc, keep = self._scp_cost(cost, N, x, X_prev.device)
        out = torch.empty_like(X_prev) if out is None else out
        self._before(wait_current_stream)
        if Q is None:
            st = self.lib.pmpc_obstacle_cost_grad_device(self.h, ctypes.byref(sc), x, N, M, _p(X_prev), _p(out))
        else:
            assert Q.shape == (M, N, x, x) and X_ref.shape == (M, N, x)
            st = self.lib.pmpc_obstacle_ref_shift_device(self.h, ctypes.byref(sc), x, N, M, _p(X_prev), _p(Q), _p(X_ref), _p(out))
        self._after(wait_current_stream)
        if st != 0:
            raise RuntimeError(f"obstacle cost kernels failed ({st})")
        if Q is not None and check:
            self.check_bad_pivots("obstacle_cost_grad")
        if not wait_current_stream:
            self.sync()
        del keep  # (the cost's device arrays: the launch is done, or the caller's stream — where torch reuses their memory — waits for it)
        return out

    # ---- keep-out constraints (csrc/keepout.hip) ---------------------------------------------------------------
    def prepare_cstr(self, cstr, M, N, x, device="cuda"):
        """A handle of a built-in constraint dict(kind="keepout", pos_idx=, centres=, radius=) for repeated `keepout_augment` calls on
        (M particles, N stages, x states): the descriptor and its device arrays, uploaded once.  centres: (K, pos_dim) static,
        (N, K, pos_dim) per stage, (M, N, K, pos_dim) per particle and stage.  A handle passes through.
        dict(kind="custom", cstr=pmpc_amd.CustomConstraint, params=(M, pdim)): the constraint is loaded on this solver and params uploaded; a
        kind-2 descriptor whose second entry is [params on the device, the CustomConstraint] (`scp_loop` takes it; `keepout_augment` does not)."""
        self._need("pmpc_keepout_augment_device")
        if isinstance(cstr, tuple):
            return cstr
        from .custom_constraint import check_cstr_dict, is_custom

        if is_custom(cstr):
            self._need("pmpc_cstr_load")
            check_cstr_dict(cstr, M, x)  # (host side, before anything is loaded)
            cc = cstr["cstr"]
            gid = self.load_cstr(cc)
            gparams = torch.as_tensor(cstr["params"], dtype=torch.float64).to(device).reshape(M, cc.pdim).contiguous()
            if torch.is_tensor(cstr["params"]) and gparams.data_ptr() == cstr["params"].data_ptr():
                gparams = gparams.clone()  # (the handle's array is its own: MPCController.set_constraint_params writes it in place)
            torch.cuda.current_stream(self.device).synchronize()  # (uploaded on the caller's stream; the kernels read it on the solver's)
            return _lib.PmpcScpCstr(kind=2, K=cc.kdim, id=gid, gparams=gparams.data_ptr()), [gparams, cc]
        from .extra_cstrs import _keepout_arrays

        pos_idx, cen, rad = _keepout_arrays(cstr, M, N, x, _TorchF64(device))
        K, pd = int(rad.shape[0]), len(pos_idx)
        if x + K > 16:
            raise ValueError(f"keep-out constraint: {x} states + {K} auxiliary states exceed the solver's 16")
        stride_p = N * K * pd if cen.shape[0] != 1 else 0
        stride_s = K * pd if cen.shape[1] != 1 or cen.shape[0] != 1 else 0
        keep = [cen.contiguous(), rad.contiguous()]
        torch.cuda.current_stream(self.device).synchronize()  # (they were just uploaded on the caller's stream; the kernel reads them on the solver's)
        sc = _lib.PmpcScpCstr(kind=1, K=K, pos_dim=pd, pos_idx=(ctypes.c_int * 3)(*pos_idx), centre_stride_particle=stride_p,
                              centre_stride_stage=stride_s, centres=keep[0].data_ptr(), radius=keep[1].data_ptr())
        return sc, keep

    def keepout_augment(self, cstr, X_prev, f, fx, fu, X_ref=None, out=None, wait_current_stream=True):
        """The linearisation (f, fx, fu: ABI layout) with the keep-out rows about X_prev restated as upper bounds on K auxiliary states
        (pmpc_amd.extra_cstrs.keepout_augment is the specification), one launch: returns dict(f (M, N, xd), fx (M, N, xd, xd),
        fu (M, N, u, xd), X_prev (M, N, xd), X_ref (M, N, xd), xu (M, N, xd)), xd = x + K.  Of `xu` only the K auxiliary entries of every
        stage are written (the rows' right-hand sides); `X_ref` is written if an X_ref is given.  `out`: the same dict, preallocated."""
        M, N, x = X_prev.shape
        u = fu.shape[-2]
        sc, keep = self.prepare_cstr(cstr, M, N, x, X_prev.device)
        if sc.kind != 1:
            raise ValueError("keepout_augment takes the keep-out constraint; a custom constraint goes through custom_cstr_rows and rows_augment")
        xd = x + sc.K
        assert f.shape == (M, N, x) and fx.shape == (M, N, x, x) and fu.shape == (M, N, u, x) and (X_ref is None or X_ref.shape == (M, N, x))
        if out is None:
            mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=X_prev.device)
            out = dict(f=mk(M, N, xd), fx=mk(M, N, xd, xd), fu=mk(M, N, u, xd), X_prev=mk(M, N, xd), X_ref=mk(M, N, xd), xu=mk(M, N, xd))
        for k, shape in (("f", (M, N, xd)), ("fx", (M, N, xd, xd)), ("fu", (M, N, u, xd)), ("X_prev", (M, N, xd)), ("X_ref", (M, N, xd)), ("xu", (M, N, xd))):
            assert out[k].shape == shape, (k, out[k].shape, shape)
        self._before(wait_current_stream)
        st = self.lib.pmpc_keepout_augment_device(self.h, ctypes.byref(sc), x, u, N, M, _p(X_prev), _p(f), _p(fx), _p(fu), _p(X_ref), _p(out["f"]),
                                                  _p(out["fx"]), _p(out["fu"]), _p(out["X_prev"]), _p(out["X_ref"]), _p(out["xu"]))
        self._after(wait_current_stream)
        if st != 0:
            raise RuntimeError(f"pmpc_keepout_augment_device failed ({st})")
        if not wait_current_stream:
            self.sync()
        del keep  # (the constraint's device arrays: the launch is done, or the caller's stream — where torch reuses their memory — waits for it)
        return out

    def scp_residual(self, X, X_prev, U, U_prev, out=None, wait_current_stream=True):
        """max(max_ij ||X - X_prev||_2, max_ij ||U - U_prev||_2) of pmpc/scp_mpc.py:397-403 as a one-element device tensor
        (one fused pass on the solver's stream; inf if a trajectory holds a NaN)."""
        M, N, x = X.shape
        out = torch.empty((1,), dtype=torch.float64, device=X.device) if out is None else out
        self._before(wait_current_stream)
        self.lib.pmpc_scp_residual_device(self.h, x, U.shape[-1], N, M, _p(X), _p(X_prev), _p(U), _p(U_prev), _p(out))
        self._after(wait_current_stream)
        return out

    def strip_residual(self, X_aug, X, X_prev, U, U_prev, out=None, wait_current_stream=True):
        """The way back from a sub-problem with K auxiliary states, one launch: `X` (M, N, x) <- `X_aug[..., :x]` (X_aug (M, N, x + K)),
        and the SCP residual of (X, X_prev), (U, U_prev) as `scp_residual` gives it for the stripped array, a one-element device tensor."""
        self._need("pmpc_keepout_strip_residual_device")
        M, N, x = X.shape
        K = X_aug.shape[-1] - x
        assert X_aug.shape == (M, N, x + K) and X_prev.shape == X.shape and U.shape == U_prev.shape and U.shape[:2] == (M, N)
        out = torch.empty((1,), dtype=torch.float64, device=X.device) if out is None else out
        self._before(wait_current_stream)
        st = self.lib.pmpc_keepout_strip_residual_device(self.h, x, K, U.shape[-1], N, M, _p(X_aug), _p(X), _p(X_prev), _p(U), _p(U_prev), _p(out))
        self._after(wait_current_stream)
        if st != 0:
            raise RuntimeError(f"pmpc_keepout_strip_residual_device failed ({st}): K outside 1 .. 4, x + K > 16, an empty array, or a HIP error")
        return out

    def scp_loop(self, model: int, params, steps: int, *, f2, fx2, fu2, first_cold=True, res=None, wait_current_stream=True, cost=None, cstr=None,
                 aug=None, **kw):
        """`steps` SCP iterations (linearise -> sub-problem -> residual -> swap) for a built-in dynamics model (or a custom one, by the
        id of `load_model`: dense float64 Jacobians, refused with status 2 next to float32 matrices) in ONE library
        call: the host is out of the loop body (no Python / ctypes work between iterations, the residual and the next
        linearisation are enqueued behind the sub-problem's rounds before their outcome is read back).  `kw` as for
        `lqp_solve` / `lsoc_solve` with `f, fx, fu` (scratch the linearisation writes), `X_prev, U_prev` (start iterate,
        OVERWRITTEN) and `X_out, U_out`; `f2, fx2, fu2`: a second scratch set.  Returns (res, infos, last_in_out, done):
        per-iteration residuals (device tensor), per-iteration info dicts, whether the final iterate is in (X_out, U_out)
        (else in (X_prev, U_prev)), iterations completed.  `cost=dict(kind="obstacles", pos_idx=, centres=, sigma=, w=)`: the built-in
        obstacle cost (`obstacle_cost_grad`) is linearised about every iterate and the sub-problem tracks X_ref - Q^-1 cx (float64 Q
        with symmetric positive definite blocks; refused with status 2 next to float32 matrices).  `cost=dict(kind="custom",
        cost=pmpc_amd.CustomCost, params=(M, pdim))`: the user's stage cost (`custom_cost_grad`); the sub-problem tracks X_ref - Q^-1 cx
        and, unless the cost has uses_u=False, U_ref - R^-1 cu (R likewise).
        `cstr=`: a keep-out constraint or dict(kind="custom", cstr=pmpc_amd.CustomConstraint, params=(M, pdim)) (rows about every iterate from
        `custom_cstr_rows`, augmented by `rows_augment`; K = kdim), the dict of `prepare_cstr` or its handle, with `aug=pmpc_amd.device_problem.keepout_buffers(problem, K)`
        (two sets), allocated once by the caller: every iteration's sub-problem runs at x + K states on those buffers (`keepout_augment`'s
        launch in front of it, `strip_residual`'s behind it); everything this method takes and returns stays at x states.  Refused by
        the library with status 2: a stage cone, slew penalties, float32 matrices, a sharded context, smooth_cstr="squareplus"."""
        if kw.pop("builtin_cstr", None) is not None:
            raise ValueError("scp_loop: builtin_cstr is not supported (the keep-out constraint enters the library loop as cstr=, a dict or the handle "
                             "of prepare_cstr, with aug=keepout_buffers(...); solve(..., device=..., builtin_cstr=...) carries it in the Python-driven loop)")
        prob, X_out, U_out = self._problem(**kw)
        res = torch.empty((steps,), dtype=torch.float64, device=f2.device) if res is None else res
        infos = (_lib.PmpcInfo * steps)()
        last = ctypes.c_int(0)
        M, N, x = kw["f"].shape
        self._check_custom(model, M, params=params)  # (dimensions that are not the problem's: the library refuses them, status 2)
        if cost is not None:
            sc, keep = self._scp_cost(cost, N, x, f2.device, M, kw["U_prev"].shape[-1])
        if cstr is not None:
            self._need("pmpc_scp_loop_device_cstr")
            if aug is None:
                raise ValueError("scp_loop(cstr=...) needs aug=keepout_buffers(problem, K): the augmented buffers, allocated once")
            own_cstr = not isinstance(cstr, tuple)
            cs, keep_cstr = self.prepare_cstr(cstr, M, N, x, f2.device)
            sets = aug["sets"]
            if aug["K"] != cs.K or len(sets) != 2 or aug["X_out"].shape != (M, N, x + cs.K):
                raise ValueError(f"scp_loop(cstr=...): aug is not keepout_buffers(problem, K={cs.K}, sets=2) of this problem")
            two = lambda k: (ctypes.c_void_p * 2)(_p(sets[0][k]), _p(sets[1][k]))
            ab = _lib.PmpcScpAug(Q=_p(aug["Qa"]), x0=_p(aug["x0"]), lx=_p(aug["lx"]), f=two("f"), fx=two("fx"), fu=two("fu"), X_prev=two("X_prev"),
                                 X_ref=two("X_ref"), xu=two("xu"), X_out=_p(aug["X_out"]))
        self._before(wait_current_stream)
        jd = kw["fx"].dtype
        head = (self.h, int(model), _p(params), ctypes.byref(prob), _p(f2), _p(fx2, jd), _p(fu2, jd), int(steps), int(bool(first_cold)), _p(res), infos,
                ctypes.byref(last))
        if cstr is not None:
            done = self.lib.pmpc_scp_loop_device_cstr(*head, ctypes.byref(sc) if cost is not None else None, ctypes.byref(cs), ctypes.byref(ab))
            if cost is not None or own_cstr:
                self.sync()  # (device arrays that are this call's own: the launches that read them are done before they go)
            del keep_cstr
        elif cost is None:
            done = self.lib.pmpc_scp_loop_device(*head)
        else:
            done = self.lib.pmpc_scp_loop_device_cost(*head, ctypes.byref(sc))
            self.sync()  # (the cost's device arrays are this call's own: the launches that read them are done before they go)
        if cost is not None:
            del keep
        self._after(wait_current_stream)
        if cost is not None:
            self.check_bad_pivots("scp_loop(cost=...): Q" + (" or R" if sc.kind == 2 else ""))
        if cstr is not None and cs.kind == 2:
            self.check_bad_rows("scp_loop(cstr=...)")
        out = [{k: getattr(infos[i], k) for k, _ in _lib.PmpcInfo._fields_} for i in range(min(done + 1, steps))]
        if out:
            self.last_info = out[min(done, steps) - 1] if done > 0 else out[0]
        return res, out, bool(last.value), done

    def sync(self):
        self.lib.pmpc_sync(self.h)

    def profile(self, level):
        """0 / False: off; 1 / True: HIP events around the dominant kernel (factor sweep) only; 2: every launch class."""
        self.lib.pmpc_profile_enable(self.h, int(level))

    def profile_read(self):
        """{class: (sum_ms, launches)} of HIP-event timings on the solver stream since the last read."""
        ms = (ctypes.c_double * 4)()
        n = (ctypes.c_longlong * 4)()
        self.lib.pmpc_profile_read(self.h, ms, n)
        names = ("bwd_factor", "bwd_vec", "fwd", "consensus")
        out = {k: (ms[i], n[i]) for i, k in enumerate(names)}
        pms, pn = ctypes.c_double(), ctypes.c_longlong()
        self.lib.pmpc_profile_read_partial(self.h, ctypes.byref(pms), ctypes.byref(pn))
        out["bwd_factor_partial"] = (pms.value, pn.value)  # active-set rounds that skip the settled particles (level 2 only)
        ms8, n8 = (ctypes.c_double * 8)(), (ctypes.c_longlong * 8)()
        self.lib.pmpc_profile_read_all(self.h, ms8, n8, 8)
        for k, name in ((5, "as_bookkeeping"), (6, "linearize"), (7, "scp_residual")):
            out[name] = (ms8[k], n8[k])
        return out

    def restart_stats(self, reset: bool = True):
        """Factor sweeps of unsettled particles in the later rounds since the last reset (option ``as_ckpt``):
        ``dict(restarted=, restarted_stages=, full=, full_stages=)`` — sweeps that started from a checkpoint / from the
        terminal cost, and the stages they ran."""
        out = (ctypes.c_ulonglong * 4)()
        self.lib.pmpc_restart_stats(self.h, out, 1 if reset else 0)
        return dict(restarted=int(out[0]), restarted_stages=int(out[1]), full=int(out[2]), full_stages=int(out[3]))


def to_device_problem(prob: dict, device="cuda"):
    """py-layout numpy problem (pmpc_amd.dynamics.make_*_problem) -> ABI-layout CUDA tensors."""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=device)
    tm = lambda a: torch.as_tensor(np.ascontiguousarray(np.swapaxes(a, -1, -2)), dtype=torch.float64, device=device)
    out = dict(x0=t(prob["x0"]), Q=tm(prob["Q"]), R=tm(prob["R"]), X_ref=t(prob["X_ref"]), U_ref=t(prob["U_ref"]),
               X_prev=t(prob["X_prev"]), U_prev=t(prob["U_prev"]), params=t(prob["params"]))
    for k_src, k_dst in (("u_l", "lu"), ("u_u", "uu"), ("x_l", "lx"), ("x_u", "ux")):
        if prob.get(k_src) is not None:
            out[k_dst] = t(prob[k_src])
    return out
