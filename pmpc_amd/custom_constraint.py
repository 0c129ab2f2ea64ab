"""Custom state constraints: g_k(X[i, j]; p_i, j, N) <= 0 for every stage j of every particle i, written as a short piece of device code,
compiled at run time for the GPU with forward-mode automatic differentiation for the rows a_k'x <= h_k the SCP loops impose about the
previous iterate (pmpc_amd/csrc/cstr_jit.hip, model_dual.h, cstr_kernels.h).

    speed = pmpc_amd.CustomConstraint('''
    template <class T> __device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g) {   // x[XD], p[PD] -> g[KD]
      g[0] = x[3] - (p[0] - p[1] * j / N);          // v <= vmax, tightening along the horizon
      g[1] = p[2] - x[3];                           // v >= vmin
    }''', xdim=4, kdim=2, pdim=3)
    ctl = pmpc_amd.MPCController(builtin_model="bicycle", constraint=dict(cstr=speed, params=P), ...)

`x` is row j of X_prev (0-based stage j: the state after j + 1 steps); `T` is `double` or a dual number with the operator and function set
of `pmpc_amd.CustomModel`.  `p` points into global memory, so `pdim` may be 1 .. 64; `kdim` is 1 .. 4 and `xdim + kdim` at most 16 (the
sub-problem carries one auxiliary state per row).  About xbar = X_prev[i, j] an iteration imposes a_k'x <= h_k with a_k = grad g_k(xbar),
h_k = a_k'xbar - g_k(xbar).  The constraint reads states only.  The dict `dict(kind="custom", cstr=CustomConstraint, params=(M, pdim))`
enters wherever the keep-out constraint does: `solve(..., device=..., builtin_cstr=)`, `DeviceSolver.scp_loop(cstr=, aug=)`; the controller
takes it as `MPCController(constraint=dict(cstr=, params=))`.  Compiling needs no GPU.
"""
from __future__ import annotations

from typing import Optional

from .custom_jit import CustomCode, check_custom_dict, is_custom  # noqa: F401 (is_custom: imported from here by others)

MAX_DIM, MAX_KDIM, MAX_PDIM = 16, 4, 64  # states + rows: the solver's limit; parameters are read from global memory


class CustomConstraint(CustomCode):
    def __init__(self, cstr_source: str, xdim: int, kdim: int, pdim: int, name: Optional[str] = None):
        self.cstr_source, self.name = str(cstr_source), name
        self.xdim, self.kdim, self.pdim = int(xdim), int(kdim), int(pdim)
        for what, d, hi in (("xdim", self.xdim, MAX_DIM), ("kdim", self.kdim, MAX_KDIM), ("pdim", self.pdim, MAX_PDIM)):
            if not 1 <= d <= hi:
                raise ValueError(f"CustomConstraint: {what} = {d} is outside 1 .. {hi}")
        if self.xdim + self.kdim > MAX_DIM:
            raise ValueError(f"CustomConstraint: xdim + kdim = {self.xdim + self.kdim} exceeds the solver's {MAX_DIM} states")

    def __repr__(self):
        return f"CustomConstraint({self.name or 'unnamed'}, xdim={self.xdim}, kdim={self.kdim}, pdim={self.pdim})"

    def compile(self, arch: str = "gfx950") -> bytes:
        """The code object for `arch` (a target id; what follows a ':' is dropped), compiled once per object and architecture.
        A compile error is a ValueError that carries the compiler's log; a missing runtime compiler a RuntimeError."""
        return self._compile("pmpc_cstr_compile", "custom constraints", self.cstr_source, (self.xdim, self.kdim, self.pdim), arch)

    def check_problem(self, M: int, xdim: int, params) -> None:
        """Refuse a problem whose state dimension or `params` (M, pdim) are not this constraint's (host-side: no device is touched)."""
        if int(xdim) != self.xdim:
            raise ValueError(f"{self!r}: the problem has {xdim} states, not the constraint's dimensions")
        self._check_params(M, params)


def check_cstr_dict(cstr, M: int, xdim: int) -> None:
    """The host-side refusals of dict(kind="custom", cstr=, params=): no CustomConstraint, dimensions that are not the problem's, params
    that are not (M, pdim).  Any other constraint passes (the keep-out constraint has checks of its own)."""
    check_custom_dict(cstr, "cstr", CustomConstraint, "constraint", M, xdim)
