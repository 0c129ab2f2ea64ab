"""Custom stage costs without a GPU: the runtime compile for gfx950 (it needs no device), its refusals, the test costs under the dual
arithmetic of pmpc_amd/csrc/model_dual.h as host C++ against their closed forms, the layout of pmpc_scp_cost, and the front ends'
refusals before a device is touched."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pmpc_amd
from pmpc_amd import _lib
from tests.support import custom_costs as cc

ROOT = Path(__file__).resolve().parent.parent
TOL = dict(rtol=1e-12, atol=1e-12)  # the tolerance of tests/test_custom_model.py
NAMES = ["obstacles_u", "soft_speed"] + [f"generic_{x}_{u}" for x, u in cc.GENERIC_DIMS]
HOST_NAMES = ["obstacles_u", "soft_speed", "generic_3_5"]  # the three costs of the host test


@pytest.mark.parametrize("name", NAMES)
def test_compiles_for_gfx950_without_a_device(name):
    cost = cc.make(name)
    code = cost.compile(arch="gfx950")
    assert isinstance(code, bytes) and len(code) > 1000 and code[:4] == b"\x7fELF"
    assert cost.compile("gfx950:sramecc+:xnack-") is code  # cached per target id; a feature suffix is dropped


def test_uses_u_false_compiles_to_another_code_object():
    a, b = cc.make("obstacles_u", uses_u=True).compile(), cc.make("obstacles_u", uses_u=False).compile()
    assert a[:4] == b[:4] == b"\x7fELF" and a != b


def test_compile_errors_carry_the_compilers_text():
    bad = pmpc_amd.CustomCost("template <class T> __device__ T stage_cost(const T *x, const T *u, const double *p, int j, int N) { return x[0] + ; }", 1, 1, 1)
    with pytest.raises(ValueError, match=r"error: expected expression"):
        bad.compile()
    none = pmpc_amd.CustomCost("__device__ double helper(double a) { return a; }", 2, 1, 1)
    with pytest.raises(ValueError, match=r"error: .*'stage_cost'"):
        none.compile()


@pytest.mark.parametrize("dims", [(0, 1, 1), (17, 1, 1), (1, 0, 1), (1, 17, 1), (1, 1, 0), (1, 1, 65)])
def test_dimensions_outside_the_limits_are_refused(dims):
    with pytest.raises(ValueError, match="outside 1 .. (16|64)"):
        pmpc_amd.CustomCost(cc.SOFT_SPEED_SRC, *dims)
    # the library's own refusal (a caller of the C ABI): nothing is compiled
    code, n, log = ctypes.c_void_p(), ctypes.c_size_t(0), ctypes.create_string_buffer(256)
    rc = _lib.load().pmpc_cost_compile(cc.SOFT_SPEED_SRC.encode(), *dims, 1, b"gfx950", ctypes.byref(code), ctypes.byref(n), log, len(log))
    assert rc == 1 and not code.value and n.value == 0 and b"1 .. 16" in log.value and b"1 .. 64" in log.value


def test_sixty_four_parameters_are_taken():
    src = ("template <class T> __device__ T stage_cost(const T *x, const T *u, const double *p, int j, int N) "
           "{ T c = 0.0; for (int k = 0; k < CD; k++) c += p[k] * x[0]; return c; }")
    assert pmpc_amd.CustomCost(src, 1, 1, 64, uses_u=False).compile()[:4] == b"\x7fELF"


# ---- the test costs under the dual arithmetic, on the host ------------------------------------------------------------------------
HOST_MAIN = r"""
#include <cstdio>
#include "model_dual.h"
#define __device__
using pmpc_dual::Dual;

@COSTS@

template <int X, int U, class F, class G>
static void cost(const char *key, F dual, G plain, const double *xv, const double *uv, const double *p, int j, int N) {
  Dual<X + U> x[X], u[U];
  for (int k = 0; k < X; k++) { x[k] = xv[k]; x[k].d[k] = 1.0; }
  for (int k = 0; k < U; k++) { u[k] = uv[k]; u[k].d[X + k] = 1.0; }
  const Dual<X + U> c = dual(x, u, p, j, N);
  printf("%s %.17g", key, c.v);
  for (int k = 0; k < X + U; k++) printf(" %.17g", c.d[k]);
  printf("\n%s_double %.17g\n", key, plain(xv, uv, p, j, N));
}

int main() {
  double px[16], pu[16], pp[64];
  for (int k = 0; k < 16; k++) { px[k] = 0.3 - 0.11 * k + 0.013 * k * k; pu[k] = 0.2 - 0.07 * k; }
  for (int k = 0; k < 64; k++) pp[k] = 0.9 + 0.05 * k;
@CALLS@
  return 0;
}
"""
J, NST = 2, 7  # the stage and the horizon of the host evaluation


def _host_inputs(dims):
    x, u, cd = dims
    k = np.arange(16)
    px, pu, pp = 0.3 - 0.11 * k + 0.013 * k * k, 0.2 - 0.07 * k, 0.9 + 0.05 * np.arange(64)
    return px[:x], pu[:u], pp[:cd]


@pytest.fixture(scope="module")
def host_values(tmp_path_factory):
    """{key: numbers} as the host program prints them: the test costs under Dual<XD + UD> and under double, compiled with g++."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host test of the custom costs")
    tmp = tmp_path_factory.mktemp("cost_dual")
    costs, calls = "", ""
    for name in HOST_NAMES:
        e = cc.entry(name)
        x, u, cd = e["dims"]
        costs += f"#define XD {x}\n#define UD {u}\n#define CD {cd}\nnamespace c_{name} {{\n{e['src']}\n}}\n#undef XD\n#undef UD\n#undef CD\n"
        calls += (f'  cost<{x}, {u}>("{name}", [](auto... q) {{ return c_{name}::stage_cost(q...); }}, '
                  f"[](auto... q) {{ return c_{name}::stage_cost<double>(q...); }}, px, pu, pp, {J}, {NST});\n")
    (tmp / "main.cpp").write_text(HOST_MAIN.replace("@COSTS@", costs).replace("@CALLS@", calls))
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", str(ROOT / "pmpc_amd" / "csrc"), str(tmp / "main.cpp"), "-o", str(tmp / "cost_host")],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp / "cost_host")], check=True, capture_output=True, text=True).stdout
    return {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in out.splitlines()}


@pytest.mark.parametrize("name", HOST_NAMES)
def test_costs_under_dual_against_closed_forms(host_values, name):
    e = cc.entry(name)
    x, u, cd = e["dims"]
    px, pu, pp = _host_inputs(e["dims"])
    # stage J of a horizon of NST: the closed forms take the stage from axis 1
    X, U = np.tile(px[None, None], (1, NST, 1)), np.tile(pu[None, None], (1, NST, 1))
    val, cx, cu = e["np"](X, U, pp[None])
    got = host_values[name]
    np.testing.assert_allclose(got[0], val[0, J], **TOL)
    np.testing.assert_allclose(got[1:1 + x], cx[0, J], **TOL)
    np.testing.assert_allclose(got[1 + x:], cu[0, J], **TOL)
    np.testing.assert_allclose(host_values[f"{name}_double"][0], val[0, J], **TOL)  # one body, both instantiations
    assert np.abs(cx[0, J]).max() > 1e-3 and np.abs(cu[0, J]).max() > 1e-3  # (the point is not a stationary one)


def test_closed_form_of_obstacles_u_is_the_builtin_obstacle_cost():
    """cw = 0: value and gradient of pmpc_amd.dynamics.obstacle_cost with the same two bumps; a drift is per-stage centres."""
    from pmpc_amd import dynamics as dyn

    rng = np.random.default_rng(3)
    M, N = 3, 5
    X, U = rng.standard_normal((M, N, 4)), rng.standard_normal((M, N, 2))
    cost = dict(kind="obstacles", pos_idx=(0, 1), centres=np.array([[3.0, 0.2], [5.5, 2.5]]) / 4, sigma=np.array([1.0, 1.5]), w=np.array([3.0, 2.0]))
    val, cx, cu = cc.obstacles_u_np(X, U, cc.obstacle_params(cost, M))
    J_ref, cx_ref = dyn.obstacle_cost(X, cost)[:2]
    np.testing.assert_allclose(val.sum(), np.sum(J_ref), **TOL)
    np.testing.assert_allclose(cx, cx_ref, **TOL)
    assert not cu.any()
    moving = np.tile(cost["centres"][None], (N, 1, 1))
    moving[..., 0] += 0.05 * np.arange(N)[:, None]
    np.testing.assert_allclose(cc.obstacles_u_np(X, U, cc.obstacle_params(cost, M), drift=0.05)[1], dyn.obstacle_cost(X, dict(cost, centres=moving))[1], **TOL)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_custom_cost_entry_points_and_agrees_on_the_struct():
    lib = _lib.load()  # must load without a GPU
    for sym in ("pmpc_cost_compile", "pmpc_cost_load", "pmpc_cost_unload", "pmpc_custom_cost_grad_device"):
        assert hasattr(lib, sym) and sym in _lib.ABI_SYMBOLS, sym
    assert ctypes.sizeof(_lib.PmpcScpCost) == lib.pmpc_abi_scp_cost_size()
    # kind 2's members share the storage of the kind-1 members it does not use
    assert _lib.PmpcScpCost.id.offset == _lib.PmpcScpCost.K.offset == 4 and _lib.PmpcScpCost.uses_u.offset == _lib.PmpcScpCost.pos_dim.offset == 8
    assert _lib.PmpcScpCost.cparams.offset == _lib.PmpcScpCost.centres.offset
    sc = _lib.PmpcScpCost(kind=2, id=1003, uses_u=1, cparams=4096)
    assert (sc.kind, sc.id, sc.uses_u, sc.cparams) == (2, 1003, 1, 4096)
    assert pmpc_amd.CustomCost is cc.make("soft_speed").__class__


# ---- the front ends' refusals, before a device is touched ---------------------------------------------------------------------------
class _NoDevice:
    """Stands where a DeviceSolver would: any use of it is a failure of the test (tests/test_warm_shift.py)."""

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came after the solver was touched ({name})")


def _controller_args(M=3, N=4, x=4, u=2):
    eye = lambda d: np.tile(np.eye(d), (M, N, 1, 1))
    return dict(builtin_model="bicycle", params=np.ones((M, 2)), Q=eye(x), R=eye(u), solver_settings=dict(solver="osqp", Nc=1), solver=_NoDevice(),
                device="cpu")


def test_controller_refuses_cost_params_of_the_wrong_shape():
    cost = cc.make("soft_speed")
    for bad in (np.ones((3, 3)), np.ones((2, 4)), np.ones(12)):
        with pytest.raises(ValueError, match=r"params must be \(M, pdim\) = \(3, 4\)"):
            pmpc_amd.MPCController(builtin_cost=dict(kind="custom", cost=cost, params=bad), **_controller_args())


def test_controller_refuses_dimensions_that_disagree_with_the_problem():
    with pytest.raises(ValueError, match="not the cost's dimensions"):
        pmpc_amd.MPCController(builtin_cost=dict(kind="custom", cost=cc.make("generic_3_5"), params=np.ones((3, 8))), **_controller_args())


def test_controller_refuses_a_custom_dict_without_a_custom_cost():
    for cost in (dict(kind="custom", params=np.ones((3, 4))), dict(kind="custom", cost="soft_speed", params=np.ones((3, 4)))):
        with pytest.raises(ValueError, match="needs cost=, a pmpc_amd.CustomCost"):
            pmpc_amd.MPCController(builtin_cost=cost, **_controller_args())
    with pytest.raises(ValueError, match="needs params="):
        pmpc_amd.MPCController(builtin_cost=dict(kind="custom", cost=cc.make("soft_speed")), **_controller_args())


def test_build_problem_checks_a_custom_cost_on_the_cpu():
    from pmpc_amd.device_problem import build_problem

    M, N = 3, 4
    eye = lambda d: np.tile(np.eye(d), (M, N, 1, 1))
    cost = cc.make("soft_speed")
    p = build_problem(eye(4), eye(2), np.zeros((M, 4)), device="cpu", builtin_cost=dict(kind="custom", cost=cost, params=np.ones((M, 4))))
    assert (p.M, p.xdim, p.udim) == (M, 4, 2)
    with pytest.raises(ValueError, match="params must be"):
        build_problem(eye(4), eye(2), np.zeros((M, 4)), device="cpu", builtin_cost=dict(kind="custom", cost=cost, params=np.ones((M, 5))))
    with pytest.raises(ValueError, match="not the cost's dimensions"):
        build_problem(eye(2), eye(1), np.zeros((M, 2)), device="cpu", builtin_cost=dict(kind="custom", cost=cost, params=np.ones((M, 4))))
    with pytest.raises(ValueError, match="needs cost="):
        build_problem(eye(4), eye(2), np.zeros((M, 4)), device="cpu", builtin_cost=dict(kind="custom", cost=None, params=np.ones((M, 4))))
    with pytest.raises(ValueError, match="symmetric"):  # need_sym applies as for the built-in cost
        Qn = eye(4)
        Qn[..., 0, 1] += 0.1
        build_problem(Qn, eye(2), np.zeros((M, 4)), device="cpu", need_sym="builtin_cost needs",
                      builtin_cost=dict(kind="custom", cost=cost, params=np.ones((M, 4))))
