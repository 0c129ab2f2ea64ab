"""Custom state constraints without a GPU: the runtime compile for gfx950 (it needs no device), its refusals, the test constraints under the
dual arithmetic of pmpc_amd/csrc/model_dual.h as host C++ against their closed forms, the layout of pmpc_scp_cstr, the numpy
specification of the dense-row augmentation, and the front ends' refusals before a device is touched."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pmpc_amd
from pmpc_amd import _lib
from pmpc_amd import extra_cstrs as ec
from tests.support import custom_cstrs as cg

ROOT = Path(__file__).resolve().parent.parent
TOL = dict(rtol=1e-12, atol=1e-12)  # the tolerance of tests/test_custom_model.py: AD against closed forms
HOST_NAMES = ["balls", "speed_band", "generic_3_3"]  # the three constraints of the host test


@pytest.mark.parametrize("name", cg.NAMES + ["log"])
def test_compiles_for_gfx950_without_a_device(name):
    cstr = cg.make(name)
    code = cstr.compile(arch="gfx950")
    assert isinstance(code, bytes) and len(code) > 1000 and code[:4] == b"\x7fELF"
    assert cstr.compile("gfx950:sramecc+:xnack-") is code  # cached per target id; a feature suffix is dropped


def test_compile_errors_carry_the_compilers_text():
    bad = pmpc_amd.CustomConstraint("template <class T> __device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g) { g[0] = x[0] + ; }", 1, 1, 1)
    with pytest.raises(ValueError, match=r"error: expected expression"):
        bad.compile()
    none = pmpc_amd.CustomConstraint("__device__ double helper(double a) { return a; }", 2, 1, 1)
    with pytest.raises(ValueError, match=r"error: .*'stage_cstr'"):
        none.compile()


@pytest.mark.parametrize("dims", [(0, 1, 1), (16, 1, 1), (1, 0, 1), (1, 5, 1), (13, 4, 1), (15, 2, 1), (1, 1, 0), (1, 1, 65)])
def test_dimensions_outside_the_limits_are_refused(dims):
    with pytest.raises(ValueError, match=r"outside 1 \.\. (16|4|64)|exceeds the solver's 16"):
        pmpc_amd.CustomConstraint(cg.SPEED_BAND_SRC, *dims)
    # the library's own refusal (a caller of the C ABI): nothing is compiled
    code, n, log = ctypes.c_void_p(), ctypes.c_size_t(0), ctypes.create_string_buffer(256)
    rc = _lib.load().pmpc_cstr_compile(cg.SPEED_BAND_SRC.encode(), *dims, b"gfx950", ctypes.byref(code), ctypes.byref(n), log, len(log))
    assert rc == 1 and not code.value and n.value == 0 and b"1 .. 4" in log.value and b"at most 16" in log.value and b"1 .. 64" in log.value


def test_the_limits_themselves_are_taken():
    src = ("template <class T> __device__ void stage_cstr(const T *x, const double *p, int j, int N, T *g) "
           "{ T c = 0.0; for (int k = 0; k < PD; k++) c += p[k] * x[0]; for (int k = 0; k < KD; k++) g[k] = c * x[XD - 1]; }")
    assert pmpc_amd.CustomConstraint(src, 12, 4, 64).compile()[:4] == b"\x7fELF"
    assert pmpc_amd.CustomConstraint(src, 15, 1, 1).compile()[:4] == b"\x7fELF"


# ---- the test constraints under the dual arithmetic, on the host -------------------------------------------------------------------
HOST_MAIN = r"""
#include <cstdio>
#include "model_dual.h"
#define __device__
using pmpc_dual::Dual;

@CSTRS@

template <int X, int K, class F, class G>
static void cstr(const char *key, F dual, G plain, const double *xv, const double *p, int j, int N) {
  Dual<X> x[X], g[K];
  double gd[K];
  for (int k = 0; k < X; k++) { x[k] = xv[k]; x[k].d[k] = 1.0; }
  dual(x, p, j, N, g);
  plain(xv, p, j, N, gd);
  for (int k = 0; k < K; k++) {
    printf("%s_%d %.17g", key, k, g[k].v);
    for (int c = 0; c < X; c++) printf(" %.17g", g[k].d[c]);
    printf("\n%s_%d_double %.17g\n", key, k, gd[k]);
  }
}

int main() {
  double px[16], pp[64];
  for (int k = 0; k < 16; k++) px[k] = 0.3 - 0.11 * k + 0.013 * k * k;
  for (int k = 0; k < 64; k++) pp[k] = 0.9 + 0.05 * k;
@CALLS@
  return 0;
}
"""
J, NST = 2, 7  # the stage and the horizon of the host evaluation


@pytest.fixture(scope="module")
def host_values(tmp_path_factory):
    """{key: numbers} as the host program prints them: the test constraints under Dual<XD> and under double, compiled with g++."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host test of the custom constraints")
    tmp = tmp_path_factory.mktemp("cstr_dual")
    cstrs, calls = "", ""
    for name in HOST_NAMES:
        e = cg.entry(name)
        x, K, pd = e["dims"]
        cstrs += f"#define XD {x}\n#define KD {K}\n#define PD {pd}\nnamespace c_{name} {{\n{e['src']}\n}}\n#undef XD\n#undef KD\n#undef PD\n#undef BALL_PD\n"
        calls += (f'  cstr<{x}, {K}>("{name}", [](auto... q) {{ c_{name}::stage_cstr(q...); }}, '
                  f"[](auto... q) {{ c_{name}::stage_cstr<double>(q...); }}, px, pp, {J}, {NST});\n")
    (tmp / "main.cpp").write_text(HOST_MAIN.replace("@CSTRS@", cstrs).replace("@CALLS@", calls))
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", str(ROOT / "pmpc_amd" / "csrc"), str(tmp / "main.cpp"), "-o", str(tmp / "cstr_host")],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp / "cstr_host")], check=True, capture_output=True, text=True).stdout
    return {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in out.splitlines()}


@pytest.mark.parametrize("name", HOST_NAMES)
def test_constraints_under_dual_against_closed_forms(host_values, name):
    e = cg.entry(name)
    x, K, pd = e["dims"]
    k16 = np.arange(16)
    px, pp = (0.3 - 0.11 * k16 + 0.013 * k16 * k16)[:x], (0.9 + 0.05 * np.arange(64))[:pd]
    g, a = e["np"](np.tile(px[None, None], (1, NST, 1)), pp[None])  # stage J of a horizon of NST: the closed forms take the stage from axis 1
    for k in range(K):
        got = host_values[f"{name}_{k}"]
        np.testing.assert_allclose(got[0], g[0, J, k], **TOL)
        np.testing.assert_allclose(got[1:], a[0, J, k], **TOL)
        np.testing.assert_allclose(host_values[f"{name}_{k}_double"][0], g[0, J, k], **TOL)  # one body, both instantiations
        assert np.abs(a[0, J, k]).max() > 1e-3


def test_closed_form_of_balls_is_the_keepout_rows():
    rng = np.random.default_rng(5)
    M, N = 3, 4
    X = rng.standard_normal((M, N, 4))
    cstr = dict(kind="keepout", pos_idx=(0, 1), centres=rng.uniform(2, 3, (2, 2)), radius=np.array([0.3, 0.5]))
    a, h, _ = cg.rows_np("balls", X, cg.ball_params(cstr, M))
    a_ref, h_ref = ec.keepout_rows(X, cstr)
    np.testing.assert_allclose(a, a_ref, **TOL)
    np.testing.assert_allclose(h, h_ref, **TOL)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_the_struct_keeps_its_layout():
    lib = _lib.load()  # must load without a GPU
    for sym in ("pmpc_cstr_compile", "pmpc_cstr_load", "pmpc_cstr_unload", "pmpc_custom_cstr_rows_device", "pmpc_rows_augment_device", "pmpc_cstr_bad_rows"):
        assert hasattr(lib, sym) and sym in _lib.ABI_SYMBOLS, sym
    S = _lib.PmpcScpCstr
    assert lib.pmpc_abi_scp_cstr_size() == ctypes.sizeof(S) == 56
    assert (S.kind.offset, S.K.offset, S.pos_dim.offset, S.pos_idx.offset) == (0, 4, 8, 12)
    assert (S.centre_stride_particle.offset, S.centre_stride_stage.offset, S.centres.offset, S.radius.offset) == (24, 32, 40, 48)
    # kind 2's members share the storage of the kind-1 members it does not use
    assert S.id.offset == S.pos_dim.offset and S.gparams.offset == S.centres.offset
    sc = S(kind=2, K=3, id=1003, gparams=4096)
    assert (sc.kind, sc.K, sc.id, sc.gparams) == (2, 3, 1003, 4096) and (sc.pos_dim, sc.centres) == (1003, 4096)
    assert pmpc_amd.CustomConstraint is cg.make("speed_band").__class__


# ---- the numpy specification ----------------------------------------------------------------------------------------------------------
def _rand_lin(rng, M, N, x, u, K):
    f, fx, fu = rng.standard_normal((M, N, x)), rng.standard_normal((M, N, x, x)), rng.standard_normal((M, N, x, u))
    X_prev, U_prev, X_ref = rng.standard_normal((M, N, x)), rng.standard_normal((M, N, u)), rng.standard_normal((M, N, x))
    Q = rng.standard_normal((M, N, x, x))
    x0, x_l, x_u = rng.standard_normal((M, x)), -1.0 - rng.random((M, N, x)), 1.0 + rng.random((M, N, x))
    return dict(x0=x0, f=f, fx=fx, fu=fu, X_prev=X_prev, U_prev=U_prev, Q=Q, X_ref=X_ref, x_l=x_l, x_u=x_u)


@pytest.mark.parametrize("shape", [(2, 3, 4, 2, 2), (1, 1, 12, 4, 4)])
def test_rows_augment_is_aux_state_problem_with_the_rows_in_form_0(shape):
    M, N, x, u, K = shape
    rng = np.random.default_rng(11)
    d = _rand_lin(rng, M, N, x, u, K)
    a, h = rng.standard_normal((M, N, K, x)), rng.standard_normal((M, N, K))
    got = ec.rows_augment(a, h, d["x0"], d["f"], d["fx"], d["fu"], d["X_prev"], d["X_ref"], d["Q"], 0.7, d["x_l"], d["x_u"])
    rows = [(i, j, 0, a[i, j, k], np.zeros(u), float(h[i, j, k])) for i in range(M) for j in range(N) for k in range(K)]
    ref = ec.aux_state_problem(rows, d["x0"], d["f"], d["fx"], d["fu"], d["X_prev"], d["U_prev"], d["Q"], d["X_ref"], 0.7, d["x_l"], d["x_u"])
    assert got["m"] == ref["m"] == K
    for key in ("x0", "f", "fx", "fu", "X_prev", "Q", "X_ref", "x_l", "x_u"):
        np.testing.assert_allclose(got[key], ref[key], rtol=1e-13, atol=1e-13, err_msg=key)


@pytest.mark.parametrize("shape", [(2, 3, 4, 2, 2), (1, 1, 12, 4, 4)])
def test_rows_augment_is_keepout_augment_on_the_keepout_rows(shape):
    M, N, x, u, K = shape
    rng = np.random.default_rng(12)
    d = _rand_lin(rng, M, N, x, u, K)
    cstr = dict(kind="keepout", pos_idx=(1, 0, 3)[:2 + (x > 4)], centres=rng.standard_normal((K, 2 + (x > 4))), radius=0.1 + rng.random(K))
    a, h = ec.keepout_rows(d["X_prev"], cstr)
    got = ec.rows_augment(a, h, d["x0"], d["f"], d["fx"], d["fu"], d["X_prev"], d["X_ref"], d["Q"], 0.7, d["x_l"], d["x_u"])
    ref = ec.keepout_augment(cstr, d["x0"], d["f"], d["fx"], d["fu"], d["X_prev"], d["X_ref"], d["Q"], 0.7, d["x_l"], d["x_u"])
    for key in ("x0", "f", "fx", "fu", "X_prev", "Q", "X_ref", "x_l", "x_u"):
        assert np.array_equal(got[key], ref[key]), key


def test_rows_extra_cstrs_fn_holds_the_linearised_rows():
    M, N, Nc = 2, 3, 1
    X, P = cg.rand_inputs("generic_3_3", M, N, seed=2)
    fn = cg.entry("generic_3_3")["np"]
    tup = ec.make_rows_extra_cstrs_fn(lambda Z: fn(Z, P)[0], lambda Z: fn(Z, P)[1], Nc)(X, np.zeros((M, N, 2)))[0]
    a, h, g = cg.rows_np("generic_3_3", X, P)
    ncu = Nc * 2 + M * (N - Nc) * 2
    assert tup[0] == M * N * 3 and tup[3].shape == (M * N * 3, ncu + M * N * 3)
    z = np.concatenate([np.zeros(ncu), X.reshape(-1)])
    np.testing.assert_allclose(tup[3] @ z - tup[5], g.reshape(-1), **TOL)  # G z - h at the iterate is g
    np.testing.assert_allclose(tup[5], h.reshape(-1), **TOL)


# ---- the front ends' refusals, before a device is touched ---------------------------------------------------------------------------
class _NoDevice:
    """Stands where a DeviceSolver would: any use of it but a look at the (host-side) shard count is a failure of the test."""
    world = 1

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came after the solver was touched ({name})")


def _controller_args(M=3, N=4, x=4, u=2, **over):
    eye = lambda d: np.tile(np.eye(d), (M, N, 1, 1))
    return dict(dict(builtin_model="bicycle", params=np.ones((M, 2)), Q=eye(x), R=eye(u), solver_settings=dict(solver="osqp", Nc=1), solver=_NoDevice(),
                     device="cpu"), **over)


def test_controller_refuses_params_of_the_wrong_shape_and_foreign_dimensions():
    band = cg.make("speed_band")
    for bad in (np.ones((3, 2)), np.ones((2, 3)), np.ones(9)):
        with pytest.raises(ValueError, match=r"params must be \(M, pdim\) = \(3, 3\)"):
            pmpc_amd.MPCController(constraint=dict(cstr=band, params=bad), **_controller_args())
    with pytest.raises(ValueError, match="not the constraint's dimensions"):
        pmpc_amd.MPCController(constraint=dict(cstr=cg.make("generic_3_3"), params=np.ones((3, 6))), **_controller_args())
    with pytest.raises(ValueError, match="needs cstr=, a pmpc_amd.CustomConstraint"):
        pmpc_amd.MPCController(constraint=dict(cstr="speed_band", params=np.ones((3, 3))), **_controller_args())
    with pytest.raises(ValueError, match="needs params="):
        pmpc_amd.MPCController(constraint=dict(cstr=band), **_controller_args())


def test_controller_refuses_the_constraint_next_to_keepout_and_warm_shift():
    con = dict(cstr=cg.make("speed_band"), params=np.ones((3, 3)))
    keepout = dict(pos_idx=(0, 1), centres=np.zeros((1, 2)), radius=np.array([0.1]))
    with pytest.raises(ValueError, match="constraint= is not supported next to keepout="):
        pmpc_amd.MPCController(constraint=con, keepout=keepout, **_controller_args())
    with pytest.raises(ValueError, match="warm_shift=True is not supported next to constraint="):
        pmpc_amd.MPCController(constraint=con, warm_shift=True, u_l=-np.ones((3, 4, 2)), u_u=np.ones((3, 4, 2)), **_controller_args())
    with pytest.raises(ValueError, match="slew penalties"):  # what keepout= is refused with
        pmpc_amd.MPCController(constraint=con, slew_rate=0.1, **_controller_args())


def test_solve_refuses_a_custom_constraint_before_a_device_is_touched():
    M, N = 3, 4
    eye = lambda d: np.tile(np.eye(d), (M, N, 1, 1))
    band = cg.make("speed_band")
    kw = dict(device="cuda", builtin_model="bicycle", params=np.ones((M, 2)), solver=_NoDevice())
    with pytest.raises(ValueError, match="params must be"):
        pmpc_amd.solve(None, eye(4), eye(2), np.zeros((M, 4)), builtin_cstr=dict(kind="custom", cstr=band, params=np.ones((M, 4))), **kw)
    with pytest.raises(ValueError, match="not the constraint's dimensions"):
        pmpc_amd.solve(None, eye(3), eye(2), np.zeros((M, 3)), builtin_cstr=dict(kind="custom", cstr=band, params=np.ones((M, 3))), **kw)
    with pytest.raises(ValueError, match="cones on the controls"):
        pmpc_amd.solve(None, eye(4), eye(2), np.zeros((M, 4)), builtin_cstr=dict(kind="custom", cstr=band, params=np.ones((M, 3))),
                       soc=dict(W=np.eye(2), w0=np.zeros(2), v=np.zeros(2), v0=1.0), **kw)


def test_the_keepout_kind_check_names_the_custom_route():
    with pytest.raises(ValueError, match="CustomConstraint"):
        ec._keepout_arrays(dict(kind="corridor", pos_idx=(0, 1), centres=np.zeros((1, 2)), radius=np.ones(1)), 1, 1)
