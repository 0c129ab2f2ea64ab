"""Custom dynamics models without a GPU: the runtime compile for gfx950 (it needs no device), its refusals, the dual arithmetic of
pmpc_amd/csrc/model_dual.h as host C++ against closed forms, and the controller's refusals before a device is touched."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pmpc_amd
from tests.support import custom_models as cm

ROOT = Path(__file__).resolve().parent.parent
TOL = dict(rtol=1e-12, atol=1e-12)  # the tolerance of tests/test_bicycle_gpu.py


@pytest.mark.parametrize("name", sorted(cm.SOURCES))
def test_compiles_for_gfx950_without_a_device(name):
    model = cm.make(name)
    code = model.compile(arch="gfx950")
    assert isinstance(code, bytes) and len(code) > 1000 and code[:4] == b"\x7fELF"
    assert model.compile("gfx950:sramecc+:xnack-") is code  # cached per target id; a feature suffix is dropped


def test_compile_errors_carry_the_compilers_text():
    bad = pmpc_amd.CustomModel("template <class T> __device__ void step(const T *x, const T *u, const double *p, T *xn) { xn[0] = x[0] + ; }", 1, 1, 1)
    with pytest.raises(ValueError, match=r"error: expected expression"):
        bad.compile()
    none = pmpc_amd.CustomModel("__device__ double helper(double a) { return a; }", 2, 1, 1)
    with pytest.raises(ValueError, match=r"error: .*'step'"):
        none.compile()


@pytest.mark.parametrize("dims", [(0, 1, 1), (17, 1, 1), (1, 0, 1), (1, 17, 1), (1, 1, 0), (1, 1, 17)])
def test_dimensions_outside_the_solvers_limits_are_refused(dims):
    import ctypes

    from pmpc_amd import _lib

    with pytest.raises(ValueError, match="outside 1 .. 16"):
        pmpc_amd.CustomModel(cm.PENDULUM_SRC, *dims)
    # the library's own refusal (a caller of the C ABI): nothing is compiled
    code, n, log = ctypes.c_void_p(), ctypes.c_size_t(0), ctypes.create_string_buffer(256)
    rc = _lib.load().pmpc_model_compile(cm.PENDULUM_SRC.encode(), *dims, b"gfx950", ctypes.byref(code), ctypes.byref(n), log, len(log))
    assert rc == 1 and not code.value and n.value == 0 and b"1 .. 16" in log.value


# ---- the dual arithmetic on the host ---------------------------------------------------------------------------------------------
A, B = 0.7, -1.3  # a carries direction 0, b direction 1

HOST_MAIN = r"""
#include <cstdio>
#include "model_dual.h"
#define __device__
using pmpc_dual::Dual;
typedef Dual<2> D2;

static void show(const char *key, const D2 &r) { printf("%s %.17g %.17g %.17g\n", key, r.v, r.d[0], r.d[1]); }
template <class T>
static T both(T x) { return sin(x) * fmax(x, 0.5) + pow(x, 2.0) + fabs(x) + atan2(x, T(2.0)) + fmin(x, 5.0) / 3.0 - exp(-x) + log(x) * sqrt(x) + tanh(x) + atan(x) + cos(x) * tan(x); }

@MODELS@

template <int X, int U, class F>
static void model(const char *key, F f, const double *xv, const double *uv, const double *p) {
  Dual<X + U> x[X], u[U], xn[X];
  for (int k = 0; k < X; k++) { x[k] = xv[k]; x[k].d[k] = 1.0; }
  for (int k = 0; k < U; k++) { u[k] = uv[k]; u[k].d[X + k] = 1.0; }
  f(x, u, p, xn);
  for (int r = 0; r < X; r++) {
    printf("%s.%d %.17g", key, r, xn[r].v);
    for (int c = 0; c < X + U; c++) printf(" %.17g", xn[r].d[c]);
    printf("\n");
  }
}

int main() {
  D2 a(@A@), b(@B@);
  a.d[0] = 1.0;
  b.d[1] = 1.0;
  show("add", a + b); show("sub", a - b); show("mul", a * b); show("div", a / b);
  show("add_c", a + 2.5); show("c_add", 2.5 + a); show("sub_c", a - 2.5); show("c_sub", 2.5 - a);
  show("mul_c", a * 2.5); show("c_mul", 2.5 * a); show("div_c", a / 2.5); show("c_div", 2.5 / a);
  show("neg", -a); show("int_mul", 2 * a);
  D2 c = a; c += b; c *= a; c -= 2.0; c /= b; c += 1.0; c *= 3.0; c /= 2.0; c -= a;
  show("compound", c);
  show("sin", sin(a)); show("cos", cos(a)); show("tan", tan(a)); show("exp", exp(a)); show("log", log(a)); show("sqrt", sqrt(a));
  show("tanh", tanh(a)); show("atan", atan(a)); show("atan2", atan2(a, b)); show("atan2_c", atan2(a, 2.0)); show("c_atan2", atan2(2.0, b));
  show("pow", pow(a, 2.5)); show("fabs_neg", fabs(b)); show("fabs_pos", fabs(a));
  show("fmin", fmin(a, b)); show("fmax", fmax(a, b)); show("fmin_c", fmin(a, 0.5)); show("fmax_c", fmax(a, 0.5));
  show("c_fmin", fmin(0.5, b)); show("c_fmax", fmax(0.5, b));
  // kinks: the branch of the value
  D2 z(0.0); z.d[0] = 1.0;
  show("fabs_kink", fabs(z));
  D2 t(@A@); t.d[1] = 1.0;  // the value of a, another direction: a tie
  show("fmin_tie", fmin(a, t)); show("fmax_tie", fmax(a, t));
  printf("cmp %d %d %d %d %d %d %d %d\n", a < b, a > b, a <= @A@, a == @A@, b != a, a >= b, 0.0 < a, b >= 0.0);
  // one body, both instantiations
  show("both_dual", both(a));
  printf("both_double %.17g 0 0\n", both(@A@));
  double px[16], pu[16], pp[16];
  for (int k = 0; k < 16; k++) { px[k] = 0.3 - 0.11 * k + 0.013 * k * k; pu[k] = 0.2 - 0.07 * k; pp[k] = 0.9 + 0.05 * k; }
  pp[1] = 0.1;
  model<4, 2>("bicycle", [](auto... q) { m_bicycle::step(q...); }, px, pu, pp);
  model<2, 1>("pendulum", [](auto... q) { m_pendulum::step(q...); }, px, pu, pp);
  model<9, 3>("ring", [](auto... q) { m_ring::step(q...); }, px, pu, pp);
  double xn[9];
  m_ring::step<double>(px, pu, pp, xn);
  printf("ring_double");
  for (int k = 0; k < 9; k++) printf(" %.17g", xn[k]);
  printf("\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def host_values(tmp_path_factory):
    """{key: numbers} as the host program prints them: model_dual.h compiled with g++, the three test models under Dual."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host test of model_dual.h")
    tmp = tmp_path_factory.mktemp("dual")
    models = ""
    for name, (src, (x, u, p)) in cm.SOURCES.items():
        models += f"#define XD {x}\n#define UD {u}\n#define PD {p}\nnamespace m_{name} {{\n{src}\n}}\n#undef XD\n#undef UD\n#undef PD\n"
    text = HOST_MAIN.replace("@MODELS@", models).replace("@A@", repr(A)).replace("@B@", repr(B))
    (tmp / "main.cpp").write_text(text)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", str(ROOT / "pmpc_amd" / "csrc"), str(tmp / "main.cpp"), "-o", str(tmp / "dual_host")],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp / "dual_host")], check=True, capture_output=True, text=True).stdout
    return {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in out.splitlines()}


def _closed_forms():
    a, b = A, B
    r2 = a * a + b * b
    sec2 = 1.0 / np.cos(a) ** 2
    return {
        "add": (a + b, 1, 1), "sub": (a - b, 1, -1), "mul": (a * b, b, a), "div": (a / b, 1 / b, -a / b ** 2),
        "add_c": (a + 2.5, 1, 0), "c_add": (2.5 + a, 1, 0), "sub_c": (a - 2.5, 1, 0), "c_sub": (2.5 - a, -1, 0),
        "mul_c": (2.5 * a, 2.5, 0), "c_mul": (2.5 * a, 2.5, 0), "div_c": (a / 2.5, 1 / 2.5, 0), "c_div": (2.5 / a, -2.5 / a ** 2, 0),
        "neg": (-a, -1, 0), "int_mul": (2 * a, 2, 0),
        "sin": (np.sin(a), np.cos(a), 0), "cos": (np.cos(a), -np.sin(a), 0), "tan": (np.tan(a), sec2, 0), "exp": (np.exp(a), np.exp(a), 0),
        "log": (np.log(a), 1 / a, 0), "sqrt": (np.sqrt(a), 0.5 / np.sqrt(a), 0), "tanh": (np.tanh(a), 1 - np.tanh(a) ** 2, 0),
        "atan": (np.arctan(a), 1 / (1 + a * a), 0), "atan2": (np.arctan2(a, b), b / r2, -a / r2),
        "atan2_c": (np.arctan2(a, 2.0), 2.0 / (a * a + 4.0), 0), "c_atan2": (np.arctan2(2.0, b), 0, -2.0 / (b * b + 4.0)),
        "pow": (a ** 2.5, 2.5 * a ** 1.5, 0), "fabs_neg": (-b, 0, -1), "fabs_pos": (a, 1, 0),
        "fmin": (b, 0, 1), "fmax": (a, 1, 0), "fmin_c": (0.5, 0, 0), "fmax_c": (a, 1, 0), "c_fmin": (b, 0, 1), "c_fmax": (0.5, 0, 0),
        "fabs_kink": (0.0, 1, 0), "fmin_tie": (a, 1, 0), "fmax_tie": (a, 1, 0),
        # c = a; c += b; c *= a; c -= 2; c /= b; c += 1; c *= 3; c /= 2; c -= a
        "compound": ((((a + b) * a - 2.0) / b + 1.0) * 1.5 - a, 1.5 * (2 * a + b) / b - 1.0, 1.5 * (2.0 - a * a) / b ** 2),
    }


def test_dual_arithmetic_against_closed_forms(host_values):
    for key, want in _closed_forms().items():
        np.testing.assert_allclose(host_values[key], np.array(want, float), err_msg=key, **TOL)
    # comparisons go by value
    assert host_values["cmp"].tolist() == [float(v) for v in (A < B, A > B, True, True, True, A >= B, True, False)]


def test_one_body_serves_double_and_dual(host_values):
    a = A
    want = (np.sin(a) * max(a, 0.5) + a ** 2 + abs(a) + np.arctan2(a, 2.0) + min(a, 5.0) / 3.0 - np.exp(-a) + np.log(a) * np.sqrt(a) + np.tanh(a)
            + np.arctan(a) + np.cos(a) * np.tan(a))
    d = (np.cos(a) * a + np.sin(a) + 2 * a + 1.0 + 2.0 / (a * a + 4.0) + 1.0 / 3.0 + np.exp(-a) + np.sqrt(a) / a + np.log(a) * 0.5 / np.sqrt(a)
         + 1 - np.tanh(a) ** 2 + 1 / (1 + a * a) + (-np.sin(a) * np.tan(a) + np.cos(a) / np.cos(a) ** 2))
    np.testing.assert_allclose(host_values["both_dual"], [want, d, 0.0], **TOL)
    np.testing.assert_allclose(host_values["both_double"][0], want, **TOL)


@pytest.mark.parametrize("name", sorted(cm.SOURCES))
def test_models_under_dual_against_closed_forms(host_values, name):
    x, u, p = cm.SOURCES[name][1]
    k = np.arange(16)
    px, pu, pp = 0.3 - 0.11 * k + 0.013 * k * k, 0.2 - 0.07 * k, 0.9 + 0.05 * k
    pp[1] = 0.1
    f, fx, fu = cm.CLOSED_FORMS[name](px[None, None, :x], pu[None, None, :u], pp[None, :p])
    got = np.stack([host_values[f"{name}.{r}"] for r in range(x)])
    np.testing.assert_allclose(got[:, 0], f[0, 0], **TOL)
    np.testing.assert_allclose(got[:, 1:1 + x], fx[0, 0], **TOL)
    np.testing.assert_allclose(got[:, 1 + x:], fu[0, 0], **TOL)
    if name == "ring":
        np.testing.assert_allclose(host_values["ring_double"], f[0, 0], **TOL)


# ---- the controller's refusals, before a device is touched ------------------------------------------------------------------------
class _NoDevice:
    """Stands where a DeviceSolver would: any use of it is a failure of the test (tests/test_warm_shift.py)."""

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came after the solver was touched ({name})")


def _controller_args(M=3, N=4, x=4, u=2):
    eye = lambda d: np.tile(np.eye(d), (M, N, 1, 1))
    return dict(Q=eye(x), R=eye(u), solver_settings=dict(solver="osqp", Nc=1), solver=_NoDevice(), device="cpu")


def test_controller_refuses_params_of_the_wrong_width():
    with pytest.raises(ValueError, match=r"params must be \(M, pdim\) = \(3, 2\)"):
        pmpc_amd.MPCController(builtin_model=cm.make("bicycle"), params=np.ones((3, 3)), **_controller_args())


def test_controller_refuses_dimensions_that_disagree_with_Q():
    with pytest.raises(ValueError, match="not the model's dimensions"):
        pmpc_amd.MPCController(builtin_model=cm.make("pendulum"), params=np.ones((3, 3)), **_controller_args())
    with pytest.raises(ValueError, match="not the model's dimensions"):  # (R: the bicycle has two controls)
        pmpc_amd.MPCController(builtin_model=cm.make("bicycle"), params=np.ones((3, 2)), **_controller_args(u=3))


def test_build_problem_checks_a_custom_model_on_the_cpu():
    from pmpc_amd.device_problem import build_problem

    M, N = 3, 4
    eye = lambda d: np.tile(np.eye(d), (M, N, 1, 1))
    model = cm.make("pendulum")
    p = build_problem(eye(2), eye(1), np.zeros((M, 2)), builtin_model=model, params=np.ones((M, 3)), device="cpu")
    assert p.model is model and tuple(p.params.shape) == (M, 3)
    with pytest.raises(ValueError, match="params must be"):
        build_problem(eye(2), eye(1), np.zeros((M, 2)), builtin_model=model, params=np.ones((M, 2)), device="cpu")
    with pytest.raises(ValueError, match="not the model's dimensions"):
        build_problem(eye(4), eye(2), np.zeros((M, 4)), builtin_model=model, params=np.ones((M, 3)), device="cpu")


def test_earlier_refusals_stand():
    with pytest.raises(ValueError, match="needs builtin_model"):
        pmpc_amd.MPCController(builtin_model=None, params=np.ones((3, 2)), **_controller_args())
    with pytest.raises(ValueError, match="unknown built-in model"):
        pmpc_amd.MPCController(builtin_model="tricycle", params=np.ones((3, 2)), **_controller_args())
