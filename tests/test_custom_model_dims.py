"""The model family of the dimension tests (tests/support/custom_models.py: FAMILY_SRC, nine (x, u, p) cases) without a GPU: every
case compiles for gfx950 through the runtime compiler, the body under Dual<x + u> built with g++ agrees with the float64 torch
restatement the GPU tests use as their reference, and the restated `lin_units` gives the block geometry each case is named for."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.support import custom_models as cm

ROOT = Path(__file__).resolve().parent.parent
TOL = dict(rtol=1e-12, atol=1e-12)  # the tolerance of tests/test_bicycle_gpu.py
UNITS = 16  # (x, u, p) points per case on the host: both sides of every kink of row type 5 occur among them (asserted below)

HOST_MAIN = r"""
#include <cstdio>
#include "model_dual.h"
#define __device__
using pmpc_dual::Dual;

@MODELS@

// `units` points of one case from stdin (x, u, p of each); per point and row: the key, the value, the x + u derivatives
template <int X, int U, int P, class F, class G>
static int model(const char *key, int units, F dual_step, G double_step) {
  for (int n = 0; n < units; n++) {
    double xv[X], uv[U], p[P], xd[X];
    for (int k = 0; k < X; k++) if (scanf("%lf", &xv[k]) != 1) return 1;
    for (int k = 0; k < U; k++) if (scanf("%lf", &uv[k]) != 1) return 1;
    for (int k = 0; k < P; k++) if (scanf("%lf", &p[k]) != 1) return 1;
    Dual<X + U> x[X], u[U], xn[X];
    for (int k = 0; k < X; k++) { x[k] = xv[k]; x[k].d[k] = 1.0; }
    for (int k = 0; k < U; k++) { u[k] = uv[k]; u[k].d[X + k] = 1.0; }
    dual_step(x, u, p, xn);
    double_step(xv, uv, p, xd);
    for (int r = 0; r < X; r++) {
      printf("%s %.17g %.17g", key, xd[r], xn[r].v);
      for (int c = 0; c < X + U; c++) printf(" %.17g", xn[r].d[c]);
      printf("\n");
    }
  }
  return 0;
}

int main() {
  int bad = 0;
@CALLS@
  return bad;
}
"""


def _host_inputs(case):
    """x0 (UNITS, x), U (UNITS, 1, u), P (UNITS, p): UNITS particles of one stage."""
    x0, _, Up, P = cm.family_inputs(cm.FAMILY_CASES[case], UNITS, 1, seed=21)
    return x0, Up, P


@pytest.fixture(scope="module")
def host_values(tmp_path_factory):
    """{case: (UNITS, x, 2 + x + u)}: per point and row, the value of step<double>, then value and derivatives of step<Dual<x + u>>,
    FAMILY_SRC and model_dual.h compiled with g++."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host test of the model family")
    tmp = tmp_path_factory.mktemp("family")
    models, calls, stdin = "", "", []
    for case, (x, u, p) in cm.FAMILY_CASES.items():
        models += f"#define XD {x}\n#define UD {u}\n#define PD {p}\nnamespace m_{case} {{\n{cm.FAMILY_SRC}\n}}\n#undef XD\n#undef UD\n#undef PD\n"
        calls += (f'  bad |= model<{x}, {u}, {p}>("{case}", {UNITS}, [](auto... q) {{ m_{case}::step(q...); }}, '
                  f"[](auto... q) {{ m_{case}::step<double>(q...); }});\n")
        x0, Up, P = _host_inputs(case)
        for n in range(UNITS):
            stdin.append(" ".join(repr(float(v)) for v in np.concatenate([x0[n], Up[n, 0], P[n]])))
    (tmp / "main.cpp").write_text(HOST_MAIN.replace("@MODELS@", models).replace("@CALLS@", calls))
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", str(ROOT / "pmpc_amd" / "csrc"), str(tmp / "main.cpp"), "-o", str(tmp / "family_host")],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp / "family_host")], input="\n".join(stdin) + "\n", check=True, capture_output=True, text=True).stdout
    rows = {}
    for ln in out.splitlines():
        rows.setdefault(ln.split()[0], []).append([float(v) for v in ln.split()[1:]])
    return {case: np.array(rows[case]).reshape(UNITS, x, 2 + x + u) for case, (x, u, _) in cm.FAMILY_CASES.items()}


@pytest.mark.parametrize("case", list(cm.FAMILY_CASES))
def test_every_case_compiles_for_gfx950_without_a_device(case):
    code = cm.make_family(case).compile("gfx950")
    assert isinstance(code, bytes) and len(code) > 1000 and code[:4] == b"\x7fELF"


@pytest.mark.parametrize("case", list(cm.FAMILY_CASES))
def test_torch_reference_against_the_body_under_dual_on_the_host(host_values, case):
    x, u, p = cm.FAMILY_CASES[case]
    x0, Up, P = _host_inputs(case)
    assert cm.family_kink_margin(x0, Up[:, 0]) >= cm.KINK_MARGIN  # (a condition on the inputs)
    f, fx, fu = cm.family_ref(x0[:, None], Up, P)
    got = host_values[case]
    print(f"{case}: max |df| {np.abs(got[..., 1] - f[:, 0]).max():.2e} |dfx| {np.abs(got[..., 2:2 + x] - fx[:, 0]).max():.2e} "
          f"|dfu| {np.abs(got[..., 2 + x:] - fu[:, 0]).max():.2e}")
    np.testing.assert_allclose(got[..., 0], f[:, 0], **TOL)  # step<double>
    np.testing.assert_allclose(got[..., 1], f[:, 0], **TOL)  # step<Dual>: the value
    np.testing.assert_allclose(got[..., 2:2 + x], fx[:, 0], **TOL)
    np.testing.assert_allclose(got[..., 2 + x:], fu[:, 0], **TOL)
    np.testing.assert_array_equal(cm.family_f(x0[:, None], Up, P), f)  # F alone (rollout, plan shift) is the f of the reference
    # the constant row: its value is the last parameter, its derivatives are zeros
    for k in range(7, x, 8):
        np.testing.assert_array_equal(f[:, 0, k], P[:, -1])
        assert not fx[:, 0, k].any() and not fu[:, 0, k].any()


def test_host_points_reach_both_sides_of_every_kink():
    """Row type 5 at the widest case: fabs(b), fmax(b, 0.1), fmin(0.2, c) and fmin(c, d) each take both branches among the points."""
    x0, Up, _ = _host_inputs("every_limit")
    b, c, d = x0[:, 6], Up[:, 0, 5], Up[:, 0, 8]  # row 5: b = x[6], c = u[5], d = u[8]
    for what, side in (("fabs", b > 0), ("fmax", b > 0.1), ("fmin const", c > 0.2), ("fmin", c > d)):
        assert side.any() and not side.all(), what


def test_restated_lin_units_gives_the_geometry_the_cases_are_named_for():
    for case, (x, u, _) in cm.FAMILY_CASES.items():
        assert cm.lin_units(x, u) == cm.FAMILY_UNITS[case], case
    got = {case: (cm.lin_units(x, u), 256 // cm.lin_units(x, u), -(-(x + u) // 4)) for case, (x, u, _) in cm.FAMILY_CASES.items()}
    assert list(got.values()) == [(64, 4, 1), (64, 4, 1), (64, 4, 5), (64, 4, 5), (32, 8, 4), (32, 8, 5), (16, 16, 5), (8, 32, 8), (64, 4, 5)]
    x, u, _ = cm.FAMILY_CASES["units_32_even_record"]
    rec = x + x * x + x * u
    assert rec == 252 and (rec | 1) == 253 and 32 * 253 * 8 == 64768  # the LD = REC | 1 padding where REC is even
    x, u, _ = cm.FAMILY_CASES["second_trip_last_direction_live"]
    assert ((x + x * x + x * u) | 1) == 127 and 64 * 127 * 8 == 65024 and (x + u) % 4 == 1  # the widest record at 64 units; pass 4 holds u[9] alone
    # the restatement's threshold: the record that just fits, and the one that does not
    assert cm.lin_units(16, 16) == 8 and cm.lin_units(16, 15) == 8 and cm.lin_units(7, 1) == 64 and cm.lin_units(8, 8) == 32
