"""The host mathematics of the smoothed cone objective's Newton iteration (pmpc_amd/csrc/cone_smooth_math.h, used by SmoothSolve in
solver_cone_smooth.hip) without a GPU: the header compiled with g++ into a stand-alone program that prints its results for fixed inputs,
compared with numpy in float64 (the saturating sigmoid and softplus against extended precision).  Every tolerance is a roundoff bound for
the sizes used here, none a measured number."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CAP = 1.001  # 1 + eps: the multipliers' upper end

# ---- inputs ----
W = [0.0, 1e-3, -1e-3, 39.9, -39.9, 40.0, -40.0, float(np.nextafter(40.0, 50.0)), float(np.nextafter(-40.0, -50.0)), 40.1, -40.1, 700.0, -700.0]


def _rows_cases():
    """name -> (lam, J, rho, K): one row; seven random rows; eight rows of which all but two are saturated (|lam| = 30), worst-4."""
    rng = np.random.default_rng(11)
    sat = np.array([30.0, -30.0, 0.3, 30.0, -30.0, -0.2, 30.0, -30.0])
    return {"m1": (np.array([0.4]), np.array([1.7]), 0.5, 0.999), "m7": (rng.standard_normal(7), rng.standard_normal(7), 0.5, 0.999 * 7),
            "m8": (sat, rng.standard_normal(8), 0.5, 0.999 * 4)}


def _system_cases():
    """name -> (M, nc, H upper triangles (lower: NaN), gb, ga, dots, sig, K - sum mu)."""
    rng = np.random.default_rng(12)
    out = {}
    for name, M, nc, kind in [("s3_0", 3, 0, ""), ("s3_1", 3, 1, ""), ("s4_3", 4, 3, ""), ("s2_12", 2, 12, ""), ("cc0", 3, 1, "cc0"), ("pivot", 3, 1, "pivot")]:
        B = rng.standard_normal((M, nc, nc))
        H = B @ np.swapaxes(B, -1, -2) / max(nc, 1) + 0.5 * np.eye(nc)
        if kind == "pivot":
            H = np.zeros((M, nc, nc))
        Hup = np.where(np.triu(np.ones((nc, nc), bool)), H, np.nan)  # [i, r, q]: read only for r <= q
        dots = np.stack([-np.abs(rng.standard_normal(M)), rng.standard_normal(M), np.full(M, np.nan)], -1)  # {-kappa, pi, not read}
        sig = np.zeros(M) if kind else 0.1 + 2.0 * rng.random(M)
        out[name] = (M, nc, H, Hup, rng.standard_normal((M, nc)), rng.standard_normal((M, nc)), dots, sig, float(rng.standard_normal()))
    return out


def _aitken_updates():
    """name -> (rho per update, per update the per-row changes of the logits): three rows inside the hinge, start logits LAM0."""
    c = np.array([0.8, -0.5, 0.3])
    geo = lambda rates: [c * np.prod(rates[:k + 1]) for k in range(len(rates))]
    return {"steady": ([1.0] * 6, geo([1.0] + [0.74] * 5)), "unsteady": ([1.0] * 3, geo([1.0, 0.74, 0.5])), "rho_changed": ([1.0, 1.0, 2.0], geo([1.0, 0.74, 0.74])),
            "capped": ([1.0] * 3, geo([1.0, 0.984, 0.984]))}


LAM0 = np.array([0.5, -1.0, 2.0])


def _arr(name, a):
    vals = ", ".join("NAN" if v != v else repr(float(v)) for v in np.asarray(a, float).ravel())
    return f"static const double {name}[] = {{{vals if vals else '0.0'}}};\n"


def _program():
    src = '#include <cstdio>\n#include "cone_smooth_math.h"\nusing namespace pmpc_smooth;\n'
    src += "static void out(const char *k, const double *v, int n) { printf(\"%s\", k); for (int i = 0; i < n; i++) printf(\" %.17g\", v[i]); printf(\"\\n\"); }\n"
    src += "static void out1(const char *k, double v) { out(k, &v, 1); }\n"
    src += _arr("W", W)
    body = f"  for (int i = 0; i < {len(W)}; i++) {{ const double v[2] = {{sigm(W[i]), softplus(W[i])}}; char k[32]; snprintf(k, 32, \"w%d\", i); out(k, v, 2); }}\n"
    for name, (lam, J, rho, K) in _rows_cases().items():
        src += _arr(f"lam_{name}", lam) + _arr(f"J_{name}", J)
        body += f"""  {{ HingeRows r; r.lam.assign(lam_{name}, lam_{name} + {len(lam)}); r.rho = {rho!r}; r.cap = {CAP!r}; r.K = {K!r};
    const std::vector<double> J(J_{name}, J_{name} + {len(lam)});
    const double guesses[4] = {{NAN, 1e9, -1e9, 0.0}}; double t[5];
    for (int g = 0; g < 4; g++) {{ r.t_guess = guesses[g]; t[g] = r.solve_t(J); }}
    t[4] = r.t_guess; out("t_{name}", t, 5); out1("F_{name}", r.Fval(J, t[0], 0.25)); }}\n"""
    for name, (M, nc, H, Hup, gb, ga, dots, sig, kms) in _system_cases().items():
        src += _arr(f"H_{name}", np.swapaxes(Hup, -1, -2)) + _arr(f"gb_{name}", gb) + _arr(f"ga_{name}", ga) + _arr(f"dots_{name}", dots) + _arr(f"sig_{name}", sig)  # (column-major blocks)
        body += f"""  {{ NewtonSystem sys({M}, {nc}); double coef[{M}] = {{0}};
    const bool ok = sys.solve(H_{name}, gb_{name}, ga_{name}, dots_{name}, sig_{name}, {kms!r}, coef);
    out1("ok_{name}", ok ? 1.0 : 0.0); out("sol_{name}", sys.sol.data(), {nc + 1}); out("coef_{name}", coef, {M}); }}\n"""
    src += _arr("LAM0", LAM0)
    for name, (rhos, deltas) in _aitken_updates().items():
        src += _arr(f"d_{name}", np.array(deltas)) + _arr(f"rho_{name}", rhos)
        body += f"""  {{ Aitken ait(3); std::vector<double> lam(LAM0, LAM0 + 3);
    for (int k = 0; k < {len(rhos)}; k++) {{
      const std::vector<double> before = lam;
      for (int i = 0; i < 3; i++) lam[i] += d_{name}[3 * k + i];
      const Aitken::Outcome o = ait.step(lam, before, rho_{name}[k], {CAP!r});
      const double v[6] = {{o.extrapolated ? 1.0 : 0.0, o.r, o.gain, lam[0] - before[0], lam[1] - before[1], lam[2] - before[2]}};
      char key[32]; snprintf(key, 32, "ait_{name}_%d", k); out(key, v, 6); }} }}\n"""
    return src + "int main() {\n" + body + "  return 0;\n}\n"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """{key: numbers} as the host program prints them."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host test of cone_smooth_math.h")
    tmp = tmp_path_factory.mktemp("smooth_math")
    (tmp / "main.cpp").write_text(_program())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "pmpc_amd" / "csrc"), str(tmp / "main.cpp"), "-o", str(tmp / "smooth_math")],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp / "smooth_math")], check=True, capture_output=True, text=True).stdout
    return {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in out.splitlines()}


def _sigm(w):  # float64, the stable form
    w = np.asarray(w, float)
    e = np.exp(-np.abs(w))
    return np.where(w >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def test_header_needs_neither_hip_nor_the_context():
    text = (ROOT / "pmpc_amd" / "csrc" / "cone_smooth_math.h").read_text()
    assert "hip" not in text.split("#pragma once")[1].replace("solver_cone_smooth.hip", "") and "pmpc_ctx" not in text


def test_sigmoid_and_softplus_to_4_ulp_with_their_cut_offs(host):
    L = np.longdouble
    for i, w in enumerate(W):
        e = np.exp(-abs(L(w)))
        want = np.array([float(1 / (1 + e) if w >= 0 else e / (1 + e)), float(max(L(w), L(0)) + np.log1p(e))])
        assert np.all(np.abs(host[f"w{i}"] - want) <= 4 * np.spacing(want)), (w, host[f"w{i}"], want)
    # what the cut-offs at +-40 rely on: there the saturated form and the full one differ by less than 1e-17 relative (e^-40 = 4.2e-18)
    e = np.exp(L(-40))
    for full, cut in ((1 / (1 + e), L(1)), (e / (1 + e), e), (L(40) + np.log1p(e), L(40)), (np.log1p(e), e)):
        assert abs(cut - full) / full < 1e-17


@pytest.mark.parametrize("name", ["m1", "m7", "m8"])
def test_threshold_solve_meets_the_multiplier_sum_whatever_the_guess(host, name):
    lam, J, rho, K = _rows_cases()[name]
    t = host[f"t_{name}"]
    assert abs(np.sum(CAP * _sigm(lam + (J - t[0]) / rho)) - K) <= 1e-12 * K
    assert t[1] == t[0] and t[2] == t[0]  # a NaN guess and guesses outside the bracket are ignored alike
    assert abs(np.sum(CAP * _sigm(lam + (J - t[3]) / rho)) - K) <= 1e-12 * K and abs(t[3] - t[0]) <= 1e-12 * max(1.0, abs(t[0]))  # (a usable guess: same root)
    assert t[4] == t[3]  # the guess kept for the next solve is where the last one ended
    z = lam + (J - t[0]) / rho
    F = K * t[0] + 0.25 + rho * CAP * np.sum(np.logaddexp(0.0, z) - np.logaddexp(0.0, lam))
    assert abs(host[f"F_{name}"][0] - F) <= 1e-13 * max(1.0, abs(F)) * len(lam)


def _dense(M, nc, H, gb, ga, dots, sig, kms):
    kap, pi = np.maximum(0.0, -dots[:, 0]), dots[:, 1]
    sp = sig / (1.0 + sig * kap)
    A, rhs = np.zeros((nc + 1, nc + 1)), np.zeros(nc + 1)
    A[:nc, :nc] = H.sum(0) + np.einsum("i,ir,iq->rq", sp, ga, ga)
    A[:nc, nc] = A[nc, :nc] = -(sp[:, None] * ga).sum(0)
    A[nc, nc] = sp.sum()
    rhs[:nc] = -(gb + (sp * pi)[:, None] * ga).sum(0)
    rhs[nc] = (sp * pi).sum() - kms
    return A, rhs, kap, pi


@pytest.mark.parametrize("name", ["s3_0", "s3_1", "s4_3", "s2_12"])
def test_newton_system_against_the_dense_solve(host, name):
    M, nc, H, _, gb, ga, dots, sig, kms = _system_cases()[name]
    A, rhs, kap, pi = _dense(M, nc, H, gb, ga, dots, sig, kms)
    sol = np.linalg.solve(A, rhs)
    coef = sig * (pi - sol[nc] + ga @ sol[:nc]) / (1.0 + sig * kap)
    assert host[f"ok_{name}"][0] == 1.0
    assert np.abs(host[f"sol_{name}"] - sol).max() <= 1e-10 * np.abs(sol).max()
    assert np.abs(host[f"coef_{name}"] - coef).max() <= 1e-10 * np.abs(coef).max()


def test_newton_system_without_a_row_inside_leaves_the_threshold(host):
    M, nc, H, _, gb, ga, dots, sig, kms = _system_cases()["cc0"]
    assert host["ok_cc0"][0] == 1.0 and host["sol_cc0"][nc] == 0.0 and np.all(host["coef_cc0"] == 0.0)
    du = np.linalg.solve(H.sum(0), -gb.sum(0))
    assert np.abs(host["sol_cc0"][:nc] - du).max() <= 1e-10 * np.abs(du).max()


def test_newton_system_reports_a_zero_pivot(host):
    assert host["ok_pivot"][0] == 0.0


def test_aitken_sums_a_steady_contraction_and_only_that(host):
    ups = _aitken_updates()
    fired = lambda name: [int(host[f"ait_{name}_{k}"][0]) for k in range(len(ups[name][0]))]
    # two updates to see a ratio, a third to see it steady; after an extrapolation the same again
    assert fired("steady") == [0, 0, 1, 0, 0, 1]
    got = host["ait_steady_2"]
    d = ups["steady"][1][2]
    assert abs(got[1] - 0.74) <= 1e-12 and abs(got[2] - 0.74 / 0.26) <= 1e-11
    # the step taken is the rest of the geometric series: delta + delta r / (1 - r) = delta / (1 - r), the limit
    assert np.abs(got[3:] - d / 0.26).max() <= 1e-12 * np.abs(d / 0.26).max()
    assert fired("unsteady") == [0, 0, 0] and fired("rho_changed") == [0, 0, 0]
    assert fired("capped") == [0, 0, 1] and host["ait_capped_2"][2] == 50.0  # r / (1 - r) = 61.5: capped
