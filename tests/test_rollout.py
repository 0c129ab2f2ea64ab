"""Numpy specifications of the nonlinear rollout and the receding-horizon plan shift (pmpc_amd.dynamics.rollout / shift_plan), and the
two entry points that run them on the device in the library's symbol list.  No GPU."""
import numpy as np
import pytest

from pmpc_amd import dynamics as dyn

MODELS = {"unicycle": dyn.make_unicycle_problem, "quadrotor": dyn.make_quadrotor_problem, "bicycle": dyn.make_bicycle_problem}


def _inputs(name, M, N, seed=11):
    """The model's problem with seeded controls: inside the boxes (unicycle, bicycle), near hover (quadrotor).  The unicycle's turn control
    keeps |u| >= 0.1 inside its box of +-1, as tests/test_device_gpu.py::test_linearize_matches_numpy keeps it: the closed form divides a
    difference of O(1) terms by u2^2 = (w_scale u)^2 (pmpc_amd/dynamics.py: n1 * iu22), so one ulp of sin / cos, 1.1e-16, arrives in f as about
    1.1e-16 |u1| / u2^2 — 4e-14 per ulp at |u| = 0.1 (|u1| <= 1.4, w_scale >= 0.6), but 1e-11 and more below |u| = 0.005, which a uniform
    draw over the box meets once in 200 samples.  A one-step comparison of two sin / cos implementations at 1e-12 is a statement about the
    kernel only where the function itself is conditioned for it."""
    rng = np.random.default_rng(seed)
    prob = MODELS[name](M=M, N=N)
    if name == "quadrotor":
        U = prob["U_ref"] + 0.05 * rng.standard_normal(prob["U_ref"].shape)
    else:
        U = prob["u_l"] + rng.uniform(0.0, 1.0, prob["u_l"].shape) * (prob["u_u"] - prob["u_l"])
    if name == "unicycle":
        U[..., 1] = np.where(U[..., 1] >= 0.0, 1.0, -1.0) * (0.1 + 0.9 * np.abs(U[..., 1]))
        assert np.all(U >= prob["u_l"]) and np.all(U <= prob["u_u"])
    return prob, U


@pytest.mark.parametrize("name", sorted(MODELS))
def test_rollout_has_zero_defect_under_the_model_function(name):
    prob, U = _inputs(name, 5, 7)
    for model in (name, dyn.model_id(name)):
        X = dyn.rollout(model, prob["x0"], U, prob["params"])
        assert X.shape == (5, 7, prob["x0"].shape[-1]) and np.isfinite(X).all()
        X_lin = np.concatenate([prob["x0"][:, None, :], X[:, :-1]], 1)
        np.testing.assert_array_equal(prob["f_fx_fu_fn"](X_lin, U)[0], X)


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("s", [1, 3, 6])
@pytest.mark.parametrize("with_tail", [False, True])
def test_shift_plan_copies_the_head_and_rolls_out_the_tail(name, s, with_tail):
    M, N = 4, 7  # (s = 6 is N - 1: one stage is kept)
    prob, U = _inputs(name, M, N)
    X = dyn.rollout(name, prob["x0"], U, prob["params"])
    U_tail = _inputs(name, M, N, seed=12)[1][:, :s] if with_tail else None
    Xn, Un, um1 = dyn.shift_plan(name, X, U, prob["params"], s=s, U_tail=U_tail)
    assert Xn.shape == X.shape and Un.shape == U.shape
    np.testing.assert_array_equal(Xn[:, :N - s], X[:, s:])
    np.testing.assert_array_equal(Un[:, :N - s], U[:, s:])
    tail = U_tail if with_tail else np.repeat(U[:, -1:], s, 1)
    np.testing.assert_array_equal(Un[:, N - s:], tail)
    np.testing.assert_array_equal(Xn[:, N - s:], dyn.rollout(name, X[:, N - 1], tail, prob["params"]))
    np.testing.assert_array_equal(um1, U[:, s - 1])
    assert um1 is not U and not np.shares_memory(um1, U)


def test_shift_plan_refuses_a_shift_outside_the_horizon():
    prob, U = _inputs("bicycle", 3, 5)
    X = dyn.rollout("bicycle", prob["x0"], U, prob["params"])
    for s in (0, 5, -1, 6):
        with pytest.raises(ValueError):
            dyn.shift_plan("bicycle", X, U, prob["params"], s=s)
    with pytest.raises(ValueError):
        dyn.rollout("tricycle", prob["x0"], U, prob["params"])
    with pytest.raises(ValueError):
        dyn.rollout(3, prob["x0"], U, prob["params"])


def test_rollout_and_shift_entry_points_are_declared_and_exported():
    from pmpc_amd import _lib

    lib = _lib.load()  # must load without a GPU
    for sym in ("pmpc_rollout_device", "pmpc_shift_plan_device"):
        assert sym in _lib.ABI_SYMBOLS
        assert hasattr(lib, sym), sym
    assert len(lib.pmpc_rollout_device.argtypes) == 8 and len(lib.pmpc_shift_plan_device.argtypes) == 12
