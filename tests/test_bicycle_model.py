"""Kinematic bicycle (built-in model 2): the numpy specification `pmpc_amd.dynamics.bicycle` against complex-step differentiation of
its own `f`, and the table of live entries of its compact Jacobian records (pmpc_amd/csrc/jac_compact.h) against that specification.
No GPU: the table is read from the built library on the host."""
import numpy as np
import pytest


def _points(rng, n):
    x = rng.standard_normal((n, 4)) * 2.0
    x[:, 3] = rng.uniform(-8.0, 8.0, n)  # speed, both directions
    u = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.0, 1.0, n)], -1)  # |delta| <= 1.0
    return x, u


def test_bicycle_jacobians_equal_complex_step_derivatives_of_its_own_f():
    """Complex step (h = 1e-30: no subtraction, the derivative is exact to rounding), 200 random points, per-point parameters."""
    from pmpc_amd import dynamics as dyn

    rng = np.random.default_rng(11)
    n, h = 200, 1e-30
    x, u = _points(rng, n)
    p = np.stack([2.7 * (1 + rng.uniform(-0.1, 0.1, n)), rng.uniform(0.05, 0.2, n)], -1)
    f, fx, fu = dyn.bicycle(x, u, p)
    assert f.shape == (n, 4) and fx.shape == (n, 4, 4) and fu.shape == (n, 4, 2) and fx.dtype == np.float64
    # the step itself, written out once more
    L, dt = p[:, 0], p[:, 1]
    f_direct = np.stack([x[:, 0] + dt * x[:, 3] * np.cos(x[:, 2]), x[:, 1] + dt * x[:, 3] * np.sin(x[:, 2]),
                         x[:, 2] + dt * x[:, 3] * np.tan(u[:, 1]) / L, x[:, 3] + dt * u[:, 0]], -1)
    np.testing.assert_allclose(f, f_direct, rtol=0, atol=1e-13)
    err = 0.0
    for t in range(4):
        xc = x.astype(complex)
        xc[:, t] += 1j * h
        err = max(err, float(np.abs(dyn.bicycle(xc, u, p)[0].imag / h - fx[:, :, t]).max()))
    for t in range(2):
        uc = u.astype(complex)
        uc[:, t] += 1j * h
        err = max(err, float(np.abs(dyn.bicycle(x, uc, p)[0].imag / h - fu[:, :, t]).max()))
    print("bicycle: max |closed form - complex step| =", err)
    assert err <= 1e-12


def test_bicycle_torch_equals_the_numpy_specification():
    import torch

    from pmpc_amd import dynamics as dyn

    rng = np.random.default_rng(12)
    x, u = _points(rng, 50)
    p = np.stack([2.7 * (1 + rng.uniform(-0.1, 0.1, 50)), np.full(50, 0.1)], -1)
    ref = dyn.bicycle(x, u, p)
    got = dyn.bicycle_torch(torch.tensor(x), torch.tensor(u), torch.tensor(p))
    for a, b in zip(got, ref):
        np.testing.assert_allclose(a.numpy(), b, rtol=1e-14, atol=1e-14)


def test_entries_the_bicycle_records_hold_constant_are_constant_in_the_numpy_model():
    from pmpc_amd import _lib
    from pmpc_amd import dynamics as dyn

    mx, mu = _lib.jac_live_mask(2, 4, 2)
    assert mx.shape == (4, 4) and mu.shape == (4, 2)
    assert (int(mx.sum()), int(mu.sum())) == (5, 1)
    rng = np.random.default_rng(7)
    for _ in range(3):  # three particles with parameters of their own
        p = np.array([2.7 * (1 + rng.uniform(-0.1, 0.1)), rng.uniform(0.05, 0.2)])
        x, u = _points(rng, 200)
        _, fx, fu = dyn.bicycle(x, u, p[None, :])
        moves_x = np.ptp(fx, axis=0) > 0.0
        moves_u = np.ptp(fu, axis=0) > 0.0
        assert not (moves_x & ~mx).any(), np.argwhere(moves_x & ~mx)
        assert not (moves_u & ~mu).any(), np.argwhere(moves_u & ~mu)
        # and the table is not lazy: every entry it stores per stage does move
        assert (moves_x | ~mx).all() and (moves_u | ~mu).all()


def test_bicycle_records_are_not_offered_for_other_dimensions():
    from pmpc_amd import _lib

    with pytest.raises(ValueError):
        _lib.jac_live_mask(2, 12, 4)
    with pytest.raises(ValueError):
        _lib.jac_live_mask(3, 4, 2)  # the first id that names no model


def test_unicycle_table_is_unchanged_by_a_second_model_of_its_dimensions():
    from pmpc_amd import _lib

    mx, mu = _lib.jac_live_mask(0, 4, 2)
    assert (int(mx.sum()), int(mu.sum())) == (4, 4)
    bx, bu = _lib.jac_live_mask(2, 4, 2)
    assert not (np.array_equal(mx, bx) and np.array_equal(mu, bu))  # same dimensions, another table


def test_make_bicycle_problem_has_the_keys_and_limits_of_the_other_generators():
    from pmpc_amd import dynamics as dyn

    M, N = 5, 9
    prob, ref = dyn.make_bicycle_problem(M=M, N=N, seed=1, Nc=1), dyn.make_unicycle_problem(M=M, N=N, seed=1, Nc=1)
    assert set(prob) == set(ref)
    assert prob["params"].shape == (M, 2) and np.all(prob["params"][:, 1] == 0.1)
    L = prob["params"][:, 0]
    assert np.all(np.abs(L / 2.7 - 1.0) <= 0.1 + 1e-15) and np.ptp(L) > 0.0
    assert np.all(prob["u_u"][..., 0] == 2.0) and np.all(prob["u_u"][..., 1] == 0.5) and np.array_equal(prob["u_l"], -prob["u_u"])
    X_lin = np.concatenate([prob["x0"][:, None, :], prob["X_prev"][:, :-1]], 1)
    f, fx, fu = prob["f_fx_fu_fn"](X_lin, prob["U_prev"])
    assert f.shape == (M, N, 4) and fx.shape == (M, N, 4, 4) and fu.shape == (M, N, 4, 2)
