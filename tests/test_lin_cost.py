"""Linearised nonlinear costs, host side: the numpy specification of the built-in obstacle cost (pmpc_amd.dynamics.obstacle_cost), the
host loop's reference shift with it, and the ABI of the device side.  No GPU needed."""
import ctypes

import numpy as np
import pytest


def _cost(rng, pos_dim, per_stage, N, K=3):
    return dict(kind="obstacles", pos_idx=(0, 1, 4)[:pos_dim], centres=rng.standard_normal((N, K, pos_dim) if per_stage else (K, pos_dim)),
                sigma=rng.uniform(0.5, 2.0, K), w=rng.uniform(0.1, 1.0, K))


@pytest.mark.parametrize("pos_dim", [2, 3])
@pytest.mark.parametrize("per_stage", [False, True])
def test_obstacle_cost_gradient_equals_central_differences(pos_dim, per_stage):
    """cx of `obstacle_cost` against central differences of its J, step h = 1e-5, K = 3 obstacles, sigma >= 0.5: rel 1e-6 of the
    largest gradient entry.  The truncation term is h^2 / 6 |J'''| with |J'''| <= a few w / sigma^3 <= 10 here, i.e. ~2e-10, and the
    rounding term eps |J| / h ~ 1e-10; both are far below 1e-6 of a gradient of order w / sigma ~ 0.1 - 1."""
    from pmpc_amd import dynamics as dyn

    rng = np.random.default_rng(10 * pos_dim + per_stage)
    M, N, x, h = 4, 6, 6, 1e-5
    X = rng.standard_normal((M, N, x))
    cost = _cost(rng, pos_dim, per_stage, N)
    J, cx = dyn.obstacle_cost(X, cost)
    assert cx.shape == X.shape and J > 0.0
    fd = np.zeros_like(X)
    for idx in np.ndindex(X.shape):
        Xp, Xm = X.copy(), X.copy()
        Xp[idx] += h
        Xm[idx] -= h
        fd[idx] = (dyn.obstacle_cost(Xp, cost)[0] - dyn.obstacle_cost(Xm, cost)[0]) / (2 * h)
    err = np.abs(fd - cx).max() / np.abs(cx).max()
    print(f"pos_dim {pos_dim} per_stage {per_stage}: max |fd - cx| / max |cx| = {err:.3e}")
    assert err <= 1e-6
    others = [k for k in range(x) if k not in cost["pos_idx"]]
    assert np.all(cx[..., others] == 0.0) and np.abs(cx[..., list(cost["pos_idx"])]).min() > 0.0


def test_torch_twin_of_the_obstacle_cost_equals_numpy():
    import torch

    from pmpc_amd import dynamics as dyn

    rng = np.random.default_rng(3)
    X = rng.standard_normal((3, 5, 4))
    for per_stage in (False, True):
        cost = _cost(rng, 2, per_stage, 5)
        J, cx = dyn.obstacle_cost(X, cost)
        Jt, cxt = dyn.obstacle_cost_torch(torch.tensor(X), cost)
        np.testing.assert_allclose(float(Jt), J, rtol=1e-14)
        np.testing.assert_allclose(cxt.numpy(), cx, rtol=1e-13, atol=1e-15)
        fn = dyn.make_obstacle_lin_cost_fn(cost)
        got, cu = fn(torch.tensor(X), None, None)
        assert cu is None and torch.is_tensor(got) and torch.equal(got, cxt)


def test_bad_cost_descriptions_are_refused():
    from pmpc_amd import dynamics as dyn

    X = np.zeros((2, 3, 4))
    good = dict(pos_idx=(0, 1), centres=np.zeros((2, 2)), sigma=np.ones(2), w=np.ones(2))
    dyn.obstacle_cost(X, good)
    for bad in (dict(good, pos_idx=(0,)), dict(good, pos_idx=(0, 0)), dict(good, centres=np.zeros((4, 2, 2))), dict(good, kind="walls"),
                dict(good, centres=np.zeros((17, 2)), sigma=np.ones(17), w=np.ones(17))):
        with pytest.raises(ValueError):
            dyn.obstacle_cost(X, bad)


def test_host_loop_shift_with_the_obstacle_cost_moves_only_what_q_inverse_reaches():
    """`_augment_cost` with `make_obstacle_lin_cost_fn`: X_ref - Q^-1 cx, cx non-zero in the pos_idx entries only.  With Q coupling
    states (0, 1) to state 2 and nothing to state 3, rows 0 - 2 of the reference move and row 3 stays bit for bit; U_ref is returned
    as it is (cu is None)."""
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.scp_mpc import _augment_cost

    rng = np.random.default_rng(5)
    M, N, x, u = 3, 4, 4, 2
    Qb = np.diag([2.0, 3.0, 1.5, 1.0])
    Qb[0, 2] = Qb[2, 0] = 0.3
    Qb[1, 2] = Qb[2, 1] = -0.2
    Q, R = np.tile(Qb, (M, N, 1, 1)), np.tile(np.eye(u), (M, N, 1, 1))
    X_ref, U_ref = rng.standard_normal((M, N, x)), rng.standard_normal((M, N, u))
    X_prev, U_prev = rng.standard_normal((M, N, x)), rng.standard_normal((M, N, u))
    cost = _cost(rng, 2, False, N)
    Xr, Ur = _augment_cost(dyn.make_obstacle_lin_cost_fn(cost), X_prev, U_prev, Q, R, X_ref, U_ref, {})
    assert Ur is U_ref
    cx = dyn.obstacle_cost(X_prev, cost)[1]
    np.testing.assert_allclose(Xr, X_ref - np.einsum("rt,mnt->mnr", np.linalg.inv(Qb), cx), rtol=0, atol=1e-14)
    assert np.all(Xr[..., 3] == X_ref[..., 3])
    assert np.abs(Xr[..., :3] - X_ref[..., :3]).min() > 0.0


def test_library_exports_the_cost_entry_points_and_agrees_on_the_struct():
    from pmpc_amd import _lib

    lib = _lib.load()  # must load without a GPU
    new = ["pmpc_ref_shift_device", "pmpc_ref_shift_bad_pivots", "pmpc_obstacle_cost_grad_device", "pmpc_obstacle_ref_shift_device",
           "pmpc_scp_loop_device_cost", "pmpc_abi_scp_cost_size"]
    for sym in new:
        assert hasattr(lib, sym), sym
        assert sym in _lib.ABI_SYMBOLS
    assert lib.pmpc_abi_scp_cost_size() == ctypes.sizeof(_lib.PmpcScpCost)
    # the mirror's layout: five ints and the index triple, then three pointers (8-byte aligned)
    assert _lib.PmpcScpCost.pos_idx.offset == 12 and _lib.PmpcScpCost.per_stage.offset == 24 and _lib.PmpcScpCost.centres.offset == 32
    assert ctypes.sizeof(_lib.PmpcScpCost) == 56
