"""Keep-out constraint (include/pmpc_abi.h pmpc_scp_cstr), host side: the numpy specification of csrc/keepout.hip — `keepout_rows`,
`keepout_augment` —, the host loop's `extra_cstrs_fns` helper, the binding and every refusal.  No GPU."""
import ctypes
import types

import numpy as np
import pytest

from pmpc_amd import extra_cstrs as ec


def _cstr(rng, M, N, K, pd, shape, pos_idx=None):
    cshape = {"static": (K, pd), "stage": (N, K, pd), "particle": (M, N, K, pd)}[shape]
    return dict(kind="keepout", pos_idx=tuple(range(pd)) if pos_idx is None else pos_idx, centres=rng.uniform(-1, 1, cshape),
                radius=rng.uniform(0.2, 0.6, K))


def _centre(cstr, M, N, i, j, k):
    c = np.asarray(cstr["centres"])
    return c[k] if c.ndim == 2 else c[j, k] if c.ndim == 3 else c[i, j, k]


@pytest.mark.parametrize("shape", ["static", "stage", "particle"])
@pytest.mark.parametrize("pd", [2, 3])
def test_rows_match_a_direct_loop_and_keep_every_feasible_point_outside_the_ball(shape, pd):
    rng = np.random.default_rng(100 + pd)
    M, N, x, K = 3, 5, 6, 3
    pos_idx = (4, 1, 2)[:pd]
    cstr = _cstr(rng, M, N, K, pd, shape, pos_idx)
    X = rng.uniform(-1, 1, (M, N, x))
    a_x, h = ec.keepout_rows(X, cstr)
    assert a_x.shape == (M, N, K, x) and h.shape == (M, N, K)
    P = rng.uniform(-2, 2, (4000, pd))
    for i in range(M):
        for j in range(N):
            for k in range(K):
                c, r = _centre(cstr, M, N, i, j, k), cstr["radius"][k]
                d = X[i, j, list(pos_idx)] - c
                n = d / np.linalg.norm(d)
                ref = np.zeros(x)
                ref[list(pos_idx)] = -n
                np.testing.assert_allclose(a_x[i, j, k], ref, rtol=0, atol=1e-15)
                assert abs(h[i, j, k] - (-r - n @ c)) < 1e-15
                feas = P @ a_x[i, j, k][list(pos_idx)] <= h[i, j, k]
                assert feas.any() and np.all(np.linalg.norm(P[feas] - c, axis=-1) >= r)  # Cauchy-Schwarz
                # the previous iterate's own side of the ball: pbar + t n is feasible for large t
                assert a_x[i, j, k][list(pos_idx)] @ (c + 2 * r * n) <= h[i, j, k]


def test_degenerate_direction_is_the_first_position_axis():
    rng = np.random.default_rng(7)
    M, N, x = 2, 3, 4
    cstr = _cstr(rng, M, N, 2, 2, "particle", (2, 0))
    X = rng.uniform(-1, 1, (M, N, x))
    X[1, 2, [2, 0]] = cstr["centres"][1, 2, 1]  # exactly on the centre
    X[0, 1, [2, 0]] = cstr["centres"][0, 1, 0] + np.array([3e-13, -4e-13])  # within 1e-12 of it
    a_x, h = ec.keepout_rows(X, cstr)
    for (i, j, k) in ((1, 2, 1), (0, 1, 0)):
        assert np.array_equal(a_x[i, j, k], np.array([0.0, 0.0, -1.0, 0.0]))  # -e of pos_idx[0] = state 2
        assert h[i, j, k] == -cstr["radius"][k] - cstr["centres"][i, j, k][0]
    assert np.isfinite(a_x).all() and np.isfinite(h).all()
    assert not np.array_equal(a_x[0, 0, 0], np.array([0.0, 0.0, -1.0, 0.0]))


@pytest.mark.parametrize("Nc", [0, 1, -1])
@pytest.mark.parametrize("pd", [2, 3])
def test_augment_equals_aux_state_problem_on_the_helpers_tuple(Nc, pd):
    """Entries are sums of at most 3 products of numbers in [-1, 1]: two summation orders differ by a few 1.1e-16; bound 1e-15."""
    rng = np.random.default_rng(200 + pd)
    M, N, x, u, K = 3, 5, 5, 2, 2
    U = lambda *s: rng.uniform(-1, 1, s)
    f, fx, fu, Xp, Xr, x0, Up, Q = U(M, N, x), U(M, N, x, x), U(M, N, x, u), U(M, N, x), U(M, N, x), U(M, x), U(M, N, u), U(M, N, x, x)
    cstr = _cstr(rng, M, N, K, pd, "stage", (3, 0, 1)[:pd])
    cstr["centres"][2, 1] = Xp[1, 2, list(cstr["pos_idx"])]  # one degenerate unit
    for boxes in (False, True):
        x_l, x_u = (U(M, N, x) - 2, U(M, N, x) + 2) if boxes else (None, None)
        tup = ec.make_keepout_extra_cstrs_fn(cstr, Nc)(Xp, Up, None)
        assert len(tup) == 1 and tup[0][0] == M * N * K and tup[0][3].shape[0] == M * N * K
        rows = ec.stage_rows_from_extra_cstrs(tup, M, N, x, u, Nc)
        assert len(rows) == M * N * K and all(r[2] == 0 for r in rows)
        A = ec.aux_state_problem(rows, x0, f, fx, fu, Xp, Up, Q, Xr, 1.3, x_l, x_u)
        B = ec.keepout_augment(cstr, x0, f, fx, fu, Xp, Xr, Q, 1.3, x_l, x_u)
        assert A["m"] == B["m"] == K
        for k in ("x0", "f", "fx", "fu", "X_prev", "Q", "X_ref", "x_l", "x_u"):
            assert A[k].shape == B[k].shape, k
            inf = np.isinf(A[k])
            assert np.array_equal(inf, np.isinf(B[k])) and np.array_equal(A[k][inf], B[k][inf]), k
            err = np.max(np.abs(A[k][~inf] - B[k][~inf]), initial=0.0)
            assert err <= 1e-15, (k, err)
        for k in ("x0", "X_prev", "Q", "X_ref", "x_l"):  # nothing computed in these
            assert np.array_equal(A[k], B[k]), k


def test_bad_descriptions_are_refused():
    X = np.zeros((2, 3, 4))
    good = dict(kind="keepout", pos_idx=(0, 1), centres=np.ones((2, 2)), radius=np.ones(2))
    ec.keepout_rows(X, good)
    for bad in (dict(good, pos_idx=(0,)), dict(good, pos_idx=(0, 0)), dict(good, pos_idx=(0, 4)), dict(good, centres=np.ones((4, 2, 2))),
                dict(good, kind="walls"), dict(good, radius=np.array([1.0, 0.0])), dict(good, centres=np.ones((5, 2)), radius=np.ones(5))):
        with pytest.raises(ValueError):
            ec.keepout_rows(X, bad)


def test_new_symbols_are_exported_and_the_struct_size_agrees():
    import pmpc_amd
    from pmpc_amd import _lib

    for name in ("keepout_rows", "keepout_augment", "make_keepout_extra_cstrs_fn"):
        assert getattr(pmpc_amd, name) is getattr(ec, name)
    lib = _lib.load()  # must load without a GPU
    for sym in ("pmpc_keepout_augment_device", "pmpc_abi_scp_cstr_size"):
        assert hasattr(lib, sym) and sym in _lib.ABI_SYMBOLS, sym
    assert lib.pmpc_abi_scp_cstr_size() == ctypes.sizeof(_lib.PmpcScpCstr) == 56
    assert _lib.PmpcScpCstr.pos_idx.offset == 12 and _lib.PmpcScpCstr.centre_stride_particle.offset == 24 and _lib.PmpcScpCstr.centres.offset == 40
    assert len(lib.pmpc_keepout_augment_device.argtypes) == 17


CSTR = dict(kind="keepout", pos_idx=(0, 1), centres=np.array([[1.0, 0.0]]), radius=np.array([0.5]))


def _solve(**kw):
    import pmpc_amd

    M, N = 2, 4
    Q, R = np.tile(np.eye(4), (M, N, 1, 1)), np.tile(np.eye(2), (M, N, 1, 1))
    args = dict(device="cuda", builtin_model="bicycle", params=np.ones((M, 2)), builtin_cstr=CSTR)
    args.update(kw)
    return pmpc_amd.solve(None, Q, R, np.zeros((M, 4)), **args)


@pytest.mark.parametrize("kw, why", [
    (dict(soc=dict(W=np.eye(2), w0=np.zeros(2), v=np.ones(2), v0=1.0, u_interior=np.zeros(2))), "cones on the controls"),
    (dict(solver_settings=dict(extra_cstrs=[(0, [2], 0, None, None, None, None, None)])), "cones on the controls"),
    (dict(slew_rate=0.1), "slew penalties"),
    (dict(u0_slew=np.zeros(2), solver_settings=dict(slew_reg=1.0)), "slew penalties"),
    (dict(solver_settings=dict(smooth_cstr="squareplus", smooth_alpha=8.0)), "squareplus"),
    (dict(solver=types.SimpleNamespace(world=2)), "sharded context"),
])
def test_the_device_loop_refuses_what_the_constraint_cannot_be_combined_with(kw, why):
    """Each refusal comes before anything touches a device: it is raised on a machine without one."""
    with pytest.raises(ValueError, match=why):
        _solve(**kw)


def test_fp32_jacobians_are_refused():
    import torch

    from pmpc_amd.scp_device import _refuse_with_cstr

    _refuse_with_cstr(jac_dtype=torch.float64)
    with pytest.raises(ValueError, match="fp32 storage"):
        _refuse_with_cstr(jac_dtype=torch.float32)


def test_the_library_loop_and_the_controller_refuse_the_constraint():
    import pmpc_amd
    from pmpc_amd.device import DeviceSolver

    with pytest.raises(ValueError, match="builtin_cstr is not supported"):
        DeviceSolver.scp_loop(None, 2, None, 1, f2=None, fx2=None, fu2=None, builtin_cstr=CSTR)
    M, N = 2, 4
    with pytest.raises(ValueError, match="builtin_cstr is not supported"):
        pmpc_amd.MPCController(builtin_model="bicycle", params=np.ones((M, 2)), Q=np.tile(np.eye(4), (M, N, 1, 1)), R=np.tile(np.eye(2), (M, N, 1, 1)),
                               builtin_cstr=CSTR)
