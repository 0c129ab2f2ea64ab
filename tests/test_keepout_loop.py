"""Keep-out constraints in the library SCP loop and `MPCController`, the parts that need no GPU: the new entry points and the ABI struct
of the augmented buffers, the refusals of `MPCController(keepout=...)` (all raised before a device is touched), and the buffer helper
`pmpc_amd.device_problem.keepout_buffers` against `keepout_static`'s specification on CPU tensors."""
import ctypes
import math
import types

import numpy as np
import pytest

from tests.support.keepout_problems import bicycle_keepout_problem


def test_new_symbols_are_exported_and_the_struct_size_agrees():
    from pmpc_amd import _lib

    lib = _lib.load()  # must load without a GPU
    for sym in ("pmpc_scp_loop_device_cstr", "pmpc_keepout_strip_residual_device", "pmpc_abi_scp_aug_size", "pmpc_scp_loop_follow_ups"):
        assert hasattr(lib, sym) and sym in _lib.ABI_SYMBOLS, sym
    # pmpc_scp_loop_device_cost's 13 arguments + the constraint + the buffers; ctx, xdim, K, udim, N, M + six arrays
    assert len(lib.pmpc_scp_loop_device_cstr.argtypes) == len(lib.pmpc_scp_loop_device_cost.argtypes) + 2 == 15
    assert len(lib.pmpc_keepout_strip_residual_device.argtypes) == 12
    assert lib.pmpc_abi_scp_aug_size() == ctypes.sizeof(_lib.PmpcScpAug) == 16 * 8  # 3 static + 6 pairs + X_out, all pointers
    assert _lib.PmpcScpAug.f.offset == 24 and _lib.PmpcScpAug.xu.offset == 24 + 5 * 16 and _lib.PmpcScpAug.X_out.offset == 120
    assert len(_lib.scp_loop_follow_ups()) == 2  # (a host-side counter: readable without a device)


def _controller(**kw):
    import pmpc_amd

    M, N = 2, 4
    args = dict(builtin_model="bicycle", params=np.ones((M, 2)), Q=np.tile(np.eye(4), (M, N, 1, 1)), R=np.tile(np.eye(2), (M, N, 1, 1)),
                keepout=dict(pos_idx=(0, 1), centres=np.array([[1.0, 0.0]]), radius=np.array([0.5])))
    args.update(kw)
    return pmpc_amd.MPCController(**args)


GOOD = dict(pos_idx=(0, 1), centres=np.ones((2, 2)), radius=np.ones(2))


@pytest.mark.parametrize("kw, why", [
    (dict(soc=dict(W=np.eye(2), w0=np.zeros(2), v=np.ones(2), v0=1.0, u_interior=np.zeros(2))), "cones on the controls"),
    (dict(solver_settings=dict(extra_cstrs=[(0, [2], 0, None, None, None, None, None)])), "cones on the controls"),
    (dict(slew_rate=0.1), "slew penalties"),
    (dict(u0_slew=np.zeros(2), solver_settings=dict(slew_reg=1.0)), "slew penalties"),
    (dict(solver_settings=dict(smooth_cstr="squareplus", smooth_alpha=8.0)), "squareplus"),
    (dict(solver=types.SimpleNamespace(world=2)), "sharded context"),
    (dict(keepout=dict(GOOD, pos_idx=(0,))), "pos_idx"),
    (dict(keepout=dict(GOOD, pos_idx=(0, 0))), "pos_idx"),
    (dict(keepout=dict(GOOD, pos_idx=(0, 4))), "outside the 4 states"),
    (dict(keepout=dict(GOOD, centres=np.ones((5, 2)), radius=np.ones(5))), "1 to 4 balls"),
    (dict(keepout=dict(GOOD, centres=np.ones((3, 2, 2)))), "centres must be"),
    (dict(keepout=dict(GOOD, radius=np.array([1.0, 0.0]))), "radius"),
    (dict(keepout=dict(GOOD, kind="walls")), "walls"),
    (dict(Q=np.tile(np.eye(13), (2, 4, 1, 1)), keepout=dict(pos_idx=(0, 1), centres=np.ones((4, 2)), radius=np.ones(4))), "exceed the solver's 16"),
])
def test_the_controller_refuses_what_the_constraint_cannot_be_combined_with(kw, why):
    """Each refusal comes before anything touches a device: it is raised on a machine without one."""
    with pytest.raises(ValueError, match=why):
        _controller(**kw)


def test_the_old_keyword_names_the_new_one():
    with pytest.raises(ValueError, match="builtin_cstr is not supported.*keepout="):
        _controller(keepout=None, builtin_cstr=dict(GOOD, kind="keepout"))
    from pmpc_amd.device import DeviceSolver

    with pytest.raises(ValueError, match="builtin_cstr is not supported.*cstr="):
        DeviceSolver.scp_loop(None, 2, None, 1, f2=None, fx2=None, fu2=None, builtin_cstr=dict(GOOD, kind="keepout"))


@pytest.mark.parametrize("boxes", [False, True])
def test_buffer_helper_makes_what_keepout_static_specifies(boxes):
    import torch

    from pmpc_amd.device_problem import build_problem, keepout_buffers, keepout_static

    kw, _ = bicycle_keepout_problem(M=3, N=5)
    M, N, x, u, K = 3, 5, 4, 2, 2
    rng = np.random.default_rng(3)
    x_l, x_u = (None, None)
    if boxes:
        x_l, x_u = -1.0 - rng.uniform(size=(M, N, x)), 1.0 + rng.uniform(size=(M, N, x))
        x_l[0, 1, 2], x_u[1, 2, 3] = np.nan, np.nan  # no bound there
    p = build_problem(kw["Q"], kw["R"], kw["x0"], kw["X_ref"], kw["U_ref"], kw["X_prev"], kw["U_prev"], x_l, x_u, kw["u_l"], kw["u_u"], kw["reg_x"],
                      kw["reg_u"], None, None, dict(solver="osqp", Nc=1), None, "bicycle", kw["params"], "cpu")
    xd = x + K
    b = keepout_buffers(p, K)
    st = keepout_static(p, K)
    assert b["K"] == K and len(b["sets"]) == 2 and b["X_out"].shape == (M, N, xd)
    for k in ("Qa", "x0", "lx"):
        assert torch.equal(b[k], st[k]), k
    Qa = b["Qa"].numpy()
    np.testing.assert_array_equal(Qa[..., :x, :x], np.swapaxes(kw["Q"], -1, -2))
    aux = np.arange(x, xd)
    np.testing.assert_array_equal(Qa[..., aux, aux], np.full((M, N, K), -kw["reg_x"]))
    off = Qa.copy()
    off[..., :x, :x] = 0.0
    off[..., aux, aux] = 0.0
    assert not off.any()
    np.testing.assert_array_equal(b["x0"].numpy(), np.concatenate([kw["x0"], np.zeros((M, K))], -1))
    lx = b["lx"].numpy()
    assert np.all(lx[..., x:] == -math.inf)
    np.testing.assert_array_equal(lx[..., :x], np.where(np.isnan(x_l), -math.inf, x_l) if boxes else np.full((M, N, x), -math.inf))
    want_xu = np.where(np.isnan(x_u), math.inf, x_u) if boxes else np.full((M, N, x), math.inf)
    for s in b["sets"]:
        assert s["f"].shape == s["X_prev"].shape == s["X_ref"].shape == s["xu"].shape == (M, N, xd)
        assert s["fx"].shape == (M, N, xd, xd) and s["fu"].shape == (M, N, u, xd)
        np.testing.assert_array_equal(s["xu"].numpy()[..., :x], want_xu)
        assert not np.isnan(s["xu"].numpy()).any()
    assert b["sets"][0]["xu"].data_ptr() != b["sets"][1]["xu"].data_ptr()  # a copy each: the kernel writes the K other entries of both
    one = keepout_buffers(p, K, sets=1)
    assert len(one["sets"]) == 1 and torch.equal(one["sets"][0]["xu"][..., :x], b["sets"][0]["xu"][..., :x])
