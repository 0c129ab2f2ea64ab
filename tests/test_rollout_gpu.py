"""Nonlinear rollout and receding-horizon plan shift of the built-in models on the GPU (k_rollout, k_shift_plan of
pmpc_amd/csrc/dynamics.hip) against their numpy specifications, pmpc_amd.dynamics.rollout / shift_plan.

The kernels are compared ONE STEP at a time: X_dev[j] against F_np(X_dev[j - 1], U[j]) with rtol = atol = 1e-12, the tolerance
tests/test_bicycle_gpu.py applies to the same functions — a whole-horizon comparison would let the last bits of sin / cos compound
(measured on an MI355X: quadrotor (130, 33) 3.6e-8 against the numpy rollout, 7.1e-15 one step at a time).  Measured one-step differences over
the four shapes: bicycle 1.8e-15, quadrotor 7.1e-15, unicycle 1.6e-14 (inputs: tests/test_rollout.py::_inputs); `f` of `linearize` at the
rolled-out iterate was bit-equal to it in all twelve cases."""
import ctypes

import numpy as np
import pytest

from tests.test_rollout import MODELS, _inputs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 2), (67, 9), (130, 33)]  # partial waves, more than one block, N odd and no multiple of a staging depth
TOL = dict(rtol=1e-12, atol=1e-12)


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def solver():
    from pmpc_amd.device import DeviceSolver

    s = DeviceSolver(0)
    yield s
    s.close()


def _one_step(prob, x_first, X, U):
    """F_np([x_first, X[:-1]][j], U[j]) for every stage j at once."""
    X_lin = np.concatenate([x_first[:, None, :], X[:, :-1]], 1)
    return prob["f_fx_fu_fn"](X_lin, U)[0]


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("M,N", SHAPES)
def test_rollout_equals_the_specification_step_by_step_and_is_feasible_for_linearize(solver, name, M, N):
    import torch

    from pmpc_amd import dynamics as dyn

    prob, U = _inputs(name, M, N)
    X_np = dyn.rollout(name, prob["x0"], U, prob["params"])
    assert np.isfinite(X_np).all()  # (a condition on the inputs, not on the kernel)
    mid = dyn.model_id(name)
    x0, Ud, P = _dev(prob["x0"]), _dev(U), _dev(prob["params"])
    X_dev = solver.rollout(mid, x0, Ud, P)
    solver.sync()
    X = X_dev.cpu().numpy()
    assert X.shape == X_np.shape and np.isfinite(X).all()
    want = _one_step(prob, prob["x0"], X, U)
    print(f"{name} ({M}, {N}): one-step max abs difference {np.abs(X - want).max():.3e}; against the numpy rollout {np.abs(X - X_np).max():.3e}")
    np.testing.assert_allclose(X, want, **TOL)
    # feasibility through the library's own linearisation: f at (x0, X_prev = X_dev, U) is X_dev
    f, _, _ = solver.linearize(mid, x0, X_dev, Ud, P)
    solver.sync()
    print(f"{name} ({M}, {N}): f of linearize bit-equal to the rollout: {bool(torch.equal(f, X_dev))}; max abs defect {float((f - X_dev).abs().max()):.3e}")
    np.testing.assert_allclose(f.cpu().numpy(), X, **TOL)


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("s", [1, 2, 8])
@pytest.mark.parametrize("with_tail", [False, True])
def test_shift_plan_copies_exactly_rolls_out_the_tail_and_stays_inside_its_buffers(solver, name, s, with_tail):
    import torch

    from pmpc_amd import dynamics as dyn

    M, N, G = 67, 9, 2  # (s = 8 is N - 1); G guard stages before and after every output
    prob, U = _inputs(name, M, N)
    X = dyn.rollout(name, prob["x0"], U, prob["params"])
    assert np.isfinite(X).all()
    U_tail = _inputs(name, M, N, seed=12)[1][:, :s] if with_tail else None
    x, u = X.shape[-1], U.shape[-1]
    mid = dyn.model_id(name)
    Xd, Ud, P = _dev(X), _dev(U), _dev(prob["params"])
    GUARD = -777.0
    bufX = torch.full((M * N * x + 2 * G * x,), GUARD, dtype=torch.float64, device="cuda")
    bufU = torch.full((M * N * u + 2 * G * u,), GUARD, dtype=torch.float64, device="cuda")
    bufm = torch.full((M * u + 2 * G * u,), GUARD, dtype=torch.float64, device="cuda")
    Xo, Uo, mo = bufX[G * x:-G * x].view(M, N, x), bufU[G * u:-G * u].view(M, N, u), bufm[G * u:-G * u].view(M, u)
    solver.shift_plan(mid, Xd, Ud, P, s=s, U_tail=None if U_tail is None else _dev(U_tail), X_out=Xo, U_out=Uo, um1_out=mo)
    solver.sync()
    for buf, d in ((bufX, x), (bufU, u), (bufm, u)):
        assert bool((buf[:G * d] == GUARD).all()) and bool((buf[-G * d:] == GUARD).all())
    assert torch.equal(Xd, _dev(X)) and torch.equal(Ud, _dev(U))  # the source pair is read only
    assert torch.equal(Xo[:, :N - s], Xd[:, s:]) and torch.equal(Uo[:, :N - s], Ud[:, s:]) and torch.equal(mo, Ud[:, s - 1])
    tail = U_tail if with_tail else np.repeat(U[:, -1:], s, 1)
    assert torch.equal(Uo[:, N - s:], _dev(tail))
    Xt = Xo[:, N - s:].cpu().numpy()
    assert np.isfinite(Xt).all()
    X_lin = np.concatenate([X[:, N - 1:], Xt[:, :-1]], 1)
    pp = prob["params"][:, None, :]
    want = {"unicycle": dyn.unicycle, "quadrotor": dyn.quadrotor, "bicycle": dyn.bicycle}[name](X_lin, tail, pp)[0]
    print(f"{name} s = {s} tail = {with_tail}: one-step max abs difference on the tail {np.abs(Xt - want).max():.3e}")
    np.testing.assert_allclose(Xt, want, **TOL)
    # um1_out is optional: without it the same plan
    X2, U2 = torch.empty_like(Xd), torch.empty_like(Ud)
    st = solver.lib.pmpc_shift_plan_device(solver.h, mid, N, M, s, ctypes.c_void_p(Xd.data_ptr()), ctypes.c_void_p(Ud.data_ptr()), ctypes.c_void_p(P.data_ptr()),
                                           None if U_tail is None else ctypes.c_void_p(_dev(U_tail).data_ptr()), ctypes.c_void_p(X2.data_ptr()),
                                           ctypes.c_void_p(U2.data_ptr()), None)
    solver.sync()
    assert st == 0 and torch.equal(X2, Xo) and torch.equal(U2, Uo)


def test_refused_calls_return_2_and_write_nothing(solver):
    import torch

    from pmpc_amd import dynamics as dyn

    M, N = 5, 4
    prob, U = _inputs("bicycle", M, N)
    X = dyn.rollout("bicycle", prob["x0"], U, prob["params"])
    Xd, Ud, P, x0 = _dev(X), _dev(U), _dev(prob["params"]), _dev(prob["x0"])
    Xo, Uo, mo = torch.full_like(Xd, 7.0), torch.full_like(Ud, 7.0), torch.full((M, 2), 7.0, dtype=torch.float64, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    lib, h = solver.lib, solver.h
    shift = lambda model, s, Xn, Un: lib.pmpc_shift_plan_device(h, model, N, M, s, vp(Xd), vp(Ud), vp(P), None, vp(Xn), vp(Un), vp(mo))
    assert shift(7, 1, Xo, Uo) == 2
    assert shift(2, 0, Xo, Uo) == 2
    assert shift(2, N, Xo, Uo) == 2
    assert shift(2, 1, Xd, Uo) == 2  # X_new is X
    assert shift(2, 1, Xo, Ud) == 2  # U_new is U
    assert lib.pmpc_rollout_device(h, 7, N, M, vp(x0), vp(Ud), vp(P), vp(Xo)) == 2
    assert lib.pmpc_rollout_device(h, 2, 0, M, vp(x0), vp(Ud), vp(P), vp(Xo)) == 2
    solver.sync()
    assert bool((Xo == 7.0).all()) and bool((Uo == 7.0).all()) and bool((mo == 7.0).all())
    assert torch.equal(Xd, _dev(X)) and torch.equal(Ud, _dev(U))
    # ... and the Python layer says why
    with pytest.raises(RuntimeError):
        solver.rollout(7, x0, Ud, P, out=Xo)
    for kw in (dict(s=0), dict(s=N), dict(X_out=Xd)):
        with pytest.raises(ValueError):
            solver.shift_plan(2, Xd, Ud, P, **dict(dict(s=1, X_out=Xo, U_out=Uo), **kw))
    solver.sync()
    assert bool((Xo == 7.0).all()) and bool((Uo == 7.0).all())
