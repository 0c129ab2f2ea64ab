"""The runtime-compiled kernels (pmpc_amd/csrc/model_kernels.h) over the dimension range, on the GPU: the model family of
tests/support/custom_models.py (FAMILY_SRC: every function of model_dual.h, a constant row) at nine (x, u, p) that reach 64, 32, 16
and 8 units per block, one to eight AD passes and the second trip of the pass loop, against the float64 torch restatement
`cm.family_ref` (pinned on the host by tests/test_custom_model_dims.py).  Outputs are views into sentinel-filled buffers with guard
records on both sides.  Tolerance: rtol = atol = 1e-12, that of tests/test_bicycle_gpu.py.  Rollout and plan shift are compared one
step at a time, for the reason tests/test_rollout_gpu.py gives.  Each model is compiled once for the module.

Measured on an MI355X, the largest absolute differences over all cases and shapes (per row type in CHANGELOG.md): linearise against the
reference f 2.2e-16, fx 2.2e-16, fu 1.9e-16; rollout one step at a time 2.2e-16; the tail of the plan shift 4.4e-16; `f` of `linearize`
at the rolled-out iterate 2.2e-16 off the rollout (bit-equal at (1, 1, 1) and at M = N = 1 only).  The nine runtime compiles take about
3 s of the module's 6 s."""
import ctypes
import functools

import numpy as np
import pytest

from tests.support import custom_models as cm

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-12, atol=1e-12)
SENTINEL = -777.0
G = 2  # guard records before and after every output
ROLL_CASES = ["smallest_half_empty_chunk", "second_trip_of_the_pass_loop", "units_32_even_record", "every_limit"]


@pytest.fixture(scope="module")
def models():
    return {case: cm.make_family(case) for case in cm.FAMILY_CASES}


@pytest.fixture(scope="module")
def solver():
    from pmpc_amd.device import DeviceSolver

    s = DeviceSolver(0)
    yield s
    s.close()


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()  # (a copy: the shared inputs are read-only)


def _guarded(records, *rec_shape):
    """(buffer, view): `records` records of shape rec_shape inside a sentinel-filled buffer, G guard records on either side."""
    import torch

    n = int(np.prod(rec_shape))
    buf = torch.full(((records + 2 * G) * n,), SENTINEL, dtype=torch.float64, device="cuda")
    return buf, buf[G * n:(records + G) * n].view(records, *rec_shape)


def _guards_untouched(buf, view):
    n = (buf.numel() - view.numel()) // 2
    return bool((buf[:n] == SENTINEL).all()) and bool((buf[-n:] == SENTINEL).all())


def _lin_shapes(case):
    U = cm.FAMILY_UNITS[case]
    return [(1, 1), (2, U), (3, U + 3), (67, 3)]  # one unit; two full blocks; full blocks and a partial one; idx / N steps inside a block


@functools.lru_cache(maxsize=None)
def _lin_problem(case, shape):
    """Inputs and the reference of one linearise case, computed once: x0, X_prev, U_prev, P, (f, fx, fu) in the py layout."""
    M, N = shape
    x0, Xp, Up, P = cm.family_inputs(cm.FAMILY_CASES[case], M, N, seed=31)
    X_ = np.concatenate([x0[:, None], Xp[:, :-1]], 1)
    assert cm.family_kink_margin(X_, Up) >= cm.KINK_MARGIN  # (a condition on the inputs, not on the kernel)
    ref = cm.family_ref(X_, Up, P)
    for a in (x0, Xp, Up, P, *ref):
        a.setflags(write=False)
    return x0, Xp, Up, P, ref


def _by_row_type(diff, axis):
    """max |diff| per row type k % 8, `axis` the axis of the output row."""
    d = np.moveaxis(np.abs(diff), axis, -1)
    return " ".join(f"{t}:{d[..., t::8].max():.1e}" for t in range(min(8, d.shape[-1])))


LIN_PARAMS = [(case, i) for case in cm.FAMILY_CASES for i in range(4)]


@pytest.mark.parametrize("case,shape_no", LIN_PARAMS, ids=[f"{c}-{('one_unit', 'two_full_blocks', 'partial_block', 'short_horizon')[i]}" for c, i in LIN_PARAMS])
def test_linearize_against_the_torch_reference_inside_guarded_buffers(models, solver, case, shape_no):
    import torch

    x, u, p = cm.FAMILY_CASES[case]
    M, N = _lin_shapes(case)[shape_no]
    assert cm.lin_units(x, u) == cm.FAMILY_UNITS[case]
    x0, Xp, Up, P, (fo, fxo, fuo) = _lin_problem(case, (M, N))
    if N == 1:  # the kernel must not read X_prev: stage 0 is linearised at x0 and there is no other stage
        Xp = np.full_like(Xp, np.nan)
    else:  # (the inputs tell x0 from X_prev[:, 0], so agreement with the reference shows stage 0 was linearised at x0)
        assert np.abs(fo[:, 0] - cm.family_f(Xp[:, :1], Up[:, :1], P)[:, 0]).max() > 1e-3
    ins = [_dev(a) for a in (x0, Xp, Up, P)]
    before = [t.clone() for t in ins]
    (bf, f), (bfx, fx), (bfu, fu) = _guarded(M * N, x), _guarded(M * N, x, x), _guarded(M * N, u, x)
    mid = solver.load_model(models[case])
    solver.linearize(mid, *ins, f=f.view(M, N, x), fx=fx.view(M, N, x, x), fu=fu.view(M, N, u, x))
    solver.sync()
    for buf, view, what in ((bf, f, "f"), (bfx, fx, "fx"), (bfu, fu, "fu")):
        assert _guards_untouched(buf, view), f"{what}: a guard record was written"
        assert not bool((view == SENTINEL).any()), f"{what}: an entry of the record was not written"
        assert bool(torch.isfinite(view).all()), what
    for t, b in zip(ins, before):
        assert torch.equal(t.view(torch.int64), b.view(torch.int64))  # the inputs are read only (bit patterns: X_prev may hold NaN)
    f, fx, fu = f.view(M, N, x).cpu().numpy(), fx.view(M, N, x, x).cpu().numpy(), fu.view(M, N, u, x).cpu().numpy()
    fx, fu = np.swapaxes(fx, -1, -2), np.swapaxes(fu, -1, -2)  # ABI blocks are [column][row]
    print(f"{case} ({x}, {u}, {p}) M {M} N {N}: max |df| {np.abs(f - fo).max():.2e} |dfx| {np.abs(fx - fxo).max():.2e} |dfu| {np.abs(fu - fuo).max():.2e}; "
          f"by row type: f {_by_row_type(f - fo, -1)}; fx {_by_row_type(fx - fxo, -2)}; fu {_by_row_type(fu - fuo, -2)}")
    np.testing.assert_allclose(f, fo, **TOL)
    np.testing.assert_allclose(fx, fxo, **TOL)
    np.testing.assert_allclose(fu, fuo, **TOL)
    for k in range(7, x, 8):  # the constant row: zeros were written, not left
        assert not fx[..., k, :].any() and not fu[..., k, :].any() and np.array_equal(f[..., k], np.broadcast_to(P[:, None, -1], (M, N)))


def _one_step(x_first, X, U, P):
    """F([x_first, X[:-1]][j], U[j]) of the reference for every stage j at once."""
    return cm.family_f(np.concatenate([x_first[:, None, :], X[:, :-1]], 1), U, P)


@functools.lru_cache(maxsize=None)
def _roll_problem(case, shape):
    M, N = shape
    x0, _, U, P = cm.family_inputs(cm.FAMILY_CASES[case], M, N, seed=41)
    X = cm.family_rollout(x0, U, P)
    assert np.isfinite(X).all()  # (a condition on the inputs, not on the kernel)
    for a in (x0, U, P, X):
        a.setflags(write=False)
    return x0, U, P, X


@pytest.mark.parametrize("case", ROLL_CASES)
@pytest.mark.parametrize("M,N", [(1, 1), (64, 5), (67, 5)])  # one lane; exactly one wave; a second block with three lanes
def test_rollout_step_by_step_inside_a_guarded_buffer_and_feasible_for_linearize(models, solver, case, M, N):
    import torch

    x, u, p = cm.FAMILY_CASES[case]
    x0, U, P, X_ref = _roll_problem(case, (M, N))
    x0d, Ud, Pd = _dev(x0), _dev(U), _dev(P)
    buf, Xv = _guarded(M * N, x)
    mid = solver.load_model(models[case])
    X_dev = solver.rollout(mid, x0d, Ud, Pd, out=Xv.view(M, N, x))
    solver.sync()
    assert _guards_untouched(buf, Xv) and not bool((Xv == SENTINEL).any())
    assert torch.equal(x0d, _dev(x0)) and torch.equal(Ud, _dev(U)) and torch.equal(Pd, _dev(P))
    X = X_dev.cpu().numpy()
    assert np.isfinite(X).all()
    want = _one_step(x0, X, U, P)
    print(f"{case} ({M}, {N}): one-step max abs difference {np.abs(X - want).max():.3e} (by row type {_by_row_type(X - want, -1)}); "
          f"against the reference rollout {np.abs(X - X_ref).max():.3e}")
    np.testing.assert_allclose(X, want, **TOL)
    # f of linearize at the rolled-out iterate is the rollout, within the tolerance: step<double> and step<Dual> may contract differently
    f, _, _ = solver.linearize(mid, x0d, X_dev, Ud, Pd)
    solver.sync()
    print(f"{case} ({M}, {N}): f of linearize bit-equal to the rollout: {bool(torch.equal(f, X_dev))}; max abs defect {float((f - X_dev).abs().max()):.3e}")
    np.testing.assert_allclose(f.cpu().numpy(), X, **TOL)


@pytest.mark.parametrize("case", ROLL_CASES)
@pytest.mark.parametrize("s", [1, 4])
@pytest.mark.parametrize("with_tail", [False, True])
def test_shift_plan_copies_exactly_rolls_out_the_tail_and_stays_inside_its_buffers(models, solver, case, s, with_tail):
    import torch

    M, N = 67, 5  # (s = 4 is N - 1)
    x, u, p = cm.FAMILY_CASES[case]
    _, U, P, X = _roll_problem(case, (M, N))
    U_tail = cm.family_inputs((x, u, p), M, s, seed=43)[2] if with_tail else None
    Xd, Ud, Pd = _dev(X), _dev(U), _dev(P)
    Td = None if U_tail is None else _dev(U_tail)
    (bX, Xo), (bU, Uo), (bm, mo) = _guarded(M * N, x), _guarded(M * N, u), _guarded(M, u)
    Xo, Uo = Xo.view(M, N, x), Uo.view(M, N, u)
    mid = solver.load_model(models[case])
    solver.shift_plan(mid, Xd, Ud, Pd, s=s, U_tail=Td, X_out=Xo, U_out=Uo, um1_out=mo)
    solver.sync()
    for buf, view, what in ((bX, Xo, "X_out"), (bU, Uo, "U_out"), (bm, mo, "um1_out")):
        assert _guards_untouched(buf, view), f"{what}: a guard record was written"
        assert not bool((view == SENTINEL).any()), f"{what}: an entry was not written"
    assert torch.equal(Xd, _dev(X)) and torch.equal(Ud, _dev(U)) and torch.equal(Pd, _dev(P))  # the source pair is read only
    assert Td is None or torch.equal(Td, _dev(U_tail))
    assert torch.equal(Xo[:, :N - s], Xd[:, s:]) and torch.equal(Uo[:, :N - s], Ud[:, s:]) and torch.equal(mo, Ud[:, s - 1])
    tail = U_tail if with_tail else np.repeat(U[:, -1:], s, 1)
    assert torch.equal(Uo[:, N - s:], _dev(tail))
    Xt = Xo[:, N - s:].cpu().numpy()
    assert np.isfinite(Xt).all()
    want = _one_step(X[:, N - 1], Xt, tail, P)
    assert np.isfinite(want).all()
    print(f"{case} s = {s} tail = {with_tail}: one-step max abs difference on the tail {np.abs(Xt - want).max():.3e}")
    np.testing.assert_allclose(Xt, want, **TOL)
    # um1_out is optional: without it the same plan
    X2, U2 = torch.full_like(Xd, SENTINEL), torch.full_like(Ud, SENTINEL)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = solver.lib.pmpc_shift_plan_device(solver.h, mid, N, M, s, vp(Xd), vp(Ud), vp(Pd), vp(Td), vp(X2), vp(U2), None)
    solver.sync()
    assert st == 0 and torch.equal(X2, Xo) and torch.equal(U2, Uo)
