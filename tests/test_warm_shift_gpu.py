"""The active set moved along with the plan on the GPU: k_shift_active_set (pmpc_amd/csrc/dynamics.hip) bitwise against its numpy
specification `pmpc_amd.dynamics.shift_active_set`, the same launch on the context's stored set (`DeviceSolver.warm_shift`), and
`MPCController(warm_shift=True)` — the same answers as the same sub-problems solved cold, and the warm path actually taken."""
import numpy as np
import pytest

from tests.test_warm_shift import BOXES, case, grid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from pmpc_amd.device import DeviceSolver

    s = DeviceSolver(0)
    yield s
    s.close()


def _dev(a, dtype=None):
    import torch

    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def _wide():
    """M = 65: more than one wave of entries per stage row, not a multiple of 64; N = 9, every box kind, tail held and given."""
    for u in (2, 4):
        for Nc in (0, 1, 2, -1):
            for s in (1, 2, 8):
                for with_tail in (False, True):
                    for kind in BOXES:
                        yield 65, 9, u, Nc, s, with_tail, kind


@pytest.mark.parametrize("kind", BOXES)
def test_kernel_equals_the_specification_bitwise(solver, kind):
    import ctypes

    import torch

    from pmpc_amd import dynamics as dyn

    n = 0
    for g in list(grid()) + list(_wide()):
        if g[-1] != kind:
            continue
        c = case(*g)
        act_e, U_e = dyn.shift_active_set(**c)
        M, N, u = c["U"].shape
        guard = 16  # (the outputs sit inside larger buffers: nothing is written outside them)
        Ub, ab = torch.full((M * N * u + 2 * guard,), -7.0, dtype=torch.float64, device="cuda"), torch.full((M * N * u + 2 * guard,), -7, dtype=torch.int32, device="cuda")
        U_o, a_o = Ub[guard:-guard].view(M, N, u), ab[guard:-guard].view(M, N, u)
        vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        Ud, Ut, ad, lo, hi = _dev(c["U"]), _dev(c["U_tail"]), _dev(c["act"], torch.int32), _dev(c["lo"]), _dev(c["hi"])
        torch.cuda.synchronize()
        st = solver.lib.pmpc_shift_active_set_device(solver.h, N, M, u, c["Nc"], c["s"], vp(Ud), vp(Ut), vp(ad), vp(lo), vp(hi), vp(U_o), vp(a_o))
        solver.sync()
        assert st == 0
        assert U_o.cpu().numpy().tobytes() == U_e.tobytes(), g  # (bitwise: signed zeros, infinities and NaN included)
        np.testing.assert_array_equal(a_o.cpu().numpy(), act_e, err_msg=str(g))
        assert bool((Ub[:guard] == -7.0).all() and (Ub[-guard:] == -7.0).all() and (ab[:guard] == -7).all() and (ab[-guard:] == -7).all()), g
        n += 1
    print(f"{kind}: {n} cases bitwise equal")
    assert n >= 348


def test_method_and_refusals(solver):
    import ctypes

    import torch

    from pmpc_amd import dynamics as dyn

    c = case(3, 9, 2, 1, 2, True, "staged")
    act_e, U_e = dyn.shift_active_set(**c)
    Ud, ad = _dev(c["U"]), _dev(c["act"], torch.int32)
    a_o, U_o = solver.shift_active_set(ad, Ud, _dev(c["lo"]), _dev(c["hi"]), c["Nc"], s=c["s"], U_tail=_dev(c["U_tail"]))
    np.testing.assert_array_equal(a_o.cpu().numpy(), act_e)
    assert U_o.cpu().numpy().tobytes() == U_e.tobytes()
    for kw in (dict(s=0), dict(s=9), dict(U_out=Ud), dict(act_out=ad)):
        with pytest.raises(ValueError):
            solver.shift_active_set(ad, Ud, None, None, 1, **dict(dict(s=1), **kw))
    # the entry points themselves: 2 and nothing launched (the outputs keep their fill)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    Uo, ao = torch.full_like(Ud, -7.0), torch.full_like(ad, -7)
    lib, h, flag = solver.lib, solver.h, ctypes.c_int(5)
    assert lib.pmpc_shift_active_set_device(h, 9, 3, 2, 1, 9, vp(Ud), None, vp(ad), None, None, vp(Uo), vp(ao)) == 2
    assert lib.pmpc_shift_active_set_device(h, 9, 3, 2, 1, 1, vp(Ud), None, vp(ad), None, None, vp(Ud), vp(ao)) == 2
    assert lib.pmpc_shift_active_set_device(h, 9, 3, 2, 1, 1, vp(Ud), None, None, None, None, vp(Uo), vp(ao)) == 2
    assert lib.pmpc_warm_shift_device(h, 9, 3, 2, 1, 0, vp(Ud), None, None, None, vp(Uo), ctypes.byref(flag)) == 2
    assert lib.pmpc_warm_shift_device(h, 9, 3, 2, 1, 1, vp(Ud), None, None, None, vp(Uo), None) == 2
    solver.sync()
    assert bool((Uo == -7.0).all() and (ao == -7).all())


def _controller(name, prob, solver, **kw):
    from tests.test_mpc_gpu import _controller as make

    return make(name, prob, solver, **kw)


def test_stored_set_follows_the_plan():
    """One accepted solve through the controller's first step (bicycle M 16, N 9, Nc 1); `warm_set` -> `warm_shift` -> `warm_set`: the second
    read and the controls written equal the specification applied to the first read and the plan, bitwise.  On a fresh context nothing is
    stored: `warm_shift` says so and leaves its output alone."""
    import torch

    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver

    M, N, u = 16, 9, 2
    prob = dyn.make_bicycle_problem(M=M, N=N, Nc=1)
    s1, s2 = DeviceSolver(0), DeviceSolver(0)
    try:
        ctl = _controller("bicycle", prob, s1)
        ctl.reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
        u0, info = ctl.step(prob["x0"], iterations=1)
        assert info["status"] == 0 and info["warm_shift"] is False
        print("first step (ipm_iters, active_set_rounds):", [(i["ipm_iters"], i["active_set_rounds"]) for i in info["infos"]])
        a0 = s1.warm_set(M, N, u)
        assert a0 is not None and s1.warm_set(M, N + 1, u) is None
        lu, uu = ctl._kw["lu"], ctl._kw["uu"]
        U_new = torch.full_like(ctl.U, -7.0)
        assert s1.warm_shift(ctl.U, lu, uu, 1, s=1, U_out=U_new) is True
        a1 = s1.warm_set(M, N, u)
        act_e, U_e = dyn.shift_active_set(a0.cpu().numpy(), ctl.U.cpu().numpy(), prob["u_l"], prob["u_u"], 1, 1)
        print(f"stored statuses: {int((a0 != 0).sum())} held of {a0.numel()}, {int((a1 != 0).sum())} after the shift")
        np.testing.assert_array_equal(a1.cpu().numpy(), act_e)
        assert U_new.cpu().numpy().tobytes() == U_e.tobytes()
        # a second shift moves what the first left (the buffers were swapped, not copied)
        U_2 = torch.full_like(U_new, -7.0)
        assert s1.warm_shift(U_new, lu, uu, 1, s=2, U_out=U_2) is True
        act_e2, U_e2 = dyn.shift_active_set(act_e, U_e, prob["u_l"], prob["u_u"], 1, 2)
        np.testing.assert_array_equal(s1.warm_set(M, N, u).cpu().numpy(), act_e2)
        assert U_2.cpu().numpy().tobytes() == U_e2.tobytes()
        # fresh context
        assert s2.warm_set(M, N, u) is None
        U_3 = torch.full_like(U_new, -7.0)
        assert s2.warm_shift(U_new, lu, uu, 1, s=1, U_out=U_3) is False
        s2.sync()
        assert bool((U_3 == -7.0).all())
    finally:
        s1.close()
        s2.close()


def _tightening(prob):
    """Stage-dependent control boxes that tighten towards stage 0 (factor 0.55 at stage 0, 1 at the last stage): a control on its bound
    at stage j + 1 is outside stage j's box, so the clamp and the dropped statuses run inside a real step."""
    N = prob["u_l"].shape[1]
    grow = (0.55 + 0.45 * np.arange(N) / (N - 1))[None, :, None]
    prob["u_l"], prob["u_u"] = prob["u_l"] * grow, prob["u_u"] * grow
    return prob


CASES = {"bicycle": ("bicycle", 48, 20, 1, False), "bicycle_tightening": ("bicycle", 48, 20, 1, True), "unicycle": ("unicycle", 16, 5, 2, False)}


@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("case_name", sorted(CASES))
def test_warm_steps_equal_the_same_sub_problems_solved_cold(case_name, iterations):
    """4 MPC steps with the seeded 0.01 disturbance of tests/test_mpc_gpu.py::_plant, controller with warm_shift=True.  Expectation of a
    step, on a second context with fresh buffers: numpy `shift_plan` of the controller's previous plan, numpy `shift_active_set` with the
    statuses `warm_set` read back before the step, then `scp_loop(first_cold=True)` from (X', U_new): the same sequence of sub-problems,
    solved cold.  Plans atol 1e-7, residuals rtol 1e-6 / atol 1e-9 (the tolerances of tests/test_mpc_gpu.py), u0 == U[:, 0] exactly, every
    status 0."""
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver, to_device_problem
    from tests.test_mpc_gpu import _hand_step, _plant

    name, M, N, Nc, tighten = CASES[case_name]
    prob = getattr(dyn, f"make_{name}_problem")(M=M, N=N, Nc=Nc)
    if tighten:
        prob = _tightening(prob)
    assert prob["solver_settings"]["Nc"] == Nc
    mid, u = dyn.model_id(name), prob["u_l"].shape[-1]
    d = to_device_problem(prob)
    rng = np.random.default_rng(5)
    s1, s2 = DeviceSolver(0), DeviceSolver(0)
    try:
        ctl = _controller(name, prob, s1, warm_shift=True)
        ctl.reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
        X_start, U_start, x0 = prob["X_prev"], prob["U_prev"], prob["x0"]
        warm_steps = clamped = dropped = 0
        for k in range(4):
            stored = s1.warm_set(M, N, u) if k > 0 else None
            u0, info = ctl.step(x0, iterations=iterations, shift=1)
            assert info["status"] == 0 and info["iterations_done"] == iterations and all(i["status"] == 0 for i in info["infos"]), info
            assert info["warm_shift"] == (stored is not None)
            if stored is not None:  # the start controls the warm step ran from
                a_prev = stored.cpu().numpy()
                a_new, U_new = dyn.shift_active_set(a_prev, U, prob["u_l"], prob["u_u"], Nc, 1)
                clamped += int((U_new != U_start).sum())
                dropped += int(((np.concatenate([a_prev[:, 1:], a_prev[:, -1:]], 1) != 0) & (a_new == 0)).sum())
                U_start = U_new
                warm_steps += 1
            X, U = ctl.X.cpu().numpy(), ctl.U.cpu().numpy()
            res_h, X_h, U_h = _hand_step(s2, mid, prob, d, X_start, U_start, x0, iterations)
            print(f"{case_name} x{iterations} step {k}: warm {info['warm_shift']}; residuals {info['resid']} cold {res_h}; max |dX| {np.abs(X - X_h).max():.3e} "
                  f"max |dU| {np.abs(U - U_h).max():.3e}; (ipm, rounds) {[(i['ipm_iters'], i['active_set_rounds']) for i in info['infos']]}")
            np.testing.assert_allclose(X, X_h, rtol=0, atol=1e-7)
            np.testing.assert_allclose(U, U_h, rtol=0, atol=1e-7)
            np.testing.assert_allclose(info["resid"], res_h, rtol=1e-6, atol=1e-9)
            np.testing.assert_array_equal(u0, U[:, 0])
            X_start, U_start, _ = dyn.shift_plan(name, X, U, prob["params"], s=1)
            x0 = _plant(name, prob, np.broadcast_to(x0, (M, X.shape[-1]))[0], u0, rng)
        print(f"{case_name} x{iterations}: {warm_steps} of 3 shifted steps started warm; start controls moved by the clamp {clamped}, statuses dropped {dropped}")
        if tighten and warm_steps:
            assert clamped > 0  # (the case is there for the clamp branch: it ran)
    finally:
        s1.close()
        s2.close()


def test_the_warm_path_is_taken():
    """A shifted step of ONE iteration: with warm_shift=True its solve starts with the forward sweep's defect variant (the no-rollout warm
    start: `fwd` launch codes with bit 0 set) and says so in info; with warm_shift=False no such launch happens."""
    from pmpc_amd import _lib
    from pmpc_amd import dynamics as dyn
    from pmpc_amd.device import DeviceSolver
    from tests.test_mpc_gpu import _plant

    prob = dyn.make_bicycle_problem(M=48, N=20, Nc=1)
    for warm in (True, False):
        rng = np.random.default_rng(5)
        s = DeviceSolver(0)
        try:
            ctl = _controller("bicycle", prob, s, warm_shift=warm)
            ctl.reset(X_prev=prob["X_prev"], U_prev=prob["U_prev"])
            x0, firsts, flags, counts = prob["x0"], [], [], []
            for k in range(4):
                _lib.as_sweep_launches("fwd", reset=True)
                u0, info = ctl.step(x0, iterations=1)
                assert info["status"] == 0
                counts.append(sum(_lib.as_sweep_launches("fwd")[1::2]))  # (code = defect + 2 pf2 + 4 cone + 8 f32 + 16 sens)
                firsts.append((info["infos"][0]["ipm_iters"], info["infos"][0]["active_set_rounds"]))
                flags.append(info["warm_shift"])
                x0 = _plant("bicycle", prob, np.broadcast_to(x0, (48, 4))[0], u0, rng)
            print(f"warm_shift={warm}: first iterations (ipm_iters, active_set_rounds) {firsts}; started warm {flags}; defect-variant forward sweeps {counts}")
            if warm:
                assert flags[0] is False and counts[0] == 0  # (the first step after reset has no shift)
                assert flags[1] is True and counts[1] > 0
                assert all(c > 0 for c, f in zip(counts, flags) if f) and all(c == 0 for c, f in zip(counts, flags) if not f)
            else:
                assert not any(flags) and sum(counts) == 0
        finally:
            s.close()
