"""The active set moved along with the plan (pmpc_amd.dynamics.shift_active_set, the specification of csrc/dynamics.hip
k_shift_active_set): its postcondition — the outputs are a base point the solver's no-rollout warm start accepts —, the three entry points
in the library's symbol list, and what `MPCController(warm_shift=True)` refuses before it needs a device.  No GPU."""
import itertools

import numpy as np
import pytest

from pmpc_amd import dynamics as dyn

BOXES = ("constant", "staged", "one_sided", "pinned", "none", "empty")


def boxes(kind, M, N, u, rng):
    """(lo, hi) (M, N, u) or None.  constant: one box per (particle, control) along the horizon; staged: boxes that tighten towards stage 0
    (a control on its bound at stage j + s is outside stage j's box: the clamp and the dropped statuses); one_sided: +-inf on one side
    per entry; pinned: lo == hi on a third of the entries; empty: the staged boxes with one entry lo > hi."""
    if kind == "none":
        return None, None
    lo, hi = -rng.uniform(0.5, 1.5, (M, 1, u)) * np.ones((1, N, 1)), rng.uniform(0.5, 1.5, (M, 1, u)) * np.ones((1, N, 1))
    if kind == "constant":
        return lo, hi
    grow = (0.4 + 0.6 * (np.arange(N) + 1.0) / N)[None, :, None]
    lo, hi = lo * grow, hi * grow
    if kind == "one_sided":
        side = rng.integers(0, 3, (M, N, u))
        lo, hi = np.where(side == 0, -np.inf, lo), np.where(side == 1, np.inf, hi)
    elif kind == "pinned":
        pin = rng.integers(0, 3, (M, N, u)) == 0
        hi = np.where(pin, lo, hi)
    elif kind == "empty":
        lo[M - 1, N // 2, u - 1] = hi[M - 1, N // 2, u - 1] + 0.25
    return lo, hi


def plan(lo, hi, M, N, u, Nc, rng):
    """(act, U) as an accepted solve leaves them: statuses 0 / 1 / 2 by a seeded draw (a side without a bound is never held), held controls
    exactly on their bound, free ones inside the box (a few zeros of either sign among them), the consensus stages uniform over the
    particles with particle 0's box."""
    l = np.full((M, N, u), -np.inf) if lo is None else lo.copy()
    h = np.full((M, N, u), np.inf) if hi is None else hi.copy()
    nc = N if Nc < 0 else min(Nc, N)
    l[:, :nc], h[:, :nc] = l[:1, :nc], h[:1, :nc]
    act = rng.integers(0, 3, (M, N, u)).astype(np.int32)
    act[(act == 1) & ~np.isfinite(l)] = 0
    act[(act == 2) & ~np.isfinite(h)] = 0
    with np.errstate(invalid="ignore"):
        a, b = np.where(np.isfinite(l), l, -2.0), np.where(np.isfinite(h), h, 2.0)
        U = a + rng.uniform(0.0, 1.0, (M, N, u)) * (b - a)
    zero = rng.integers(0, 8, (M, N, u)) == 0
    U = np.where(zero & (l <= 0.0) & (h >= 0.0), np.where(rng.integers(0, 2, (M, N, u)) == 0, 0.0, -0.0), U)
    U = np.where(act == 1, l, np.where(act == 2, h, U))
    act[:, :nc], U[:, :nc] = act[:1, :nc], U[:1, :nc]
    return act, U


def grid():
    """(M, N, u, Nc, s, with_tail, box kind): M in {1, 3}, N in {2, 3, 9}, u in {1, 2, 4}, Nc in {0, 1, 2, N, -1}, s in {1, 2, N - 1}."""
    for M, N, u in itertools.product((1, 3), (2, 3, 9), (1, 2, 4)):
        for Nc in sorted({0, 1, 2, N, -1}):
            for s in sorted({1, 2, N - 1} & set(range(1, N))):
                for with_tail in (False, True):
                    for kind in BOXES:
                        yield M, N, u, Nc, s, with_tail, kind


def case(M, N, u, Nc, s, with_tail, kind):
    """The seeded inputs of one grid point: dict(act, U, lo, hi, Nc, s, U_tail).  The tail reaches 1.3 times the widest box."""
    rng = np.random.default_rng([M, N, u, Nc + 1, s, int(with_tail), BOXES.index(kind)])
    lo, hi = boxes(kind, M, N, u, rng)
    act, U = plan(lo, hi, M, N, u, Nc, rng)
    U_tail = rng.uniform(-2.0, 2.0, (M, s, u)) if with_tail else None
    return dict(act=act, U=U, lo=lo, hi=hi, Nc=Nc, s=s, U_tail=U_tail)


def check_postcondition(c, act_n, U_n):
    """What the first round of the warm start verifies (kernels_as.hip, the DEFECT branch of the forward sweep): the rule `snapped = lo
    where 1, hi where 2, clamp(U) otherwise` gives U itself, against particle 0's box on the consensus stages, which are uniform."""
    M, N, u = U_n.shape
    nc = N if c["Nc"] < 0 else min(c["Nc"], N)
    l = np.full((M, N, u), -np.inf) if c["lo"] is None else c["lo"].copy()
    h = np.full((M, N, u), np.inf) if c["hi"] is None else c["hi"].copy()
    l[:, :nc], h[:, :nc] = l[:1, :nc], h[:1, :nc]
    assert act_n.dtype == np.int32 and act_n.shape == U_n.shape and set(np.unique(act_n)) <= {0, 1, 2}
    snapped = np.where(act_n == 1, l, np.where(act_n == 2, h, np.minimum(np.maximum(U_n, l), h)))
    ok = ~(l > h)  # (an empty box passes through with status 0: the solve's own check refuses the problem)
    np.testing.assert_array_equal(snapped[ok], U_n[ok])
    assert np.all(act_n[~ok] == 0)
    np.testing.assert_array_equal(U_n[:, :nc], np.broadcast_to(U_n[:1, :nc], U_n[:, :nc].shape))
    np.testing.assert_array_equal(act_n[:, :nc], np.broadcast_to(act_n[:1, :nc], act_n[:, :nc].shape))


def test_the_shifted_set_is_a_base_point_the_warm_start_accepts():
    seen = {k: 0 for k in ("clamped", "dropped", "kept", "set_by_clamp", "empty")}
    n = 0
    for g in grid():
        c = case(*g)
        act_n, U_n = dyn.shift_active_set(**c)
        check_postcondition(c, act_n, U_n)
        # the sources, restated entry by entry for the particle-own stages
        M, N, u, Nc, s, with_tail, kind = g
        nc = N if Nc < 0 else min(Nc, N)
        for j in range(N):
            src_U = c["U"][:, j + s] if j < N - s else (c["U_tail"][:, j - (N - s)] if with_tail else c["U"][:, N - 1])
            src_a = c["act"][:, j + s] if j < N - s else (np.zeros((M, u), np.int32) if with_tail else c["act"][:, N - 1])
            if j < nc:
                src_U, src_a = np.broadcast_to(src_U[:1], (M, u)), np.broadcast_to(src_a[:1], (M, u))
            moved = U_n[:, j] != src_U
            seen["clamped"] += int(moved.sum())
            seen["dropped"] += int(((src_a != 0) & (act_n[:, j] == 0)).sum())
            seen["kept"] += int(((src_a != 0) & (act_n[:, j] == src_a)).sum())
            seen["set_by_clamp"] += int(((src_a == 0) & (act_n[:, j] != 0)).sum())
            assert np.all(act_n[:, j][moved] != 0) or kind == "empty"  # a clamped control is held on the bound it was moved to
        seen["empty"] += kind == "empty"
        n += 1
    print(f"{n} cases; entries {seen}")
    assert all(v > 0 for v in seen.values()), seen  # every branch of the rule ran


def test_constant_boxes_with_a_held_tail_change_no_value():
    """Boxes that do not depend on the stage, tail held, no consensus stage: the shifted controls are already the base point of the
    shifted statuses — no control moves, no status changes.  (On consensus stages particle 0's control is written to every particle.)"""
    for M, N, u in itertools.product((1, 3), (2, 3, 9), (1, 2, 4)):
        for s in sorted({1, 2, N - 1} & set(range(1, N))):
            c = case(M, N, u, 0, s, False, "constant")
            act_n, U_n = dyn.shift_active_set(**c)
            idx = np.minimum(np.arange(N) + s, N - 1)
            assert U_n.tobytes() == np.ascontiguousarray(c["U"][:, idx]).tobytes()  # (bitwise: signed zeros included)
            np.testing.assert_array_equal(act_n, c["act"][:, idx])
            for Nc in (1, 2, N, -1):  # with consensus stages: the same statement about particle 0's plan on those stages
                c = case(M, N, u, Nc, s, False, "constant")
                act_n, U_n = dyn.shift_active_set(**c)
                nc = N if Nc < 0 else min(Nc, N)
                exp_U, exp_a = c["U"][:, idx].copy(), c["act"][:, idx].copy()
                lo0, hi0 = c["lo"][0, :nc], c["hi"][0, :nc]
                exp_U[:, :nc], exp_a[:, :nc] = exp_U[:1, :nc], exp_a[:1, :nc]
                # (stages nc - s .. nc - 1 come from per-particle stages of particle 0: inside ITS box, which is the consensus box)
                np.testing.assert_array_equal(U_n, exp_U)
                np.testing.assert_array_equal(act_n, exp_a)
                assert np.all(U_n[:, :nc] >= lo0) and np.all(U_n[:, :nc] <= hi0)


def test_a_nan_control_passes_through_with_status_zero():
    c = case(3, 9, 2, 1, 1, False, "staged")
    c["U"][1, 5, 0] = np.nan
    act_n, U_n = dyn.shift_active_set(**c)
    assert np.isnan(U_n[1, 4, 0]) and act_n[1, 4, 0] == 0 and np.isnan(U_n).sum() == 1


def test_shift_outside_the_horizon_is_refused():
    c = case(3, 3, 2, 1, 1, False, "constant")
    for s in (0, 3, -1, 4):
        with pytest.raises(ValueError):
            dyn.shift_active_set(**dict(c, s=s))


def test_entry_points_are_declared_and_exported():
    from pmpc_amd import _lib

    lib = _lib.load()  # must load without a GPU
    for sym in ("pmpc_shift_active_set_device", "pmpc_warm_shift_device", "pmpc_warm_set_read_device"):
        assert sym in _lib.ABI_SYMBOLS
        assert hasattr(lib, sym), sym
    assert len(lib.pmpc_shift_active_set_device.argtypes) == 13 and len(lib.pmpc_warm_shift_device.argtypes) == 12
    assert len(lib.pmpc_warm_set_read_device.argtypes) == 3


class _NoDevice:
    """Stands where a DeviceSolver would: any use of it is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came after the solver was touched ({name})")


@pytest.mark.parametrize("kw,word", [
    (dict(solver_settings=dict(solver="ecos", Nc=1)), "cone objective"),
    (dict(solver_settings=dict(Nc=1)), "cone objective"),  # (the default solver is the reference's: the cone path)
    (dict(solver_settings=dict(solver="osqp", Nc=1, smooth_alpha=1e2)), "cone objective"),
    (dict(soc=dict(W=np.eye(2), w0=np.zeros(2), v=np.zeros(2), v0=1.0, u_interior=np.zeros(2))), "stage cone"),
    (dict(solver_settings=dict(solver="osqp", Nc=1, extra_cstrs=[("l", "A", "b")], soc_u_interior=np.zeros(2))), "stage cone"),
    (dict(x_l=-np.ones((4, 6, 4)), x_u=np.ones((4, 6, 4))), "state boxes"),
    (dict(slew_rate=0.5), "slew"),
    (dict(solver_settings=dict(solver="osqp", Nc=1, slew_reg=0.1)), "slew"),
    (dict(keepout=dict(pos_idx=(0, 1), centres=np.array([[5.0, 5.0]]), radius=np.array([0.5]))), "keepout"),
])
def test_warm_shift_is_refused_before_a_device_is_needed(kw, word):
    import pmpc_amd

    prob = dyn.make_bicycle_problem(M=4, N=6, Nc=1)
    args = dict(builtin_model="bicycle", params=prob["params"], Q=prob["Q"], R=prob["R"], X_ref=prob["X_ref"], U_ref=prob["U_ref"], u_l=prob["u_l"],
                u_u=prob["u_u"], reg_x=prob["reg_x"], reg_u=prob["reg_u"], solver_settings=dict(solver="osqp", Nc=1), solver=_NoDevice(),
                device="cpu", warm_shift=True)
    args.update(kw)
    with pytest.raises(ValueError, match="warm_shift=True is not supported next to.*" + word):
        pmpc_amd.MPCController(**args)
