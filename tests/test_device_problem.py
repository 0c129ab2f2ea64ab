"""`pmpc_amd.device_problem`: the resident problem that `solve(..., device=...)` and `MPCController` share, built on the CPU — it is plain
tensor work, so everything about it is checked without a GPU."""
import math

import numpy as np
import pytest
import torch

from pmpc_amd import extra_cstrs as ec
from pmpc_amd.device_problem import build_problem, keepout_static

SHAPES = [(2, 3, 4, 2), (2, 3, 12, 4)]


def _args(M, N, x, u, seed=0):
    rng = np.random.default_rng(seed)
    A, B = rng.standard_normal((M, N, x, x)), rng.standard_normal((M, N, u, u))
    Q = A @ A.transpose(0, 1, 3, 2) + np.eye(x)  # symmetric blocks
    R = B @ B.transpose(0, 1, 3, 2) + np.eye(u)
    return dict(Q=Q, R=R, x0=rng.standard_normal((M, x)), X_ref=rng.standard_normal((M, N, x)), U_ref=rng.standard_normal((M, N, u)))


def _build(a, **kw):
    return build_problem(**dict(a, device="cpu", **kw))


@pytest.mark.parametrize("shape", SHAPES)
def test_layout_shapes_and_symmetry(shape):
    M, N, x, u = shape
    a = _args(*shape)
    p = _build(a)
    assert (p.M, p.N, p.xdim, p.udim, p.single) == (M, N, x, u, False)
    assert torch.equal(p.Q, torch.as_tensor(a["Q"])) and torch.equal(p.R, torch.as_tensor(a["R"]))
    assert torch.equal(p.Qa, p.Q.transpose(-1, -2)) and torch.equal(p.Ra, p.R.transpose(-1, -2))
    assert p.Qa.is_contiguous() and p.Ra.is_contiguous() and p.x0.is_contiguous()
    assert p.sym is True
    assert torch.equal(p.X_prev, p.X_ref) and torch.equal(p.U_prev, p.U_ref)  # the default start iterate
    assert p.X_prev.data_ptr() != p.X_ref.data_ptr() and p.U_prev.data_ptr() != p.U_ref.data_ptr()
    a["Q"] = a["Q"].copy()
    a["Q"][1, 2, 0, 1] += 0.5  # one asymmetric block
    q = _build(a)
    assert q.sym is False and torch.equal(q.Qa, q.Q.transpose(-1, -2))
    with pytest.raises(ValueError, match="builtin_cost needs symmetric Q and R blocks"):
        _build(a, need_sym="builtin_cost needs")
    kw = p.solve_kw()
    assert kw["Q"] is p.Qa and kw["R"] is p.Ra and kw["x0"] is p.x0 and kw["symmetric_cost"] is True
    assert (kw["reg_x"], kw["reg_u"], kw["Nc"]) == (1.0, 1e-2, -1) and kw["slew_reg"] is None and kw["lu"] is None
    assert not {"f", "fx", "fu", "X_prev", "U_prev", "X_ref", "U_ref", "X_out", "U_out"} & set(kw)  # what an iteration sets


@pytest.mark.parametrize("shape", SHAPES)
def test_boxes(shape):
    M, N, x, u = shape
    a = _args(*shape)
    lo, hi = -np.ones((M, N, u)), np.ones((M, N, u))
    for kw in (dict(), dict(u_l=lo), dict(u_u=hi), dict(u_l=lo, u_u=np.zeros(0)), dict(u_l=[], u_u=hi), dict(u_l=torch.zeros(0), u_u=torch.as_tensor(hi))):
        p = _build(a, **kw)
        assert p.lu is None and p.uu is None and p.lx is None and p.ux is None, kw
    xl, xu = -2 * np.ones((M, N, x)), 3 * np.ones((M, N, x))
    pn = _build(a, u_l=lo, u_u=hi, x_l=xl, x_u=xu)
    pt = _build(a, u_l=torch.as_tensor(lo), u_u=torch.as_tensor(hi), x_l=torch.as_tensor(xl), x_u=torch.as_tensor(xu))
    for k in ("lu", "uu", "lx", "ux"):
        assert torch.equal(getattr(pn, k), getattr(pt, k)) and getattr(pn, k).dtype == torch.float64
    assert torch.equal(pn.lu, torch.as_tensor(lo)) and torch.equal(pn.ux, torch.as_tensor(xu))
    assert pn.solve_kw()["lx"] is pn.lx and pn.solve_kw()["uu"] is pn.uu


def test_settings():
    a = _args(*SHAPES[0])
    p = _build(a)
    assert p.cone and p.Nc == -1 and math.isnan(p.smooth_alpha) and p.solver_verbose is False
    for name in ("ecos", "gurobi", "mosek", "cosmo", "ECOS"):
        assert _build(a, solver_settings=dict(solver=name)).cone, name
    assert not _build(a, solver_settings=dict(solver="osqp")).cone
    assert _build(a, solver_settings=dict(solver="osqp", smooth_cstr="logbarrier")).cone
    q = _build(a, solver_settings=dict(solver="osqp", smooth_alpha=8.0, Nc=2, verbose=True), reg_x=3, reg_u=0.5)
    assert q.cone and q.smooth_alpha == 8.0 and q.Nc == 2 and q.solver_verbose is True
    assert (q.reg_x, q.reg_u) == (3.0, 0.5) and isinstance(q.reg_x, float)


@pytest.mark.parametrize("shape", SHAPES)
def test_slew(shape):
    M, N, x, u = shape
    a = _args(*shape)
    assert _build(a).slew is None and _build(a, slew_rate=0).slew is None and _build(a, slew_rate=0.0).slew is None
    assert torch.equal(_build(a, slew_rate=0.25).slew, torch.full((M,), 0.25, dtype=torch.float64))
    p = _build(a, solver_settings=dict(slew_reg=2.0))  # no u0_slew: the first control has nothing to be compared with
    assert p.slew0 is None and p.um1 is None
    assert torch.equal(p.slew_reg0, torch.full((M,), 2.0, dtype=torch.float64))
    p = _build(a, u0_slew=np.arange(u, dtype=float))  # no slew_reg
    assert p.slew0 is None and p.um1 is None and p.slew_reg0 is None
    p = _build(a, solver_settings=dict(slew_reg=2.0), u0_slew=np.arange(u, dtype=float))
    assert torch.equal(p.slew0, torch.full((M,), 2.0, dtype=torch.float64))
    assert p.um1.shape == (M, u) and p.um1.is_contiguous() and torch.equal(p.um1, torch.arange(u, dtype=torch.float64).expand(M, u))


@pytest.mark.parametrize("shape", SHAPES)
def test_stage_cones(shape):
    M, N, x, u = shape
    a = _args(*shape)
    rng = np.random.default_rng(1)
    soc = dict(W=rng.standard_normal((3, u)), w0=rng.standard_normal(3), v=rng.standard_normal(u), v0=1.5, u_interior=np.zeros(u))
    assert _build(a).soc_kw == {}
    want = _build(a, soc=soc).soc_kw
    assert want["soc_W"].shape == (3, u) and want["soc_w0"].shape == (3,) and want["soc_v"].shape == (u,) and want["soc_v0"] == 1.5
    for Nc in (-1, 1):
        tup = ec.stage_soc_to_extra_cstrs(soc["W"], soc["w0"], soc["v"], soc["v0"], M, N, x, u, Nc)
        got = _build(a, solver_settings=dict(Nc=Nc, extra_cstrs=[tup], soc_u_interior=soc["u_interior"])).soc_kw
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]) if torch.is_tensor(want[k]) else got[k] == want[k], k
    with pytest.raises(ValueError, match="one extra_cstrs tuple"):
        _build(a, solver_settings=dict(extra_cstrs=[tup, tup], soc_u_interior=soc["u_interior"]))
    with pytest.raises(ValueError, match="soc_u_interior.*is required"):
        _build(a, solver_settings=dict(Nc=1, extra_cstrs=[tup]))


@pytest.mark.parametrize("shape", SHAPES)
def test_a_single_problem_is_promoted(shape):
    M, N, x, u = shape
    a = _args(*shape)
    one = {k: v[0] for k, v in a.items()}
    p = _build(one, u_l=-np.ones((N, u)), u_u=np.ones((N, u)), X_prev=np.zeros((N, x)), builtin_model="unicycle", params=np.ones(3))
    assert p.single and (p.M, p.N, p.xdim, p.udim) == (1, N, x, u)
    for k, s in dict(Q=(1, N, x, x), Ra=(1, N, u, u), x0=(1, x), X_ref=(1, N, x), U_ref=(1, N, u), X_prev=(1, N, x), U_prev=(1, N, u),
                     lu=(1, N, u), uu=(1, N, u), params=(1, 3)).items():
        assert getattr(p, k).shape == s, k
    assert torch.equal(p.Q[0], torch.as_tensor(one["Q"])) and torch.equal(p.X_prev, torch.zeros(1, N, x, dtype=torch.float64))
    q = _build(dict(a, x0=None))  # no x0 (the controller's case): nothing to promote
    assert q.x0 is None and not q.single and q.M == M


def test_the_caller_chooses_who_owns_the_references():
    M, N, x, u = SHAPES[0]
    a = {k: torch.as_tensor(v) for k, v in _args(*SHAPES[0]).items()}
    lo, hi, P = -torch.ones(M, N, u, dtype=torch.float64), torch.ones(M, N, u, dtype=torch.float64), torch.ones(M, 3, dtype=torch.float64)
    for own in (False, True):
        p = _build(a, u_l=lo, u_u=hi, builtin_model="unicycle", params=P, own_copies=own)
        for mine, theirs in ((p.X_ref, a["X_ref"]), (p.U_ref, a["U_ref"]), (p.lu, lo), (p.uu, hi), (p.params, P)):
            assert torch.equal(mine, theirs) and (mine.data_ptr() != theirs.data_ptr()) == own
        assert p.X_prev.data_ptr() not in (p.X_ref.data_ptr(), a["X_ref"].data_ptr())  # the start iterate is overwritten: always a copy
    Xp = torch.zeros(M, N, x, dtype=torch.float64)
    assert _build(a, X_prev=Xp).X_prev.data_ptr() != Xp.data_ptr()


def test_models():
    a = _args(*SHAPES[0])
    assert _build(a).model is None and _build(a).params is None
    for k, name in enumerate(("unicycle", "quadrotor", "bicycle")):
        p = _build(a, builtin_model=name, params=np.ones((2, 3)))
        assert p.model == k and p.params.shape == (2, 3) and p.params.is_contiguous()
    with pytest.raises(ValueError, match="unknown built-in model"):
        _build(a, builtin_model="tricycle", params=np.ones((2, 3)))
    with pytest.raises(AssertionError, match="needs `params`"):
        _build(a, builtin_model="unicycle")


@pytest.mark.parametrize("boxes", ["nan", "both", "none"])
@pytest.mark.parametrize("shape", SHAPES)
def test_keepout_static_arrays_are_those_of_the_specification(shape, boxes):
    M, N, x, u = shape
    K, reg_x = 2, 0.7
    a = _args(*shape)
    rng = np.random.default_rng(2)
    xl, xu = (None, None) if boxes == "none" else (-1.0 - rng.random((M, N, x)), 1.0 + rng.random((M, N, x)))
    if boxes == "nan":
        xl[0, 1, 2] = xu[1, 0, 3] = xu[1, 2, 0] = xl[1, 2, 0] = np.nan
    cstr = dict(kind="keepout", pos_idx=(0, 1), centres=rng.standard_normal((K, 2)), radius=np.array([0.5, 0.25]))
    f, fx, fu = rng.standard_normal((M, N, x)), rng.standard_normal((M, N, x, x)), rng.standard_normal((M, N, x, u))
    want = ec.keepout_augment(cstr, a["x0"], f, fx, fu, a["X_ref"], a["X_ref"], a["Q"], reg_x, xl, xu)
    p = _build(a, x_l=xl, x_u=xu, reg_x=reg_x)
    got = keepout_static(p, K)
    assert np.array_equal(got["Qa"].transpose(-1, -2).numpy(), want["Q"]) and got["Qa"].is_contiguous()
    assert np.array_equal(got["x0"].numpy(), want["x0"])
    assert np.array_equal(got["lx"].numpy(), want["x_l"])
    assert np.array_equal(got["xu"].numpy()[..., :x], want["x_u"][..., :x])
    assert got["xu"].shape == (M, N, x + K) and bool(torch.isinf(got["xu"][..., x:]).all())  # (the rows' right-hand sides: every iteration's)
