"""The load half of the runtime-compiled models, costs and constraints (pmpc_amd/csrc/jit_module.hip; include/pmpc_abi.h: pmpc_model_load,
pmpc_cost_load, pmpc_cstr_load and their _unload): the refusals -2 and -3 through the library's entry points, that a refused load leaves
neither a HIP error nor a table entry behind, the ids, and the unload of everything a solver owns when it closes.  Every input is a valid
code object or a null.  The launches are M = 3, N = 2: six units, a partial block; tolerances are those of test_custom_*_gpu.py."""
import numpy as np
import pytest

from tests.support import custom_costs as cc
from tests.support import custom_cstrs as cg
from tests.support import custom_models as cm

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-12, atol=1e-12)  # AD against closed forms (tests/test_custom_model_gpu.py, _cost_gpu.py, _cstr_gpu.py)
M, N = 3, 2

# per kind: the stated dimensions of `first`, each of them off by one (for a cost also uses_u flipped), dimensions outside the limits,
# and the kind whose code object must be refused here (its dims symbol is absent)
KINDS = {
    "model": dict(dims=(4, 2, 2), off=[(5, 2, 2), (4, 3, 2), (4, 2, 3)], outside=[(17, 2, 2), (4, 0, 2), (4, 2, 17)], other="cost"),
    "cost": dict(dims=(4, 2, 4, 1), off=[(5, 2, 4, 1), (4, 3, 4, 1), (4, 2, 5, 1), (4, 2, 4, 0)], outside=[(17, 2, 4, 1), (4, 0, 4, 1), (4, 2, 65, 1)], other="cstr"),
    "cstr": dict(dims=(4, 2, 3), off=[(5, 2, 3), (4, 3, 3), (4, 2, 4)], outside=[(4, 5, 3), (13, 4, 3), (4, 2, 65)], other="model"),
}


@pytest.fixture(scope="module")
def objects():
    """kind -> (first, second): two different objects per kind, each compiled once for the module."""
    return dict(model=(cm.make("bicycle"), cm.make("pendulum")), cost=(cc.make("soft_speed"), cc.make("obstacles_u")),
                cstr=(cg.make("speed_band"), cg.make("log")))


def _fresh():
    from pmpc_amd.device import DeviceSolver

    return DeviceSolver(0)


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _object_code(s, obj):
    import torch

    return obj.compile(torch.cuda.get_device_properties(s.device).gcnArchName.split(":")[0])


def _lib_load(s, kind):
    return getattr(s.lib, f"pmpc_{kind}_load")


def _load(s, kind, obj):
    return dict(model=s.load_model, cost=s.load_cost, cstr=s.load_cstr)[kind](obj)


def _launch_is_right(s, kind, obj):
    """One launch of `obj` (the `first` of its kind) on `s` against the support module's closed form."""
    def got(*ts):
        s.sync()
        return [t.cpu().numpy() for t in ts]

    if kind == "model":
        x0, Xp, Up, P = cm.rand_inputs("bicycle", M, N, seed=1)
        f, fx, fu = got(*s.linearize(s.load_model(obj), _dev(x0), _dev(Xp), _dev(Up), _dev(P)))
        want = cm.CLOSED_FORMS["bicycle"](np.concatenate([x0[:, None], Xp[:, :-1]], 1), Up, P)
        have = (f, np.swapaxes(fx, -1, -2), np.swapaxes(fu, -1, -2))  # ABI blocks are [column][row]
    elif kind == "cost":
        X, U, P = cc.rand_inputs("soft_speed", M, N, seed=2)
        cx, cu, val = got(*s.custom_cost_grad(obj, _dev(X), _dev(U), _dev(P), value=True))
        want, have = cc.soft_speed_np(X, U, P), (val, cx, cu)
    else:
        X, P = cg.rand_inputs("speed_band", M, N, seed=3)
        have = got(*s.custom_cstr_rows(obj, _dev(X), _dev(P), value=True, check=True))
        want = cg.rows_np("speed_band", X, P)
    for h, w in zip(have, want):
        np.testing.assert_allclose(h, w, **TOL)


@pytest.mark.parametrize("kind", list(KINDS))
def test_refused_loads_leave_nothing_behind(objects, kind):
    k = KINDS[kind]
    first, second = objects[kind]
    s = _fresh()
    try:
        load, code = _lib_load(s, kind), _object_code(s, first)
        for dims in k["off"]:  # compiled for other than what is stated
            assert load(s.h, code, len(code), *dims) == -3, dims
        foreign = _object_code(s, objects[k["other"]][0])  # a code object of another kind
        assert load(s.h, foreign, len(foreign), *k["dims"]) == -3
        assert load(s.h, code, 0, *k["dims"]) == -2
        assert load(s.h, None, len(code), *k["dims"]) == -2
        assert load(None, code, len(code), *k["dims"]) == -2
        for dims in k["outside"]:
            assert load(s.h, code, len(code), *dims) == -2, dims
        i = _load(s, kind, first)
        assert i >= 1000 and _load(s, kind, first) == i
        j = _load(s, kind, second)
        assert j >= 1000 and j != i
        _launch_is_right(s, kind, first)
    finally:
        s.close()


def test_close_unloads_every_kind_and_ids_belong_to_their_solver(objects):
    s1, s2 = _fresh(), _fresh()
    try:
        ids = {kind: _load(s1, kind, objects[kind][0]) for kind in KINDS}
        unload = lambda s, kind, i: getattr(s.lib, f"pmpc_{kind}_unload")(s.h, i)
        for kind, i in ids.items():
            assert unload(s2, kind, i) == 2  # an id of another solver
        s1.close()
        for kind, i in ids.items():
            assert unload(s2, kind, i) == 2  # ... and of a solver that is gone
        for kind in KINDS:  # the same three objects on a fresh solver
            i = _load(s2, kind, objects[kind][0])
            assert i >= 1000
            _launch_is_right(s2, kind, objects[kind][0])
            assert unload(s2, kind, i) == 0 and unload(s2, kind, i) == 2  # an unloaded id
    finally:
        s1.close()
        s2.close()
