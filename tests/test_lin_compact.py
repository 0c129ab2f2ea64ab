"""Compact Jacobian records of the built-in models (pmpc_amd/csrc/jac_compact.h): the table of live entries against the numpy
specification of the models.  No GPU: the table is read from the built library on the host."""
import numpy as np
import pytest


def _jacobians(model, rng, n):
    """Jacobians of ONE particle (fixed parameters) at n random states / controls: what a compact record may treat as constant
    must not move here."""
    from pmpc_amd import dynamics as dyn

    if model == "unicycle":
        p = np.array([1.0 + 0.1 * rng.standard_normal(), 1.0 + 0.1 * rng.standard_normal(), 0.3])
        x = rng.standard_normal((n, 4)) * 2.0
        u = rng.standard_normal((n, 2))
        u = np.sign(u) * (0.1 + np.abs(u))
        _, fx, fu = dyn.unicycle(x, u, p[None, :])
    else:
        p = np.array([1.0, 0.01, 0.012, 0.02]) * (1.0 + 0.1 * rng.standard_normal(4))
        x = rng.standard_normal((n, 12))
        x[:, 7] = np.clip(x[:, 7], -1.2, 1.2)  # (pitch away from the Euler-angle singularity)
        u = rng.standard_normal((n, 4))
        u[:, 0] += 9.81
        _, fx, fu = dyn.quadrotor(x, u, p[None, :])
    return fx, fu


@pytest.mark.parametrize("model,mid,x,u,live", [("unicycle", 0, 4, 2, (4, 4)), ("quadrotor", 1, 12, 4, (25, 3))])
def test_entries_the_compact_records_hold_constant_are_constant_in_the_numpy_model(model, mid, x, u, live):
    from pmpc_amd import _lib

    mx, mu = _lib.jac_live_mask(mid, x, u)
    assert mx.shape == (x, x) and mu.shape == (x, u)
    assert (int(mx.sum()), int(mu.sum())) == live  # (the counts the design was sized for: a larger table would still be correct, only larger)
    rng = np.random.default_rng(7)
    for _ in range(3):  # three particles with parameters of their own
        fx, fu = _jacobians(model, rng, 200)
        moves_x = np.ptp(fx, axis=0) > 0.0
        moves_u = np.ptp(fu, axis=0) > 0.0
        assert not (moves_x & ~mx).any(), np.argwhere(moves_x & ~mx)
        assert not (moves_u & ~mu).any(), np.argwhere(moves_u & ~mu)
        # and the table is not lazy: every entry it stores per stage does move
        assert (moves_x | ~mx).all() and (moves_u | ~mu).all()


def test_unknown_model_has_no_compact_records():
    from pmpc_amd import _lib

    with pytest.raises(ValueError):
        _lib.jac_live_mask(5, 4, 2)
    with pytest.raises(ValueError):
        _lib.jac_live_mask(0, 12, 4)
