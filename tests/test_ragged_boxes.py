"""The gate of tests/test_ragged_boxes_gpu.py, on the CPU: every case of tests/support/ragged_boxes.py::TABLES is solved by the oracle
alone, its KKT certificate passes, the case meets check_conditions (so a kernel that ignored a removed side, applied every particle's own
box on the consensus stages or moved a pinned entry would give ANOTHER answer), and effective_boxes reads the boxes as
oracle/lqp_assemble.c does.  The generator's own promises, and check_conditions' refusals, are tested on hand-made inputs."""
import numpy as np
import pytest

from tests.support import ragged_boxes as rb

ALL = [(t, c) for t, cases in rb.TABLES.items() for c in cases]
# the certificate bound of oracle/lqp_oracle.py::solve_qp_exact (1e-9 max(1, |q|)) is asserted inside the oracle; its residuals are
# round-off of sparse solves refined three times (1e-13 and below at these sizes) — 1e-10 leaves room for the larger shapes and still is
# 1e3 below the GPU tests' tightest tolerance
CERT = 1e-10


@pytest.mark.parametrize("table,case", ALL, ids=[f"{t}-{rb.case_id(c)}" for t, c in ALL])
def test_case_is_certified_by_the_oracle_and_meets_its_conditions(table, case, oracle):
    ref = rb.reference(table, case)
    path, M, N, x, u, Nc, kind, b, extra = case
    Xo, Uo, info = ref["Xo"], ref["Uo"], ref["info"]
    assert np.all(np.isfinite(Xo)) and np.all(np.isfinite(Uo))
    qp = info.get("qp", info)  # (cone objective: the weighted QP's certificate)
    if "cert" in qp and "alpha" not in dict(extra):
        assert max(qp["cert"].values()) <= CERT, qp["cert"]
    elif path == "soc":  # the cone oracle returns no certificate: tests/support/kkt_certificate.py computes one from the answer
        from tests.support.kkt_certificate import kkt_certificate

        c = rb.soc_cone(u, b)
        kw = ref["kw"]
        elo, ehi = rb.effective_boxes(kw["u_l"], kw["u_u"], Nc)
        cert = kkt_certificate(*ref["args"], kw["reg_x"], kw["reg_u"], Nc, elo, ehi, Xo, Uo, soc=dict(W=c["W"], w0=c["w0"], v=c["v"], v0=c["v0"]), tol_act=1e-6)
        print(cert)
        assert max(v for v in cert.values() if isinstance(v, float)) <= 1e-6, cert
    out = rb.case_conditions(table, case, ref)
    print(rb.case_id(case), out)
    # oracle/lqp_assemble.c reads particle 0's boxes on the consensus stages: the caller's boxes and the effective ones are one problem
    kw = ref["kw"]
    elo, ehi = rb.effective_boxes(kw["u_l"], kw["u_u"], Nc)
    if rb.shared_stages(N, Nc) and M > 1:
        assert not (np.array_equal(elo, kw["u_l"]) and np.array_equal(ehi, kw["u_u"]))
    if path in ("qp", "xbox"):
        X2, U2 = oracle.lqp_solve_py(*ref["args"], Nc=Nc, **dict(kw, u_l=elo, u_u=ehi))
        assert np.max(np.abs(X2 - Xo)) <= 1e-12 * max(1.0, np.max(np.abs(Xo))) and np.max(np.abs(U2 - Uo)) <= 1e-12


@pytest.mark.parametrize("kind", rb.KINDS + ("mixed",))
def test_generator_draws_what_it_says(kind):
    M, N, u, b = 7, 9, 3, 0.4
    lo, hi, plo, phi = rb.ragged_boxes(np.random.default_rng(3), M, N, u, kind, b)
    assert all(a.shape == (M, N, u) and a.dtype == np.float64 for a in (lo, hi, plo, phi))
    assert not np.isnan(lo).any() and not np.isnan(hi).any() and np.all(lo <= hi)
    assert np.all((plo <= -0.5 * b) & (plo >= -1.5 * b) & (phi >= 0.5 * b) & (phi <= 1.5 * b)) or kind == "offset"
    assert len(np.unique(phi)) == M * N * u  # per particle, stage and control
    if kind == "per_entry":
        assert np.array_equal(lo, plo) and np.array_equal(hi, phi)
    if kind == "one_sided":
        no_lo, no_hi = np.isneginf(lo), np.isposinf(hi)
        assert not (no_lo & no_hi).any() and min(no_lo.sum(), no_hi.sum(), (~no_lo & ~no_hi).sum()) > M * N * u // 5
        assert np.array_equal(lo[~no_lo], plo[~no_lo]) and np.array_equal(hi[~no_hi], phi[~no_hi])
    if kind == "upper_only":
        assert np.isneginf(lo).all() and np.array_equal(hi, phi)
    if kind == "pinned":
        pin = lo == hi
        assert M * N * u // 8 < pin.sum() < M * N * u // 2 and np.all((lo[pin] >= plo[pin]) & (hi[pin] <= phi[pin]))
        assert np.array_equal(lo[~pin], plo[~pin]) and np.array_equal(hi[~pin], phi[~pin])
    if kind == "offset":
        assert np.all((hi - lo >= 0.1 - 1e-12) & (hi - lo <= 1.0 + 1e-12)) and ((lo > 0) | (hi < 0)).sum() > M * N * u // 4
    if kind == "mixed":
        assert np.isneginf(lo).any() and np.isposinf(hi).any() and (lo == hi).any() and ((lo > 0) | (hi < 0)).any()


def test_effective_boxes_writes_particle_0_onto_the_consensus_stages_only():
    lo, hi, _, _ = rb.ragged_boxes(np.random.default_rng(4), 4, 6, 2, "one_sided", 0.4)
    for Nc, k in ((0, 0), (2, 2), (-1, 6), (6, 6)):
        elo, ehi = rb.effective_boxes(lo, hi, Nc)
        assert np.array_equal(elo[:, k:], lo[:, k:]) and np.array_equal(ehi[:, k:], hi[:, k:])
        assert np.array_equal(elo[:, :k], np.broadcast_to(lo[:1, :k], (4, k, 2))) and np.array_equal(ehi[:, :k], np.broadcast_to(hi[:1, :k], (4, k, 2)))
    assert elo is not lo and not np.shares_memory(elo, lo)


def test_check_conditions_refuses_cases_that_cannot_tell():
    """Hand-made optima: each misses exactly one condition."""
    M, N, u = 2, 3, 1
    lo, hi = np.full((M, N, u), -1.0), np.full((M, N, u), 1.0)
    Uo = np.zeros((M, N, u))
    Uo[0, 1], Uo[0, 2] = -1.0, 1.0
    prev = np.zeros((M, N, u))
    rb.check_conditions("per_entry", Uo, lo, hi, (lo, hi), 0, prev)
    with pytest.raises(AssertionError, match="upper"):
        rb.check_conditions("per_entry", np.minimum(Uo, 0.5), lo, hi, (lo, hi), 0, prev)
    with pytest.raises(AssertionError, match="lower"):
        rb.check_conditions("per_entry", np.maximum(Uo, -0.5), lo, hi, (lo, hi), 0, prev)
    with pytest.raises(AssertionError, match="free"):
        rb.check_conditions("per_entry", np.where(Uo == 0, 1.0, Uo), lo, hi, (lo, hi), 0, prev)
    with pytest.raises(AssertionError, match="removed"):  # a side removed, but nothing goes beyond where it was
        lo1 = lo.copy()
        lo1[1, 0] = -np.inf
        rb.check_conditions("one_sided", Uo, lo1, hi, (lo, hi), 0, prev)
    with pytest.raises(AssertionError, match="pinned"):  # pinned where the parent's optimum already was
        lo2, hi2 = lo.copy(), hi.copy()
        lo2[1, 0] = hi2[1, 0] = 0.0
        rb.check_conditions("pinned", Uo, lo2, hi2, (lo, hi), 0, prev, U_parent=Uo)
    with pytest.raises(AssertionError, match="excludes"):
        rb.check_conditions("offset", Uo, lo, hi, (lo, hi), 0, prev)
    with pytest.raises(AssertionError, match="own box"):  # consensus: particle 1's own box holds the shared optimum too
        Uc = Uo.copy()
        Uc[1, 0] = Uc[0, 0]
        rb.check_conditions("per_entry", Uc, lo, hi, (lo, hi), 1, prev)
    lo3 = lo.copy()
    lo3[1, 0] = 0.5  # ... and now it does not
    rb.check_conditions("per_entry", Uc, lo3, hi, (lo, hi), 1, prev)


def test_tables_hold_the_shapes_and_kinds_the_paths_need():
    t = rb.TABLES
    assert {c[6] for c in t["qp"]} == set(rb.KINDS) and {c[5] for c in t["qp"]} >= {0, 1, 2, -1}
    assert {1, 65} <= {c[1] for c in t["qp"]} and 1 in {c[2] for c in t["qp"]}
    assert len({(tb, rb.case_seed(tb, c)) for tb, c in ALL}) == len(ALL)


def test_sequence_of_kinds_is_certified_step_by_step():
    """Section i of the GPU tests: sequence() asserts its own conditions (the removed side is one the previous optimum sat on, and the
    control moves beyond it; every boxed step holds controls on sides, leaves some free, and has a particle whose own box the shared
    optimum violates; moving particle 0's box moves the shared optimum)."""
    args, base, steps = rb.sequence()
    assert [st["name"] for st in steps] == list(rb.SEQ_STEPS)
    empty = steps[5]
    assert empty["Xo"] is None and np.sum(empty["lo"] > empty["hi"]) == 1
    assert all(np.all(np.isfinite(st["Uo"])) for st in steps if st["Uo"] is not None)
    assert np.array_equal(steps[7]["Uo"], steps[6]["Uo"]) and rb.rel(steps[9]["Uo"], steps[6]["Uo"]) > 1e-3
