"""Registers and scratch of the compiled active-set sweeps (pmpc_amd/csrc/kernels_as.hip), read from the loaded code object
(pmpc_as_sweep_resources -> hipFuncGetAttributes; nothing is launched).

The sweeps of the flagship shape are bound by vector-instruction issue at FOUR waves per SIMD, and sit on the 128-register step that
allows four: the deep full factor sweep at 127 - 128, the two SENS forward sweeps at 125 - 128.  One register more costs the fourth
wave — a slowdown of the dominant kernels that no parity test sees.  Scratch in any sweep would be a spill in a stage loop."""
import itertools

import pytest

pytestmark = pytest.mark.gpu

# (sweep, variant record) of (12, 4) that must stay at four waves per SIMD: the lean and the deep full factor sweep
# (<12,4,0,false,false>, <12,4,1,false,true>) and the two SENS forward sweeps (DEFECT and not, on the three-stage ring)
FOUR_WAVES = [("bwd", (0, 0, 0, 0, 0)), ("bwd", (1, 0, 1, 0, 0)), ("fwd", (1, 1, 0, 0, 1)), ("fwd", (0, 1, 0, 0, 1))]
BWD_RECORDS = list(itertools.product(range(3), range(2), range(2), range(3), range(2)))  # (mode, skip, defect, ex, f32)
FWD_RECORDS = list(itertools.product(range(2), repeat=5))                                 # (defect, pf2, cone, f32, sens)


@pytest.mark.parametrize("sweep,variant", FOUR_WAVES, ids=[f"{s}-{''.join(map(str, v))}" for s, v in FOUR_WAVES])
def test_flagship_sweeps_stay_on_the_four_wave_step(sweep, variant):
    from pmpc_amd import _lib

    r = _lib.as_sweep_resources(sweep, 12, 4, variant)
    assert r is not None, "not compiled"
    print(sweep, variant, r)
    assert r["regs"] <= 128, r
    assert r["scratch_bytes"] == 0, r


@pytest.mark.parametrize("x,u", [(12, 4), (4, 2)])
def test_no_compiled_sweep_uses_scratch(x, u):
    from pmpc_amd import _lib

    seen = 0
    for sweep, records in (("bwd", BWD_RECORDS), ("fwd", FWD_RECORDS)):
        for v in records:
            r = _lib.as_sweep_resources(sweep, x, u, v)
            if r is None:
                continue
            seen += 1
            print(sweep, v, r)
            assert r["scratch_bytes"] == 0 and r["regs"] > 0 and r["max_threads"] >= 64, (sweep, v, r)
    assert seen >= 20, seen  # (the plain family alone has 9 factor and 4 forward sweeps)
