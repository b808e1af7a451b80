"""The repair of a lost in-kernel flag (include/dibs_hip.h: dibs_engine_flag_fallbacks) in the FIRST guarded chunk of an engine: that chunk
also allocates the chunk-start copy of the loop carry, so the copy must not race with anything the allocation leaves queued (a zero fill
on the null stream, which the engine's non-blocking stream does not wait for, could land after the copy and wipe it).  Every fresh engine
must end bit-identical to the undisturbed run."""
import numpy as np
import pytest

from dibs_amd import random as prng

pytestmark = pytest.mark.gpu

CASE = dict(d=50, M=128, S=64, Sa=16, chunks=[[0, 3], [3, 3], [6, 2]], seed=5, data_seed=1)


@pytest.fixture(autouse=True)
def _flags_even_with_other_engines_alive(monkeypatch):
    monkeypatch.setenv("DIBS_FLAGS_MULTI", "1")   # (latched at creation: the engines below use the flags although others are alive)


def _run(drop_first):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    from dibs_amd.engine import Engine
    from ipc_rank_worker import case_config, case_data
    eng = Engine(case_config(CASE))
    try:
        eng.set_data(case_data(CASE))
        eng.init_particles(prng.PRNGKey(CASE["seed"]))
        for i, (t0, n) in enumerate(CASE["chunks"]):
            if drop_first and i == 0:
                eng.debug_drop_next_flag()
            eng.run(t0, n)
        return eng.get_state(), eng.flag_fallbacks()
    finally:
        eng.close()


def test_lost_flag_in_the_first_chunk_of_fresh_engines():
    ref, fb0 = _run(False)
    assert fb0 == 0
    for rep in range(3):   # (three fresh engines: three fresh copy buffers)
        got, fb = _run(True)
        assert fb == 1, "the first chunk must have been repeated exactly once (is the engine using the flags at all?)"
        for k in ("z", "v_z", "baseline", "key"):
            assert np.array_equal(got[k], ref[k]), (rep, k)
