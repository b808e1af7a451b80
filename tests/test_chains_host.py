"""Host-side checks of the chains engine (include/dibs_hip.h, dibs_config.reserved_i[2] = n_chains) and of sample_chains: the
configuration field, what dibs_engine_create rejects before any device call, and what sample_chains rejects before any device work -- so
these run without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import make_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = r"^chains engine \(n_chains > 1\): "


def _joint(d=5, seed=3, **kw):
    from dibs_amd.inference import JointDiBS
    data, gm, lm = make_data(d, seed=seed, joint=True)
    return JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, **kw)


def _marginal(d=5, seed=0, **kw):
    from dibs_amd.inference import MarginalDiBS
    data, gm, lm = make_data(d, seed=seed)
    return MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, **kw)


def test_sample_chains_is_exported():
    import dibs_amd.inference as inf
    from dibs_amd.inference.chains import sample_chains
    assert inf.sample_chains is sample_chains


def test_make_config_sets_n_chains():
    from dibs_amd._abi import make_config
    kw = dict(n_vars=8, n_particles=4, n_observations=40, joint=True, likelihood="lingauss")
    c = make_config(**kw)
    assert list(c.reserved_i) == [1, 0, 0, 0, 0]
    c = make_config(n_chains=5, **kw)
    assert c.reserved_i[2] == 5 and c.reserved_i[0] == 1 and c.reserved_i[1] == 0


def test_header_documents_the_field():
    src = open(os.path.join(ROOT, "include", "dibs_hip.h")).read()
    assert re.search(r"\[2\] n_chains", src) and "CHAINS ENGINE" in src


JOINT = dict(n_vars=8, n_particles=4, n_observations=40, joint=True, likelihood="lingauss")


@pytest.mark.parametrize("kw,msg", [
    (dict(n_chains=-1), "n_chains .* must be >= 0"),
    (dict(n_chains=2, n_problems=2), "n_problems"),
    (dict(n_chains=2, n_problems=2, joint=False, likelihood="bge"), "n_problems"),
    (dict(n_chains=2, joint=False, likelihood="bge"), "marginal models are not supported"),
    (dict(n_chains=2, n_ranks=2), "n_ranks must be 1"),
    (dict(n_chains=2, precision=64), "float64"),
    (dict(n_chains=2, precision=64, joint=False, likelihood="bge", grad_estimator_z="score"), "marginal models|float64"),
    (dict(n_chains=2, n_particles=256), "must be < 256"),
    (dict(n_chains=3, n_particles=255, likelihood="densenn"), None),                       # (accepted: the first failure is the device's)
    (dict(n_chains=(1 << 17) + 1, n_particles=128), r"must be <= 2\^24"),
    (dict(n_chains=3000, n_particles=128, n_vars=100), r"would pass 2\^31 elements"),     # (packed rows: 3000 * 128 * 60 004 floats)
    (dict(n_chains=40000, n_particles=8, n_vars=40, n_acyclicity_mc_samples=64), r"would pass 2\^31 elements"),   # (acyclicity partial sums)
    (dict(n_chains=60000, n_particles=16, n_grad_mc_samples=4096), r"would pass 2\^31 elements"),                 # (log-probabilities)
])
def test_engine_create_rejects_unsupported_chains(kw, msg):
    import torch
    from dibs_amd import _lib
    from dibs_amd._abi import make_config
    from dibs_amd.engine import Engine
    _lib.build()
    cfg = make_config(**dict(JOINT, **kw))
    if msg is None:
        if torch.cuda.is_available():
            Engine(cfg).close()
            return
        with pytest.raises(_lib.DibsHipError) as ei:
            Engine(cfg)
        assert not re.search(PREFIX, str(ei.value)), str(ei.value)
        return
    with pytest.raises(_lib.DibsHipError, match=PREFIX + ".*(" + msg + ")"):
        Engine(cfg)


def test_null_engine_is_refused_by_the_entry_points_chains_use():
    from dibs_amd import _lib
    _lib.build()
    lib = _lib.load()
    keys = (ctypes.c_uint32 * 4)()
    assert lib.dibs_engine_init_particles_batch(None, keys) != 0 and lib.dibs_engine_get_keys(None, keys) != 0


@pytest.mark.parametrize("keys,msg", [
    ([], "empty"),
    (5, "sequence"),
    ([[1, 2, 3], [4, 5, 6]], "key 0 is not a PRNG key"),
    ([np.zeros(2, np.uint32), np.zeros((2, 2), np.uint32)], "key 1 is not a PRNG key"),
    ([np.zeros(2, np.float32), np.zeros(2, np.float32)], "key 0 is not a PRNG key"),
])
def test_sample_chains_rejects_bad_keys(keys, msg):
    from dibs_amd.inference import sample_chains
    with pytest.raises(ValueError, match=msg):
        sample_chains(_joint(), keys=keys, n_particles=4, steps=2)
    with pytest.raises(ValueError, match=msg):
        sample_chains(_marginal(), keys=keys, n_particles=4, steps=2)


def test_sample_chains_rejects_float64_and_non_models():
    from dibs_amd.inference import sample_chains
    with pytest.raises(ValueError, match="float64"):
        sample_chains(_marginal(precision="float64"), keys=[0, 1], n_particles=4, steps=2)
    for bad in (object(), None, "JointDiBS", [_joint(), _joint()]):
        with pytest.raises(ValueError, match="must be a JointDiBS or a MarginalDiBS"):
            sample_chains(bad, keys=[0, 1], n_particles=4, steps=2)


def test_marginal_model_keeps_the_rules_of_sample_batch():
    from dibs_amd.inference import sample_chains
    with pytest.raises(ValueError, match="score-function"):
        sample_chains(_marginal(grad_estimator_z="reparam"), keys=[0, 1], n_particles=4, steps=2)


@pytest.mark.parametrize("make", [_joint, _marginal])
def test_one_key_is_plain_sample(make, monkeypatch):
    from dibs_amd import random
    from dibs_amd.inference import sample_chains
    m = make()
    calls = []

    def fake_sample(**kw):
        calls.append(kw)
        m.last_state = dict(z="state")
        return "result"
    monkeypatch.setattr(m, "sample", fake_sample)
    cb = lambda **kw: None
    out = sample_chains(m, keys=[7], n_particles=4, steps=6, n_dim_particles=3, callback=cb, callback_every=2)
    assert out == ["result"] and len(calls) == 1
    kw = calls[0]
    assert np.array_equal(kw.pop("key"), random.PRNGKey(7))
    assert kw == dict(n_particles=4, steps=6, n_dim_particles=3, callback=cb, callback_every=2)
    assert m.last_chain_states == [dict(z="state")]
