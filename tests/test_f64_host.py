"""Host-side checks of the float64 engine (include/dibs_hip.h, dibs_config.reserved_i[1] = 64): the config field, and every unsupported
combination rejected at dibs_engine_create -- before any device call, so these run without a GPU -- and by the Python facade."""
import numpy as np
import pytest

from conftest import make_data
from dibs_amd._abi import make_config
from dibs_amd.inference import MarginalDiBS, sample_batch


def test_make_config_carries_precision():
    assert make_config(n_vars=5, n_particles=4, n_observations=10, precision=64).reserved_i[1] == 64
    assert make_config(n_vars=5, n_particles=4, n_observations=10).reserved_i[1] == 0   # float32: the field as before


@pytest.mark.parametrize("kw,msg", [
    (dict(joint=True, likelihood="lingauss"), "joint models are not supported"),
    (dict(joint=True, likelihood="densenn"), "joint models are not supported"),
    (dict(grad_estimator_z="reparam"), "reparam estimator is not supported"),
    (dict(n_ranks=2), "n_ranks must be 1"),
    (dict(n_problems=2), "n_problems must be 1"),
    (dict(n_vars=65), "n_vars must be in \\[2, 64\\]"),
    (dict(n_particles=1025), "n_particles must be <= 1024"),
    (dict(precision=16), "reserved_i\\[1\\] \\(precision\\) must be"),
])
def test_engine_create_rejects_unsupported_float64(kw, msg):
    from dibs_amd import _lib
    from dibs_amd.engine import Engine
    args = dict(n_vars=8, n_particles=4, n_observations=20, precision=64)
    args.update(kw)
    with pytest.raises(_lib.DibsHipError, match="^float64 engine: .*" + msg):
        Engine(make_config(**args))


def test_marginal_dibs_precision_argument():
    data, gm, lm = make_data(5)
    with pytest.raises(ValueError, match="precision"):
        MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, precision="float16")
    m = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, precision="float64")
    assert m.precision == "float64"
    assert m._make_config(4, 5).reserved_i[1] == 64
    assert MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)._make_config(4, 5).reserved_i[1] == 0


def test_float64_model_rejects_what_it_does_not_support():
    data, gm, lm = make_data(5)
    m = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, precision="float64")
    z = np.zeros((2, 5, 5, 2))
    keys = np.zeros((2, 2), np.uint32)
    with pytest.raises(NotImplementedError, match="float64"):
        m.eltwise_grad_z_likelihood(z, None, np.zeros(2), 1, keys)
    with pytest.raises(NotImplementedError, match="float64"):
        m.eltwise_grad_latent_prior(z, keys, 1)
    with pytest.raises(NotImplementedError, match="float64"):
        m.eltwise_log_marginal_likelihood_observ(np.zeros((1, 5, 5), np.int32), data.x)
    with pytest.raises(NotImplementedError, match="float64"):
        m.eltwise_log_joint_prob(np.zeros((1, 5, 5), np.int32), None)
    from dibs_amd.distributed import sample_sharded, sample_sharded_native
    for f in (sample_sharded, sample_sharded_native):
        with pytest.raises(NotImplementedError, match="float64"):
            f(m, key=0, n_particles=4, steps=2)


def test_sample_batch_rejects_float64_models():
    data, gm, lm = make_data(6)
    a = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, precision="float64")
    b = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, precision="float64")
    with pytest.raises(ValueError, match="float64"):
        sample_batch([a, b], keys=[0, 1], n_particles=4, steps=2)
    with pytest.raises(ValueError, match="float64"):
        sample_batch([MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm), a], keys=[0, 1], n_particles=4, steps=2)
