"""Host-side checks of the batched engine (include/dibs_hip.h, n_problems > 1) and of sample_batch: everything that must be rejected
is rejected before any device work, so these run without a GPU."""
import pytest

from conftest import make_data
from dibs_amd._abi import make_config
from dibs_amd.inference import MarginalDiBS, sample_batch
from dibs_amd.kernel import AdditiveFrobeniusSEKernel


def _model(d=6, seed=0, **kw):
    data, gm, lm = make_data(d, seed=seed)
    return MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, **kw)


def test_make_config_carries_n_problems():
    c = make_config(n_vars=5, n_particles=4, n_observations=10, n_problems=3)
    assert c.reserved_i[0] == 3
    assert make_config(n_vars=5, n_particles=4, n_observations=10).reserved_i[0] == 1


@pytest.mark.parametrize("kw", [
    dict(n_grad_mc_samples=64),
    dict(n_acyclicity_mc_samples=8),
    dict(alpha_linear=0.5),
    dict(beta_linear=2.0),
    dict(tau=0.5),
    dict(score_function_baseline=0.1),
    dict(optimizer="gd"),
    dict(optimizer_param={"stepsize": 0.01}),
    dict(kernel=AdditiveFrobeniusSEKernel, kernel_param={"h": 3.0}),
    dict(latent_prior_std=0.5),
])
def test_sample_batch_rejects_models_that_differ(kw):
    a, b = _model(seed=0), _model(seed=1, **kw)
    with pytest.raises(ValueError, match="differs from model 0"):
        sample_batch([a, b], keys=[0, 1], n_particles=4, steps=2)


def test_sample_batch_rejects_other_sizes_priors_and_bge_parameters():
    a = _model(d=6)
    with pytest.raises(ValueError, match="n_vars"):
        sample_batch([a, _model(d=7)], keys=[0, 1], n_particles=4, steps=2)
    data, gm, lm = make_data(6, seed=1, prior="sf")
    with pytest.raises(ValueError, match="graph_prior"):
        sample_batch([a, MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)], keys=[0, 1], n_particles=4, steps=2)
    data, gm, lm = make_data(6, seed=1, edges_per_node=1)
    with pytest.raises(ValueError, match="graph_prior_edges_per_node"):
        sample_batch([a, MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)], keys=[0, 1], n_particles=4, steps=2)
    from dibs_amd import random
    from dibs_amd.target import make_linear_gaussian_equivalent_model
    for extra, field in ((dict(bge_alpha_mu=2.0), "bge_alpha_mu"), (dict(bge_alpha_lambd=20.0), "bge_alpha_lambd")):
        data, gm, lm = make_linear_gaussian_equivalent_model(key=random.PRNGKey(3), n_vars=6, graph_prior_str="er", **extra)
        with pytest.raises(ValueError, match=field):
            sample_batch([a, MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)], keys=[0, 1], n_particles=4, steps=2)


def test_sample_batch_rejects_reparam_and_key_count():
    with pytest.raises(ValueError, match="score-function"):
        sample_batch([_model(), _model(grad_estimator_z="reparam")], keys=[0, 1], n_particles=4, steps=2)
    with pytest.raises(ValueError, match="keys"):
        sample_batch([_model(), _model(seed=1)], keys=[0], n_particles=4, steps=2)


def test_sample_batch_rejects_joint_models():
    from dibs_amd.inference import JointDiBS
    data, gm, lm = make_data(5, seed=3, joint=True)
    j = JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm)
    with pytest.raises(ValueError, match="MarginalDiBS"):
        sample_batch([j, j], keys=[0, 1], n_particles=4, steps=2)


@pytest.mark.parametrize("kw,msg", [
    (dict(joint=True, likelihood="lingauss"), "joint models are not supported"),
    (dict(joint=True, likelihood="densenn"), "joint models are not supported"),
    (dict(grad_estimator_z="reparam"), "reparam estimator is not supported"),
    (dict(n_ranks=2), "n_ranks must be 1"),
    (dict(n_particles=256), "must be < 256"),
    (dict(n_vars=100, n_particles=200, n_problems=2000), "must be < 2\\^32"),
])
def test_engine_create_rejects_unsupported_batches(kw, msg):
    from dibs_amd import _lib
    from dibs_amd.engine import Engine
    args = dict(n_vars=8, n_particles=4, n_observations=20, n_problems=2)
    args.update(kw)
    with pytest.raises(_lib.DibsHipError, match="batched engine \\(n_problems > 1\\): .*" + msg):
        Engine(make_config(**args))
