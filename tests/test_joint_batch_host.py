"""Host-side checks of sample_joint_batch (dibs_amd/inference/joint_batch.py): everything it rejects is rejected before an engine is
created, so these run without a GPU -- Engine is replaced by a class that fails the test when it is constructed."""
import re

import numpy as np
import pytest

from conftest import make_data

ROOT_ARGS = dict(n_particles=4, steps=2)


def _joint(d=5, seed=3, n_obs=100, **kw):
    from dibs_amd.inference import JointDiBS
    data, gm, lm = make_data(d, seed=seed, n_obs=n_obs, joint=True)
    return JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, **kw)


def _marginal(d=5, seed=0):
    from dibs_amd.inference import MarginalDiBS
    data, gm, lm = make_data(d, seed=seed)
    return MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)


def _densenn(d=5):
    from dibs_amd import random
    from dibs_amd.inference import JointDiBS
    from dibs_amd.target import make_nonlinear_gaussian_model
    data, gm, lm = make_nonlinear_gaussian_model(key=random.PRNGKey(0), n_vars=d, graph_prior_str="er", n_observations=40)
    return JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm)


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    import dibs_amd.inference.joint_batch as jb

    class NoEngine:
        def __init__(self, *a, **kw):
            raise AssertionError("sample_joint_batch created an engine before it had validated its arguments")
    monkeypatch.setattr(jb, "Engine", NoEngine)


def test_sample_joint_batch_is_exported():
    import dibs_amd.inference as inf
    from dibs_amd.inference.joint_batch import sample_joint_batch
    assert inf.sample_joint_batch is sample_joint_batch


def test_empty_list_returns_empty_list():
    from dibs_amd.inference import sample_joint_batch
    assert sample_joint_batch([], keys=[], **ROOT_ARGS) == []


@pytest.mark.parametrize("bad", ["marginal", "object", "none"])
def test_rejects_models_that_are_no_joint_dibs(bad):
    from dibs_amd.inference import sample_joint_batch
    other = dict(marginal=_marginal, object=object, none=lambda: None)[bad]()
    with pytest.raises(ValueError, match="every model must be a JointDiBS, model 1 is a"):
        sample_joint_batch([_joint(), other], keys=[0, 1], **ROOT_ARGS)


def test_rejects_dense_nonlinear_gaussian_and_points_to_the_alternatives():
    from dibs_amd.inference import sample_joint_batch
    with pytest.raises(ValueError, match=r"model 1 has a DenseNonlinearGaussian likelihood.*sample_chains.*sample\(\)"):
        sample_joint_batch([_joint(), _densenn()], keys=[0, 1], **ROOT_ARGS)


def test_rejects_float64_models():
    from dibs_amd.inference import sample_joint_batch
    m = _joint()
    m.precision = "float64"
    with pytest.raises(ValueError, match="float64 models are not supported"):
        sample_joint_batch([_joint(), m], keys=[0, 1], **ROOT_ARGS)


@pytest.mark.parametrize("n_keys", [1, 3])
def test_rejects_a_key_count_that_differs_from_the_model_count(n_keys):
    from dibs_amd.inference import sample_joint_batch
    with pytest.raises(ValueError, match=f"2 models but {n_keys} keys"):
        sample_joint_batch([_joint(), _joint(seed=4)], keys=list(range(n_keys)), **ROOT_ARGS)


@pytest.mark.parametrize("kw,fields", [
    (dict(d=6), ["n_vars"]),
    (dict(n_obs=90), ["n_observations"]),
    (dict(alpha_linear=0.1), ["alpha_linear"]),
    (dict(n_grad_mc_samples=64, tau=2.0), ["tau", "n_grad_mc_samples"]),
    (dict(grad_estimator_z="score"), ["grad_estimator_z"]),
    (dict(optimizer="gd"), ["optimizer"]),
    (dict(kernel_param={"h_latent": 5.0, "h_theta": 100.0}), ["h_theta"]),
])
def test_rejects_models_that_disagree_on_what_the_batch_shares(kw, fields):
    from dibs_amd.inference import sample_joint_batch
    with pytest.raises(ValueError, match="model 2 differs from model 0 in ") as ei:
        sample_joint_batch([_joint(), _joint(seed=4), _joint(seed=5, **kw)], keys=[0, 1, 2], **ROOT_ARGS)
    named = re.search(r"differs from model 0 in ([\w, ]+) \(", str(ei.value)).group(1).split(", ")
    for f in fields:
        assert f in named, (f, named)
    assert "has_interventions" not in named and "reserved_i" not in named


def test_data_interventions_and_keys_may_differ():
    """Two models that differ in data, interventions and key only pass validation: the next thing that happens is the engine."""
    from dibs_amd.inference import JointDiBS, sample_joint_batch
    data, gm, lm = make_data(5, seed=4, joint=True)
    mask = np.zeros(np.asarray(data.x).shape, np.int32)
    mask[:3, 1] = 1
    b = JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, interv_mask=mask)
    with pytest.raises(AssertionError, match="created an engine"):
        sample_joint_batch([_joint(), b], keys=[0, 1], **ROOT_ARGS)


def test_one_model_is_plain_sample(monkeypatch):
    from dibs_amd import random
    from dibs_amd.inference import sample_joint_batch
    m = _joint()
    calls = []

    def fake_sample(**kw):
        calls.append(kw)
        return "result"
    monkeypatch.setattr(m, "sample", fake_sample)
    cb = lambda **kw: None
    out = sample_joint_batch([m], keys=[7], n_particles=4, steps=6, n_dim_particles=3, callback=cb, callback_every=2)
    assert out == ["result"] and len(calls) == 1
    kw = calls[0]
    assert np.array_equal(kw.pop("key"), random.PRNGKey(7))
    assert kw == dict(n_particles=4, steps=6, n_dim_particles=3, callback=cb, callback_every=2)
