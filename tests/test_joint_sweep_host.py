"""Host-side checks of sample_joint_sweep (dibs_amd/inference/joint_sweep.py) and of the per-chain hyper-parameters of the chains engine
(include/dibs_hip.h, dibs_engine_set_chain_hparams): everything a sweep rejects is rejected before an engine is created, so these run
without a GPU -- Engine is replaced by a class that fails the test when it is constructed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import make_data
from dibs_amd.kernel import JointAdditiveFrobeniusSEKernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT_ARGS = dict(n_particles=4, steps=2)


def _joint(d=5, seed=3, n_obs=100, data_kw=None, **kw):
    from dibs_amd.inference import JointDiBS
    data, gm, lm = make_data(d, seed=seed, n_obs=n_obs, joint=True, **(data_kw or {}))
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
            raise AssertionError("sample_joint_sweep created an engine before it had validated its arguments")
    monkeypatch.setattr(jb, "Engine", NoEngine)


def _sweep(models, keys=None, **kw):
    from dibs_amd.inference import sample_joint_sweep
    return sample_joint_sweep(models, keys=list(range(len(models))) if keys is None else keys, **dict(ROOT_ARGS, **kw))


def test_sample_joint_sweep_is_exported():
    import dibs_amd.inference as inf
    from dibs_amd.inference.joint_sweep import sample_joint_sweep
    assert inf.sample_joint_sweep is sample_joint_sweep


def test_empty_list_returns_empty_list():
    assert _sweep([], keys=[]) == []


def test_one_model_is_plain_sample(monkeypatch):
    from dibs_amd import random
    from dibs_amd.inference import sample_joint_sweep
    m = _joint()
    calls = []

    def fake_sample(**kw):
        calls.append(kw)
        return "result"
    monkeypatch.setattr(m, "sample", fake_sample)
    cb = lambda **kw: None
    out = sample_joint_sweep([m], keys=[7], n_particles=4, steps=6, n_dim_particles=3, callback=cb, callback_every=2)
    assert out == ["result"] and len(calls) == 1
    kw = calls[0]
    assert np.array_equal(kw.pop("key"), random.PRNGKey(7))
    assert kw == dict(n_particles=4, steps=6, n_dim_particles=3, callback=cb, callback_every=2)


# ---- what a sweep refuses --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,fields", [
    (dict(d=6), ["n_vars"]),
    (dict(n_obs=90), ["n_observations"]),
    (dict(n_grad_mc_samples=64, tau=2.0), ["tau", "n_grad_mc_samples"]),
    (dict(n_acyclicity_mc_samples=8), ["n_acyclicity_mc_samples"]),
    (dict(grad_estimator_z="score"), ["grad_estimator_z"]),
    (dict(optimizer="gd"), ["optimizer"]),
    (dict(kernel=JointAdditiveFrobeniusSEKernel, kernel_param={"h_latent": 5.0, "h_theta": 500.0, "scale_latent": 2.0}), ["scale_latent"]),
    (dict(kernel=JointAdditiveFrobeniusSEKernel, kernel_param={"h_latent": 5.0, "h_theta": 500.0, "scale_theta": 2.0}), ["scale_theta"]),
    (dict(data_kw=dict(prior="sf")), ["graph_prior"]),
])
def test_rejects_models_that_disagree_on_what_the_sweep_shares(kw, fields):
    with pytest.raises(ValueError, match="sample_joint_sweep: model 2 differs from model 0 in ") as ei:
        _sweep([_joint(), _joint(seed=4, alpha_linear=0.1), _joint(seed=5, **kw)])
    named = re.search(r"differs from model 0 in ([\w, ]+) \(", str(ei.value)).group(1).split(", ")
    for f in fields:
        assert f in named, (f, named)
    from dibs_amd._abi import JOINT_SWEEPABLE
    assert not set(named) & set(JOINT_SWEEPABLE) and "has_interventions" not in named and "reserved_i" not in named


def test_rejects_other_likelihood_parameters():
    from dibs_amd import random
    from dibs_amd.inference import JointDiBS
    from dibs_amd.target import make_linear_gaussian_model
    data, gm, lm = make_linear_gaussian_model(key=random.PRNGKey(3), n_vars=5, graph_prior_str="er", obs_noise=0.5)
    with pytest.raises(ValueError, match="differs from model 0 in .*lin_obs_noise"):
        _sweep([_joint(), JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm)])


def test_rejects_dense_nonlinear_gaussian_and_points_to_the_alternatives():
    with pytest.raises(ValueError, match=r"sample_joint_sweep: model 1 has a DenseNonlinearGaussian likelihood.*sample_chains.*sample\(\)"):
        _sweep([_joint(), _densenn()])


def test_rejects_marginal_models_and_points_to_sample_sweep():
    with pytest.raises(ValueError, match="sample_joint_sweep: model 1 is a MarginalDiBS.*sample_sweep"):
        _sweep([_joint(), _marginal()])


@pytest.mark.parametrize("bad", [object, lambda: None])
def test_rejects_models_that_are_no_joint_dibs(bad):
    with pytest.raises(ValueError, match="sample_joint_sweep: every model must be a JointDiBS, model 1 is a"):
        _sweep([_joint(), bad()])


def test_rejects_float64_models():
    m = _joint()
    m.precision = "float64"
    with pytest.raises(ValueError, match="sample_joint_sweep: float64 models are not supported"):
        _sweep([_joint(), m])


@pytest.mark.parametrize("n_keys", [1, 3])
def test_rejects_a_key_count_that_differs_from_the_model_count(n_keys):
    with pytest.raises(ValueError, match=f"sample_joint_sweep: 2 models but {n_keys} keys"):
        _sweep([_joint(), _joint(seed=4)], keys=list(range(n_keys)))


def test_swept_fields_beyond_64_variables_or_latent_dimensions_are_rejected_with_the_sizes():
    from dibs_amd.inference.joint_sweep import _plan
    a, b = _joint(d=65, n_obs=20), _joint(d=65, n_obs=20, seed=4, alpha_linear=0.5)
    with pytest.raises(ValueError, match=r"alpha_linear.*n_vars <= 64 and n_dim_particles <= 64 \(got 65, 65\)"):
        _plan([a, b], [0, 1], 4, None)
    with pytest.raises(ValueError, match=r"h_theta.*n_vars <= 64 and n_dim_particles <= 64 \(got 5, 65\)"):
        _plan([_joint(), _joint(seed=4, kernel_param={"h_latent": 5.0, "h_theta": 100.0})], [0, 1], 4, 65)
    _plan([a, _joint(d=65, n_obs=20, seed=4)], [0, 1], 4, None)   # (nothing swept: any size a batch accepts)


# ---- what a sweep accepts --------------------------------------------------------------------------------------------------------------
SWEPT = [
    (dict(alpha_linear=0.5), "alpha_linear"),
    (dict(beta_linear=2.0), "beta_linear"),
    (dict(kernel_param={"h_latent": 3.0, "h_theta": 500.0}), "h_latent"),
    (dict(kernel_param={"h_latent": 5.0, "h_theta": 100.0}), "h_theta"),
    (dict(optimizer_param={"stepsize": 0.01}), "stepsize"),
    (dict(score_function_baseline=0.1), "score_function_baseline"),
    (dict(latent_prior_std=0.5), "latent_prior_std"),
    (dict(data_kw=dict(edges_per_node=2)), "graph_prior_edges_per_node"),
]


@pytest.mark.parametrize("kw,field", SWEPT, ids=[f for _, f in SWEPT])
def test_models_that_differ_in_a_swept_field_pass_and_the_difference_arrives_per_model(kw, field):
    from dibs_amd._abi import JOINT_SWEEPABLE, ChainHparams
    from dibs_amd.inference.joint_sweep import _plan
    a, b = _joint(seed=3), _joint(seed=4, **kw)
    keys, n_dim, cfg, hps = _plan([a, b], [0, 1], 4, None)
    assert n_dim == 5 and cfg.n_vars == 5 and len(keys) == 2 and len(hps) == 2 and all(isinstance(h, ChainHparams) for h in hps)
    ha, hb = ({n: getattr(h, n) for n in JOINT_SWEEPABLE} for h in hps)
    assert [n for n in JOINT_SWEEPABLE if ha[n] != hb[n]] == [field]
    assert all(getattr(cfg, n) == ha[n] for n in JOINT_SWEEPABLE)        # the engine's config carries model 0's values
    ca, cb = (m._make_config(4, 5) for m in (a, b))
    assert all(hb[n] == getattr(cb, n) and ha[n] == getattr(ca, n) for n in JOINT_SWEEPABLE)
    with pytest.raises(AssertionError, match="created an engine"):           # (validation passed: the next thing is the engine)
        _sweep([a, b])


def test_latent_prior_std_default_and_its_explicit_value_are_the_same_setting():
    """An unset latent_prior_std travels as given (<= 0: the engine's default 1 / sqrt(k)); a model that spells the default out does not
    count as swept, and a model with another value does."""
    from dibs_amd.inference.joint_sweep import _plan
    default = float(np.float32(1.0) / np.sqrt(np.float32(5)))
    a, b, c = _joint(seed=3), _joint(seed=4, latent_prior_std=default), _joint(seed=5, latent_prior_std=0.5)
    _, _, cfg, hps = _plan([a, b, c], [0, 1, 2], 4, None)
    assert hps[0].latent_prior_std <= 0 and hps[1].latent_prior_std == default and hps[2].latent_prior_std == 0.5
    big = [_joint(d=65, n_obs=20, seed=3), _joint(d=65, n_obs=20, seed=4, latent_prior_std=float(np.float32(1.0) / np.sqrt(np.float32(65))))]
    _plan(big, [0, 1], 4, None)   # (not swept: no size limit applies)


def test_data_interventions_and_keys_may_differ():
    from dibs_amd.inference import JointDiBS
    data, gm, lm = make_data(5, seed=4, joint=True)
    mask = np.zeros(np.asarray(data.x).shape, np.int32)
    mask[:3, 1] = 1
    b = JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, interv_mask=mask, alpha_linear=0.2)
    with pytest.raises(AssertionError, match="created an engine"):
        _sweep([_joint(), b])


def test_sample_joint_batch_still_rejects_swept_models():
    from dibs_amd.inference import sample_joint_batch
    with pytest.raises(ValueError, match="sample_joint_batch: model 1 differs from model 0 in alpha_linear"):
        sample_joint_batch([_joint(), _joint(seed=4, alpha_linear=0.5)], keys=[0, 1], **ROOT_ARGS)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from dibs_amd import _lib
    from dibs_amd._abi import JOINT_SWEEPABLE, SWEEPABLE, ChainHparams, ProblemHparams
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dibs_hip.h")).read(), flags=re.S)
    for name in ("dibs_engine_set_chain_hparams", "dibs_engine_get_chain_hparams"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.EXPORTS
    body = re.search(r"typedef struct dibs_chain_hparams \{(.*?)\} dibs_chain_hparams;", src, flags=re.S).group(1)
    assert tuple(re.findall(r"double\s+([a-z_]+)\s*;", body)) == JOINT_SWEEPABLE
    assert sorted(JOINT_SWEEPABLE) == sorted(SWEEPABLE + ("h_theta",))
    assert [n for n, _ in ChainHparams._fields_] == list(JOINT_SWEEPABLE) and ctypes.sizeof(ChainHparams) == 64
    assert ctypes.sizeof(ProblemHparams) == 56 and len(SWEEPABLE) == 7      # (the per-problem struct is what it was)


def test_chain_hparams_is_eight_doubles_in_the_headers_order(tmp_path):
    """A two-line C program against the header prints the size and the offset of every field; ChainHparams must agree."""
    from dibs_amd._abi import JOINT_SWEEPABLE, ChainHparams
    cc = "gcc"   # (as tests/test_abi.py does for dibs_config)
    offs = ", ".join(f"offsetof(dibs_chain_hparams, {n})" for n in JOINT_SWEEPABLE)
    fmt = " ".join(["%zu"] * (1 + len(JOINT_SWEEPABLE)))
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dibs_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", sizeof(dibs_chain_hparams), {offs}); return 0; }}\n')
    exe = tmp_path / "t"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(ChainHparams) == 64
    assert got[1:] == [getattr(ChainHparams, n).offset for n in JOINT_SWEEPABLE] == [8 * i for i in range(8)]


def test_a_null_engine_is_refused_by_both_calls_without_touching_a_device():
    from dibs_amd import _lib
    from dibs_amd._abi import ChainHparams
    _lib.build()
    lib = _lib.load()
    assert lib.dibs_engine_set_chain_hparams.argtypes[2] == ctypes.POINTER(ChainHparams)
    assert lib.dibs_engine_get_chain_hparams.argtypes[2] == ctypes.POINTER(ChainHparams)
    h = ChainHparams()
    for f in (lib.dibs_engine_set_chain_hparams, lib.dibs_engine_get_chain_hparams):
        assert f(None, 0, ctypes.byref(h)) != 0
        msg = lib.dibs_last_error()
        assert msg.startswith(b"chains engine (n_chains > 1): dibs_engine_") and b"null" in msg
