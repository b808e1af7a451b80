"""Host-side checks of sample_sweep and of the per-problem hyper-parameters of the batched engine (include/dibs_hip.h,
dibs_engine_set_problem_hparams): what a sweep shares is checked before any device work, so these run without a GPU."""
import ctypes
import os
import re

import pytest

from conftest import make_data
from dibs_amd.kernel import AdditiveFrobeniusSEKernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(d=6, seed=0, **kw):
    from dibs_amd.inference import MarginalDiBS
    data, gm, lm = make_data(d, seed=seed)
    return MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, **kw)


def _sweep(models, keys=None, **kw):
    from dibs_amd.inference import sample_sweep
    return sample_sweep(models, keys=list(range(len(models))) if keys is None else keys, n_particles=4, steps=2, **kw)


def test_sample_sweep_is_exported():
    import dibs_amd.inference as inf
    from dibs_amd.inference.sweep import sample_sweep
    assert inf.sample_sweep is sample_sweep


@pytest.mark.parametrize("kw,field", [
    (dict(n_grad_mc_samples=64), "n_grad_mc_samples"),
    (dict(n_acyclicity_mc_samples=8), "n_acyclicity_mc_samples"),
    (dict(tau=0.5), "tau"),
    (dict(optimizer="gd"), "optimizer"),
    (dict(kernel=AdditiveFrobeniusSEKernel, kernel_param={"h": 5.0, "scale": 2.0}), "scale_latent"),
])
def test_sample_sweep_rejects_what_a_sweep_shares(kw, field):
    with pytest.raises(ValueError, match=f"differs from model 0 in .*{field}"):
        _sweep([_model(seed=0), _model(seed=1, **kw)])


def test_sample_sweep_rejects_other_sizes_priors_and_bge_parameters():
    from dibs_amd import random
    from dibs_amd.inference import MarginalDiBS
    from dibs_amd.target import make_linear_gaussian_equivalent_model
    a = _model(d=6)
    with pytest.raises(ValueError, match="n_vars"):
        _sweep([a, _model(d=7)])
    data, gm, lm = make_data(6, seed=1, prior="sf")
    with pytest.raises(ValueError, match="graph_prior"):
        _sweep([a, MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)])
    for extra, field in ((dict(bge_alpha_mu=2.0), "bge_alpha_mu"), (dict(bge_alpha_lambd=20.0), "bge_alpha_lambd")):
        data, gm, lm = make_linear_gaussian_equivalent_model(key=random.PRNGKey(3), n_vars=6, graph_prior_str="er", **extra)
        with pytest.raises(ValueError, match=field):
            _sweep([a, MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)])


def test_sample_sweep_rejects_estimator_joint_float64_and_key_count():
    from dibs_amd.inference import JointDiBS
    with pytest.raises(ValueError, match="score-function"):
        _sweep([_model(), _model(grad_estimator_z="reparam")])
    data, gm, lm = make_data(5, seed=3, joint=True)
    j = JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm)
    with pytest.raises(ValueError, match="MarginalDiBS"):
        _sweep([j, j])
    with pytest.raises(ValueError, match="float64"):
        _sweep([_model(), _model(seed=1, precision="float64")])
    with pytest.raises(ValueError, match="keys"):
        _sweep([_model(), _model(seed=1)], keys=[0])


SWEPT = [
    dict(alpha_linear=0.5),
    dict(beta_linear=2.0),
    dict(score_function_baseline=0.1),
    dict(optimizer_param={"stepsize": 0.01}),
    dict(kernel=AdditiveFrobeniusSEKernel, kernel_param={"h": 3.0}),
    dict(latent_prior_std=0.5),
]


@pytest.mark.parametrize("kw", SWEPT)
def test_models_that_differ_in_a_sweepable_setting_pass_the_validation(kw):
    from dibs_amd._abi import SWEEPABLE
    from dibs_amd.inference.sweep import _plan
    a, b = _model(seed=0), _model(seed=1, **kw)
    keys, n_dim, cfg, hps = _plan([a, b], [0, 1], 4, None)
    assert n_dim == 6 and cfg.n_vars == 6 and len(hps) == 2 and len(keys) == 2
    ha, hb = ({n: getattr(h, n) for n in SWEEPABLE} for h in hps)
    assert [n for n in SWEEPABLE if ha[n] != hb[n]] != []          # the difference arrives in the per-problem struct
    assert all(getattr(cfg, n) == ha[n] for n in SWEEPABLE)        # the engine's config carries model 0's values


def test_edges_per_node_is_per_problem():
    from dibs_amd.inference import MarginalDiBS
    from dibs_amd.inference.sweep import _plan
    data, gm, lm = make_data(6, seed=1, edges_per_node=1)
    _, _, cfg, hps = _plan([_model(d=6), MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)], [0, 1], 4, None)
    assert [h.graph_prior_edges_per_node for h in hps] == [2.0, 1.0]


def test_sweep_reaches_engine_creation_without_a_gpu():
    """the Python validation lets a sweep through; without a device the first failure is the engine's"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from dibs_amd import _lib
    _lib.build()
    with pytest.raises(_lib.DibsHipError):
        _sweep([_model(seed=0), _model(seed=1, alpha_linear=0.5, beta_linear=2.0)])


def test_differing_values_beyond_64_variables_are_rejected_on_the_host():
    from dibs_amd.inference.sweep import _plan
    a, b = _model(d=65), _model(d=65, seed=1, alpha_linear=0.5)
    with pytest.raises(ValueError, match="alpha_linear.*n_vars <= 64"):
        _plan([a, b], [0, 1], 4, None)
    _plan([a, _model(d=65, seed=1)], [0, 1], 4, None)   # (nothing swept: any size a batch accepts)


def test_new_symbols_are_declared_exported_and_bound():
    from dibs_amd import _lib
    from dibs_amd._abi import SWEEPABLE, ProblemHparams
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dibs_hip.h")).read(), flags=re.S)
    for name in ("dibs_engine_set_problem_hparams", "dibs_engine_get_problem_hparams"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.EXPORTS
    # the POD of seven doubles, in the header's order
    body = re.search(r"typedef struct dibs_problem_hparams \{(.*?)\} dibs_problem_hparams;", src, flags=re.S).group(1)
    assert tuple(re.findall(r"double\s+([a-z_]+)\s*;", body)) == SWEEPABLE
    assert ctypes.sizeof(ProblemHparams) == 8 * len(SWEEPABLE) == 56
    _lib.build()
    lib = _lib.load()
    assert lib.dibs_engine_set_problem_hparams.argtypes[2] == ctypes.POINTER(ProblemHparams)
    h = ProblemHparams()
    assert lib.dibs_engine_set_problem_hparams(None, 0, ctypes.byref(h)) != 0   # (null engine: refused, no device touched)
    assert b"null" in lib.dibs_last_error()


def test_sample_batch_still_rejects_swept_models():
    from dibs_amd.inference import sample_batch
    with pytest.raises(ValueError, match="differs from model 0"):
        sample_batch([_model(seed=0), _model(seed=1, alpha_linear=0.5)], keys=[0, 1], n_particles=4, steps=2)
