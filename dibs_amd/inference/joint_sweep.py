"""``sample_joint_sweep``: a hyper-parameter grid of JointDiBS + LinearGaussian runs in ONE chains engine (include/dibs_hip.h,
dibs_engine_set_chain_hparams).

``sample_joint_batch`` shares every hyper-parameter between its problems; here each problem has its own ``alpha_linear``,
``beta_linear``, the two kernel bandwidths ``h_latent`` and ``h_theta``, optimizer step size, ``score_function_baseline``,
``latent_prior_std`` and ``n_edges_per_node`` of the graph prior -- the scalars a kernel takes as a launch argument, which select no
size, code path or buffer.  Everything else is shared as in ``sample_joint_batch`` (the number of observations included).  Entry i of
the result equals ``models[i].sample(key=keys[i], ...)`` bit for bit.  A grid over one data set uploads it once per grid point."""
from . import _multirun
from .._abi import JOINT_SWEEPABLE, chain_hparams
from .joint_batch import _sample, _validate
from .svgd import MarginalDiBS


def _plan(models, keys, n_particles, n_dim_particles):
    """The validation of sample_joint_sweep, without any device work: (keys, n_dim, the engine's dibs_config, per model a ChainHparams)."""
    models = list(models)
    for i, m in enumerate(models):
        if isinstance(m, MarginalDiBS):
            raise ValueError(f"sample_joint_sweep: model {i} is a MarginalDiBS; a grid of marginal models is sample_sweep")
    models, keys = _validate(models, keys, "sample_joint_sweep")
    _multirun._refuse_edgewise(models, "sample_joint_sweep", "the per-chain hyper-parameter tier of the chains engine")
    if not models:
        return keys, None, None, []
    n_dim = n_dim_particles or models[0].n_vars
    cfgs = [m._make_config(n_particles, n_dim) for m in models]
    _multirun.check_shared(cfgs, JOINT_SWEEPABLE, "sample_joint_sweep", "a sweep shares every size, the number of observations, the prior, "
                           "estimator and optimizer kind, tau, the kernel scales and the likelihood's parameters; per model: "
                           f"{', '.join(JOINT_SWEEPABLE)}", extra=_multirun.joint_extra(models, cfgs))
    return keys, n_dim, cfgs[0], [chain_hparams(c) for c in cfgs]


def sample_joint_sweep(models, *, keys, n_particles, steps, n_dim_particles=None, callback=None, callback_every=None):
    """Run ``models[i].sample(key=keys[i], n_particles=..., steps=..., ...)`` for every i in one chains engine; returns the list of the
    results ``(g, theta)``.  The models may differ in data, interventions, key and in the per-chain settings
    (``dibs_amd._abi.JOINT_SWEEPABLE``); anything else that differs raises ``ValueError`` naming the fields before any device work, and so
    do MarginalDiBS models (``sample_sweep``), DenseNonlinearGaussian likelihoods (``sample_chains`` / ``sample()``), float64 models and
    swept settings beyond 64 variables or latent dimensions.  Chunking, step overshoot, the callback protocol and ``last_state`` are
    those of ``sample_joint_batch``.  The usual call is a grid: one model object per grid point on the same data."""
    models = list(models)
    keys, _, cfg, hparams = _plan(models, keys, n_particles, n_dim_particles)
    if not models:
        return []
    return _sample(models, keys, cfg, hparams=hparams, n_particles=n_particles, steps=steps, n_dim_particles=n_dim_particles,
                   callback=callback, callback_every=callback_every)
