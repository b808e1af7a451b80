"""``sample_joint_sweep``: a hyper-parameter grid of JointDiBS + LinearGaussian runs in ONE chains engine (include/dibs_hip.h,
dibs_engine_set_chain_hparams).

``sample_joint_batch`` shares every hyper-parameter between its problems; here each problem has its own ``alpha_linear``,
``beta_linear``, the two kernel bandwidths ``h_latent`` and ``h_theta``, optimizer step size, ``score_function_baseline``,
``latent_prior_std`` and ``n_edges_per_node`` of the graph prior -- the scalars a kernel takes as a launch argument, which select no
size, code path or buffer.  Everything else is shared as in ``sample_joint_batch`` (the number of observations included).  Entry i of
the result equals ``models[i].sample(key=keys[i], ...)`` bit for bit.  A grid over one data set uploads it once per grid point."""
from .._abi import JOINT_SWEEPABLE, chain_hparams
from .batch import _refuse_edgewise, _shared_fields
from .joint_batch import _run, _validate
from .svgd import MarginalDiBS

# beyond these sizes the engine's kernels take the per-chain values as launch arguments of all chains (include/dibs_hip.h)
_MAX_VARS = 64


def _plan(models, keys, n_particles, n_dim_particles):
    """The validation of sample_joint_sweep, without any device work: (keys, n_dim, the engine's dibs_config, per model a ChainHparams)."""
    models = list(models)
    for i, m in enumerate(models):
        if isinstance(m, MarginalDiBS):
            raise ValueError(f"sample_joint_sweep: model {i} is a MarginalDiBS; a grid of marginal models is sample_sweep")
    models, keys = _validate(models, keys, "sample_joint_sweep")
    _refuse_edgewise(models, "sample_joint_sweep", "the per-chain hyper-parameter tier of the chains engine")
    if not models:
        return keys, None, None, []
    n_dim = n_dim_particles or models[0].n_vars
    cfgs = [m._make_config(n_particles, n_dim) for m in models]
    fields = [_shared_fields(c) for c in cfgs]   # (latent_prior_std: the default filled in)
    for i, (c, got) in enumerate(zip(cfgs[1:], fields[1:]), 1):
        diff = [k for k in fields[0] if k not in JOINT_SWEEPABLE and fields[0][k] != got[k]]
        if c.n_observations != cfgs[0].n_observations:
            diff.append("n_observations")
        if diff:
            raise ValueError(f"sample_joint_sweep: model {i} differs from model 0 in {', '.join(diff)} (a sweep shares every size, the "
                             "number of observations, the prior, estimator and optimizer kind, tau, the kernel scales and the "
                             f"likelihood's parameters; per model: {', '.join(JOINT_SWEEPABLE)})")
    swept = [k for k in JOINT_SWEEPABLE if any(f[k] != fields[0][k] for f in fields[1:])]
    if swept and (cfgs[0].n_vars > _MAX_VARS or cfgs[0].n_dim > _MAX_VARS):
        raise ValueError(f"sample_joint_sweep: models differ in {', '.join(swept)}, which needs n_vars <= {_MAX_VARS} and "
                         f"n_dim_particles <= {_MAX_VARS} (got {cfgs[0].n_vars}, {cfgs[0].n_dim})")
    return keys, n_dim, cfgs[0], [chain_hparams(c) for c in cfgs]


def sample_joint_sweep(models, *, keys, n_particles, steps, n_dim_particles=None, callback=None, callback_every=None):
    """Run ``models[i].sample(key=keys[i], n_particles=..., steps=..., ...)`` for every i in one chains engine; returns the list of the
    results ``(g, theta)``.  The models may differ in data, interventions, key and in the per-chain settings
    (``dibs_amd._abi.JOINT_SWEEPABLE``); anything else that differs raises ``ValueError`` naming the fields before any device work, and so
    do MarginalDiBS models (``sample_sweep``), DenseNonlinearGaussian likelihoods (``sample_chains`` / ``sample()``), float64 models and
    swept settings beyond 64 variables or latent dimensions.  Chunking, step overshoot, the callback protocol and ``last_state`` are
    those of ``sample_joint_batch``.  The usual call is a grid: one model object per grid point on the same data."""
    models = list(models)
    keys, n_dim, cfg, hparams = _plan(models, keys, n_particles, n_dim_particles)
    if not models:
        return []
    if len(models) == 1:  # (a sweep of one is the standalone engine)
        return [models[0].sample(key=keys[0], n_particles=n_particles, steps=steps, n_dim_particles=n_dim_particles,
                                 callback=callback, callback_every=callback_every)]
    return _run(models, keys, cfg, n_particles, n_dim, steps, callback, callback_every, hparams=hparams)
