"""``sample_sweep``: a hyper-parameter grid of MarginalDiBS + BGe runs in ONE batched engine (include/dibs_hip.h,
dibs_engine_set_problem_hparams).

``sample_batch`` shares every hyper-parameter between its problems; here each problem has its own ``alpha_linear``, ``beta_linear``,
kernel bandwidth ``h``, optimizer step size, ``score_function_baseline``, ``latent_prior_std`` and ``n_edges_per_node`` of the graph
prior -- the scalars a kernel takes as a launch argument, which select no size, code path or buffer.  Everything else is shared as in
``sample_batch``.  Entry i of the result equals ``models[i].sample(key=keys[i], ...)`` bit for bit."""
from . import _multirun
from .._abi import SWEEPABLE, problem_hparams
from .batch import _batchable, _sample


def _plan(models, keys, n_particles, n_dim_particles):
    """The validation of sample_sweep, without any device work: (keys, n_dim, the engine's dibs_config, per problem a ProblemHparams)."""
    models, keys = _batchable(models, keys, "sample_sweep")
    if not models:
        return keys, None, None, []
    n_dim = n_dim_particles or models[0].n_vars
    cfgs = [m._make_config(n_particles, n_dim) for m in models]
    _multirun.check_shared(cfgs, SWEEPABLE, "sample_sweep", "a sweep shares every size, the prior and optimizer kind, tau and the BGe "
                           f"parameters; per problem: {', '.join(SWEEPABLE)}")
    return keys, n_dim, cfgs[0], [problem_hparams(c) for c in cfgs]


def sample_sweep(models, *, keys, n_particles, steps, n_dim_particles=None, callback=None, callback_every=None):
    """Run ``models[i].sample(key=keys[i], n_particles=..., steps=..., ...)`` for every i in one batched engine; returns the list of the
    results.  The models may differ in data, interventions, key and in the per-problem settings (``dibs_amd._abi.SWEEPABLE``); anything
    else that differs raises ``ValueError`` naming the field before any device work.  Chunking, step overshoot, the callback protocol and
    ``last_state`` are those of ``sample_batch``.  The usual call is a grid: one model object per grid point on the same data, times a
    few keys."""
    models = list(models)
    keys, _, cfg, hparams = _plan(models, keys, n_particles, n_dim_particles)
    if not models:
        return []
    return _sample(models, keys, cfg, hparams=hparams, n_particles=n_particles, steps=steps, n_dim_particles=n_dim_particles,
                   callback=callback, callback_every=callback_every)
