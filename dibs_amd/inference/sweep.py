"""``sample_sweep``: a hyper-parameter grid of MarginalDiBS + BGe runs in ONE batched engine (include/dibs_hip.h,
dibs_engine_set_problem_hparams).

``sample_batch`` shares every hyper-parameter between its problems; here each problem has its own ``alpha_linear``, ``beta_linear``,
kernel bandwidth ``h``, optimizer step size, ``score_function_baseline``, ``latent_prior_std`` and ``n_edges_per_node`` of the graph
prior -- the scalars a kernel takes as a launch argument, which select no size, code path or buffer.  Everything else is shared as in
``sample_batch``.  Entry i of the result equals ``models[i].sample(key=keys[i], ...)`` bit for bit."""
from .._abi import SWEEPABLE, problem_hparams
from .batch import _batchable, _run_batched, _shared_fields

# beyond these sizes the engine's kernels take the per-problem values as launch arguments of the whole batch (include/dibs_hip.h)
_MAX_VARS = 64


def _plan(models, keys, n_particles, n_dim_particles):
    """The validation of sample_sweep, without any device work: (keys, n_dim, the engine's dibs_config, per problem a ProblemHparams)."""
    models, keys = _batchable(models, keys, "sample_sweep")
    if not models:
        return keys, None, None, []
    n_dim = n_dim_particles or models[0].n_vars
    cfgs = [m._make_config(n_particles, n_dim) for m in models]
    fields = [_shared_fields(c) for c in cfgs]   # (latent_prior_std: the default filled in)
    for i, got in enumerate(fields[1:], 1):
        diff = [k for k in fields[0] if k not in SWEEPABLE and fields[0][k] != got[k]]
        if diff:
            raise ValueError(f"sample_sweep: model {i} differs from model 0 in {', '.join(diff)} (a sweep shares every size, the prior "
                             f"and optimizer kind, tau and the BGe parameters; per problem: {', '.join(SWEEPABLE)})")
    swept = [k for k in SWEEPABLE if any(f[k] != fields[0][k] for f in fields[1:])]
    if swept and (cfgs[0].n_vars > _MAX_VARS or cfgs[0].n_dim > _MAX_VARS):
        raise ValueError(f"sample_sweep: models differ in {', '.join(swept)}, which needs n_vars <= {_MAX_VARS} and "
                         f"n_dim_particles <= {_MAX_VARS} (got {cfgs[0].n_vars}, {cfgs[0].n_dim})")
    return keys, n_dim, cfgs[0], [problem_hparams(c) for c in cfgs]


def sample_sweep(models, *, keys, n_particles, steps, n_dim_particles=None, callback=None, callback_every=None):
    """Run ``models[i].sample(key=keys[i], n_particles=..., steps=..., ...)`` for every i in one batched engine; returns the list of the
    results.  The models may differ in data, interventions, key and in the per-problem settings (``dibs_amd._abi.SWEEPABLE``); anything
    else that differs raises ``ValueError`` naming the field before any device work.  Chunking, step overshoot, the callback protocol and
    ``last_state`` are those of ``sample_batch``.  The usual call is a grid: one model object per grid point on the same data, times a
    few keys."""
    models = list(models)
    keys, n_dim, cfg, hparams = _plan(models, keys, n_particles, n_dim_particles)
    if not models:
        return []
    if len(models) == 1:  # (a sweep of one is the standalone engine)
        return [models[0].sample(key=keys[0], n_particles=n_particles, steps=steps, n_dim_particles=n_dim_particles,
                                 callback=callback, callback_every=callback_every)]
    return _run_batched(models, keys, cfg, n_particles, n_dim, steps, callback, callback_every, hparams=hparams)
