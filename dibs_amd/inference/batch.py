"""``sample_batch``: many independent MarginalDiBS + BGe inference problems in ONE batched engine (include/dibs_hip.h, n_problems).

What a user of the reference gets by vmapping the SVGD loop over keys and data: entry i of the result equals
``models[i].sample(key=keys[i], ...)`` bit for bit, but every device launch of a step covers all problems, so B small problems cost
about as much as one (the step of a small problem is launch latency, not work).  The problems share every size and hyper-parameter;
each has its own data, intervention mask and key.  The same model object may appear several times (several seeds on one data set)."""
from . import _multirun
from ..engine import Engine
from .svgd import MarginalDiBS


def _batchable(models, keys, who):
    """What sample_batch and sample_sweep (`who`) ask of their arguments alike: as many keys as models, every model a float32 MarginalDiBS
    with the score-function estimator and no edge-wise graph prior.  Returns (models, keys) as lists."""
    def rule(i, m):
        if m.grad_estimator_z != "score":
            raise ValueError(f"{who}: only the score-function estimator is batched (grad_estimator_z='score')")
        if getattr(m.likelihood_model, "_dibs_likelihood", None) == "bdeu":
            raise ValueError(f"{who}: model {i} has a BDeu likelihood (discrete data), which the batched engine does not support: it runs "
                             "BGe only (use sample() per problem)")
    not_marginal = lambda i, m: "every model must be a MarginalDiBS (joint models are not batched)"
    models, keys = _multirun.check_runs(models, keys, who, MarginalDiBS, not_marginal, rule, "not batched")
    _multirun._refuse_edgewise(models, who, "the batched engine")
    return models, keys


def _sample(models, keys, cfg, hparams=None, **kw):
    """The problems in one batched engine created from ``cfg`` (one problem: the standalone engine); ``hparams``: per problem a
    ProblemHparams (sample_sweep), or None for the configuration's values.  Sets every model's ``last_state`` and returns the list of hard
    graphs."""
    out, states = _multirun.sample_runs(Engine, cfg, "problems", models, keys, data="per_run_mean_obs", hparams=hparams, **kw)
    for m, st in zip(models, states or ()):
        m.last_state = st
    return out


def sample_batch(models, *, keys, n_particles, steps, n_dim_particles=None, callback=None, callback_every=None):
    """Run ``models[i].sample(key=keys[i], n_particles=..., steps=..., ...)`` for every i in one batched engine; returns the list of the
    results (hard graphs ``[n_particles, d, d]`` per problem).  Chunking, step overshoot and the callback protocol are those of
    ``sample()``: after every chunk ``callback(dibs=models[i], t=..., zs=z_i)`` is called for each i in order.  Raises ``ValueError``
    before any device work if the models are not all MarginalDiBS with the score-function estimator, or disagree on anything the batch
    shares (sizes, graph prior, hyper-parameters, BGe parameters, estimator, optimizer, kernel)."""
    models, keys = _batchable(models, keys, "sample_batch")
    if not models:
        return []
    cfgs = [m._make_config(n_particles, n_dim_particles or models[0].n_vars) for m in models]
    _multirun.check_shared(cfgs, (), "sample_batch", "a batch shares every size and hyper-parameter; only data, interventions and keys differ")
    return _sample(models, keys, cfgs[0], n_particles=n_particles, steps=steps, n_dim_particles=n_dim_particles, callback=callback,
                   callback_every=callback_every)
