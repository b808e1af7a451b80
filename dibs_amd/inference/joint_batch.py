"""``sample_joint_batch``: many JointDiBS + LinearGaussian inference problems, each on a data set of its own, in ONE chains engine
(include/dibs_hip.h, CHAINS ENGINE with per-chain data).

The evaluation loop of a DiBS study -- ``JointDiBS.sample()`` on 20-30 random ground-truth graphs and data sets of one size -- as one
call: entry i of the result equals ``models[i].sample(key=keys[i], ...)`` bit for bit, but every device launch of a step covers all
problems.  The problems share every size (the number of observations included) and hyper-parameter; each has its own data, intervention
mask and key.  DenseNonlinearGaussian models are not covered: their chains share one data set (``sample_chains``)."""
from . import _multirun
from ..engine import Engine
from .svgd import JointDiBS


def _validate(models, keys, who="sample_joint_batch"):
    def not_joint(i, m):
        return (f"every model must be a JointDiBS, model {i} is a {type(m).__name__} "
                f"(MarginalDiBS models: {'sample_sweep' if who == 'sample_joint_sweep' else 'sample_batch'})")

    def rule(i, m):
        if m.likelihood_model._dibs_likelihood != "lingauss":
            raise ValueError(f"{who}: model {i} has a {type(m.likelihood_model).__name__} likelihood; only LinearGaussian "
                             "problems are batched on data sets of their own (DenseNonlinearGaussian: sample_chains for several seeds on "
                             "one data set, or sample() per problem)")
    return _multirun.check_runs(models, keys, who, JointDiBS, not_joint, rule, "not supported")


def _sample(models, keys, cfg, hparams=None, **kw):
    """The problems in one chains engine created from ``cfg`` (one problem: the standalone engine); ``hparams``: per problem a ChainHparams
    (sample_joint_sweep), or None for the configuration's values.  Sets every model's ``last_state`` and returns the list of
    ``(g, theta)``."""
    # (one table of an edge-wise graph prior: sample_joint_batch has compared the models')
    edge_probs = models[0].graph_model.edge_probs if _multirun._edgewise(models[0]) else None
    out, states = _multirun.sample_runs(Engine, cfg, "chains", models, keys, data="per_run", edge_probs=edge_probs, hparams=hparams, **kw)
    for m, st in zip(models, states or ()):
        m.last_state = st
    return out


def sample_joint_batch(models, *, keys, n_particles, steps, n_dim_particles=None, callback=None, callback_every=None):
    """Run ``models[i].sample(key=keys[i], n_particles=..., steps=..., ...)`` for every i in one engine; returns the list of the results
    ``(g, theta)``.  Chunking, step overshoot and the callback protocol are those of ``sample_chains``: after every chunk
    ``callback(dibs=models[i], t=..., zs=..., thetas=...)`` is called for each i in order.  Every model's ``last_state`` is set as
    ``sample()`` sets it.  Raises ``ValueError`` before any device work if a model is not a float32 JointDiBS with a LinearGaussian
    likelihood, if the keys do not match the models, or if the models disagree on anything the batch shares (every size, the number of
    observations, graph prior, hyper-parameters, estimator, optimizer, kernel)."""
    models, keys = _validate(models, keys)
    if not models:
        return []
    cfgs = [m._make_config(n_particles, n_dim_particles or models[0].n_vars) for m in models]
    _multirun.check_shared(cfgs, (), "sample_joint_batch", "a batch shares every size, the number of observations and every "
                           "hyper-parameter; only data, interventions and keys differ", extra=_multirun.joint_extra(models, cfgs))
    return _sample(models, keys, cfgs[0], n_particles=n_particles, steps=steps, n_dim_particles=n_dim_particles, callback=callback,
                   callback_every=callback_every)
