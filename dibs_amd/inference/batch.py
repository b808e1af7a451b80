"""``sample_batch``: many independent MarginalDiBS + BGe inference problems in ONE batched engine (include/dibs_hip.h, n_problems).

What a user of the reference gets by vmapping the SVGD loop over keys and data: entry i of the result equals
``models[i].sample(key=keys[i], ...)`` bit for bit, but every device launch of a step covers all problems, so B small problems cost
about as much as one (the step of a small problem is launch latency, not work).  The problems share every size and hyper-parameter;
each has its own data, intervention mask and key.  The same model object may appear several times (several seeds on one data set)."""
import numpy as np

from .. import random
from ..engine import Engine
from .svgd import MarginalDiBS

# fields of dibs_config that belong to a problem's data, not to what the batch shares
_PER_PROBLEM = ("n_observations", "has_interventions", "reserved_i")


def _shared_fields(cfg):
    out = {}
    for name, _ in cfg._fields_:
        if name in _PER_PROBLEM:
            continue
        v = getattr(cfg, name)
        out[name] = tuple(v) if hasattr(v, "__len__") else v
    if out["latent_prior_std"] <= 0:  # (unset: the default sample() fills in, 1 / sqrt(k) in float32 -- the engine's own default)
        out["latent_prior_std"] = float(np.float32(1.0) / np.sqrt(np.float32(cfg.n_dim)))
    return out


def _edgewise(m):
    return getattr(getattr(m, "graph_model", None), "_dibs_prior", None) == "edgewise"


def _refuse_edgewise(models, who, engine):
    """The engines whose tail kernel reads a per-problem table have no edge-wise form (include/dibs_hip.h, EDGE-WISE GRAPH PRIOR)."""
    for i, m in enumerate(models):
        if _edgewise(m):
            raise ValueError(f"{who}: model {i} has an edge-wise graph prior (EdgePriorDAGDistribution), which {engine} does not "
                             "support: per-problem tables are not built (use sample() per problem; JointDiBS models with one shared "
                             "table: sample_chains / sample_joint_batch)")


def _batchable(models, keys, who):
    """What sample_batch and sample_sweep (`who`) ask of their arguments alike: as many keys as models, every model a float32 MarginalDiBS
    with the score-function estimator.  Returns (models, keys) as lists."""
    models = list(models)
    keys = [random.as_key(k) for k in keys]
    if not models:
        return models, keys
    if len(keys) != len(models):
        raise ValueError(f"{who}: {len(models)} models but {len(keys)} keys")
    for m in models:
        if not isinstance(m, MarginalDiBS):
            raise ValueError(f"{who}: every model must be a MarginalDiBS (joint models are not batched)")
        if m.grad_estimator_z != "score":
            raise ValueError(f"{who}: only the score-function estimator is batched (grad_estimator_z='score')")
        if getattr(m, "precision", "float32") != "float32":
            raise ValueError(f"{who}: float64 models are not batched (the float64 engine runs one problem; use sample())")
    _refuse_edgewise(models, who, "the batched engine")
    return models, keys


def sample_batch(models, *, keys, n_particles, steps, n_dim_particles=None, callback=None, callback_every=None):
    """Run ``models[i].sample(key=keys[i], n_particles=..., steps=..., ...)`` for every i in one batched engine; returns the list of the
    results (hard graphs ``[n_particles, d, d]`` per problem).  Chunking, step overshoot and the callback protocol are those of
    ``sample()``: after every chunk ``callback(dibs=models[i], t=..., zs=z_i)`` is called for each i in order.  Raises ``ValueError``
    before any device work if the models are not all MarginalDiBS with the score-function estimator, or disagree on anything the batch
    shares (sizes, graph prior, hyper-parameters, BGe parameters, estimator, optimizer, kernel)."""
    models, keys = _batchable(models, keys, "sample_batch")
    if not models:
        return []
    n_dim = n_dim_particles or models[0].n_vars
    cfgs = [m._make_config(n_particles, n_dim) for m in models]
    ref = _shared_fields(cfgs[0])
    for i, c in enumerate(cfgs[1:], 1):
        got = _shared_fields(c)
        diff = [k for k in ref if ref[k] != got[k]]
        if diff:
            raise ValueError(f"sample_batch: model {i} differs from model 0 in {', '.join(diff)} (a batch shares every size and "
                             "hyper-parameter; only data, interventions and keys differ)")
    B = len(models)
    if B == 1:  # (a batch of one is the standalone engine)
        return [models[0].sample(key=keys[0], n_particles=n_particles, steps=steps, n_dim_particles=n_dim_particles,
                                 callback=callback, callback_every=callback_every)]
    return _run_batched(models, keys, cfgs[0], n_particles, n_dim, steps, callback, callback_every)


def _run_batched(models, keys, cfg, n_particles, n_dim, steps, callback, callback_every, hparams=None):
    """The B problems in one batched engine created from ``cfg``; ``hparams``: per problem a ProblemHparams (sample_sweep), or None for
    the configuration's values.  Sets every model's ``last_state`` and returns the list of hard graphs."""
    B = len(models)
    cfg.reserved_i[0] = B
    eng = Engine(cfg)
    try:
        for i, m in enumerate(models):
            eng.set_data_problem(i, m.x, m.interv_mask if m.interv_mask.any() else None, getattr(m.likelihood_model, "mean_obs", None))
            if hparams is not None:
                eng.set_problem_hparams(i, hparams[i])
        eng.init_particles_batch(np.stack([np.asarray(k, np.uint32).reshape(2) for k in keys]))
        for m in models:
            if m.latent_prior_std is None:
                m.latent_prior_std = float(np.float32(1.0) / np.sqrt(np.float32(n_dim)))
        callback_every = callback_every or steps
        for t in (range(0, steps, callback_every) if steps else range(0)):
            eng.run(t, callback_every)
            if callback:
                z = eng.get_state()["z"].reshape(B, n_particles, models[0].n_vars, n_dim, 2)
                for i, m in enumerate(models):
                    callback(dibs=m, t=t + callback_every, zs=z[i])
        st = eng.get_state()
    finally:
        eng.close()
    shape = (B, n_particles, models[0].n_vars, n_dim, 2)
    z, v_z, base = st["z"].reshape(shape), st["v_z"].reshape(shape), st["baseline"].reshape(B, n_particles)
    out = []
    for i, m in enumerate(models):
        m.last_state = dict(z=z[i].copy(), v_z=v_z[i].copy(), theta=None, v_theta=None, key=st["key"][i].copy(),
                            baseline=base[i].copy())
        out.append(m.particle_to_g_lim(m.last_state["z"]))
    return out
