"""``sample_joint_batch``: many JointDiBS + LinearGaussian inference problems, each on a data set of its own, in ONE chains engine
(include/dibs_hip.h, CHAINS ENGINE with per-chain data).

The evaluation loop of a DiBS study -- ``JointDiBS.sample()`` on 20-30 random ground-truth graphs and data sets of one size -- as one
call: entry i of the result equals ``models[i].sample(key=keys[i], ...)`` bit for bit, but every device launch of a step covers all
problems.  The problems share every size (the number of observations included) and hyper-parameter; each has its own data, intervention
mask and key.  DenseNonlinearGaussian models are not covered: their chains share one data set (``sample_chains``)."""
import numpy as np

from .. import random
from ..engine import Engine
from .batch import _edgewise, _shared_fields
from .svgd import JointDiBS


def _validate(models, keys, who="sample_joint_batch"):
    models = list(models)
    keys = [random.as_key(k) for k in keys]
    if not models:
        return models, keys
    if len(keys) != len(models):
        raise ValueError(f"{who}: {len(models)} models but {len(keys)} keys")
    for i, m in enumerate(models):
        if not isinstance(m, JointDiBS):
            raise ValueError(f"{who}: every model must be a JointDiBS, model {i} is a {type(m).__name__} "
                             f"(MarginalDiBS models: {'sample_sweep' if who == 'sample_joint_sweep' else 'sample_batch'})")
        if m.likelihood_model._dibs_likelihood != "lingauss":
            raise ValueError(f"{who}: model {i} has a {type(m.likelihood_model).__name__} likelihood; only LinearGaussian "
                             "problems are batched on data sets of their own (DenseNonlinearGaussian: sample_chains for several seeds on "
                             "one data set, or sample() per problem)")
        if getattr(m, "precision", "float32") != "float32":
            raise ValueError(f"{who}: float64 models are not supported (the float64 engine runs one problem; use sample())")
    return models, keys


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
    n_dim = n_dim_particles or models[0].n_vars
    cfgs = [m._make_config(n_particles, n_dim) for m in models]
    ref = _shared_fields(cfgs[0])
    for i, c in enumerate(cfgs[1:], 1):
        got = _shared_fields(c)
        diff = [k for k in ref if ref[k] != got[k]]
        if c.n_observations != cfgs[0].n_observations:
            diff.append("n_observations")
        if _edgewise(models[0]) and _edgewise(models[i]) and not np.array_equal(models[0].graph_model.log_odds, models[i].graph_model.log_odds):
            diff.append("edge_probs")   # (the table of an edge-wise graph prior: one per engine)
        if diff:
            raise ValueError(f"sample_joint_batch: model {i} differs from model 0 in {', '.join(diff)} (a batch shares every size, the "
                             "number of observations and every hyper-parameter; only data, interventions and keys differ)")
    if len(models) == 1:  # (a batch of one is the standalone engine)
        return [models[0].sample(key=keys[0], n_particles=n_particles, steps=steps, n_dim_particles=n_dim_particles,
                                 callback=callback, callback_every=callback_every)]
    return _run(models, keys, cfgs[0], n_particles, n_dim, steps, callback, callback_every)


def _run(models, keys, cfg, n_particles, n_dim, steps, callback, callback_every, hparams=None):
    """The B problems in one chains engine created from ``cfg``; ``hparams``: per problem a ChainHparams (sample_joint_sweep), or None
    for the configuration's values.  Sets every model's ``last_state`` and returns the list of ``(g, theta)``."""
    B, d = len(models), models[0].n_vars
    cfg.reserved_i[2] = B
    eng = Engine(cfg)
    try:
        if _edgewise(models[0]):   # (one table: sample_joint_batch has compared the models')
            eng.set_edge_prior(models[0].graph_model.edge_probs)
        for i, m in enumerate(models):
            eng.set_data_problem(i, m.x, m.interv_mask if m.interv_mask.any() else None, None)
            if hparams is not None:
                eng.set_chain_hparams(i, hparams[i])
        eng.init_particles_batch(np.stack([np.asarray(k, np.uint32).reshape(2) for k in keys]))
        for m in models:
            if m.latent_prior_std is None:
                m.latent_prior_std = float(np.float32(1.0) / np.sqrt(np.float32(n_dim)))
        callback_every = callback_every or steps
        for t in (range(0, steps, callback_every) if steps else range(0)):
            eng.run(t, callback_every)
            if callback:
                st = eng.get_state()
                z, th = st["z"].reshape(B, n_particles, d, n_dim, 2), st["theta"].reshape(B, n_particles, -1)
                for i, m in enumerate(models):
                    callback(dibs=m, t=t + callback_every, zs=z[i], thetas=m._theta_out(th[i]))
        st = eng.get_state()
    finally:
        eng.close()
    zshape = (B, n_particles, d, n_dim, 2)
    z, v_z = st["z"].reshape(zshape), st["v_z"].reshape(zshape)
    th, v_th = st["theta"].reshape(B, n_particles, -1), st["v_theta"].reshape(B, n_particles, -1)
    base = st["baseline"].reshape(B, n_particles)
    out = []
    for i, m in enumerate(models):
        m.last_state = dict(z=z[i].copy(), v_z=v_z[i].copy(), theta=th[i].copy(), v_theta=v_th[i].copy(), key=st["key"][i].copy(),
                            baseline=base[i].copy())
        out.append((m.particle_to_g_lim(m.last_state["z"]), m._theta_out(m.last_state["theta"])))
    return out
