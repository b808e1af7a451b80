"""``sample_chains``: many seeds (random restarts) of ONE model on ONE data set in one engine.

For a ``JointDiBS`` model this is the chains engine (include/dibs_hip.h, n_chains): chain c of the result equals
``model.sample(key=keys[c], ...)`` bit for bit, but every device launch of a step covers all chains -- the data and every hyper-parameter
are shared, only the keys differ.  A ``MarginalDiBS`` model goes to ``sample_batch([model] * C, keys=...)``, the batched engine."""
import numpy as np

from .. import random
from ..engine import Engine
from .svgd import JointDiBS, MarginalDiBS


def _chain_keys(keys):
    try:
        keys = list(keys)
    except TypeError:
        raise ValueError("sample_chains: keys must be a sequence of PRNG keys (or integer seeds), one per chain") from None
    if not keys:
        raise ValueError("sample_chains: keys is empty (one key per chain)")
    out = []
    for c, k in enumerate(keys):
        if isinstance(k, (int, np.integer)) and not isinstance(k, bool):
            out.append(random.as_key(k))
            continue
        a = np.asarray(k)
        if a.shape != (2,) or a.dtype.kind not in "ui":
            raise ValueError(f"sample_chains: key {c} is not a PRNG key (uint32 [2]) or an integer seed: shape {a.shape}, dtype {a.dtype}")
        out.append(random.as_key(a))
    return out


def sample_chains(model, *, keys, n_particles, steps, n_dim_particles=None, callback=None, callback_every=None):
    """Run ``model.sample(key=keys[c], n_particles=..., steps=..., ...)`` for every chain c in one engine; returns the list of the results
    (``(g, theta)`` per chain for a JointDiBS, ``g`` for a MarginalDiBS).  Chunking, step overshoot and the callback protocol are those of
    ``sample()``: after every chunk the callback is called once per chain, in order, with ``dibs=model, t=..., zs=...`` and, for joint
    models, ``thetas=...``.  The per-chain final states go to ``model.last_chain_states`` (a list of dicts with the keys of
    ``last_state``, which is not touched).  Raises ``ValueError`` before any device work for a float64 model, an object that is no DiBS
    model, and an empty or ill-shaped key list."""
    if not isinstance(model, (JointDiBS, MarginalDiBS)):
        raise ValueError(f"sample_chains: model must be a JointDiBS or a MarginalDiBS, got {type(model).__name__}")
    if getattr(model, "precision", "float32") != "float32":
        raise ValueError("sample_chains: float64 models are not supported (the float64 engine runs one chain; use sample())")
    keys = _chain_keys(keys)
    kw = dict(n_particles=n_particles, steps=steps, n_dim_particles=n_dim_particles, callback=callback, callback_every=callback_every)
    if len(keys) == 1:  # (one chain is the standalone engine)
        out = [model.sample(key=keys[0], **kw)]
        model.last_chain_states = [model.last_state]
        return out
    if isinstance(model, MarginalDiBS):
        return _marginal_chains(model, keys, kw)
    return _run_chains(model, keys, n_particles, n_dim_particles or model.n_vars, steps, callback, callback_every)


def _marginal_chains(model, keys, kw):
    """``sample_batch([model] * C, keys=...)``, the batched engine, with the per-chain final states kept: sample_batch leaves a problem's
    state in its model's ``last_state``, so each chain gets a shallow copy of the model to carry it (the copies share the data and every
    setting; callbacks see ``model``, whose own ``last_state`` is not touched)."""
    import copy
    from .batch import sample_batch
    clones = [copy.copy(model) for _ in keys]
    cb = kw["callback"]
    if cb is not None:
        kw = dict(kw, callback=lambda dibs, **k: cb(dibs=model, **k))
    out = sample_batch(clones, keys=keys, **kw)
    model.last_chain_states = [c.last_state for c in clones]
    if model.latent_prior_std is None:
        model.latent_prior_std = clones[0].latent_prior_std
    return out


def _run_chains(model, keys, n_particles, n_dim, steps, callback, callback_every):
    C, d = len(keys), model.n_vars
    cfg = model._make_config(n_particles, n_dim)
    cfg.reserved_i[2] = C
    eng = Engine(cfg)
    try:
        eng.set_data(model.x, model.interv_mask if model.interv_mask.any() else None, None)
        if model.graph_model._dibs_prior == "edgewise":   # (one table: the chains share it)
            eng.set_edge_prior(model.graph_model.edge_probs)
        eng.init_particles_batch(np.stack([np.asarray(k, np.uint32).reshape(2) for k in keys]))
        if model.latent_prior_std is None:
            model.latent_prior_std = float(np.float32(1.0) / np.sqrt(np.float32(n_dim)))
        callback_every = callback_every or steps
        for t in (range(0, steps, callback_every) if steps else range(0)):
            eng.run(t, callback_every)
            if callback:
                st = eng.get_state()
                z, th = st["z"].reshape(C, n_particles, d, n_dim, 2), st["theta"].reshape(C, n_particles, -1)
                for c in range(C):
                    callback(dibs=model, t=t + callback_every, zs=z[c], thetas=model._theta_out(th[c]))
        st = eng.get_state()
    finally:
        eng.close()
    zshape = (C, n_particles, d, n_dim, 2)
    z, v_z = st["z"].reshape(zshape), st["v_z"].reshape(zshape)
    th, v_th = st["theta"].reshape(C, n_particles, -1), st["v_theta"].reshape(C, n_particles, -1)
    base = st["baseline"].reshape(C, n_particles)
    states, out = [], []
    for c in range(C):
        s = dict(z=z[c].copy(), v_z=v_z[c].copy(), theta=th[c].copy(), v_theta=v_th[c].copy(), key=st["key"][c].copy(), baseline=base[c].copy())
        states.append(s)
        out.append((model.particle_to_g_lim(s["z"]), model._theta_out(s["theta"])))
    model.last_chain_states = states
    return out
