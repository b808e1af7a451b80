"""``sample_chains``: many seeds (random restarts) of ONE model on ONE data set in one engine.

For a ``JointDiBS`` model this is the chains engine (include/dibs_hip.h, n_chains): chain c of the result equals
``model.sample(key=keys[c], ...)`` bit for bit, but every device launch of a step covers all chains -- the data and every hyper-parameter
are shared, only the keys differ.  A ``MarginalDiBS`` model goes to ``sample_batch([model] * C, keys=...)``, the batched engine."""
import numpy as np

from . import _multirun
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
    if isinstance(model, MarginalDiBS) and len(keys) > 1:
        return _marginal_chains(model, keys, kw)
    cfg = model._make_config(n_particles, n_dim_particles or model.n_vars)
    # (one table of an edge-wise graph prior: the chains share it, as they share the data)
    edge_probs = model.graph_model.edge_probs if _multirun._edgewise(model) else None
    out, states = _multirun.sample_runs(Engine, cfg, "chains", [model] * len(keys), keys, data="shared", edge_probs=edge_probs, **kw)
    model.last_chain_states = states or [model.last_state]   # (one chain: sample() has left its state there)
    return out


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
