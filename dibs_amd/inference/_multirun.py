"""What the multi-run entry points share (``sample_batch``, ``sample_sweep``, ``sample_chains``, ``sample_joint_batch``,
``sample_joint_sweep``): the checks of their arguments, the comparison of what the runs must share, and the one loop that drives a batched
or a chains engine (include/dibs_hip.h, n_problems / n_chains).  Each entry point keeps its public function, the rules that are its own and
the wording of its errors."""
import numpy as np

from .. import random

# fields of dibs_config that belong to a run's data, not to what the runs share
_PER_RUN = ("n_observations", "has_interventions", "reserved_i")
# beyond these sizes the engines' kernels take the per-run hyper-parameters as launch arguments of all runs (include/dibs_hip.h)
MAX_SWEPT_VARS = 64
# where dibs_config carries the run count of each engine kind
_COUNT_SLOT = {"problems": 0, "chains": 2}


def chunks(steps, callback_every):
    """``(t, n)`` of every ``engine.run(t, n)`` of a sampling call: chunks of ``callback_every`` steps (all steps in one without it); the
    last chunk is a whole one, so the step count may overshoot as the reference's does."""
    n = callback_every or steps
    return [(t, n) for t in (range(0, steps, n) if steps else range(0))]


def default_latent_prior_std(n_dim):
    """1 / sqrt(k) in float32: what ``sample()`` fills in for an unset ``latent_prior_std`` -- the engine's own default."""
    return float(np.float32(1.0) / np.sqrt(np.float32(n_dim)))


def _shared_fields(cfg):
    out = {}
    for name, _ in cfg._fields_:
        if name in _PER_RUN:
            continue
        v = getattr(cfg, name)
        out[name] = tuple(v) if hasattr(v, "__len__") else v
    if out["latent_prior_std"] <= 0:  # (unset: the default filled in)
        out["latent_prior_std"] = default_latent_prior_std(cfg.n_dim)
    # reserved_i is per run but for its slot 3: which kernels take the median-rule bandwidth is one setting of the engine
    out["kernel bandwidth rule"] = int(cfg.reserved_i[3])
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


def check_runs(models, keys, who, cls, not_cls, rule, float64):
    """What every entry point that takes a list of models asks alike: as many keys as models, every model a float32 ``cls``.  The wording
    is the caller's: ``not_cls(i, m)`` says what is wrong with a model of another class, ``rule(i, m)`` raises for what else the entry
    point does not take, ``float64`` completes "float64 models are ...".  Returns (models, keys) as lists."""
    models = list(models)
    keys = [random.as_key(k) for k in keys]
    if models and len(keys) != len(models):
        raise ValueError(f"{who}: {len(models)} models but {len(keys)} keys")
    for i, m in enumerate(models):
        if not isinstance(m, cls):
            raise ValueError(f"{who}: {not_cls(i, m)}")
        rule(i, m)
        if getattr(m, "precision", "float32") != "float32":
            raise ValueError(f"{who}: float64 models are {float64} (the float64 engine runs one problem; use sample())")
    return models, keys


def joint_extra(models, cfgs):
    """What the runs of a chains engine with per-chain data share beyond the configuration's fields, for ``check_shared(extra=...)``."""
    def extra(i):
        diff = []
        if cfgs[i].n_observations != cfgs[0].n_observations:
            diff.append("n_observations")
        if _edgewise(models[0]) and _edgewise(models[i]) and not np.array_equal(models[0].graph_model.log_odds, models[i].graph_model.log_odds):
            diff.append("edge_probs")   # (the table of an edge-wise graph prior: one per engine)
        return diff
    return extra


def check_shared(cfgs, free, who, tail_text, extra=None):
    """Every model's configuration must equal model 0's in every shared field but those of ``free`` (latent_prior_std: the default filled
    in), and in what ``extra(i)`` names; ``tail_text`` says what is shared.  Fields of ``free`` that do differ need at most
    ``MAX_SWEPT_VARS`` variables and latent dimensions."""
    fields = [_shared_fields(c) for c in cfgs]
    for i, got in enumerate(fields[1:], 1):
        diff = [k for k in fields[0] if k not in free and fields[0][k] != got[k]]
        if extra is not None:
            diff += extra(i)
        if diff:
            raise ValueError(f"{who}: model {i} differs from model 0 in {', '.join(diff)} ({tail_text})")
    swept = [k for k in free if any(f[k] != fields[0][k] for f in fields[1:])]
    if swept and (cfgs[0].n_vars > MAX_SWEPT_VARS or cfgs[0].n_dim > MAX_SWEPT_VARS):
        raise ValueError(f"{who}: models differ in {', '.join(swept)}, which needs n_vars <= {MAX_SWEPT_VARS} and "
                         f"n_dim_particles <= {MAX_SWEPT_VARS} (got {cfgs[0].n_vars}, {cfgs[0].n_dim})")


def sample_runs(Engine, cfg, kind, models, keys, *, data, n_particles, steps, n_dim_particles=None, callback=None, callback_every=None,
                edge_probs=None, hparams=None):
    """``models[i].sample(key=keys[i], ...)`` for every i in one engine of ``kind`` ("problems": batched, "chains") created from ``cfg``.
    Returns (the results as ``sample()`` returns them, the final states with the keys of ``last_state``); what to do with the states is
    the caller's.  Exactly one run is the standalone engine: ``sample()`` itself, which leaves the state in the model's ``last_state``, and
    the states returned are None.  See ``_run`` for the other arguments."""
    kw = dict(n_particles=n_particles, steps=steps, n_dim_particles=n_dim_particles, callback=callback, callback_every=callback_every)
    if len(models) == 1:
        return [models[0].sample(key=keys[0], **kw)], None
    states = _run(Engine, cfg, kind, models, keys, data, edge_probs, hparams, **kw)
    out = []
    for m, s in zip(models, states):
        g = m.particle_to_g_lim(s["z"])
        out.append(g if s["theta"] is None else (g, m._theta_out(s["theta"])))
    return out, states


def _run(Engine, cfg, kind, models, keys, data, edge_probs, hparams, *, n_particles, steps, n_dim_particles, callback, callback_every):
    """``data``: "shared" (one ``set_data`` from model 0), "per_run" (``set_data_problem`` for every run) or "per_run_mean_obs" (the same
    with the BGe model's ``mean_obs``).  ``edge_probs``: the table of an edge-wise graph prior, shared by all runs.  ``hparams``: per run a
    ProblemHparams / ChainHparams, or None for the configuration's values.  Chunking, step overshoot and the callback protocol are those of
    ``sample()``: after every chunk ``callback(dibs=models[i], t=..., zs=...)`` for each i in order, with ``thetas=...`` for joint models."""
    B, d, n_dim = len(models), models[0].n_vars, n_dim_particles or models[0].n_vars
    joint = models[0]._joint

    def per_run(st):
        """the engine's state, rows [B * n_particles] run-major, as B states of one run each (views; no theta for marginal models)"""
        rows = lambda a, *shape: [None] * B if a is None else a.reshape(B, n_particles, *shape)
        z, v_z, th, v_th = rows(st["z"], d, n_dim, 2), rows(st["v_z"], d, n_dim, 2), rows(st["theta"], -1), rows(st["v_theta"], -1)
        base = rows(st["baseline"])
        return [dict(z=z[i], v_z=v_z[i], theta=th[i], v_theta=v_th[i], key=st["key"][i], baseline=base[i]) for i in range(B)]

    cfg.reserved_i[_COUNT_SLOT[kind]] = B
    eng = Engine(cfg)
    try:
        if edge_probs is not None:
            eng.set_edge_prior(edge_probs)
        mask = lambda m: m.interv_mask if m.interv_mask.any() else None
        if data == "shared":
            eng.set_data(models[0].x, mask(models[0]), None)
        for i, m in enumerate(models):
            if data != "shared":
                eng.set_data_problem(i, m.x, mask(m), getattr(m.likelihood_model, "mean_obs", None) if data == "per_run_mean_obs" else None)
            if hparams is not None:
                (eng.set_chain_hparams if kind == "chains" else eng.set_problem_hparams)(i, hparams[i])
        eng.init_particles_batch(np.stack([np.asarray(k, np.uint32).reshape(2) for k in keys]))
        for m in models:
            if m.latent_prior_std is None:
                m.latent_prior_std = default_latent_prior_std(n_dim)
        for t, n in chunks(steps, callback_every):
            eng.run(t, n)
            if callback:
                for m, s in zip(models, per_run(eng.get_state())):
                    callback(dibs=m, t=t + n, zs=s["z"], **(dict(thetas=m._theta_out(s["theta"])) if joint else {}))
        st = eng.get_state()
        for m, bw in zip(models, eng.read("BANDWIDTH").reshape(B, 2)):
            m.last_bandwidth = bw.copy()   # (as sample() leaves it; one model object in several runs keeps the last run's)
    finally:
        eng.close()
    return [{name: None if a is None else a.copy() for name, a in s.items()} for s in per_run(st)]
