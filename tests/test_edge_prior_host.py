"""Host-side checks of the edge-wise graph prior (EdgePriorDAGDistribution, DIBS_PRIOR_EDGEWISE, dibs_engine_set_edge_prior): the model
class, the ABI mirror, and the ValueErrors of the five multi-run entry points, which are raised before an engine is created -- Engine is
replaced by a class that fails the test when it is constructed.  No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import make_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = dict(n_particles=4, steps=2)


def _table(d, seed=0, lo=0.01, hi=0.99):
    p = np.random.default_rng(seed).uniform(lo, hi, size=(d, d))
    assert not np.allclose(p, p.T)
    return p


def _prior(d, seed=0):
    from dibs_amd.models import EdgePriorDAGDistribution
    return EdgePriorDAGDistribution(d, _table(d, seed))


def _hand_sum(g, p, cols=None):
    """sum_{i != j} g_ij (log p_ij - log(1 - p_ij)), written out"""
    d, tot = g.shape[0], 0.0
    for i in range(d):
        for j in (range(d) if cols is None else cols):
            if i != j:
                tot += float(g[i, j]) * (np.log(p[i, j]) - np.log(1.0 - p[i, j]))
    return tot


# ---- the model class --------------------------------------------------------------------------------------------------------------------
def test_class_is_exported_beside_the_other_priors():
    import dibs_amd.models as models
    from dibs_amd.models.graph import EdgePriorDAGDistribution
    assert models.EdgePriorDAGDistribution is EdgePriorDAGDistribution
    assert EdgePriorDAGDistribution._dibs_prior == "edgewise"
    doc = EdgePriorDAGDistribution.__doc__
    assert "1e-6" in doc and "1 - 1e-6" in doc and "masking" in doc


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 1.5, np.nan, np.inf])
def test_validation_names_the_first_offending_entry(bad):
    from dibs_amd.models import EdgePriorDAGDistribution
    p = _table(5)
    p[3, 1] = bad
    p[4, 0] = bad   # (a later one: the message names the first)
    with pytest.raises(ValueError, match=r"\(3, 1\)"):
        EdgePriorDAGDistribution(5, p)


def test_validation_shape_and_diagonal():
    from dibs_amd.models import EdgePriorDAGDistribution
    with pytest.raises(ValueError, match="shape"):
        EdgePriorDAGDistribution(5, _table(4))
    p = _table(5)
    np.fill_diagonal(p, [0.0, 1.0, np.nan, -3.0, 7.0])   # the diagonal is ignored
    gm = EdgePriorDAGDistribution(5, p)
    assert not gm.log_odds.diagonal().any() and np.isfinite(gm.log_odds).all()
    q = _table(5)
    assert EdgePriorDAGDistribution(5, p).unnormalized_log_prob(g=np.ones((5, 5))) == EdgePriorDAGDistribution(5, q).unnormalized_log_prob(g=np.ones((5, 5)))


def test_log_probs_against_a_hand_written_sum():
    d = 6
    gm, p = _prior(d, 1), _table(d, 1)
    rng = np.random.default_rng(2)
    g = (rng.random((d, d)) < 0.4).astype(np.int32)
    soft = rng.random((d, d))
    assert abs(gm.unnormalized_log_prob(g=g) - _hand_sum(g, p)) < 1e-12
    assert abs(gm.unnormalized_log_prob_soft(soft_g=soft) - _hand_sum(soft, p)) < 1e-12
    for j in range(d):
        assert abs(gm.unnormalized_log_prob_single(g=g, j=j) - _hand_sum(g, p, cols=[j])) < 1e-12
    assert abs(sum(gm.unnormalized_log_prob_single(g=g, j=j) for j in range(d)) - gm.unnormalized_log_prob(g=g)) < 1e-12
    # asymmetric: the transposed graph has another probability
    assert abs(gm.unnormalized_log_prob(g=g) - gm.unnormalized_log_prob(g=g.T)) > 1e-3


def test_uniform_table_is_the_erdos_renyi_prior_up_to_its_constant():
    from dibs_amd.models import EdgePriorDAGDistribution, ErdosReniDAGDistribution
    d = 7
    er = ErdosReniDAGDistribution(d, 2)
    gm = EdgePriorDAGDistribution(d, np.full((d, d), er.p))
    rng = np.random.default_rng(3)
    g1, g2 = (np.triu((rng.random((d, d)) < q).astype(np.int32), 1) for q in (0.3, 0.6))
    want = er.unnormalized_log_prob(g=g1) - er.unnormalized_log_prob(g=g2)
    assert abs((gm.unnormalized_log_prob(g=g1) - gm.unnormalized_log_prob(g=g2)) - want) < 1e-10


def test_log_graph_prior_and_get_mixture_plumbing():
    """DiBS.log_graph_prior goes through unnormalized_log_prob_soft without further change"""
    from dibs_amd.inference import MarginalDiBS
    d = 5
    data, _, lm = make_data(d)
    gm = _prior(d, 4)
    dibs = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)
    soft = np.random.default_rng(5).random((d, d))
    assert abs(dibs.log_graph_prior(soft_g=soft) - _hand_sum(soft, _table(d, 4))) < 1e-12


def test_sample_g_returns_a_dag():
    from dibs_amd import random
    from dibs_amd.graph_utils import mat_is_dag
    d = 9
    gm = _prior(d, 6)
    seen = set()
    for s in range(20):
        g = gm.sample_G(random.PRNGKey(s))
        assert g.shape == (d, d) and set(np.unique(g)) <= {0, 1} and not g.diagonal().any()
        assert mat_is_dag(g)
        seen.add(g.tobytes())
    assert len(seen) > 1
    assert np.array_equal(gm.sample_G(random.PRNGKey(3)), gm.sample_G(random.PRNGKey(3)))


def test_sample_g_keeps_only_edges_of_a_near_certain_triangle():
    from dibs_amd import random
    from dibs_amd.models import EdgePriorDAGDistribution
    d = 8
    order = np.array([3, 0, 6, 1, 7, 2, 5, 4])
    rank = np.empty(d, np.int64)
    rank[order] = np.arange(d)
    tri = rank[:, None] < rank[None, :]
    gm = EdgePriorDAGDistribution(d, np.where(tri, 1.0 - 1e-9, 1e-9))
    n_edges = 0
    for s in range(20):
        g = gm.sample_G(random.PRNGKey(s))
        assert not g[~tri].any(), "an edge outside the triangle of the fixed order"
        n_edges += int(g.sum())
    assert n_edges > 0   # (the draws' own order agrees with the fixed one on some pairs)


# ---- ABI mirror -------------------------------------------------------------------------------------------------------------------------
def test_make_config_carries_the_enum_value():
    from dibs_amd._abi import PRIOR, make_config
    assert PRIOR["edgewise"] == 3
    assert make_config(n_vars=5, n_particles=4, n_observations=10, graph_prior="edgewise").graph_prior == 3
    hdr = open(os.path.join(ROOT, "include", "dibs_hip.h")).read()
    assert re.search(r"DIBS_PRIOR_EDGEWISE\s*=\s*3\b", hdr)
    assert re.search(r"int\s+dibs_engine_set_edge_prior\s*\(\s*dibs_engine\s*\*\s*e\s*,\s*const\s+double\s*\*\s*edge_probs\s*\)\s*;", hdr)


def test_symbol_is_listed_and_the_abi_version_stayed():
    from dibs_amd import _abi, _lib
    assert "dibs_engine_set_edge_prior" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "dibs_hip.h")).read()
    assert int(re.search(r"#define DIBS_ABI_VERSION (\d+)", hdr).group(1)) == _abi.ABI_VERSION == 2   # (as for dibs_engine_set_chain_hparams)


def test_model_lowering_selects_the_prior():
    from dibs_amd.inference import JointDiBS, MarginalDiBS
    d = 5
    data, _, lm = make_data(d)
    assert MarginalDiBS(x=data.x, graph_model=_prior(d), likelihood_model=lm)._make_config(4, d).graph_prior == 3
    data, _, lm = make_data(d, joint=True)
    assert JointDiBS(x=data.x, graph_model=_prior(d), likelihood_model=lm)._make_config(4, d).graph_prior == 3


# ---- the five multi-run entry points ----------------------------------------------------------------------------------------------------
@pytest.fixture
def no_engine(monkeypatch):
    import dibs_amd.inference.batch as b
    import dibs_amd.inference.chains as c
    import dibs_amd.inference.joint_batch as jb
    import dibs_amd.engine as eng

    class NoEngine:
        def __init__(self, *a, **kw):
            raise AssertionError("an engine was created before the arguments had been validated")
    for mod in (b, c, jb, eng):
        monkeypatch.setattr(mod, "Engine", NoEngine)


def _marginal(d=5, seed=0, table_seed=0):
    from dibs_amd.inference import MarginalDiBS
    data, _, lm = make_data(d, seed=seed)
    return MarginalDiBS(x=data.x, graph_model=_prior(d, table_seed), likelihood_model=lm)


def _joint(d=5, seed=3, table_seed=0, **kw):
    from dibs_amd.inference import JointDiBS
    data, _, lm = make_data(d, seed=seed, joint=True)
    return JointDiBS(x=data.x, graph_model=_prior(d, table_seed), likelihood_model=lm, **kw)


def test_sample_batch_refuses(no_engine):
    from dibs_amd.inference import sample_batch
    with pytest.raises(ValueError, match=r"sample_batch: model 0 has an edge-wise graph prior.*per-problem tables are not built"):
        sample_batch([_marginal(), _marginal(seed=1)], keys=[0, 1], **ARGS)


def test_sample_sweep_refuses(no_engine):
    from dibs_amd.inference import sample_sweep
    with pytest.raises(ValueError, match=r"sample_sweep: model 0 has an edge-wise graph prior.*per-problem tables are not built"):
        sample_sweep([_marginal(), _marginal(seed=1)], keys=[0, 1], **ARGS)


def test_sample_joint_sweep_refuses(no_engine):
    from dibs_amd.inference import sample_joint_sweep
    with pytest.raises(ValueError, match=r"sample_joint_sweep: model 0 has an edge-wise graph prior.*per-problem tables are not built"):
        sample_joint_sweep([_joint(), _joint(alpha_linear=0.1)], keys=[0, 1], **ARGS)


def test_sample_chains_of_a_marginal_model_refuses(no_engine):
    """(a MarginalDiBS goes to the batched engine; a JointDiBS runs -- tests/test_gpu_edge_prior.py)"""
    from dibs_amd.inference import sample_chains
    with pytest.raises(ValueError, match=r"edge-wise graph prior.*per-problem tables are not built"):
        sample_chains(_marginal(), keys=[0, 1, 2], **ARGS)


def test_sample_joint_batch_compares_the_tables(no_engine):
    from dibs_amd.inference import sample_joint_batch
    with pytest.raises(ValueError, match=r"sample_joint_batch: model 1 differs from model 0 in edge_probs"):
        sample_joint_batch([_joint(), _joint(seed=4, table_seed=1)], keys=[0, 1], **ARGS)
    # an edge-wise model beside an Erdos-Renyi one: the prior kind is a shared field
    from dibs_amd.inference import JointDiBS
    data, gm, lm = make_data(5, seed=3, joint=True)
    with pytest.raises(ValueError, match=r"differs from model 0 in .*graph_prior"):
        sample_joint_batch([_joint(), JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm)], keys=[0, 1], **ARGS)
    # equal tables pass the validation: the next thing sample_joint_batch does is to create the engine
    with pytest.raises(AssertionError, match="an engine was created"):
        sample_joint_batch([_joint(), _joint(seed=4)], keys=[0, 1], **ARGS)
