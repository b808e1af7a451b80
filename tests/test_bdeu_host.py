"""Host-side checks of the BDeu marginal likelihood on discrete data (include/dibs_hip.h, BDEU): the float64
definition ``bdeu_log_marginal_numpy`` against an independent restatement with the log-gamma function (``mpmath.loggamma``, 40 digits)
and against the properties a BDeu score has; the plain-C++ header the kernel shares with the host (tests/tools/bdeu_score_check.cpp), and that the cases of
tests/bdeu_states.py reach every launch shape its plan can pick; the facade's lowering and every
refusal (those of dibs_engine_create come before any device call, so they run without a GPU); the discrete-data factory."""
import fractions
import functools
import itertools
import subprocess
import tempfile

import mpmath
import numpy as np
import pytest

from bdeu_states import (CASES, PLAN_TIERS, TIER_CASES, arities_of, build_score_check, graph_names, key_words, make_case, make_graphs,
                         plan_of)
from dibs_amd import random
from dibs_amd._abi import LIK, make_config
from dibs_amd._lib import DibsHipError
from dibs_amd.engine import Engine
from dibs_amd.graph_utils import mat_is_dag
from dibs_amd.inference import JointDiBS, MarginalDiBS, sample_batch, sample_sweep
from dibs_amd.models import BDeu, ErdosReniDAGDistribution, bdeu_log_marginal_numpy
from dibs_amd.target import make_discrete_model


@functools.lru_cache(maxsize=None)
def _lgamma(num, den, n):
    """lgamma(num / den + n) to 40 digits: at n = 4 096 a float64 gammaln is near 3e4, one ulp 3.6e-12, and a node of few large groups
    is a difference of such values four orders smaller"""
    return mpmath.loggamma(mpmath.mpf(num) / den + n)


def restated(g, x, arities, mask, eta):
    """BDeu as the textbooks write it: every one of the q configurations enumerated, the log-gamma function of alpha itself; evaluated
    with 40 digits and rounded once"""
    x = np.asarray(x, np.int64)
    N, d = x.shape
    eta = fractions.Fraction(eta)
    with mpmath.workdps(40):
        total = mpmath.mpf(0)
        for j in range(d):
            rows = np.ones(N, bool) if mask is None else mask[:, j] == 0
            pa = [i for i in range(d) if i != j and g[i, j]]
            q = int(np.prod([arities[i] for i in pa])) if pa else 1
            a, a1 = eta / q, eta / (q * int(arities[j]))
            for conf in itertools.product(*[range(arities[i]) for i in pa]):
                sel = rows & np.all(x[:, pa] == np.asarray(conf, np.int64), axis=1) if pa else rows
                n_ck = np.bincount(x[sel, j], minlength=arities[j])
                total += _lgamma(a.numerator, a.denominator, 0) - _lgamma(a.numerator, a.denominator, int(n_ck.sum()))
                for v in n_ck:
                    total += _lgamma(a1.numerator, a1.denominator, int(v)) - _lgamma(a1.numerator, a1.denominator, 0)
        return float(total)


def _max_q(g, arities):
    d = len(arities)
    return max(int(np.prod([int(arities[i]) for i in range(d) if i != j and g[i, j]] or [1])) for j in range(d))


@pytest.mark.parametrize("case", [c for c in CASES if CASES[c]["d"] <= 7])
def test_numpy_definition_against_gammaln_restatement(case):
    x, mask, r, eta = make_case(case)
    n = 0
    for name, g in zip(graph_names(case), make_graphs(case)):
        if _max_q(g, r) > 10 ** 4:   # (the restatement enumerates all q configurations)
            continue
        got, want = bdeu_log_marginal_numpy(g, x, r, mask, eta), restated(g, x, r, mask, eta)
        assert abs(got - want) <= 1e-12 * (1 + abs(want)), (case, name, got, want)
        per = bdeu_log_marginal_numpy(g, x, r, mask, eta, per_node=True)
        assert per.shape == (len(r),) and abs(per.sum() - got) <= 1e-12 * (1 + abs(got))
        n += 1
    assert n >= 2


def test_score_equivalence_collider_and_limits():
    rng = np.random.default_rng(0)
    r = np.array([2, 3, 4], np.int32)
    x = rng.integers(0, r, size=(65, 3)).astype(np.float32)
    x[:, 1] = (x[:, 0] + (rng.random(65) < 0.2)) % 3   # dependent columns: the scores of different classes differ clearly
    x[:, 2] = (x[:, 1] + (rng.random(65) < 0.2)) % 4

    def G(*edges):
        g = np.zeros((3, 3), np.int32)
        for i, j in edges:
            g[i, j] = 1
        return g
    f = lambda g: bdeu_log_marginal_numpy(g, x, r)
    pairs = [(G((0, 1)), G((1, 0))), (G((0, 1), (1, 2)), G((2, 1), (1, 0))), (G((0, 1), (1, 2)), G((1, 0), (1, 2)))]
    for a, b in pairs:   # 0 -> 1 | 1 -> 0, chain | reversed chain, chain | fork: Markov equivalent
        assert abs(f(a) - f(b)) < 1e-10
    assert abs(f(G((0, 1), (2, 1))) - f(G((0, 1), (1, 2)))) > 1     # the collider is not
    # 200 parents of arity 16: alpha = eta / q leaves double range, log alpha does not
    d, N = 201, 40
    big = rng.integers(0, 16, size=(N, d)).astype(np.float32)
    g = np.zeros((d, d), np.int32)
    g[1:, 0] = 1
    v = bdeu_log_marginal_numpy(g, big, 16, per_node=True)
    assert np.all(np.isfinite(v)) and v[0] < 0
    # a node whose rows are all intervened on scores 0; the others do not change
    mask = np.zeros((65, 3), np.int32)
    mask[:, 1] = 1
    per = bdeu_log_marginal_numpy(G((0, 1), (1, 2)), x, r, mask, per_node=True)
    assert per[1] == 0.0 and per[0] == bdeu_log_marginal_numpy(G((0, 1), (1, 2)), x, r, per_node=True)[0] and per[2] < 0


@pytest.fixture(scope="module")
def score_check():
    with tempfile.TemporaryDirectory() as td:
        yield build_score_check(td)


def test_bdeu_score_header_against_plain_loops(score_check):
    r = subprocess.run([score_check], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert "bdeu_score_check: ok" in r.stdout and "check_hash: at most" in r.stdout


def test_cases_cover_every_launch_shape_of_the_plan(score_check):
    """the cases of tests/bdeu_states.py reach all six (waves per block, rows in LDS) pairs of bdeu_plan and every table size it can return
    up to the limit; the plan is asked of the header (bdeu_score_check --plan), so a later change to it that un-covers a shape fails here"""
    assert key_words([16] * 128) == 8 and key_words([16] * 40) == 3 and key_words([2] * 130) == 3 and key_words([4] * 30) == 1
    plans = {case: plan_of(score_check, c["N"], key_words(arities_of(case))) for case, c in CASES.items()}
    for case, pl in plans.items():
        print(f"{case}: N = {CASES[case]['N']}, KW = {key_words(arities_of(case))}: waves {pl[0]}, rows in LDS {pl[1]}, T {pl[2]}, {pl[3]} bytes")
    pairs = sorted({pl[:2] for pl in plans.values()})
    sizes = sorted({pl[2] for pl in plans.values()})
    print("plans", pairs, "table sizes", sizes)
    assert pairs == [(w, l) for w in (1, 2, 4) for l in (0, 1)]
    assert sizes == [64 << k for k in range(8)] and sizes[-1] == plan_of(score_check, 4096, 1)[2]
    for N, tier in PLAN_TIERS.items():                                # what the table of cases says of itself
        assert plans[f"d5_n{N}"][:3] == tier, (N, plans[f"d5_n{N}"], tier)
    assert len(TIER_CASES) == len(PLAN_TIERS)
    assert plans["d128_arity16_kw8"][:2] == (4, 0) and plans["d40_arity16_n1400"][:2] == (2, 0)
    assert subprocess.run([score_check, "--plan", "4097", "1"], capture_output=True).returncode != 0


def _model(d=5, arities=3, n=20, **kw):
    data, gm, lm = make_discrete_model(key=random.PRNGKey(3), n_vars=d, arities=arities, n_observations=n, edges_per_node=1)
    return data, gm, lm, MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, **kw)


def test_config_lowering():
    assert LIK["bdeu"] == 3
    base = dict(n_vars=5, n_particles=4, n_observations=10)
    c = make_config(likelihood="bdeu", bdeu_ess=2.5, **base)
    assert c.likelihood == 3 and c.reserved_d[0] == 2.5 and list(c.reserved_d)[1:] == [0.0] * 5
    assert make_config(likelihood="bdeu", **base).reserved_d[0] == 1.0
    assert list(make_config(**base).reserved_d) == [0.0] * 6          # (BGe: the slot stays unused)
    lm = BDeu(n_vars=5, arities=[2, 3, 4, 2, 5], equivalent_sample_size=10.0)
    assert lm._dibs_likelihood == "bdeu" and lm._config_kwargs() == dict(likelihood="bdeu", bdeu_ess=10.0)
    assert BDeu(n_vars=4, arities=3).arities.tolist() == [3, 3, 3, 3]
    for f in (lambda: lm.get_theta_shape(n_vars=5), lambda: lm.sample_parameters(key=None, n_vars=5),
              lambda: lm.sample_obs(key=None, n_samples=1, g=None, theta=None)):
        with pytest.raises(NotImplementedError):
            f()
    with pytest.raises(ValueError):
        BDeu(n_vars=5, arities=[2, 3])
    with pytest.raises(ValueError):
        BDeu(n_vars=2, arities=[2, 1])
    with pytest.raises(ValueError):
        BDeu(n_vars=2, arities=2, equivalent_sample_size=0.0)
    _, _, _, m = _model()
    c = m._make_config(4, 5)
    assert c.likelihood == 3 and c.joint == 0 and c.grad_estimator_z == 0 and c.reserved_d[0] == 1.0 and c.n_observations == 20


def test_facade_refusals():
    data, gm, lm, _ = _model()
    with pytest.raises(ValueError, match="reparam.*soft-graph"):
        MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, grad_estimator_z="reparam")
    with pytest.raises(ValueError, match="float64"):
        MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, precision="float64")
    with pytest.raises(NotImplementedError, match="likelihood_model must be one of"):
        JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm)
    bad = data.x.copy()
    bad[7, 2] = 3.0
    with pytest.raises(ValueError, match=r"column 2 of x holds .*3\.0.*arity 3"):
        MarginalDiBS(x=bad, graph_model=gm, likelihood_model=lm)
    bad[4, 1] = 0.5                                                   # (the first offending column is named)
    with pytest.raises(ValueError, match=r"column 1 of x holds .*0\.5"):
        MarginalDiBS(x=bad, graph_model=gm, likelihood_model=lm)
    bad = data.x.copy()
    bad[0, 0] = -1.0
    with pytest.raises(ValueError, match="column 0"):
        MarginalDiBS(x=bad, graph_model=gm, likelihood_model=lm)
    models = [MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm) for _ in range(2)]
    keys = [random.PRNGKey(0), random.PRNGKey(1)]
    for f in (sample_batch, sample_sweep):
        with pytest.raises(ValueError, match="BDeu"):
            f(models, keys=keys, n_particles=4, steps=2)


@pytest.mark.parametrize("kw,msg", [
    (dict(joint=True, grad_estimator_z="score"), "^BDeu: joint = 1 is not supported"),
    (dict(grad_estimator_z="reparam"), "^BDeu: the reparam estimator is not supported"),
    (dict(n_observations=4097), "^BDeu: n_observations = 4097 but must be in \\[1, 4096\\]"),
    (dict(precision=64), "^float64 engine: only the BGe marginal likelihood"),
    (dict(n_problems=3), "^batched engine \\(n_problems > 1\\): only the BGe marginal likelihood"),
])
def test_create_refusals_before_any_device_call(kw, msg):
    base = dict(n_vars=5, n_particles=4, n_observations=10, likelihood="bdeu")
    base.update(kw)
    with pytest.raises(DibsHipError, match=msg):
        Engine(make_config(**base))


def test_make_discrete_model():
    kw = dict(n_vars=8, arities=[2, 3, 4, 2, 5, 3, 2, 7], n_observations=50, n_ho_observations=30, n_intervention_sets=3)
    data, gm, lm = make_discrete_model(key=random.PRNGKey(5), **kw)
    assert isinstance(gm, ErdosReniDAGDistribution) and isinstance(lm, BDeu)
    assert data.x.shape == (50, 8) and data.x_ho.shape == (30, 8) and data.x.dtype == np.float32
    assert mat_is_dag(data.g)
    for x in [data.x, data.x_ho] + [xi for _, xi in data.x_interv]:
        lm.check_data(x)                                              # integral, 0 <= x < arity column by column
    assert len(data.x_interv) == 3
    for interv, xi in data.x_interv:
        assert xi.shape == (50, 8)
        for node, value in interv.items():
            assert 0 <= value < lm.arities[node] and np.all(xi[:, node] == value)
    again, _, _ = make_discrete_model(key=random.PRNGKey(5), **kw)
    assert np.array_equal(again.x, data.x) and np.array_equal(again.g, data.g) and np.array_equal(again.x_interv[2][1], data.x_interv[2][1])
    other, _, _ = make_discrete_model(key=random.PRNGKey(6), **kw)
    assert not np.array_equal(other.x, data.x)
    # the data depend on the graph: the true graph outscores the empty one on enough data
    big, _, lm3 = make_discrete_model(key=random.PRNGKey(1), n_vars=6, arities=3, n_observations=500)
    assert big.g.sum() > 0
    assert bdeu_log_marginal_numpy(big.g, big.x, lm3.arities) > bdeu_log_marginal_numpy(np.zeros((6, 6)), big.x, lm3.arities)
