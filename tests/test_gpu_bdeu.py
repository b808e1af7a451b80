"""BDeu on the device (include/dibs_hip.h, BDEU): k_bdeu_nodes against the float64 numpy definition on the
constructed cases of tests/bdeu_states.py (every launch shape of bdeu_plan among them; repeated graphs bit for bit), a second and later
problem per wave at the largest and the smallest tables, one SVGD step stage by stage, determinism and chunking, the facade, two rank
engines, and the refusals that need an engine.

Bounds.  Node scores and per-graph sums are double on the device: 1e-9 (1 + |value|), the bound tests/test_gpu_f64.py holds double
node scores to.  dibs_score_graphs' own `out` is float: it is held to the float rounding of the double sum (2^-23 relative, doubled).
LOGPROBS_Z (float sums of the node scores) likewise; W_LIK to the 2e-3 of tests/test_gpu_parity.py."""
import functools
import tempfile

import numpy as np
import pytest

from bdeu_states import CASES, TIER_CASES, build_score_check, decode_masks, graph_names, key_words, make_case, make_graphs, plan_of
from conftest import assert_update_parity, make_data, rel_err, update_check
from dibs_amd import random
from dibs_amd._abi import make_config
from dibs_amd._lib import DibsHipError
from dibs_amd.engine import Engine
from dibs_amd.inference import MarginalDiBS, scoring
from dibs_amd.inference.scoring import score_graphs
from dibs_amd.models import BDeu, ErdosReniDAGDistribution, bdeu_log_marginal_numpy
from dibs_amd.target import make_discrete_model
from oracle import prng

pytestmark = pytest.mark.gpu
F32 = 2.0 ** -22


def close(a, b, tol=1e-9):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= tol * (1 + np.abs(b))))


@functools.lru_cache(maxsize=None)
def _reference(case):
    """per-node float64 scores [4, d] of the case's four graphs (computed once, shared, never written)"""
    x, mask, r, eta = make_case(case)
    out = np.stack([bdeu_log_marginal_numpy(g, x, r, mask, eta, per_node=True) for g in make_graphs(case)])
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def score_check():
    """tests/tools/bdeu_score_check, for its --plan query: the launch shape of a size, from the header the launcher uses"""
    with tempfile.TemporaryDirectory() as td:
        yield build_score_check(td)


def _resident_waves(score_check, N, KW):
    """the waves bdeu_launch_nodes keeps resident: min(32, waves * floor(160 KiB / lds)) per CU"""
    import torch
    waves, _, _, lds = plan_of(score_check, N, KW)
    return min(32, waves * ((160 * 1024) // lds)) * torch.cuda.get_device_properties(0).multi_processor_count


def _score(eng, g, x, mask):
    """dibs_score_graphs of the n <= S graphs g: (node scores [n, d] double, the chunk's parent masks, out [n] float)"""
    n, d = g.shape[0], g.shape[-1]
    g = np.ascontiguousarray(g, np.int32)
    out = np.empty(n, np.float32)
    p = lambda a: None if a is None else a.ctypes.data
    m32 = None if mask is None else np.ascontiguousarray(mask, np.int32)
    rc = eng.lib.dibs_score_graphs(eng._h, p(g), None, n, p(x), p(m32), x.shape[0], p(out))
    assert rc == 0, eng.lib.dibs_last_error()
    ns = eng.read("NODE_SCORES")[:d * n].reshape(d, n).T              # the chunk's per-node doubles, [graph, node]
    return ns.copy(), eng.read("PARENT_MASKS")[:d * n * ((d + 63) // 64)], out


# ---- 1: hard graphs through dibs_score_graphs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_score_graphs_against_the_numpy_definition(case):
    x, mask, r, eta = make_case(case)
    g = make_graphs(case)
    names = graph_names(case)
    d, n = CASES[case]["d"], len(names)
    ref = _reference(case)
    eng = Engine(make_config(n_vars=d, n_particles=1, n_observations=1, likelihood="bdeu", bdeu_ess=eta, graph_prior="uniform",
                             n_grad_mc_samples=8, n_acyclicity_mc_samples=4))
    try:
        eng.set_arities(r)
        ns, masks, out = _score(eng, g, x, mask)
        if case in TIER_CASES:                                        # the same graphs twice in one call
            ns8, masks8, _ = _score(eng, np.concatenate([g, g]), x, mask)
    finally:
        eng.close()
    for i, name in enumerate(names):
        print(f"{case}/{name}: device {ns[i].sum():.12f} numpy {ref[i].sum():.12f} max node err "
              f"{np.abs(ns[i] - ref[i]).max():.2e}")
    assert np.array_equal(decode_masks(masks, 1, d, n)[0], g)
    assert close(ns, ref), (case, np.abs(ns - ref).max())
    assert close(ns.sum(axis=1), ref.sum(axis=1)), case               # per graph
    assert close(out, ns.sum(axis=1), F32), case                      # the float output is the rounded double sum
    if CASES[case]["interv"] == "node_all":
        assert (ns == 0.0).all(axis=0).any()                          # the node without a used row scores exactly 0, whatever its parents
    if case in TIER_CASES:
        assert np.array_equal(decode_masks(masks8, 1, d, 2 * n)[0], np.concatenate([g, g]))
        assert np.array_equal(ns8[:n], ns8[n:]) and np.array_equal(ns8[:n], ns), case   # a repeated graph scores the same, bit for bit
        assert close(ns8, np.concatenate([ref, ref])), case


def test_second_pass_of_the_grid_at_large_n(score_check):
    """256 graphs (16 distinct ones, tiled) against 2 049 rows through the facade: d S problems per chunk on the one resident wave per CU
    of the (1 wave, rows in LDS) plan, so every wave scores at least two problems -- the key-mask clear, the table re-initialisation and
    the stale entries of the previous problem's table"""
    case = "d5_n2049"
    x, mask, r, eta = make_case(case)
    d, N = CASES[case]["d"], CASES[case]["N"]
    rng = np.random.default_rng(11)
    g16 = (rng.random((16, d, d)) < 0.5).astype(np.int32) * (1 - np.eye(d, dtype=np.int32))
    assert len({gi.tobytes() for gi in g16}) == 16
    got = score_graphs(BDeu(n_vars=d, arities=r, equivalent_sample_size=eta), np.tile(g16, (16, 1, 1)), None, x, mask)
    S_chunk = int(next(reversed(scoring._ENGINES.values())).cfg.n_grad_mc_samples)
    resident = _resident_waves(score_check, N, key_words(r))
    print(f"{d * S_chunk} problems per call on {resident} resident waves")
    assert d * S_chunk >= 2 * resident, (d, S_chunk, resident)        # (otherwise no wave strides: the test would show nothing)
    want = np.array([bdeu_log_marginal_numpy(gi, x, r, mask, eta) for gi in g16])
    got = got.reshape(16, 16)                                         # [copy, graph]
    assert np.array_equal(got, np.tile(got[:1], (16, 1)))             # every copy of a graph, bit for bit
    assert close(got[0], want), np.abs(got[0] - want).max()


def test_score_graphs_facade_chunks_and_cache():
    """the Python scorer returns float64, chunk by chunk of the scoring engine's S graphs, and keys its engine cache on the arities"""
    case = "d5_n65_interv"
    x, mask, r, eta = make_case(case)
    lm = BDeu(n_vars=5, arities=r, equivalent_sample_size=eta)
    rng = np.random.default_rng(0)
    g = (rng.random((150, 5, 5)) < 0.4).astype(np.int32) * (1 - np.eye(5, dtype=np.int32))   # more than one chunk of 128
    got = score_graphs(lm, g, None, x, mask)
    assert got.dtype == np.float64
    want = np.array([bdeu_log_marginal_numpy(gi, x, r, mask, eta) for gi in g])
    assert close(got, want)
    r2 = np.array([3, 3, 4, 2, 5], np.int32)
    got2 = score_graphs(BDeu(n_vars=5, arities=r2, equivalent_sample_size=eta), g[:3], None, x, mask)
    assert close(got2, [bdeu_log_marginal_numpy(gi, x, r2, mask, eta) for gi in g[:3]]) and not close(got2, want[:3])


# ---- 2: one SVGD step, stage by stage ------------------------------------------------------------------------------------------------------
def _step_case(d, N, M=3, S=8):
    r = np.resize(np.array([2, 3, 4, 5, 7, 8, 16, 3], np.int32), d)
    rng = np.random.default_rng(d)
    x = rng.integers(0, r, size=(N, d))
    x[:, 1:] = np.where(rng.random((N, d - 1)) < 0.6, x[:, :-1] % r[1:], x[:, 1:])   # neighbouring columns depend on each other
    mask = np.zeros((N, d), np.int32)
    mask[rng.random(N) < 0.25, 2] = 1
    kw = dict(n_vars=d, n_particles=M, n_observations=N, n_grad_mc_samples=S, n_acyclicity_mc_samples=4)
    return x.astype(np.float32), mask, r, kw


@pytest.mark.parametrize("d,N", [(8, 65), (70, 40), (8, 2049)])
def test_one_step_stage_by_stage(d, N):
    x, mask, r, kw = _step_case(d, N)
    M, S, t = kw["n_particles"], kw["n_grad_mc_samples"], 2
    cfg = make_config(likelihood="bdeu", **kw)
    eng = Engine(cfg)
    bge = Engine(make_config(**kw))
    try:
        eng.set_arities(r)
        eng.set_data(x, mask)
        bge.set_data(np.random.default_rng(1).normal(size=(N, d)).astype(np.float32))
        for e in (eng, bge):
            e.init_particles(random.PRNGKey(4))
            e.run(0, 1)                                               # (t = 0 has alpha = 0: a step with it would show nothing)
        # the same particles in both (the first step moved them differently)
        prev = eng.get_state()
        bge.set_state(z=prev["z"], v_z=prev["v_z"], key=prev["key"], baseline=prev["baseline"])
        eng.run(t, 1)
        bge.run(t, 1)
        masks = eng.read("PARENT_MASKS")
        assert np.array_equal(masks, bge.read("PARENT_MASKS"))        # the same Threefry streams: the same graphs, bit for bit
        g = decode_masks(masks, M, d, S)
        assert g.sum() > 0 and all(g[:, :, i, i].sum() == 0 for i in range(d))
        ns = eng.read("NODE_SCORES").reshape(M, d, S)
        want = np.array([[bdeu_log_marginal_numpy(g[m, s], x, r, mask, per_node=True) for s in range(S)] for m in range(M)])   # [M, S, d]
        print(f"d={d}: node scores max err {np.abs(ns.transpose(0, 2, 1) - want).max():.2e} of {np.abs(want).max():.1f}")
        assert close(ns.transpose(0, 2, 1), want)
        # LOGPROBS_Z and W_LIK from the device's own scores, masks and node scores, in float64
        logp = ns.sum(axis=1)                                         # [M, S]
        assert close(eng.read("LOGPROBS_Z").reshape(M, S), logp, F32)
        alpha = float(np.float32(cfg.alpha_linear * t))
        probs = 1.0 / (1.0 + np.exp(-alpha * eng.read("SCORES").reshape(M, d, d).astype(np.float64)))
        w = np.exp(logp - logp.max(axis=1, keepdims=True))
        w /= w.sum(axis=1, keepdims=True)
        w_lik = alpha * (np.einsum("ms,msij->mij", w, g.astype(np.float64)) - probs) * (1 - np.eye(d))
        assert rel_err(eng.read("W_LIK").reshape(M, d, d), w_lik) < 2e-3
        # the optimizer step from the engine's own phi
        st = eng.get_state()
        phi = eng.read("PHI_Z")
        assert np.isfinite(phi).all() and np.abs(phi).max() > 0
        u = update_check(cfg, prev["z"], prev["v_z"], phi, phi, st["z"], st["z"])
        assert_update_parity(u, 0.0, f"bdeu d={d}")
    finally:
        eng.close()
        bge.close()


def test_second_pass_of_the_grid_at_small_n():
    """one SVGD step with more problems than waves fit the device (32 per CU at the smallest tables): M d S > 32 CUs, so waves score a
    second problem on training data, 8 rows with interventions on one column"""
    import torch
    d, S, N = 16, 32, 8
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = (32 * cus) // (d * S) + 4
    assert M * d * S > 32 * cus
    x, _, r, kw = _step_case(d, N, M=M, S=S)
    mask = np.zeros((N, d), np.int32)
    mask[[1, 5], 2] = 1
    eng = _engine(x, mask, r, kw, key=3)
    try:
        eng.run(0, 1)
        eng.run(2, 1)
        g = decode_masks(eng.read("PARENT_MASKS"), M, d, S)           # [M, S, d, d]
        ns = eng.read("NODE_SCORES").reshape(M, d, S)
    finally:
        eng.close()

    @functools.lru_cache(maxsize=None)
    def node_score(j, parents):
        """score of node j under the parent set `parents` (bytes of a 0/1 column): the definition on the columns (parents, j) alone, the
        parents' own scores left out by marking their rows unused"""
        pa = np.nonzero(np.frombuffer(parents, np.int32))[0]
        cols = list(pa) + [j]
        gs = np.zeros((len(cols), len(cols)), np.int32)
        gs[:-1, -1] = 1
        ms = np.ones((N, len(cols)), np.int32)
        ms[:, -1] = mask[:, j]
        return bdeu_log_marginal_numpy(gs, x[:, cols], r[cols], ms, per_node=True)[-1]

    want = np.array([[[node_score(j, np.ascontiguousarray(g[m, s, :, j]).tobytes()) for s in range(S)] for j in range(d)] for m in range(M)])
    print(f"{M * d * S} problems on {cus} CUs, {node_score.cache_info().currsize} distinct (node, parent set); max err {np.abs(ns - want).max():.2e}")
    full = bdeu_log_marginal_numpy(g[0, 0], x, r, mask, per_node=True)   # (the cached form is the definition's: one graph scored whole)
    assert np.array_equal(full, want[0, :, 0])
    assert g.sum() > 0 and np.abs(ns).max() > 0
    assert close(ns, want), np.abs(ns - want).max()


# ---- 3: determinism and chunking -----------------------------------------------------------------------------------------------------------
def _engine(x, mask, r, kw, key=1, **more):
    e = Engine(make_config(likelihood="bdeu", **{**kw, **more}))
    e.set_arities(r)
    e.set_data(x, mask)
    e.init_particles(random.PRNGKey(key))
    return e


@pytest.mark.parametrize("N", [220, 2049])
def test_determinism_across_plans(N):
    """three steps in one call and one by one, at (2 waves, rows global) and (1 wave, rows in LDS): state and node scores bit for bit"""
    x, mask, r, kw = _step_case(8, N)
    a, b = (_engine(x, mask, r, kw) for _ in range(2))
    try:
        a.run(0, 3)
        for t in range(3):
            b.run(t, 1)
        sa, sb = a.get_state(), b.get_state()
        for name in ("z", "v_z", "key", "baseline"):
            assert np.array_equal(sa[name], sb[name]), name
        assert np.array_equal(a.read("NODE_SCORES"), b.read("NODE_SCORES")) and np.abs(a.read("NODE_SCORES")).max() > 0
    finally:
        a.close()
        b.close()


def test_determinism_and_chunking():
    x, mask, r, kw = _step_case(8, 65)
    a, b, c = (_engine(x, mask, r, kw) for _ in range(3))
    try:
        a.run(0, 6)
        for t in range(6):
            b.run(t, 1)
        sa, sb = a.get_state(), b.get_state()
        for name in ("z", "v_z", "key", "baseline"):
            assert np.array_equal(sa[name], sb[name]), name
        assert np.array_equal(a.read("NODE_SCORES"), b.read("NODE_SCORES"))
        # the same step twice from the same state
        c.run(0, 3)
        before = c.get_state()
        c.run(3, 1)
        first = c.read("NODE_SCORES").copy()
        c.set_state(z=before["z"], v_z=before["v_z"], key=before["key"], baseline=before["baseline"])
        c.run(3, 1)
        assert np.array_equal(first, c.read("NODE_SCORES")) and np.abs(first).max() > 0
    finally:
        for e in (a, b, c):
            e.close()


def _dibs(d=8, N=65, **kw):
    x, mask, r, _ = _step_case(d, N)
    lm = BDeu(n_vars=d, arities=r)
    gm = ErdosReniDAGDistribution(n_vars=d, n_edges_per_node=1)
    return x, mask, r, MarginalDiBS(x=x, interv_mask=mask, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=8, n_acyclicity_mc_samples=4, **kw)


def test_sample_with_a_callback_has_the_shape_of_the_bge_path():
    x, mask, r, m = _dibs()
    seen = []
    g = m.sample(key=random.PRNGKey(2), n_particles=3, steps=5, callback_every=2, callback=lambda dibs, t, zs: seen.append((t, zs.shape, zs.dtype)))
    data, gm, lm = make_data(8, n_obs=65)
    ref = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=8, n_acyclicity_mc_samples=4)
    seen_ref = []
    g_ref = ref.sample(key=random.PRNGKey(2), n_particles=3, steps=5, callback_every=2, callback=lambda dibs, t, zs: seen_ref.append((t, zs.shape, zs.dtype)))
    assert g.shape == g_ref.shape == (3, 8, 8) and g.dtype == g_ref.dtype
    assert seen == seen_ref and len(seen) == 3
    assert np.isfinite(m.last_state["z"]).all() and m.last_state["z"].dtype == ref.last_state["z"].dtype
    assert m.get_empirical(g).logp.shape[0] >= 1


# ---- 4: the facade -------------------------------------------------------------------------------------------------------------------------
def test_get_mixture_and_held_out_scorers():
    data, gm, lm = make_discrete_model(key=random.PRNGKey(2), n_vars=6, arities=[2, 3, 4, 2, 5, 3], n_observations=60, n_ho_observations=33,
                                       n_intervention_sets=2, edges_per_node=1)
    m = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=8, n_acyclicity_mc_samples=4)
    rng = np.random.default_rng(3)
    g = np.stack([np.triu((rng.random((6, 6)) < 0.4).astype(np.int32), 1) for _ in range(5)] + [np.asarray(data.g, np.int32)])
    logp = np.array([bdeu_log_marginal_numpy(gi, data.x, lm.arities) for gi in g])
    want = logp - logp.max()
    want -= np.log(np.exp(want).sum())
    mix = m.get_mixture(g)
    assert close(mix.logp, want) and close(np.exp(mix.logp), np.exp(want))
    assert close(m.eltwise_log_joint_prob(g, None), logp)
    assert close(m.eltwise_log_marginal_likelihood_observ(g, data.x_ho), [bdeu_log_marginal_numpy(gi, data.x_ho, lm.arities) for gi in g])
    interv, xi = data.x_interv[0]
    mi = np.zeros(xi.shape, np.int32)
    mi[:, list(interv)] = 1
    got = m.eltwise_log_marginal_likelihood_interv(g, xi, mi)
    assert close(got, [bdeu_log_marginal_numpy(gi, xi, lm.arities, mi) for gi in g])
    assert close(lm.log_marginal_likelihood(g=g[5], x=xi, interv_targets=mi), got[5])


def test_explicit_keys_reproduce_the_engines_own_step():
    x, mask, r, dibs = _dibs()
    d, M, t = 8, 3, 3
    eng = Engine(dibs._make_config(M, d))
    eng.set_arities(r)
    eng.set_data(x, mask)
    eng.init_particles(random.PRNGKey(1))
    eng.run(0, t)
    st = eng.get_state()
    k1 = prng.split(st["key"], M + 1, "legacy")
    k2 = prng.split(k1[0], M + 1, "legacy")
    eng.run(t, 1)
    total = eng.read("GRAD_Z").reshape(M, d, d, 2)
    eng.close()
    gz, _ = dibs.eltwise_grad_z_likelihood(st["z"], None, st["baseline"], t, k1[1:])
    gp = dibs.eltwise_grad_latent_prior(st["z"], k2[1:], t)
    assert np.abs(gz).max() > 0
    assert rel_err(gz + gp, total) < 2e-6


def test_median_bandwidth_step_equals_the_fixed_bandwidth_engine():
    x, mask, r, kw = _step_case(8, 65, M=5)
    med = _engine(x, mask, r, kw, key=7, h_latent="median")
    try:
        for t in range(2):
            before = med.get_state()
            med.run(t, 1)
            h = med.read("BANDWIDTH")
            after = med.get_state()
            fixed = _engine(x, mask, r, kw, h_latent=float(h[0]))
            try:
                fixed.set_state(z=before["z"], v_z=before["v_z"], key=before["key"], baseline=before["baseline"])
                fixed.run(t, 1)
                got = fixed.get_state()
                for name in ("z", "v_z", "key", "baseline"):
                    assert np.array_equal(after[name], got[name]), (name, t, h)
            finally:
                fixed.close()
    finally:
        med.close()
    _, _, _, m = _dibs(kernel_param={"h": "median"})
    m.sample(key=random.PRNGKey(1), n_particles=4, steps=3)
    assert m.last_bandwidth[0] > 0 and m.last_bandwidth[0] != np.float32(5.0) and np.isfinite(m.last_state["z"]).all()


# ---- 5: rank engines -----------------------------------------------------------------------------------------------------------------------
def test_two_rank_engines_equal_the_halves_of_one():
    import torch
    x, mask, r, kw = _step_case(8, 65, M=4)
    one = _engine(x, mask, r, kw, key=5)
    tstream = torch.cuda.Stream()
    ranks = []
    try:
        for rank in range(2):
            e = Engine(make_config(likelihood="bdeu", rank=rank, n_ranks=2, **kw), stream=tstream.cuda_stream)
            e.set_arities(r)
            e.set_data(x, mask)
            e.init_particles(random.PRNGKey(5))
            ranks.append(e)
        n = ranks[0].gather_elems_per_rank()
        with torch.cuda.stream(tstream):
            sends = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(2)]
            recv = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
            for t in range(2):
                for e, s in zip(ranks, sends):
                    e.step_local(t, s.data_ptr())
                torch.cat(sends, out=recv)
                if t == 0:
                    for e in ranks:
                        e.step_update(t, recv.data_ptr())
        torch.cuda.synchronize()
        one.run(0, 1)
        send1 = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()                                      # (the zero fill ran on torch's stream, the engine has its own)
        one.step_local(1, send1.data_ptr())
        one.sync()
        for name in ("PARENT_MASKS", "NODE_SCORES"):
            whole = one.read(name)
            halves = np.concatenate([e.read(name) for e in ranks])
            assert np.array_equal(whole, halves), name
        assert np.abs(one.read("NODE_SCORES")).max() > 0
    finally:
        one.close()
        for e in ranks:
            e.close()


# ---- 6: refusals on the device -------------------------------------------------------------------------------------------------------------
def test_device_refusals():
    x, mask, r, kw = _step_case(8, 65)
    e = Engine(make_config(likelihood="bdeu", **kw))
    bge = Engine(make_config(**kw))
    try:
        with pytest.raises(DibsHipError, match="^BDeu: dibs_engine_set_data: dibs_engine_set_arities has not been called"):
            e.set_data(x, mask)
        g, out = np.zeros((1, 8, 8), np.int32), np.zeros(1, np.float32)
        rc = e.lib.dibs_score_graphs(e._h, g.ctypes.data, None, 1, x.ctypes.data, None, x.shape[0], out.ctypes.data)
        assert rc != 0 and e.lib.dibs_last_error().decode().startswith("BDeu: dibs_score_graphs: dibs_engine_set_arities has not been called")
        with pytest.raises(DibsHipError, match="not a BDeu engine"):
            bge.set_arities(r)
        with pytest.raises(DibsHipError, match="^BDeu: arity 17 of variable 3 is outside the supported range \\[2, 16\\]"):
            e.set_arities(np.where(np.arange(8) == 3, 17, r))
        with pytest.raises(DibsHipError, match="^BDeu: arity 1 of variable 0"):
            e.set_arities(np.where(np.arange(8) == 0, 1, r))
        e.set_arities(r)
        e.init_particles(random.PRNGKey(0))
        with pytest.raises(DibsHipError, match="dibs_engine_set_data has not been called"):
            e.run(0, 1)
        bad = x.copy()
        bad[11, 4] = 1.5
        with pytest.raises(DibsHipError, match=r"^BDeu: dibs_engine_set_data: x\[11, 4\] = 1.5 is not a category code"):
            e.set_data(bad, mask)
        bad[11, 4] = float(r[4])
        with pytest.raises(DibsHipError, match=rf"x\[11, 4\] = {int(r[4])} is not a category code of variable 4 \(integers 0 \.\. {int(r[4]) - 1}\)"):
            e.set_data(bad, mask)
        with pytest.raises(DibsHipError, match="dibs_engine_set_data has not been called"):
            e.run(0, 1)                                               # (a failed set_data leaves the engine without data)
        e.set_data(x, mask)
        big = np.zeros((4097, 8), np.float32)
        rc = e.lib.dibs_score_graphs(e._h, g.ctypes.data, None, 1, big.ctypes.data, None, 4097, out.ctypes.data)
        msg = e.lib.dibs_last_error().decode()
        assert rc != 0 and msg.startswith("BDeu: dibs_score_graphs: 4097 observations") and "1 .. 4096" in msg
        e.run(0, 1)                                                   # the engine is still usable
        assert np.isfinite(e.get_state()["z"]).all()
    finally:
        e.close()
        bge.close()
    wide = Engine(make_config(likelihood="bdeu", **{**kw, "n_vars": 200}))
    try:
        with pytest.raises(DibsHipError, match="^BDeu: the bit fields of a packed row need 13 64-bit words, more than 8"):
            wide.set_arities(np.full(200, 16, np.int32))
    finally:
        wide.close()
