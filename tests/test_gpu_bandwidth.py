"""GPU tests of the median-heuristic kernel bandwidth (include/dibs_hip.h, MEDIAN-HEURISTIC KERNEL BANDWIDTH):
the selection is exact, the distances are right, a step on the rule equals -- bit for bit -- the step of a fixed-rule engine configured
with the bandwidths the rule selected, chunking is transparent, and the multi-run engines keep run i identical to the standalone engine.
S = 16, Sa = 8 throughout; every state comparison is np.array_equal."""
import math

import numpy as np
import pytest

from conftest import make_data, rel_err
from dibs_amd import random
from dibs_amd._abi import make_config
from dibs_amd.engine import Engine

pytestmark = pytest.mark.gpu

STATE = ("z", "v_z", "theta", "v_theta", "baseline")
FLT_MIN = np.finfo(np.float32).tiny
CHUNKS = [(0, 5), (5, 3)]


# ---- configurations and data ------------------------------------------------------------------------------------------------------------
def _bge(d, M, **kw):
    return dict(dict(n_vars=d, n_particles=M, n_grad_mc_samples=16, n_acyclicity_mc_samples=8, h_latent="median"), **kw)


def _lin(d, M, **kw):
    return dict(dict(n_vars=d, n_particles=M, joint=True, likelihood="lingauss", n_grad_mc_samples=16, n_acyclicity_mc_samples=8), **kw)


def _nn(d, M, **kw):
    return dict(dict(n_vars=d, n_particles=M, joint=True, likelihood="densenn", nn_hidden=(5,), n_grad_mc_samples=16,
                     n_acyclicity_mc_samples=8), **kw)


_DATA = {}


def _x(d, joint, seed=1, n_obs=40):
    key = (d, joint, seed, n_obs)
    if key not in _DATA:
        data, _, _ = make_data(d, n_obs=n_obs, seed=seed, joint=joint)
        _DATA[key] = np.asarray(data.x, np.float32)[:n_obs]
    return _DATA[key]


def _engine(kw, x, key=None, **extra):
    e = Engine(make_config(n_observations=x.shape[0], **dict(kw, **extra)))
    e.set_data(x, None)
    if key is not None:
        e.init_particles(random.PRNGKey(key))
    return e


def _set(e, st):
    e.set_state(z=st["z"], v_z=st["v_z"], theta=st["theta"], v_theta=st["v_theta"], key=st["key"], baseline=st["baseline"])


def _assert_states_equal(a, b, what):
    assert np.isfinite(a["z"]).all() and np.isfinite(b["z"]).all(), what
    for k in STATE:
        if a[k] is None:
            assert b[k] is None, (what, k)
            continue
        assert np.array_equal(a[k], b[k]), (what, k, np.abs(a[k].astype(np.float64) - b[k]).max())
    assert np.array_equal(a["key"], b["key"]), what


# ---- the rule in numpy ------------------------------------------------------------------------------------------------------------------
def _sq_f64(x):
    """float64 squared distances of the rows of x [M, ...]"""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    return ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)


def _h_from_v(v, M):
    """the formula in float32 on a distance matrix v [M, M] (float32): upper triangle, sorted, the two middle order statistics"""
    u = np.sort(np.asarray(v, np.float32).reshape(M, M)[np.triu_indices(M, 1)])
    P = u.size
    med = u[(P - 1) // 2] if P % 2 else np.float32(np.float32(0.5) * np.float32(u[P // 2 - 1] + u[P // 2]))
    return np.float32(max(np.float32(np.float64(med) * (1.0 / math.log(M + 1))), FLT_MIN))


def _within_one_ulp(a, b):
    a, b = np.float32(a), np.float32(b)
    return a == b or a == np.nextafter(b, np.float32(np.inf)) or a == np.nextafter(b, np.float32(0))


def _lattice(M, d, rng):
    """rows of small integers with a few duplicated rows: every squared distance is an integer below 2^24 -- exact in float32 whatever the
    order of the sums -- with many ties and zeros"""
    z = rng.integers(-2, 3, size=(M, d, d, 2)).astype(np.float32)
    for a, b in ((1, 0), (M - 1, M // 2)):
        if a != b and a < M:
            z[a] = z[b]
    return z


# ---- 1: the selection is exact ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 4, 7, 33, 64, 255])   # one pair, both parities of P, FULL phi, the tiled matrix, the largest run
def test_selection_is_exact(M):
    d = 8
    x = _x(d, False)
    e = _engine(_bge(d, M), x, key=M)
    try:
        e.run(0, 1)
        h = e.read("BANDWIDTH")
        v = e.read("SQDIST_Z").reshape(M, M)
        assert h.shape == (2,) and h[1] == np.float32(500.0)   # (h_theta: not on the rule, the configuration's value)
        assert np.array_equal(v, v.T) and not v.diagonal().any() and np.isfinite(v).all()
        want = _h_from_v(v, M)
        print(f"M = {M}: h = {h[0]!r}, numpy {want!r}")
        assert _within_one_ulp(h[0], want), (h[0], want)
        # a lattice state: every distance exact, many ties, duplicated rows -> the distances and h equal numpy exactly
        st = e.get_state()
        z = _lattice(M, d, np.random.default_rng(M))
        e.set_state(z=z)
        e.run(1, 1)
        v = e.read("SQDIST_Z").reshape(M, M)
        assert np.array_equal(v, _sq_f64(z).astype(np.float32))
        assert e.read("BANDWIDTH")[0] == _h_from_v(v, M)
        assert st["z"].shape == z.shape
    finally:
        e.close()


def test_more_than_half_of_the_rows_identical_gives_flt_min_and_a_finite_state():
    # 7 of 9 rows identical: 21 of 36 pairs have distance 0, the median is 0 and the floor applies.  The other rows differ from the block by
    # less than 1 per coordinate: with h = FLT_MIN the repulsion's factor 2 / h is 1.7e38, and (2 / h) (x_b - x_a) must stay below FLT_MAX
    # for the zero kernel entry to annihilate it (limits)
    M, d = 9, 8
    e = _engine(_bge(d, M), _x(d, False), key=3)
    try:
        rng = np.random.default_rng(5)
        z = np.repeat(rng.normal(size=(1, d, d, 2)).astype(np.float32) * 0.3, M, axis=0)
        z[7] += rng.uniform(-0.4, 0.4, size=z[7].shape).astype(np.float32)
        z[8] += rng.uniform(-0.4, 0.4, size=z[8].shape).astype(np.float32)
        e.set_state(z=z)
        e.run(0, 1)
        assert e.read("BANDWIDTH")[0] == FLT_MIN
        st = e.get_state()
        assert np.isfinite(st["z"]).all() and np.isfinite(st["v_z"]).all()
        assert not np.array_equal(st["z"], z)
    finally:
        e.close()


# ---- 2: the distances are right ---------------------------------------------------------------------------------------------------------
# relative bound 1e-5 (max norm), the bound the stage tests hold KXX to: the terms are non-negative and a lane's float chain at
# D = 2 d k <= 5 000 is <= 40 fused adds, i.e. <= 2.4e-6
def test_distances_direct_path_both_segments():
    d, M = 8, 7
    e = _engine(_lin(d, M, h_latent="median", h_theta="median"), _x(d, True), key=2)
    try:
        e.run(0, 2)
        st = e.get_state()
        e.run(2, 1)
        for name, rows in (("SQDIST_Z", st["z"]), ("SQDIST_THETA", st["theta"])):
            err = rel_err(e.read(name).reshape(M, M), _sq_f64(rows))
            print(f"{name}: rel err {err:.2e}")
            assert err < 1e-5, (name, err)
    finally:
        e.close()


def test_distances_tiled_path(monkeypatch):
    monkeypatch.setenv("DIBS_KMAT_TILED_MIN", "64")
    d, M = 8, 64
    e = _engine(_bge(d, M), _x(d, False), key=4)
    try:
        e.run(0, 1)
        st = e.get_state()
        e.run(1, 1)
        err = rel_err(e.read("SQDIST_Z").reshape(M, M), _sq_f64(st["z"]))
        print(f"SQDIST_Z tiled: rel err {err:.2e}")
        assert err < 1e-5, err
    finally:
        e.close()


def test_a_segment_off_the_rule_has_no_distance_buffer():
    from dibs_amd import _lib
    e = _engine(_lin(6, 4, h_theta="median"), _x(6, True), key=1)
    try:
        with pytest.raises(_lib.DibsHipError, match="no such buffer"):
            e.read("SQDIST_Z")
        e.run(0, 1)
        assert e.read("SQDIST_THETA").shape == (16,)
        assert e.read("BANDWIDTH")[0] == np.float32(5.0)
    finally:
        e.close()
    e = _engine(_lin(6, 4), _x(6, True), key=1)   # the fixed rule: the configuration's values, no distance buffers
    try:
        assert np.array_equal(e.read("BANDWIDTH"), np.array([5.0, 500.0], np.float32))
        with pytest.raises(_lib.DibsHipError, match="no such buffer"):
            e.read("SQDIST_THETA")
    finally:
        e.close()


# ---- 3: a step on the rule equals the fixed-bandwidth engine's --------------------------------------------------------------------------
CASES = {
    "bge_d8_M7_direct_in_sample": (_bge(8, 7), False),
    "bge_d8_M64_full_phi": (_bge(8, 64), False),
    "bge_d8_M128_tiled": (_bge(8, 128), False),                # (D = 128: one chunk, the fixed engine's tiled matrix in phase B)
    "bge_d12_M128_tiled_riders": (_bge(12, 128), False),       # (D = 288: two chunks, the fixed engine's tile units ride in the tail launch)
    "lin_d6_M5": (_lin(6, 5, h_latent="median", h_theta="median"), True),
    "lin_d6_M64": (_lin(6, 64, h_latent="median", h_theta="median"), True),
    "nn_d5_M6": (_nn(5, 6, h_latent="median", h_theta="median", edges_per_node=1), True),   # (5 variables: 2 edges per node is no ER prior)
    "lin_latent_only": (_lin(6, 5, h_latent="median"), True),
    "lin_theta_only": (_lin(6, 5, h_theta="median"), True),
    "bge_gd": (_bge(8, 7, optimizer="gd", stepsize=0.05), False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_step_equals_the_fixed_bandwidth_engine(name):
    kw, joint = CASES[name]
    x = _x(kw["n_vars"], joint)
    med = _engine(kw, x, key=7)
    try:
        seen = []
        for t in range(3):
            before = med.get_state()
            med.run(t, 1)
            h = med.read("BANDWIDTH")
            after = med.get_state()
            fixed = _engine(kw, x, h_latent=float(h[0]), h_theta=float(h[1]))
            try:
                assert fixed.cfg.reserved_i[3] == 0
                _set(fixed, before)
                fixed.run(t, 1)
                _assert_states_equal(after, fixed.get_state(), (name, t, h))
            finally:
                fixed.close()
            seen.append(tuple(h))
        print(name, seen)
        rule = med.cfg.reserved_i[3]
        for s, dflt in ((0, 5.0), (1, 500.0)):
            if rule >> s & 1:
                assert len({h[s] for h in seen}) == 3, seen   # (the particles move: so does the bandwidth)
            else:
                assert all(h[s] == np.float32(dflt) for h in seen), seen
    finally:
        med.close()


# ---- 4: chunking and determinism --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bge_d8_M7_direct_in_sample", "lin_d6_M5"])
def test_chunking_and_determinism(name):
    kw, joint = CASES[name]
    x = _x(kw["n_vars"], joint)

    def run(chunks):
        e = _engine(kw, x, key=9)
        try:
            for t0, n in chunks:
                e.run(t0, n)
            return e.get_state(), e.read("BANDWIDTH")
        finally:
            e.close()

    one, h1 = run([(0, 6)])
    two, h2 = run([(0, 3), (3, 3)])
    again, h3 = run([(0, 6)])
    _assert_states_equal(one, two, "run(0, 6) against run(0, 3); run(3, 3)")
    _assert_states_equal(one, again, "two identical runs")
    assert np.array_equal(h1, h2) and np.array_equal(h1, h3)


# ---- 5: the multi-run engines -----------------------------------------------------------------------------------------------------------
def _multi(kw, count, datas, keys, shared):
    e = Engine(make_config(n_observations=datas[0].shape[0], **dict(kw, **count)))
    try:
        if shared:
            e.set_data(datas[0], None)
        else:
            for p, x in enumerate(datas):
                e.set_data_problem(p, x, None)
        e.init_particles_batch(np.stack([random.PRNGKey(k) for k in keys]))
        for t0, n in CHUNKS:
            e.run(t0, n)
        return e.get_state(), e.read("BANDWIDTH").reshape(len(keys), 2)
    finally:
        e.close()


def _check_multi(kw, count, datas, keys, shared):
    M, B = kw["n_particles"], len(keys)
    mst, mh = _multi(kw, count, datas, keys, shared)
    for p, key in enumerate(keys):
        e = _engine(kw, datas[0 if shared else p], key=key)
        try:
            for t0, n in CHUNKS:
                e.run(t0, n)
            st, h = e.get_state(), e.read("BANDWIDTH")
        finally:
            e.close()
        sl = slice(p * M, (p + 1) * M)
        run = {k: (None if mst[k] is None else mst[k][sl]) for k in STATE}
        run["key"] = mst["key"][p]
        _assert_states_equal(run, st, ("run", p))
        assert np.array_equal(mh[p], h), (p, mh[p], h)
    rule = make_config(n_observations=4, **kw).reserved_i[3]
    for s in range(2):
        if rule >> s & 1:
            assert len({float(v) for v in mh[:, s]}) == B, mh   # (every run selects its own bandwidth)


def test_batched_engine():
    _check_multi(_bge(8, 4), dict(n_problems=3), [_x(8, False, seed=s) for s in (1, 2, 3)], [3, 4, 5], shared=False)


@pytest.mark.parametrize("kind", ["lingauss", "densenn"])
def test_chains_engine(kind):
    kw = _lin(8, 4, h_latent="median", h_theta="median") if kind == "lingauss" else _nn(8, 4, h_latent="median", h_theta="median")
    _check_multi(kw, dict(n_chains=3), [_x(8, True)], [11, 12, 13], shared=True)


def test_chains_engine_with_per_chain_data():
    _check_multi(_lin(8, 4, h_latent="median", h_theta="median"), dict(n_chains=3), [_x(8, True, seed=s) for s in (1, 2, 3)], [21, 22, 23],
                 shared=False)


def _compare_facade(multi, seq, out, keys, joint, steps):
    for i, k in enumerate(keys):
        r = seq[i].sample(key=random.PRNGKey(k), n_particles=4, steps=steps)
        g = r[0] if joint else r
        assert np.array_equal(out[i][0] if joint else out[i], g), i
        if joint:
            assert np.array_equal(out[i][1], r[1]), i
        for name in seq[i].last_state:
            a, b = multi[i].last_state[name], seq[i].last_state[name]
            assert (a is None and b is None) or np.array_equal(a, b), (i, name)
        assert np.isfinite(seq[i].last_state["z"]).all()
        assert np.array_equal(multi[i].last_bandwidth, seq[i].last_bandwidth), i
    assert not np.array_equal(seq[0].last_state["z"], seq[1].last_state["z"])


def test_sample_sweep_on_the_rule():
    from dibs_amd.inference import MarginalDiBS, sample_sweep
    data, gm, lm = make_data(8, n_obs=40, seed=1)
    grid = lambda: [MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=8,
                                 alpha_linear=al, kernel_param={"h": "median"}) for al in (1.0, 0.5, 2.0)]
    multi, seq, keys = grid(), grid(), [31, 32, 33]
    out = sample_sweep(multi, keys=keys, n_particles=4, steps=5)
    _compare_facade(multi, seq, out, keys, False, 5)


def test_sample_joint_sweep_on_the_rule():
    from dibs_amd.inference import JointDiBS, sample_joint_sweep
    data, gm, lm = make_data(8, n_obs=40, seed=1, joint=True)
    grid = lambda: [JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=8,
                              alpha_linear=al, kernel_param={"h_latent": "median", "h_theta": "median"}) for al in (0.05, 0.1, 0.02)]
    multi, seq, keys = grid(), grid(), [41, 42, 43]
    out = sample_joint_sweep(multi, keys=keys, n_particles=4, steps=5)
    _compare_facade(multi, seq, out, keys, True, 5)


def test_sample_batch_and_sample_joint_batch_on_the_rule():
    from dibs_amd.inference import JointDiBS, MarginalDiBS, sample_batch, sample_joint_batch
    sets = [make_data(8, n_obs=40, seed=s) for s in (1, 2, 3)]
    grid = lambda: [MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=8,
                                 kernel_param={"h": "median"}) for data, gm, lm in sets]
    multi, seq, keys = grid(), grid(), [51, 52, 53]
    _compare_facade(multi, seq, sample_batch(multi, keys=keys, n_particles=4, steps=5), keys, False, 5)
    jsets = [make_data(8, n_obs=40, seed=s, joint=True) for s in (1, 2, 3)]
    jgrid = lambda: [JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=8,
                               kernel_param={"h_latent": "median", "h_theta": "median"}) for data, gm, lm in jsets]
    multi, seq = jgrid(), jgrid()
    _compare_facade(multi, seq, sample_joint_batch(multi, keys=keys, n_particles=4, steps=5), keys, True, 5)


@pytest.mark.parametrize("kind", ["lingauss", "densenn"])
def test_sample_chains_on_the_rule(kind):
    from dibs_amd.inference import JointDiBS, sample_chains
    if kind == "lingauss":
        data, gm, lm = make_data(8, n_obs=40, seed=1, joint=True)
    else:
        from dibs_amd.target import make_nonlinear_gaussian_model
        data, gm, lm = make_nonlinear_gaussian_model(key=random.PRNGKey(1), n_vars=8, graph_prior_str="er", edges_per_node=2, n_observations=40,
                                                     hidden_layers=(5,))
    new = lambda: JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=8,
                            kernel_param={"h_latent": "median", "h_theta": "median"})
    m, keys = new(), [61, 62, 63]
    out = sample_chains(m, keys=keys, n_particles=4, steps=5)
    for c, k in enumerate(keys):
        s = new()
        g, theta = s.sample(key=random.PRNGKey(k), n_particles=4, steps=5)
        assert np.array_equal(out[c][0], g), c
        for name in s.last_state:
            assert np.array_equal(m.last_chain_states[c][name], s.last_state[name]), (c, name)
        assert np.isfinite(s.last_state["z"]).all() and np.isfinite(s.last_state["theta"]).all()


# ---- 6: the facade ----------------------------------------------------------------------------------------------------------------------
def test_marginal_dibs_sample_sets_last_bandwidth():
    from dibs_amd.inference import JointDiBS, MarginalDiBS
    from dibs_amd.kernel import median_bandwidth
    data, gm, lm = make_data(8, n_obs=40, seed=1)
    m = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=8,
                     kernel_param={"h": "median"})
    seen = []
    g = m.sample(key=random.PRNGKey(1), n_particles=6, steps=4, callback_every=3, callback=lambda dibs, t, zs: seen.append(zs.copy()))
    assert g.shape == (6, 8, 8) and np.isfinite(m.last_state["z"]).all()
    h = m.last_bandwidth
    assert h.shape == (2,) and h.dtype == np.float32 and np.isfinite(h).all() and h[0] > 0 and h[1] == np.float32(500.0)
    assert h[0] != np.float32(5.0)
    # the documented host reference on the particles the last step started from is not available here (the last chunk has 3 steps); on
    # the particles after the first chunk it gives the bandwidth a further step would select: the same order of magnitude
    assert 0.1 < float(median_bandwidth(seen[0])) / float(h[0]) < 10
    dj, gj, lj = make_data(8, n_obs=40, seed=1, joint=True)
    j = JointDiBS(x=dj.x, graph_model=gj, likelihood_model=lj, n_grad_mc_samples=16, n_acyclicity_mc_samples=8,
                  kernel_param={"h_latent": "median", "h_theta": "median"})
    j.sample(key=random.PRNGKey(2), n_particles=4, steps=3)
    assert np.isfinite(j.last_state["theta"]).all() and (j.last_bandwidth > 0).all() and j.last_bandwidth[1] != np.float32(500.0)
    fixed = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=16, n_acyclicity_mc_samples=8)
    fixed.sample(key=random.PRNGKey(1), n_particles=4, steps=2)
    assert np.array_equal(fixed.last_bandwidth, np.array([5.0, 500.0], np.float32))
