"""GPU tests of the batched engine (include/dibs_hip.h, n_problems > 1) and of sample_batch: problem p of a batch must end BIT-IDENTICAL
to a standalone engine run with (x_p, mask_p, key_p) and the same chunking -- particles, RMSprop moments, score-function baselines and the
loop-carry key.  Every comparison is np.array_equal."""
import numpy as np
import pytest

from conftest import make_data
from dibs_amd import random
from dibs_amd._abi import make_config
from dibs_amd.engine import Engine
from dibs_amd.inference import MarginalDiBS, sample_batch

pytestmark = pytest.mark.gpu


def _problem(d, n_obs, seed, interv=False):
    data, gm, lm = make_data(d, n_obs=n_obs, seed=seed)
    x = np.asarray(data.x, np.float32)[:n_obs]
    mask = None
    if interv:  # hard interventions on a few nodes for a block of rows each
        mask = np.zeros(x.shape, np.int32)
        for q, j in enumerate((1, d // 2, d - 1)):
            mask[5 * q:5 * q + 4 + q, j] = 1
    return x, mask


def _standalone(kw, x, mask, key, chunks):
    e = Engine(make_config(n_observations=x.shape[0], **kw))
    try:
        e.set_data(x, mask)
        e.init_particles(random.PRNGKey(key))
        for t0, n in chunks:
            e.run(t0, n)
        return e.get_state()
    finally:
        e.close()


def _batched(kw, probs, keys, chunks):
    B = len(probs)
    e = Engine(make_config(n_observations=probs[0][0].shape[0], n_problems=B, **kw))
    try:
        for p, (x, mask) in enumerate(probs):
            e.set_data_problem(p, x, mask)
        e.init_particles_batch(np.stack([random.PRNGKey(k) for k in keys]))
        for t0, n in chunks:
            e.run(t0, n)
        return e.get_state()
    finally:
        e.close()


def _assert_problem_equal(bst, p, M, st):
    sl = slice(p * M, (p + 1) * M)
    assert np.isfinite(st["z"]).all(), p
    assert np.array_equal(bst["z"][sl], st["z"]), (p, np.abs(bst["z"][sl] - st["z"]).max())
    assert np.array_equal(bst["v_z"][sl], st["v_z"]), p
    assert np.array_equal(bst["baseline"][sl], st["baseline"]), p
    assert np.array_equal(bst["key"][p], st["key"]), p


def _check(kw, probs, keys, chunks):
    M = kw["n_particles"]
    bst = _batched(kw, probs, keys, chunks)
    assert bst["z"].shape[0] == len(probs) * M and bst["key"].shape == (len(probs), 2)
    for p, ((x, mask), key) in enumerate(zip(probs, keys)):
        _assert_problem_equal(bst, p, M, _standalone(kw, x, mask, key, chunks))
    return bst


def test_config2_shape_interventions_and_row_counts():
    d, M = 20, 32
    kw = dict(n_vars=d, n_particles=M, graph_prior="er")
    n_obs = (50, 80, 100, 120, 60)
    probs = [_problem(d, n, 10 + p, interv=(p == 2)) for p, n in enumerate(n_obs)]
    _check(kw, probs, [3, 4, 5, 6, 7], [(0, 6)])


@pytest.mark.parametrize("prior", ["sf", "uniform"])
def test_small_problems_gd_and_baseline(prior):
    d, M = 8, 4
    kw = dict(n_vars=d, n_particles=M, graph_prior=prior, optimizer="gd", stepsize=0.005, score_function_baseline=0.001,
              n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    probs = [_problem(d, 40 + 7 * p, 20 + p, interv=(p == 4)) for p in range(7)]
    _check(kw, probs, list(range(100, 107)), [(0, 5), (5, 3)])


def test_split_f16_acyclicity_tier():
    d, M = 50, 16
    kw = dict(n_vars=d, n_particles=M, n_grad_mc_samples=64, n_acyclicity_mc_samples=16)
    probs = [_problem(d, 100, 30 + p, interv=(p == 1)) for p in range(3)]
    _check(kw, probs, [1, 2, 3], [(0, 4)])


def test_wide_graphs_global_memory_paths():
    d, M = 130, 4
    kw = dict(n_vars=d, n_particles=M, n_grad_mc_samples=16, n_acyclicity_mc_samples=4)
    probs = [_problem(d, 60, 40), _problem(d, 70, 41, interv=True)]
    _check(kw, probs, [8, 9], [(0, 3)])


def test_chunking_is_transparent():
    d, M = 8, 4
    kw = dict(n_vars=d, n_particles=M, n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    probs = [_problem(d, 50, 50 + p) for p in range(3)]
    a = _batched(kw, probs, [1, 2, 3], [(0, 10), (10, 10)])
    b = _batched(kw, probs, [1, 2, 3], [(0, 20)])
    for k in ("z", "v_z", "baseline", "key"):
        assert np.array_equal(a[k], b[k]), k


def test_problems_are_isolated():
    d, M = 8, 4
    kw = dict(n_vars=d, n_particles=M, n_grad_mc_samples=32, n_acyclicity_mc_samples=8)
    p0, p1, p1b = _problem(d, 50, 60), _problem(d, 50, 61), _problem(d, 90, 62, interv=True)
    a = _batched(kw, [p0, p1], [1, 2], [(0, 8)])
    b = _batched(kw, [p0, p1b], [1, 2], [(0, 8)])
    sl = slice(0, M)
    for k in ("z", "v_z", "baseline"):
        assert np.array_equal(a[k][sl], b[k][sl]), k
    assert np.array_equal(a["key"][0], b["key"][0])
    assert not np.array_equal(a["z"][M:], b["z"][M:])


def test_keys_roundtrip_and_state_rules():
    d, M = 8, 4
    e = Engine(make_config(n_vars=d, n_particles=M, n_observations=50, n_problems=2, n_grad_mc_samples=16, n_acyclicity_mc_samples=4))
    try:
        from dibs_amd import _lib
        with pytest.raises(_lib.DibsHipError, match="set_data_problem"):
            e.run(0, 1)
        for p in range(2):
            e.set_data_problem(p, _problem(d, 50, 70 + p)[0])
        e.init_particles_batch(np.stack([random.PRNGKey(1), random.PRNGKey(2)]))
        k = np.array([[1, 2], [3, 4]], np.uint32)
        e.set_keys(k)
        assert np.array_equal(e.get_keys(), k)
        with pytest.raises(_lib.DibsHipError, match="key must be null"):
            e.set_state(key=np.zeros(2, np.uint32))
        with pytest.raises(_lib.DibsHipError, match="set_data_problem"):
            e.set_data(np.zeros((50, d), np.float32))
        e.run(0, 2)
        assert e.read("Z").size == 2 * M * d * d * 2 and e.read("KXX").size == 2 * M * M
    finally:
        e.close()


def _models(d, seeds, **kw):
    out = []
    for s in seeds:
        data, gm, lm = make_data(d, seed=s)
        out.append(MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, n_grad_mc_samples=32, n_acyclicity_mc_samples=8, **kw))
    return out


def test_sample_batch_equals_sequential_sample_with_callbacks():
    d, M, steps, every = 8, 4, 7, 3   # (callback_every does not divide steps: the last chunk overshoots to step 9, as in sample())
    ms = _models(d, [80, 81, 82])
    ms.append(ms[0])  # the same model twice: two seeds on one data set
    keys = [11, 12, 13, 14]
    seen_b, seen_s = [], []
    gb = sample_batch(ms, keys=keys, n_particles=M, steps=steps, callback_every=every,
                      callback=lambda dibs, t, zs: seen_b.append((id(dibs), t, zs.copy())))
    for i, (m, k) in enumerate(zip(ms, keys)):
        g = m.sample(key=random.PRNGKey(k), n_particles=M, steps=steps, callback_every=every,
                     callback=lambda dibs, t, zs: seen_s.append((id(dibs), t, zs.copy())))
        assert np.array_equal(gb[i], g), i
    # after every chunk, every problem in order (the sequential runs give them problem by problem)
    n_chunks = -(-steps // every)
    assert len(seen_b) == len(seen_s) == 4 * n_chunks
    for c in range(n_chunks):
        for i in range(4):
            ib, tb, zb = seen_b[c * 4 + i]
            is_, ts, zs = seen_s[i * n_chunks + c]
            assert ib == is_ == id(ms[i]) and tb == ts == (c + 1) * every
            assert np.array_equal(zb, zs), (c, i)


def test_batch_of_one_is_plain_sample():
    ms = _models(8, [90])
    g1 = sample_batch(ms, keys=[5], n_particles=4, steps=4)[0]
    z1 = ms[0].last_state["z"]
    g2 = ms[0].sample(key=random.PRNGKey(5), n_particles=4, steps=4)
    assert np.array_equal(g1, g2) and np.array_equal(z1, ms[0].last_state["z"])


def test_full_size_config2_batch_of_8():
    d, M = 20, 32
    kw = dict(n_vars=d, n_particles=M)
    probs = [_problem(d, 100, 200 + p) for p in range(8)]
    _check(kw, probs, list(range(8)), [(0, 200)])


def test_full_size_headline_batch_of_2():
    d, M = 50, 128
    kw = dict(n_vars=d, n_particles=M)
    probs = [_problem(d, 100, 300 + p) for p in range(2)]
    _check(kw, probs, [0, 1], [(0, 20)])
