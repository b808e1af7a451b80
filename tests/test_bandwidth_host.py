"""Host-side checks of the median-heuristic kernel bandwidth (include/dibs_hip.h, MEDIAN-HEURISTIC KERNEL BANDWIDTH; DESIGN.md section
10.6): the documented reference ``dibs_amd.kernel.median_bandwidth`` against a brute-force sort, the config bits and the kernel classes,
every refusal of dibs_engine_create (before any device call, so these run without a GPU), the rule mismatch of the multi-run entry
points, and the plain-C++ header the selection kernel shares with the host (tests/tools/bandwidth_select_check.cpp)."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import make_data
from dibs_amd._abi import make_config
from dibs_amd.inference import JointDiBS, MarginalDiBS, sample_batch, sample_joint_batch, sample_joint_sweep, sample_sweep
from dibs_amd.kernel import AdditiveFrobeniusSEKernel, JointAdditiveFrobeniusSEKernel, median_bandwidth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MIN = np.finfo(np.float32).tiny


def brute(x):
    """the rule, pair by pair in Python: float64 sums, float32 values, np.sort, the two middle order statistics"""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    M = len(x)
    v = np.sort(np.array([np.float32(((x[a] - x[b]) ** 2).sum()) for a in range(M) for b in range(a + 1, M)], np.float32))
    P = len(v)
    assert P == M * (M - 1) // 2
    med = v[(P - 1) // 2] if P % 2 else np.float32(np.float32(0.5) * np.float32(v[P // 2 - 1] + v[P // 2]))
    h = np.float32(np.float64(med) * (1.0 / math.log(M + 1)))
    return np.float32(max(h, FLT_MIN))


@pytest.mark.parametrize("M", [2, 3, 4, 5, 33])   # P = 1, 3, 6, 10, 528: one pair, both parities
def test_median_bandwidth_equals_brute_force(M):
    rng = np.random.default_rng(M)
    x = rng.normal(size=(M, 4, 3, 2))
    h = median_bandwidth(x)
    assert h.dtype == np.float32 and h.shape == ()
    assert h == brute(x)
    assert median_bandwidth(x.reshape(M, -1)) == h   # (trailing axes are one particle, flattened)


def test_median_bandwidth_ties_duplicates_and_batch():
    rng = np.random.default_rng(0)
    lattice = rng.integers(-2, 3, size=(9, 6)).astype(np.float64)   # small integers: exact distances, many ties
    assert median_bandwidth(lattice) == brute(lattice)
    dup = np.repeat(rng.normal(size=(1, 5)), 6, axis=0)
    dup[0] += 1.0                                                  # 10 of 15 pairs identical: med = 0
    assert median_bandwidth(dup) == FLT_MIN == brute(dup)
    two = np.array([[0.0, 0.0], [3.0, 4.0]])
    assert median_bandwidth(two) == np.float32(25.0 / math.log(3.0))
    xs = rng.normal(size=(2, 3, 5, 7))                             # leading batch shape [2, 3], M = 5
    hb = median_bandwidth(xs, batch_dims=2)
    assert hb.shape == (2, 3) and hb.dtype == np.float32
    for i in range(2):
        for j in range(3):
            assert hb[i, j] == brute(xs[i, j])
    with pytest.raises(ValueError, match="two particles"):
        median_bandwidth(np.zeros((1, 4)))


def test_config_bits_and_defaults():
    base = dict(n_vars=5, n_particles=4, n_observations=10)
    assert list(make_config(**base).reserved_i) == [1, 0, 0, 0, 0]
    assert list(make_config(joint=True, likelihood="lingauss", **base).reserved_i) == [1, 0, 0, 0, 0]
    assert make_config(h_latent="median", **base).reserved_i[3] == 1
    c = make_config(joint=True, likelihood="lingauss", h_theta="median", **base)
    assert c.reserved_i[3] == 2 and c.h_latent == 5.0
    assert make_config(joint=True, likelihood="lingauss", h_latent="median", h_theta="median", **base).reserved_i[3] == 3
    with pytest.raises(ValueError, match="median"):
        make_config(h_latent="mean", **base)


def test_kernel_classes():
    assert AdditiveFrobeniusSEKernel(h="median").h == "median"
    k = JointAdditiveFrobeniusSEKernel(h_theta="median")
    assert k.h_theta == "median" and k.h_latent == 5.0
    assert JointAdditiveFrobeniusSEKernel(h_latent="median").h_theta == 500.0
    for bad in (lambda: AdditiveFrobeniusSEKernel(h="auto"), lambda: JointAdditiveFrobeniusSEKernel(h_latent="med"),
                lambda: JointAdditiveFrobeniusSEKernel(h_theta="")):
        with pytest.raises(ValueError, match="median"):
            bad()
    x = np.zeros((3, 3, 2))
    with pytest.raises(ValueError, match="median_bandwidth"):
        AdditiveFrobeniusSEKernel(h="median").eval(x=x, y=x)
    with pytest.raises(ValueError, match="median_bandwidth"):
        JointAdditiveFrobeniusSEKernel(h_theta="median").eval(x_latent=x, x_theta=x, y_latent=x, y_theta=x)
    assert AdditiveFrobeniusSEKernel(h=2.0).eval(x=x, y=x) == 1.0   # (fixed bandwidths: as before)


def test_models_lower_the_rule():
    data, gm, lm = make_data(5)
    m = MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, kernel_param={"h": "median"})
    assert m._make_config(4, 5).reserved_i[3] == 1
    assert MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm)._make_config(4, 5).reserved_i[3] == 0
    dj, gj, lj = make_data(5, joint=True)
    for kp, rule in (({"h_latent": "median"}, 1), ({"h_theta": "median"}, 2), ({"h_latent": "median", "h_theta": "median"}, 3)):
        assert JointDiBS(x=dj.x, graph_model=gj, likelihood_model=lj, kernel_param=kp)._make_config(4, 5).reserved_i[3] == rule
    with pytest.raises(ValueError, match="median"):
        MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, kernel_param={"h": "auto"})


@pytest.mark.parametrize("kw,msg", [
    (dict(n_particles=256), "n_particles \\(per run\\) must be < 256.*follow-up"),
    (dict(n_particles=1024), "n_particles \\(per run\\) must be < 256"),
    (dict(n_particles=1), "n_particles must be >= 2"),
    (dict(n_particles=4, n_ranks=2), "n_ranks must be 1"),
    (dict(precision=64), "float64 engine is not supported"),
    (dict(h_theta="median"), "needs a joint model"),
    (dict(n_problems=3, n_particles=256), "n_particles \\(per run\\) must be < 256"),
    (dict(joint=True, likelihood="lingauss", n_chains=3, n_particles=300, h_theta="median"), "n_particles \\(per run\\) must be < 256"),
])
def test_engine_create_refusals(kw, msg):
    from dibs_amd import _lib
    from dibs_amd.engine import Engine
    args = dict(n_vars=8, n_particles=8, n_observations=20, h_latent="median")
    args.update(kw)
    with pytest.raises(_lib.DibsHipError, match="^median bandwidth: .*" + msg):
        Engine(make_config(**args))


def test_engine_create_refuses_a_rule_out_of_range():
    from dibs_amd import _lib
    from dibs_amd.engine import Engine
    for rule in (4, -1):
        c = make_config(n_vars=8, n_particles=8, n_observations=20)
        c.reserved_i[3] = rule
        with pytest.raises(_lib.DibsHipError, match="^median bandwidth: .*must be 0 .. 3"):
            Engine(c)


def _marginal(d=5, **kp):
    data, gm, lm = make_data(d)
    return MarginalDiBS(x=data.x, graph_model=gm, likelihood_model=lm, kernel_param=kp or None)


def _joint(d=5, **kp):
    data, gm, lm = make_data(d, joint=True)
    return JointDiBS(x=data.x, graph_model=gm, likelihood_model=lm, kernel_param=kp or None)


def test_multirun_rule_mismatch_is_a_value_error():
    kw = dict(keys=[1, 2], n_particles=4, steps=2)
    for f in (sample_batch, sample_sweep):
        with pytest.raises(ValueError, match=f"{f.__name__}: model 1 differs from model 0 in .*kernel bandwidth rule"):
            f([_marginal(h="median"), _marginal(h=5.0)], **kw)
    for f in (sample_joint_batch, sample_joint_sweep):
        with pytest.raises(ValueError, match=f"{f.__name__}: model 1 differs from model 0 in .*kernel bandwidth rule"):
            f([_joint(h_latent="median", h_theta=500.0), _joint(h_latent=5.0, h_theta="median")], **kw)
        with pytest.raises(ValueError, match="kernel bandwidth rule"):
            f([_joint(), _joint(h_latent="median", h_theta="median")], **kw)


def test_bandwidth_select_header_against_sort_and_plan_invariants():
    src = os.path.join(ROOT, "tests", "tools", "bandwidth_select_check.cpp")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "bandwidth_select_check")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", src, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert "bandwidth_select_check: ok" in r.stdout
