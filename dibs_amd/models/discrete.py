"""Discrete (categorical) data: the BDeu marginal likelihood (Heckerman, Geiger & Chickering 1995).

``bdeu_log_marginal_numpy`` is the definition in float64 numpy (include/dibs_hip.h, BDEU): what the device
kernel k_bdeu_nodes is tested against, as ``kernel.median_bandwidth`` is for the bandwidth rule.  ``BDeu`` is the likelihood class
``MarginalDiBS`` lowers to the device."""
import math

import numpy as np


def _arities(arities, n_vars):
    a = np.asarray(arities)
    if a.ndim == 0:
        a = np.full(n_vars, int(a))
    if a.shape != (n_vars,):
        raise ValueError(f"arities must be an int or a sequence of length n_vars = {n_vars}, got shape {a.shape}")
    if not np.all(a == np.floor(a)):
        raise ValueError("arities must be integers")
    return a.astype(np.int64)


def _rise_terms(log_alpha, n):
    """the n terms of rise(log alpha, n) = lgamma(alpha + n) - lgamma(alpha) for integer n >= 0, from log alpha: log alpha itself, then
    log(alpha + i), i = 1 .. n - 1.  alpha itself may underflow (hundreds of parents), which the terms i >= 1 absorb."""
    if n == 0:
        return np.zeros(0, np.float64)
    i = np.arange(1, n, dtype=np.float64)
    return np.concatenate([[float(log_alpha)], np.log(np.exp(log_alpha) + i)])


def bdeu_log_marginal_numpy(g, x, arities, interv_mask=None, equivalent_sample_size=1.0, per_node=False):
    """log p(D | G) under the BDeu score, float64.  ``g [d, d]`` (``g[i, j]`` = edge i -> j), ``x [N, d]`` category codes, variable i in
    ``0 .. arities[i] - 1``; node j uses the rows with ``interv_mask[n, j] == 0`` (a parent's value counts in every such row).
    ``per_node``: the d node scores instead of their sum."""
    g = np.asarray(g)
    x = np.asarray(x)
    n_obs, d = x.shape
    r = _arities(arities, d)
    codes = x.astype(np.int64)
    used_all = np.ones((n_obs, d), bool) if interv_mask is None else np.asarray(interv_mask) == 0
    log_r = np.log(r.astype(np.float64))
    log_eta = np.log(float(equivalent_sample_size))
    out = np.zeros(d, np.float64)
    for j in range(d):
        rows = np.nonzero(used_all[:, j])[0]
        if rows.size == 0:
            continue
        pa = [i for i in range(d) if i != j and g[i, j] != 0]
        log_a = log_eta - float(np.sum(log_r[pa]))
        log_a1 = log_a - log_r[j]
        # configurations in the order of their first used row, each with its child-value counts
        first, counts = {}, []
        for n in rows:
            c = tuple(codes[n, pa])
            if c not in first:
                first[c] = len(counts)
                counts.append(np.zeros(r[j], np.int64))
            counts[first[c]][codes[n, j]] += 1
        # one exactly rounded sum over the terms of every rise of the node: a node with few, large groups is a small difference of sums
        # near N log N, and adding rise by rise would leave the rounding of those (an ulp of 3.6e-12 at N = 4 096) in the result
        terms = []
        for n_ck in counts:
            terms.append(-_rise_terms(log_a, int(n_ck.sum())))
            terms.extend(_rise_terms(log_a1, int(v)) for v in n_ck)
        out[j] = math.fsum(np.concatenate(terms))
    return out if per_node else float(out.sum())


class BDeu:
    """BDeu marginal likelihood of categorical data: ``arities`` (an int, or one per variable) values per variable, coded 0 .. r - 1;
    ``equivalent_sample_size`` the prior's weight."""
    _dibs_likelihood = "bdeu"

    def __init__(self, *, n_vars, arities, equivalent_sample_size=1.0):
        self.n_vars = n_vars
        self.arities = _arities(arities, n_vars).astype(np.int32)
        if np.any(self.arities < 2):
            raise ValueError("arities must be >= 2")
        if not equivalent_sample_size > 0:
            raise ValueError("equivalent_sample_size must be > 0")
        self.equivalent_sample_size = float(equivalent_sample_size)
        self.no_interv_targets = np.zeros(self.n_vars, bool)

    def get_theta_shape(self, *, n_vars):
        raise NotImplementedError("Not available for the BDeu score: a marginal likelihood has no parameters.")

    def sample_parameters(self, *, key, n_vars, n_particles=0, batch_size=0):
        raise NotImplementedError("Not available for the BDeu score: a marginal likelihood has no parameters.")

    def sample_obs(self, *, key, n_samples, g, theta, toporder=None, interv=None):
        raise NotImplementedError("Not available for the BDeu score; `target.make_discrete_model` samples discrete data.")

    def _config_kwargs(self):
        return dict(likelihood="bdeu", bdeu_ess=self.equivalent_sample_size)

    def check_data(self, x):
        """ValueError naming the first column (and its first value) that is not integral or outside 0 .. arity - 1"""
        x = np.asarray(x)
        if x.ndim != 2 or x.shape[1] != self.n_vars:
            raise ValueError(f"x must have shape [N, {self.n_vars}], got {x.shape}")
        for i in range(self.n_vars):
            col = x[:, i]
            bad = ~((col >= 0) & (col < self.arities[i]) & (col == np.floor(col)))
            if bad.any():
                n = int(np.argmax(bad))
                raise ValueError(f"BDeu: column {i} of x holds {col[n]!r} (row {n}), which is not a category code of a variable of arity "
                                 f"{int(self.arities[i])} (integers 0 .. {int(self.arities[i]) - 1})")

    def interventional_log_marginal_prob(self, g, _, x, interv_targets, rng=None):
        """log p(D | G) of one hard graph, evaluated on the device."""
        from ..inference.scoring import score_graphs
        return float(score_graphs(self, np.asarray(g)[None], None, x, interv_targets)[0])

    def log_marginal_likelihood(self, *, g, x, interv_targets):
        return self.interventional_log_marginal_prob(g, None, x, interv_targets)
