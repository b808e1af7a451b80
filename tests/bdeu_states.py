"""Constructed discrete data sets and hard graphs for the BDeu tests (tests/test_bdeu_host.py, tests/test_gpu_bdeu.py): one table of
cases, chosen for where the device kernel can go wrong -- mask words (d = 64 / 65 / 130), key words (130 binary variables, 40 of arity
16), every field width (arities 2 .. 16), N around the wave size and at 1 024, one group / all groups distinct, every kind of parent set,
both equivalent sample sizes, and interventions down to a node without a used row."""
import numpy as np

# name: d, arities (cycled to d), N, rows ("random" / "identical" / "distinct"), interventions ("none" / "some" / "node_all"), eta
CASES = {
    "d5_n65_interv":  dict(d=5, arities=[2, 3, 4, 2, 5], N=65, rows="random", interv="some", eta=1.0),
    "d5_n1":          dict(d=5, arities=[2, 3, 4, 2, 5], N=1, rows="random", interv="none", eta=1.0),
    "d5_n2":          dict(d=5, arities=[2, 3, 4, 2, 5], N=2, rows="random", interv="none", eta=10.0),
    "d5_n63":         dict(d=5, arities=[2, 3, 4, 2, 5], N=63, rows="random", interv="none", eta=1.0),
    "d5_n64_eta10":   dict(d=5, arities=[3, 3, 3, 3, 3], N=64, rows="random", interv="none", eta=10.0),
    "d5_n130":        dict(d=5, arities=[2, 3, 4, 5, 7], N=130, rows="random", interv="some", eta=1.0),
    "d5_n1024":       dict(d=5, arities=[2, 3, 4, 5, 7], N=1024, rows="random", interv="none", eta=1.0),
    "d7_all_widths":  dict(d=7, arities=[2, 3, 4, 5, 7, 8, 16], N=130, rows="random", interv="some", eta=10.0),
    "d5_identical":   dict(d=5, arities=[2, 3, 4, 2, 5], N=64, rows="identical", interv="none", eta=1.0),
    "d5_distinct":    dict(d=5, arities=[4, 5, 7, 8, 16], N=130, rows="distinct", interv="none", eta=1.0),
    "d64":            dict(d=64, arities=[2, 3, 4], N=65, rows="random", interv="none", eta=1.0),
    "d65_node_all":   dict(d=65, arities=[2, 3, 4], N=65, rows="random", interv="node_all", eta=1.0),
    "d130_binary":    dict(d=130, arities=[2], N=63, rows="random", interv="some", eta=1.0),
    "d40_arity16":    dict(d=40, arities=[16], N=64, rows="random", interv="none", eta=10.0),
}
GRAPHS = ("empty", "one_parent", "all_others", "random")


def arities_of(case):
    c = CASES[case]
    return np.resize(np.asarray(c["arities"], np.int32), c["d"])


def make_case(case):
    """(x [N, d] float32 codes, interv_mask [N, d] int32 or None, arities [d] int32, eta)"""
    c = CASES[case]
    d, N = c["d"], c["N"]
    r = arities_of(case)
    rng = np.random.default_rng(sum(map(ord, case)))
    if c["rows"] == "identical":
        x = np.repeat(rng.integers(0, r)[None], N, axis=0)
    elif c["rows"] == "distinct":
        assert int(np.prod(r.astype(np.int64))) >= N
        x = np.zeros((N, d), np.int64)
        n = np.arange(N) * 37 % int(np.prod(r.astype(np.int64)))   # distinct numbers, their mixed-radix digits
        for i in range(d):
            x[:, i] = n % r[i]
            n = n // r[i]
        assert len({tuple(row) for row in x}) == N
    else:
        # few distinct parent configurations AND repeats: half of the rows are copies of earlier rows
        x = rng.integers(0, r, size=(N, d))
        for n in range(1, N, 2):
            x[n] = x[rng.integers(0, n)]
            col = int(rng.integers(0, d))
            x[n, col] = rng.integers(0, r[col])   # (one entry redrawn)
    mask = None
    if c["interv"] != "none":
        mask = np.zeros((N, d), np.int32)
        cols = rng.choice(d, size=max(1, d // 3), replace=False)
        for j in cols:
            mask[rng.random(N) < 0.3, j] = 1
        if c["interv"] == "node_all":
            mask[:, int(cols[0])] = 1
    return x.astype(np.float32), mask, r, c["eta"]


def make_graphs(case):
    """[4, d, d] int32 in the order of GRAPHS: no edges; the chain i -> i + 1 (one parent); every off-diagonal entry (each node has all
    others as parents -- scoring takes any hard graph); off-diagonal Bernoulli(0.5)"""
    d = CASES[case]["d"]
    rng = np.random.default_rng(1 + sum(map(ord, case)))
    off = 1 - np.eye(d, dtype=np.int32)
    chain = np.zeros((d, d), np.int32)
    chain[np.arange(d - 1), np.arange(1, d)] = 1
    return np.stack([np.zeros((d, d), np.int32), chain, off, (rng.random((d, d)) < 0.5).astype(np.int32) * off])


def decode_masks(masks, Mloc, d, S):
    """PARENT_MASKS u64 [Mloc, d, S, W] -> hard graphs [Mloc, S, d, d] (g[i, j] = bit i of node j's set)"""
    W = (d + 63) // 64
    m = np.asarray(masks, np.uint64).reshape(Mloc, d, S, W)
    g = np.zeros((Mloc, S, d, d), np.int32)
    for i in range(d):
        bit = (m[:, :, :, i >> 6] >> np.uint64(i & 63)) & np.uint64(1)     # [Mloc, d(j), S]
        g[:, :, i, :] = bit.transpose(0, 2, 1)
    return g
