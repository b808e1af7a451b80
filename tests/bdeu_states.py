"""Constructed discrete data sets and hard graphs for the BDeu tests (tests/test_bdeu_host.py, tests/test_gpu_bdeu.py): one table of
cases, chosen for where the device kernel can go wrong -- mask words (d = 64 / 65 / 130), key words (130 binary variables, 40 of arity
16), every field width (arities 2 .. 16), N around the wave size and at 1 024, one group / all groups distinct, every kind of parent set,
both equivalent sample sizes, and interventions down to a node without a used row; then every launch shape of k_bdeu_nodes (PLAN_TIERS:
the (waves per block, rows in LDS) pairs and table sizes bdeu_plan picks between N = 150 and the limit of 4 096 --
tests/test_bdeu_host.py asserts that the cases cover them all), the largest group and the fullest table, the largest row layout (8 words),
and parents whose fields are the top bits of a word with as many configurations as rows."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: d, arities (cycled to d), N, rows ("random" / "identical" / "distinct" / "high_digits"), interventions ("none" / "some" /
# "node_all"), eta; optionally graphs: the names of the case's own graph tuple (make_graphs; GRAPHS otherwise)
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
# one case per launch shape: (waves, rows in LDS, T) of bdeu_plan(N, 1) beside each N
PLAN_TIERS = {150: (4, 0, 512), 220: (2, 0, 512), 300: (2, 0, 1024), 400: (1, 0, 1024), 500: (4, 1, 1024), 600: (1, 0, 2048),
              1025: (2, 1, 4096), 2048: (2, 0, 4096), 2049: (1, 1, 8192), 4096: (1, 0, 8192)}
for _n in PLAN_TIERS:
    CASES[f"d5_n{_n}"] = dict(d=5, arities=[2, 3, 4, 5, 7], N=_n, rows="random", interv="some" if _n == 2049 else "none", eta=1.0)
TIER_CASES = tuple(f"d5_n{_n}" for _n in PLAN_TIERS)
HIGH_BIT_GRAPHS = ("node0_parents_24_29", "node29_parents_23_28", "node12_parents_0_5", "all_parent_29")
CASES.update({
    # one group of 4 096 rows: the last entry of the rise table, across all 64 chunks of its scan
    "d5_identical_n4096": dict(d=5, arities=[2, 3, 4, 5, 7], N=4096, rows="identical", interv="none", eta=1.0),
    # 2 048 groups in 4 096 slots: load factor exactly 1/2 in both passes
    "d5_distinct_n2048":  dict(d=5, arities=[4, 5, 7, 8, 16], N=2048, rows="distinct", interv="none", eta=1.0),
    # 512 field bits: 8 key words, the largest layout
    "d128_arity16_kw8":   dict(d=128, arities=[16], N=72, rows="random", interv="none", eta=1.0),
    # 3 key words, rows read from global memory by 2 waves per block
    "d40_arity16_n1400":  dict(d=40, arities=[16], N=1400, rows="random", interv="none", eta=1.0),
    # bits 48 .. 59 of the only key word take 1 024 distinct values (columns 24 .. 29: the base-4 digits of a permutation of the rows)
    "d30_high_bits":      dict(d=30, arities=[4], N=1024, rows="high_digits", interv="none", eta=1.0, graphs=HIGH_BIT_GRAPHS),
})
GRAPHS = ("empty", "one_parent", "all_others", "random")


def graph_names(case):
    return CASES[case].get("graphs", GRAPHS)


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
    elif c["rows"] == "high_digits":
        assert d == 30 and all(r == 4) and N <= 4 ** 6
        x = rng.integers(0, r, size=(N, d))
        n = rng.permutation(N)
        for i in range(24, 30):
            x[:, i] = n % 4
            n = n // 4
        assert len({tuple(row) for row in x[:, 24:30]}) == N
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
    others as parents -- scoring takes any hard graph); off-diagonal Bernoulli(0.5).  A case with its own tuple (graph_names): the
    high-bit case's four graphs -- node 0 with parents 24 .. 29 (as many configurations as rows, all in the word's top bits), node 29 with
    parents 23 .. 28, node 12 with parents 0 .. 5 (the low-bit control), every node with the single parent 29"""
    d = CASES[case]["d"]
    if graph_names(case) is HIGH_BIT_GRAPHS:
        g = np.zeros((4, d, d), np.int32)
        g[0, 24:30, 0] = 1
        g[1, 23:29, 29] = 1
        g[2, 0:6, 12] = 1
        g[3, 29, :29] = 1
        return g
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


def build_score_check(td):
    """tests/tools/bdeu_score_check.cpp compiled into the directory `td`; the executable's path"""
    src = os.path.join(ROOT, "tests", "tools", "bdeu_score_check.cpp")
    exe = os.path.join(td, "bdeu_score_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", src, "-o", exe], check=True)
    return exe


def plan_of(exe, N, KW):
    """(waves, rows_lds, T, lds_bytes) of bdeu_plan(N, KW), from the header itself"""
    r = subprocess.run([exe, "--plan", str(N), str(KW)], capture_output=True, text=True, check=True)
    waves, rows_lds, T, lds = map(int, r.stdout.split())
    return waves, rows_lds, T, lds


def key_words(arities):
    """bdeu_layout's word count: fields of ceil(log2 r) bits in variable order, none straddling a 64-bit word"""
    word, used = 0, 0
    for r in arities:
        b = max(1, int(r - 1).bit_length())
        if used + b > 64:
            word, used = word + 1, 0
        used += b
    return word + 1
