"""By hand: komb_biconnected_run at full size (C3: |V| = 10 M, |E| = 100 M; --size c2: |V| = 1 M, |E| = 10 M), k = 2 on the
whole-graph k-truss result.  It asserts the invariants of the block-cut forest from the library's outputs alone, confirms on
sampled vertices and edges with scipy's connected_components that deleting a reported articulation point / bridge raises
the number of components and that deleting one that is not reported does not, and prints depth and the device time: one
warm-up run, then --runs runs, beside komb_components_run(KOMB_COMP_TRUSS, 2) on the same result (one link pass over the
same edges) and the ratio of the two.
    python tests/manual/c3_biconnected_check.py [--size c2|c3] [--runs N] [--samples N] [--out FILE]
(default: c3, 5 runs, 100 samples of each of the four kinds, profiles/biconnected_<size>_check.txt; a sample costs one
connected_components over the whole graph, about 1 s at C2 and 15 s at C3)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

import komb_amd

SIZES = {"c2": (1_000_000, 2_425_000), "c3": (10_000_000, 24_250_000)}
args = sys.argv[1:]


def opt(name, default):
    if name in args:
        i = args.index(name); v = args[i + 1]; del args[i:i + 2]
        return v
    return default


size = opt("--size", "c3")
runs, samples = int(opt("--runs", 5)), int(opt("--samples", 100))
out = open(opt("--out", os.path.join(ROOT, "profiles", f"biconnected_{size}_check.txt")), "w")
NV, N_CLIQUES = SIZES[size]
NAME = size.upper()


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n"); out.flush()


def n_components(nv, eu, ev, keep_e=None, without_v=None):
    """Components among the vertices that are left."""
    sel = np.ones(len(eu), bool) if keep_e is None else keep_e
    if without_v is not None:
        sel = sel & (eu != without_v) & (ev != without_v)
    n, _ = connected_components(csr_matrix((np.ones(int(sel.sum()), np.int8), (eu[sel], ev[sel])), shape=(nv, nv)), directed=False)
    return n - (1 if without_v is not None else 0)           # (the deleted vertex stays behind as a component of its own)


t0 = time.time()
uv = komb_amd.gen_hug_edges(NV, N_CLIQUES, 2.6, 42)
with komb_amd.KombAccel() as a:
    a.from_edges(NV, uv)
    del uv
    eu, ev, tr = a.run_truss()
    say(f"{NAME}: |V| = {NV}, |E| = {len(eu)}, t_max = {int(tr.max())} (generated, built and peeled in {time.time() - t0:.1f} s)")
    a.biconnected_run(2)                                    # (the first run of a process pays for the code object's load)
    a.components_run("truss", 2)
    ms_b, ms_c = [], []
    for _ in range(runs):
        a.biconnected_run(2)
        ms_b.append(a.biconnected_info()["ms"])
        a.components_run("truss", 2)
        ms_c.append(a.components_info()["ms"])
    info = a.biconnected_info()
    n_comp = a.components_info()["n_components"]
    say(f"{NAME} k = 2: " + ", ".join(f"{k} {v}" for k, v in info.items() if k != "ms"))
    say(f"{NAME} k = 2: depth {info['depth']}; komb_biconnected_run {min(ms_b):.2f} .. {max(ms_b):.2f} ms over {runs} runs, "
        f"komb_components_run(truss, 2) {min(ms_c):.2f} .. {max(ms_c):.2f} ms, ratio of the medians {np.median(ms_b) / np.median(ms_c):.1f}")
    block, bsize = a.biconnected_fetch_edges()
    nb, ecc_label, ecc_size = a.biconnected_fetch_vertices()
    blocks = a.biconnected_fetch_blocks()

# ---- the invariants (the block-cut structure is a forest)
nb64 = nb.astype(np.int64)
assert int(nb64[nb64 >= 2].sum()) == info["n_blocks"] + info["n_articulation"] - n_comp
assert int(blocks["n_edges"].astype(np.int64).sum()) == info["n_member_edges"] == len(eu)
assert int(blocks["n_verts"].astype(np.int64).sum()) == int(nb64.sum())
assert info["n_bridges"] == int((blocks["n_edges"] == 1).sum()) == int((bsize == 1).sum())
assert np.array_equal(block[blocks["rep"]], blocks["rep"]) and len(blocks["rep"]) == info["n_blocks"]
assert info["n_articulation"] == int((nb >= 2).sum()) and info["n_member_vertices"] == int((nb >= 1).sum())
assert np.array_equal(ecc_label[ecc_label[ecc_label >= 0]], ecc_label[ecc_label >= 0])
say(f"{NAME}: the invariants hold ({n_comp} components, {info['n_blocks']} blocks, {info['n_articulation']} articulation points, "
    f"{info['n_bridges']} bridges, {info['n_ecc']} 2-edge-connected components)")

# ---- sampled deletions against scipy
rng = np.random.default_rng(1)
base = n_components(NV, eu, ev)
kinds = (("articulation point", np.flatnonzero(nb >= 2), True, True), ("other member vertex", np.flatnonzero(nb == 1), True, False),
         ("bridge", np.flatnonzero(bsize == 1), False, True), ("other edge", np.flatnonzero(bsize > 1), False, False))
for what, pool, is_vertex, raises in kinds:
    pick = rng.choice(pool, min(samples, len(pool)), replace=False)
    t1 = time.time()
    for x in pick.tolist():
        if is_vertex:
            n = n_components(NV, eu, ev, without_v=x)
        else:
            keep = np.ones(len(eu), bool); keep[x] = False
            n = n_components(NV, eu, ev, keep_e=keep)
        assert (n > base) == raises, (what, x, n, base)
    say(f"{NAME}: {len(pick)} sampled deletions of a(n) {what}: the component count {'rises' if raises else 'stays'} every time "
        f"({time.time() - t1:.0f} s)")
