"""By hand: komb_betweenness_run at full-size C2 (|V| = 1 M, |E| ~ 10 M, bench.py's configuration).  No reference takes that
size for the floating-point values, so only the integer outputs of 64 sources -- n_reached, sum_dist, ecc -- are compared, with
scipy's unweighted shortest paths over the library's own CSR.  It prints the device time of one 64-source batch and of 1024 sources
(best of 3), depth_max, the line of option BTW_DEBUG (the row entries the sweeps looked at and those some lane needed), and, as
a CPU anchor, the single-thread time of tests/betweenness_ref.py for 64 sources on a 20 000-vertex graph of the same generator,
on which the GPU result is also compared bit for bit.
    python tests/manual/c2_betweenness_check.py [--out FILE]      (default: profiles/betweenness_c2_check.txt)
"""
import os, re, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import komb_amd
import betweenness_ref as R

REPS = 3
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "betweenness_c2_check.txt")
if "--out" in args:
    i = args.index("--out"); out_path = args[i + 1]; del args[i:i + 2]
out = open(out_path, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n"); out.flush()


def traced_run(a, sources):
    """(ms of the run, the BTW_DEBUG line cut before its per-batch list) of one run"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            a.betweenness_run(sources)
        finally:
            os.dup2(keep, 2); os.close(keep)
        f.seek(0)
        m = re.search(rb"komb betweenness: [^\n;]*", f.read())
    return a.betweenness_info()["ms"], m.group(0).decode() if m else "(no trace)"


def bfs(rowptr, col, sources):
    """[(n_reached, sum_dist, ecc)] of the sources: scipy's unweighted shortest paths, eight sources at a time"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    n = len(rowptr) - 1
    g = csr_matrix((np.ones(len(col), np.int8), col, rowptr), shape=(n, n))
    res = []
    for i in range(0, len(sources), 8):
        d = dijkstra(g, directed=False, unweighted=True, indices=np.asarray(sources[i:i + 8], dtype=np.int64))
        for row in d:
            r = row[np.isfinite(row)].astype(np.int64)
            res.append((len(r), int(r.sum()), int(r.max())))
    return res


ok = True
rng = np.random.default_rng(1)

# ---- C2
nv = 1_000_000
uv = komb_amd.gen_hug_edges(nv, 2_450_000, 2.6, 42)
a = komb_amd.KombAccel(); a.from_edges(nv, uv); del uv
a.set_option("BTW_DEBUG", "1")
src = np.sort(rng.permutation(nv)[:1024]).astype(np.int32)
for n in (64, 1024):
    best = min((traced_run(a, src[:n]) for _ in range(REPS)), key=lambda x: x[0])
    info = a.betweenness_info()
    say("C2 nv", a.nv, "ne", a.ne, "sources", n, "ms %.3f" % best[0], "depth_max", info["depth_max"], "n_level_steps", info["n_level_steps"],
        "flags", info["flags"])
    say("C2", best[1])
a.betweenness_run(src[:64])
per = a.betweenness_fetch_sources()
bc = a.betweenness_fetch()
rowptr, col = a.get_csr()
t0 = time.time()
want = bfs(rowptr, col, src[:64])
same = ([int(x) for x in per["n_reached"]], [int(x) for x in per["sum_dist"]], [int(x) for x in per["ecc"]]) == tuple(
    [w[i] for w in want] for i in range(3))
ok = ok and same and bool(np.isfinite(bc).all()) and bool((bc >= 0).all())
say("C2: integer outputs of 64 sources against scipy's search (%.1f s): %s; bc finite and non-negative, largest %.17g" %
    (time.time() - t0, same, bc.max()))
a.close()

# ---- the CPU anchor
nv = 20_000
uv = komb_amd.gen_hug_edges(nv, 50_000, 2.6, 7)
a = komb_amd.KombAccel(); a.from_edges(nv, uv)
src = np.sort(rng.permutation(nv)[:64]).astype(np.int32)
best = min((traced_run(a, src) for _ in range(REPS)), key=lambda x: x[0])
got = a.betweenness_fetch()
rowptr, col = a.get_csr()
rows = R.rows_of_csr(rowptr.tolist(), col.tolist())
t0 = time.time()
want = R.betweenness(rows, src.tolist())
cpu = time.time() - t0
same = bool(np.array_equal(got.view(np.uint64), want["bc"].view(np.uint64)))
ok = ok and same
say("anchor nv", a.nv, "ne", a.ne, "sources 64: device %.3f ms; tests/betweenness_ref.py, one thread, %.1f s; bit-equal %s" % (best[0], cpu, same))
a.close()
say("BETWEENNESS_CHECK", "OK" if ok else "MISMATCH")
