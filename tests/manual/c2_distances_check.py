"""By hand: komb_distances_run at full-size C2 (|V| = 1 M, |E| ~ 10 M, bench.py's configuration), one process.  For the 64 and the
1024 sources of profiles/betweenness_c2_check.txt and each DIST_WORDS in 1, 2, 4 it prints the device time (HIP events,
komb_distances_info's ms; best of 3), the line of option DIST_DEBUG and the share of row entries the early exit skipped; it
compares the per-source integers with komb_betweenness_fetch_sources on the same sources, the per-vertex sums with the
per-source sums, and all outputs between the three widths; then it times 64 batches of the default width from the first vertices
and, when the extrapolation to every vertex stays under LIMIT_S seconds, runs every vertex once.
    python tests/manual/c2_distances_check.py [--out FILE]      (default: profiles/distances_c2_check.txt)
"""
import os, re, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import komb_amd

REPS = 3
LIMIT_S = 150.0
DEFAULT_WORDS = 4
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "distances_c2_check.txt")
if "--out" in args:
    i = args.index("--out"); out_path = args[i + 1]; del args[i:i + 2]
out = open(out_path, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n"); out.flush()


def traced_run(a, sources):
    """(ms of the run, the DIST_DEBUG line) of one run"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            a.distances_run(sources)
        finally:
            os.dup2(keep, 2); os.close(keep)
        f.seek(0)
        m = re.search(rb"komb distances: [^\n]*", f.read())
    return a.distances_info()["ms"], m.group(0).decode() if m else "(no trace)"


def skipped(line):
    m = re.search(r"(\d+) of (\d+) row entries", line)
    return 1.0 - int(m.group(1)) / max(int(m.group(2)), 1) if m else float("nan")


ok = True
rng = np.random.default_rng(1)
nv = 1_000_000
uv = komb_amd.gen_hug_edges(nv, 2_450_000, 2.6, 42)
a = komb_amd.KombAccel(); a.from_edges(nv, uv); del uv
a.set_option("DIST_DEBUG", "1")
src = np.sort(rng.permutation(nv)[:1024]).astype(np.int32)                 # the sources of c2_betweenness_check.py
a.distances_run(src[:64])                                                  # (warm-up: the first launches load the code)

results = {}
for n in (64, 1024):
    for words in (1, 2, 4):
        a.set_option("DIST_WORDS", str(words))
        best = min((traced_run(a, src[:n]) for _ in range(REPS)), key=lambda x: x[0])
        info = a.distances_info()
        say("C2 nv", a.nv, "ne", a.ne, "sources", n, "words", words, "ms %.3f" % best[0], "depth_max", info["depth_max"], "n_batches",
            info["n_batches"], "n_level_steps", info["n_level_steps"], "early exit skipped %.1f %% of the row entries" % (100 * skipped(best[1])))
        say("C2", best[1])
        results[(n, words)] = (a.distances_fetch(), a.distances_fetch_sources(), a.distances_histogram())
    first = results[(n, 1)]
    same = all(np.array_equal(first[0][k].view(np.uint64) if k == "harmonic" else first[0][k],
                              results[(n, w)][0][k].view(np.uint64) if k == "harmonic" else results[(n, w)][0][k])
               for w in (2, 4) for k in first[0])
    same = same and all(np.array_equal(first[1][k], results[(n, w)][1][k]) for w in (2, 4) for k in first[1])
    same = same and all(np.array_equal(first[2], results[(n, w)][2]) for w in (2, 4))
    a.betweenness_run(src[:n])
    per = a.betweenness_fetch_sources()
    btw = all(np.array_equal(first[1][k], per[k]) for k in per)
    views = int(first[0]["n_reached"].sum()) == int(first[1]["n_reached"].sum()) == int(first[2].sum()) and \
        int(first[0]["sum_dist"].sum()) == int(first[1]["sum_dist"].sum())
    ok = ok and same and btw and views
    say("C2 sources", n, ": outputs identical for 1, 2 and 4 words (harmonic bit for bit):", same, "; per-source integers equal to "
        "komb_betweenness_fetch_sources (%.3f ms there):" % a.betweenness_info()["ms"], btw, "; per-vertex sums equal the per-source sums "
        "and the histogram:", views, "; largest harmonic %.17g" % first[0]["harmonic"].max())
results.clear()

# ---- every vertex as a source
a.set_option("DIST_WORDS", str(DEFAULT_WORDS))
per = 64 * DEFAULT_WORDS
ms, line = traced_run(a, np.arange(64 * per, dtype=np.int32))
total = -(-nv // per)
guess = ms * total / 64 / 1000.0
say("C2 first %d vertices as sources (64 batches of %d words): %.3f ms; EXTRAPOLATED to all %d batches: %.1f s" % (64 * per, DEFAULT_WORDS, ms, total, guess))
if guess <= LIMIT_S:
    t0 = time.time()
    ms, line = traced_run(a, None)
    info = a.distances_info()
    vert, persrc = a.distances_fetch(), a.distances_fetch_sources()
    sym = all(np.array_equal(vert[k], persrc[k]) for k in ("n_reached", "sum_dist", "ecc"))
    ok = ok and sym and info["flags"] == komb_amd._lib.KOMB_DISTANCES_ALL
    say("C2 every vertex: MEASURED device %.1f s (host %.1f s)," % (ms / 1000.0, time.time() - t0), "depth_max (diameter)", info["depth_max"],
        "depth_min (radius)", info["depth_min"], "n_pairs", info["n_pairs"], "sum_all", info["sum_all"], "n_level_steps", info["n_level_steps"],
        "; the per-vertex view equals the per-source view:", sym)
    say("C2", line)
    say("C2 hop plot:", a.distances_histogram().tolist())
else:
    say("C2 every vertex: not run (the extrapolation is over the checker's limit of %.0f s)" % LIMIT_S)
a.close()
say("DISTANCES_CHECK", "OK" if ok else "MISMATCH")
