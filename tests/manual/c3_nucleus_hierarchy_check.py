"""By hand: komb_nucleus_hierarchy_run at full-size C2 (|V| = 1 M) and C3 (|V| = 10 M, |E| ~ 100 M), bench.py's configurations,
on the nucleus decomposition of the whole-graph k-truss result.  It records the nodes, the roots, the depth and the device time
of the run, best of 5, beside its yardsticks: the device time of komb_nucleus_run and of its 4-clique pass alone (option
NUC_DEBUG) on the same graph in the same process, best of 3.  Every output -- the node arrays, node[], info, and the labels and
the nuclei of a few thresholds -- is compared with tests/nucleus_hierarchy_ref.py where that finishes: on the k-truss result
induced by a seeded vertex sample (C2: 200 000 vertices, C3: 1 000 000; --sample N for both), and, after all measurements, on the
WHOLE result of C2 (plain Python over 9.7 M triangles: minutes and gigabytes, both recorded; --full adds C3's, --no-full skips
C2's).
    python tests/manual/c3_nucleus_hierarchy_check.py [C2|C3 ...] [--sample N] [--full|--no-full] [--out FILE]
                                                                      (default: profiles/nucleus_hierarchy_c2_c3_check.txt)
"""
import os, re, resource, sys, tempfile, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import komb_amd
import nucleus_hierarchy_ref as R

CONFIGS = {"C2": (1_000_000, 2_450_000), "C3": (10_000_000, 24_250_000)}
SAMPLE = {"C2": 200_000, "C3": 1_000_000}                  # vertices of the sampled comparison
WHOLE = {"C2"}                                              # whole-result comparison by default
REPS = 5
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "nucleus_hierarchy_c2_c3_check.txt")
sample_n = None
if "--out" in args:
    i = args.index("--out"); out_path = args[i + 1]; del args[i:i + 2]
if "--sample" in args:
    i = args.index("--sample"); sample_n = int(args[i + 1]); del args[i:i + 2]
if "--full" in args:
    args.remove("--full"); WHOLE = set(CONFIGS)
if "--no-full" in args:
    args.remove("--no-full"); WHOLE = set()
out = open(out_path, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n"); out.flush()


def traced_nucleus_run(a):
    """komb_nucleus_run with the library's stderr trace caught: the trace line's times by name."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            a.nucleus_run()
        finally:
            os.dup2(keep, 2); os.close(keep)
        f.seek(0)
        text = f.read().decode(errors="replace")
    return {k: float(v) for k, v in re.findall(r"(run|triangle pass|clique pass|peel) ([0-9.]+) ms", text)}


def compare(a, nv, vmask, what):
    eu, ev, _ = a.run_truss(vmask)
    a.nucleus_run()
    a.nucleus_hierarchy_run()
    theta = a.nucleus_fetch()["theta"]
    t = time.time()
    done = threading.Event()

    def beat():                                             # (stdout only: a long reference stays visibly alive)
        while not done.wait(60.0):
            print(f"  ... reference of {what}: {time.time() - t:.0f} s", flush=True)
    threading.Thread(target=beat, daemon=True).start()
    try:
        h, dec = R.hierarchy(nv, eu, ev, theta)
    finally:
        done.set()
    nodes, node, info = a.nucleus_hierarchy_fetch_nodes(), a.nucleus_hierarchy_fetch_triangles(), a.nucleus_hierarchy_info()
    same = all(np.array_equal(nodes[k], h[k]) for k in R.FIELDS) and np.array_equal(node, h["node"])
    same = same and tuple(info[k] for k in ("n_nodes", "n_roots", "theta_max", "depth", "n_member_triangles")) == R.info(h, theta)
    top = max(info["theta_max"], 1)
    for k in sorted({1, 2, (top + 1) // 2, top, -1}):
        label, size = a.nucleus_hierarchy_labels(k)
        wl, ws = R.walk_up(h, theta, k)
        got, want = a.nucleus_hierarchy_nuclei(k), R.nuclei(h, dec, k)
        same = same and np.array_equal(label, wl) and np.array_equal(size, ws) and all(np.array_equal(got[f], want[f]) for f in R.NUCLEI_FIELDS)
    say(f"{what}: edges {len(eu)} triangles {len(theta)} cliques {dec['info']['n_cliques4']} nodes {info['n_nodes']} roots {info['n_roots']} "
        f"depth {info['depth']} members {info['n_member_triangles']}; reference {time.time() - t:.1f} s, "
        f"peak memory {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20:.1f} GB; equal: {bool(same)}")
    return same


def load(name):
    nv, ncl = CONFIGS[name]
    uv = komb_amd.gen_hug_edges(nv, ncl, 2.6, 42)
    a = komb_amd.KombAccel(); a.from_edges(nv, uv); del uv
    a.set_option("NUC_DEBUG", "1")
    return nv, a


ok = True
names = args or ["C2", "C3"]
for name in names:
    nv, a = load(name)
    a.truss_run()
    nuc = None
    for _ in range(3):                                      # the yardsticks: komb_nucleus_run and its clique pass, best of 3
        times = traced_nucleus_run(a)
        nuc = times if nuc is None else {k: min(nuc[k], times[k]) for k in times}
    ni = a.nucleus_info()
    best = None
    for _ in range(REPS):
        a.nucleus_hierarchy_run()
        ms = a.nucleus_hierarchy_info()["ms"]
        best = ms if best is None else min(best, ms)
    info = a.nucleus_hierarchy_info()
    say(name, "nv", a.nv, "ne", a.ne, "triangles", ni["n_triangles"], "cliques", ni["n_cliques4"], "theta_max", ni["theta_max"])
    say(f"{name}: nodes {info['n_nodes']} roots {info['n_roots']} depth {info['depth']} members {info['n_member_triangles']}")
    say(f"{name}: hierarchy run {best:.3f} ms; komb_nucleus_run {nuc['run']:.3f} ms (clique pass {nuc['clique pass']:.3f} ms); "
        f"hierarchy / nucleus run = {best / nuc['run']:.2f}, hierarchy / clique pass = {best / nuc['clique pass']:.2f}")
    t = time.time()
    per_k = {k: a.nucleus_hierarchy_nuclei(k) for k in (1, -1)}
    say(f"{name}: nuclei at k = 1: {len(per_k[1]['rep'])}, at theta_max: {len(per_k[-1]['rep'])} "
        f"(largest: {int(per_k[-1]['n_triangles'].max()) if len(per_k[-1]['rep']) else 0} triangles on "
        f"{int(per_k[-1]['n_vertices'][per_k[-1]['n_triangles'].argmax()]) if len(per_k[-1]['rep']) else 0} vertices); both calls {time.time() - t:.2f} s wall")
    rng = np.random.default_rng(7)
    n_s = min(sample_n or SAMPLE[name], nv)
    vmask = np.zeros(nv, np.uint8); vmask[rng.choice(nv, size=n_s, replace=False)] = 1
    ok = compare(a, nv, vmask, f"{name} sample of {int(vmask.sum())} vertices") and ok
    a.close()
for name in names:                                          # the long comparisons last: the measurements above are on record by then
    if name in WHOLE:
        nv, a = load(name)
        ok = compare(a, nv, None, f"{name} whole result") and ok
        a.close()
say("NUCLEUS_HIERARCHY_CHECK", "OK" if ok else "MISMATCH")
