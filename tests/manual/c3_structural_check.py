"""By hand: komb_structural_clusters_run at full-size C2 (|V| = 1 M) and C3 (|V| = 10 M, |E| ~ 100 M), bench.py's configurations,
on the whole-graph k-truss result at (eps, mu) = (1/2, 3) and (7/10, 3): every output against the restatement of
tests/structural_ref.py (eps_den is small, so its int64 path holds), the device time of the run and of the similarity pass
alone (option STRUCT_DEBUG), best of 5, beside the two floors of that pass: its bytes -- eu, ev, sup in, one 64-byte line per
gather of d, the flag out -- over 8 TB/s, and its similar edges over 25.5 G atomics/s (profiles/r05_atomic_rate.txt).
    python tests/manual/c3_structural_check.py [C2|C3 ...] [--out FILE]      (default: profiles/structural_c2_c3_check.txt)
"""
import os, re, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import komb_amd
import structural_ref as R

CONFIGS = {"C2": (1_000_000, 2_450_000), "C3": (10_000_000, 24_250_000)}
PARAMS = [(1, 2, 3), (7, 10, 3)]
REPS = 5
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "structural_c2_c3_check.txt")
if "--out" in args:
    i = args.index("--out"); out_path = args[i + 1]; del args[i:i + 2]
out = open(out_path, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n"); out.flush()


def timed_run(a, p):
    """(ms of the run, ms of the similarity pass) of one run: the library's own HIP-event times, the second from its trace."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            a.structural_clusters_run(*p)
        finally:
            os.dup2(keep, 2); os.close(keep)
        f.seek(0)
        m = re.search(rb"run ([0-9.]+) ms, similarity pass ([0-9.]+) ms", f.read())
    return a.structural_clusters_info()["ms"], float(m.group(2)) if m else float("nan")


ok = True
for name in args or ["C2", "C3"]:
    nv, ncl = CONFIGS[name]
    uv = komb_amd.gen_hug_edges(nv, ncl, 2.6, 42)
    a = komb_amd.KombAccel(); a.from_edges(nv, uv); del uv
    a.set_option("STRUCT_DEBUG", "1")
    eu, ev, tr, sup = a.run_truss(with_support=True)
    m = len(eu)
    say(name, "nv", a.nv, "ne", a.ne, "triangles", int(sup.sum()) // 3)
    for p in PARAMS:
        best = None
        for _ in range(REPS):
            ms = timed_run(a, p)
            best = ms if best is None else (min(best[0], ms[0]), min(best[1], ms[1]))
        label, size, role, sim_deg = a.structural_clusters_fetch()
        similar = a.structural_clusters_fetch_edges()
        info = a.structural_clusters_info()
        t = time.time()
        want = R.clusters(nv, eu, ev, sup, *p)
        same = (np.array_equal(label, want["label"]) and np.array_equal(size, want["size"]) and np.array_equal(role, want["role"])
                and np.array_equal(sim_deg, want["sim_deg"]) and np.array_equal(similar, want["similar"])
                and all(info[k] == v for k, v in want["info"].items()))
        ok = ok and same
        floor_bytes = m * (12 + 2 * 64 + 1) / 8e12 * 1e3
        floor_atomics = info["n_similar_edges"] / 25.5e9 * 1e3
        floor = max(floor_bytes, floor_atomics)
        say(f"{name} eps={p[0]}/{p[1]} mu={p[2]}: similar={info['n_similar_edges']} cores={info['n_cores']} borders={info['n_borders']} "
            f"hubs={info['n_hubs']} outliers={info['n_outliers']} clusters={info['n_clusters']} largest={info['largest']}")
        say(f"{name} eps={p[0]}/{p[1]} mu={p[2]}: run {best[0]:.3f} ms, similarity pass {best[1]:.3f} ms; floors: bytes {floor_bytes:.3f} ms, "
            f"atomics {floor_atomics:.3f} ms; pass / larger floor = {best[1] / max(floor, 1e-9):.2f}; reference {time.time() - t:.1f} s equal: {bool(same)}")
        del want
    a.close()
say("STRUCTURAL_CHECK", "OK" if ok else "MISMATCH")
