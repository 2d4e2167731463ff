"""By hand: komb_nucleus_run at full-size C2 (|V| = 1 M) and C3 (|V| = 10 M, |E| ~ 100 M), bench.py's configurations, on the
whole-graph k-truss result.  It records the triangles, the 4-cliques, theta_max, the levels and the sub-rounds, the device time
of the run and of the 4-clique pass alone (option NUC_DEBUG), best of 5, beside two yardsticks: the k-truss step of the same
graph in the same process (support + peel, komb_stats), and the byte floor of the clique pass -- every 16-byte clique record
written and read once and every 4-byte incidence written once, over 8 TB/s.  A run the library refuses (KOMB_ERR_LIMIT) is
recorded as the result, with the counts the refusal names.  Every output is compared with the restatement of
tests/nucleus_ref.py where that finishes: on the k-truss result induced by a seeded vertex sample (C2: 200 000 vertices, C3:
1 000 000; --sample N for both), and, after all measurements, on the WHOLE result of C2 (plain Python over 9.7 M triangles:
minutes and gigabytes, both recorded; --full adds C3's, --no-full skips C2's).
    python tests/manual/c3_nucleus_check.py [C2|C3 ...] [--sample N] [--full|--no-full] [--out FILE]   (default: profiles/nucleus_c2_c3_check.txt)
"""
import os, re, resource, sys, tempfile, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import komb_amd
import nucleus_ref as R

CONFIGS = {"C2": (1_000_000, 2_450_000), "C3": (10_000_000, 24_250_000)}
SAMPLE = {"C2": 200_000, "C3": 1_000_000}                  # vertices of the sampled comparison
WHOLE = {"C2"}                                              # whole-result comparison by default
REPS = 5
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "nucleus_c2_c3_check.txt")
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


def traced_run(a):
    """One run with the library's stderr trace caught: (error or None, the trace line's times by name)."""
    sys.stderr.flush()
    err = None
    with tempfile.TemporaryFile() as f:
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            a.nucleus_run()
        except komb_amd.KombError as e:
            err = e
        finally:
            os.dup2(keep, 2); os.close(keep)
        f.seek(0)
        text = f.read().decode(errors="replace")
    times = {k: float(v) for k, v in re.findall(r"(run|triangle pass|clique pass|peel) ([0-9.]+) ms", text)}
    return err, times


def compare(a, nv, vmask, what):
    eu, ev, _ = a.run_truss(vmask)
    err, _ = traced_run(a)
    if err is not None:
        say(what, "refused:", err)
        return True
    t = time.time()
    done = threading.Event()

    def beat():                                             # (stdout only: a long restatement stays visibly alive)
        while not done.wait(60.0):
            print(f"  ... restatement of {what}: {time.time() - t:.0f} s", flush=True)
    threading.Thread(target=beat, daemon=True).start()
    try:
        want = R.decompose(nv, eu, ev)
    finally:
        done.set()
    tris, et, vt, info = a.nucleus_fetch(), a.nucleus_fetch_edges(), a.nucleus_fetch_vertices(), a.nucleus_info()
    same = (all(np.array_equal(tris[k], want[k]) for k in ("a", "b", "c", "key0", "theta")) and np.array_equal(et, want["edge_theta"])
            and np.array_equal(vt, want["vertex_theta"]) and all(info[k] == v for k, v in want["info"].items()))
    say(f"{what}: edges {len(eu)} triangles {info['n_triangles']} cliques {info['n_cliques4']} theta_max {info['theta_max']} "
        f"levels {info['n_levels']} sub-rounds {info['n_subrounds']}; restatement {time.time() - t:.1f} s, "
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
    truss_ms = None
    for _ in range(3):                                      # the yardstick: the k-truss step of this graph, best of 3 (the first prepares)
        a.truss_run()
        st = a.stats()
        ms = st["ms_support"] + st["ms_peel"]
        truss_ms = ms if truss_ms is None else min(truss_ms, ms)
    say(name, "nv", a.nv, "ne", a.ne, "triangles (k-truss step)", st["triangles"], f"k-truss step {truss_ms:.3f} ms")
    best, err = None, None
    for _ in range(REPS):
        err, times = traced_run(a)
        if err is not None:
            break
        best = times if best is None else {k: min(best[k], times[k]) for k in times}
    if err is not None:
        say(f"{name}: refused: {err}")
    else:
        info = a.nucleus_info()
        floor = (2 * 16 + 4 * 4) * info["n_cliques4"] / 8e12 * 1e3
        say(f"{name}: triangles {info['n_triangles']} cliques {info['n_cliques4']} theta_max {info['theta_max']} levels {info['n_levels']} "
            f"sub-rounds {info['n_subrounds']}")
        say(f"{name}: run {best['run']:.3f} ms (triangle pass {best['triangle pass']:.3f}, clique pass {best['clique pass']:.3f}, peel {best['peel']:.3f}); "
            f"k-truss step {truss_ms:.3f} ms; clique pass byte floor {floor:.3f} ms; clique pass / floor = {best['clique pass'] / max(floor, 1e-9):.1f}")
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
say("NUCLEUS_CHECK", "OK" if ok else "MISMATCH")
