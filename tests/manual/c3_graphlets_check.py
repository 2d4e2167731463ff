"""By hand: komb_graphlets_run at full-size C2 (|V| = 1 M) and C3 (|V| = 10 M, |E| ~ 100 M), bench.py's configurations, on the
whole-graph k-truss result.  No reference takes these sizes, so the outputs are checked against each other and against the
clique census: the six redundancy identities of the orbit sums, triangle and clique4 against komb_clique_census_run(3, 4), and
sum_e cycles4 = 4 (cycle4 + diamond + 3 clique4).  It prints the line of option GRAPHLET_DEBUG -- the walked entries, the roots
per tier, the device time of the run and of its three passes -- best of 3, beside the floor of the 4-cycle pass: cycle_items
over 25.5 G atomics/s (profiles/r05_atomic_rate.txt).
    python tests/manual/c3_graphlets_check.py [C2|C3 ...] [--out FILE]      (default: profiles/graphlets_c2_c3_check.txt)
"""
import os, re, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import komb_amd
from graphlets_ref import IDENTITIES

CONFIGS = {"C2": (1_000_000, 2_450_000), "C3": (10_000_000, 24_250_000)}
REPS = 3
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "graphlets_c2_c3_check.txt")
if "--out" in args:
    i = args.index("--out"); out_path = args[i + 1]; del args[i:i + 2]
out = open(out_path, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n"); out.flush()


def traced_run(a):
    """(ms of the run, the GRAPHLET_DEBUG line) of one run"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            a.graphlets_run()
        finally:
            os.dup2(keep, 2); os.close(keep)
        f.seek(0)
        m = re.search(rb"komb graphlets: [^\n]*", f.read())
    return a.graphlets_info()["ms"], m.group(0).decode() if m else "(no trace)"


def exact_sum(x):
    """the sum of a uint64 array as a Python integer: the two halves apart, so nothing overflows"""
    return (int((x >> np.uint64(32)).sum()) << 32) + int((x & np.uint64(0xFFFFFFFF)).sum())


ok = True
for name in args or ["C2", "C3"]:
    nv, ncl = CONFIGS[name]
    uv = komb_amd.gen_hug_edges(nv, ncl, 2.6, 42)
    a = komb_amd.KombAccel(); a.from_edges(nv, uv); del uv
    a.set_option("GRAPHLET_DEBUG", "1")
    a.truss_run()
    best = min((traced_run(a) for _ in range(REPS)), key=lambda x: x[0])
    info = a.graphlets_info()
    orbit = a.graphlets_fetch_vertices()
    cyc, clq = a.graphlets_fetch_edges()
    sums = [exact_sum(orbit[o]) for o in range(15)]
    ident = all(sums[x] * fx == sums[y] * fy for x, fx, y, fy in IDENTITIES)
    total = info["total"]
    census_total = a.run_clique_census(3, 4)[0]
    cliques = [int(x) for x in census_total] == [total["triangle"], total["clique4"]]
    cycles = exact_sum(cyc) == 4 * (total["cycle4"] + total["diamond"] + 3 * total["clique4"])
    ok = ok and ident and cliques and cycles and info["flags"] == 0
    say(name, "nv", a.nv, "ne", a.ne, "max_degree", info["max_degree"], "totals", total)
    say(name, best[1])
    say(f"{name}: run {best[0]:.3f} ms; cycle_items {info['cycle_items']}; floor of the 4-cycle pass at 25.5 G atomics/s "
        f"{info['cycle_items'] / 25.5e9 * 1e3:.3f} ms; identities {ident}, clique census {cliques}, cycle sum {cycles}")
    a.close()
say("GRAPHLETS_CHECK", "OK" if ok else "MISMATCH")
