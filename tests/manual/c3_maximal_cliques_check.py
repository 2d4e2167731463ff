"""By hand: komb_maximal_cliques_run at full-size C2 (|V| = 1 M) and C3 (|V| = 10 M, |E| ~ 100 M), bench.py's configurations, on
the whole-graph k-truss result, with option MAXIMAL_DEBUG (one stderr line per run).  Per graph: the maximal cliques of at
least a high k_min (C2: 18, C3: 32), then of the lowest k_min the library accepts under its limit of 4096 candidates and
excluded vertices per root (tried from 2 upwards; every refusal is recorded).  It records the histogram, omega, the flags, the
cliques, the nodes, the roots opened, the largest candidate list and the device time of each -- single runs -- beside the
k-truss step (support + peel, komb_stats) and, as the yardstick, a clique census over the window (k_min, t_max) of the same graph
in the same process, and checks the sum of count against the sum of size * hist, omega against the census' and, where the
list is held, largest against the list.
Every graph is a step of its own: a child process under a time limit.  After a step that failed, was killed or ran out of
time nothing more is started.
    python tests/manual/c3_maximal_cliques_check.py [C2|C3 ...] [--limit SECONDS] [--out FILE]   (default: profiles/maximal_cliques_c2_c3_check.txt)
"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = {"C2": (1_000_000, 2_450_000, 18), "C3": (10_000_000, 24_250_000, 32)}
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "maximal_cliques_c2_c3_check.txt")
limit = 300
step = None
if "--out" in args:
    i = args.index("--out"); out_path = args[i + 1]; del args[i:i + 2]
if "--limit" in args:
    i = args.index("--limit"); limit = int(args[i + 1]); del args[i:i + 2]
if "--step" in args:
    i = args.index("--step"); step = args[i + 1]; del args[i:i + 2]

if step is None:                                         # the driver: one child per graph, appending to the same file
    open(out_path, "w").close()
    for name in (args or ["C2", "C3"]):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--out", out_path], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            with open(out_path, "a") as f:
                f.write(f"{name}: the step ended with status {rc}; nothing was run after it\n")
            sys.exit(rc)
    sys.exit(0)

import numpy as np
import komb_amd

out = open(out_path, "a")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n"); out.flush()


def fields(info):
    return ", ".join(f"{k} {v:.3f}" if k == "ms" else f"{k} {v}" for k, v in info.items())


def both(a, name, k_min):
    """The maximal cliques of >= k_min vertices and the census of the same window, one run each."""
    hist, count, largest, info = a.run_maximal_cliques(k_min)
    what = f"k_min = {k_min}"
    say(f"{name} {what}: " + fields(info))
    say(f"{name} {what}: hist[{info['k_min']} .. {info['k_hi']}] = {[int(x) for x in hist]}")
    sizes = np.arange(info["k_min"], info["k_hi"] + 1)
    say(f"{name} {what}: sum of count = {int(count.astype(np.int64).sum())}, sum of size * hist = {int((sizes * hist).sum())}, "
        f"vertices in a clique {int((count > 0).sum())}, largest count {int(count.max())}")
    if info["flags"] & komb_amd._lib.KOMB_MAXIMAL_LISTED:
        offset, verts = a.maximal_cliques_list()
        seen = np.zeros_like(largest)
        np.maximum.at(seen, verts, np.repeat(np.diff(offset), np.diff(offset)).astype(np.int32))
        say(f"{name} {what}: the list holds {len(offset) - 1} cliques, {len(verts)} vertices; largest equals the list's: {bool(np.array_equal(seen, largest))}")
    else:
        say(f"{name} {what}: the list is not held")
    total, _, cinfo = a.run_clique_census(k_min, -1, 0)
    say(f"{name} {what}, the census of the window: " + fields(cinfo))
    say(f"{name} {what}: omega {info['omega']} against the census' {cinfo['omega']}; device time {info['ms']:.3f} ms against the census' {cinfo['ms']:.3f} ms")


name = step
nv, n_cliques, k_high = CONFIGS[name]
t0 = time.time()
uv = komb_amd.gen_hug_edges(nv, n_cliques, 2.6, 42)
with komb_amd.KombAccel() as a:
    a.from_edges(nv, uv)
    del uv
    eu, ev, tr = a.run_truss()
    st = a.stats()
    t_max = int(tr.max())
    say(f"{name}: |V| = {nv}, |E| = {len(eu)}, t_max = {t_max}, k-truss step {st['ms_support'] + st['ms_peel']:.2f} ms "
        f"(generated, built and peeled in {time.time() - t0:.1f} s)")
    del eu, ev, tr
    a.set_option("MAXIMAL_DEBUG", "1")
    both(a, name, k_high)
    for k_min in range(2, t_max + 1):
        try:
            both(a, name, k_min)                         # (a refusal comes from its first call, before anything is reported)
        except komb_amd.KombError as e:
            if e.code != komb_amd._lib.KOMB_ERR_LIMIT:
                raise
            say(f"{name} k_min = {k_min}: refused: {e}")
            continue
        say(f"{name}: the lowest k_min accepted is {k_min}")
        break
