"""By hand: komb_clique_census_run at full-size C2 (|V| = 1 M) and C3 (|V| = 10 M, |E| ~ 100 M), bench.py's configurations, on the
whole-graph k-truss result, with option CENSUS_DEBUG (one stderr line per run).  Per graph: the census of the window
(t_max - 8, t_max), then the lowest k_lo the library accepts under its limit of 4096 candidates per root (tried from 2 upwards;
every refusal is recorded) with the window (k_lo, t_max) and k_local = k_lo.  It records the totals, omega, the flags, the
nodes, the roots opened, the largest candidate set and the device time of each -- single runs -- beside the k-truss step
(support + peel, komb_stats) and a maximum-clique run of the same graph in the same process, and checks omega and total[omega]
against that run and the sum of local against k_local * total[k_local].
Every graph is a step of its own: a child process under a time limit.  After a step that failed, was killed or ran out of
time nothing more is started.
    python tests/manual/c3_clique_census_check.py [C2|C3 ...] [--limit SECONDS] [--out FILE]   (default: profiles/clique_census_c2_c3_check.txt)
"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = {"C2": (1_000_000, 2_450_000), "C3": (10_000_000, 24_250_000)}
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "clique_census_c2_c3_check.txt")
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


def show(name, what, total, local, info):
    say(f"{name} {what}: " + ", ".join(f"{k} {v:.3f}" if k == "ms" else f"{k} {v}" for k, v in info.items()))
    say(f"{name} {what}: total[{info['k_lo']} .. {info['k_hi']}] = {[int(x) for x in total]}")
    if local is not None:
        kl = info["k_local"]
        want = kl * int(total[kl - info["k_lo"]])
        both = int((local >> np.uint64(32)).sum()) * 2 ** 32 + int((local & np.uint64(0xFFFFFFFF)).sum())   # (no 64-bit overflow)
        say(f"{name} {what}: sum of local = {both}, k_local * total[k_local] = {want}, largest local {int(local.max())}")


name = step
nv, n_cliques = CONFIGS[name]
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
    minfo = a.run_max_clique()[0]
    say(f"{name} maximum-clique run: " + ", ".join(f"{k} {v:.3f}" if k == "ms" else f"{k} {v}" for k, v in minfo.items()))
    a.set_option("CENSUS_DEBUG", "1")
    total, local, info = a.run_clique_census(max(t_max - 8, 2), -1, 0)
    show(name, "high window", total, local, info)
    at_omega = int(total[info["omega"] - info["k_lo"]]) if info["omega"] else 0    # (omega 0: the window lies above every clique)
    say(f"{name} high window: omega {info['omega']} and total[omega] {at_omega} against the maximum-clique run's {minfo['omega']} and {minfo['n_max_cliques']}")
    for k_lo in range(2, t_max + 1):
        try:
            total, local, info = a.run_clique_census(k_lo, -1, k_lo)
        except komb_amd.KombError as e:
            if e.code != komb_amd._lib.KOMB_ERR_LIMIT:
                raise
            say(f"{name} k_lo = {k_lo}: refused: {e}")
            continue
        say(f"{name}: the lowest k_lo accepted is {k_lo}")
        show(name, f"k_lo = {k_lo}", total, local, info)
        break
