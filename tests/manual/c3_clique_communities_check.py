"""By hand: komb_clique_communities_run at full-size C2 (|V| = 1 M), bench.py's configuration, on the whole-graph k-truss result,
with option PERC_DEBUG (one stderr line per run).  The maximal cliques at k_min = k = 18 (4 578 cliques, listed), then at lower
k_min = k whose list is still held (15, 12).  Per k it records pair_tests, the communities, the largest, the covered and the
overlapping vertices and the device time -- single runs -- beside the device time of komb_maximal_cliques_run on the same graph in
the same process, and checks that every member clique lies inside the community of its label and that n_comm sums to the vertices
of the communities.  A refusal by the budget is recorded, not an error.
The run is a step of its own: a child process under a time limit.
    python tests/manual/c3_clique_communities_check.py [--limit SECONDS] [--out FILE]   (default: profiles/clique_communities_c2_check.txt)
"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

NV, N_CLIQUES, KS = 1_000_000, 2_450_000, (18, 15, 12)
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "clique_communities_c2_check.txt")
limit = 300
step = False
if "--out" in args:
    i = args.index("--out"); out_path = args[i + 1]; del args[i:i + 2]
if "--limit" in args:
    i = args.index("--limit"); limit = int(args[i + 1]); del args[i:i + 2]
if "--step" in args:
    step = True

if not step:                                             # the driver: one child, under the limit
    open(out_path, "w").close()
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--out", out_path], timeout=limit).returncode
    except subprocess.TimeoutExpired:
        rc = 124
    if rc != 0:
        with open(out_path, "a") as f:
            f.write(f"C2: the step ended with status {rc}\n")
    sys.exit(rc)

import numpy as np
import komb_amd

out = open(out_path, "a")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n"); out.flush()


def fields(info):
    return ", ".join(f"{k} {v:.3f}" if k == "ms" else f"{k} {v}" for k, v in info.items())


def one(a, k):
    _, _, _, minfo = a.run_maximal_cliques(k)
    what = f"C2 k = {k}"
    say(f"{what}: the maximal cliques: " + fields(minfo))
    if not minfo["flags"] & komb_amd._lib.KOMB_MAXIMAL_LISTED:
        say(f"{what}: the list is not held")
        return
    try:
        label, size, rep, ncl, offset, verts, n_comm, first, info = a.run_clique_communities(k)
    except komb_amd.KombError as e:
        if e.code != komb_amd._lib.KOMB_ERR_LIMIT:
            raise
        say(f"{what}: refused: {e}")
        return
    say(f"{what}: the communities: " + fields(info))
    coff, cverts = a.maximal_cliques_list()
    number = {int(r): c for c, r in enumerate(rep.tolist())}
    sets = [set(verts[offset[c]:offset[c + 1]].tolist()) for c in range(len(rep))]
    inside = all(set(cverts[coff[i]:coff[i + 1]].tolist()) <= sets[number[int(label[i])]] for i in range(len(label)) if label[i] >= 0)
    say(f"{what}: every member clique lies inside its community: {inside}; sum of n_comm = {int(n_comm.astype(np.int64).sum())}, "
        f"vertices of the communities = {len(verts)}; community sizes (vertices) = {sorted(np.diff(offset).tolist(), reverse=True)[:12]}")
    say(f"{what}: pair_tests {info['pair_tests']} in {info['ms']:.3f} ms of device time (all launches of the run, the two sorts included); "
        f"komb_maximal_cliques_run took {minfo['ms']:.3f} ms")


t0 = time.time()
uv = komb_amd.gen_hug_edges(NV, N_CLIQUES, 2.6, 42)
with komb_amd.KombAccel() as a:
    a.from_edges(NV, uv)
    del uv
    eu, ev, tr = a.run_truss()
    st = a.stats()
    say(f"C2: |V| = {NV}, |E| = {len(eu)}, t_max = {int(tr.max())}, k-truss step {st['ms_support'] + st['ms_peel']:.2f} ms "
        f"(generated, built and peeled in {time.time() - t0:.1f} s)")
    del eu, ev, tr
    a.set_option("PERC_DEBUG", "1")
    one(a, KS[0])                                        # (the first run of a process pays for the code object's load)
    for k in KS:
        one(a, k)
