"""By hand: komb_community_hierarchy_run at full-size C2 (|V| = 1 M) and C3 (|V| = 10 M, |E| ~ 100 M).  At C2 against the
full reference of tests/community_hierarchy_ref.py: every node array, node[] and info.  At C3 the reference does not fit
(one scipy component search over 100 M edges per level, the labels of all levels kept): the invariants, and
komb_community_hierarchy_labels(k) against komb_truss_communities_run(k) for every k from 0 to k_max + 1 and KOMB_COMM_K_MAX,
and the k = 3 labels against the hash pinned in tests/test_gpu_truss_communities.py (the full CPU reference's).
    python tests/manual/c3_community_hierarchy_check.py [C2|C3 ...] > c3_community_hierarchy.log
"""
import hashlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import komb_amd
import community_hierarchy_ref as CH

import threading
def _heartbeat(t0=time.time()):                      # a line a minute: the reference's passes are silent for longer than that
    while True:
        time.sleep(60)
        print(f"  ... {time.time() - t0:.0f} s", flush=True)
threading.Thread(target=_heartbeat, daemon=True).start()

CONFIGS = {"C2": (1_000_000, 2_425_000), "C3": (10_000_000, 24_250_000)}
PINNED_K3 = {"C2": "f55c813dc95dc030", "C3": "d6d55a7399ecbbae"}       # tests/test_gpu_truss_communities.py
sha = lambda x: hashlib.sha256(np.ascontiguousarray(x, np.int32).tobytes()).hexdigest()[:16]
ok = True
for name in sys.argv[1:] or ["C2", "C3"]:
    nv, ncl = CONFIGS[name]
    uv = komb_amd.gen_hug_edges(nv, ncl, 2.6, 42)
    a = komb_amd.KombAccel(); a.from_edges(nv, uv); del uv
    eu, ev, tr = a.run_truss()
    tmax = int(tr.max())
    nodes, node = a.run_community_hierarchy()
    info = a.community_hierarchy_info()
    print(name, "nv", a.nv, "ne", a.ne, "tmax", tmax, info, {f: sha(nodes[f]) for f in CH.FIELDS}, "node", sha(node), flush=True)
    CH.check_invariants(dict(nodes, node=node))
    same = np.array_equal(node >= 0, tr >= 3) and np.array_equal(nodes["k"][node[node >= 0]], tr[node >= 0])
    for k in list(range(0, tmax + 2)) + [-1]:
        want = a.run_truss_communities(k)
        got = a.community_hierarchy_labels(k)
        eq = np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        if k == 3:
            eq = eq and sha(got[0]) == PINNED_K3[name]
        print(name, "k", k, "labels equal:", bool(eq), flush=True)
        same = same and eq
    if name == "C2":
        t = time.time()
        want = CH.community_hierarchy(nv, eu, ev, tr)
        CH.check_invariants(want)
        eq = (all(np.array_equal(nodes[f], want[f]) for f in CH.FIELDS) and np.array_equal(node, want["node"]) and
              tuple(info[f] for f in ("n_nodes", "n_roots", "k_max", "depth", "n_member_edges")) == CH.info(want))
        print(name, "reference", round(time.time() - t, 1), "s  equal:", bool(eq), flush=True)
        same = same and eq
    ok = ok and bool(same)
    a.close()
print("COMMUNITY_HIERARCHY_CHECK", "OK" if ok else "MISMATCH")
