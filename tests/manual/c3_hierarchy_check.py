"""By hand: komb_hierarchy_run at full-size C2 (|V| = 1 M) and C3 (|V| = 10 M, |E| ~ 100 M), both kinds, against the full
scipy reference of tests/hierarchy_ref.py: every node array, node[] and info.  Too large for the test suite (one scipy
component search per level at 100 M edges; the labels of all levels are kept: about 3 GB at C3).
    python tests/manual/c3_hierarchy_check.py [C2|C3 ...] > c3_hierarchy.log
"""
import hashlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import komb_amd
import hierarchy_ref as H

import threading
def _heartbeat(t0=time.time()):                      # a line a minute: the reference's passes are silent for longer than that
    while True:
        time.sleep(60)
        print(f"  ... {time.time() - t0:.0f} s", flush=True)
threading.Thread(target=_heartbeat, daemon=True).start()

CONFIGS = {"C2": (1_000_000, 2_425_000), "C3": (10_000_000, 24_250_000)}
sha = lambda x: hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]
ok = True
for name in sys.argv[1:] or ["C2", "C3"]:
    nv, ncl = CONFIGS[name]
    uv = komb_amd.gen_hug_edges(nv, ncl, 2.6, 42)
    a = komb_amd.KombAccel(); a.from_edges(nv, uv); del uv
    rowptr, col = a.get_csr()
    _, core = a.run_core()
    eu, ev, tr = a.run_truss()
    print(name, "nv", a.nv, "ne", a.ne, "kmax", int(core.max()), "tmax", int(tr.max()), flush=True)
    for kind in ("core", "truss"):
        nodes, node = a.run_hierarchy(kind)
        info = a.hierarchy_info()
        print(name, kind, info, {f: sha(nodes[f]) for f in H.FIELDS}, "node", sha(node), flush=True)
        t = time.time()
        want = H.core_hierarchy(rowptr, col, core) if kind == "core" else H.truss_hierarchy(nv, eu, ev, tr)
        H.check_invariants(want, kind == "core")
        same = (all(np.array_equal(nodes[f], want[f]) for f in H.FIELDS) and np.array_equal(node, want["node"]) and
                (info["n_nodes"], info["n_roots"], info["k_max"], info["depth"]) == H.info(want, kind))
        print(name, kind, "reference", round(time.time() - t, 1), "s  equal:", bool(same), flush=True)
        ok = ok and same
    a.close()
print("HIERARCHY_CHECK", "OK" if ok else "MISMATCH")
