"""By hand: komb_truss_communities_run at full-size C3 (|V| = 10 M, |E| ~ 100 M) against the full numpy / scipy reference
of tests/truss_communities_ref.py, every label, size and n_comm entry, for k = 3 and K_MAX.  Too large for the test suite
(about 15 min of CPU and 25 GB of host memory); tests/test_gpu_truss_communities.py pins the k = 3 label hash instead.
    python tests/manual/c3_communities_check.py [k ...] > c3_communities.log
"""
import hashlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import komb_amd
import truss_communities_ref as R

import threading
def _heartbeat(t0=time.time()):                      # a line a minute: the reference's passes are silent for longer than that
    while True:
        time.sleep(60)
        print(f"  ... {time.time() - t0:.0f} s", flush=True)
threading.Thread(target=_heartbeat, daemon=True).start()

ks = [int(x) for x in sys.argv[1:]] or [3, -1]
nv = 10_000_000
uv = komb_amd.gen_hug_edges(nv, 24_250_000, 2.6, 42)
a = komb_amd.KombAccel(); a.from_edges(nv, uv); del uv
eu, ev, tr = a.run_truss()
print("graph nv", a.nv, "ne", a.ne, "tmax", int(tr.max()), flush=True)
t = time.time(); tri = R.triangles(nv, eu, ev); print("reference triangles", len(tri[0]), round(time.time() - t, 1), "s", flush=True)
ok = True
for k in ks:
    kk = int(tr.max()) if k < 0 else max(k, 2)
    label, size = a.run_truss_communities(k)
    n_comm = a.truss_communities_fetch_vertices()
    info = a.truss_communities_info()
    t = time.time(); want = R.communities(nv, eu, ev, tr, kk, tri)
    same = (np.array_equal(label, want) and np.array_equal(size, R.sizes(want)) and
            np.array_equal(n_comm, R.vertex_multiplicity(nv, eu, ev, want)) and
            (info["n_member_edges"], info["n_communities"], info["largest"], info["n_multi_vertices"]) == R.summary(nv, eu, ev, want))
    print("k", kk, info, "sha256(label)", hashlib.sha256(label.tobytes()).hexdigest()[:16], "reference", round(time.time() - t, 1), "s  equal:", bool(same), flush=True)
    ok = ok and same
print("C3_COMMUNITIES", "OK" if ok else "MISMATCH")
