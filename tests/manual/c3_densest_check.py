"""By hand: komb_densest_subgraph_run at full-size C2 (|V| = 1 M) and C3 (|V| = 10 M, |E| ~ 100 M), bench.py's configurations,
at iters = 0, 16 and 64, every output against the restatement of tests/densest_ref.py; prints |P|, |E_P|, the density found,
the certificate, the total device time and the time per round (the difference of the 64- and the 16-round run over 48).
    python tests/manual/c3_densest_check.py [C2|C3 ...] > c3_densest.log
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import komb_amd
import densest_ref as D

CONFIGS = {"C2": (1_000_000, 2_450_000), "C3": (10_000_000, 24_250_000)}
REPS = 5
ok = True
for name in sys.argv[1:] or ["C2", "C3"]:
    nv, ncl = CONFIGS[name]
    uv = komb_amd.gen_hug_edges(nv, ncl, 2.6, 42)
    a = komb_amd.KombAccel(); a.from_edges(nv, uv); del uv
    rowptr, col = a.get_csr()
    _, core = a.run_core()
    print(name, "nv", a.nv, "ne", a.ne, "kmax", int(core.max()), flush=True)
    ms = {}
    for iters in (0, 16, 64):
        best = None
        for _ in range(REPS):
            member, load, info = a.run_densest_subgraph(iters)
            best = info["ms"] if best is None else min(best, info["ms"])
        ms[iters] = best
        n_k, m_k = a.densest_subgraph_profile()
        t = time.time()
        want = D.densest(rowptr, col, core, iters)
        same = (np.array_equal(member, want["member"]) and np.array_equal(load, want["load"]) and np.array_equal(n_k, want["n_k"])
                and np.array_equal(m_k, want["m_k"]) and all(info[f] == want[f] for f in D.INFO_FIELDS))
        ok = ok and same
        found = info["m_sub"] / max(info["n_sub"], 1)
        bound = min(info["k_max"], info["load_max"] / iters) if iters else info["k_max"]
        print(f"{name} iters={iters} |P|={info['n_pruned']} |E_P|={info['m_pruned']} k*={info['k_best']} c={info['k_prune']} "
              f"source={info['source']} found={info['m_sub']}/{info['n_sub']}={found:.4f} certificate<={bound:.4f} "
              f"(load_max={info['load_max']}, k_max={info['k_max']}) ms={best:.3f} reference {time.time() - t:.1f} s equal: {bool(same)}", flush=True)
    per_round = (ms[64] - ms[16]) / 48.0
    floor_us = info["m_pruned"] / 25.5e9 * 1e6                # 24-27 G integer atomics per second (profiles/r05_atomic_rate.txt)
    print(f"{name} ms per round = {per_round * 1000:.2f} us; atomic floor |E_P| / 25.5 G/s = {floor_us:.2f} us; ratio {per_round * 1000 / max(floor_us, 1e-9):.1f}", flush=True)
    a.close()
print("DENSEST_CHECK", "OK" if ok else "MISMATCH")
