"""Warm device times of komb_community_hierarchy_run at C2 and C3, in one process:
`community_hierarchy_time.py [reps [config ...]]`.  Prints one JSON line: per config the median, best and worst ms of `reps`
calls after one warm-up (komb_community_hierarchy_info, HIP events; every call waits for its result, so each runs on an idle
device), the forest's figures, and beside them the yardstick from the same session and graph: the sum over the populated
levels k = 3 .. k_max of komb_truss_communities_run(k)'s ms -- what a user who asks level by level pays today -- and one
komb_truss_run for scale."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import komb_amd

CONFIGS = {"C2": (1_000_000, 2_425_000, 2.6, 42), "C3": (10_000_000, 24_250_000, 2.6, 42)}


def timed(run, info, reps):
    run()                                                   # warm: pool blocks made
    ms = []
    for _ in range(reps):
        run()
        ms.append(info()["ms"])
    return {"ms_median": round(float(np.median(ms)), 3), "ms_best": round(min(ms), 3), "ms_worst": round(max(ms), 3)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    names = sys.argv[2:] or list(CONFIGS)
    out = {"reps": reps}
    with komb_amd.KombAccel() as a:
        for name in names:
            nv, ncl, alpha, seed = CONFIGS[name]
            uv = komb_amd.gen_hug_edges(nv, ncl, alpha, seed)
            a.from_edges(nv, uv)
            del uv
            a.truss_run()
            _, _, tr = a.run_truss()                        # warm: the preparation is resident, the pool holds the blocks
            st = a.stats()
            levels = [int(k) for k in np.unique(tr) if k >= 3]
            del tr
            res = {"nv": nv, "ne": a.ne, "triangles": st["triangles"], "truss_run_ms": round(st["ms_support"] + st["ms_peel"] + st["ms_gather"], 3)}
            h = timed(a.community_hierarchy_run, a.community_hierarchy_info, reps)
            info = a.community_hierarchy_info()
            h.update({f: info[f] for f in ("n_nodes", "n_roots", "k_max", "depth", "n_member_edges")}, populated_levels=len(levels))
            res["community_hierarchy"] = h
            per_level = {}
            for k in levels:
                per_level[k] = timed(lambda: a.truss_communities_run(k), a.truss_communities_info, reps)["ms_median"]
            res["communities_per_level_ms"] = per_level
            res["communities_sum_ms"] = round(sum(per_level.values()), 3)
            res["per_level_sum_over_hierarchy"] = round(res["communities_sum_ms"] / h["ms_median"], 2)
            out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
