"""Warm device times of komb_hierarchy_run at C2 and C3, in one process: `hierarchy_time.py [reps [config ...]]`.
Prints one JSON line: per config and kind, the median, best and worst ms of `reps` calls after one warm-up
(komb_hierarchy_info, HIP events; every call waits for its result, so each runs on an idle device), the forest's figures and
its populated levels, and beside them the yardstick from the same session and graph: komb_components_run for core k = 0
(and truss k = 2) -- what one threshold costs a user who asks level by level."""
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
            _, core = a.run_core()
            _, _, tr = a.run_truss()
            res = {"nv": nv, "ne": a.ne}
            for kind, k0, levels in (("core", 0, len(np.unique(core))), ("truss", 2, len(np.unique(tr)))):
                h = timed(lambda: a.hierarchy_run(kind), a.hierarchy_info, reps)
                info = a.hierarchy_info()
                h.update({f: info[f] for f in ("n_nodes", "n_roots", "k_max", "depth")}, populated_levels=levels)
                c = timed(lambda: a.components_run(kind, k0), a.components_info, reps)
                h["components_k%d" % k0] = c
                h["per_level_over_hierarchy"] = round(c["ms_median"] * levels / h["ms_median"], 2)
                res[kind] = h
            out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
