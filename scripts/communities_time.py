"""Warm device times of komb_truss_communities_run at C2 and C3, in one process: `communities_time.py [reps [config ...]]`.
Prints one JSON line: per config, the device time of komb_truss_run on the same graph (komb_stats: preparation kept,
support + peel + gather), the truss-kind komb_components_run at k = 3 and, for k = 3 and K_MAX, the median and best ms of
`reps` communities calls after one warm-up (komb_truss_communities_info, HIP events; every call waits for its result,
so each runs on an idle device) with what it found, plus the wall time of the first vertex pass (fetch_vertices)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import komb_amd

CONFIGS = {"C2": (1_000_000, 2_425_000, 2.6, 42), "C3": (10_000_000, 24_250_000, 2.6, 42)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    names = sys.argv[2:] or list(CONFIGS)
    out = {"reps": reps}
    with komb_amd.KombAccel() as a:
        for name in names:
            nv, ncl, alpha, seed = CONFIGS[name]
            uv = komb_amd.gen_hug_edges(nv, ncl, alpha, seed)
            a.from_edges(nv, uv)
            del uv
            a.truss_run()
            a.truss_run()                                       # warm: the preparation is resident, the pool holds the blocks
            st = a.stats()
            res = {"nv": nv, "ne": a.ne, "max_trussness": st["max_trussness"],
                   "truss_run_ms": round(st["ms_support"] + st["ms_peel"] + st["ms_gather"], 3), "prepare_ms": None}
            a.truss_unprepare(); a.truss_run()
            res["prepare_ms"] = round(a.stats()["ms_prepare"], 3)
            a.components_run("truss", 3)
            ms = []
            for _ in range(reps):
                a.components_run("truss", 3)
                ms.append(a.components_info()["ms"])
            res["components_truss_k3_ms"] = {"median": round(float(np.median(ms)), 3), "best": round(min(ms), 3)}
            for k in (3, -1):
                a.truss_communities_run(k)                      # warm: pool blocks made
                ms = []
                for _ in range(reps):
                    a.truss_communities_run(k)
                    ms.append(a.truss_communities_info()["ms"])
                t0 = time.perf_counter()
                a.truss_communities_fetch_vertices()
                wall_v = time.perf_counter() - t0
                info = a.truss_communities_info()
                info.pop("ms")
                res[f"k{'max' if k < 0 else k}"] = dict(info, ms_median=round(float(np.median(ms)), 3), ms_best=round(min(ms), 3),
                                                        vertices_wall_ms=round(1e3 * wall_v, 1))
            out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
