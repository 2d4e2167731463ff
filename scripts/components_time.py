"""Warm device times of komb_components_run at C2 and C3, in one process: `components_time.py [reps [config ...]]`.
Prints one JSON line: per config, komb_stats.ms_core of the same graph and, for core k = 0, core K_MAX and truss k = 3
with COMP_SAMPLE 0 and 1, the median and best ms of `reps` calls after one warm-up (komb_components_info, HIP events;
every call waits for its result, so each runs on an idle device), with the members / components / largest it found."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import komb_amd

CONFIGS = {"C2": (1_000_000, 2_425_000, 2.6, 42), "C3": (10_000_000, 24_250_000, 2.6, 42)}
CASES = (("core", 0), ("core", -1), ("truss", 3))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    names = sys.argv[2:] or list(CONFIGS)
    out = {"reps": reps}
    with komb_amd.KombAccel() as a:
        for name in names:
            nv, ncl, alpha, seed = CONFIGS[name]
            uv = komb_amd.gen_hug_edges(nv, ncl, alpha, seed)
            a.from_edges(nv, uv)
            del uv
            a.core_run()
            a.core_run()
            res = {"nv": nv, "ne": a.ne, "core_ms": round(a.stats()["ms_core"], 3)}
            a.truss_run()
            for kind, k in CASES:
                for sample in ("0", "1"):
                    a.set_option("COMP_SAMPLE", sample)
                    a.components_run(kind, k)                   # warm: pool blocks made
                    ms = []
                    for _ in range(reps):
                        a.components_run(kind, k)
                        ms.append(a.components_info()["ms"])
                    info = a.components_info()
                    res[f"{kind}_k{'max' if k < 0 else k}_sample{sample}"] = {
                        "ms_median": round(float(np.median(ms)), 3), "ms_best": round(min(ms), 3), "k_used": info["k_used"],
                        "n_members": info["n_members"], "n_components": info["n_components"], "largest": info["largest"]}
            a.set_option("COMP_SAMPLE", None)
            out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
