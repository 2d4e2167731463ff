"""Warm device times of komb_core_run and komb_onion_run at C2 and C3, in one process: `onion_time.py [reps [config ...]]`.
Prints one JSON line: per config, best and median ms of `reps` calls of each (HIP events, komb_stats.ms_core and
komb_onion_info), the onion's layer count and the ratio of the medians."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import komb_amd

CONFIGS = {"C2": (1_000_000, 2_450_000, 2.6, 42), "C3": (10_000_000, 24_250_000, 2.6, 42)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    names = sys.argv[2:] or list(CONFIGS)
    out = {"reps": reps}
    with komb_amd.KombAccel() as a:
        for name in names:
            nv, ncl, alpha, seed = CONFIGS[name]
            uv = komb_amd.gen_hug_edges(nv, ncl, alpha, seed)
            a.from_edges(nv, uv)
            del uv
            a.core_run()
            a.onion_run()                               # warm: code object loaded, pool blocks made
            core_ms, onion_ms = [], []
            for _ in range(reps):
                a.core_run()
                core_ms.append(a.stats()["ms_core"])
                a.onion_run()
                onion_ms.append(a.onion_info()["ms"])
            info = a.onion_info()
            c, o = np.median(core_ms), np.median(onion_ms)
            out[name] = {"nv": nv, "ne": a.ne, "n_layers": info["n_layers"], "max_coreness": info["max_coreness"],
                         "core_ms_best": round(min(core_ms), 3), "core_ms_median": round(float(c), 3),
                         "onion_ms_best": round(min(onion_ms), 3), "onion_ms_median": round(float(o), 3),
                         "onion_over_core": round(float(o / c), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
