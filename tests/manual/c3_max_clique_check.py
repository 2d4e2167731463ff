"""By hand: komb_max_clique_run at full-size C2 (|V| = 1 M) and C3 (|V| = 10 M, |E| ~ 100 M), bench.py's configurations, on the
whole-graph k-truss result, with option MAXCLQ_DEBUG (one stderr line per run: the nodes and the device time of each phase).
It records omega, upper, t_max, the flags, the maximum cliques, the roots opened, the nodes and the device time, best of 3, with
and without the seed, beside the k-truss step of the same graph in the same process (support + peel, komb_stats).  A run the
library refuses (KOMB_ERR_LIMIT: a root with more than 4096 candidates) is recorded as the result.  The witness and every listed
clique are checked pair by pair against the fetched edge list.
    python tests/manual/c3_max_clique_check.py [C2|C3 ...] [--budget N] [--out FILE]   (default: profiles/max_clique_c2_c3_check.txt)
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import komb_amd

CONFIGS = {"C2": (1_000_000, 2_450_000), "C3": (10_000_000, 24_250_000)}
REPS = 3
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "max_clique_c2_c3_check.txt")
budget = 0
if "--out" in args:
    i = args.index("--out"); out_path = args[i + 1]; del args[i:i + 2]
if "--budget" in args:
    i = args.index("--budget"); budget = int(args[i + 1]); del args[i:i + 2]
out = open(out_path, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n"); out.flush()


def is_clique(c, keys, nv):
    c = np.sort(np.asarray(c, np.int64))
    i, j = np.triu_indices(len(c), 1)
    want = c[i] * nv + c[j]
    pos = np.searchsorted(keys, want)
    return len(set(c.tolist())) == len(c) and bool(np.all(pos < len(keys))) and bool(np.all(keys[np.minimum(pos, len(keys) - 1)] == want))


for name in (args or ["C2", "C3"]):
    nv, n_cliques = CONFIGS[name]
    t0 = time.time()
    uv = komb_amd.gen_hug_edges(nv, n_cliques, 2.6, 42)
    with komb_amd.KombAccel() as a:
        a.from_edges(nv, uv)
        del uv
        eu, ev, tr = a.run_truss()
        st = a.stats()
        say(f"{name}: |V| = {nv}, |E| = {len(eu)}, t_max = {int(tr.max())}, k-truss step {st['ms_support'] + st['ms_peel']:.2f} ms "
            f"(generated, built and peeled in {time.time() - t0:.1f} s)")
        keys = eu.astype(np.int64) * nv + ev
        a.set_option("MAXCLQ_DEBUG", "1")
        for seed in ("1", "0"):
            a.set_option("MAXCLQ_SEED", seed)
            best = None
            for _ in range(REPS):
                try:
                    a.max_clique_run(budget)
                except komb_amd.KombError as e:
                    say(f"{name} seed={seed}: refused: {e}")
                    break
                info = a.max_clique_info()
                best = info if best is None or info["ms"] < best["ms"] else best
            if best is None:
                continue
            say(f"{name} seed={seed}: " + ", ".join(f"{k} {v:.3f}" if k == "ms" else f"{k} {v}" for k, v in best.items()))
            count, witness = a.max_clique_fetch()
            ok = is_clique(witness, keys, nv)
            if best["flags"] & 4:
                cliques = a.max_clique_list()
                ok = ok and all(is_clique(c, keys, nv) for c in cliques) and int(count.sum()) == cliques.size
            say(f"{name} seed={seed}: witness {witness.tolist()}, every reported clique is one: {ok}")
