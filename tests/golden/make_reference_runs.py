"""Generates tests/golden/reference_runs.json -- the answers of the REFERENCE's own CoreA.h and HashIndexedMinHeap.h
(oracle/_ref/corea_ref, oracle/_ref/merge_ref) on the inputs of tests/test_oracle.py's reference tests, so that those
tests run where the reference binaries cannot be built (they still check the binaries live where they are built).

Run where oracle/_ref/ has been built (`make -C oracle ref`):

    python tests/golden/make_reference_runs.py

Sections:
  corea  random (degree, coreness) vectors -> scores of `corea_ref arrays` (exact doubles as hex)
  tsv    one kcore.tsv in the reference's format -> scores of `corea_ref tsv` (CoreA::readKOMBOutput)
  merge  random raw edge lists -> `merge_ref` on the simplified graph, unweighted and weighted with the oracle's CoreA
         scores: removal order, sides, block size, density (hex)
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import oracle as O               # noqa: E402

TSV_DEGREE = [4, 3, 3, 3, 6, 1, 1, 1, 1, 1, 0]
TSV_CORENESS = [3, 3, 3, 3, 1, 1, 1, 1, 1, 1, 0]


def tsv_text(deg, core):
    """kcore.tsv as the reference writes it (src/graph.cpp:467,474)."""
    return "#VID\tName\tCoreness\tDegree\n" + "".join("%d\t%s\t%d\t%d\n" % (i, "u%d" % i, c, d) for i, (d, c) in enumerate(zip(deg, core)))


def corea_cases():
    rng = np.random.default_rng(5)
    cases = []
    for n in (1, 2, 17, 400):
        core = rng.integers(0, 9, n).astype(np.int32)
        deg = (core + rng.integers(0, 30, n)).astype(np.int32)
        cases.append((deg, core))
    return cases


def merge_cases():
    rng = np.random.default_rng(77)
    cases = [(1, np.zeros((0, 2), np.int64)), (5, np.zeros((0, 2), np.int64)), (2, np.array([[0, 1]], np.int64)),
             (6, np.stack(np.triu_indices(6, 1), axis=1).astype(np.int64))]
    for _ in range(25):
        nv = int(rng.integers(2, 250))
        cases.append((nv, rng.integers(0, nv, (int(rng.integers(0, 8 * nv)), 2)).astype(np.int64)))
    return cases


def main():
    O.build()
    if O.ref_corea_path() is None or O.ref_merge_path() is None:
        raise SystemExit("oracle/_ref/corea_ref and oracle/_ref/merge_ref are needed (make -C oracle ref)")
    out = {"corea": [], "tsv": None, "merge": []}
    for deg, core in corea_cases():
        want = O.ref_corea_scores(deg, core)
        out["corea"].append({"degree": deg.tolist(), "coreness": core.tolist(), "ref_scores_hex": [float(x).hex() for x in want]})
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "kcore.tsv")
        with open(p, "w") as f:
            f.write(tsv_text(TSV_DEGREE, TSV_CORENESS))
        got = subprocess.run([O.ref_corea_path(), "tsv", p], capture_output=True, text=True, check=True).stdout.split()
    out["tsv"] = {"degree": TSV_DEGREE, "coreness": TSV_CORENESS, "ref_scores_hex": [float(x).hex() for x in got]}
    for nv, uv in merge_cases():
        rowptr, col = O.simplify(nv, uv)
        deg = O.degree(rowptr)
        case = {"nv": nv, "raw": uv.reshape(-1).tolist()}
        for tag, susp in (("", None), ("w_", O.corea_scores(deg, O.coreness(rowptr, col)))):
            order, side, nb, dens = O.ref_run_merge(rowptr, col, susp)
            case.update({tag + "order": order.tolist(), tag + "side": side.tolist(), tag + "n_block": nb, tag + "density_hex": float(dens).hex()})
        out["merge"].append(case)
    with open(os.path.join(HERE, "reference_runs.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
