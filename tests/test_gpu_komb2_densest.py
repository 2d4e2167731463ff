"""komb2 with KOMB_DENSEST on the generated SAM + FASTA fixture: densest_subgraph.tsv and core_density.tsv hold, keyed by
unitig Name, what the restatement of tests/densest_ref.py gives on the graph the SAM files define (in the vertex numbering of
the run's own kcore.tsv: the tie rules of the search read vertex ids); without the variable nothing changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import densest_ref as D
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_DENSEST", "KOMB_DENSEST_LOCAL", "KOMB_TRUSS", "KOMB_ONION", "KOMB_COMPONENTS", "KOMB_HIERARCHY")


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("densest_komb2")
    fasta, s1, s2 = samgraph.make_fixture(2000, 20000, seed=1)
    (d / "unitigs.l-1.fasta").write_bytes(fasta)
    (d / "reads1.fastq.sam").write_bytes(s1)
    (d / "reads2.fastq.sam").write_bytes(s2)
    return d, s1, s2


def _run(d, out, threads, **env_add):
    out.mkdir()
    cmd = [KOMB2, "-t", str(threads), "-l", "-1", "-o", str(out), "-i", f"{d}/reads1.fastq.sam", "-j", f"{d}/reads2.fastq.sam",
           "-u", f"{d}/unitigs.l-1.fasta"]
    env = {k: v for k, v in os.environ.items() if k not in VARS}
    env.update(env_add)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _rows(path, header):
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert rows[0] == header
    return rows[1:]


@pytest.mark.parametrize("threads", [1, 4])
def test_komb2_densest_tsv(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    names, edges = samgraph.build_graph(s1, s2, threads)

    off = tmp_path / "off"
    stdout_off = _run(d, off, threads)
    assert not (off / "densest_subgraph.tsv").exists() and not (off / "core_density.tsv").exists()

    for iters in (0, 16):
        out = tmp_path / f"on_{iters}"
        stdout_on = _run(d, out, threads, KOMB_DENSEST=str(iters))
        kc = _rows(out / "kcore.tsv", open(off / "kcore.tsv").readline().rstrip("\n").split("\t"))
        vid = {x[1]: int(x[0]) for x in kc}
        assert set(vid) == set(names) and sorted(vid.values()) == list(range(len(names)))
        nv = len(vid)
        core = np.zeros(nv, np.int32)
        for x in kc:
            core[int(x[0])] = int(x[2])
        name_of = {v: nm for nm, v in vid.items()}
        uv = np.array([[vid[a], vid[b]] for a, b in (tuple(e) for e in edges)], dtype=np.int64).reshape(-1, 2)
        rowptr, col = D.csr_of_edges(nv, uv)
        want = D.densest(rowptr, col, core, iters)

        rows = _rows(out / "densest_subgraph.tsv", ["#VID", "Name", "Coreness", "Load"])
        assert [int(x[0]) for x in rows] == sorted(int(x[0]) for x in rows)        # VID order
        assert all(vid[x[1]] == int(x[0]) for x in rows)
        got = {x[1]: (int(x[2]), int(x[3])) for x in rows}
        members = np.flatnonzero(want["member"])
        assert len(rows) == len(members) == want["n_sub"]
        assert got == {name_of[int(v)]: (int(core[v]), int(want["load"][v])) for v in members}
        assert D.edges_inside(rowptr, col, want["member"]) == want["m_sub"]

        prof = _rows(out / "core_density.tsv", ["#K", "Vertices", "Edges"])
        assert [[int(y) for y in x] for x in prof] == [[k, int(want["n_k"][k]), int(want["m_k"][k])] for k in range(want["k_max"] + 1)]

        # the existing files and stdout are what they are without the variable
        for f in ("kcore.tsv", "CoreA_anomaly.txt", "edgelist.txt"):
            assert (out / f).read_bytes() == (off / f).read_bytes(), f
        mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
        assert mask(stdout_on) == mask(stdout_off).replace(str(off), str(out))
