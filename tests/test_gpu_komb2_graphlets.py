"""komb2 with KOMB_GRAPHLETS on the generated SAM + FASTA fixture: graphlet_orbits.tsv, graphlet_census.tsv and (edges)
graphlet_edges.tsv hold, keyed by unitig Name, what census() of tests/graphlets_ref.py gives on the whole graph's k-truss
result; any other value is refused with the usage line; the truss stage behind it and every other file are what they are
without the variable."""
import os
import re
import subprocess

import numpy as np
import pytest

import samgraph
from graphlets_ref import ORBITS, TYPES, census

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_GRAPHLETS", "KOMB_STRUCTURAL", "KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_TRUSS", "KOMB_ONION", "KOMB_HIERARCHY",
        "KOMB_DENSEST", "KOMB_COMMUNITY_HIERARCHY")
USAGE = "expected 1 or edges"
TABLES = ["graphlet_census.tsv", "graphlet_orbits.tsv"]


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("graphlets_komb2")
    fasta, s1, s2 = samgraph.make_fixture(2000, 20000, seed=1)
    (d / "unitigs.l-1.fasta").write_bytes(fasta)
    (d / "reads1.fastq.sam").write_bytes(s1)
    (d / "reads2.fastq.sam").write_bytes(s2)
    return d, s1, s2


def _run(d, out, threads, check=True, **env_add):
    out.mkdir()
    cmd = [KOMB2, "-t", str(threads), "-l", "-1", "-o", str(out), "-i", f"{d}/reads1.fastq.sam", "-j", f"{d}/reads2.fastq.sam",
           "-u", f"{d}/unitigs.l-1.fasta"]
    env = {k: v for k, v in os.environ.items() if k not in VARS}
    env.update(env_add)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if check:
        assert r.returncode == 0, r.stderr
    return r


def _reference(s1, s2, threads, kcore_tsv):
    """The whole graph's k-truss result on the graph the SAM files define, in the VIDs of a komb2 run with as many threads
    (the rows of its kcore.tsv), and its census."""
    import komb_amd
    names, edges = samgraph.build_graph(s1, s2, threads)
    order = [ln.split("\t")[1] for ln in list(open(kcore_tsv))[1:]]
    assert sorted(order) == sorted(names)
    vid = {nm: i for i, nm in enumerate(order)}
    uv = np.array([[vid[a], vid[b]] for a, b in (tuple(e) for e in edges)], dtype=np.int64).reshape(-1, 2)
    with komb_amd.KombAccel() as a:
        a.from_edges(len(order), uv)
        eu, ev, _, sup = a.run_truss(with_support=True)
    want = census(len(order), eu, ev)
    assert np.array_equal(want["sup"], sup)
    return order, eu, ev, want


def _check_files(out, order, eu, ev, want, with_edges):
    nv = len(order)
    kc_vid = {x[1]: int(x[0]) for x in (ln.rstrip("\n").split("\t") for ln in list(open(out / "kcore.tsv"))[1:])}
    rows = [ln.rstrip("\n").split("\t") for ln in open(out / "graphlet_orbits.tsv")]
    assert rows[0] == ["#VID", "Name"] + ["O%d" % o for o in range(ORBITS)]
    rows = rows[1:]
    assert len(rows) == nv and [int(x[0]) for x in rows] == list(range(nv))              # one row per unitig, this run's VID order
    assert all(kc_vid[x[1]] == int(x[0]) for x in rows)
    got = {x[1]: [int(y) for y in x[2:]] for x in rows}
    assert got == {order[v]: [int(want["orbit"][o, v]) for o in range(ORBITS)] for v in range(nv)}
    rows = [ln.rstrip("\n").split("\t") for ln in open(out / "graphlet_census.tsv")]
    assert rows[0] == ["#Graphlet", "Count"]
    assert [(x[0], int(x[1])) for x in rows[1:]] == [(t, want["total"][t]) for t in TYPES]
    if with_edges:
        rows = [ln.rstrip("\n").split("\t") for ln in open(out / "graphlet_edges.tsv")]
        assert rows[0] == ["#U", "V", "Triangles", "Cycles4", "Cliques4"]
        assert [(x[0], x[1], int(x[2]), int(x[3]), int(x[4])) for x in rows[1:]] == [
            (order[int(eu[i])], order[int(ev[i])], int(want["sup"][i]), int(want["cycles4"][i]), int(want["cliques4"][i]))
            for i in range(len(eu))]                                                     # canonical order


@pytest.mark.parametrize("threads", [1, 4])
def test_komb2_graphlet_tables(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    off = tmp_path / "off"
    r_off = _run(d, off, threads, KOMB_TRUSS="1")
    order, eu, ev, want = _reference(s1, s2, threads, off / "kcore.tsv")
    files_off = sorted(os.listdir(off))
    assert not any(f.startswith("graphlet_") for f in files_off)
    assert want["total"]["triangle"] > 0 and want["total"]["cycle4"] > 0 and want["total"]["claw"] > 0    # the tables show something
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    for setting, extra in (("1", []), ("edges", ["graphlet_edges.tsv"])):
        out = tmp_path / ("on_" + setting)
        r_on = _run(d, out, threads, KOMB_GRAPHLETS=setting, KOMB_TRUSS="1")
        _check_files(out, order, eu, ev, want, bool(extra))
        # the truss stage behind it, the other files and stdout are what they are without the variable
        assert sorted(os.listdir(out)) == sorted(files_off + TABLES + extra)
        for f in files_off:
            assert (out / f).read_bytes() == (off / f).read_bytes(), f
        assert mask(r_on.stdout) == mask(r_off.stdout).replace(str(off), str(out))


def test_komb2_graphlet_switches(fixture, tmp_path):
    d, _, _ = fixture
    for i, bad in enumerate(("0", "2", "abc", "edges,1")):
        r = _run(d, tmp_path / f"bad{i}", 2, check=False, KOMB_GRAPHLETS=bad)
        assert r.returncode != 0
        assert f"KOMB_GRAPHLETS={bad}: {USAGE}" in r.stderr
        assert not any(f.startswith("graphlet_") for f in os.listdir(tmp_path / f"bad{i}"))
    # without the variable the output directory holds exactly the files it holds today; alone, it adds its tables
    plain = _run(d, tmp_path / "plain", 2)
    assert sorted(os.listdir(tmp_path / "plain")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv"]
    alone = _run(d, tmp_path / "alone", 2, KOMB_GRAPHLETS="1")
    assert sorted(os.listdir(tmp_path / "alone")) == sorted(["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv"] + TABLES)
    for f in os.listdir(tmp_path / "plain"):
        assert (tmp_path / "alone" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(alone.stdout) == mask(plain.stdout).replace(str(tmp_path / "plain"), str(tmp_path / "alone"))
