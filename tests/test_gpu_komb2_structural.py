"""komb2 with KOMB_STRUCTURAL on the generated SAM + FASTA fixture: structural_clusters.tsv holds, keyed by unitig Name, what
the restatement of tests/structural_ref.py gives on the whole graph's k-truss result; a malformed value is refused with the
usage line; the truss stage behind it and every other file are what they are without the variable."""
import os
import re
import subprocess

import numpy as np
import pytest

import samgraph
import structural_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_STRUCTURAL", "KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_TRUSS", "KOMB_ONION", "KOMB_HIERARCHY", "KOMB_DENSEST",
        "KOMB_COMMUNITY_HIERARCHY")
ROLES = ("outlier", "hub", "border", "core")
USAGE = "expected <num>/<den>,<mu> with 1 <= num <= den <= 1000000 and mu >= 2"


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("structural_komb2")
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
    (the rows of its kcore.tsv): the Cluster column names the unitig with the smallest VID among a cluster's cores."""
    import komb_amd
    names, edges = samgraph.build_graph(s1, s2, threads)
    order = [ln.split("\t")[1] for ln in list(open(kcore_tsv))[1:]]
    assert sorted(order) == sorted(names)
    vid = {nm: i for i, nm in enumerate(order)}
    uv = np.array([[vid[a], vid[b]] for a, b in (tuple(e) for e in edges)], dtype=np.int64).reshape(-1, 2)
    with komb_amd.KombAccel() as a:
        a.from_edges(len(order), uv)
        eu, ev, _, sup = a.run_truss(with_support=True)
    return order, eu, ev, sup


def _check_file(out, order, eu, ev, sup, params):
    nv = len(order)
    want = R.clusters(nv, eu, ev, sup, *params)
    kc_vid = {x[1]: int(x[0]) for x in (ln.rstrip("\n").split("\t") for ln in list(open(out / "kcore.tsv"))[1:])}
    rows = [ln.rstrip("\n").split("\t") for ln in open(out / "structural_clusters.tsv")]
    assert rows[0] == ["#VID", "Name", "Role", "Cluster", "ClusterSize", "SimilarNeighbours"]
    rows = rows[1:]
    assert len(rows) == nv and [int(x[0]) for x in rows] == list(range(nv))              # one row per unitig, this run's VID order
    assert all(kc_vid[x[1]] == int(x[0]) for x in rows)
    got = {x[1]: (x[2], x[3], int(x[4]), int(x[5])) for x in rows}
    exp = {order[v]: (ROLES[int(want["role"][v])], order[int(want["label"][v])] if want["label"][v] >= 0 else "-",
                      int(want["size"][v]), int(want["sim_deg"][v])) for v in range(nv)}
    assert got == exp
    return want["info"]


@pytest.mark.parametrize("threads", [1, 4])
def test_komb2_structural_tsv(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    off = tmp_path / "off"
    r_off = _run(d, off, threads, KOMB_TRUSS="1")
    order, eu, ev, sup = _reference(s1, s2, threads, off / "kcore.tsv")
    files_off = sorted(os.listdir(off))
    assert "structural_clusters.tsv" not in files_off
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    seen = set()
    for setting, params in (("7/10,3", (7, 10, 3)), ("1/2,3", (1, 2, 3)), ("3/10,2", (3, 10, 2)), ("1000000/1000000,2", (1000000, 1000000, 2))):
        out = tmp_path / ("on_" + setting.replace("/", "_").replace(",", "_"))
        r_on = _run(d, out, threads, KOMB_STRUCTURAL=setting, KOMB_TRUSS="1")
        info = _check_file(out, order, eu, ev, sup, params)
        seen |= {k for k in ("n_cores", "n_borders", "n_hubs", "n_outliers") if info[k] > 0}
        # the truss stage behind it, the other files and stdout are what they are without the variable
        assert sorted(os.listdir(out)) == sorted(files_off + ["structural_clusters.tsv"])
        for f in files_off:
            assert (out / f).read_bytes() == (off / f).read_bytes(), f
        assert mask(r_on.stdout) == mask(r_off.stdout).replace(str(off), str(out))
    assert seen == {"n_cores", "n_borders", "n_hubs", "n_outliers"}                       # the table shows every role somewhere


def test_komb2_structural_switches(fixture, tmp_path):
    d, _, _ = fixture
    for i, bad in enumerate(("abc", "7/10", "7/10,", "7,10,3", "0/10,3", "11/10,3", "7/10,1", "7/10,3x", "-7/10,3", "7/1000001,3", "7/10,99999999999")):
        r = _run(d, tmp_path / f"bad{i}", 2, check=False, KOMB_STRUCTURAL=bad)
        assert r.returncode != 0
        assert f"KOMB_STRUCTURAL={bad}: {USAGE}" in r.stderr
        assert "structural_clusters.tsv" not in os.listdir(tmp_path / f"bad{i}")
    # without the variable the output directory holds exactly the files it holds today; alone, it adds its one table
    plain = _run(d, tmp_path / "plain", 2)
    assert sorted(os.listdir(tmp_path / "plain")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv"]
    alone = _run(d, tmp_path / "alone", 2, KOMB_STRUCTURAL="7/10,3")
    assert sorted(os.listdir(tmp_path / "alone")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv", "structural_clusters.tsv"]
    for f in os.listdir(tmp_path / "plain"):
        assert (tmp_path / "alone" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(alone.stdout) == mask(plain.stdout).replace(str(tmp_path / "plain"), str(tmp_path / "alone"))
