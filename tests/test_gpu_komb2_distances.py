"""komb2 with KOMB_DISTANCES on the generated SAM + FASTA fixture: distances.tsv, distance_sources.tsv and
distance_histogram.tsv read back hold exactly what tests/distances_ref.py gives on the graph the SAM files define from the sources
the switch names (every unitig, or the splitmix64 sample of KOMB_BETWEENNESS, recomputed here) -- Harmonic read back with float()
bit for bit; a malformed value is refused with the usage line; without the variable no file appears, and every other file is
what it is without it."""
import os
import re
import subprocess

import numpy as np
import pytest

import betweenness_ref as B
import distances_ref as R
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_DISTANCES", "KOMB_BETWEENNESS", "KOMB_GRAPHLETS", "KOMB_STRUCTURAL", "KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_TRUSS",
        "KOMB_ONION", "KOMB_HIERARCHY", "KOMB_DENSEST", "KOMB_COMMUNITY_HIERARCHY")
USAGE = "expected all or <n>[:<seed>]"
TABLES = ["distances.tsv", "distance_sources.tsv", "distance_histogram.tsv"]
PLAIN = ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv"]


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("distances_komb2")
    fasta, s1, s2 = samgraph.make_fixture(600, 6000, seed=1)
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


def _graph(s1, s2, threads, kcore_tsv):
    """The rows of the graph the SAM files define, in the VIDs of a komb2 run with as many threads (the rows of its kcore.tsv)."""
    names, edges = samgraph.build_graph(s1, s2, threads)
    order = [ln.split("\t")[1] for ln in list(open(kcore_tsv))[1:]]
    assert sorted(order) == sorted(names)
    vid = {nm: i for i, nm in enumerate(order)}
    return order, R.adjacency(len(order), [[vid[a], vid[b]] for a, b in (tuple(e) for e in edges)])


def _table(path, header):
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert rows[0] == header
    return rows[1:]


def _check_files(out, order, want):
    nv = len(order)
    rows = _table(out / "distances.tsv", ["#VID", "Name", "Reached", "SumDist", "Ecc", "Harmonic"])
    assert [int(x[0]) for x in rows] == list(range(nv)) and [x[1] for x in rows] == order      # one row per unitig in VID order
    for col, name in ((2, "n_reached"), (3, "sum_dist"), (4, "ecc")):
        assert [int(x[col]) for x in rows] == want[name].tolist(), name
    got = np.asarray([float(x[5]) for x in rows], dtype=np.float64)
    assert np.array_equal(R.bits(got), R.bits(want["harmonic"]))
    per = want["sources"]
    rows = _table(out / "distance_sources.tsv", ["#VID", "Name", "Reached", "SumDist", "Ecc"])
    assert [(int(x[0]), x[1], int(x[2]), int(x[3]), int(x[4])) for x in rows] == [
        (int(s), order[int(s)], int(per["n_reached"][i]), int(per["sum_dist"][i]), int(per["ecc"][i])) for i, s in enumerate(per["source"])]
    rows = _table(out / "distance_histogram.tsv", ["#Distance", "Pairs"])
    assert [(int(x[0]), int(x[1])) for x in rows] == list(enumerate(want["pairs"].tolist()))


@pytest.mark.parametrize("threads", [1, 4])
def test_komb2_distances_tables(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    off = tmp_path / "off"
    r_off = _run(d, off, threads)
    order, rows = _graph(s1, s2, threads, off / "kcore.tsv")
    nv = len(order)
    assert sorted(os.listdir(off)) == PLAIN
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    cache = {}
    for setting, sources in (("all", None), ("5:7", B.sample_sources(nv, 5, 7)), ("3", B.sample_sources(nv, 3, 1)), (str(nv + 9), None)):
        want = R.distances(rows, sources, cache=cache)
        if setting == "all":
            assert (want["harmonic"] != np.floor(want["harmonic"])).any()      # values whose digits matter
            assert (want["ecc"] >= 0).all()
        out = tmp_path / ("on_" + setting.replace(":", "_"))
        r_on = _run(d, out, threads, KOMB_DISTANCES=setting)
        _check_files(out, order, want)
        # the other files and stdout are what they are without the variable
        assert sorted(os.listdir(out)) == sorted(PLAIN + TABLES)
        for f in PLAIN:
            assert (out / f).read_bytes() == (off / f).read_bytes(), f
        assert mask(r_on.stdout) == mask(r_off.stdout).replace(str(off), str(out))


def test_komb2_distances_switches(fixture, tmp_path):
    d, s1, s2 = fixture
    for i, bad in enumerate(("1x", "-3", "5:", "all:2", "5:7:9")):
        r = _run(d, tmp_path / f"bad{i}", 2, check=False, KOMB_DISTANCES=bad)
        assert r.returncode != 0
        assert f"KOMB_DISTANCES={bad}: {USAGE}" in r.stderr
        assert not any(f.startswith("distance") for f in os.listdir(tmp_path / f"bad{i}"))
    _run(d, tmp_path / "zero", 2, KOMB_DISTANCES="0")                          # no source: nothing reached, an empty source table
    lines = list(open(tmp_path / "zero" / "distances.tsv"))[1:]
    assert lines and all(ln.rstrip("\n").split("\t")[2:] == ["0", "0", "-1", "0"] for ln in lines)
    assert list(open(tmp_path / "zero" / "distance_sources.tsv")) == ["#VID\tName\tReached\tSumDist\tEcc\n"]
    assert list(open(tmp_path / "zero" / "distance_histogram.tsv")) == ["#Distance\tPairs\n", "0\t0\n"]
    # the same value names the same sources to both switches
    _run(d, tmp_path / "both", 2, KOMB_DISTANCES="6:3", KOMB_BETWEENNESS="6:3")
    ours, theirs = (list(open(tmp_path / "both" / f)) for f in ("distance_sources.tsv", "betweenness_sources.tsv"))
    assert ours == theirs and len(ours) == 7
