"""komb2 with KOMB_TRUSS=1 and KOMB_CLIQUE_COMMUNITIES=<k>[:<budget>] on the generated SAM + FASTA fixture:
clique_communities.tsv and clique_community_unitigs.tsv hold, keyed by unitig Name, what the library (and the restatement of
tests/clique_communities_ref.py) gives on the truss stage's result; the list of a KOMB_MAXIMAL_CLIQUES run is reused when its k_min
allows it; a bad value is refused; without the variable nothing changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import clique_communities_ref as C
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_TRUSS", "KOMB_ONION", "KOMB_NUCLEUS", "KOMB_MAX_CLIQUE", "KOMB_CLIQUE_CENSUS",
        "KOMB_MAXIMAL_CLIQUES", "KOMB_CLIQUE_COMMUNITIES")
NEW = ["clique_communities.tsv", "clique_community_unitigs.tsv"]
MAXIMAL = ["maximal_clique_sizes.tsv", "maximal_clique_unitigs.tsv", "maximal_cliques.tsv"]


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("clique_communities_komb2")
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


def _reference(s1, s2, threads, k):
    """The k-clique communities of the truss stage's result (the k-truss of the max-core subgraph), by the library and by Name."""
    import komb_amd
    names, edges = samgraph.build_graph(s1, s2, threads)
    order = sorted(names)
    vid = {nm: i for i, nm in enumerate(order)}
    uv = np.array([[vid[a], vid[b]] for a, b in (tuple(e) for e in edges)], dtype=np.int64).reshape(-1, 2)
    nv = len(order)
    with komb_amd.KombAccel() as a:
        a.from_edges(nv, uv)
        _, core = a.run_core()
        a.truss_run((core == int(core.max())).astype(np.uint8))
        a.maximal_cliques_run(k)
        offset, verts = a.maximal_cliques_list()
        got = a.run_clique_communities(k)
    cliques = [tuple(verts[offset[i]:offset[i + 1]].tolist()) for i in range(len(offset) - 1)]
    want = C.solve(nv, cliques, k)
    info = got[8]
    assert info["pair_tests"] == C.pair_tests(cliques, k)
    for name in ("n_member_cliques", "n_communities", "largest", "n_covered", "n_overlap"):
        assert info[name] == want[name], name
    for x, name in zip(got[:8], ("label", "size", "rep", "n_cliques", "offset", "verts", "n_comm", "first")):
        assert np.array_equal(x, want[name]), name
    return order, info, want


def _read(out):
    lines = [ln.rstrip("\n") for ln in open(out / "clique_communities.tsv")]
    m = re.fullmatch(r"# k (\d+) communities (\d+) member_cliques (\d+) covered (\d+) overlap (\d+) pair_tests (\d+)", lines[0])
    assert m
    rows = [ln.split("\t") for ln in lines[1:]]
    assert [int(r[0]) for r in rows] == list(range(len(rows))) and all(int(r[2]) == len(r) - 3 for r in rows)
    urows = [ln.rstrip("\n").split("\t") for ln in open(out / "clique_community_unitigs.tsv")]
    assert urows[0] == ["#Name", "Communities", "First"]
    return [int(x) for x in m.groups()], [(int(r[1]), frozenset(r[3:])) for r in rows], [(x[0], int(x[1]), int(x[2])) for x in urows[1:]]


def _same_communities(rows, urows, order, want):
    """-t decides the VIDs, and with them the list order and the community numbers: the communities compare as sets of Names with
    their clique counts, the unitigs by their number of communities."""
    mine = sorted((int(n), sorted(order[v] for v in c)) for n, c in zip(want["n_cliques"].tolist(), want["communities"]))
    assert sorted((n, sorted(c)) for n, c in rows) == mine
    assert sorted((nm, n) for nm, n, _ in urows) == sorted((order[v], int(want["n_comm"][v])) for v in range(len(order)) if want["n_comm"][v] > 0)
    for nm, _, first in urows:                                                   # First is the smallest number among the rows that hold the Name
        assert first == min(c for c, (_, names) in enumerate(rows) if nm in names)


@pytest.mark.parametrize("threads", [2])
def test_komb2_clique_communities_tsv(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    # the max core of the fixture is dense: 69 292 maximal cliques of 11 .. 33 unitigs, 804 of them of at least 31
    k = 31
    order, info, want = _reference(s1, s2, threads, k)
    assert 2 <= info["n_member_cliques"] <= 3000 and info["n_communities"] >= 1   # the fixture shows something, the restatement stays quick

    off = tmp_path / "off"
    r_off = _run(d, off, threads, KOMB_TRUSS="1")
    files_off = sorted(os.listdir(off))
    assert not set(NEW) & set(files_off)

    out = tmp_path / "on"
    r_on = _run(d, out, threads, KOMB_CLIQUE_COMMUNITIES=str(k), KOMB_TRUSS="1")
    head, rows, urows = _read(out)
    # (pair_tests counts positions in the list and breaks ties by VID, and -t decides the VIDs: it is compared between runs of komb2)
    assert head[:5] == [k, info["n_communities"], info["n_member_cliques"], info["n_covered"], info["n_overlap"]] and head[5] >= 0
    _same_communities(rows, urows, order, want)
    # the existing files and stdout are what they are without the variable
    assert sorted(os.listdir(out)) == sorted(files_off + NEW)
    for f in files_off:
        assert (out / f).read_bytes() == (off / f).read_bytes(), f
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(r_on.stdout) == mask(r_off.stdout).replace(str(off), str(out))

    # the list of a KOMB_MAXIMAL_CLIQUES run with a k_min <= k is used as it stands: more cliques in it, the same communities
    reuse = tmp_path / "reuse"
    _run(d, reuse, threads, KOMB_CLIQUE_COMMUNITIES=str(k), KOMB_MAXIMAL_CLIQUES=str(k - 1), KOMB_TRUSS="1")
    assert sorted(os.listdir(reuse)) == sorted(files_off + NEW + MAXIMAL)
    head2, rows2, urows2 = _read(reuse)
    assert head2[:5] == head[:5]
    _same_communities(rows2, urows2, order, want)
    assert open(reuse / "maximal_cliques.tsv").readline().startswith("# k_min %d flags 3 " % (k - 1))
    # a KOMB_MAXIMAL_CLIQUES run with a larger k_min lacks member cliques: the communities come from a run of their own
    both = tmp_path / "both"
    _run(d, both, threads, KOMB_CLIQUE_COMMUNITIES=str(k), KOMB_MAXIMAL_CLIQUES=str(k + 1), KOMB_TRUSS="1")
    assert _read(both) == (head, rows, urows)
    assert open(both / "maximal_cliques.tsv").readline().startswith("# k_min %d flags 3 " % (k + 1))
    # a budget below pair_tests: the library refuses, komb2 says so and fails
    r = _run(d, tmp_path / "cut", threads, check=False, KOMB_CLIQUE_COMMUNITIES="%d:1" % k, KOMB_TRUSS="1")
    assert r.returncode != 0 and "komb_clique_communities_run" in r.stderr and "budget" in r.stderr


def test_komb2_clique_communities_switches(fixture, tmp_path):
    d, _, _ = fixture
    for i, bad in enumerate(("1", "x", "3:", "3:0", "3:5:6", "-3", "3:x")):
        r = _run(d, tmp_path / f"bad{i}", 2, check=False, KOMB_CLIQUE_COMMUNITIES=bad, KOMB_TRUSS="1")
        assert r.returncode != 0, bad
        assert f"KOMB_CLIQUE_COMMUNITIES={bad}: expected 0 or <k>[:<budget>]" in r.stderr, bad
    plain = _run(d, tmp_path / "plain", 2)
    assert sorted(os.listdir(tmp_path / "plain")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv"]
    zero = _run(d, tmp_path / "zero", 2, KOMB_TRUSS="1", KOMB_CLIQUE_COMMUNITIES="0")
    assert sorted(os.listdir(tmp_path / "zero")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv", "truss_unitigs.fasta"]
    # without KOMB_TRUSS=1 there is no truss stage, and so no communities
    alone = _run(d, tmp_path / "alone", 2, KOMB_CLIQUE_COMMUNITIES="3")
    assert sorted(os.listdir(tmp_path / "alone")) == sorted(os.listdir(tmp_path / "plain"))
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(alone.stdout) == mask(plain.stdout).replace(str(tmp_path / "plain"), str(tmp_path / "alone"))
    assert plain.returncode == 0 and zero.returncode == 0
