"""komb2 with KOMB_TRUSS=1 and KOMB_MAXIMAL_CLIQUES=<k_min>[:<budget>] on the generated SAM + FASTA fixture:
maximal_cliques.tsv, maximal_clique_sizes.tsv and maximal_clique_unitigs.tsv hold, keyed by size and by unitig Name, what the
library (and the restatement of tests/maximal_cliques_ref.py) gives on the truss stage's result; a bad value is refused; without
the variable nothing changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import maximal_cliques_ref as M
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_TRUSS", "KOMB_ONION", "KOMB_NUCLEUS", "KOMB_MAX_CLIQUE", "KOMB_CLIQUE_CENSUS",
        "KOMB_MAXIMAL_CLIQUES")
NEW = ["maximal_clique_sizes.tsv", "maximal_clique_unitigs.tsv", "maximal_cliques.tsv"]


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("maximal_cliques_komb2")
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


def _reference(s1, s2, threads, k_min):
    """The maximal cliques of the truss stage's result (the k-truss of the max-core subgraph), by the library and by Name."""
    import komb_amd
    names, edges = samgraph.build_graph(s1, s2, threads)
    order = sorted(names)
    vid = {nm: i for i, nm in enumerate(order)}
    uv = np.array([[vid[a], vid[b]] for a, b in (tuple(e) for e in edges)], dtype=np.int64).reshape(-1, 2)
    nv = len(order)
    with komb_amd.KombAccel() as a:
        a.from_edges(nv, uv)
        _, core = a.run_core()
        su, sv, _ = a.run_truss((core == int(core.max())).astype(np.uint8))
        hist, count, largest, info = a.run_maximal_cliques(k_min)
        offset, verts = a.maximal_cliques_list()
    want = M.solve(nv, su, sv, k_min)
    cliques = [tuple(verts[offset[i]:offset[i + 1]].tolist()) for i in range(len(offset) - 1)]
    assert info["flags"] == 3 == want["flags"] and np.array_equal(hist, want["hist"]) and cliques == want["cliques"]
    assert np.array_equal(count, want["count"]) and np.array_equal(largest, want["largest"])
    return order, info, hist, count, largest, cliques


def _read(out):
    lines = [ln.rstrip("\n") for ln in open(out / "maximal_cliques.tsv")]
    m = re.fullmatch(r"# k_min (\d+) flags (\d+) omega (\d+) cliques (\d+) nodes (\d+) roots (\d+)", lines[0])
    assert m
    rows = [ln.split("\t") for ln in lines[1:]]
    assert all(int(r[0]) == len(r) - 1 for r in rows)
    sizes = [[int(x) for x in ln.split("\t")] for ln in open(out / "maximal_clique_sizes.tsv")]
    assert all(len(r) == 2 for r in sizes)
    urows = [ln.rstrip("\n").split("\t") for ln in open(out / "maximal_clique_unitigs.tsv")]
    assert urows[0] == ["#Name", "Count", "Largest"]
    return [int(x) for x in m.groups()], [frozenset(r[1:]) for r in rows], sizes, [(x[0], int(x[1]), int(x[2])) for x in urows[1:]]


@pytest.mark.parametrize("threads", [2])
def test_komb2_maximal_cliques_tsv(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    # the max core of the fixture is dense: 69 292 maximal cliques of 11 .. 33 unitigs, 10 629 of them of at least 28
    k_min = 28
    order, info, hist, count, largest, cliques = _reference(s1, s2, threads, k_min)
    assert info["omega"] > k_min and 2 <= info["n_cliques"] <= 65536             # the fixture shows something, and the list is held

    off = tmp_path / "off"
    r_off = _run(d, off, threads, KOMB_TRUSS="1")
    files_off = sorted(os.listdir(off))
    assert not set(NEW) & set(files_off)

    out = tmp_path / "on"
    r_on = _run(d, out, threads, KOMB_MAXIMAL_CLIQUES=str(k_min), KOMB_TRUSS="1")
    head, rows, sizes, urows = _read(out)
    assert head[:4] == [k_min, 3, info["omega"], info["n_cliques"]] and head[4] >= info["n_cliques"] and head[5] >= 1
    # -t decides the VIDs: the cliques are compared as sets of Names, the unitigs as a table
    assert len(rows) == len(cliques) and sorted(map(sorted, rows)) == sorted(sorted(order[v] for v in c) for c in cliques)
    assert sizes == [[k_min + i, int(x)] for i, x in enumerate(hist.tolist())]
    assert sorted(urows) == sorted((order[v], int(count[v]), int(largest[v])) for v in range(len(order)) if count[v] > 0)
    assert sum(c for _, c, _ in urows) == sum(k * n for k, n in sizes)
    # the existing files and stdout are what they are without the variable
    assert sorted(os.listdir(out)) == sorted(files_off + NEW)
    for f in files_off:
        assert (out / f).read_bytes() == (off / f).read_bytes(), f
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(r_on.stdout) == mask(r_off.stdout).replace(str(off), str(out))

    # a budget that cuts the run short: the header alone, the other two tables as far as the run came
    cut = tmp_path / "cut"
    _run(d, cut, threads, KOMB_MAXIMAL_CLIQUES="%d:1" % (k_min + 2), KOMB_TRUSS="1")
    head, rows, sizes, urows = _read(cut)
    assert head[:2] == [k_min + 2, 0] and rows == [] and [k for k, _ in sizes] == list(range(k_min + 2, info["k_hi"] + 1))
    assert all(n <= int(hist[k - k_min]) for k, n in sizes) and sum(n for _, n in sizes) == head[3]
    assert sum(c for _, c, _ in urows) == sum(k * n for k, n in sizes)
    # more cliques than the list keeps (k_min = 2: all of them): complete, the header alone again, the sizes in full
    full = tmp_path / "full"
    _run(d, full, threads, KOMB_MAXIMAL_CLIQUES="2", KOMB_TRUSS="1")
    head, rows, sizes, urows = _read(full)
    assert head[:3] == [2, 1, info["omega"]] and head[3] > 65536 and rows == []
    assert sizes[k_min - 2:] == [[k_min + i, int(x)] for i, x in enumerate(hist.tolist())] and sum(n for _, n in sizes) == head[3]


def test_komb2_maximal_cliques_switches(fixture, tmp_path):
    d, _, _ = fixture
    for i, bad in enumerate(("1", "x", "2:", "2:0", "2:5:6", "-3", "2:x")):
        r = _run(d, tmp_path / f"bad{i}", 2, check=False, KOMB_MAXIMAL_CLIQUES=bad, KOMB_TRUSS="1")
        assert r.returncode != 0, bad
        assert f"KOMB_MAXIMAL_CLIQUES={bad}: expected 0 or <k_min>[:<budget>]" in r.stderr, bad
    plain = _run(d, tmp_path / "plain", 2)
    assert sorted(os.listdir(tmp_path / "plain")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv"]
    zero = _run(d, tmp_path / "zero", 2, KOMB_TRUSS="1", KOMB_MAXIMAL_CLIQUES="0")
    assert sorted(os.listdir(tmp_path / "zero")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv", "truss_unitigs.fasta"]
    # without KOMB_TRUSS=1 there is no truss stage, and so no cliques
    alone = _run(d, tmp_path / "alone", 2, KOMB_MAXIMAL_CLIQUES="2")
    assert sorted(os.listdir(tmp_path / "alone")) == sorted(os.listdir(tmp_path / "plain"))
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(alone.stdout) == mask(plain.stdout).replace(str(tmp_path / "plain"), str(tmp_path / "alone"))
    assert plain.returncode == 0 and zero.returncode == 0
