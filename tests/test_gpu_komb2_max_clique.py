"""komb2 with KOMB_TRUSS=1 and KOMB_MAX_CLIQUE=1 on the generated SAM + FASTA fixture: max_cliques.tsv and
max_clique_unitigs.tsv hold, keyed by unitig Name, what the library (and the restatement of tests/max_clique_ref.py) gives on the
truss stage's result; a budget that is too small leaves the witness alone; a bad value is refused; without the variable
nothing changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import max_clique_ref as M
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_TRUSS", "KOMB_ONION", "KOMB_NUCLEUS", "KOMB_MAX_CLIQUE")
NEW = ["max_clique_unitigs.tsv", "max_cliques.tsv"]


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("max_clique_komb2")
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


def _reference(s1, s2, threads):
    """The maximum cliques of the truss stage's result (the k-truss of the max-core subgraph), by the library and by Name."""
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
        info, count, _ = a.run_max_clique()
        cliques = a.max_clique_list()
    want = M.solve(nv, su, sv)
    assert info["flags"] == 7 and [tuple(c) for c in cliques.tolist()] == want["cliques"] and np.array_equal(count, want["count"])
    return order, info, count, cliques, su, sv


def _read(out):
    lines = [ln.rstrip("\n") for ln in open(out / "max_cliques.tsv")]
    m = re.fullmatch(r"# omega (\d+) upper (\d+) flags (\d+) cliques (-?\d+)", lines[0])
    assert m
    rows = [ln.split("\t") for ln in lines[1:]]
    urows = [ln.rstrip("\n").split("\t") for ln in open(out / "max_clique_unitigs.tsv")]
    assert urows[0] == ["#Name", "Count"]
    return [int(x) for x in m.groups()], rows, {x[0]: int(x[1]) for x in urows[1:]}, len(urows) - 1


@pytest.mark.parametrize("threads", [2])
def test_komb2_max_clique_tsv(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    order, info, count, cliques, su, sv = _reference(s1, s2, threads)
    assert info["omega"] >= 3 and info["n_max_cliques"] >= 1                     # the fixture shows something

    off = tmp_path / "off"
    r_off = _run(d, off, threads, KOMB_TRUSS="1")
    files_off = sorted(os.listdir(off))
    assert not set(NEW) & set(files_off)

    out = tmp_path / "on"
    r_on = _run(d, out, threads, KOMB_MAX_CLIQUE="1", KOMB_TRUSS="1")
    head, rows, by_name, n_rows = _read(out)
    assert head == [info["omega"], info["upper"], 7, info["n_max_cliques"]]
    assert all(len(r) == info["omega"] for r in rows) and len(rows) == info["n_max_cliques"]
    assert {frozenset(r) for r in rows} == {frozenset(order[v] for v in c) for c in cliques.tolist()}
    assert len({frozenset(r) for r in rows}) == len(rows)
    assert by_name == {order[v]: int(count[v]) for v in np.flatnonzero(count)} and n_rows == len(by_name)
    # the existing files and stdout are what they are without the variable
    assert sorted(os.listdir(out)) == sorted(files_off + NEW)
    for f in files_off:
        assert (out / f).read_bytes() == (off / f).read_bytes(), f
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(r_on.stdout) == mask(r_off.stdout).replace(str(off), str(out))

    # a budget of two nodes: not enumerated, one line with a clique of the result, its unitigs counted once
    cut = tmp_path / "cut"
    _run(d, cut, threads, KOMB_MAX_CLIQUE="2", KOMB_TRUSS="1")
    head, rows, by_name, _ = _read(cut)
    assert not head[2] & 2 and head[3] == -1 and 2 <= head[0] <= info["omega"] <= head[1]
    assert len(rows) == 1 and len(set(rows[0])) == head[0] and by_name == {nm: 1 for nm in rows[0]}
    vid = {nm: i for i, nm in enumerate(order)}
    edges = set(zip(su.tolist(), sv.tolist()))
    w = sorted(vid[nm] for nm in rows[0])
    assert all((w[i], w[j]) in edges for i in range(len(w)) for j in range(i + 1, len(w)))


def test_komb2_max_clique_switches(fixture, tmp_path):
    d, _, _ = fixture
    for i, bad in enumerate(("-1", "1x")):
        r = _run(d, tmp_path / f"bad{i}", 2, check=False, KOMB_MAX_CLIQUE=bad, KOMB_TRUSS="1")
        assert r.returncode != 0
        assert f"KOMB_MAX_CLIQUE={bad}: expected 0, 1 or a node budget" in r.stderr
    plain = _run(d, tmp_path / "plain", 2)
    assert sorted(os.listdir(tmp_path / "plain")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv"]
    zero = _run(d, tmp_path / "zero", 2, KOMB_TRUSS="1", KOMB_MAX_CLIQUE="0")
    assert sorted(os.listdir(tmp_path / "zero")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv", "truss_unitigs.fasta"]
    # without KOMB_TRUSS=1 there is no truss stage, and so no search
    alone = _run(d, tmp_path / "alone", 2, KOMB_MAX_CLIQUE="1")
    assert sorted(os.listdir(tmp_path / "alone")) == sorted(os.listdir(tmp_path / "plain"))
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(alone.stdout) == mask(plain.stdout).replace(str(tmp_path / "plain"), str(tmp_path / "alone"))
    assert plain.returncode == 0 and zero.returncode == 0
