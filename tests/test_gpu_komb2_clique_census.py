"""komb2 with KOMB_TRUSS=1 and KOMB_CLIQUE_CENSUS=<k_lo>:<k_hi>[:<k_local>] on the generated SAM + FASTA fixture:
clique_census.tsv and clique_census_unitigs.tsv hold, keyed by size and by unitig Name, what the library (and the restatement
of tests/clique_census_ref.py) gives on the truss stage's result; a bad value is refused; without the variable nothing
changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import clique_census_ref as C
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_TRUSS", "KOMB_ONION", "KOMB_NUCLEUS", "KOMB_MAX_CLIQUE", "KOMB_CLIQUE_CENSUS")
NEW = ["clique_census.tsv", "clique_census_unitigs.tsv"]


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("clique_census_komb2")
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


def _reference(s1, s2, threads, k_lo, k_hi, k_local):
    """The census of the truss stage's result (the k-truss of the max-core subgraph), by the library and by Name."""
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
        total, local, info = a.run_clique_census(k_lo, k_hi, k_local)
    want = C.census(nv, su, sv, k_lo, k_hi, k_local)
    assert info["flags"] == 1 == want["flags"] and np.array_equal(total, want["total"]) and np.array_equal(local, want["local"])
    return order, info, total, local


def _read(out, unitigs=True):
    lines = [ln.rstrip("\n") for ln in open(out / "clique_census.tsv")]
    m = re.fullmatch(r"# k_lo (\d+) k_hi (\d+) k_local (\d+) flags (\d+) omega (\d+) nodes (\d+) roots (\d+)", lines[0])
    assert m
    rows = [[int(x) for x in ln.split("\t")] for ln in lines[1:]]
    assert all(len(r) == 2 for r in rows)
    if not unitigs:
        return [int(x) for x in m.groups()], rows, None
    urows = [ln.rstrip("\n").split("\t") for ln in open(out / "clique_census_unitigs.tsv")]
    assert urows[0] == ["#Name", "Count"]
    return [int(x) for x in m.groups()], rows, [(x[0], int(x[1])) for x in urows[1:]]


@pytest.mark.parametrize("threads", [2])
def test_komb2_clique_census_tsv(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    order, info, total, local = _reference(s1, s2, threads, 2, -1, 3)
    assert info["omega"] >= 3 and int(total[1]) >= 1                             # the fixture shows something

    off = tmp_path / "off"
    r_off = _run(d, off, threads, KOMB_TRUSS="1")
    files_off = sorted(os.listdir(off))
    assert not set(NEW) & set(files_off)

    out = tmp_path / "on"
    r_on = _run(d, out, threads, KOMB_CLIQUE_CENSUS="2:max:3", KOMB_TRUSS="1")
    head, rows, urows = _read(out)
    assert head[:5] == [2, info["k_hi"], 3, 1, info["omega"]] and head[5] >= 1 and head[6] >= 1
    assert rows == [[2 + i, int(x)] for i, x in enumerate(total.tolist())]
    # every unitig, in VID order (-t decides the VIDs: the Names are compared as a table)
    assert sorted(urows) == sorted((order[v], int(local[v])) for v in range(len(order)))
    assert sum(c for _, c in urows) == 3 * int(total[1])
    # the existing files and stdout are what they are without the variable
    assert sorted(os.listdir(out)) == sorted(files_off + NEW)
    for f in files_off:
        assert (out / f).read_bytes() == (off / f).read_bytes(), f
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(r_on.stdout) == mask(r_off.stdout).replace(str(off), str(out))

    # a window without a k_local: one table, k_hi as given
    win = tmp_path / "window"
    _run(d, win, threads, KOMB_CLIQUE_CENSUS="3:4", KOMB_TRUSS="1")
    head, rows, _ = _read(win, unitigs=False)
    k_hi = max(3, min(4, info["t_max"]))
    assert head[:3] == [3, k_hi, 0] and rows == [[k, int(total[k - 2])] for k in range(3, k_hi + 1)]
    assert sorted(os.listdir(win)) == sorted(files_off + NEW[:1])


def test_komb2_clique_census_switches(fixture, tmp_path):
    d, _, _ = fixture
    for i, bad in enumerate(("2", "1:3", "3:2", "2:5:6", "2:max:", "2:max:3:4")):
        r = _run(d, tmp_path / f"bad{i}", 2, check=False, KOMB_CLIQUE_CENSUS=bad, KOMB_TRUSS="1")
        assert r.returncode != 0, bad
        assert f"KOMB_CLIQUE_CENSUS={bad}: expected 0 or <k_lo>:<k_hi>[:<k_local>]" in r.stderr, bad
    plain = _run(d, tmp_path / "plain", 2)
    assert sorted(os.listdir(tmp_path / "plain")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv"]
    zero = _run(d, tmp_path / "zero", 2, KOMB_TRUSS="1", KOMB_CLIQUE_CENSUS="0")
    assert sorted(os.listdir(tmp_path / "zero")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv", "truss_unitigs.fasta"]
    # without KOMB_TRUSS=1 there is no truss stage, and so no census
    alone = _run(d, tmp_path / "alone", 2, KOMB_CLIQUE_CENSUS="2:max")
    assert sorted(os.listdir(tmp_path / "alone")) == sorted(os.listdir(tmp_path / "plain"))
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(alone.stdout) == mask(plain.stdout).replace(str(tmp_path / "plain"), str(tmp_path / "alone"))
    assert plain.returncode == 0 and zero.returncode == 0
