"""komb2 with KOMB_TRUSS=1 and KOMB_NUCLEUS=1 on the generated SAM + FASTA fixture: nucleus_triangles.tsv and
nucleus_unitigs.tsv hold, keyed by unitig Name, what the restatement of tests/nucleus_ref.py gives on the truss stage's
result; a bad value is refused; without the variable nothing changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import nucleus_ref as R
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_TRUSS", "KOMB_ONION", "KOMB_NUCLEUS")
NEW = ["nucleus_triangles.tsv", "nucleus_unitigs.tsv"]


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("nucleus_komb2")
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
    """The truss stage's result (the k-truss of the max-core subgraph) on the graph the SAM files define, by Name."""
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
    return order, nv, su, sv


def _check_files(out, order, nv, su, sv):
    want = R.decompose(nv, su, sv)
    kc_vid = {x[1]: int(x[0]) for x in (ln.rstrip("\n").split("\t") for ln in list(open(out / "kcore.tsv"))[1:])}

    rows = [ln.rstrip("\n").split("\t") for ln in open(out / "nucleus_triangles.tsv")]
    assert rows[0] == ["#Name_A", "Name_B", "Name_C", "Cliques", "Theta"]
    rows = rows[1:]
    assert len(rows) == want["info"]["n_triangles"]
    vids = [tuple(kc_vid[x[i]] for i in range(3)) for x in rows]
    assert vids == sorted(vids) and all(a < b < c for a, b, c in vids)           # triangle order of this run's VIDs
    got = {frozenset(x[:3]): (int(x[3]), int(x[4])) for x in rows}
    assert len(got) == len(rows)
    names = lambda i: frozenset((order[want["a"][i]], order[want["b"][i]], order[want["c"][i]]))
    assert got == {names(i): (int(want["key0"][i]), int(want["theta"][i])) for i in range(len(rows))}

    vrows = [ln.rstrip("\n").split("\t") for ln in open(out / "nucleus_unitigs.tsv")]
    assert vrows[0] == ["#VID", "Name", "Theta"]
    vrows = vrows[1:]
    assert [int(x[0]) for x in vrows] == sorted(int(x[0]) for x in vrows) and all(kc_vid[x[1]] == int(x[0]) for x in vrows)
    inside = sorted(set(su.tolist()) | set(sv.tolist()))                         # one row per vertex of the result
    assert {x[1]: int(x[2]) for x in vrows} == {order[v]: int(want["vertex_theta"][v]) for v in inside}
    assert len(vrows) == len(inside)
    return want


@pytest.mark.parametrize("threads", [1, 4])
def test_komb2_nucleus_tsv(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    order, nv, su, sv = _reference(s1, s2, threads)

    off = tmp_path / "off"
    r_off = _run(d, off, threads, KOMB_TRUSS="1")
    files_off = sorted(os.listdir(off))
    assert not set(NEW) & set(files_off)

    out = tmp_path / "on"
    r_on = _run(d, out, threads, KOMB_NUCLEUS="1", KOMB_TRUSS="1")
    want = _check_files(out, order, nv, su, sv)
    assert want["info"]["n_triangles"] > 0 and want["info"]["n_cliques4"] > 0    # the fixture shows something
    # the existing files and stdout are what they are without the variable
    assert sorted(os.listdir(out)) == sorted(files_off + NEW)
    for f in files_off:
        assert (out / f).read_bytes() == (off / f).read_bytes(), f
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(r_on.stdout) == mask(r_off.stdout).replace(str(off), str(out))


def test_komb2_nucleus_switches(fixture, tmp_path):
    d, _, _ = fixture
    # a bad value exits non-zero with the message
    for i, bad in enumerate(("abc", "2", "-1", "1x", "yes")):
        r = _run(d, tmp_path / f"bad{i}", 2, check=False, KOMB_NUCLEUS=bad, KOMB_TRUSS="1")
        assert r.returncode != 0
        assert f"KOMB_NUCLEUS={bad}: expected 0 or 1" in r.stderr
    # without the variable, or with 0, the output directory holds exactly the files it holds today
    plain = _run(d, tmp_path / "plain", 2)
    assert sorted(os.listdir(tmp_path / "plain")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv"]
    truss = _run(d, tmp_path / "truss", 2, KOMB_TRUSS="1")
    assert sorted(os.listdir(tmp_path / "truss")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv", "truss_unitigs.fasta"]
    zero = _run(d, tmp_path / "zero", 2, KOMB_TRUSS="1", KOMB_NUCLEUS="0")
    assert sorted(os.listdir(tmp_path / "zero")) == sorted(os.listdir(tmp_path / "truss"))
    for f in os.listdir(tmp_path / "truss"):
        assert (tmp_path / "zero" / f).read_bytes() == (tmp_path / "truss" / f).read_bytes(), f
    # without KOMB_TRUSS=1 there is no truss stage, and so no decomposition
    alone = _run(d, tmp_path / "alone", 2, KOMB_NUCLEUS="1")
    assert sorted(os.listdir(tmp_path / "alone")) == sorted(os.listdir(tmp_path / "plain"))
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(alone.stdout) == mask(plain.stdout).replace(str(tmp_path / "plain"), str(tmp_path / "alone"))
    assert plain.returncode == 0 and truss.returncode == 0 and zero.returncode == 0
