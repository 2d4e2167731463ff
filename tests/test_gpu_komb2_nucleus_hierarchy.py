"""komb2 with KOMB_TRUSS=1 and KOMB_NUCLEUS_HIERARCHY=1 on the generated SAM + FASTA fixture: nucleus_hierarchy.tsv and
nucleus_hierarchy_triangles.tsv hold, keyed by unitig Name, what tests/nucleus_hierarchy_ref.py gives on the truss stage's
result; a bad value is refused; without the variable nothing changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import nucleus_hierarchy_ref as R
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_TRUSS", "KOMB_ONION", "KOMB_NUCLEUS", "KOMB_NUCLEUS_HIERARCHY")
NEW = ["nucleus_hierarchy.tsv", "nucleus_hierarchy_triangles.tsv"]
NUC = ["nucleus_triangles.tsv", "nucleus_unitigs.tsv"]


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("nucleus_hierarchy_komb2")
    fasta, s1, s2 = samgraph.make_fixture(1000, 6000, seed=1)
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
    """Both tables by Name.  The run numbers its unitigs by its own VIDs, so triangle ids, reps and node numbers differ from the
    reference's: a node is identified by (Theta, the Names of its triangles)."""
    h, dec = R.hierarchy(nv, su, sv)
    tri_names = [frozenset((order[dec["a"][i]], order[dec["b"][i]], order[dec["c"][i]])) for i in range(len(dec["theta"]))]

    trows = [ln.rstrip("\n").split("\t") for ln in open(out / "nucleus_hierarchy_triangles.tsv")]
    assert trows[0] == ["#Name_A", "Name_B", "Name_C", "Theta", "Node"]
    trows = trows[1:]
    members = [i for i in range(len(tri_names)) if dec["theta"][i] >= 1]
    assert len(trows) == len(members)
    got_theta = {frozenset(x[:3]): int(x[3]) for x in trows}
    got_node = {frozenset(x[:3]): int(x[4]) for x in trows}
    assert len(got_theta) == len(trows)
    assert got_theta == {tri_names[i]: int(dec["theta"][i]) for i in members}

    rows = [ln.rstrip("\n").split("\t") for ln in open(out / "nucleus_hierarchy.tsv")]
    assert rows[0] == ["#Node", "Theta", "Rep_A", "Rep_B", "Rep_C", "Parent", "Triangles", "Shell", "Edges", "Vertices"]
    rows = rows[1:]
    assert len(rows) == len(h["k"]) and [int(x[0]) for x in rows] == list(range(len(rows)))
    assert [int(x[1]) for x in rows] == sorted(int(x[1]) for x in rows)          # ascending Theta
    assert all(int(x[5]) < int(x[0]) for x in rows)

    def node_sets(kk, parent, shell_of):
        """node -> (level, the Names of all its triangles): its shell and its children's sets."""
        sets = [set(shell_of(j)) for j in range(len(kk))]
        for j in reversed(range(len(kk))):                                       # parents have smaller numbers
            if parent[j] >= 0:
                sets[parent[j]] |= sets[j]
        return [(int(kk[j]), frozenset(sets[j])) for j in range(len(kk))]

    shells_got = {}
    for name, nd in got_node.items():
        shells_got.setdefault(nd, []).append(name)
    shells_want = {}
    for i in members:
        shells_want.setdefault(int(h["node"][i]), []).append(tri_names[i])
    got_sets = node_sets([int(x[1]) for x in rows], [int(x[5]) for x in rows], lambda j: shells_got.get(j, []))
    want_sets = node_sets(h["k"], h["parent"].tolist(), lambda j: shells_want.get(j, []))
    index = {s: j for j, s in enumerate(want_sets)}
    assert len(index) == len(want_sets) and len(set(got_sets)) == len(got_sets)  # a node is its (level, triangles)
    assert set(got_sets) == set(index)
    per_level = {k: R.nuclei(h, dec, k) for k in set(h["k"].tolist())}
    for x, s in zip(rows, got_sets):
        j = index[s]
        nuc = per_level[int(h["k"][j])]
        at = int(np.searchsorted(nuc["rep"], h["rep"][j]))
        assert frozenset(x[2:5]) in s[1]                                         # the rep triangle lies in the node
        assert (int(x[6]), int(x[7])) == (int(h["size"][j]), int(h["shell"][j])) and int(x[6]) == len(s[1])
        assert (int(x[8]), int(x[9])) == (int(nuc["n_edges"][at]), int(nuc["n_vertices"][at]))
        p = int(x[5])
        assert (got_sets[p] if p >= 0 else None) == (want_sets[h["parent"][j]] if h["parent"][j] >= 0 else None)
    return h, dec


@pytest.mark.parametrize("threads", [1, 4])
def test_komb2_nucleus_hierarchy_tsv(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    order, nv, su, sv = _reference(s1, s2, threads)

    off = tmp_path / "off"
    r_off = _run(d, off, threads, KOMB_TRUSS="1")
    files_off = sorted(os.listdir(off))
    assert not set(NEW) & set(files_off)

    out = tmp_path / "on"
    r_on = _run(d, out, threads, KOMB_NUCLEUS_HIERARCHY="1", KOMB_TRUSS="1")     # (runs the decomposition itself)
    h, dec = _check_files(out, order, nv, su, sv)
    assert len(h["k"]) > 0 and dec["info"]["n_cliques4"] > 0                     # the fixture shows something
    # the existing files and stdout are what they are without the variable
    assert sorted(os.listdir(out)) == sorted(files_off + NEW)
    for f in files_off:
        assert (out / f).read_bytes() == (off / f).read_bytes(), f
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(r_on.stdout) == mask(r_off.stdout).replace(str(off), str(out))

    both = tmp_path / "both"                                                     # with KOMB_NUCLEUS=1: its tables too, the same forest
    _run(d, both, threads, KOMB_NUCLEUS_HIERARCHY="1", KOMB_NUCLEUS="1", KOMB_TRUSS="1")
    assert sorted(os.listdir(both)) == sorted(files_off + NEW + NUC)
    for f in NEW:
        assert (both / f).read_bytes() == (out / f).read_bytes(), f


def test_komb2_nucleus_hierarchy_switches(fixture, tmp_path):
    d, _, _ = fixture
    # a bad value exits non-zero with the message
    for i, bad in enumerate(("abc", "2", "-1", "1x", "yes")):
        r = _run(d, tmp_path / f"bad{i}", 2, check=False, KOMB_NUCLEUS_HIERARCHY=bad, KOMB_TRUSS="1")
        assert r.returncode != 0
        assert f"KOMB_NUCLEUS_HIERARCHY={bad}: expected 0 or 1" in r.stderr
    # without the variable, or with 0, the output directory holds exactly the files it holds today
    plain = _run(d, tmp_path / "plain", 2)
    assert sorted(os.listdir(tmp_path / "plain")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv"]
    truss = _run(d, tmp_path / "truss", 2, KOMB_TRUSS="1")
    assert sorted(os.listdir(tmp_path / "truss")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv", "truss_unitigs.fasta"]
    zero = _run(d, tmp_path / "zero", 2, KOMB_TRUSS="1", KOMB_NUCLEUS_HIERARCHY="0")
    assert sorted(os.listdir(tmp_path / "zero")) == sorted(os.listdir(tmp_path / "truss"))
    for f in os.listdir(tmp_path / "truss"):
        assert (tmp_path / "zero" / f).read_bytes() == (tmp_path / "truss" / f).read_bytes(), f
    # without KOMB_TRUSS=1 there is no truss stage, and so no forest
    alone = _run(d, tmp_path / "alone", 2, KOMB_NUCLEUS_HIERARCHY="1")
    assert sorted(os.listdir(tmp_path / "alone")) == sorted(os.listdir(tmp_path / "plain"))
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(alone.stdout) == mask(plain.stdout).replace(str(tmp_path / "plain"), str(tmp_path / "alone"))
    assert plain.returncode == 0 and truss.returncode == 0 and zero.returncode == 0
