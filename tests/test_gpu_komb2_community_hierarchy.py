"""komb2 with KOMB_TRUSS=1 KOMB_COMMUNITY_HIERARCHY=1 on the generated SAM + FASTA fixture: truss_community_hierarchy.tsv and
truss_community_hierarchy_edges.tsv hold, by unitig Name, the forest of the reference (tests/community_hierarchy_ref.py) on
the graph the SAM files define; without the variable nothing changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import community_hierarchy_ref as CH
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_COMMUNITY_HIERARCHY", "KOMB_HIERARCHY", "KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_TRUSS", "KOMB_ONION")
FILES = ("truss_community_hierarchy.tsv", "truss_community_hierarchy_edges.tsv")


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("community_hierarchy_komb2")
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


def _by_name(k, parent, size, shell, node_of_edge):
    """A forest without its numbering: {(K, edge set S by Name)} -> (parent's (K, S) or None, size, shell), S put together
    from the shells of the node and of everything below it.  node_of_edge: {frozenset of two Names: node}."""
    n = len(k)
    own = [set() for _ in range(n)]
    for e, i in node_of_edge.items():
        own[i].add(e)
    for i in range(n - 1, -1, -1):                       # parent[i] < i: children first
        if parent[i] >= 0:
            own[parent[i]] |= own[i]
    key = [(k[i], frozenset(own[i])) for i in range(n)]
    assert len(set(key)) == n
    return {key[i]: (key[parent[i]] if parent[i] >= 0 else None, size[i], shell[i]) for i in range(n)}


@pytest.mark.parametrize("threads", [1, 4])
def test_komb2_community_hierarchy_tsv(fixture, tmp_path, threads):
    import komb_amd
    d, s1, s2 = fixture
    names, edges = samgraph.build_graph(s1, s2, threads)
    order = sorted(names)
    vid = {nm: i for i, nm in enumerate(order)}
    uv = np.array([[vid[a], vid[b]] for a, b in (tuple(e) for e in edges)], dtype=np.int64).reshape(-1, 2)
    nv = len(order)
    with komb_amd.KombAccel() as a:
        a.from_edges(nv, uv)
        _, core = a.run_core()
        su, sv, st = a.run_truss((core == int(core.max())).astype(np.uint8))
    want = CH.community_hierarchy(nv, su, sv, st)
    CH.check_invariants(want)
    assert len(want["k"]) >= 1
    pair = lambda i: frozenset((order[su[i]], order[sv[i]]))
    want_edges = {pair(i): (int(st[i]), int(want["node"][i])) for i in range(len(st)) if want["node"][i] >= 0}
    want_forest = _by_name(want["k"].tolist(), want["parent"].tolist(), want["size"].tolist(), want["shell"].tolist(),
                           {e: i for e, (_, i) in want_edges.items()})

    off = tmp_path / "off"
    stdout_off = _run(d, off, threads, KOMB_TRUSS="1")
    assert not any((off / f).exists() for f in FILES)
    out = tmp_path / "on"
    stdout_on = _run(d, out, threads, KOMB_TRUSS="1", KOMB_COMMUNITY_HIERARCHY="1")
    kc_vid = {x[1]: int(x[0]) for x in [ln.rstrip("\n").split("\t") for ln in open(out / "kcore.tsv")][1:]}

    nodes = _rows(out / FILES[0], ["#Node", "K", "Rep_U", "Rep_V", "Parent", "Size", "Shell"])
    rows = _rows(out / FILES[1], ["#VID_U", "Name_U", "VID_V", "Name_V", "Trussness", "Node"])
    n = len(nodes)
    assert [int(x[0]) for x in nodes] == list(range(n))
    k, parent, size, shell = ([int(x[c]) for x in nodes] for c in (1, 4, 5, 6))
    assert all(-1 <= parent[i] < i for i in range(n))
    # the edges table: canonical order of this run's VIDs, the members with their trussness
    canon = [(int(x[0]), int(x[2])) for x in rows]
    assert canon == sorted(canon) and all(u < v for u, v in canon)
    assert all(kc_vid[x[1]] == int(x[0]) and kc_vid[x[3]] == int(x[2]) for x in rows)
    got_edges = {frozenset((x[1], x[3])): (int(x[4]), int(x[5])) for x in rows}
    assert len(got_edges) == len(rows)
    assert {e: t for e, (t, _) in got_edges.items()} == {e: t for e, (t, _) in want_edges.items()}
    assert all(0 <= i < n and k[i] == t for t, i in got_edges.values())
    # the forest by Name
    got_forest = _by_name(k, parent, size, shell, {e: i for e, (_, i) in got_edges.items()})
    assert got_forest == want_forest
    # node order: ascending (K, the node's first edge in this run's canonical order), and Rep is that edge
    first = {}
    for x in rows:
        i = int(x[5])
        while i >= 0:
            first.setdefault(i, (x[1], x[3]))
            i = parent[i]
    assert [(x[2], x[3]) for x in nodes] == [first[i] for i in range(n)]
    keys = [(k[i], kc_vid[nodes[i][2]], kc_vid[nodes[i][3]]) for i in range(n)]
    assert keys == sorted(keys)

    # the existing files and stdout are what they are without the variable
    assert sorted(os.listdir(out)) == sorted(os.listdir(off) + list(FILES))
    for f in ("kcore.tsv", "CoreA_anomaly.txt", "edgelist.txt", "truss_unitigs.fasta"):
        assert (out / f).read_bytes() == (off / f).read_bytes(), f
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(stdout_on) == mask(stdout_off).replace(str(off), str(out))

    # without KOMB_TRUSS the variable does nothing
    alone = tmp_path / "alone"
    _run(d, alone, threads, KOMB_COMMUNITY_HIERARCHY="1")
    assert not any((alone / f).exists() for f in FILES)
