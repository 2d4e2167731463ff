"""komb2 with KOMB_HIERARCHY on the generated SAM + FASTA fixture: core_hierarchy.tsv / core_hierarchy_vertices.tsv (and,
with KOMB_TRUSS=1, the truss pair) hold a forest whose implied partition by unitig Name equals, for every k, the scipy
reference's on the graph the SAM files define; without the variable nothing changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import components_ref as R
import hierarchy_ref as H
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_HIERARCHY", "KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_TRUSS", "KOMB_ONION")
FILES = ("core_hierarchy.tsv", "core_hierarchy_vertices.tsv", "truss_hierarchy.tsv", "truss_hierarchy_vertices.tsv")


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("hierarchy_komb2")
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


def _partition_by_name(order, label):
    groups = {}
    for v, lab in enumerate(label):
        if lab >= 0:
            groups.setdefault(int(lab), []).append(order[v])
    return {frozenset(m) for m in groups.values()}


def _check_forest(nodes, verts, kc_vid, k_min, want_partition_at, want_level):
    """nodes / verts: the rows of a node table and of its vertices table; kc_vid: Name -> VID of this run;
    want_partition_at(k): the reference partition of G_k by Name; want_level: Name -> level of the members."""
    n = len(nodes)
    assert [int(x[0]) for x in nodes] == list(range(n))
    K = [int(x[1]) for x in nodes]
    rep = [x[2] for x in nodes]
    parent, size, shell = ([int(x[c]) for x in nodes] for c in (3, 4, 5))
    assert all(-1 <= parent[i] < i for i in range(n)) and all(K[parent[i]] < K[i] for i in range(n) if parent[i] >= 0)
    assert [(K[i], kc_vid[rep[i]]) for i in range(n)] == sorted((K[i], kc_vid[rep[i]]) for i in range(n))   # node order
    # the vertices table: VID order, the members with their levels
    assert [int(x[0]) for x in verts] == sorted(int(x[0]) for x in verts)
    assert all(kc_vid[x[1]] == int(x[0]) for x in verts)
    assert {x[1]: int(x[2]) for x in verts} == want_level
    vnode = {x[1]: int(x[3]) for x in verts}
    assert all(0 <= i < n and K[i] == want_level[nm] for nm, i in vnode.items())
    assert [sum(1 for i in vnode.values() if i == j) for j in range(n)] == shell
    kids = [0] * n
    for i in range(n):
        if parent[i] >= 0:
            kids[parent[i]] += size[i]
    assert [shell[i] + kids[i] for i in range(n)] == size
    # for every k, the partition the files imply: walk up from the vertex' node while the parent's level is still >= k
    members_of = {}
    for k in range(k_min, max(K, default=k_min) + 2):
        groups = {}
        for nm, i in vnode.items():
            if want_level[nm] < k:
                continue
            while parent[i] >= 0 and K[parent[i]] >= k:
                i = parent[i]
            groups.setdefault(i, []).append(nm)
        assert {frozenset(m) for m in groups.values()} == want_partition_at(k), k
        for i, m in groups.items():
            if K[i] == k:
                members_of[i] = m
    assert sorted(members_of) == list(range(n))                # every node is the top of a walk at its own level
    for i, m in members_of.items():
        assert len(m) == size[i] and rep[i] in m and kc_vid[rep[i]] == min(kc_vid[nm] for nm in m)   # Rep has the smallest VID


@pytest.mark.parametrize("threads", [1, 4])
def test_komb2_hierarchy_tsv(fixture, tmp_path, threads):
    import komb_amd
    d, s1, s2 = fixture
    names, edges = samgraph.build_graph(s1, s2, threads)
    order = sorted(names)
    vid = {nm: i for i, nm in enumerate(order)}
    uv = np.array([[vid[a], vid[b]] for a, b in (tuple(e) for e in edges)], dtype=np.int64).reshape(-1, 2)
    nv = len(order)
    with komb_amd.KombAccel() as a:
        a.from_edges(nv, uv)
        rowptr, col = a.get_csr()
        _, core = a.run_core()
        su, sv, st = a.run_truss((core == int(core.max())).astype(np.uint8))
    lvl = H.truss_levels(nv, su, sv, st)

    off = tmp_path / "off"
    stdout_off = _run(d, off, threads, KOMB_TRUSS="1")
    assert not any((off / f).exists() for f in FILES)
    out = tmp_path / "on"
    stdout_on = _run(d, out, threads, KOMB_HIERARCHY="1", KOMB_TRUSS="1")
    kc = [ln.rstrip("\n").split("\t") for ln in open(out / "kcore.tsv")][1:]
    kc_vid = {x[1]: int(x[0]) for x in kc}

    verts = _rows(out / "core_hierarchy_vertices.tsv", ["#VID", "Name", "Coreness", "Node"])
    assert [(x[0], x[1], x[2]) for x in verts] == [(x[0], x[1], x[2]) for x in kc]         # every vertex, kcore.tsv's Coreness
    _check_forest(_rows(out / "core_hierarchy.tsv", ["#Node", "K", "Rep", "Parent", "Size", "Shell"]), verts, kc_vid, 0,
                  lambda k: _partition_by_name(order, R.core_components(rowptr, col, core, k)),
                  {order[v]: int(core[v]) for v in range(nv)})
    _check_forest(_rows(out / "truss_hierarchy.tsv", ["#Node", "K", "Rep", "Parent", "Size", "Shell"]),
                  _rows(out / "truss_hierarchy_vertices.tsv", ["#VID", "Name", "Trussness", "Node"]), kc_vid, 2,
                  lambda k: _partition_by_name(order, R.truss_components(nv, su, sv, st, k)),
                  {order[v]: int(lvl[v]) for v in range(nv) if lvl[v] >= 2})

    # the existing files and stdout are what they are without the variable
    for f in ("kcore.tsv", "CoreA_anomaly.txt", "edgelist.txt", "truss_unitigs.fasta"):
        assert (out / f).read_bytes() == (off / f).read_bytes(), f
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(stdout_on) == mask(stdout_off).replace(str(off), str(out))

    # without KOMB_TRUSS: the core pair alone
    out = tmp_path / "core_only"
    _run(d, out, threads, KOMB_HIERARCHY="1")
    assert not (out / "truss_hierarchy.tsv").exists() and not (out / "truss_hierarchy_vertices.tsv").exists()
    for f in FILES[:2]:
        assert (out / f).read_bytes() == (tmp_path / "on" / f).read_bytes()
