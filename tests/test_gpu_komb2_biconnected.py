"""komb2 with KOMB_TRUSS=1 and KOMB_BICONNECTED on a generated SAM + FASTA fixture: truss_blocks.tsv and
truss_articulation.tsv hold, keyed by unitig Name, what the reference of tests/biconnected_ref.py gives on the k-truss of
the graph the SAM files define; a bad value is refused; without the variable nothing changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import biconnected_ref as R
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_BICONNECTED", "KOMB_TRUSS", "KOMB_ONION")
NEW = ["truss_articulation.tsv", "truss_blocks.tsv"]
# (blocks, articulation points, bridges) of the fixture's graph, counted with networkx (3000 lines: the default fixture of
# 20000 lines has only two blocks)
COUNTS = {2: (54, 44, 48), 3: (11, 10, 0)}


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("biconnected_komb2")
    fasta, s1, s2 = samgraph.make_fixture(2000, 3000, seed=1)
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
    """The k-truss result of the whole graph the SAM files define, by Name."""
    import komb_amd
    names, edges = samgraph.build_graph(s1, s2, threads)
    order = sorted(names)
    vid = {nm: i for i, nm in enumerate(order)}
    uv = np.array([[vid[a], vid[b]] for a, b in (tuple(e) for e in edges)], dtype=np.int64).reshape(-1, 2)
    nv = len(order)
    with komb_amd.KombAccel() as a:
        a.from_edges(nv, uv)
        eu, ev, tr = a.run_truss()
    return order, nv, eu, ev, tr


def _check_files(out, order, nv, eu, ev, tr, k):
    want = R.biconnected(nv, eu, ev, tr, k)
    key = lambda u, v: frozenset((order[u], order[v]))
    want_edge = {key(u, v): (int(t), int(b), int(s)) for u, v, t, b, s in
                 zip(eu.tolist(), ev.tolist(), tr.tolist(), want["block"].tolist(), want["size"].tolist()) if b >= 0}
    want_groups = {}
    for e, (_, b, _) in want_edge.items():
        want_groups.setdefault(b, set()).add(e)
    kc_vid = {x[1]: int(x[0]) for x in (ln.rstrip("\n").split("\t") for ln in list(open(out / "kcore.tsv"))[1:])}

    rows = [ln.rstrip("\n").split("\t") for ln in open(out / "truss_blocks.tsv")]
    assert rows[0] == ["#VID_U", "Name_U", "VID_V", "Name_V", "Trussness", "Block", "Size", "Bridge"]
    rows = rows[1:]
    assert len(rows) == len(want_edge)
    got_groups, seen = {}, 0
    pairs = [(int(x[0]), int(x[2])) for x in rows]
    assert pairs == sorted(pairs) and all(u < v for u, v in pairs)               # canonical order of this run's VIDs
    for x in rows:
        assert kc_vid[x[1]] == int(x[0]) and kc_vid[x[3]] == int(x[2])
        e = frozenset((x[1], x[3]))
        t, _, s = want_edge[e]
        assert (int(x[4]), int(x[6]), int(x[7])) == (t, s, 1 if s == 1 else 0) and t >= k
        c = int(x[5])
        assert 0 <= c <= seen                                                    # numbered in the order of their first edge
        seen += 1 if c == seen else 0
        got_groups.setdefault(c, set()).add(e)
    assert len(set(frozenset((x[1], x[3])) for x in rows)) == len(rows)
    assert {frozenset(g) for g in got_groups.values()} == {frozenset(g) for g in want_groups.values()}

    vrows = [ln.rstrip("\n").split("\t") for ln in open(out / "truss_articulation.tsv")]
    assert vrows[0] == ["#VID", "Name", "Blocks", "Articulation", "Component2E", "Size2E"]
    vrows = vrows[1:]
    assert [int(x[0]) for x in vrows] == sorted(int(x[0]) for x in vrows) and all(kc_vid[x[1]] == int(x[0]) for x in vrows)
    nb, lab, sz = want["n_blocks"], want["ecc_label"], want["ecc_size"]
    # a component is named by its member of smallest VID: VIDs follow -t, so the partition is compared, and the name within it
    assert {x[1]: (int(x[2]), int(x[3]), int(x[5])) for x in vrows} == \
        {order[v]: (int(nb[v]), 1 if nb[v] >= 2 else 0, int(sz[v])) for v in range(nv) if lab[v] >= 0}
    got_parts, want_parts = {}, {}
    for x in vrows:
        got_parts.setdefault(x[4], set()).add(x[1])
    for v in range(nv):
        if lab[v] >= 0:
            want_parts.setdefault(int(lab[v]), set()).add(order[v])
    assert {frozenset(p) for p in got_parts.values()} == {frozenset(p) for p in want_parts.values()}
    for name, part in got_parts.items():
        assert name in part and kc_vid[name] == min(kc_vid[n] for n in part)
    bridges = sum(1 for x in rows if x[7] == "1")
    return len(want_groups), sum(1 for x in vrows if x[3] == "1"), bridges


@pytest.mark.parametrize("threads", [1, 4])
def test_komb2_biconnected_tsv(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    order, nv, eu, ev, tr = _reference(s1, s2, threads)
    tmax = int(tr.max()) if len(tr) else 2
    assert len(tr) > 0 and tmax >= 3

    off = tmp_path / "off"
    r_off = _run(d, off, threads, KOMB_TRUSS="1")
    files_off = sorted(os.listdir(off))
    assert not set(NEW) & set(files_off)

    for setting, k in (("2", 2), ("3", 3), ("max", tmax)):
        out = tmp_path / f"on_{setting}"
        r_on = _run(d, out, threads, KOMB_BICONNECTED=setting, KOMB_TRUSS="1")
        counts = _check_files(out, order, nv, eu, ev, tr, k)
        if k in COUNTS:
            assert counts == COUNTS[k], k
        assert counts[0] >= 1
        # the existing files and stdout are what they are without the variable
        assert sorted(os.listdir(out)) == sorted(files_off + NEW)
        for f in files_off:
            assert (out / f).read_bytes() == (off / f).read_bytes(), f
        mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
        assert mask(r_on.stdout) == mask(r_off.stdout).replace(str(off), str(out))


def test_komb2_biconnected_switches(fixture, tmp_path):
    d, _, _ = fixture
    # a bad value exits non-zero with the message
    for i, bad in enumerate(("abc", "-3", "3x", "99999999999")):
        r = _run(d, tmp_path / f"bad{i}", 2, check=False, KOMB_BICONNECTED=bad, KOMB_TRUSS="1")
        assert r.returncode != 0
        assert f"KOMB_BICONNECTED={bad}: expected a trussness threshold >= 0 or max" in r.stderr
    # without KOMB_TRUSS=1 there is no truss stage, and so no blocks
    plain = _run(d, tmp_path / "plain", 2)
    alone = _run(d, tmp_path / "alone", 2, KOMB_BICONNECTED="3")
    assert sorted(os.listdir(tmp_path / "alone")) == sorted(os.listdir(tmp_path / "plain")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv"]
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(alone.stdout) == mask(plain.stdout).replace(str(tmp_path / "plain"), str(tmp_path / "alone"))
