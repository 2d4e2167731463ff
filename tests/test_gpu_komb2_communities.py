"""komb2 with KOMB_TRUSS=1 and KOMB_COMMUNITIES on the generated SAM + FASTA fixture: truss_communities.tsv and
truss_community_vertices.tsv hold, keyed by unitig Name, what the reference of tests/truss_communities_ref.py gives on
the truss stage's result; a bad value is refused; without the variable nothing changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import samgraph
import truss_communities_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_COMPONENTS", "KOMB_COMMUNITIES", "KOMB_TRUSS", "KOMB_ONION")


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("communities_komb2")
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
        su, sv, st = a.run_truss((core == int(core.max())).astype(np.uint8))
    return order, nv, su, sv, st


def _check_files(out, order, nv, su, sv, st, k):
    lab = R.communities(nv, su, sv, st, k)
    sz = R.sizes(lab)
    multi = R.vertex_multiplicity(nv, su, sv, lab)
    key = lambda u, v: frozenset((order[u], order[v]))
    want_edge = {key(u, v): (int(t), int(l), int(s)) for u, v, t, l, s in zip(su.tolist(), sv.tolist(), st.tolist(), lab.tolist(), sz.tolist()) if l >= 0}
    want_groups = {}
    for e, (_, l, _) in want_edge.items():
        want_groups.setdefault(l, set()).add(e)
    kc_vid = {x[1]: int(x[0]) for x in (ln.rstrip("\n").split("\t") for ln in list(open(out / "kcore.tsv"))[1:])}

    rows = [ln.rstrip("\n").split("\t") for ln in open(out / "truss_communities.tsv")]
    assert rows[0] == ["#VID_U", "Name_U", "VID_V", "Name_V", "Trussness", "Community", "Size"]
    rows = rows[1:]
    assert len(rows) == len(want_edge)
    got_groups, seen = {}, 0
    pairs = [(int(x[0]), int(x[2])) for x in rows]
    assert pairs == sorted(pairs) and all(u < v for u, v in pairs)               # canonical order of this run's VIDs
    for x in rows:
        assert kc_vid[x[1]] == int(x[0]) and kc_vid[x[3]] == int(x[2])
        e = frozenset((x[1], x[3]))
        t, _, s = want_edge[e]
        assert (int(x[4]), int(x[6])) == (t, s) and t >= k
        c = int(x[5])
        assert 0 <= c <= seen                                                    # numbered in the order of their first edge
        seen += 1 if c == seen else 0
        got_groups.setdefault(c, set()).add(e)
    assert len(set(frozenset((x[1], x[3])) for x in rows)) == len(rows)
    assert {frozenset(g) for g in got_groups.values()} == {frozenset(g) for g in want_groups.values()}

    vrows = [ln.rstrip("\n").split("\t") for ln in open(out / "truss_community_vertices.tsv")]
    assert vrows[0] == ["#VID", "Name", "Communities"]
    vrows = vrows[1:]
    assert [int(x[0]) for x in vrows] == sorted(int(x[0]) for x in vrows) and all(kc_vid[x[1]] == int(x[0]) for x in vrows)
    assert {x[1]: int(x[2]) for x in vrows} == {order[v]: int(multi[v]) for v in range(nv) if multi[v] >= 1}
    return len(want_groups)


@pytest.mark.parametrize("threads", [1, 4])
def test_komb2_communities_tsv(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    order, nv, su, sv, st = _reference(s1, s2, threads)
    tmax = int(st.max()) if len(st) else 2
    assert len(st) > 0 and tmax >= 3

    off = tmp_path / "off"
    r_off = _run(d, off, threads, KOMB_TRUSS="1")
    files_off = sorted(os.listdir(off))
    assert "truss_communities.tsv" not in files_off and "truss_community_vertices.tsv" not in files_off

    for setting, k in (("max", tmax), ("3", 3), ("0", 2)):
        out = tmp_path / f"on_{setting}"
        r_on = _run(d, out, threads, KOMB_COMMUNITIES=setting, KOMB_TRUSS="1")
        assert _check_files(out, order, nv, su, sv, st, k) >= 1
        # the existing files and stdout are what they are without the variable
        assert sorted(os.listdir(out)) == sorted(files_off + ["truss_communities.tsv", "truss_community_vertices.tsv"])
        for f in files_off:
            assert (out / f).read_bytes() == (off / f).read_bytes(), f
        mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
        assert mask(r_on.stdout) == mask(r_off.stdout).replace(str(off), str(out))


def test_komb2_communities_switches(fixture, tmp_path):
    d, _, _ = fixture
    # a bad value exits non-zero with the message
    for i, bad in enumerate(("abc", "-3", "3x", "99999999999")):
        r = _run(d, tmp_path / f"bad{i}", 2, check=False, KOMB_COMMUNITIES=bad, KOMB_TRUSS="1")
        assert r.returncode != 0
        assert f"KOMB_COMMUNITIES={bad}: expected a trussness threshold >= 0 or max" in r.stderr
    # without the variable the output directory holds exactly the files it holds today
    plain = _run(d, tmp_path / "plain", 2)
    assert sorted(os.listdir(tmp_path / "plain")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv"]
    truss = _run(d, tmp_path / "truss", 2, KOMB_TRUSS="1")
    assert sorted(os.listdir(tmp_path / "truss")) == ["CoreA_anomaly.txt", "edgelist.txt", "kcore.tsv", "truss_unitigs.fasta"]
    # without KOMB_TRUSS=1 there is no truss stage, and so no communities
    alone = _run(d, tmp_path / "alone", 2, KOMB_COMMUNITIES="3")
    assert sorted(os.listdir(tmp_path / "alone")) == sorted(os.listdir(tmp_path / "plain"))
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(alone.stdout) == mask(plain.stdout).replace(str(tmp_path / "plain"), str(tmp_path / "alone"))
    assert plain.returncode == 0 and truss.returncode == 0
