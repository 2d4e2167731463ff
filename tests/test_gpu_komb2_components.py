"""komb2 with KOMB_COMPONENTS on the generated SAM + FASTA fixture: core_components.tsv (and, with KOMB_TRUSS=1,
truss_components.tsv) hold, as a partition by unitig Name with sizes, what the scipy reference gives on the graph the
SAM files define; without the variable nothing changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import components_ref as R
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")
VARS = ("KOMB_COMPONENTS", "KOMB_TRUSS", "KOMB_ONION")


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("components_komb2")
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


def _table(path, third):
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert rows[0] == ["#VID", "Name", third, "Component", "Size"]
    return rows[1:]


def _partition_by_name(order, label):
    """{name: (frozenset of the names of its component)} of a reference label vector over the vids of `order`."""
    groups = {}
    for v, lab in enumerate(label):
        if lab >= 0:
            groups.setdefault(int(lab), []).append(order[v])
    out = {}
    for members in groups.values():
        fs = frozenset(members)
        for nm in members:
            out[nm] = fs
    return out


def _check_table(rows, kc_vid, want_parts):
    """rows: a components table; kc_vid: Name -> VID of this run; want_parts: the reference partition by Name."""
    assert [int(x[0]) for x in rows] == sorted(int(x[0]) for x in rows)            # VID order
    assert all(kc_vid[x[1]] == int(x[0]) for x in rows)
    assert {x[1] for x in rows} == set(want_parts) and len(rows) == len(want_parts)   # rows are exactly the members
    got = {}
    for x in rows:
        got.setdefault(x[3], []).append(x[1])
    for rep, members in got.items():
        fs = frozenset(members)
        assert rep in fs and want_parts[rep] == fs
        assert kc_vid[rep] == min(kc_vid[nm] for nm in members)                  # the representative has the smallest VID
    for x in rows:
        assert int(x[4]) == len(want_parts[x[1]])


@pytest.mark.parametrize("threads", [1, 4])
def test_komb2_components_tsv(fixture, tmp_path, threads):
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
        kmax = int(core.max())
        su, sv, st = a.run_truss((core == kmax).astype(np.uint8))
    tmax = int(st.max()) if len(st) else 2

    off = tmp_path / "off"
    stdout_off = _run(d, off, threads, KOMB_TRUSS="1")
    assert not (off / "core_components.tsv").exists() and not (off / "truss_components.tsv").exists()

    for setting, k in (("max", kmax), ("2", 2)):
        out = tmp_path / f"on_{setting}"
        stdout_on = _run(d, out, threads, KOMB_COMPONENTS=setting, KOMB_TRUSS="1")
        kc = [ln.rstrip("\n").split("\t") for ln in open(out / "kcore.tsv")][1:]
        kc_vid = {x[1]: int(x[0]) for x in kc}
        kc_core = {x[1]: x[2] for x in kc}
        rows = _table(out / "core_components.tsv", "Coreness")
        assert all(x[2] == kc_core[x[1]] and int(x[2]) >= k for x in rows)
        _check_table(rows, kc_vid, _partition_by_name(order, R.core_components(rowptr, col, core, k)))

        trows = _table(out / "truss_components.tsv", "Trussness")
        assert all(int(x[2]) == tmax for x in trows)
        fasta_names = [ln[len(">Unitig_"):].rstrip("\n") for ln in open(out / "truss_unitigs.fasta") if ln.startswith(">")]
        assert sorted(x[1] for x in trows) == sorted(fasta_names)
        _check_table(trows, kc_vid, _partition_by_name(order, R.truss_components(nv, su, sv, st, tmax)))

        # the existing files and stdout are what they are without the variable
        for f in ("kcore.tsv", "CoreA_anomaly.txt", "edgelist.txt", "truss_unitigs.fasta"):
            assert (out / f).read_bytes() == (off / f).read_bytes(), f
        mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
        assert mask(stdout_on) == mask(stdout_off).replace(str(off), str(out))

    # without KOMB_TRUSS: the core table alone
    out = tmp_path / "core_only"
    _run(d, out, threads, KOMB_COMPONENTS="max")
    assert (out / "core_components.tsv").exists() and not (out / "truss_components.tsv").exists()
    assert (out / "core_components.tsv").read_bytes() == (tmp_path / "on_max" / "core_components.tsv").read_bytes()
