"""komb2 with KOMB_ONION=1 on the generated SAM + FASTA fixture: onion.tsv is written beside kcore.tsv and matches
networkx.onion_layers on the graph the SAM files define (keyed by unitig Name); without the variable nothing changes."""
import os
import re
import subprocess

import numpy as np
import pytest

import onion_ref as R
import samgraph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOMB2 = os.path.join(ROOT, "komb_amd", "bin", "komb2")


@pytest.fixture(scope="module")
def fixture(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("onion_komb2")
    fasta, s1, s2 = samgraph.make_fixture(2000, 20000, seed=1)
    (d / "unitigs.l-1.fasta").write_bytes(fasta)
    (d / "reads1.fastq.sam").write_bytes(s1)
    (d / "reads2.fastq.sam").write_bytes(s2)
    return d, s1, s2


def _run(d, out, threads, onion):
    out.mkdir()
    cmd = [KOMB2, "-t", str(threads), "-l", "-1", "-o", str(out), "-i", f"{d}/reads1.fastq.sam", "-j", f"{d}/reads2.fastq.sam",
           "-u", f"{d}/unitigs.l-1.fasta"]
    env = {k: v for k, v in os.environ.items() if k != "KOMB_ONION"}
    if onion:
        env["KOMB_ONION"] = "1"
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.mark.parametrize("threads", [1, 4])
def test_komb2_onion_tsv(fixture, tmp_path, threads):
    d, s1, s2 = fixture
    out = tmp_path / "on"
    stdout_on = _run(d, out, threads, True)
    rows = [ln.rstrip("\n").split("\t") for ln in open(out / "onion.tsv")]
    assert rows[0] == ["#VID", "Name", "Coreness", "Layer"]
    rows = rows[1:]
    kc = [ln.rstrip("\n").split("\t") for ln in open(out / "kcore.tsv")][1:]
    assert [int(x[0]) for x in rows] == list(range(len(kc)))
    assert [x[1] for x in rows] == [x[1] for x in kc]
    assert [x[2] for x in rows] == [x[2] for x in kc]                   # the coreness column is kcore.tsv's

    # the graph of the SAM files, by name, against networkx
    names, edges = samgraph.build_graph(s1, s2, threads)
    order = sorted(names)
    vid = {nm: i for i, nm in enumerate(order)}
    uv = np.array([[vid[a], vid[b]] for a, b in (tuple(e) for e in edges)], dtype=np.int64).reshape(-1, 2)
    rowptr, col = R.simple_csr(len(order), uv)
    want, n = R.networkx_layers(len(order), rowptr, col)
    got = {x[1]: int(x[3]) for x in rows}
    assert got == {nm: int(want[vid[nm]]) for nm in order}
    assert max(got.values()) == n

    # without the variable: no onion.tsv, the same files and stdout
    off = tmp_path / "off"
    stdout_off = _run(d, off, threads, False)
    assert not (off / "onion.tsv").exists()
    for f in ("kcore.tsv", "CoreA_anomaly.txt", "edgelist.txt"):
        assert (out / f).read_bytes() == (off / f).read_bytes(), f
    mask = lambda s: re.sub(r"\d+\.\d+ s", "T s", re.sub(r"= \d+\.\d+", "= T", s))
    assert mask(stdout_on) == mask(stdout_off)
