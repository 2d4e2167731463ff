"""CPU tests of tests/sequence_model.py: the model against hand-worked sequences taken sentence by sentence from
include/komb_accel.h, the graphs against the facts the model keeps of them, and conditions a-k on what the committed plans
exercise (conditions, not measurements: the generator appends directed steps until the plans alone meet them)."""
import os
import re

import numpy as np
import pytest

import sequence_model as SM
from sequence_model import ARG, OK, STATE

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "komb_accel.h")


def _run(*ops):
    m = SM.Model()
    return m, [m.apply(op) for op in ops]


def _all_held():
    """A model with a graph and all nineteen results held."""
    m, codes = _run(("load", "A", "edges"), ("core", "plain"), ("onion",), ("comp", "core", 2), ("hier", "core"), ("dens", 8),
                    ("truss", "plain", None), ("comm", 3), ("bic", 2), ("chier",), ("sc", 1, 2, 3), ("nuc",), ("nhier",), ("mclq", 0),
                    ("cens", 2, -1, 0), ("mxl", 2), ("perc", 3), ("gl",), ("btw", ("prefix", 65)), ("dist", ("prefix", 257)))
    assert codes == [OK] * len(codes) and set(m.held) == set(SM.RESULTS)
    return m


# ---- the table and the header

def test_table_lines_name_the_header_sentences():
    """Every row of the table points at a line of the header that says what the row says (a word of the sentence is there)."""
    lines = open(HEADER).read().split("\n")
    words = {"load": "drops the previous graph", "load_bad": "drops the previous graph", "core": "komb_core_run computes", "core_sharded": "bit-equal",
             "onion": "changes no k-core", "comp": "snapshot in arrays of its own", "hier": "snapshot in arrays of its own", "dens": "snapshot in arrays of its own",
             "truss": "drops the previous k-truss result", "truss_vmask": "drops the previous k-truss result", "slice": "NO exchange",
             "truss_sharded": "world == 1 is komb_truss_run", "prepare": "komb_truss_prepare makes it ahead of time", "unprepare": "komb_truss_unprepare drops it",
             "comm": "changes no k-core", "bic": "neither change nor drop it", "chier": "neither change nor drop them", "sc": "neither change nor drop it",
             "nuc": "a new komb_nucleus_run", "nhier": "No other call changes or drops", "mclq": "No other call changes or drops",
             "cens": "No other call changes or drops", "mxl": "goes with it", "perc": "No other call changes or drops",
             "gl": "No other call changes or drops it; a run changes no other result",
             "btw": "graph load drops it.  No k-core, k-truss or other analysis call changes or drops it",
             "dist": "a graph load drops it.  No k-core, k-truss, betweenness or other analysis call changes or drops it",
             "corea": "CoreA calls neither change nor drop", "densest_block": "leaves the resident", "moments": "Measurement only", "get_csr": "Copy the resident CSR"}
    assert set(words) == set(SM.ROWS)
    for row in SM.ROWS:
        n = SM.HEADER_LINE[row]
        assert any(words[row] in " ".join(s.strip(" *") for s in lines[i - 1:i + 1]) for i in (n - 1, n, n + 1)), (row, n, lines[n - 1])


def test_table_shape():
    assert len(SM.ROWS) == 31 and len(SM.RESULTS) == 19
    # two loads drop everything; four kinds of k-truss run drop the eleven, unprepare those and the k-truss result; a nucleus
    # run and a maximal-cliques run one each.  23 rows compute a result, which is neither dropped nor kept by its own row.
    assert sum(len(SM.DROPS[r]) for r in SM.ROWS) == 2 * 19 + 4 * 11 + 12 + 1 + 1 == 96
    assert sum(1 for r in SM.ROWS if SM.OWN[r] is not None) == 23
    assert sum(len(SM.KEEPS[r]) for r in SM.ROWS) == 31 * 19 - 96 - 23 == 470
    assert len(SM.TRUSS_DERIVED) == 11 and set(SM.BASE) | {"truss"} | set(SM.TRUSS_DERIVED) | set(SM.GRAPH_OWNED) == set(SM.RESULTS)
    for row in ("truss", "truss_vmask", "slice", "truss_sharded", "unprepare"):    # what belongs to the graph outlives them all
        assert "gl" in SM.DROPS[row] and set(SM.GRAPH_OWNED) <= SM.KEEPS[row], row
    assert set(SM.STATS_FROZEN) >= {"gl", "btw", "dist"}
    for row in SM.ROWS:
        assert not SM.DROPS[row] & SM.KEEPS[row] and SM.OWN[row] not in SM.KEEPS[row]
    assert set(SM.OPS) == {n[3:] for n in dir(SM.Model) if n.startswith("op_")}


# ---- hand-worked sequences

def test_a_vmask_run_drops_the_eleven_and_keeps_the_seven():
    m = _all_held()
    assert m.apply(("truss", "plain", "maxcore")) == OK
    assert set(m.held) == {"core", "onion", "comp", "hier", "dens", "truss", "btw", "dist"} and m.truss["kind"] == "vmask"
    for r in SM.TRUSS_DERIVED:
        assert m.apply(("read", r, None)) == STATE
    for r in SM.BASE + SM.GRAPH_OWNED:
        assert m.apply(("read", r, None)) == OK
    assert m.held["btw"] == ("prefix", 65) and m.held["dist"] == ("prefix", 257)


def test_every_kind_of_truss_run_and_unprepare_drop_the_eleven():
    for op in (("truss", "plain", None), ("truss", "sharded", None), ("truss", "sharded", "random"), ("slice", 0, 1, None), ("slice", 1, 3, None),
               ("slice", 1, 3, "maxcore")):
        m = _all_held()
        assert m.apply(op) == OK and set(m.held) == set(SM.BASE) | {"truss"} | set(SM.GRAPH_OWNED), op
    m = _all_held()
    assert m.apply(("unprepare",)) == OK and set(m.held) == set(SM.BASE) | set(SM.GRAPH_OWNED) and m.truss is None and not m.prepared
    assert m.apply(("read", "truss", 0)) == STATE and m.apply(("read", "gl", None)) == STATE
    assert m.apply(("read", "btw", None)) == OK and m.apply(("read", "dist", None)) == OK


def test_nucleus_run_drops_the_nucleus_hierarchy_only():
    m = _all_held()
    assert m.apply(("nuc",)) == OK and set(m.held) == set(SM.RESULTS) - {"nhier"}
    assert m.apply(("read", "nhier", 1)) == STATE and m.apply(("nhier",)) == OK


def test_a_maximal_cliques_run_that_succeeds_drops_the_clique_communities():
    m = _all_held()
    assert m.apply(("mxl", 1)) == ARG and "perc" in m.held                  # a refused run drops nothing
    assert m.apply(("mxl", 3)) == OK and set(m.held) == set(SM.RESULTS) - {"perc"}
    assert m.apply(("perc", 2)) == STATE                                     # the list lacks the member cliques of k = 2
    assert m.apply(("perc", 3)) == OK and m.held["perc"] == (3, 3, None)


def test_every_other_run_drops_nothing():
    for op in (("core", "plain"), ("core", "sharded"), ("onion",), ("comp", "truss", -1), ("hier", "truss"), ("dens", 0), ("prepare",), ("comm", 2), ("bic", -1),
               ("chier",), ("sc", 7, 10, 3), ("nhier",), ("mclq", 0), ("cens", 3, 5, 3), ("perc", 4), ("gl",), ("btw", ("prefix", 1)), ("btw", ("prefix", 0)),
               ("dist", ("prefix", 257)), ("stateless", "corea"), ("stateless", "densest_block"),
               ("stateless", "moments"), ("stateless", "get_csr"), ("option", "FINISH", "lds"), ("poison", "0x00000001"), ("checkpoint",)):
        m = _all_held()
        assert m.apply(op) == OK and set(m.held) == set(SM.RESULTS), op


def test_a_partial_slice_refuses_every_analysis_of_the_result_and_the_whole_range_does_not():
    m, _ = _run(("load", "B", "csr"), ("core", "plain"), ("slice", 1, 2, None))
    assert m.truss["kind"] == "partial" and (m.truss["lo"], m.truss["hi"]) == (4709, 9418)
    for op in (("comp", "truss", 3), ("hier", "truss"), ("comm", 3), ("bic", 2), ("chier",), ("sc", 1, 2, 3), ("nuc",), ("nhier",), ("mclq", 0),
               ("cens", 2, -1, 0), ("mxl", 2), ("perc", 3), ("gl",)):
        assert m.apply(op) == STATE, op
    assert m.apply(("comp", "core", 2)) == OK and m.apply(("hier", "core")) == OK and m.apply(("read", "truss", 1)) == OK
    assert m.apply(("btw", ("prefix", 1))) == OK and m.apply(("dist", ("prefix", 257))) == OK      # they need no other result
    assert m.apply(("read", "btw", None)) == OK and m.apply(("read", "dist", None)) == OK
    assert m.apply(("slice", 0, 1, None)) == OK and m.truss["kind"] == "whole"
    for op in (("comp", "truss", 3), ("hier", "truss"), ("comm", 3), ("bic", 2), ("chier",), ("sc", 1, 2, 3), ("nuc",), ("nhier",), ("mclq", 0),
               ("cens", 2, -1, 0), ("mxl", 2), ("perc", 3), ("gl",)):
        assert m.apply(op) == OK, op
    assert "btw" in m.held and "dist" in m.held                              # (the whole-range slice dropped neither)
    assert m.apply(("slice", 2, 2, None)) == ARG and "nuc" in m.held         # refused: the arguments were not accepted
    m, _ = _run(("load", "A", "edges"), ("slice", 2, 3, "random"))           # with a vmask the results are complete on every rank
    assert m.truss["kind"] == "vmask" and m.apply(("nuc",)) == OK
    m, _ = _run(("load", "edge", "edges"), ("slice", 1, 2, None))            # one edge: rank 1 of 2 holds [0, 1), the whole range
    assert m.truss["kind"] == "whole"
    m, _ = _run(("load", "iso7", "edges"), ("slice", 1, 2, None))            # no edge: nothing is missing
    assert m.truss["kind"] == "empty" and m.apply(("mclq", 0)) == OK


def test_a_failed_load_leaves_no_graph():
    m = _all_held()
    assert m.apply(("load_bad", "A")) == ARG and m.graph is None and not m.held
    for r in SM.RESULTS:
        assert m.apply(("read", r, None)) == (STATE if r in ("core", "truss") else ARG), r
    for op, code in ((("core", "plain"), STATE), (("truss", "plain", None), STATE), (("prepare",), STATE), (("unprepare",), OK), (("onion",), ARG),
                     (("comp", "core", 0), ARG), (("hier", "core"), ARG), (("dens", 1), ARG), (("comm", 3), ARG), (("bic", 2), ARG), (("chier",), ARG),
                     (("sc", 1, 2, 3), ARG), (("nuc",), ARG), (("nhier",), ARG), (("mclq", 0), ARG), (("cens", 2, -1, 0), ARG), (("mxl", 2), ARG),
                     (("perc", 3), ARG), (("gl",), ARG), (("btw", ("prefix", 0)), ARG), (("btw", "all"), ARG), (("dist", ("prefix", 1)), ARG),
                     (("dist", ("bad", "count")), ARG), (("stateless", "densest_block"), STATE), (("stateless", "moments"), STATE), (("stateless", "get_csr"), STATE)):
        assert m.apply(op) == code, op
    assert m.apply(("load", "A", "csr")) == OK and not m.held
    assert m.apply(("read", "nuc", None)) == STATE


def test_call_order_and_arguments():
    m, _ = _run(("load", "A", "edges"))
    assert m.apply(("comp", "core", 0)) == OK                                # the whole graph needs nothing but a graph
    assert [m.apply(op) for op in (("comp", "core", 1), ("comp", "core", -1), ("hier", "core"), ("dens", 8))] == [STATE] * 4
    assert [m.apply(op) for op in (("comp", "truss", 2), ("hier", "truss"), ("nuc",))] == [STATE] * 3
    assert m.apply(("core", "bad")) == ARG and "core" not in m.held
    assert m.apply(("core", "sharded")) == OK
    assert [m.apply(op) for op in (("comp", 7, 2), ("comp", "core", -2), ("hier", 7), ("dens", -1))] == [ARG] * 4
    assert m.apply(("truss", "plain", None)) == OK
    assert [m.apply(op) for op in (("comm", -2), ("bic", -2), ("sc", 0, 10, 2), ("sc", 11, 10, 2), ("sc", 1, 2, 1), ("mclq", -1), ("cens", 1, -1, 0),
                                   ("cens", 4, 3, 0), ("mxl", 1), ("perc", 1))] == [ARG] * 10
    assert m.apply(("nhier",)) == STATE and m.apply(("perc", 3)) == STATE    # no decomposition, no list
    assert set(m.held) == {"core", "comp", "truss"}
    assert [m.apply((r, ("bad", how))) for r in SM.GRAPH_OWNED for how in SM.BAD_SOURCES] == [ARG] * 6 and set(m.held) == {"core", "comp", "truss"}


def test_graphlets_index_one_complete_k_truss_result():
    """ "on the last COMPLETE k-truss result (whole graph or vmask) ... after komb_truss_run_slice / a sharded run that
    materialised only part of the canonical edges, after komb_truss_unprepare, fetch / info before a run: KOMB_ERR_STATE" """
    m, _ = _run(("load", "A", "edges"))
    assert m.apply(("gl",)) == STATE and m.apply(("read", "gl", None)) == STATE          # no k-truss result at all
    assert m.apply(("slice", 1, 3, None)) == OK and m.apply(("gl",)) == STATE            # a part of the canonical edges
    assert m.apply(("slice", 0, 1, None)) == OK and m.apply(("read", "gl", None)) == STATE and m.apply(("gl",)) == OK
    assert m.held["gl"] == (None,) and m.log[-1]["ceu"] == ("gl", "first") and m.log[-1]["sup_first"] == "gl" and m.sup_ready
    assert m.apply(("nuc",)) == OK and m.apply(("sc", 1, 2, 3)) == OK and m.apply(("read", "gl", None)) == OK   # "No other call changes or drops it"
    assert "sup_first" not in m.log[-2]                                      # (the census had made the supports)
    for op in (("truss", "plain", "maxcore"), ("truss", "sharded", None), ("slice", 0, 2, None), ("unprepare",), ("load", "A", "csr")):
        m, _ = _run(("load", "A", "edges"), ("truss", "plain", None), ("gl",))
        assert m.apply(op) == OK and "gl" not in m.held and m.apply(("read", "gl", None)) == STATE, op
    m, _ = _run(("load", "A", "edges"), ("truss", "plain", "random"), ("gl",))           # a vmask result is complete
    assert m.held["gl"] == ("random",) and "ceu" not in m.log[-1] and "sup_first" not in m.log[-1]
    m, _ = _run(("load", "iso7", "edges"), ("truss", "plain", None), ("gl",))            # "the empty graph is not an error"
    assert m.held["gl"] == (None,) and m.truss["kind"] == "empty"


@pytest.mark.parametrize("r", SM.GRAPH_OWNED)
def test_betweenness_and_distances_belong_to_the_graph(r):
    """ "It needs no other result ... An id outside [0, nv) or n_sources < 0: KOMB_ERR_ARG ... a refused or failed run leaves the
    PREVIOUS result readable.  It belongs to the graph: a graph load drops it.  No k-core, k-truss or other analysis call
    changes or drops it" """
    other = SM.GRAPH_OWNED[1 - SM.GRAPH_OWNED.index(r)]
    m, _ = _run(("load", "B", "edges"))
    assert m.apply(("read", r, None)) == STATE and m.apply((r, ("prefix", 65))) == OK and m.held == {r: ("prefix", 65)}
    for how in SM.BAD_SOURCES:                                               # a bad id, a negative count: the held result stays
        assert m.apply((r, ("bad", how))) == ARG and m.held[r] == ("prefix", 65) and m.log[-1]["refused"] == r
        assert m.apply(("read", r, None)) == OK
    for op in (("core", "plain"), ("truss", "plain", None), ("gl",), ("nuc",), ("slice", 1, 3, None), ("truss", "sharded", "maxcore"), ("unprepare",),
               (other, ("prefix", 257)), (other, ("bad", "id_high")), ("truss", "plain", None), ("mxl", 2), ("stateless", "moments")):
        m.apply(op)
        assert m.held[r] == ("prefix", 65) and m.apply(("read", r, None)) == OK, op
    assert m.apply((r, ("prefix", 0))) == OK and m.held[r] == ("prefix", 0) and other in m.held     # a new run replaces it, and only it
    assert m.apply(("load_bad", "B")) == ARG and m.apply(("read", r, None)) == ARG and m.apply((r, ("prefix", 0))) == ARG
    assert m.apply(("load", "nv0", "edges")) == OK and m.apply(("read", r, None)) == STATE
    assert m.apply((r, "all")) == OK and m.apply((r, ("prefix", 0))) == OK and m.apply((r, ("bad", "id_negative"))) == ARG
    with pytest.raises(AssertionError):
        m.apply((r, ("prefix", 1)))                                          # (no list of the menu has an entry there: any id is refused)


def test_source_menus_and_master_lists():
    for g, (nv, _, _) in SM.FACTS.items():
        menu = SM.source_menu(g)
        assert ("prefix", 0) in menu and (("all" in menu) == (nv <= SM.SMALL_NV)), g
        assert all(s == "all" or (s[0] == "prefix" and 0 <= s[1] <= SM.MASTER_LEN) for s in menu), g
    assert SM.source_menu("C") == (("prefix", 0),) and SM.source_menu("strided")[-1] == ("prefix", 3)
    assert ("prefix", 257) in SM.source_menu("A") and ("prefix", 257) in SM.source_menu("book257") and SM.source_menu("nv0") == (("prefix", 0), "all")
    deg = np.asarray([1, 0, 3, 1, 1, 0] + [0] * 94)
    master = SM.master_sources("x", 100, deg)
    assert len(master) == SM.MASTER_LEN == 257 and len(set(master)) <= SM.MASTER_POOL == 40 and len(set(master)) > 20
    assert master[0] == 2 and deg[master[3]] == 0 and master == SM.master_sources("x", 100, deg) != SM.master_sources("y", 100, deg)
    assert len(master) > len(set(master)) and master != sorted(master)      # repeats, no order
    assert set(SM.master_sources("edge", 2, np.asarray([1, 1]))) <= {0, 1} and SM.master_sources("nv0", 0, np.zeros(0)) == []


def test_lazily_made_arrays():
    m, _ = _run(("load", "A", "edges"), ("truss", "plain", None))
    assert not m.ceu and not m.sup_ready and m.prepared
    m.apply(("comm", 3))
    assert m.log[-1]["ceu"] == ("comm", "first") and m.ceu and not m.sup_ready and not m.comm_v
    m.apply(("read", "comm", "info"))
    assert m.log[-1]["comm_v_first"] == "info" and m.comm_v
    m.apply(("sc", 1, 2, 3))
    assert m.log[-1]["ceu"] == ("sc", "later") and m.log[-1]["sup_first"] == "sc" and m.sup_ready
    m.apply(("unprepare",))
    assert m.ceu and not m.prepared and not m.sup_ready                      # the canonical edge list is kept with the graph
    m.apply(("truss", "plain", None)); m.apply(("read", "truss", 0))
    assert m.log[-1]["ceu"] == ("fetch", "later") and m.log[-1]["sup_first"] == "fetch_support"
    m.apply(("truss", "plain", "maxcore")); m.apply(("bic", 2))
    assert "ceu" not in m.log[-1]                                            # a run under a vmask makes its subgraph's list itself
    m.apply(("truss", "plain", None)); m.apply(("gl",))
    assert m.log[-1]["ceu"] == ("gl", "later") and m.log[-1]["sup_first"] == "gl" and m.sup_ready   # "made here as those fetches make them"
    m.apply(("read", "truss", 0))
    assert "sup_first" not in m.log[-1]
    m.apply(("load", "A", "edges"))
    assert not m.ceu and not m.prepared
    m.apply(("stateless", "moments"))
    assert m.prepared


# ---- the graphs

@pytest.fixture(scope="module")
def graphs(built):
    import komb_amd
    from oracle import oracle
    return SM.build_graphs(komb_amd.gen_hug_edges, oracle, SM.SEEDS[0])


def test_graphs_are_the_ones_the_model_knows(graphs):
    assert set(graphs) == set(SM.FACTS) and {g for order in SM.ORDERS for g in order} == set(SM.FACTS)
    for name, g in graphs.items():
        nv, ne, sub = SM.FACTS[name]
        assert (g.nv, g.ne()) == (nv, ne), name
        assert (g.ne("maxcore") == sub) if sub is not None else g.ne("maxcore") > 0, name
        if ne >= SM.SMALL_NE:
            assert g.ne("random") > 0, name
    a, b, c, d = (graphs[n] for n in "ABCD")
    assert (int(a.base[None][2].max()), int(a.deg.max()), a.tri) == (9, 290, 15140)
    assert (int(b.base[None][2].max()), int(b.deg.max())) == (16, 487) and int(d.deg.max()) == 708
    window = lambda small, big: small <= big <= small + small // 4 + 4096      # DevPool::get hands back bytes .. bytes + bytes / 4 + 4096
    assert window(4 * a.nv, 4 * b.nv) and window(4 * a.ne(), 4 * b.ne())        # A's arrays land in B's blocks, with a stale tail
    assert window(4 * a.ne(), 4 * c.nv) and window(4 * c.nv, 4 * b.ne())        # C's vertex arrays among the edge arrays of A and B
    e, e2 = graphs["E"], graphs["E2"]
    assert (e.nv, e.ne()) == (e2.nv, e2.ne()) and int(e.base[None][2].max()) == 60 and int(e2.base[None][2].max()) <= 3


def test_ids_are_permuted_per_plan(built):
    import komb_amd
    raw = SM.raw_graphs(komb_amd.gen_hug_edges, SM.hand_graphs())
    p, q = SM.permuted(raw, SM.SEEDS[0]), SM.permuted(raw, SM.SEEDS[1])
    for name in raw:
        same = np.array_equal(p[name][1], raw[name][1])
        if name in SM.UNPERMUTED:
            assert same, name
        elif len(raw[name][1]) >= 20:                                        # (a permutation of a few ids may be the identity)
            assert not same and p[name][0] == raw[name][0], name
    assert not np.array_equal(p["E"][1], q["E"][1])


# ---- the plans

@pytest.fixture(scope="module")
def plans():
    return [SM.make_plan(seed) for seed in SM.SEEDS]


@pytest.fixture(scope="module")
def cover(plans):
    return SM.coverage(plans)


def test_plans_are_plain_printable_and_deterministic(plans):
    for seed, plan in zip(SM.SEEDS, plans):
        assert eval(repr(plan)) == plan and SM.make_plan(seed) == plan
        plain = lambda x: type(x) in (str, int, type(None)) or (type(x) is tuple and all(type(y) in (str, int) for y in x))
        assert all(plain(x) for op in plan for x in op) and all(op[0] in SM.OPS for op in plan)  # (a source-list spec is a pair)
        assert all(type(x) is not tuple or op[0] in SM.GRAPH_OWNED for op in plan for x in op)


def test_replay_of_a_prefix_reproduces_the_model_state(plans):
    for plan in plans:
        m = SM.Model()
        for i, op in enumerate(plan):
            if i % 37 == 0:
                assert SM.replay(eval(repr(plan[:i]))).snapshot() == m.snapshot(), i
            m.apply(op)


def test_plan_shape(plans, cover):
    for plan in plans:
        secs = SM.sections(plan)
        assert 6 <= len(secs) <= 8 and all(40 <= hi - lo <= 90 for _, lo, hi in secs), [(g, hi - lo) for g, lo, hi in secs]
        assert secs[-1][2] == len(plan)
        big = [SM.FACTS[g][0] >= 900 for g, _, _ in secs]
        assert sum(x != y for x, y in zip(big, big[1:])) >= 4                # larger and smaller in turn
        # every graph ends with a checkpoint: everything read, the blocks in use recorded, and once more after calls that
        # must change nothing
        for _, lo, hi in secs:
            reads = [op[1] for op in plan[lo:hi] if op[0] == "read"]
            tail = plan[hi - 27:hi]
            assert plan[hi - 1] == ("checkpoint",) and sum(op == ("checkpoint",) for op in plan[lo:hi]) == 2
            assert {op[1] for op in tail if op[0] == "read"} == set(SM.RESULTS)
    assert len(plans) == 4 and cover["n_ops"] == [len(p) for p in plans]


def test_condition_a_every_run_often_and_in_variety(cover):
    for r in SM.RESULTS:
        assert cover["runs"][r] >= 5, r
        # (four runs take no parameter, and the budget of the maximum-clique search stays at its default)
        assert cover["values"][r] >= 2 or r in SM.PARAMLESS + ("mclq",), r
    for r in SM.TRUSS_DERIVED:
        assert set(cover["kinds"][r]) >= {"whole", "vmask", "empty"}, r


def test_conditions_b_and_c_every_cell_of_the_table(cover):
    assert cover["drop_missing"] == [] and cover["drop_cells"] == (96, 96)
    assert cover["keep_missing"] == [] and cover["keep_cells"] == (470, 470)


def test_conditions_d_e_f_every_lazy_array_first_asked_for_by_each_consumer(cover):
    for c in SM.CEU_CONSUMERS:
        assert cover["ceu"][c, "first"] >= 1 and cover["ceu"][c, "later"] >= 1, c
    assert all(cover["sup_first"][c] >= 1 for c in SM.SUP_CONSUMERS)
    assert all(cover["comm_v_first"][c] >= 1 for c in SM.COMM_V_CONSUMERS)


def test_condition_g_every_refusable_run_refused_with_its_result_held(cover):
    """onion takes no argument; komb_nucleus_run, komb_community_hierarchy_run, komb_nucleus_hierarchy_run and komb_graphlets_run
    take none either, and whatever makes them KOMB_ERR_STATE (no complete k-truss result, no decomposition) has dropped their
    result before: the contract has no refusal of these five with a result of their own held, short of a failed allocation
    (tests/test_gpu_alloc_failure.py) or, for the census, a degree of 2^20.  Betweenness and distances are refused with their
    result held, and verified after, at least twice each."""
    assert set(SM.REFUSABLE) | set(SM.PARAMLESS) == set(SM.RESULTS)
    for r in SM.REFUSABLE:
        assert cover["refused"][r] >= (2 if r in SM.GRAPH_OWNED else 1), r


def test_condition_h_every_consumer_straight_after_unprepare_and_a_run(cover):
    for c in SM.CEU_CONSUMERS:
        assert cover["after_unprepare"][c] >= 1, c


def test_condition_i_size_reuse_transitions(cover):
    for t in SM.REUSE_TRANSITIONS:
        assert cover["transitions"][t] >= 1, t


def test_condition_j_graphlets_as_consumer_and_maker(cover):
    """The census is a twelfth consumer of the canonical edge list and a third maker of the canonical supports, and it runs on
    every kind of complete result (condition a has the kinds)."""
    assert cover["ceu"]["gl", "first"] >= 2 and cover["ceu"]["gl", "later"] >= 3
    assert cover["after_unprepare"]["gl"] >= 1 and cover["sup_first"]["gl"] >= 2
    assert set(cover["kinds"]["gl"]) >= {"whole", "vmask", "empty"}


def test_condition_k_runs_and_source_lists_of_the_three(cover):
    for r in ("gl",) + SM.GRAPH_OWNED:
        assert cover["runs"][r] >= 20, r
    assert SM.source_lengths() == {0, 1, 3, 65, 257, "all"}
    for r in SM.GRAPH_OWNED:
        for n in SM.source_lengths():
            assert cover["source_lists"][r, n] >= (2 if n == "all" else 1), (r, n)
        assert cover["owned_across_unprepare"][r] >= 1, r                   # held across unprepare + truss_run, read after


def test_the_gpu_module_states_these_counts(plans, cover):
    """The docstring of tests/test_gpu_analysis_sequences.py carries the operation counts: they are the plans'."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_analysis_sequences.py")).read()
    assert " / ".join(str(len(p)) for p in plans) in text
    lo, hi = cover["ops_per_graph"]
    assert re.search(r"%d \.\. %d per graph" % (lo, hi), text)
