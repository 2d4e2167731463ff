"""A model of what one komb_ctx holds, written from include/komb_accel.h, and seeded plans of calls over every entry point.

Three parts, none of which touches a GPU:
  * the catalogue: one plan tuple per public call of komb_amd/api.py (OPS below says what each tuple means);
  * Model: one method per operation; it answers the status code the header promises and keeps which graph is loaded, which of
    the nineteen results are held (with the parameters of their runs), what kind of k-truss result is current and which of
    the lazily made arrays exist.  Its drop / keep table is TABLE: one line per sentence of the header, the header's line
    number beside it;
  * make_plan(seed) / coverage(plans): the plans tests/test_gpu_analysis_sequences.py drives through one context, and what
    the set of them exercises, counted from the plans and the model alone (tests/test_sequence_model_ref.py asserts it).

A plan is a list of plain tuples: printable, and replay(plan[:i]) gives the model after any prefix."""
import numpy as np

OK, ARG, STATE = 0, -1, -5

RESULTS = ("core", "onion", "comp", "hier", "dens", "truss", "comm", "bic", "chier", "sc", "nuc", "nhier", "mclq", "cens", "mxl", "perc", "gl",
           "btw", "dist")
TRUSS_DERIVED = ("comm", "bic", "chier", "sc", "nuc", "nhier", "mclq", "cens", "mxl", "perc", "gl")
BASE = ("core", "onion", "comp", "hier", "dens")
GRAPH_OWNED = ("btw", "dist")                    # only a graph load drops them
_ALL = RESULTS
_ELEVEN = TRUSS_DERIVED

# ---- the drop / keep table: (row, the result the row computes, the results it drops, header line, the sentence)
# A row keeps every result that it neither drops nor computes.  Written from include/komb_accel.h alone.
TABLE = (
    ("load", None, _ALL, 156, "A load drops the previous graph and every result on the context before it does anything else"),
    ("load_bad", None, _ALL, 156, "... so a load that fails -- an argument, a limit -- leaves NO graph"),
    ("core", "core", (), 174, "komb_core_run computes on the device and leaves degree/coreness in HBM"),
    ("core_sharded", "core", (), 184, "All ranks end with identical, complete results, bit-equal to komb_core_run's"),
    ("onion", "onion", (), 203, "The onion uses arrays of its own: it changes no k-core, k-truss or CoreA result"),
    ("comp", "comp", (), 228, "The result is a snapshot in arrays of its own ... a call changes no k-core, k-truss, onion or CoreA result"),
    ("hier", "hier", (), 261, "The result is a snapshot in arrays of its own ... a run changes none of their results"),
    ("dens", "dens", (), 422, "loading a graph drops it, no other call changes it, a run changes no other result"),
    ("truss", "truss", _ELEVEN, 800, "A run drops the previous k-truss result, and every analysis that indexes it"),
    ("truss_vmask", "truss", _ELEVEN, 800, "... (a run under a vmask alike: a new k-truss run of any kind)"),
    ("slice", "truss", _ELEVEN, 831, "komb_truss_run_slice: a new k-truss run of any kind"),
    ("truss_sharded", "truss", _ELEVEN, 823, "komb_truss_run_sharded: world == 1 is komb_truss_run"),
    ("prepare", None, (), 811, "komb_truss_prepare makes it ahead of time (a no-op when it exists)"),
    ("unprepare", None, ("truss",) + _ELEVEN, 812, "komb_truss_unprepare drops it together with the last k-truss result"),
    ("comm", "comm", (), 295, "A communities run changes no k-core, k-truss, onion, components or CoreA result"),
    ("bic", "bic", (), 335, "k-core, onion, components, communities and CoreA calls neither change nor drop it; a run changes none of their results"),
    ("chier", "chier", (), 381, "k-core, onion, components, hierarchy, communities and CoreA calls neither change nor drop them; a run changes none of their results"),
    ("sc", "sc", (), 467, "k-core, onion, components, hierarchy, communities, densest and CoreA calls neither change nor drop it; a run changes none of their results"),
    ("nuc", "nuc", ("nhier",), 558, "whatever replaces or drops that -- a new komb_nucleus_run ... -- drops it too"),
    ("nhier", "nhier", (), 560, "No other call changes or drops it; a run changes no other result"),
    ("mclq", "mclq", (), 614, "No other call changes or drops it; a run changes no other result"),
    ("cens", "cens", (), 663, "No other call changes or drops it; a run changes no other result"),
    ("mxl", "mxl", ("perc",), 771, "It describes one maximal-cliques result and goes with it: a komb_maximal_cliques_run that succeeds ... drop it"),
    ("perc", "perc", (), 772, "No other call changes or drops it; a run changes no other result"),
    ("gl", "gl", (), 907, "It indexes one k-truss result ... No other call changes or drops it; a run changes no other result"),
    ("btw", "btw", (), 953, "It belongs to the graph: a graph load drops it.  No k-core, k-truss or other analysis call changes or drops it"),
    ("dist", "dist", (), 1002, "It belongs to the graph: a graph load drops it.  No k-core, k-truss, betweenness or other analysis call changes or drops it"),
    ("corea", None, (), 294, "k-core, onion, components and CoreA calls neither change nor drop it (CoreA works on host arrays)"),
    ("densest_block", None, (), 870, "A refusal leaves the resident graph and its results as they were (a peel over copies of the graph)"),
    ("moments", None, (), 877, "Measurement only: fills komb_stats ... makes the k-truss preparation if absent"),
    ("get_csr", None, (), 169, "Copy the resident CSR back"),
)
ROWS = tuple(t[0] for t in TABLE)
OWN = {t[0]: t[1] for t in TABLE}
DROPS = {t[0]: frozenset(t[2]) for t in TABLE}
KEEPS = {t[0]: frozenset(RESULTS) - DROPS[t[0]] - {t[1]} for t in TABLE}
HEADER_LINE = {t[0]: t[3] for t in TABLE}

# the runs of which the header says "changes ... no komb_stats field"
STATS_FROZEN = ("onion", "comp", "hier", "dens", "comm", "bic", "chier", "sc", "nuc", "nhier", "mclq", "cens", "mxl", "perc", "gl", "btw", "dist")
# who makes the canonical edge list of a whole-graph k-truss result (the header says so with each of them)
CEU_CONSUMERS = ("fetch", "sc", "cens", "comm", "bic", "comp", "hier", "chier", "mclq", "mxl", "nuc", "gl")
SUP_CONSUMERS = ("fetch_support", "sc", "gl")
COMM_V_CONSUMERS = ("vertices", "info")
# the runs that the contract can refuse while a result of their own kind is held: an argument, or (hier, comp) a partial
# k-truss result under a snapshot that does not index it.  onion has no argument; nuc, chier, nhier and gl have none either, and
# whatever makes them KOMB_ERR_STATE has dropped their result before.
REFUSABLE = ("core", "comp", "hier", "dens", "truss", "comm", "bic", "sc", "mclq", "cens", "mxl", "perc", "btw", "dist")
PARAMLESS = ("onion", "chier", "nuc", "nhier", "gl")

# ---- menus (every value is one the per-analysis tests use)
KS = (2, 3, 4, -1, "above")                       # thresholds; "above" = one above the largest (the driver resolves it)
SOME = ((3, 10, 2), (1, 2, 3), (7, 10, 3), (7, 10, 4), (1, 1, 2), (1, 100, 2), (999999, 1000000, 2))      # test_gpu_structural.SOME
WINDOWS = ((2, -1, 0), (4, -1, 0), (3, 5, 0), (2, -1, 2), (4, -1, 4), (3, 5, 3))     # (k_lo, k_hi, k_local): k_local = k_lo is always inside
K_MIN = (2, 3, 4)
ITERS = (0, 1, 8, 64)
POISON_WORDS = ("0xFFFFFFFF", "0x7FFFFFFF", "0x00000001", "0x80000000")
OPTIONS = {
    "FINISH": ("none", "lds", "local", None), "INDEX": ("two_pass", None), "LOCAL_LIMIT": ("1500", None), "NO_FIRST_QUEUE": ("1", None),
    "FULL_CAPS": ("1", None), "COMP_SAMPLE": ("0", "1", None),
    # (the two length classes are switched together, in the pairs the per-analysis tests use: lane, wave, queued)
    "COMM_SHORT+COMM_HEAVY": ("1000000000+2000000000", "1+1000000000", "1+2", None),
    "NUC_SHORT+NUC_HEAVY": ("1000000000+2000000000", "1+1000000000", "1+2", None),
    "DENSEST_LOCAL": ("0", "1", None), "BICONN_HEAVY": ("0", "1", None),
    "CENSUS_LDS": ("0", "64", None), "CENSUS_PIVOT": ("first", None), "MAXCLQ_LDS": ("0", "64", None), "MAXCLQ_SEED": ("0", None),
    "MAXIMAL_LDS": ("0", "64", None), "MAXIMAL_PIVOT": ("first", None), "PERC_GROUP": ("4", "16", "64", None),
    "GRAPHLET_SHORT": ("0", "100000", None), "GRAPHLET_LDS": ("0", "64", None), "BTW_GRID": ("2", None),
    "DIST_WORDS": ("1", "2", None), "DIST_GRID": ("2", "3", None),
}
MERGE_MAX_NV = 6000
# The restatement of the clique communities tests all pairs of member cliques: its time is quadratic in the number of maximal
# cliques of at least k vertices (A has 5105 maximal cliques, B 6743, C 8998 triangles, D 16 232; k = 2 on D takes 28 s).  On
# these four graphs k is therefore drawn from the values that leave at most about 2000 member cliques (measured: A 1733 at
# k = 5, B 1923 at k = 8, D 1851 at k = 6, C none at k = 4); every other graph takes the menu KS.
PERC_KS = {"A": (5, 6, "above"), "B": (8, 9, "above"), "C": (4, "above"), "D": (6, 8, "above")}
# The source lists of betweenness and distances are prefixes of one master list per graph (Graph.master: MASTER_LEN entries
# drawn with repeats from at most MASTER_POOL vertices), so one search per distinct vertex serves every list; "all" is
# sources == NULL.  65 entries cross a batch of betweenness and of DIST_WORDS=1, 257 one of DIST_WORDS=4.  Both references
# cost O(nv) per entry, and a run costs a few launches and a host sync per level of every batch.  The strip C is about 4500
# levels deep: as measured on the MI355X, a distance run from any vertex of it takes 0.17 s and a betweenness run 0.73 s (about
# 9000 level steps), where a whole poisoned test took 0.39 s before -- so C gets the empty list only (the measurements behind
# WALL_SECONDS of tests/test_gpu_analysis_sequences.py; tests/test_gpu_distances.py and tests/test_gpu_betweenness.py have a
# path of 3000 vertices).  The 524 549 vertices of the strided graph get three entries; every vertex is a source only up to
# SMALL_NV vertices.  On the graph without a vertex any id is KOMB_ERR_ARG.
MASTER_LEN, MASTER_POOL = 257, 40
SMALL_NV = 300
SOURCE_LENGTHS = {"A": (0, 1, 65, 257), "B": (0, 1, 65, 257), "C": (0,), "D": (0, 1, 65), "E": (0, 1, 65), "E2": (0, 1, 65),
                  "strided": (0, 1, 3), "nv0": (0, "all")}
SOURCE_LENGTHS_SMALL = (0, 1, 65, 257, "all")
BAD_SOURCES = ("id_high", "id_negative", "count")

# ---- what the plan tuples mean
OPS = {
    "load": "(g, how): komb_graph_from_edges (how = 'edges') or komb_graph_from_csr ('csr') of graph g",
    "load_bad": "(g,): komb_graph_from_edges with an endpoint == nv: KOMB_ERR_ARG and no graph",
    "core": "(how,): komb_core_run ('plain'), komb_core_run_sharded(0, 1) ('sharded') or (1, 1) ('bad': KOMB_ERR_ARG)",
    "onion": "(): komb_onion_run",
    "comp": "(kind, k): komb_components_run; kind 'core' | 'truss' | 7 (unknown)",
    "hier": "(kind,): komb_hierarchy_run",
    "dens": "(iters,): komb_densest_subgraph_run",
    "truss": "(how, mask): komb_truss_run ('plain') / komb_truss_run_sharded(0, 1) ('sharded'); mask None | 'maxcore' | 'random'",
    "slice": "(rank, world, mask): komb_truss_run_slice",
    "prepare": "(): komb_truss_prepare", "unprepare": "(): komb_truss_unprepare",
    "comm": "(k,)", "bic": "(k,)", "chier": "()", "sc": "(eps_num, eps_den, mu)", "nuc": "()", "nhier": "()", "mclq": "(budget,)",
    "cens": "(k_lo, k_hi, k_local)", "mxl": "(k_min,)", "perc": "(k,)",
    "gl": "(): komb_graphlets_run; no graph: KOMB_ERR_ARG, no complete k-truss result: KOMB_ERR_STATE; it asks for the canonical edge "
          "list and the canonical supports as the fetches do; held: (mask of the k-truss result,)",
    "btw": "(spec,): komb_betweenness_run; spec ('prefix', n): the first n entries of the graph's master list | 'all': sources == NULL | "
           "('bad', 'id_high' | 'id_negative' | 'count'): an id == nv, an id == -1, n_sources == -1: KOMB_ERR_ARG, as is a run without "
           "a graph; a refused run keeps the held result; it needs no other result; held: the spec",
    "dist": "(spec,): komb_distances_run, as btw",
    "read": "(result, arg): every count / fetch / info / list / labels / nuclei / profile call of the result; held: compared with "
            "the references, else every call must be refused.  arg: truss -- the order of _fetch_varied (0..2); comm -- which "
            "of 'vertices' | 'info' comes first; chier, nhier -- the k of _labels / _nuclei",
    "stateless": "(name,): 'corea' (fractional_ranks + get_anomaly_score) | 'densest_block' | 'moments' | 'get_csr'",
    "option": "(name, value): an option switch (None unsets); 'A+B', 'x+y' sets A = x and B = y", "poison": "(word,): a new POISON word (poisoned mode only)",
    "checkpoint": "(): every held result verified, every other one probed, pool_blocks_in_use recorded",
}

# ---- the graphs: what the model needs to know of each (tests/test_sequence_model_ref.py checks these against the graphs built)
# name: (nv, ne, edges under the max-core mask)
FACTS = {
    "A": (900, 8134, None), "B": (1100, 9418, None), "C": (9000, 17997, None), "D": (3000, 29060, None),
    "E": (1830, 1770, 1770), "E2": (1830, 1770, None),
    "hand_sc": (14, 29, None), "hand_nuc": (15, 40, None), "strided": (2048 * 256 + 257 + 4, 6, 6), "book257": (259, 581, None),
    "nv0": (0, 0, 0), "iso7": (7, 0, 0), "loops": (10, 0, 0), "edge": (2, 1, 1), "tri": (3, 3, 3),
}
UNPERMUTED = ("A", "B", "C", "D")
SMALL_NE = 50                                   # below this many edges a random 60 % mask may leave none: only the max-core mask is used
ORDERS = (("B", "A", "C", "hand_sc", "D", "iso7", "E", "E2"),
          ("A", "B", "nv0", "C", "book257", "D", "tri", "hand_nuc"),
          ("D", "edge", "B", "C", "loops", "E", "E2", "A"),
          ("strided", "hand_nuc", "B", "A", "C", "edge", "D", "book257"))
SEEDS = (11, 23, 37, 41)
REUSE_TRANSITIONS = (("B", "A"), ("A", "B"), ("A|B", "C"), ("E", "E2"))


def source_lengths():
    """Every length of the menus."""
    return {n for menu in list(SOURCE_LENGTHS.values()) + [SOURCE_LENGTHS_SMALL] for n in menu}


def source_menu(g):
    """The specs a plan may give komb_betweenness_run / komb_distances_run on graph g."""
    assert g in SOURCE_LENGTHS or FACTS[g][0] <= SMALL_NV, g
    return tuple("all" if n == "all" else ("prefix", n) for n in SOURCE_LENGTHS.get(g, SOURCE_LENGTHS_SMALL))


def _clique(ids):
    ids = np.asarray(list(ids), np.int64)
    return ids[np.stack(np.triu_indices(len(ids), 1), 1)].reshape(-1, 2)


def raw_graphs(gen, hand):
    """name -> (nv, raw pairs) in the ids they are written down in.  gen: komb_amd.gen_hug_edges; hand: the three hand graphs
    of the references as {name: (nv, pairs)}."""
    g = {"A": (900, gen(900, 2200, 2.6, 6)), "B": (1100, gen(1100, 2700, 2.2, 8)), "D": (3000, gen(3000, 7350, 2.6, 5))}
    n = 9000                                                                 # a strip of triangles: 2 n - 3 edges
    g["C"] = (n, np.concatenate([np.stack([np.arange(n - 1), np.arange(1, n)], 1), np.stack([np.arange(n - 2), np.arange(2, n)], 1)]))
    g["E"] = (1830, _clique(range(60)))                                      # K_60 and 1770 isolated vertices: m = 1770
    rng = np.random.default_rng(1830)
    pairs = set()
    while len(pairs) < 1770:                                                 # a sparse random graph with the same (nv, m)
        u, v = (int(x) for x in rng.integers(0, 1830, 2))
        if u != v:
            pairs.add((min(u, v), max(u, v)))
    g["E2"] = (1830, np.asarray(sorted(pairs), np.int64))
    for name, (nv, e) in hand.items():
        g[name] = (nv, np.asarray(e, np.int64).reshape(-1, 2))
    k = 257                                                                  # the book graph of tests/test_gpu_dirty_memory.py
    pages = np.arange(2, k + 2)
    g["book257"] = (k + 2, np.concatenate([[[0, 1]], np.stack([np.zeros(k, int), pages], 1), np.stack([np.ones(k, int), pages], 1),
                                           np.stack(np.triu_indices(12, 1), 1) + 2]))
    g["nv0"] = (0, np.zeros((0, 2), np.int64))
    g["iso7"] = (7, np.zeros((0, 2), np.int64))
    g["loops"] = (10, np.stack([np.arange(10), np.arange(10)], 1))
    g["edge"] = (2, np.asarray([[0, 1]]))
    g["tri"] = (3, np.asarray([[0, 1], [1, 2], [0, 2]]))
    return {name: (nv, np.asarray(uv, np.int64).reshape(-1, 2)) for name, (nv, uv) in g.items()}


def permuted(raw, seed):
    """The graphs of one plan: every graph except A-D gets its ids permuted by the plan's rng."""
    rng = np.random.default_rng([seed, 99])
    out = {}
    for name in sorted(raw):
        nv, uv = raw[name]
        if name not in UNPERMUTED and nv > 0:
            uv = rng.permutation(nv)[uv]
        out[name] = (nv, uv)
    return out


class Model:
    """What the header says the context holds after each call, and the status code each call answers."""

    def __init__(self, facts=FACTS):
        self.facts = facts
        self.graph = None
        self.held = {}                      # result -> the parameters of the run that made it (what a reference needs)
        self.truss = None                   # None | {"kind": whole | vmask | partial | empty, "mask": tag, "lo": , "hi": }
        self.ceu = False                    # the canonical edge list of the resident graph exists
        self.sup_ready = False              # the canonical supports of the current k-truss result exist
        self.comm_v = False                 # the per-vertex pass of the held communities has run
        self.prepared = False               # the k-truss preparation of the resident graph exists
        self.log = []                       # one record per operation: what coverage() counts

    # ---- state helpers
    def _ne(self):
        return self.facts[self.graph][1]

    def complete(self):
        return self.truss is not None and self.truss["kind"] != "partial"

    def truss_key(self):
        """What a reference of a truss-derived result is keyed by: the mask of the current result (None: the whole graph)."""
        return self.truss["mask"]

    def _drop(self, results):
        gone = [r for r in results if r in self.held]
        for r in gone:
            del self.held[r]
        if "truss" in results:
            self.truss, self.sup_ready = None, False
        if "comm" in results:
            self.comm_v = False
        return gone

    def _consume_edges(self, rec, who):
        if self.truss is not None and self.truss["kind"] in ("whole", "partial"):
            rec["ceu"] = (who, "later" if self.ceu else "first")
            self.ceu = True

    def _consume_sup(self, rec, who):
        if self.truss is not None and self.truss["kind"] in ("whole", "partial") and not self.sup_ready:
            rec["sup_first"] = who
        self.sup_ready = True

    def _derived_gate(self):
        if self.graph is None:
            return ARG
        return OK if self.complete() else STATE

    # ---- the dispatcher
    def apply(self, op):
        rec = {"i": len(self.log), "op": op, "graph": self.graph, "held_before": frozenset(self.held), "row": None, "dropped": (),
               "truss_kind": self.truss["kind"] if self.truss else None, "params_before": dict(self.held)}
        code = getattr(self, "op_" + op[0])(rec, *op[1:])
        rec["code"] = code
        rec["held_after"] = frozenset(self.held)
        self.log.append(rec)
        return code

    def _ran(self, rec, row, params=None):
        """Row `row` of the table took effect."""
        rec["row"] = row
        rec["dropped"] = tuple(self._drop(DROPS[row]))
        if OWN[row] is not None:
            self.held[OWN[row]] = params
            rec["ran"] = OWN[row]
        return OK

    def _refused(self, rec, result, code):
        rec["refused"] = result
        return code

    # ---- graph loads
    def op_load(self, rec, g, how):
        self._ran(rec, "load")
        self.graph, self.ceu, self.prepared = g, False, False
        return OK

    def op_load_bad(self, rec, g):
        self._ran(rec, "load_bad")
        self.graph, self.ceu, self.prepared = None, False, False
        return ARG

    # ---- the five analyses of the resident graph
    def op_core(self, rec, how):
        if how == "bad":
            return self._refused(rec, "core", ARG)
        if self.graph is None:
            return self._refused(rec, "core", STATE)
        return self._ran(rec, "core" if how == "plain" else "core_sharded", (how,))

    def op_onion(self, rec):
        if self.graph is None:
            return self._refused(rec, "onion", ARG)
        return self._ran(rec, "onion", ())

    def _kind_gate(self, kind, needs_core):
        if kind == "core":
            return STATE if needs_core and "core" not in self.held else OK
        return OK if self.complete() else STATE

    def op_comp(self, rec, kind, k):
        if self.graph is None or kind not in ("core", "truss") or (k != "above" and k < -1):
            return self._refused(rec, "comp", ARG)
        if self._kind_gate(kind, k != 0) != OK:
            return self._refused(rec, "comp", STATE)
        if kind == "truss":
            self._consume_edges(rec, "comp")
        return self._ran(rec, "comp", (kind, k, self.truss_key() if kind == "truss" else None))

    def op_hier(self, rec, kind):
        if self.graph is None or kind not in ("core", "truss"):
            return self._refused(rec, "hier", ARG)
        if self._kind_gate(kind, True) != OK:
            return self._refused(rec, "hier", STATE)
        if kind == "truss":
            self._consume_edges(rec, "hier")
        return self._ran(rec, "hier", (kind, self.truss_key() if kind == "truss" else None))

    def op_dens(self, rec, iters):
        if self.graph is None or iters < 0:
            return self._refused(rec, "dens", ARG)
        if "core" not in self.held:
            return self._refused(rec, "dens", STATE)
        return self._ran(rec, "dens", (iters,))

    # ---- k-truss
    def _truss_ran(self, rec, row, mask, rank=0, world=1):
        self._ran(rec, row)
        ne = self._ne()
        if mask is not None:
            sub = self.facts[self.graph][2] if mask == "maxcore" else None
            kind, lo, hi = ("empty" if (ne == 0 or sub == 0) else "vmask"), 0, None
        elif ne == 0:
            kind, lo, hi = "empty", 0, 0
        else:
            lo, hi = ne * rank // world, ne * (rank + 1) // world
            kind = "whole" if (lo, hi) == (0, ne) else "partial"
            self.prepared = True
        self.truss = {"kind": kind, "mask": mask, "lo": lo, "hi": hi}
        self.held["truss"] = (mask, lo, hi)
        self.sup_ready = kind in ("vmask", "empty")
        rec["truss_after"] = kind
        return OK

    def op_truss(self, rec, how, mask):
        if self.graph is None:
            return self._refused(rec, "truss", STATE)
        return self._truss_ran(rec, "truss_sharded" if how == "sharded" else "truss_vmask" if mask else "truss", mask)

    def op_slice(self, rec, rank, world, mask):
        if world < 1 or rank < 0 or rank >= world:
            return self._refused(rec, "truss", ARG)
        if self.graph is None:
            return self._refused(rec, "truss", STATE)
        return self._truss_ran(rec, "slice", mask, rank, world)

    def op_prepare(self, rec):
        if self.graph is None:
            return STATE
        self._ran(rec, "prepare")
        self.prepared = self.prepared or self._ne() > 0
        return OK

    def op_unprepare(self, rec):
        self._ran(rec, "unprepare")
        self.prepared = False
        return OK

    # ---- the eleven analyses of a k-truss result
    def _derived(self, rec, result, params, bad_arg=False, consumes=True, extra_state=False):
        if self.graph is None or bad_arg:
            return self._refused(rec, result, ARG)
        if not self.complete() or extra_state:
            return self._refused(rec, result, STATE)
        if consumes:
            self._consume_edges(rec, result)
        return self._ran(rec, result, params + (self.truss_key(),))

    def op_comm(self, rec, k):
        code = self._derived(rec, "comm", (k,), bad_arg=k != "above" and k < -1)
        if code == OK:
            self.comm_v = False
        return code

    def op_bic(self, rec, k):
        return self._derived(rec, "bic", (k,), bad_arg=k != "above" and k < -1)

    def op_chier(self, rec):
        return self._derived(rec, "chier", ())

    def op_sc(self, rec, eps_num, eps_den, mu):
        code = self._derived(rec, "sc", (eps_num, eps_den, mu), bad_arg=not (1 <= eps_num <= eps_den <= 1000000 and mu >= 2))
        if code == OK:
            self._consume_sup(rec, "sc")
        return code

    def op_nuc(self, rec):
        return self._derived(rec, "nuc", ())

    def op_nhier(self, rec):
        return self._derived(rec, "nhier", (), consumes=False, extra_state="nuc" not in self.held)

    def op_mclq(self, rec, budget):
        return self._derived(rec, "mclq", (), bad_arg=budget < 0)

    def op_cens(self, rec, k_lo, k_hi, k_local):
        bad = k_lo < 2 or (k_hi != -1 and k_hi < k_lo) or k_local not in (0, k_lo)
        return self._derived(rec, "cens", (k_lo, k_hi, k_local), bad_arg=bad)

    def op_mxl(self, rec, k_min):
        return self._derived(rec, "mxl", (k_min,), bad_arg=k_min < 2)

    def op_perc(self, rec, k):
        bad = k != "above" and k < 2
        no_list = "mxl" not in self.held or (k != "above" and self.held["mxl"][0] > k)
        if self.graph is not None and not bad and self.complete() and not no_list:
            return self._ran(rec, "perc", (k, self.held["mxl"][0], self.truss_key()))
        return self._derived(rec, "perc", (k,), bad_arg=bad, consumes=False, extra_state=True)

    def op_gl(self, rec):
        code = self._derived(rec, "gl", ())
        if code == OK:
            self._consume_sup(rec, "gl")
        return code

    # ---- the two analyses that belong to the graph
    def _graph_owned(self, rec, result, spec):
        if self.graph is None or (spec != "all" and spec[0] == "bad"):
            return self._refused(rec, result, ARG)
        assert spec in source_menu(self.graph), (self.graph, spec)
        return self._ran(rec, result, spec)

    def op_btw(self, rec, spec):
        return self._graph_owned(rec, "btw", spec)

    def op_dist(self, rec, spec):
        return self._graph_owned(rec, "dist", spec)

    # ---- readers
    def op_read(self, rec, result, arg=None):
        rec["read"] = result
        if result not in self.held:
            no_graph = ARG if result not in ("core", "truss") else STATE
            return no_graph if self.graph is None else STATE
        if result == "truss":
            if arg == 0:
                self._consume_sup(rec, "fetch_support")
            self._consume_edges(rec, "fetch")
            self._consume_sup(rec, "fetch_support")
        if result == "comm":
            if not self.comm_v:
                rec["comm_v_first"] = arg
            self.comm_v = True
        rec["verified"] = result
        return OK

    def op_stateless(self, rec, name):
        if name == "corea":
            self._ran(rec, "corea")
            return OK
        if self.graph is None:
            return STATE
        self._ran(rec, name)
        if name == "moments":
            self.prepared = self.prepared or self._ne() > 0
        return OK

    def op_option(self, rec, name, value):
        return OK

    def op_poison(self, rec, word):
        return OK

    def op_checkpoint(self, rec):
        rec["checkpoint"] = (self.graph, frozenset(self.held))
        return OK

    def snapshot(self):
        return (self.graph, dict(self.held), None if self.truss is None else dict(self.truss), self.ceu, self.sup_ready, self.comm_v, self.prepared)


def replay(plan, facts=FACTS):
    m = Model(facts)
    for op in plan:
        m.apply(op)
    return m


# ---- the plan generator

class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng([seed, 7])
        self.m = Model()
        self.plan = []
        self.turn = {}

    def spec(self, r):
        """The source lists of a menu in turn, over all the graphs of the plan that share the menu: every vertex (where the
        menu has it), the longest prefix, the empty one, the others from long to short, and round again -- so a menu that
        only one graph has meets its longest list, whatever else the plan does on that graph."""
        menu = source_menu(self.m.graph)
        prefixes = sorted((s for s in menu if s != "all"), reverse=True)
        menu = tuple(s for s in menu if s == "all") + tuple(prefixes[:1] + prefixes[-1:] + prefixes[1:-1])
        self.turn[r, menu] = self.turn.get((r, menu), -1) + 1
        return menu[self.turn[r, menu] % len(menu)]

    def pick(self, menu):
        return menu[int(self.rng.integers(0, len(menu)))]

    def emit(self, *op):
        self.plan.append(op)
        return self.m.apply(op)

    def small(self):
        return self.m.graph is None or FACTS[self.m.graph][1] < SMALL_NE

    def mask(self):
        return "maxcore" if self.small() else self.pick(("maxcore", "random"))

    # -- one run of each kind, with what it needs
    def whole(self):
        if not self.m.complete():
            self.emit("truss", "plain", None)

    def params(self, r):
        if r == "core": return ("core", self.pick(("plain", "plain", "sharded")))
        if r == "onion": return ("onion",)
        if r == "comp":
            kind = "truss" if self.m.complete() and self.rng.random() < 0.6 else "core"
            return ("comp", kind, self.pick(KS + (0,)) if kind == "core" else self.pick(KS))
        if r == "hier": return ("hier", "truss" if self.m.complete() and self.rng.random() < 0.5 else "core")
        if r == "dens": return ("dens", self.pick(ITERS))
        if r == "truss": return ("truss", "plain", None)
        if r in ("comm", "bic"): return (r, self.pick(KS))
        if r == "sc": return ("sc",) + self.pick(SOME)
        if r == "mclq": return ("mclq", 0)
        if r == "cens": return ("cens",) + self.pick(WINDOWS)
        if r == "mxl": return ("mxl", self.pick(K_MIN))
        if r == "perc":
            menu = PERC_KS.get(self.m.graph, (2, 3, 4, "above"))
            return ("perc", self.pick(tuple(k for k in menu if k == "above" or k >= self.m.held["mxl"][0])))
        if r in GRAPH_OWNED: return (r, self.spec(r))
        return (r,)

    def run(self, r):
        """One successful run of result r, after whatever it needs."""
        if r in TRUSS_DERIVED:
            self.whole()
        if r == "nhier" and "nuc" not in self.m.held: self.emit("nuc")
        if r == "perc" and "mxl" not in self.m.held: self.emit("mxl", self.pick(K_MIN))
        if r in ("comp", "hier", "dens") and "core" not in self.m.held:
            self.emit("core", "plain")
        op = self.params(r)
        assert self.emit(*op) == OK, op

    def read(self, r):
        arg = {"truss": int(self.rng.integers(0, 3)), "comm": self.pick(COMM_V_CONSUMERS), "chier": self.pick(KS + (0,)),
               "nhier": self.pick((1, 2, -1, 0, "above"))}.get(r)
        return self.emit("read", r, arg)

    def do_row(self, row, full, reads=True):
        """Row `row` of the table with results held around it: every cell of the row that can be reached is exercised -- the
        results held before are read after (verified where the row keeps them, probed where it drops them)."""
        m = self.m
        # what the row itself needs
        if row in TRUSS_DERIVED:
            self.whole()
            if row == "nhier" and "nuc" not in m.held: self.emit("nuc")
            if row == "perc" and "mxl" not in m.held: self.emit("mxl", 2)
        if row in ("dens",) and "core" not in m.held: self.emit("core", "plain")
        # hold the others (those the row's own prerequisites would drop come after them)
        for r in RESULTS:
            if r not in m.held and (full or self.rng.random() < 0.35):
                self.run(r)
        before = [r for r in RESULTS if r in m.held]
        g = m.graph
        if row == "load": self.emit("load", g, self.pick(("edges", "csr")))                # (reads below: everything is gone)
        elif row == "load_bad": self.emit("load_bad", g)
        elif row == "core_sharded": self.emit("core", "sharded")
        elif row == "core": self.emit("core", "plain")
        elif row == "truss": self.emit("truss", "plain", None)
        elif row == "truss_vmask": self.emit("truss", "plain", self.mask())
        elif row == "truss_sharded": self.emit("truss", "sharded", self.pick((None, self.mask())))
        elif row == "slice":
            world = int(self.rng.integers(1, 5))
            self.emit("slice", int(self.rng.integers(0, world)), world, None)
        elif row in ("prepare", "unprepare"): self.emit(row)
        elif row in ("corea", "densest_block", "moments", "get_csr"):
            if row != "densest_block" or FACTS[g][0] <= MERGE_MAX_NV:
                self.emit("stateless", row)
        else:
            self.run(row)
        if not reads:                                                        # (the checkpoint that follows reads everything)
            return
        order = list(before)
        self.rng.shuffle(order)
        for r in order:
            self.read(r)
        if row == "load_bad":
            self.emit("load", g, "edges")

    def refusal(self, r):
        """Result r held, a run of its kind refused, r verified."""
        if r not in self.m.held:
            self.run(r)
        self.bad_run(r)
        self.read(r)

    def bad_run(self, r):
        bad = {"core": ("core", "bad"), "comp": ("comp", self.pick(("core", "truss", 7)), -2), "hier": ("hier", 7), "dens": ("dens", -1),
               "truss": ("slice", 2, 2, None), "comm": ("comm", -2), "bic": ("bic", -3), "sc": ("sc",) + self.pick(((0, 10, 2), (11, 10, 2), (1, 2, 1))),
               "mclq": ("mclq", -1), "cens": ("cens",) + self.pick(((1, -1, 0), (4, 3, 0))), "mxl": ("mxl", 1), "perc": ("perc", 1),
               "btw": ("btw", ("bad", self.pick(BAD_SOURCES))), "dist": ("dist", ("bad", self.pick(BAD_SOURCES)))}[r]
        if r == "comp" and bad[1] == 7:
            bad = ("comp", 7, 2)
        assert self.emit(*bad) in (ARG, STATE)

    def state_refusals(self):
        """A partial slice: every truss-derived run and the truss kinds of comp and hier answer KOMB_ERR_STATE, while the
        snapshots of the core kind stay readable and the analyses that belong to the graph run as ever."""
        if FACTS[self.m.graph][1] < 2:
            return
        if "core" not in self.m.held: self.emit("core", "plain")
        self.emit("comp", "core", self.pick((0, 2, -1)))
        self.emit("hier", "core")
        world = int(self.rng.integers(2, 5))
        self.emit("slice", int(self.rng.integers(0, world)), world, None)
        self.read("truss")
        for op in (("comp", "truss", 3), ("hier", "truss"), ("comm", 3), ("bic", 2), ("chier",), ("sc", 1, 2, 3), ("nuc",), ("nhier",), ("mclq", 0),
                   ("cens", 2, -1, 0), ("mxl", 2), ("perc", 3), ("gl",)):
            assert self.emit(*op) == STATE
        self.read("comp"); self.read("hier")
        for r in GRAPH_OWNED:
            self.run(r)
            assert self.read(r) == OK
        self.emit("slice", 0, 1, None)                                       # the whole range is a whole result
        self.run(self.pick(TRUSS_DERIVED))

    def after_unprepare(self, consumer):
        """unprepare + truss_run, then straight away a run that has to make (or find) the canonical edge list; what belongs to
        the graph is held across the three and read after them."""
        for r in GRAPH_OWNED:
            if r not in self.m.held:
                self.run(r)
        self.emit("unprepare")
        self.emit("truss", self.pick(("plain", "plain", "sharded")), None)
        self.consumer(consumer)
        for r in GRAPH_OWNED:
            assert self.read(r) == OK

    def consumer(self, c):
        if c == "fetch": self.emit("read", "truss", 2)
        elif c == "comp": self.emit("comp", "truss", self.pick(KS)); self.read("comp")
        elif c == "hier": self.emit("hier", "truss"); self.read("hier")
        else:
            assert self.emit(*self.params(c)) == OK
            self.read(c)

    def sweep(self, mask):
        """A k-truss result under a mask (or of a graph without edges), then each of the eleven analyses on it."""
        self.emit("truss", self.pick(("plain", "sharded")), mask) if mask else self.emit("truss", "plain", None)
        order = list(TRUSS_DERIVED)
        self.rng.shuffle(order)
        for r in order:
            self.run(r)
            if r not in ("nuc", "mxl"):
                self.read(r)
        self.read("nuc"); self.read("mxl"); self.read("truss")

    def graph_owned(self):
        """Betweenness and distances, in either order, a refused run of the first one, then both read."""
        order = list(GRAPH_OWNED)
        self.rng.shuffle(order)
        for r in order:
            self.run(r)
        self.bad_run(order[0])
        for r in order:
            assert self.read(r) == OK

    def noise(self):
        x = self.rng.random()
        if x < 0.4:
            name = self.pick(tuple(sorted(OPTIONS)))
            self.emit("option", name, self.pick(OPTIONS[name]))
        elif x < 0.55:
            self.emit("poison", self.pick(POISON_WORDS))
        elif x < 0.7:
            self.emit("prepare")
        else:
            name = self.pick(("corea", "densest_block", "moments", "get_csr"))
            if name != "densest_block" or FACTS[self.m.graph][0] <= MERGE_MAX_NV:
                self.emit("stateless", name)

    def checkpoint(self):
        """Everything read (held: verified; gone: probed), the pool's blocks in use recorded -- and once more after calls that
        must leave the context as it is: refused runs, CoreA, the CSR copied back."""
        for r in RESULTS:
            self.read(r)
        self.emit("checkpoint")
        held = [r for r in REFUSABLE if r in self.m.held]
        self.rng.shuffle(held)
        for r in held[:2]:
            self.bad_run(r)
        self.emit("stateless", self.pick(("corea", "get_csr")) if self.m.graph is not None else "get_csr")
        self.emit("checkpoint")


def make_plan(seed):
    """The plan of one seed: a list of plain tuples.  The seeds of SEEDS share the directed work between them (which rows of
    the table a plan exercises with everything held, which consumer comes first on which graph); the rng decides parameters,
    orders, options and the filling."""
    index = SEEDS.index(seed) if seed in SEEDS else seed % len(SEEDS)
    gen = _Gen(seed)
    n_sec = 0
    for sec, g in enumerate(ORDERS[index]):
        start = len(gen.plan)
        if gen.rng.random() < 0.3 or sec == 1:
            gen.emit("load_bad", g)
            gen.read(gen.pick(RESULTS))
        gen.emit("load", g, "csr" if (sec + index) % 3 == 1 else "edges")
        edges = FACTS[g][1] > 0
        # what belongs to the graph: on the blocks the graph before left (even sections), or on those of the opening (odd)
        if sec % 2 == 0:
            gen.graph_owned()
        if edges:
            # the opening: a whole result and a designated first consumer of the canonical edge list
            n = index * 6 + n_sec
            n_sec += 1
            gen.emit("core", "plain")
            gen.emit("truss", "plain", None)
            first = CEU_CONSUMERS[n % len(CEU_CONSUMERS)]
            gen.consumer(first)
            gen.read("truss")                                               # (the whole result itself, while it is the current one)
            gen.noise()
        if sec % 2 == 1:
            gen.graph_owned()
        if edges:
            gen.noise()
            if n % 3 == 0:
                gen.state_refusals()
            elif n % 3 == 1:
                gen.sweep(gen.mask())
            else:
                k = 2 * (n // 3)
                gen.after_unprepare(CEU_CONSUMERS[k % len(CEU_CONSUMERS)])
                gen.after_unprepare(CEU_CONSUMERS[(k + 1) % len(CEU_CONSUMERS)])
            gen.refusal(REFUSABLE[n % len(REFUSABLE)])
        else:
            gen.sweep(None if sec % 2 else "maxcore")
        # the filling: light rows, options, stateless calls, refusals
        guard = 0
        while len(gen.plan) - start < 30 and guard < 40:
            guard += 1
            x = gen.rng.random()
            if x < 0.5:
                gen.do_row(gen.pick(ROWS[2:]), full=False)
            elif x < 0.8:
                gen.noise()
            else:
                gen.refusal(gen.pick(REFUSABLE))
        # one row of the table with everything held, the rows dealt round-robin over the sections of the four plans; the
        # checkpoint's reads are the row's: what it keeps is verified, what it drops is probed
        rows = [r for i, r in enumerate(ROWS) if i % len(SEEDS) == index]
        if sec < len(rows):
            gen.do_row(rows[sec], full=True, reads=False)
        gen.checkpoint()
    return gen.plan


# ---- plan accounting

def sections(plan):
    """[(graph, first index, last index + 1)]: the stretches of the plan that end with a checkpoint, one per graph."""
    out, lo, g, n = [], 0, None, 0
    for i, op in enumerate(plan):
        if op[0] == "load":
            g = op[1]
        if op[0] == "checkpoint":
            n += 1
            if n % 2 == 0:                                                   # (a graph ends with a pair of checkpoints)
                out.append((g, lo, i + 1))
                lo = i + 1
    return out


def coverage(plans, facts=FACTS):
    """What the plans exercise, from the plans and the model alone: a dict of the counts behind conditions a-k."""
    runs = {r: 0 for r in RESULTS}
    values = {r: set() for r in RESULTS}
    kinds = {r: set() for r in TRUSS_DERIVED}
    drop_cells, keep_cells = set(), set()
    ceu = {(c, w): 0 for c in CEU_CONSUMERS for w in ("first", "later")}
    sup = {c: 0 for c in SUP_CONSUMERS}
    comm_v = {c: 0 for c in COMM_V_CONSUMERS}
    refused = {r: 0 for r in REFUSABLE}
    after_unprep = {c: 0 for c in CEU_CONSUMERS}
    transitions = {t: 0 for t in REUSE_TRANSITIONS}
    specs = {(r, n): 0 for r in GRAPH_OWNED for n in source_lengths()}
    owned_across = {r: 0 for r in GRAPH_OWNED}
    n_ops, per_graph = [], []
    for plan in plans:
        log = replay(plan, facts).log
        n_ops.append(len(plan))
        pending_drop, pending_keep, pending_refused = {}, {}, {}     # result -> the cells waiting for its next read
        for rec in log:
            op, code = rec["op"], rec["code"]
            ran, row = rec.get("ran"), rec["row"]
            if ran is not None:
                runs[ran] += 1
                values[ran].add(op)
                if ran in kinds:
                    kinds[ran].add(rec["truss_kind"])
            # a run of Y, refused or not, ends the wait of the cells on Y (b: probed before it is run again)
            touched = ran or rec.get("refused")
            if touched:
                pending_drop.pop(touched, None)
            if row is not None:
                for y in rec["dropped"]:
                    pending_drop.setdefault(y, set()).add((row, y))
                    pending_keep.pop(y, None)
                    pending_refused.pop(y, None)
                if ran is not None:
                    pending_keep.pop(ran, None)
                    pending_refused.pop(ran, None)
                for y in rec["held_before"] & KEEPS[row] & rec["held_after"]:
                    pending_keep.setdefault(y, set()).add((row, y))
            if rec.get("refused") in rec["held_before"] and rec.get("refused") in REFUSABLE:
                pending_refused[rec["refused"]] = True
            if "read" in rec:
                y = rec["read"]
                if code == OK:
                    keep_cells |= pending_keep.pop(y, set())
                    if pending_refused.pop(y, None):
                        refused[y] += 1
                else:
                    drop_cells |= pending_drop.pop(y, set())
            if "ceu" in rec:
                ceu[rec["ceu"]] += 1
            if "sup_first" in rec:
                sup[rec["sup_first"]] += 1
            if "comm_v_first" in rec:
                comm_v[rec["comm_v_first"]] += 1
        for rec in log:
            if rec.get("ran") in GRAPH_OWNED:
                specs[rec["ran"], rec["op"][1] if rec["op"][1] == "all" else rec["op"][1][1]] += 1
        for i in range(2, len(log)):
            if log[i - 2]["op"][0] == "unprepare" and log[i - 1].get("truss_after") == "whole" and "ceu" in log[i]:
                after_unprep[log[i]["ceu"][0]] += 1
                for r in GRAPH_OWNED:                    # held before the unprepare, read before it is run again
                    later = next((x for x in log[i + 1:] if x.get("ran") == r or x.get("read") == r), None)
                    if r in log[i - 2]["held_before"] and later is not None and later.get("verified") == r:
                        owned_across[r] += 1
        secs = sections(plan)
        ran_in = [{log[i]["ran"] for i in range(lo, hi) if log[i].get("ran")} for _, lo, hi in secs]
        per_graph += [hi - lo for _, lo, hi in secs]
        for (ga, _, _), (gb, _, _), ra, rb in zip(secs, secs[1:], ran_in, ran_in[1:]):
            for t in REUSE_TRANSITIONS:
                if ga in t[0].split("|") and gb == t[1] and len(ra & rb) >= 3:
                    transitions[t] += 1
    all_drop = {(x, y) for x in ROWS for y in DROPS[x]}
    all_keep = {(x, y) for x in ROWS for y in KEEPS[x]}
    return {"n_ops": n_ops, "ops_per_graph": (min(per_graph), max(per_graph)), "runs": runs,
            "values": {r: len(v) for r, v in values.items()}, "kinds": {r: sorted(k, key=str) for r, k in kinds.items()},
            "drop_cells": (len(drop_cells & all_drop), len(all_drop)), "drop_missing": sorted(all_drop - drop_cells),
            "keep_cells": (len(keep_cells & all_keep), len(all_keep)), "keep_missing": sorted(all_keep - keep_cells),
            "ceu": ceu, "sup_first": sup, "comm_v_first": comm_v, "refused": refused, "after_unprepare": after_unprep,
            "transitions": transitions, "source_lists": specs, "owned_across_unprepare": owned_across}


# ---- expected values: base inputs from the oracle, results from the restatements of tests/*_ref.py

def hand_graphs():
    import hierarchy_ref, nucleus_ref, structural_ref
    return {"hand_sc": structural_ref.hand_graph(), "hand_nuc": nucleus_ref.hand_graph(), "strided": hierarchy_ref.strided_claim_graph()}


def master_sources(name, nv, deg):
    """The master source list of a graph (in the ids the plan loads it with): MASTER_LEN entries drawn with repeats, in no
    order, from at most MASTER_POOL distinct vertices; it starts at the vertex of largest degree and has an isolated vertex
    among its first five entries where the graph has one.  Seeded from the graph's name and nv; none on the empty graph."""
    if nv == 0:
        return []
    rng = np.random.default_rng([nv] + [ord(c) for c in name])
    hub, isolated = int(np.argmax(deg)), np.flatnonzero(np.asarray(deg) == 0)[:1].tolist()
    pool = np.unique(np.concatenate([rng.permutation(nv)[:MASTER_POOL - 2], [hub], isolated]).astype(np.int64))
    master = rng.choice(pool, size=MASTER_LEN).tolist()
    master[0] = hub
    if isolated:
        master[3] = isolated[0]
    return [int(v) for v in master]


class Graph:
    """Everything the oracle says about one graph, and the restatements' results on it: computed once, never changed."""

    def __init__(self, O, name, nv, uv):
        self.name, self.nv, self.uv = name, nv, np.ascontiguousarray(uv, np.int64)
        self.rowptr, self.col = O.simplify(nv, self.uv)
        self.deg = O.degree(self.rowptr)
        self.core = O.coreness(self.rowptr, self.col)
        eu, ev = O.edge_list(self.rowptr, self.col)
        sup, self.tri = O.support(self.rowptr, self.col)
        self.base = {None: (eu, ev, O.trussness(self.rowptr, self.col), sup)}
        kmax = int(self.core.max()) if nv else 0
        self.masks = {"maxcore": (self.core == kmax).astype(np.uint8),
                      "random": (np.random.default_rng(nv + 5).random(nv) < 0.6).astype(np.uint8)}
        for tag, m in self.masks.items():
            srp, scol, _ = O.induced_subgraph(self.rowptr, self.col, m)
            self.base[tag] = tuple(O.trussness_induced(self.rowptr, self.col, m)) + (O.support(srp, scol)[0],)
        self.rd = O.fractional_rank_fast(self.deg.astype(np.int64))
        self.rk = O.fractional_rank_fast(self.core.astype(np.int64) * nv + self.deg)
        self.score = O.corea_scores(self.deg, self.core)
        self.merge = O.run_merge(self.rowptr, self.col) if 0 < nv <= MERGE_MAX_NV else None
        self.master = master_sources(name, nv, self.deg)
        self.searches = {"btw": {}, "dist": {}}            # the cache= of the two references: one search per distinct vertex
        self.refs, self.seconds = {}, 0.0

    def sources(self, spec):
        """The source list of a plan's spec: None for every vertex, else a prefix of the master list."""
        return None if spec == "all" else self.master[:spec[1]]

    def ne(self, mask=None):
        return len(self.base[mask][0])

    def t_max(self, mask, floor):
        tr = self.base[mask][2]
        return max(int(tr.max()), floor) if len(tr) else floor

    def k_max_core(self):
        return int(self.core.max()) if self.nv else 0

    def ref(self, key, make):
        """The restatement's result for key = (analysis, parameters, mask), computed once."""
        import time
        if key not in self.refs:
            t = time.perf_counter()
            self.refs[key] = make()
            self.seconds += time.perf_counter() - t
        return self.refs[key]


def build_graphs(gen, O, seed):
    """{name: Graph} of one plan: ids permuted by the plan's rng for every graph except A-D."""
    return {name: Graph(O, name, nv, uv) for name, (nv, uv) in permuted(raw_graphs(gen, hand_graphs()), seed).items()}
