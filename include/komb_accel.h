/*
 * komb_accel.h -- C ABI of the MI355X-native k-core / k-truss / CoreA path, and of the analyses of a k-truss result built on
 * it: components, communities, hierarchies, densest subgraph, structural clusters, nuclei, maximum and maximal cliques, the
 * clique census and the k-clique communities (clique percolation).
 *
 * This is the drop-in boundary for KOMB's decomposition hot path: each entry
 * point replaces the igraph / CoreA call group named beside it (paths are
 * relative to the KOMB reference tree).  Plain pointers and sizes only; the
 * caller allocates every output; the library never frees caller memory; all
 * device state lives behind the opaque komb_ctx.  Every function returns
 * KOMB_OK (0) or a negative komb_status; komb_last_error() gives the text.
 * There is no CPU fallback: without a usable gfx950 device every compute
 * entry point fails with KOMB_ERR_DEVICE.
 *
 * Edge identity across the boundary is the canonical pair (min(u,v),max(u,v))
 * in lexicographic order -- igraph's internal edge ids are not observable in
 * any KOMB output (src/graph.cpp:519-534 only maps edges back to vertices).
 *
 * Threading: call from one host thread per context (the reference reaches this
 * seam from its main thread, src/graph.cpp:449 and src/komb2.cpp:132).
 */
#ifndef KOMB_ACCEL_H
#define KOMB_ACCEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KOMB_ACCEL_ABI_VERSION 7

typedef enum komb_status {
    KOMB_OK          =  0,
    KOMB_ERR_ARG     = -1,   /* bad argument / out-of-range id / an analysis without a graph */
    KOMB_ERR_DEVICE  = -2,   /* no HIP device, or a HIP call failed                 */
    KOMB_ERR_NOMEM   = -3,   /* host or device allocation failed                    */
    KOMB_ERR_LIMIT   = -4,   /* graph exceeds the 32-bit slot/edge-id design limits */
    KOMB_ERR_STATE   = -5    /* call order violated (fetch before run, k-core / k-truss without a graph) */
} komb_status;

typedef struct komb_ctx komb_ctx;

typedef struct komb_opts {
    int32_t device;        /* HIP device ordinal (LOCAL_RANK for one process per GPU) */
    int32_t verbosity;     /* 0 silent, 1 progress on stderr, 2 + phase times of create / graph build */
    int32_t reserved[2];   /* [0]: KOMB_CREATE_* flags below; [1]: 0                  */
} komb_opts;
/* komb_opts.reserved[0] (ABI version 7; until then the library read KOMB_NULL_STREAM / KOMB_NO_WARMUP from the environment) */
#define KOMB_CREATE_NULL_STREAM 1   /* work on the legacy default stream instead of a stream of the context's own      */
#define KOMB_CREATE_NO_WARMUP   2   /* do not load the code object (a first kernel launch) inside komb_create           */
#define KOMB_CREATE_WARM_UPLOAD 4   /* make the pinned staging buffers of a >= 64 MB graph upload inside komb_create   */

typedef struct komb_stats {
    int64_t nv, ne;                 /* simple graph: vertices, undirected edges      */
    int64_t triangles;              /* T (sum of supports / 3), after komb_truss_run */
    int64_t sum_deg_sq;             /* sum_v d(v)^2 = sum_{(u,v) in E} d(u)+d(v)      */
    int64_t wedge_items;            /* sum_{(u,v) in E} min(d(u),d(v))                */
    int64_t oriented_items;         /* sum_{(a->b)} d+(a)+d+(b), (degree,id) orientation */
    int32_t max_degree, max_coreness, max_trussness;
    int32_t core_levels, core_subrounds;    /* populated levels; PROCESS sub-rounds   */
    int32_t core_launches, truss_tail_runs; /* launches issued; hand-overs to the LDS tail kernel */
    int32_t truss_levels, truss_subrounds;  /* populated levels; PROCESS sub-rounds   */
    int32_t truss_scans, truss_launches;    /* SCAN launches; launches issued         */
    /* HIP-event times (ms), each measured on the stream the kernels run on */
    double  ms_build;               /* a1: edge list -> simple CSR                    */
    double  ms_core;                /* a2+a3: degree + k-core peel launches           */
    double  ms_orient;              /* truss: induced-subgraph filter + its per-vertex lines (0 for the whole graph: the oriented CSR comes with the graph) */
    double  ms_tri_count;           /* truss: triangle enumeration, support counting  */
    double  ms_tri_fill;            /* truss: triangle enumeration, incidence fill    */
    double  ms_compact;             /* truss: blocks + sorted records (or bounded slices) -> dense index */
    double  ms_support;             /* = ms_tri_count + ms_tri_fill + ms_sort + ms_compact */
    double  ms_allreduce;           /* truss: support all-reduce callback (sharded)   */
    double  ms_peel;                /* truss: all peel launches (SCAN + PROCESS)      */
    double  ms_gather;              /* truss: canonical-order result gather           */
    double  ms_corea;               /* a9/a10: CoreA rank kernels                     */
    double  ms_tail;                /* truss: setup + LDS tail kernel, part of ms_peel */
    /* local finish (h-index fixed point on the remainder the peel hands over; ABI version 2) */
    int64_t core_local_items, truss_local_items;   /* entries of the compact index            */
    int32_t core_local_units, core_local_sweeps;   /* vertices handed over; sweeps to the fixed point */
    int32_t truss_local_units, truss_local_sweeps; /* edges handed over; sweeps                */
    double  ms_core_local;          /* part of ms_core: numbering + collect + sweeps + scatter */
    double  ms_truss_local;         /* part of ms_peel                                         */
    /* index build by record stream (ABI version 3) */
    double  ms_sort;                /* truss: sort of the incidence records by destination edge */
    int64_t tri_records;            /* truss: record positions of the stream (incl. unused claim tails) */
    int32_t index_layout;           /* truss: 0 = record stream, 1 = bounded slices, 2 = exact two-pass */
    /* sharded peel (ABI version 4): the last komb_core_run_sharded / komb_truss_run_sharded with komb_set_shard_peel */
    int32_t shard_exchanges;        /* all-reduce callbacks made by the peel (two per sub-round + level changes) */
    double  ms_exchange;            /* host time inside them (stream drain + callback); part of ms_core / ms_peel */
    int64_t exchange_words;         /* 32-bit words they carried                                                 */
    /* graph build (ABI version 5): host wall-clock parts of ms_build (which is now wall-clock too: upload + device work) */
    double  ms_build_h2d;           /* staged host -> device copy of the raw pairs / the CSR                      */
    double  ms_build_relabel;       /* 0 since ABI version 7: the k-truss side is no longer made with the graph (ms_prepare) */
    /* k-truss preparation (ABI version 7): (degree,id) renumbering, oriented CSR, canonical edge map, the enumeration's lines
     * and tasks -- made by the first komb_truss_* call of a graph (or komb_truss_prepare), inside that call */
    double  ms_prepare;             /* device time of the preparation the last k-truss call (or komb_truss_prepare) made; 0 when it found one */
    int32_t truss_prepared;         /* 1 when the last k-truss call made a preparation (whole graph or induced subgraph)      */
    int32_t engine_flags;           /* which engines the last k-core / k-truss call ran: KOMB_ENGINE_* below                  */
    double  ms_prep_vertex;         /* parts of ms_prepare: vertices ordered by (degree, id) (k_prep_vertex, radix sort, scans)   */
    double  ms_prep_edges;          /* every canonical edge handed to its oriented row (k_prep_kept, _heavy, k_prep_dplus, scan)  */
    double  ms_prep_rows;           /* rows sorted, lines and canonical map written (k_prep_rows, _heavy); the rest: task table  */
    int32_t stream_retries;         /* record-stream build: 1 when the first attempt's capacities (two triangles per edge) ran out and the enumeration ran again with what it asked for */
    int32_t reserved0;
} komb_stats;
#define KOMB_ENGINE_LOCAL_FINISH 1   /* a remainder went to the local fixed point (local_dev.h)            */
#define KOMB_ENGINE_LDS_TAIL     2   /* ... to the single-workgroup LDS tail                                */
#define KOMB_ENGINE_SHARD_PEEL   4   /* the peel ran sharded by unit range (shard_dev.h)                    */
#define KOMB_ENGINE_TWO_PASS     8   /* the incidence index was built by the exact two-pass fallback        */

/* ---- lifetime ---------------------------------------------------------- */
komb_ctx   *komb_create(const komb_opts *opts);      /* NULL only on host OOM      */
void        komb_destroy(komb_ctx *ctx);
const char *komb_last_error(const komb_ctx *ctx);    /* "" when no error           */
int         komb_abi_version(void);
/* Tuning / test switches of one context (ABI version 7; until then KOMB_* environment variables, which the library no
 * longer reads: ambient environment cannot change which engine a drop-in runs).  None changes a result.  name: FINISH
 * (local | lds | none), LOCAL_LIMIT, LOCAL_ITEMS, LOCAL_DENSITY, LOCAL_DEFER_CHUNKS, TAIL, CORE_TAIL, INDEX (stream |
 * two_pass), REC_CAP, OWN_DENSE_CAP, NO_OWN_DENSE, NO_REC_SCRATCH, NO_FIRST_QUEUE, RETIRE_EVERY, SHARD_ENGINE, and the
 * NUC_SHORT, NUC_HEAVY, NUC_CAP (komb_nucleus_run, below), MAXCLQ_SEED, MAXCLQ_LDS, MAXCLQ_LIST, MAXCLQ_DEBUG
 * (komb_max_clique_run, below), CENSUS_LDS, CENSUS_PIVOT, CENSUS_DEBUG (komb_clique_census_run, below), MAXIMAL_LDS,
 * MAXIMAL_PIVOT, MAXIMAL_LIST, MAXIMAL_DEBUG (komb_maximal_cliques_run, below), PERC_GROUP, PERC_DEBUG
 * (komb_clique_communities_run, below), BICONN_HEAVY (komb_biconnected_run, below), GRAPHLET_SHORT, GRAPHLET_LDS, GRAPHLET_DEBUG (komb_graphlets_run, below), BTW_GRID, BTW_DEBUG (komb_betweenness_run, below), DIST_WORDS, DIST_GRID, DIST_DEBUG (komb_distances_run, below), and the
 * stderr traces TRI_DEBUG, POOL_DEBUG, BUILD_DEBUG, LOCAL_DEBUG, TAIL_DEBUG, STRUCT_DEBUG, NUC_DEBUG, COMP_SAMPLE (0 | 1:
 * komb_components_run's core kind in one pass over the rows, or skipping the giant component's), DENSEST_LOCAL (0 | 1:
 * komb_densest_subgraph_run's rounds never / whenever they fit in the single-workgroup LDS kernel), and POISON ("0xWWWWWWWW": every device
 * allocation the context hands out is filled with that 32-bit word first -- tests of reads of memory nothing wrote)
 * (DESIGN.md section 8).  value NULL unsets.
 * Two more are tests' means of reaching what a call does when a device allocation fails.  Every device allocation request
 * of the context is counted.  ALLOC_FAIL_AT ("<n>", decimal): zeroes the counter; request number n from now (1-based) fails
 * with out-of-memory -- before anything is allocated, given back or touched on the device -- once, and the trigger is
 * gone; "0" only counts; NULL disarms.  ALLOC_TRIM_AT ("<n>"): zeroes the same counter; request number n, if it is one of
 * the caching pool's, first gives every cached block back to the driver, as a request the driver refuses does before it
 * tries again, and is then served normally.  A value that is not a non-negative decimal number: KOMB_ERR_ARG, nothing
 * changed.  Neither changes a result; with neither set a request pays one branch.
 * komb_alloc_info (no device needed; any output may be NULL): requests counted since either option was last set; whether
 * the ALLOC_FAIL_AT trigger has fired since it was last set (0 | 1); blocks and bytes of the pool that are handed out;
 * blocks the pool holds that nobody uses; how often the pool gave its cached blocks back (a refused request or
 * ALLOC_TRIM_AT).
 * What EVERY entry point below keeps to when a device allocation fails (KOMB_ERR_NOMEM, komb_last_error names the request):
 * no host output has been written; the pool has nothing handed out that no entry point can reach; the results of the
 * other analyses on the context read as before; the same call repeated succeeds.  Whether the entry's own previous result
 * survives is stated with the entry. */
int         komb_set_option(komb_ctx *ctx, const char *name, const char *value);
int         komb_alloc_info(komb_ctx *ctx, int64_t *requests, int32_t *fired, int64_t *pool_blocks_in_use, int64_t *pool_bytes_in_use,
                            int64_t *pool_blocks_cached, int64_t *trims);

/* ---- graph construction ------------------------------------------------ */
/* Replaces igraph_create + igraph_simplify(multiple=true, loops=true)
 * (src/graph.cpp:418, src/graph.cpp:438): n_raw (u,v) pairs exactly as
 * generateGraph leaves them in `edges` (src/graph.cpp:379-389), vertex ids in
 * [0,nv).  Removes loops and parallel edges on the device and keeps the graph
 * resident in HBM as a symmetric CSR (rows ascending, the caller's ids).  What
 * only the k-truss path needs is made by the first k-truss call (below).
 * Every result is reported in the caller's vertex ids.
 * A load drops the previous graph and every result on the context before it does anything else, so a load that fails -- an argument, a
 * limit, KOMB_ERR_NOMEM -- leaves NO graph (komb_graph_from_csr alike).  Until a load succeeds, komb_graph_info / _get_csr / _moments,
 * komb_densest_block, komb_core_run / _fetch and the komb_truss_* calls answer KOMB_ERR_STATE (komb_truss_unprepare: KOMB_OK), every analysis KOMB_ERR_ARG. */
int komb_graph_from_edges(komb_ctx *ctx, int64_t nv, int64_t n_raw,
                          const int64_t *uv_pairs);

/* Same, from an already simple, symmetric, row-sorted CSR (host pointers). */
int komb_graph_from_csr(komb_ctx *ctx, int64_t nv, const int64_t *rowptr,
                        const int32_t *col);

/* igraph_vcount / igraph_ecount (src/graph.cpp:443-444). */
int komb_graph_info(komb_ctx *ctx, int64_t *nv, int64_t *ne);

/* Copy the resident CSR back: rowptr[nv+1], col[2*ne]. */
int komb_graph_get_csr(komb_ctx *ctx, int64_t *rowptr, int32_t *col);

/* ---- k-core ------------------------------------------------------------ */
/* Replaces igraph_degree(ALL,NO_LOOPS) + igraph_coreness(ALL)
 * (src/graph.cpp:462-463).  komb_core_run computes on the device and leaves
 * degree/coreness in HBM (this is the timed region of bench.py);
 * komb_core_fetch copies them out; komb_degree_coreness = run + fetch.
 * A run writes into the result's own arrays from its first kernel on: a run that fails (KOMB_ERR_NOMEM, KOMB_ERR_DEVICE)
 * drops the previous k-core result -- komb_core_fetch, and what needs the coreness, answer KOMB_ERR_STATE until a run
 * completes -- and changes nothing else on the context. */
int komb_core_run(komb_ctx *ctx);
/* One process per GPU, every rank holding the same graph: rank r owns the vertices
 * [nv*r/world, nv*(r+1)/world) -- their live degrees and the decrements on them; every sub-round the ranks exchange
 * their parts of the frontier through `allreduce` (komb_allreduce_fn below: each rank fills its own segment of a zeroed
 * buffer, so the SUM is the concatenation), stamp the whole frontier and walk all of its rows, each applying the
 * decrements it owns.  All ranks end with identical, complete results, bit-equal to komb_core_run's.  world == 1 is
 * the same engine without a collective. */
typedef int (*komb_allreduce_fn)(void *user, void *device_u32, int64_t count);
int komb_core_run_sharded(komb_ctx *ctx, int32_t rank, int32_t world, komb_allreduce_fn allreduce, void *user);
int komb_core_fetch(komb_ctx *ctx, int32_t *degree /*[nv]*/, int32_t *coreness /*[nv]*/);
int komb_degree_coreness(komb_ctx *ctx, int32_t *degree, int32_t *coreness);

/* ---- onion decomposition ---------------------------------------------- */
/* The onion decomposition of the resident simple graph (L. Hebert-Dufresne, J. A. Grochow, A. Allard, "Multi-scale
 * structure and topological anomaly detection via a new network statistic: the onion decomposition", Scientific
 * Reports 6, 31708 (2016)): per vertex, the synchronous layer inside its k-shell in which it is peeled -- exactly what
 * networkx.onion_layers returns.  Layers are numbered from 1.  Isolated vertices (degree 0) all form layer 1 when there
 * are any, and the other layers then start at 2.  Then, with k = 1 at first, until the graph is empty: if the smallest
 * live degree is greater than k, k becomes it; the next layer is EVERY live vertex of live degree <= k; all of them are
 * removed at once and their neighbours' live degrees decremented.  The k at which a vertex leaves is its coreness (0 if
 * isolated), equal to komb_core_run's.
 * komb_onion_run computes on the device and keeps the results in HBM; komb_onion_fetch copies layer[nv] and
 * coreness[nv] out (either may be NULL); komb_onion_info reports the last run: the number of layers (the largest layer
 * number, 0 for an empty graph), the largest coreness and the run's device time in ms.  The onion uses arrays of its
 * own: it changes no k-core, k-truss or CoreA result and no komb_stats field.  No graph loaded: KOMB_ERR_ARG; fetch /
 * info before a run on the current graph: KOMB_ERR_STATE.  A run that fails (KOMB_ERR_NOMEM, KOMB_ERR_DEVICE) drops the
 * previous onion result: fetch / info answer KOMB_ERR_STATE until a run completes. */
int komb_onion_run(komb_ctx *ctx);
int komb_onion_fetch(komb_ctx *ctx, int32_t *layer /*[nv]*/, int32_t *coreness /*[nv]*/);
int komb_onion_info(komb_ctx *ctx, int64_t *n_layers, int32_t *max_coreness, double *ms);

/* ---- connected components of a k-core / k-truss subgraph ---------------- */
/* Which vertices belong together: the connected components of the subgraph a threshold k selects.
 * label[v] is the SMALLEST original vertex id of v's component, -1 for a vertex that is not a member; size[v] is the
 * number of vertices of v's component, 0 for a non-member.  Both are fully determined by the graph: they do not depend
 * on the run, on an option or on scheduling.
 * KOMB_COMP_CORE: k == 0 is the whole resident graph -- every vertex a member, an isolated vertex a component of size
 * 1 -- and needs nothing but a graph; k >= 1 or KOMB_COMP_K_MAX reads the coreness komb_core_run left on this graph
 * (KOMB_ERR_STATE if there is none; k-core is never run here).
 * KOMB_COMP_TRUSS works on whatever the last k-truss call left, whole graph or vmask run alike (the endpoints are
 * original ids either way); k <= 2 means every edge of that result.  Without a completed k-truss result on this graph,
 * or after komb_truss_run_slice / a sharded run that materialised only part of the canonical edges: KOMB_ERR_STATE.
 * Canonical endpoints of a whole-graph result that no fetch has asked for yet are made here as that fetch makes them.
 * A result with no edges has no members, and k_used is 2 under KOMB_COMP_K_MAX.
 * k above the maximum: no members, n_components == 0, largest == 0; not an error.  k < -1 or an unknown kind:
 * KOMB_ERR_ARG.  No graph loaded: KOMB_ERR_ARG.  fetch / info before a run on the current graph: KOMB_ERR_STATE.
 * komb_components_info: the kind, the threshold actually applied (KOMB_COMP_K_MAX resolved), members, components, the
 * size of the largest component and the device time of the run in ms (the context's HIP-event timer).
 * The result is a snapshot in arrays of its own: loading a graph drops it; later k-core / k-truss calls neither change
 * nor invalidate it; a call changes no k-core, k-truss, onion or CoreA result and no komb_stats field.  A run that fails
 * (KOMB_ERR_NOMEM, KOMB_ERR_DEVICE) drops the previous snapshot: fetch / info answer KOMB_ERR_STATE until a run completes.  Option
 * COMP_SAMPLE (0 | 1) selects between the one-pass and the giant-component-skipping link of the core kind. */
#define KOMB_COMP_CORE   0    /* members: vertices with coreness >= k; edges: resident edges between two members     */
#define KOMB_COMP_TRUSS  1    /* edges: those of the last k-truss result with trussness >= k; members: their endpoints */
#define KOMB_COMP_K_MAX (-1)  /* k = the largest coreness / the largest trussness of that result                        */
int komb_components_run(komb_ctx *ctx, int32_t kind, int32_t k);
int komb_components_fetch(komb_ctx *ctx, int32_t *label /*[nv]*/, int32_t *size /*[nv]*/);   /* either may be NULL */
int komb_components_info(komb_ctx *ctx, int32_t *kind, int32_t *k_used, int64_t *n_members,
                         int64_t *n_components, int64_t *largest, double *ms);               /* any may be NULL    */

/* ---- component hierarchy: the nesting forest of the k-core / k-truss components ---- */
/* All thresholds at once: which component of G_k lies inside which component of G_(k-1).
 * KOMB_COMP_CORE: G_k is the subgraph induced by the vertices of coreness >= k, k >= 0 (G_0: the whole graph, isolated
 * vertices included); lvl(v) = coreness(v).  KOMB_COMP_TRUSS: G_k is the edges of trussness >= k of the last complete
 * k-truss result, whole graph or vmask run alike, with their endpoints, k >= 2; lvl(v) = the largest trussness of an edge
 * at v, and a vertex without an edge in that result is no member.
 * A NODE is a pair (k, S): S is the vertex set of a connected component of G_k and not the vertex set of a component of
 * G_(k+1) -- S holds a vertex of level exactly k, or (truss kind only) joins two or more components of G_(k+1) by edges
 * of trussness k.  rep = the smallest original vertex id in S.  Nodes are numbered 0 .. n_nodes-1 in ascending (k, rep)
 * order.  parent = the node (k', S') with S inside S' and the largest k' < k, -1 when there is none (S is then a whole
 * component of G_0 / G_2); parent[i] < i always.  size[i] = |S|; shell[i] = the vertices v with node[v] == i; size[i] ==
 * shell[i] + the sizes of i's children.  node[v] = the node (lvl(v), the component of G_lvl(v) that holds v), -1 for a
 * non-member.  Everything is determined by the graph: it does not depend on the run, on an option or on scheduling.
 * It follows that for a member v of G_k, walking up from node[v] while the parent's k is still >= k ends at the node
 * whose rep is label[v] of komb_components_run(kind, k).
 * komb_hierarchy_info: the kind, nodes, nodes without a parent, the largest node level (without nodes: 0 / 2), depth =
 * the most nodes on a path from a root down (0 without nodes) and the device time of the run in ms.
 * No graph loaded or an unknown kind: KOMB_ERR_ARG.  Core kind without a komb_core_run result on this graph (k-core is
 * never run here), truss kind without a complete k-truss result (none yet, after komb_truss_run_slice, a sharded partial
 * result or komb_truss_unprepare), count / fetch / info before a run on the current graph: KOMB_ERR_STATE.  A failed
 * call leaves the previous result readable.  The empty graph has no nodes; not an error.
 * The result is a snapshot in arrays of its own: loading a graph drops it; later k-core, k-truss, onion, components and
 * communities calls neither change nor drop it; a run changes none of their results and no komb_stats field. */
int komb_hierarchy_run(komb_ctx *ctx, int32_t kind);                 /* KOMB_COMP_CORE | KOMB_COMP_TRUSS */
int komb_hierarchy_count(komb_ctx *ctx, int64_t *n_nodes);
int komb_hierarchy_fetch_nodes(komb_ctx *ctx, int32_t *k, int32_t *rep, int32_t *parent,
                               int32_t *size, int32_t *shell);       /* [n_nodes] each, any may be NULL */
int komb_hierarchy_fetch_vertices(komb_ctx *ctx, int32_t *node /*[nv]*/);
int komb_hierarchy_info(komb_ctx *ctx, int32_t *kind, int64_t *n_nodes, int64_t *n_roots,
                        int32_t *k_max, int32_t *depth, double *ms); /* any may be NULL */

/* ---- k-truss communities (triangle-connected edge classes) --------------- */
/* Which EDGES of the k-truss belong together: the k-truss communities of Huang, Cheng, Qin, Tian, Yu ("Querying k-truss
 * community in large and dynamic graphs", SIGMOD 2014).  Input: the last completed k-truss result, whole graph or vmask
 * run alike -- ne_sub canonical edges (eu[i], ev[i]) with trussness truss[i] -- and a threshold k.
 * Member edges: truss[i] >= k; 0 <= k <= 2 is run as 2 (every edge of the result) and k_used reports 2.  Two members are
 * adjacent when they are two sides of a triangle whose three edges are all members; the communities are the classes of
 * the transitive closure.  label[i] is the SMALLEST canonical edge index of i's community, -1 for a non-member;
 * size[i] is the number of edges of that community, 0 for a non-member.  For k >= 3 no community has size 1; for
 * k <= 2 an edge in no triangle is a community of size 1.  n_comm[v], per original vertex, is the number of distinct
 * communities among the member edges at v (0 without one): a vertex may belong to several.  All three are fully
 * determined by the graph: they do not depend on the run, on an option or on scheduling.
 * k < -1: KOMB_ERR_ARG.  No graph loaded: KOMB_ERR_ARG.  Without a completed k-truss result on this graph, or after
 * komb_truss_run_slice / a sharded run that materialised only part of the canonical edges: KOMB_ERR_STATE.  k above
 * the largest trussness: no members, every count 0, not an error.  A result with no edges has no members, and k_used is
 * 2 under KOMB_COMM_K_MAX.  Canonical endpoints of a whole-graph result that no fetch has asked for yet are made here
 * as that fetch makes them.
 * komb_truss_communities_info: the threshold applied, the member edges, the communities, the edges of the largest one,
 * the vertices with n_comm > 1, and ms -- the device time of komb_truss_communities_run (labels and sizes) on the
 * context's HIP-event timer.  n_comm and n_multi_vertices are made by the first fetch_vertices / info call that asks
 * for them after a run (a sort of the distinct (vertex, label) pairs), outside ms.
 * The result lives in arrays of its own, and its labels index the canonical edge list of the k-truss result it was
 * computed from: whatever replaces or drops that result -- a new k-truss run of any kind, komb_truss_unprepare, a graph
 * load -- drops the communities too, and fetch / info then return KOMB_ERR_STATE until the next run.  k-core, onion,
 * components and CoreA calls neither change nor drop it.  A communities run drops the previous communities when it
 * starts: one that fails (KOMB_ERR_NOMEM, KOMB_ERR_DEVICE) leaves none.  A communities run changes no k-core, k-truss, onion,
 * components or CoreA result, no komb_stats field and not the resident k-truss preparation.  Options COMM_SHORT /
 * COMM_HEAVY (tests) move the lengths at which an edge's triangle search goes from its lane to its wave / to several
 * workgroups; neither changes a result. */
#define KOMB_COMM_K_MAX (-1)   /* k = the largest trussness of the result (2 when it has no edges) */
int komb_truss_communities_run(komb_ctx *ctx, int32_t k);
int komb_truss_communities_fetch(komb_ctx *ctx, int32_t *label /*[ne_sub]*/, int32_t *size /*[ne_sub]*/);  /* either may be NULL */
int komb_truss_communities_fetch_vertices(komb_ctx *ctx, int32_t *n_comm /*[nv]*/);
int komb_truss_communities_info(komb_ctx *ctx, int32_t *k_used, int64_t *n_member_edges, int64_t *n_communities,
                                int64_t *largest, int64_t *n_multi_vertices, double *ms);                 /* any may be NULL */

/* ---- biconnected components, articulation points, bridges ------------------ */
/* Which single vertices and which single edges hold the k-truss together: the blocks of Tarjan & Vishkin ("An efficient
 * parallel biconnectivity algorithm", SIAM J. Comput. 1985), on a breadth-first spanning forest.  Input: the last
 * completed k-truss result, whole graph or vmask run alike -- ne_sub canonical edges (eu[i], ev[i]) with trussness
 * truss[i] -- and a threshold k.  Member edges: truss[i] >= k; 0 <= k <= 2 is run as 2 (every edge of the result) and
 * k_used reports 2; member vertices: the endpoints of member edges.
 * A BLOCK (biconnected component) is a maximal set of member edges any two of which lie on a common simple cycle; an edge
 * on no cycle is a block of its own, a BRIDGE.  block[i] is the SMALLEST canonical edge index of i's block, -1 for a
 * non-member; size[i] is the number of edges of that block, 0 for a non-member; a member edge is a bridge exactly when
 * size[i] == 1.  n_blocks[v], per original vertex, is the number of blocks that contain v (0 for a non-member): v is an
 * ARTICULATION POINT -- its removal separates its component -- exactly when n_blocks[v] >= 2.  ecc_label[v] is the smallest
 * vertex id of v's 2-edge-connected component (the connected component of v once all bridges are removed), -1 for a
 * non-member; ecc_size[v] is that component's number of vertices, 0 for a non-member.  The block list, in ascending rep
 * order: rep (= block[] of its edges), n_edges, n_verts; komb_biconnected_count gives its length.  Everything is fully
 * determined by the graph: it does not depend on the run, on the spanning forest, on an option or on scheduling.
 * komb_biconnected_info: the threshold applied, the member edges and vertices, the blocks, the bridges, the articulation
 * points, the edges of the largest block, the 2-edge-connected components and the vertices of the largest one, depth --
 * the number of levels of the spanning forest (0 without members) -- and ms, the device time of komb_biconnected_run on
 * the context's HIP-event timer.  A run is four launches and one small read per level of the forest plus a constant
 * number: its cost grows with depth.  Assembly-derived power-law graphs have depths in the tens; a long path has its
 * length, and depth is reported so that a caller can see it.
 * k < -1: KOMB_ERR_ARG.  No graph loaded: KOMB_ERR_ARG.  Without a completed k-truss result on this graph, or after
 * komb_truss_run_slice / a sharded run that materialised only part of the canonical edges: KOMB_ERR_STATE; count / fetch /
 * info before a run on the current result: KOMB_ERR_STATE.  A failing call writes nothing to its outputs.  k above the
 * largest trussness: no members, every count 0, not an error.  A result with no edges has no members, and k_used is 2
 * under KOMB_BICONN_K_MAX.  Canonical endpoints of a whole-graph result that no fetch has asked for yet are made here as
 * that fetch makes them.  More than 2^31 - 1 member edges do not fit the 32-bit row offsets: KOMB_ERR_LIMIT.
 * The result lives in arrays of its own, and its reps index the canonical edge list of the k-truss result it was computed
 * from: whatever replaces or drops that result -- a new k-truss run of any kind, komb_truss_unprepare, a graph load --
 * drops it too.  k-core, onion, components, communities and CoreA calls neither change nor drop it; a run changes none
 * of their results, no komb_stats field and not the resident k-truss preparation.  A run drops the previous blocks when it
 * starts: one that fails (KOMB_ERR_NOMEM, KOMB_ERR_LIMIT, KOMB_ERR_DEVICE) leaves none.  Option BICONN_HEAVY (tests) moves the
 * row length above which a frontier vertex' row is walked by its wave; it changes no result. */
#define KOMB_BICONN_K_MAX (-1)   /* k = the largest trussness of the result (2 when it has no edges) */
int komb_biconnected_run(komb_ctx *ctx, int32_t k);
int komb_biconnected_count(komb_ctx *ctx, int64_t *n_blocks);
int komb_biconnected_fetch_edges(komb_ctx *ctx, int32_t *block /*[ne_sub]*/, int32_t *size /*[ne_sub]*/);       /* either may be NULL */
int komb_biconnected_fetch_vertices(komb_ctx *ctx, int32_t *n_blocks, int32_t *ecc_label, int32_t *ecc_size);     /* [nv] each, any may be NULL */
int komb_biconnected_fetch_blocks(komb_ctx *ctx, int32_t *rep, int32_t *n_edges, int32_t *n_verts);               /* [n_blocks] each, any may be NULL */
int komb_biconnected_info(komb_ctx *ctx, int32_t *k_used, int64_t *n_member_edges, int64_t *n_member_vertices,
                          int64_t *n_blocks, int64_t *n_bridges, int64_t *n_articulation, int64_t *largest_block,
                          int64_t *n_ecc, int64_t *largest_ecc, int32_t *depth, double *ms);                     /* any may be NULL */

/* ---- k-truss community hierarchy: the nesting forest of the communities over all k ---- */
/* All thresholds at once: which k-truss community lies inside which community of a smaller k (the index of Huang et al.
 * 2014 / the EquiTruss summary of Akbas & Zhao, VLDB 2017, as a forest).  Input: the last COMPLETE k-truss result, whole
 * graph or vmask run alike -- ne_sub canonical edges (eu[i], ev[i]) with trussness t[i].
 * An edge is a MEMBER when t[i] >= 3.  An edge has trussness 2 exactly when it lies in no triangle of the result: it is in
 * no community of any k >= 3 and is no member here, node[i] = -1.
 * For k >= 3, C_k is the set of k-truss communities of komb_truss_communities_run(k): the classes of the edges with
 * t >= k under "two sides of a triangle whose three edges all have t >= k".
 * A NODE is a pair (k, S): S is the edge set of a community of C_k and not the edge set of a community of C_(k+1) -- S
 * holds an edge of trussness exactly k, or joins two or more communities of C_(k+1) through triangles whose smallest
 * trussness is k.  rep = the smallest canonical edge index in S.  Nodes are numbered 0 .. n_nodes-1 in ascending (k, rep)
 * order.  parent = the node (k', S') with S inside S' and the largest k' < k, -1 when there is none; parent[i] < i always.
 * size[i] = |S|, counted in edges; shell[i] = the edges e with node[e] == i; size[i] == shell[i] + the sizes of i's
 * children.  node[e] = the node (t[e], the community of C_t[e] that holds e), -1 for a non-member.  Everything is
 * determined by the graph: it does not depend on the run, on an option or on scheduling.
 * The walk-up rule: for an edge e with t[e] >= k >= 3, walking up from node[e] while the parent's k is still >= k ends at
 * the node whose rep is label[e] and whose size is size[e] of komb_truss_communities_run(k).
 * komb_community_hierarchy_labels runs that rule on the device, one walk per edge over the stored forest and no triangle
 * work, and returns exactly what komb_truss_communities_run(k) followed by komb_truss_communities_fetch returns, for
 * every k: KOMB_COMM_K_MAX resolves as it does there; 0 <= k <= 2 runs as 2 -- an edge of trussness 2 is then its own
 * community (label = its own index, size 1), the members take their root's rep and size; k above the largest trussness
 * gives -1 / 0 everywhere; k < -1: KOMB_ERR_ARG.  Either output may be NULL.  The call does not touch the stored result
 * of komb_truss_communities_run.
 * komb_community_hierarchy_info: nodes, nodes without a parent, the largest node level (2 without nodes), depth = the
 * most nodes on a path from a root down (0 without nodes), the member edges, and ms -- the device time of
 * komb_community_hierarchy_run on the context's HIP-event timer.
 * No graph loaded: KOMB_ERR_ARG.  Without a complete k-truss result (none yet, after komb_truss_run_slice, a sharded
 * partial result or komb_truss_unprepare), count / fetch / labels / info before a run on the current result:
 * KOMB_ERR_STATE.  A result with no edge of trussness >= 3 has no nodes; not an error.  A failed call leaves the previous
 * result readable.  The run writes two link records per triangle of the result; more than 2^31 - 1 of them do not fit its
 * 32-bit indexing: KOMB_ERR_LIMIT.
 * The arrays index the canonical edges of one k-truss result and are blocks of their own: whatever replaces or drops that
 * result -- a new k-truss run of any kind, komb_truss_unprepare, a graph load -- drops them too.  k-core, onion,
 * components, hierarchy, communities and CoreA calls neither change nor drop them; a run changes none of their results,
 * no komb_stats field and not the resident k-truss preparation.  Options COMM_SHORT / COMM_HEAVY move the length classes
 * of the triangle search here as they do for komb_truss_communities_run; neither changes a result. */
int komb_community_hierarchy_run(komb_ctx *ctx);
int komb_community_hierarchy_count(komb_ctx *ctx, int64_t *n_nodes);
int komb_community_hierarchy_fetch_nodes(komb_ctx *ctx, int32_t *k, int32_t *rep, int32_t *parent,
                                         int32_t *size, int32_t *shell);       /* [n_nodes] each, any may be NULL */
int komb_community_hierarchy_fetch_edges(komb_ctx *ctx, int32_t *node /*[ne_sub]*/);
int komb_community_hierarchy_labels(komb_ctx *ctx, int32_t k, int32_t *label /*[ne_sub]*/, int32_t *size /*[ne_sub]*/);
int komb_community_hierarchy_info(komb_ctx *ctx, int64_t *n_nodes, int64_t *n_roots, int32_t *k_max, int32_t *depth,
                                  int64_t *n_member_edges, double *ms);        /* any may be NULL */

/* ---- densest-subgraph search with a certified bound ---------------------- */
/* Which vertex set of the resident graph is the densest, and how dense can any be.  The density of a vertex set S is
 * rho(S) = m(S) / |S|, m(S) = the resident edges with both ends in S.  Every comparison of two densities is exact: a
 * cross-multiplication in 64-bit integers, never floating point.  komb_densest_subgraph_run(ctx, iters), iters >= 0, reads
 * the coreness komb_core_run left on this graph (KOMB_ERR_STATE if there is none; k-core is never run here):
 *  1. Core density profile.  For k = 0 .. k_max: n_k = the vertices of coreness >= k, m_k = the edges whose two ends both
 *     have coreness >= k.  The best core is the k that maximises m_k / n_k, the LARGER k on a tie: (k*, m*, n*).
 *  2. Prune.  c = ceil(m* / n*), P = the vertices of coreness >= c, E_P = the edges inside P.  Every densest subgraph lies
 *     inside P (each of its vertices has at least rho_opt >= m* / n* neighbours in it), so P has the same optimum.
 *  3. iters synchronous Frank-Wolfe rounds on integer loads (Danisch, Chan, Sozio, "Large scale density-friendly graph
 *     decomposition via convex programming", WWW 2017; with step 1 / (t + 1) the iterate is the average of the rounds, so
 *     the cumulative counts are the whole state).  L_0 = 0.  In round t = 0 .. iters - 1 every edge {u, v} of E_P, u < v,
 *     reads L_t and gives one unit to the endpoint with the smaller load; on equal loads to u when t is even, to v when t
 *     is odd.  L_(t+1) = L_t + those units.  Every read of round t sees L_t only: the result does not depend on scheduling.
 *  4. Extract.  P ordered by (load descending, id ascending); for every prefix length i >= 1, m_i = the edges of E_P with
 *     both ends among the first i vertices.  The best prefix maximises m_i / i, the SHORTEST on a tie.
 *  5. The result is the best prefix when iters >= 1 and it is strictly denser than the best core (source == 1,
 *     KOMB_DENSEST_PREFIX), else the best core (source == 0, KOMB_DENSEST_CORE).
 *  6. Certificate.  For iters >= 1, rho_opt <= load_max / iters with load_max = the largest load: the averaged assignment is
 *     a feasible point of the dual of Charikar's LP, and the loads inside an optimal set sum to at least its edge count.
 *     rho_opt <= k_max always.  info reports m_sub, n_sub, load_max, iters and k_max as integers; the caller forms the ratios.
 * The empty graph: no members, every count 0.  A graph without edges: the 0-core, every vertex, m_sub == 0.  iters < 0, or
 * no graph loaded: KOMB_ERR_ARG.  iters * (the largest degree inside P) above 2^31 - 1 does not fit the load word:
 * KOMB_ERR_LIMIT, before a round is queued.  fetch / profile / info before a run on the current graph: KOMB_ERR_STATE.
 * komb_densest_subgraph_fetch: member[v] = 1 | 0, load[v] = the load of v after the last round, 0 outside P; either may be
 * NULL.  komb_densest_subgraph_profile: n_k, m_k, k_max + 1 entries each (k_max from info); either may be NULL.
 * komb_densest_subgraph_info: source, k* , c, |P|, |E_P|, the result's vertices and edges, load_max, iters, k_max and the
 * device time of the run in ms (the context's HIP-event timer); any pointer may be NULL.
 * The result is a snapshot in arrays of its own: loading a graph drops it, no other call changes it, a run changes no other
 * result and no komb_stats field, and a failed run leaves the previous result readable.  Option DENSEST_LOCAL (0 = never,
 * 1 = whenever loads and deltas fit in LDS, unset = automatic) selects between one launch per round and one workgroup that
 * runs all rounds in a single launch; it changes no result. */
#define KOMB_DENSEST_CORE   0
#define KOMB_DENSEST_PREFIX 1
int komb_densest_subgraph_run(komb_ctx *ctx, int32_t iters);
int komb_densest_subgraph_fetch(komb_ctx *ctx, int32_t *member /*[nv] 0|1*/, int32_t *load /*[nv], 0 outside P*/);
int komb_densest_subgraph_profile(komb_ctx *ctx, int64_t *n_k, int64_t *m_k /*[k_max+1] each*/);
int komb_densest_subgraph_info(komb_ctx *ctx, int32_t *source, int32_t *k_best, int32_t *k_prune, int64_t *n_pruned,
                               int64_t *m_pruned, int64_t *n_sub, int64_t *m_sub, int64_t *load_max, int32_t *iters,
                               int32_t *k_max, double *ms);

/* ---- structural clustering: clusters, hubs and outliers ------------------ */
/* Which vertices tie several dense regions together, and which belong to none: structural clustering after Xu, Yuret, Feng,
 * Schweiger ("SCAN: a structural clustering algorithm for networks", KDD 2007), computed without an index as in pSCAN (Chang
 * et al., ICDE 2016).  Input: the last COMPLETE k-truss result on the resident graph, whole graph or vmask run alike -- ne_sub
 * canonical edges (eu[i], ev[i]), eu < ev, in (min, max) lexicographic order of original ids, and their initial supports
 * sup[i], the triangles of the result through edge i (komb_truss_fetch_support).  Parameters: eps = eps_num / eps_den with
 * 1 <= eps_num <= eps_den <= 1 000 000, and mu >= 2.
 * d(v) is the number of result edges at v (a whole-graph result: the CSR row length; 0 for a vertex outside the vmask and
 * for an isolated vertex).  With Gamma(v) = N(v) + {v}, sigma(u, v) = |Gamma(u) & Gamma(v)| / sqrt(|Gamma(u)| |Gamma(v)|),
 * which on an edge is (sup + 2) / sqrt((d(u) + 1) (d(v) + 1)).  Edge i is SIMILAR iff
 *     (sup + 2)^2 * eps_den^2 >= eps_num^2 * (d(u) + 1) * (d(v) + 1),
 * evaluated exactly in 128-bit integers (the left side reaches 2^102): there is no floating point anywhere.
 * sim_deg[v] is the number of similar edges at v.
 * v is a CORE iff sim_deg[v] + 1 >= mu (a vertex is similar to itself, as in the paper).  The CLUSTERS are the classes of the
 * cores under "joined by a similar edge whose two ends are both cores"; label of a core = the smallest vertex id of its class.
 * A non-core with at least one similar edge to a core is a BORDER; its label is the smallest label among those cores (a
 * border may touch several clusters and is counted in exactly one: the one place the paper leaves open, fixed here so that
 * the output is a function of the graph).  Every other vertex has label -1: it is a HUB iff two of its neighbours in the
 * result -- over any edge, not only similar ones -- carry different labels >= 0, else an OUTLIER.
 * size[v] = the vertices that carry v's label, 0 for label -1.  role[v] = KOMB_SC_*.
 * Everything is determined by the graph and the three parameters: nothing depends on the run, on scheduling or on an option.
 * komb_structural_clusters_fetch: label, size, role, sim_deg, [nv] each; komb_structural_clusters_fetch_edges: similar[i] =
 * 1 | 0 in canonical order; komb_structural_clusters_info: the parameters of the last run, the similar edges, the vertices
 * of each role, the clusters, the size of the largest one (borders included) and ms -- the device time of the run on the
 * context's HIP-event timer.  Any output pointer may be NULL.
 * No context or no graph loaded: KOMB_ERR_ARG.  A parameter outside the ranges above: KOMB_ERR_ARG.  Without a completed
 * k-truss result on this graph, after komb_truss_run_slice / a sharded run that materialised only part of the canonical
 * edges, after komb_truss_unprepare, fetch / info before a run: KOMB_ERR_STATE.  A result without edges makes every vertex
 * an outlier and every count 0; the empty graph is not an error.  Canonical endpoints and supports of a whole-graph result
 * that no fetch has asked for yet are made here as those fetches make them.
 * The result lives in arrays of its own, installed when a run has succeeded: a refused or failed run leaves the previous
 * result readable.  It indexes one k-truss result: whatever replaces or drops that result -- a new k-truss run of any kind,
 * komb_truss_unprepare, a graph load -- drops it too.  k-core, onion, components, hierarchy, communities, densest and CoreA
 * calls neither change nor drop it; a run changes none of their results, no komb_stats field and not the resident k-truss
 * preparation.  Option STRUCT_DEBUG (stderr trace: the device time of the run and of its similarity pass) changes no result. */
#define KOMB_SC_OUTLIER 0
#define KOMB_SC_HUB     1
#define KOMB_SC_BORDER  2
#define KOMB_SC_CORE    3
int komb_structural_clusters_run(komb_ctx *ctx, int32_t eps_num, int32_t eps_den, int32_t mu);
int komb_structural_clusters_fetch(komb_ctx *ctx, int32_t *label, int32_t *size, int32_t *role, int32_t *sim_deg);   /* [nv] each, any may be NULL */
int komb_structural_clusters_fetch_edges(komb_ctx *ctx, int32_t *similar /*[ne_sub] 0|1, canonical order*/);
int komb_structural_clusters_info(komb_ctx *ctx, int32_t *eps_num, int32_t *eps_den, int32_t *mu, int64_t *n_similar_edges,
                                  int64_t *n_cores, int64_t *n_borders, int64_t *n_hubs, int64_t *n_outliers, int64_t *n_clusters,
                                  int64_t *largest, double *ms);                                                     /* any may be NULL */

/* ---- (3,4)-nucleus decomposition: triangles peeled by 4-cliques ----------- */
/* The third rung of the nucleus ladder of Sariyuce, Seshadhri, Pinar, Catalyurek ("Finding the hierarchy of dense subgraphs
 * using nucleus decompositions", WWW 2015): k-core peels vertices by edges (1,2), k-truss peels edges by triangles (2,3),
 * this peels TRIANGLES by the 4-CLIQUES they lie in (3,4).  A triangle-rich region that is no near-clique has a high
 * trussness and a low nucleus number.
 * Input: the last COMPLETE k-truss result on the resident graph, whole graph or vmask run alike -- its ne_sub canonical edges
 * (eu[i], ev[i]), eu < ev, sorted by (eu, ev), original vertex ids.  Call their graph H.
 * A TRIANGLE is a < b < c with all three edges in H.  Triangles are numbered in ascending (a, b, c) order, which is also the
 * order (canonical index of (a, b), c).  A 4-CLIQUE is a < b < c < d with all six edges in H.  key0[t] is the number of
 * 4-cliques that contain triangle t.
 * theta(t), the NUCLEUS NUMBER, is the largest k such that t belongs to a family S of triangles in which every member lies
 * in at least k 4-cliques whose four triangles are all in S.  No connectivity condition is applied, exactly as coreness has
 * none.  A triangle in no 4-clique has theta = 0; K_n gives theta = n - 3 on every triangle; theta <= key0.  theta is unique:
 * nothing in any output depends on the run, on scheduling or on an option.
 * edge_theta[i] is the largest theta over the triangles through canonical edge i, -1 if there is none; vertex_theta[v] is the
 * same per vertex.
 * komb_nucleus_count: the triangles of the result.  komb_nucleus_fetch: a, b, c, key0, theta, [n_triangles] each.
 * komb_nucleus_fetch_edges: edge_theta[ne_sub], canonical order.  komb_nucleus_fetch_vertices: vertex_theta[nv].
 * komb_nucleus_info: triangles, 4-cliques, the largest theta (-1 without a triangle), n_levels -- the distinct values of
 * theta --, n_subrounds -- the frontiers the level-synchronous peel went through, >= n_levels --, and ms, the device time
 * of the run on the context's HIP-event timer.  Any output pointer may be NULL.
 * No context or no graph loaded: KOMB_ERR_ARG.  Without a completed k-truss result on this graph, after komb_truss_run_slice
 * / a sharded run that materialised only part of the canonical edges, after komb_truss_unprepare, count / fetch / info
 * before a run: KOMB_ERR_STATE.  A result without triangles is not an error: the count is 0, every edge_theta and
 * vertex_theta is -1 and theta_max = -1.  More than 2^31 - 1 triangles or more than 2^30 - 1 4-cliques: KOMB_ERR_LIMIT
 * (clique ids are 32-bit and a clique has four incidences); each count is checked after its count pass and before the
 * storage it sizes is reserved.  A pool failure: KOMB_ERR_NOMEM.
 * The result lives in arrays of its own, installed when a run has succeeded: a refused or failed run leaves the previous
 * result readable.  It indexes one k-truss result: whatever replaces or drops that result -- a new k-truss run of any kind,
 * komb_truss_unprepare, a graph load -- drops it too.  No other call changes or drops it; a run changes no other result, no
 * komb_stats field and not the resident k-truss preparation.  Options (none changes a result): NUC_SHORT / NUC_HEAVY move the
 * lengths at which a walked side goes from its lane to its wave (default 16) / in the triangle pass to several workgroups
 * (default 2048); NUC_CAP=<n> refuses above n 4-cliques with KOMB_ERR_LIMIT (tests of the refusal); NUC_DEBUG prints one
 * stderr line with the counts and the device times of the passes. */
int komb_nucleus_run(komb_ctx *ctx);
int komb_nucleus_count(komb_ctx *ctx, int64_t *n_triangles);
int komb_nucleus_fetch(komb_ctx *ctx, int32_t *a, int32_t *b, int32_t *c, int32_t *key0, int32_t *theta);   /* [n_triangles] each, any may be NULL */
int komb_nucleus_fetch_edges(komb_ctx *ctx, int32_t *edge_theta);      /* [ne_sub], canonical order */
int komb_nucleus_fetch_vertices(komb_ctx *ctx, int32_t *vertex_theta); /* [nv] */
int komb_nucleus_info(komb_ctx *ctx, int64_t *n_triangles, int64_t *n_cliques4, int32_t *theta_max,
                      int32_t *n_levels, int64_t *n_subrounds, double *ms);   /* any may be NULL */

/* ---- (3,4)-nucleus hierarchy: the nuclei as connected classes and their forest ---- */
/* theta has no connectivity condition: two K_5 that share only an edge carry theta = 2 on all twenty triangles.  The k-nuclei
 * of the paper above are CONNECTED, and their nesting over all k is its forest of dense subgraphs.
 * Input: the stored result of the last komb_nucleus_run on the current k-truss result -- the triangles, numbered in ascending
 * (a, b, c) order, with theta per triangle, and the 4-cliques of that result.
 * For k >= 1, T_k is the set of triangles with theta >= k.  A 4-clique has WEIGHT w = the smallest theta of its four
 * triangles; every 4-clique has w >= 1.  Two triangles of T_k are k-LINKED when they lie in a common 4-clique of weight >= k.
 * The k-NUCLEI N_k are the classes of the transitive closure of k-linking on T_k.  A triangle with theta = 0 lies in no clique
 * and is in no nucleus.
 * A NODE is a pair (k, S): S is in N_k and not in N_(k+1).  rep = the smallest triangle id in S.  Nodes are numbered
 * 0 .. n_nodes-1 in ascending (k, rep) order.  parent = the node of the nearest lower level whose set contains S, -1 when
 * there is none; parent[i] < i always.  size[i] = the triangles in S; shell[i] = the triangles in S with theta exactly k;
 * size[i] == shell[i] + the sizes of i's children.  node[t] = the node at level theta(t) that contains t, -1 when
 * theta(t) = 0.  Everything is determined by the input: no output depends on the run, on an option or on scheduling.
 * The walk-up rule: from node[t], moving to the parent while the parent's level is still >= k ends at the node whose set is
 * t's k-nucleus.
 * komb_nucleus_hierarchy_count: the nodes.  komb_nucleus_hierarchy_fetch_nodes: k, rep, parent, size, shell.
 * komb_nucleus_hierarchy_fetch_triangles: node[n_triangles].
 * komb_nucleus_hierarchy_labels runs the walk-up rule on the device, one walk per triangle over the stored forest:
 * label[t] = the rep of t's k-nucleus, -1 when theta(t) < k; size[t] = that nucleus's triangles, 0 when theta(t) < k.
 * KOMB_NUCLEUS_K_MAX resolves to the largest theta of the result; after that, k <= 1 runs as 1 (so a result without a
 * member gives -1 / 0 everywhere); k above the largest theta gives -1 / 0 everywhere; k < -1: KOMB_ERR_ARG.  Either output may
 * be NULL.
 * komb_nucleus_hierarchy_nuclei lists the k-nuclei as subgraphs, in ascending rep order: rep, the triangles, the distinct
 * canonical edges and the distinct vertices of each (the density edges / C(vertices, 2) is the caller's to form).  k
 * resolves as for _labels.  *n_nuclei is the number of k-nuclei; with all four arrays NULL the call only counts.  With an
 * array given, cap < the number of k-nuclei is KOMB_ERR_ARG and nothing is written.
 * komb_nucleus_hierarchy_info: nodes, nodes without a parent, the largest theta of the nucleus result (-1 without a
 * triangle), depth = the most nodes on a path from a root down (0 without nodes), the triangles with theta >= 1, and ms --
 * the device time of komb_nucleus_hierarchy_run on the context's HIP-event timer.  Any pointer may be NULL.
 * No context or no graph loaded: KOMB_ERR_ARG.  komb_nucleus_hierarchy_run without a nucleus decomposition of the current
 * k-truss result, every other call without a hierarchy of the current decomposition: KOMB_ERR_STATE.  A result without a
 * 4-clique has no nodes; not an error.  A pool failure: KOMB_ERR_NOMEM.  The run enumerates the 4-cliques once more (the
 * decomposition keeps none) into exactly n_cliques4 records; a different count is KOMB_ERR_DEVICE and installs nothing.
 * The result lives in blocks of its own (5 n_nodes + n_triangles words), installed when a run has succeeded.  It indexes one
 * nucleus result: whatever replaces or drops that -- a new komb_nucleus_run, a new k-truss run of any kind,
 * komb_truss_unprepare, a graph load -- drops it too, so a refused or failed run leaves the previous hierarchy readable
 * exactly as long as the decomposition it indexes is the current one.  No other call changes or drops it; a run changes no
 * other result, no komb_stats field and not the resident k-truss preparation.  Option NUC_SHORT moves the length at which
 * a triangle's walked tail goes from its lane to its wave here as in komb_nucleus_run; it changes no result. */
#define KOMB_NUCLEUS_K_MAX (-1)   /* k = the largest theta of the nucleus result */
int komb_nucleus_hierarchy_run(komb_ctx *ctx);
int komb_nucleus_hierarchy_count(komb_ctx *ctx, int64_t *n_nodes);                       /* n_nodes may be NULL */
int komb_nucleus_hierarchy_fetch_nodes(komb_ctx *ctx, int32_t *k, int32_t *rep, int32_t *parent,
                                       int32_t *size, int32_t *shell);         /* [n_nodes] each, any may be NULL */
int komb_nucleus_hierarchy_fetch_triangles(komb_ctx *ctx, int32_t *node /*[n_triangles]*/);
int komb_nucleus_hierarchy_labels(komb_ctx *ctx, int32_t k, int32_t *label /*[n_triangles]*/, int32_t *size /*[n_triangles]*/);
int komb_nucleus_hierarchy_nuclei(komb_ctx *ctx, int32_t k, int64_t cap, int64_t *n_nuclei, int32_t *rep,
                                  int32_t *n_triangles, int32_t *n_edges, int32_t *n_vertices);   /* [cap] each, any may be NULL */
int komb_nucleus_hierarchy_info(komb_ctx *ctx, int64_t *n_nodes, int64_t *n_roots, int32_t *theta_max, int32_t *depth,
                                int64_t *n_member_triangles, double *ms);      /* any may be NULL */

/* ---- maximum-clique search with a certified bound ------------------------- */
/* The object every rung above relaxes: the largest set of vertices that are pairwise adjacent.  For the unitig graph, a union of
 * per-read cliques, it is the largest set of unitigs that pairwise co-occur.
 * Input: the last COMPLETE k-truss result on the resident graph, whole graph or vmask run alike -- its ne_sub canonical edges
 * (eu[i], ev[i]), eu < ev, sorted by (eu, ev), original vertex ids, with their trussness t[i].  Call their graph H.  Trussness
 * here is support + 2, so K_n has trussness n: a clique of s vertices uses only edges of trussness >= s, and omega <= t_max, the
 * largest trussness of the result (0 without an edge).
 * A CLIQUE is a set of >= 2 vertices, pairwise adjacent in H.  OMEGA is the size of a largest clique of H, 0 when H has no edge
 * (singletons are not reported).  A MAXIMUM CLIQUE is a clique of omega vertices, written as its ascending id tuple.
 * The search is a branch and bound from every canonical edge (a, b) as the two smallest ids of a clique (DESIGN.md section
 * 4.6j).  A NODE is one candidate set taken off a search stack, a root's own included; every reported clique costs at least one.
 * komb_max_clique_run(ctx, budget): budget caps the nodes of the whole run -- the search for omega and the enumeration of all
 * maximum cliques.  0 means the default, 2^30; a negative value is KOMB_ERR_ARG; a value above 2^31 - 1 - KOMB_MAXCLQ_OVERSHOOT
 * runs as that (every count then fits int32).  The wavefronts add to one counter in batches of at most 256 nodes and stop
 * taking nodes once it has reached the budget: nodes <= budget + KOMB_MAXCLQ_OVERSHOOT always, so no launch runs unbounded.
 * flags: KOMB_MAXCLQ_EXACT -- omega is proven; KOMB_MAXCLQ_ENUMERATED -- every maximum clique was visited (implies EXACT);
 * KOMB_MAXCLQ_LISTED -- the sorted list is held (implies ENUMERATED).  With all three set every output is unique: nothing then
 * depends on the run, on an option or on scheduling.  A budget that runs out in the search clears all three (unless the clique
 * held has t_max vertices, which proves it); one that runs out in the enumeration leaves EXACT.
 * komb_max_clique_info: omega = the size of the witness, a clique whose every pair was checked against H on the device;
 * upper = a certified bound, omega <= the true omega <= upper <= t_max, equal to omega exactly when EXACT is set, t_max
 * otherwise -- it uses this k-truss result only (a nucleus decomposition that happens to exist does not tighten it: the bound
 * does not depend on call history); n_max_cliques = the number of maximum cliques with ENUMERATED, else -1; n_roots = the
 * canonical edges whose subproblem was opened; nodes = the nodes spent; ms = the device time of the run on the context's
 * HIP-event timer.  Any pointer may be NULL.
 * komb_max_clique_fetch: count[v] = the maximum cliques that contain v with ENUMERATED, else 1 on the witness' vertices and 0
 * elsewhere; witness[omega] ascending = the first clique of the list with LISTED, else whichever clique the search holds (NOT
 * unique: it depends on scheduling).  Either may be NULL.
 * komb_max_clique_list: all maximum cliques as ascending tuples in lexicographic order, verts[n_cliques * omega]; verts == NULL
 * returns the count only; cap < the count with verts given is KOMB_ERR_ARG and nothing is written; without LISTED:
 * KOMB_ERR_LIMIT.
 * H without an edge: omega = upper = t_max = 0, no witness, every count 0, n_max_cliques = 0, flags = 7.
 * No context or no graph loaded: KOMB_ERR_ARG, nothing is written.  Without a completed k-truss result on this graph, after
 * komb_truss_run_slice / a sharded run that materialised only part of the canonical edges, after komb_truss_unprepare, fetch /
 * list / info before a run: KOMB_ERR_STATE.  A root edge with more than 4096 candidates of the trussness the phase asks for:
 * KOMB_ERR_LIMIT (a candidate set is one 64-bit word per lane of a wavefront), checked before the phase starts.  A pool failure:
 * KOMB_ERR_NOMEM.
 * The result lives in storage of its own, installed when a run has succeeded: a refused or failed run leaves the previous result
 * readable.  It describes one k-truss result: whatever replaces or drops that result -- a new k-truss run of any kind,
 * komb_truss_unprepare, a graph load -- drops it too.  No other call changes or drops it; a run changes no other result, no
 * komb_stats field and not the resident k-truss preparation.  Options (none changes a result that carries all three flags):
 * MAXCLQ_SEED=0 skips the greedy seed (dives from edges of the largest trussness), so the search starts from lower bound 1;
 * MAXCLQ_LDS=<n>, 0 .. 512 (default 512): the largest candidate set whose bit matrix lives in LDS -- larger ones use the
 * workgroup's slot of global scratch, 0 sends everything there; MAXCLQ_LIST=<n> keeps the list only up to n maximum cliques
 * (default 65536); MAXCLQ_DEBUG=1 prints one stderr line with the counts, the nodes and the device time of each phase. */
#define KOMB_MAXCLQ_EXACT      1
#define KOMB_MAXCLQ_ENUMERATED 2
#define KOMB_MAXCLQ_LISTED     4
#define KOMB_MAXCLQ_OVERSHOOT  262144   /* 1024 wavefronts x 256 nodes */
int komb_max_clique_run(komb_ctx *ctx, int64_t budget);
int komb_max_clique_fetch(komb_ctx *ctx, int32_t *count /*[nv]*/, int32_t *witness /*[omega]*/);   /* either may be NULL */
int komb_max_clique_list(komb_ctx *ctx, int64_t cap, int64_t *n_cliques, int32_t *verts /*[cap * omega]*/);
int komb_max_clique_info(komb_ctx *ctx, int32_t *omega, int32_t *upper, int32_t *flags, int32_t *t_max, int64_t *n_max_cliques,
                         int64_t *n_roots, int64_t *nodes, double *ms);   /* any may be NULL */

/* ---- clique census: exact k-clique counts for every k ---------------------- */
/* What lies between the triangle and 4-clique counts of komb_nucleus_info and the maximum cliques above: the number of k-cliques
 * of H for every k of a window, and the k-cliques through every vertex for one k.  H, CLIQUE and t_max are those of the
 * maximum-clique search: the last COMPLETE k-truss result on the resident graph, whole graph or vmask run alike.
 * komb_clique_census_run(ctx, k_lo, k_hi, k_local, budget) computes total[k] = the number of k-cliques of H for every k in
 * [k_lo, k_hi] and, if k_local != 0, local[v] = the number of k_local-cliques of H that contain vertex v.  2 <= k_lo <= k_hi;
 * k_hi = -1 means t_max, and a k_hi above t_max runs as t_max, for no clique has more than t_max vertices -- but never below
 * k_lo, so the window always has an entry (a window that lies above t_max is all zeros); komb_clique_census_info reports the
 * k_hi the run used.  k_local is 0 or lies in [k_lo, k_hi] as used.  Anything else is KOMB_ERR_ARG.  A clique of >= k_lo
 * vertices uses only edges of trussness >= k_lo, so a high k_lo is cheap on a large graph.
 * Every count is a uint64_t and SATURATES: an entry is exactly min(the true value, 2^64 - 1).  Saturating adds of non-negative
 * numbers commute, so every output of a complete run is unique: nothing depends on the run, on an option or on scheduling.
 * The cliques are not enumerated but counted by pivoting (Jain and Seshadhri, WSDM 2020) from every
 * canonical edge (a, b) as the two smallest ids of a clique.  A NODE is one candidate set evaluated, a root's own included.
 * budget caps the nodes of the run exactly as komb_max_clique_run's does: 0 means the default, 2^30; a negative value is
 * KOMB_ERR_ARG; a value above 2^31 - 1 - KOMB_MAXCLQ_OVERSHOOT runs as that; nodes <= budget + KOMB_MAXCLQ_OVERSHOOT always.
 * flags: KOMB_CENSUS_COMPLETE -- the budget did not run out; KOMB_CENSUS_SATURATED -- some total or local entry equals
 * 2^64 - 1.  Without COMPLETE every entry is a lower bound of the true value: every clique counted is one, and none is counted
 * twice.
 * komb_clique_census_fetch: total[k_hi - k_lo + 1], entry i for k = k_lo + i, and local[nv].  Either may be NULL; local given
 * after a run with k_local == 0 is KOMB_ERR_STATE.
 * komb_clique_census_info: the window and k_local of the run; t_max; omega = the largest k of the window with total[k] > 0, 0
 * if there is none -- it is the clique number of H only when COMPLETE is set and k_hi reached t_max (a window that stops below
 * t_max, or a budget that ran out, sees only part of the cliques); flags; max_candidates = the largest candidate set of a root
 * at trussness >= k_lo; n_roots = the canonical edges whose subproblem was opened; nodes = the nodes spent; ms = the device time
 * of the run on the context's HIP-event timer.  Any pointer may be NULL.
 * H without an edge: every total 0, every local 0, omega = t_max = 0, flags = 1.
 * No context or no graph loaded: KOMB_ERR_ARG, nothing is written.  Without a completed k-truss result on this graph, after
 * komb_truss_run_slice / a sharded run that materialised only part of the canonical edges, after komb_truss_unprepare, fetch /
 * info before a run: KOMB_ERR_STATE.  A root edge with more than 4096 candidates of trussness >= k_lo: KOMB_ERR_LIMIT, checked
 * before anything is counted.  A pool failure: KOMB_ERR_NOMEM.
 * The result lives in storage of its own, installed when a run has succeeded: a refused or failed run leaves the previous result
 * readable.  It describes one k-truss result: whatever replaces or drops that result -- a new k-truss run of any kind,
 * komb_truss_unprepare, a graph load -- drops it too.  No other call changes or drops it; a run changes no other result, no
 * komb_stats field and not the resident k-truss preparation.  Options (none changes a result):
 * CENSUS_LDS=<n>, 0 .. 512 (default 512): the largest candidate set whose bit matrix lives in LDS -- larger ones use the
 * workgroup's slot of global scratch, 0 sends everything there; CENSUS_PIVOT=first|max (default max): the pivot of a node is
 * its first candidate, or the one with the most neighbours among the candidates; CENSUS_DEBUG=1 prints one stderr line with the
 * counts, the nodes and the device time. */
#define KOMB_CENSUS_COMPLETE  1
#define KOMB_CENSUS_SATURATED 2
int komb_clique_census_run(komb_ctx *ctx, int32_t k_lo, int32_t k_hi, int32_t k_local, int64_t budget);
int komb_clique_census_fetch(komb_ctx *ctx, uint64_t *total /*[k_hi - k_lo + 1]*/, uint64_t *local /*[nv]*/);   /* either may be NULL */
int komb_clique_census_info(komb_ctx *ctx, int32_t *k_lo, int32_t *k_hi, int32_t *k_local, int32_t *t_max, int32_t *omega,
                            int32_t *flags, int32_t *max_candidates, int64_t *n_roots, int64_t *nodes, double *ms);   /* any may be NULL */

/* ---- maximal cliques: Bron-Kerbosch with pivoting ---------------------------- */
/* What igraph_maximal_cliques / maximal_cliques_hist / maximal_cliques_count and networkx.find_cliques give: the cliques that
 * cannot be extended.  For the unitig graph, a union of per-read cliques, they are the repeat families themselves: the groups of
 * unitigs that all co-occur pairwise and to which no further unitig can be added.  H, CLIQUE, trussness (= support + 2) and
 * t_max are those of the maximum-clique search: the last COMPLETE k-truss result on the resident graph, whole graph or vmask
 * run alike.
 * A MAXIMAL CLIQUE is a clique of H contained in no larger clique of H.  komb_maximal_cliques_run(ctx, k_min, budget) reports
 * the maximal cliques of at least k_min vertices, k_min >= 2 (singletons are not reported; an edge in no triangle is a maximal
 * clique of 2 vertices).  The cut by k_min is exact: a clique C of >= k_min vertices uses only edges of trussness >= k_min, and
 * so does C + x for any vertex x adjacent to all of C -- so for such cliques maximal among the edges of trussness >= k_min is
 * maximal in H, the run looks at those edges only (a high k_min touches a small part of a large graph), and the maximal cliques
 * of that part with fewer than k_min vertices are simply not reported.
 * The walk is Bron-Kerbosch with pivoting from every canonical edge (a, b) as the two smallest ids of a clique, with the common
 * neighbours above b as candidates and those below b as excluded vertices.  A NODE is one pair of
 * candidate and excluded set evaluated, a root's own included; every reported clique costs at least one.  budget caps the nodes
 * of the run exactly as komb_max_clique_run's does: 0 means the default, 2^30; a negative value is KOMB_ERR_ARG; a value above
 * 2^31 - 1 - KOMB_MAXCLQ_OVERSHOOT runs as that; nodes <= budget + KOMB_MAXCLQ_OVERSHOOT always.  So n_cliques and every count
 * fit int32 and nothing saturates.
 * flags: KOMB_MAXIMAL_COMPLETE -- the budget did not run out; KOMB_MAXIMAL_LISTED -- the sorted list is held (implies
 * COMPLETE).  With COMPLETE every output is unique: nothing depends on the run, on an option or on scheduling.  Without it what
 * was reported is a lower bound: every reported clique is maximal in H and none is reported twice.
 * komb_maximal_cliques_fetch: hist[k_hi - k_min + 1], entry i = the number of reported cliques of k_min + i vertices, with
 * k_hi = max(k_min, t_max), so there is always an entry; count[nv] = the reported cliques that contain the vertex;
 * largest[nv] = the size of the largest of them, 0 if none.  Any may be NULL.
 * komb_maximal_cliques_list: the reported cliques as ascending tuples in lexicographic tuple order, CSR style: clique i is
 * verts[offset[i], offset[i + 1]), offset[n_cliques] = n_verts.  offset == NULL and verts == NULL returns the two counts only;
 * an output given with its cap below its count is KOMB_ERR_ARG and nothing is written; without LISTED: KOMB_ERR_LIMIT.
 * komb_maximal_cliques_info: k_min and k_hi of the run; t_max; omega = the largest size with a non-zero hist entry, 0 if none
 * (the clique number of H when COMPLETE is set and k_min <= it); flags; n_cliques = the sum of hist; max_candidates = the largest
 * number of candidates and excluded vertices of a root at trussness >= k_min; n_roots = the canonical edges whose subproblem
 * was opened; nodes = the nodes spent; ms = the device time of the run on the context's HIP-event timer.  Any pointer may be
 * NULL.
 * H without an edge, or k_min above t_max: every hist, count and largest entry 0, omega 0, flags = 3, an empty list.
 * No context or no graph loaded: KOMB_ERR_ARG, nothing is written.  k_min < 2 or a negative budget: KOMB_ERR_ARG.  Without a
 * completed k-truss result on this graph, after komb_truss_run_slice / a sharded run that materialised only part of the
 * canonical edges, after komb_truss_unprepare, fetch / list / info before a run: KOMB_ERR_STATE.  A root edge with more than 4096
 * candidates and excluded vertices together, of trussness >= k_min: KOMB_ERR_LIMIT, checked before anything is reported (the
 * census and the search count candidates only: this limit is this call's own).  A pool failure: KOMB_ERR_NOMEM.
 * The result lives in storage of its own, installed when a run has succeeded: a refused or failed run leaves the previous result
 * readable.  It describes one k-truss result: whatever replaces or drops that result -- a new k-truss run of any kind,
 * komb_truss_unprepare, a graph load -- drops it too.  No other call changes or drops it; a run changes no other result, no
 * komb_stats field and not the resident k-truss preparation.  Options (none changes a complete result, except that MAXIMAL_LIST
 * decides whether the list is held):
 * MAXIMAL_LDS=<n>, 0 .. 512 (default 512): the largest candidate list whose bit matrix lives in LDS -- larger ones use the
 * workgroup's slot of global scratch, 0 sends everything there; MAXIMAL_PIVOT=first|max (default max): the pivot of a node is
 * its first candidate, or the candidate or excluded vertex with the most neighbours among the candidates; MAXIMAL_LIST=<n>,
 * 0 .. 2^24 (default 65536): the list is held when the run reports at most n cliques and their sizes + 1 sum to at most
 * min(n * (t_max + 1), 2^24) words; MAXIMAL_DEBUG=1 prints one stderr line with the counts, the nodes and the device time. */
#define KOMB_MAXIMAL_COMPLETE 1   /* the budget did not run out */
#define KOMB_MAXIMAL_LISTED   2   /* the sorted list is held (implies COMPLETE) */
int komb_maximal_cliques_run(komb_ctx *ctx, int32_t k_min, int64_t budget);
int komb_maximal_cliques_fetch(komb_ctx *ctx, int64_t *hist /*[k_hi - k_min + 1]*/, int32_t *count /*[nv]*/, int32_t *largest /*[nv]*/);   /* any may be NULL */
int komb_maximal_cliques_list(komb_ctx *ctx, int64_t cap_cliques, int64_t cap_verts, int64_t *n_cliques, int64_t *n_verts,
                              int64_t *offset /*[cap_cliques + 1]*/, int32_t *verts /*[cap_verts]*/);
int komb_maximal_cliques_info(komb_ctx *ctx, int32_t *k_min, int32_t *k_hi, int32_t *t_max, int32_t *omega, int32_t *flags,
                              int64_t *n_cliques, int32_t *max_candidates, int64_t *n_roots, int64_t *nodes, double *ms);   /* any may be NULL */

/* ---- k-clique communities: clique percolation -------------------------------- */
/* What networkx.algorithms.community.k_clique_communities gives (Palla, Derenyi, Farkas, Vicsek, Nature 2005): the overlapping
 * communities of H, the last COMPLETE k-truss result.  For the unitig graph a maximal clique is one repeat family; a k-clique
 * community is a chain of families that overlap almost completely, and a unitig may lie in several of them -- which k-truss
 * communities, SCAN clusters and nuclei, each a partition of edges or triangles, cannot express.
 * Fix k >= 2.  The MEMBER cliques are the maximal cliques of H with at least k vertices.  Two member cliques are ADJACENT when
 * they share at least k - 1 vertices.  A k-CLIQUE COMMUNITY is the union of the vertex sets of one connected class of member
 * cliques.  This equals the original definition (the k-cliques of H joined through shared (k - 1)-cliques): every k-clique lies
 * in a member clique, the k-cliques inside one clique are connected, and two cliques that share k - 1 vertices hold two
 * k-cliques that do.  A vertex may lie in several communities; the communities of k + 1 lie inside those of k; at k = 2 they are
 * the connected components of H without its isolated vertices; at k = 3 their vertex sets are those of the k-truss communities
 * at k = 3, at k = 4 those of the 1-nuclei of the nucleus hierarchy.
 * komb_clique_communities_run(ctx, k, budget) works on the list that komb_maximal_cliques_run holds (KOMB_MAXIMAL_LISTED, with a
 * k_min <= k); all clique indices are positions in that sorted list, as komb_maximal_cliques_list gives it.  The REP of a
 * community is the smallest index of its cliques; communities are numbered 0 .. n - 1 in ascending rep order.
 * Adjacent pairs are found through the cliques' incidence, not by testing all pairs: a clique of s vertices has s - k + 2
 * PIVOTS, its vertices of smallest (load, id), load = the member cliques through the vertex, and every clique adjacent to it
 * contains one of them.  pair_tests = the sum over member cliques i and their pivots v of the member
 * cliques j > i through v: the candidates the run looks at, a deterministic number computed before anything is linked.
 * budget caps it: 0 means the default, 2^32; a negative value is KOMB_ERR_ARG; when pair_tests exceeds the budget the run is
 * refused with KOMB_ERR_LIMIT before anything is linked (the message names both numbers).  There are no partial results.
 * komb_clique_communities_count: the number n of communities and n_member_verts = offset[n], the sum of their vertex counts.
 * komb_clique_communities_fetch: label[i] = the rep of clique i's community, -1 for a clique of fewer than k vertices;
 * size[i] = the number of cliques of that community, 0 for such a clique; both [n_cliques of the list].
 * komb_clique_communities_fetch_communities: rep[n], n_cliques[n] = the cliques of the community, offset[n + 1] and
 * verts[n_member_verts]: community c is verts[offset[c], offset[c + 1]), ascending and distinct.
 * komb_clique_communities_fetch_vertices: n_comm[nv] = how many communities contain the vertex; first[nv] = the smallest
 * community number that contains it, -1 if none.
 * komb_clique_communities_info: k; k_min = that of the list used; n_member_cliques; n_communities; largest = the most vertices
 * in one community; n_covered = the vertices with n_comm >= 1; n_overlap = those with n_comm >= 2; pair_tests; ms = the device
 * time of the run on the context's HIP-event timer.  Any output pointer may be NULL.
 * A list without a member clique (H without an edge, k above t_max): n = 0, every label -1, every size and n_comm 0, every
 * first -1, offset = {0}; not an error.
 * No context or no graph loaded: KOMB_ERR_ARG, nothing is written.  k < 2 or a negative budget: KOMB_ERR_ARG.  No
 * maximal-cliques result of the current k-truss result, or one whose k_min is above k (the list lacks member cliques; the
 * message names both numbers): KOMB_ERR_STATE, as is a count / fetch / info before a run.  A maximal-cliques result without
 * KOMB_MAXIMAL_LISTED: KOMB_ERR_LIMIT, as komb_maximal_cliques_list answers.  A pool failure: KOMB_ERR_NOMEM.
 * The result is built on the side and installed when a run has succeeded, as komb_maximal_cliques_run does: a refused or failed
 * run leaves the previous result readable.  It describes one maximal-cliques result and goes with it: a komb_maximal_cliques_run
 * that succeeds, a new k-truss run of any kind, komb_truss_unprepare and a graph load drop it.  No other call changes or drops
 * it; a run changes no other result, no komb_stats field and not the resident k-truss preparation.  Every output is unique:
 * nothing depends on the run, on an option or on scheduling.  Options: PERC_GROUP=4|16|64: the lanes that intersect one candidate
 * with the clique at hand (default: chosen per clique from its size: up to 8 vertices 4, up to 32 vertices 16, else 64);
 * PERC_DEBUG=1 prints one stderr line with the counts, pair_tests and the device time. */
int komb_clique_communities_run(komb_ctx *ctx, int32_t k, int64_t budget);
int komb_clique_communities_count(komb_ctx *ctx, int64_t *n_communities, int64_t *n_member_verts);   /* any may be NULL */
int komb_clique_communities_fetch(komb_ctx *ctx, int32_t *label /*[n_cliques of the list]*/, int32_t *size /*[n_cliques of the list]*/);   /* any may be NULL */
int komb_clique_communities_fetch_communities(komb_ctx *ctx, int32_t *rep /*[n]*/, int32_t *n_cliques /*[n]*/, int64_t *offset /*[n + 1]*/,
                                              int32_t *verts /*[n_member_verts]*/);   /* any may be NULL */
int komb_clique_communities_fetch_vertices(komb_ctx *ctx, int32_t *n_comm /*[nv]*/, int32_t *first /*[nv]*/);   /* any may be NULL */
int komb_clique_communities_info(komb_ctx *ctx, int32_t *k, int32_t *k_min, int64_t *n_member_cliques, int64_t *n_communities, int64_t *largest,
                                 int64_t *n_covered, int64_t *n_overlap, int64_t *pair_tests, double *ms);   /* any may be NULL */

/* ---- k-truss ----------------------------------------------------------- */
/* Replaces igraph_induced_subgraph_map + igraph_trussness
 * (src/graph.cpp:502, src/graph.cpp:508).  vmask (host, nv bytes, nullable)
 * selects the induced subgraph exactly like the max-core vertex list built at
 * src/graph.cpp:470-473; NULL = whole graph.  Edges are reported with ORIGINAL
 * vertex ids (what invmap gives at src/graph.cpp:531-532), canonical order.
 * komb_truss_run computes on the device (timed region) and leaves the trussness
 * vector there in canonical edge order -- igraph_trussness's output, indexed by
 * edge id.  komb_truss_fetch copies (eu,ev,truss)[ne_sub] out; any of the three
 * may be NULL.  The ENDPOINTS of the canonical edges are what igraph_edge answers
 * afterwards (src/graph.cpp:529-532), not part of igraph_trussness: for a
 * whole-graph run they are made by the first fetch that asks for them and kept
 * with the graph (a run under a vmask makes its subgraph's before it returns).
 * Trussness of a triangle-free edge is 2.
 * A run drops the previous k-truss result, and every analysis that indexes it, once its arguments have been accepted: a
 * run that fails after that (KOMB_ERR_NOMEM, KOMB_ERR_LIMIT, KOMB_ERR_DEVICE) leaves NO k-truss result -- komb_truss_count
 * and the fetches answer KOMB_ERR_STATE -- holds nothing of the one it had begun, and changes no k-core, onion, components,
 * hierarchy or densest-subgraph result.  The record stream of the default index layout is memory the run can do without:
 * where that is refused the run builds the index by the exact two-pass layout instead and succeeds
 * (komb_stats.index_layout says which). */
int komb_truss_run(komb_ctx *ctx, const uint8_t *vmask);
/* What igraph_trussness does to its argument before it lists a triangle (src/graph.cpp:508: vertices ordered by degree,
 * every edge oriented from its lower to its higher endpoint) is the k-truss PREPARATION here: (degree,id)-ranked internal
 * ids, the oriented CSR in them, the map back to the canonical edge order, the enumeration's per-vertex lines and task
 * table.  The first k-truss call of a graph makes it, inside the call and its time
 * (komb_stats.ms_prepare), and it stays with the graph: later calls find it.  komb_truss_prepare makes it ahead of time
 * (a no-op when it exists); komb_truss_unprepare drops it together with the last k-truss result (bench.py times
 * unprepare + komb_truss_run: nothing of a previous call is reused).  A vmask run prepares its induced subgraph every time. */
int komb_truss_prepare(komb_ctx *ctx);
int komb_truss_unprepare(komb_ctx *ctx);
/* One process per GPU, every rank holding the same graph: the triangle-support
 * phase is sharded by source-vertex range [rank/world) and the partial support
 * vectors (|E|+1 words) are summed across ranks by `allreduce` -- an in-place SUM
 * all-reduce over uint32[count] in device memory (the host implements it with RCCL; the
 * library has drained its stream when it calls, the reduction must be complete when the
 * callback returns; 32-bit two's-complement sums, so an int32 view of the words is fine;
 * return 0 on success).  Incidence index, peel and gather then run on every rank; all
 * ranks end with identical results.  world == 1 is komb_truss_run.
 * komb_set_shard_peel(ctx, 1) makes the following sharded runs split the PEEL as well: rank r owns the internal edge ids
 * [m*r/world, m*(r+1)/world) -- their live supports and the decrements on them -- and the ranks exchange their parts of
 * the frontier every sub-round through the same callback (as komb_core_run_sharded does for vertices).  Same results;
 * slower than the replicated peel on one node (DESIGN.md section 6 has the measurements), hence opt-in. */
int komb_truss_run_sharded(komb_ctx *ctx, const uint8_t *vmask, int32_t rank, int32_t world,
                           komb_allreduce_fn allreduce, void *user);
int komb_set_shard_peel(komb_ctx *ctx, int32_t on);
/* One process per GPU, every rank holding the same graph, NO exchange: every rank runs the whole k-truss path (support,
 * index and peel of one graph do not shard across GPUs at a profit: DESIGN.md section 6) and materialises the results of
 * ITS slice of the canonical edges only -- truss[k], support[k] for k in [ne*rank/world, ne*(rank+1)/world), zeros
 * elsewhere (a SUM all-reduce of the ranks' arrays is the whole result; eu / ev are complete on every rank).  What
 * bench.py --gpus N runs by default.  With a vmask the results are complete on every rank.  world == 1 is komb_truss_run. */
int komb_truss_run_slice(komb_ctx *ctx, const uint8_t *vmask, int32_t rank, int32_t world);
int komb_truss_count(komb_ctx *ctx, int64_t *ne_sub);
/* (a fetch that fails -- the first one that asks for endpoints or supports makes them: KOMB_ERR_NOMEM -- has written none of
 * its outputs and leaves the result as it was) */
int komb_truss_fetch(komb_ctx *ctx, int32_t *eu, int32_t *ev, int32_t *truss);
/* per-edge triangle counts the peel started from (canonical order): an extra of this library (igraph_trussness has no
 * such output), put into canonical order by the first call after a run */
int komb_truss_fetch_support(komb_ctx *ctx, int32_t *support);
int komb_trussness(komb_ctx *ctx, const uint8_t *vmask, int64_t *ne_out,
                   int32_t *eu, int32_t *ev, int32_t *truss);

/* ---- CoreA ------------------------------------------------------------- */
/* Replaces CoreA::getAnomalyScore + CoreA::fractionalRank x2
 * (src/CoreA.h:109-140, 142-187): key = coreness*n + degree in 64-bit
 * (src/CoreA.h:122 is `int`, undefined once it overflows); fractional ranks by
 * device sort + run bounds; |ln r_deg - ln r_key| with the host libm so the
 * "%f" text of CombineCoreA::run (src/CombineCoreA.h:36-39) is unchanged.
 * degree/coreness are host arrays (what readKOMBOutput returns,
 * src/CoreA.h:24-56). */
int komb_corea_scores(komb_ctx *ctx, const int32_t *degree, const int32_t *coreness,
                      int64_t nv, double *score);
/* the two rank vectors themselves (exact half-integers), for tests */
int komb_corea_ranks(komb_ctx *ctx, const int32_t *degree, const int32_t *coreness,
                     int64_t nv, double *rank_degree, double *rank_key);

/* Replaces CombineCoreA::runMerge over its two HashIndexedMinHeap instances (src/CombineCoreA.h:45-219,
 * src/HashIndexedMinHeap.h:10-238; dead code in the reference -- nothing calls it): the greedy densest-block
 * peel over a row copy and a column copy of the resident graph.  suspiciousness: host array [nv] (what
 * getAnomalyScore returns) or NULL for plain degrees.  order[2*nv] / side[2*nv] are filled from the back, as the
 * reference fills `order` / `modes`; the first *n_block entries are the densest block (rows: side 0, columns:
 * side 1), *max_density its density.  Ties between equal priorities are resolved exactly as the reference's heap
 * resolves them (the same sift operations in the same order), which makes the peel sequential: the device runs
 * it on one lane (heaps in LDS up to 4096 nodes; graphs above 2^17 nodes are refused with KOMB_ERR_LIMIT).  Two defects of the reference are not reproduced: removed[][]
 * read uninitialised (:104-108) and `cols` sized by the number of rows (:191).
 * Without a graph loaded on the context: KOMB_ERR_STATE.  A refusal (limit, state, argument) leaves the resident
 * graph and its results as they were. */
int komb_densest_block(komb_ctx *ctx, const double *suspiciousness, int32_t *order, int32_t *side,
                       int64_t *n_block, double *max_density);

/* ---- instrumentation --------------------------------------------------- */
int komb_get_stats(komb_ctx *ctx, komb_stats *out);
/* Measurement only: fills komb_stats.sum_deg_sq / wedge_items / max_degree / oriented_items of the resident graph (the
 * inputs of the roofline model's algorithmic bytes; makes the k-truss preparation if absent).  No product path calls it
 * (until ABI version 7 every graph build ran this 2.2 ms kernel). */
int komb_graph_moments(komb_ctx *ctx);

/* ---- graphlet census: 3- and 4-vertex orbit counts --------------------- */
/* The graphlet degree vector of Przulj ("Biological network comparison using graphlet degree distribution", Bioinformatics
 * 2007), orbits 0-14 as ORCA and PGD number them, on the last COMPLETE k-truss result (whole graph or vmask).  d(v) is the
 * number of result edges at v, t_e the support of canonical edge e (komb_truss_fetch_support).  Everything is an exact
 * unsigned 64-bit count.
 * Per canonical edge, [ne_sub] in canonical order (komb_graphlets_fetch_edges; either output may be NULL): cycles4[e] = the
 * 4-cycles, induced or not, that contain e; cliques4[e] = the 4-cliques that contain e.  (The triangles through e are its support.)
 * Per vertex (komb_graphlets_fetch_vertices): orbit[o * nv + v], orbit-major, o = 0 .. 14, the INDUCED subgraphs v lies in by
 * the position it holds: 0 edge end | 1, 2 end and middle of a 2-path | 3 triangle | 4, 5 end and inner vertex of a 4-path |
 * 6, 7 leaf and centre of a claw | 8 4-cycle | 9, 10, 11 the paw's pendant vertex, its two degree-2 triangle vertices, its
 * degree-3 vertex | 12, 13 the diamond's degree-2 and degree-3 vertices | 14 4-clique.  A vertex outside the result has fifteen zeros.
 * komb_graphlets_info: total[9] = the induced graphlets of the result -- edge, wedge, triangle, path4, claw, cycle4, paw,
 * diamond, clique4 -- summed in 128 bits and reported saturating at 2^64 - 1 (flags has KOMB_GRAPHLET_SATURATED when one did);
 * max_degree = the largest d(v); cycle_items = the entries the 4-cycle pass walked, sum over the vertices v, over their
 * neighbours u below v in (d, id) order, of the neighbours of u below v; n_triangles, n_cliques4 = total[2], total[8]
 * (saturating at 2^63 - 1); ms = the device time of the run on the context's HIP-event timer.  Any output may be NULL.
 * No context or no graph loaded: KOMB_ERR_ARG, nothing is written.  Without a completed k-truss result on this graph, after
 * komb_truss_run_slice / a sharded run that materialised only part of the canonical edges, after komb_truss_unprepare, fetch /
 * info before a run: KOMB_ERR_STATE.  A largest degree of 2^20 or more: KOMB_ERR_LIMIT, before anything is counted (below
 * it every count and every intermediate of the closed forms stays under 2^63: DESIGN.md section 4.6o).  A pool failure:
 * KOMB_ERR_NOMEM.  A result without edges has zeros everywhere; the empty graph is not an error.  Canonical endpoints and
 * supports of a whole-graph result that no fetch has asked for yet are made here as those fetches make them.
 * The result lives in arrays of its own, installed when a run has succeeded: a refused or failed run (KOMB_ERR_LIMIT,
 * KOMB_ERR_NOMEM, KOMB_ERR_DEVICE) leaves the PREVIOUS graphlet result readable and every other result as it was.  It indexes one k-truss
 * result: whatever replaces or drops that result -- a new k-truss run of any kind, komb_truss_unprepare, a graph load --
 * drops it too.  No other call changes or drops it; a run changes no other result, no komb_stats field and not the resident
 * k-truss preparation, and needs no nucleus run.
 * Options (none changes a result): GRAPHLET_SHORT=<n>: a root of the 4-cycle pass that walks up to n entries stays with one
 * wavefront (default and at most 128); GRAPHLET_LDS=<n>: up to n entries its table lives in a workgroup's LDS, above in
 * global scratch (default and at most 4096; 0 sends every root to global scratch); GRAPHLET_DEBUG: one stderr line with the
 * per-pass counts and device times. */
#define KOMB_GRAPHLET_ORBITS 15
#define KOMB_GRAPHLET_TYPES  9
#define KOMB_GRAPHLET_SATURATED 1
int komb_graphlets_run(komb_ctx *ctx);
int komb_graphlets_fetch_vertices(komb_ctx *ctx, uint64_t *orbit /*[15 * nv]*/);
int komb_graphlets_fetch_edges(komb_ctx *ctx, uint64_t *cycles4, uint64_t *cliques4 /*[ne_sub] each, either may be NULL*/);
int komb_graphlets_info(komb_ctx *ctx, uint64_t *total /*[9]*/, int32_t *flags, int32_t *max_degree,
                        int64_t *cycle_items, int64_t *n_triangles, int64_t *n_cliques4, double *ms);   /* any may be NULL */

/* ---- betweenness centrality from chosen sources ------------------------ */
/* Brandes' algorithm ("A faster algorithm for betweenness centrality", J. Math. Sociol. 2001) from a list of source vertices
 * (all of them, or a sample: Brandes & Pich 2007) on the RESIDENT graph: ORIGINAL ids, the symmetric CSR with ascending rows
 * that komb_graph_get_csr returns, every edge of length 1.  It needs no other result.  The values are IEEE-754 binary64, and
 * the ORDER OF EVERY ROUNDING OPERATION IS PART OF THE DEFINITION, so a result is a function of the graph and the source list
 * alone and compares bit for bit with any implementation that follows this text:
 * sources[n_sources] are vertex ids; sources == NULL means every vertex 0 .. nv-1 in ascending order (n_sources is then
 * ignored).  Duplicates are allowed and count as often as they are given.  An id outside [0, nv) or n_sources < 0:
 * KOMB_ERR_ARG.  n_sources == 0 is a valid run with zeros everywhere.
 * Per source s, in exactly these operations, none of them fused (no fused multiply-add):
 *   dist_s = the BFS distance from s (unreached: none); sigma_s[s] = 1.0.
 *   A vertex w at distance L >= 1:  acc = 0.0; for v in the row of w, in ascending id, with dist_s[v] == L-1:
 *     acc = acc + sigma_s[v];  then sigma_s[w] = acc.
 *   A reached vertex v at distance L, levels descending:  acc = 0.0; for w in the row of v, in ascending id, with
 *     dist_s[w] == L+1:  c = (1.0 + delta_s[w]) / sigma_s[w];  p = sigma_s[v] * c;  acc = acc + p;  then delta_s[v] = acc.
 *   An unreached vertex has delta_s = 0.0.
 * bc[v]:  acc = 0.0; for i = 0 .. n_sources-1 in the order given: if sources[i] != v: acc = acc + delta_{sources[i]}[v].
 * The value is RAW: neither halved nor normalised.  With every vertex as a source it is exactly twice igraph's / networkx's
 * undirected unnormalised betweenness (every pair counts from both ends); from a sample it is the sum over the sampled sources.
 * Per source, in the order given (komb_betweenness_fetch_sources; any output may be NULL): source[i] = the id; n_reached[i] =
 * the vertices reached, s itself included; sum_dist[i] = the exact sum of their distances; ecc[i] = the largest distance --
 * the integers of closeness, harmonic reach and an eccentricity / diameter lower bound, at no extra cost.
 * komb_betweenness_info (any output may be NULL): n_sources; flags has KOMB_BETWEENNESS_ROUNDED when some sigma reached 2^53
 * or more (the result is still the defined one, but sigma no longer counts the shortest paths exactly); depth_max = the largest
 * ecc; n_batches = the batches of up to 64 consecutive sources the run was made in, ceil(n_sources / 64); n_level_steps = the
 * level sweeps of the run, the sum over the batches of (E + 1) + max(E - 1, 0) where E is the batch's largest ecc -- the cost
 * of a run is a few kernel launches per step, so it grows with the depth; ms = the device time of the run on the context's
 * HIP-event timer.
 * A sigma that reaches +inf: KOMB_ERR_LIMIT, nothing is installed.  A pool failure: KOMB_ERR_NOMEM.  No context or no graph
 * loaded: KOMB_ERR_ARG.  Fetch or info before a run on this graph: KOMB_ERR_STATE.  A failing call writes nothing to its outputs.
 * The result lives in arrays of its own and is installed only when a run has succeeded: a refused or failed run (KOMB_ERR_ARG,
 * KOMB_ERR_NOMEM, KOMB_ERR_LIMIT, KOMB_ERR_DEVICE) leaves the PREVIOUS betweenness result readable.  It belongs to the graph: a
 * graph load drops it.  No k-core, k-truss or other analysis call changes or drops it, and a run changes none of their results,
 * no komb_stats field and not the resident k-truss preparation.
 * Memory: dist, sigma and delta of one batch are [nv][64] arrays from the context's pool, about 1.3 KB per vertex, given back
 * when the run ends.
 * Options (none changes a result): BTW_GRID=<n>: at most n workgroups per level sweep (default and at most 2048; tests lower
 * it to make every wave take several vertices); BTW_DEBUG: one stderr line with the per-batch level counts and times and the
 * share of row entries the frontier masks skipped. */
#define KOMB_BETWEENNESS_ROUNDED 1
int komb_betweenness_run(komb_ctx *ctx, int64_t n_sources, const int32_t *sources /* NULL: all */);
int komb_betweenness_fetch(komb_ctx *ctx, double *bc /*[nv], may be NULL*/);
int komb_betweenness_fetch_sources(komb_ctx *ctx, int32_t *source, int64_t *n_reached, int64_t *sum_dist, int32_t *ecc /*[n_sources] each, any may be NULL*/);
int komb_betweenness_info(komb_ctx *ctx, int64_t *n_sources, int32_t *flags, int32_t *depth_max, int64_t *n_batches,
                          int64_t *n_level_steps, double *ms);   /* any may be NULL */

/* ---- distance analysis from chosen sources ----------------------------- */
/* Closeness and harmonic sums, eccentricities and the neighbourhood function (hop plot) from a list of source vertices (all of
 * them, or a sample: Eppstein & Wang 2004) on the RESIDENT graph, as for komb_betweenness_run: ORIGINAL ids, the symmetric CSR
 * that komb_graph_get_csr returns, every edge of length 1.  It needs no other result.  Let d(i, v) be the distance from
 * sources[i] to v where v can be reached; a source reaches itself at distance 0; a vertex that appears k times in the list
 * counts k times, once per entry.  sources == NULL means every vertex in ascending order (n_sources is ignored).
 * Per vertex v (komb_distances_fetch; any output may be NULL):
 *   n_reached[v] = #{i : d(i, v) exists};  sum_dist[v] = the sum of those d(i, v);  ecc[v] = the largest of them, -1 when no
 *   source reaches v.  harmonic[v] is an IEEE-754 binary64 whose ROUNDING ORDER IS PART OF THE DEFINITION:
 *     cut the list into blocks of 64 consecutive entries.  For block b: h_b = 0.0; for L = 1, 2, ... ascending: c = #{i in b :
 *     d(i, v) = L}; if c > 0: h_b = h_b + (double)c / (double)L (the division rounds once, then the addition rounds once).
 *     Then harmonic[v] = 0.0; for b ascending: harmonic[v] = harmonic[v] + h_b.
 *   It is a function of the graph and the list only, whatever DIST_WORDS and DIST_GRID are.  (Closeness in igraph's sense is
 *   (n_reached[v] - 1) / sum_dist[v] after a run from every vertex; the harmonic centrality of networkx is harmonic[v].)
 * Per source, in the order given (komb_distances_fetch_sources; any output may be NULL): the integers that
 * komb_betweenness_fetch_sources defines, with the same meaning: source[i] = the id; n_reached[i] = the vertices reached, the
 * source included; sum_dist[i] = the sum of their distances; ecc[i] = the largest.  With sources == NULL the two views agree
 * by symmetry.
 * komb_distances_histogram: pairs[L] = #{(i, v) : d(i, v) = L} for L = 0 .. depth_max.  cap = the room at pairs in entries:
 * cap < depth_max + 1 is KOMB_ERR_ARG and nothing is written.
 * komb_distances_info (any output may be NULL): n_sources; flags has KOMB_DISTANCES_ALL when the run had sources == NULL: ecc[]
 * are then the exact eccentricities, depth_max the diameter of the component with the largest one (otherwise a lower bound),
 * depth_min, the smallest per-source ecc, the radius in igraph's sense (0 when a vertex is isolated; 0 without a source), and
 * sum_all twice the Wiener index.  n_pairs = the sum of pairs[]; sum_all = the sum of L * pairs[L].  n_batches = the batches
 * of 64 W consecutive sources the run was made in, ceil(n_sources / (64 W)), W = DIST_WORDS; n_level_steps = the level steps
 * of the run, the sum over the batches of E + 1 where E is the batch's largest ecc (the last step of a batch finds nothing);
 * both are 0 on a graph without a vertex.  ms = the device time.
 * Every count fits 63 bits: n_sources and the number of vertices nv are below 2^31, so n_reached[], pairs[] and n_pairs are
 * at most n_sources * nv < 2^62, and a sum_dist[] is at most 2^31 distances below 2^31 each, < 2^62.  sum_all is n_pairs
 * times the mean distance: it fits unless that reaches 2^63, which takes more than 2^30 sources on more than 2^30 vertices
 * at a mean distance above 8 -- a run out of reach of the level-by-level traversal; the value would wrap.
 * n_sources < 0, or an id outside [0, nv): KOMB_ERR_ARG.  A pool failure: KOMB_ERR_NOMEM.  No context or no graph loaded:
 * KOMB_ERR_ARG.  Fetch, histogram or info before a run on this graph: KOMB_ERR_STATE.  A failing call writes nothing to its
 * outputs.  The result lives in arrays of its own and is installed only when a run has succeeded: a refused or failed run
 * leaves the PREVIOUS distance result readable.  It belongs to the graph: a graph load drops it.  No k-core, k-truss,
 * betweenness or other analysis call changes or drops it, and a run changes none of their results, no komb_stats field and not
 * the resident k-truss preparation.
 * Memory: three masks and a partial sum of W 64-bit words each and 28 bytes of result per vertex, about 60 to 160 bytes per
 * vertex, the masks given back when the run ends.
 * Options (none changes a result): DIST_WORDS=1|2|4: W, the 64-bit words per vertex and mask, so 64 W sources share one pass
 * over the rows (default 4; other values round down to one of the three); DIST_GRID=<n>: at most n workgroups per level step
 * (default and at most 2048; tests lower it to make every wave take several turns); DIST_DEBUG: one stderr line with the batch
 * and level counts and the share of row entries the early exit skipped. */
#define KOMB_DISTANCES_ALL 1
int komb_distances_run(komb_ctx *ctx, int64_t n_sources, const int32_t *sources /* NULL: all */);
int komb_distances_fetch(komb_ctx *ctx, int64_t *n_reached, int64_t *sum_dist, int32_t *ecc, double *harmonic /*[nv] each, any may be NULL*/);
int komb_distances_fetch_sources(komb_ctx *ctx, int32_t *source, int64_t *n_reached, int64_t *sum_dist, int32_t *ecc /*[n_sources] each, any may be NULL*/);
int komb_distances_histogram(komb_ctx *ctx, int64_t *pairs /*[depth_max + 1]*/, int64_t cap);
int komb_distances_info(komb_ctx *ctx, int64_t *n_sources, int32_t *flags, int32_t *depth_max, int32_t *depth_min,
                        int64_t *n_pairs, int64_t *sum_all, int64_t *n_batches, int64_t *n_level_steps, double *ms);   /* any may be NULL */

/* ---- synthetic workload (host code, no device) ------------------------- */
/* Power-law "hybrid unitig graph" generator of SURVEY.md section 8(d): a union
 * of n_cliques small cliques (size min(1+Geom(0.45),6)) whose members are drawn
 * from w_i ~ (i+1)^(-1/(alpha-1)) and scattered by a seeded bijection; mirrors
 * how generateGraph expands read cliques (src/graph.cpp:310-352).  Two-call
 * pattern: uv_pairs==NULL returns the number of raw pairs; otherwise fills
 * uv_pairs[2*n_raw] (must be the size the first call returned). */
int64_t komb_gen_hug_edges(int64_t nv, int64_t n_cliques, double alpha,
                           uint64_t seed, int64_t *uv_pairs);

#ifdef __cplusplus
}
#endif
#endif /* KOMB_ACCEL_H */
