/*
 * komb_oracle.h -- CPU restatement of KOMB's k-core / k-truss / CoreA hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under komb_amd/ (the product) may include,
 * link or call this; only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg use it, and only as the checker.
 *
 * Parity status:
 *   - CoreA half (rows a8-a11 of SURVEY.md section 8): PINNED.  The reference's
 *     own std-only header src/CoreA.h is compiled in place by oracle/Makefile
 *     into oracle/_ref/corea_ref and orc_corea_* is checked against it (and
 *     against the SURVEY App. D known-answer test) in tests/.
 *   - heap + runMerge (rows a12, a13): PINNED since round 3.  src/HashIndexedMinHeap.h is std-only and is
 *     compiled in place into oracle/_ref/merge_ref under a restatement of runMerge's loop (the loop itself needs
 *     <igraph.h>); orc_run_merge is checked against it on random graphs and through tests/golden/.
 *   - igraph half (rows a1-a3, a5-a6): PARITY UNPINNED by the reference.  The
 *     arithmetic lives in igraph >= 0.10 (komb.yml:7, not vendored, absent
 *     from the image) and the reference holds no tests or golden vectors for
 *     it.  The restatement follows igraph's published algorithms
 *     (Batagelj-Zaversnik coreness; triangle-support + bucket peel trussness)
 *     at the reference's call sites, and is cross-checked against definitional
 *     brute-force checkers and networkx fixtures (tests/golden/).  Coreness,
 *     degree and trussness of a simple graph are unique integers, so any
 *     correct algorithm agrees bit for bit.
 */
#ifndef KOMB_ORACLE_H
#define KOMB_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* a1  igraph_simplify(multiple=true, loops=true)  -- call site src/graph.cpp:438.
 * uv = n_raw (u,v) pairs as produced by generateGraph (src/graph.cpp:379-389).
 * Writes rowptr[nv+1] and col[2*ne] (rows sorted ascending, symmetric, no
 * loops, no duplicates); col must have room for 2*n_raw entries.
 * Returns ne (undirected edge count, what src/graph.cpp:444 prints) or -1. */
int64_t orc_simplify(int64_t nv, int64_t n_raw, const int64_t *uv,
                     int64_t *rowptr, int32_t *col);

/* a2  igraph_degree(ALL, NO_LOOPS) on the simplified graph -- src/graph.cpp:462. */
void orc_degree(int64_t nv, const int64_t *rowptr, int32_t *degree);

/* a3  igraph_coreness(IGRAPH_ALL) -- src/graph.cpp:463; Batagelj-Zaversnik
 * bin-sort sweep.  Returns max coreness. */
int32_t orc_coreness(int64_t nv, const int64_t *rowptr, const int32_t *col,
                     int32_t *coreness);

/* a5  igraph_induced_subgraph_map -- src/graph.cpp:502.  vmask[v]!=0 selects
 * vertices.  invmap[new]=old (used at src/graph.cpp:531-532).  sub_col needs
 * room for rowptr[nv] entries, sub_rowptr / invmap for nv+1 / nv.
 * Returns number of selected vertices. */
int64_t orc_induced_subgraph(int64_t nv, const int64_t *rowptr, const int32_t *col,
                             const uint8_t *vmask, int64_t *sub_rowptr,
                             int32_t *sub_col, int32_t *invmap);

/* Canonical edge list of a symmetric CSR: edges (u<v) in lexicographic order.
 * eu/ev have room for ne = rowptr[nv]/2 entries.  Returns ne. */
int64_t orc_edge_list(int64_t nv, const int64_t *rowptr, const int32_t *col,
                      int32_t *eu, int32_t *ev);

/* Per-edge triangle count (the "support" igraph_trussness starts from),
 * canonical edge order.  Returns the number of triangles T. */
int64_t orc_support(int64_t nv, const int64_t *rowptr, const int32_t *col,
                    int32_t *support);

/* a6  igraph_trussness -- src/graph.cpp:508: triangle
 * support, then bucket peel; trussness = level + 2, triangle-free edge -> 2.
 * Canonical edge order.  Returns max trussness (2 if ne>0 and no triangles,
 * 0 if ne==0). */
int32_t orc_trussness(int64_t nv, const int64_t *rowptr, const int32_t *col,
                      int32_t *trussness);

/* a10  CoreA::fractionalRank -- src/CoreA.h:142-187.  Faithful restatement:
 * unique values sorted descending, two full passes per unique value (O(U*n)).
 * Unlike the reference it does not free its input.  rank_out[n]. */
void orc_fractional_rank_faithful(const double *scores, int64_t n, double *rank_out);

/* Same ranks by sort + run lengths (O(n log n)); bit-identical to the faithful
 * form because every rank is the exact half-integer (first+last)/2. */
void orc_fractional_rank_fast(const int64_t *keys, int64_t n, double *rank_out);

/* a9  CoreA::getAnomalyScore -- src/CoreA.h:109-140.
 * key_i = coreness_i*n + degree_i; score = |ln rank_deg - ln rank_key|.
 * faithful!=0 : int arithmetic for the key exactly as src/CoreA.h:122 (caller
 * must keep max_coreness*n + max_degree < 2^31) and the O(U*n) ranker.
 * faithful==0 : int64 keys and the fast ranker. */
void orc_corea_scores(const int32_t *degree, const int32_t *coreness, int64_t n,
                      int faithful, double *score);

/* a12 + a13  HashIndexedMinHeap (src/HashIndexedMinHeap.h:10-238) and its only user, the dead
 * CombineCoreA::runMerge (src/CombineCoreA.h:45-219): greedy densest-block peel over a row copy and a column
 * copy of the graph.  susp: per-node suspiciousness or NULL (then priorities are plain degrees).  order[2*nv] /
 * side[2*nv] are filled from the back as the reference fills `order` / `modes`; the first n_block (the return
 * value) entries are the densest block: its rows are the order[i] with side[i] == 0, its columns those with
 * side[i] == 1.  PINNED against the reference's own heap class compiled in place (oracle/_ref/merge_ref). */
int32_t orc_run_merge(int64_t nv, const int64_t *rowptr, const int32_t *col, const double *susp,
                      int32_t *order, int32_t *side, double *max_density);

/* a6 with every host core (OpenMP builds only: oracle/Makefile target `native`): a level-synchronous parallel peel;
 * the same values as orc_trussness.  nthreads <= 0: OpenMP's default. */
int32_t orc_trussness_omp(int64_t nv, const int64_t *rowptr, const int32_t *col,
                          int32_t *truss, int nthreads);

/* ---- references for the clique analyses and the (3,4)-nucleus decomposition (include/komb_accel.h has the definitions).
 * Each walks from a VERTEX over sorted-array intersections of the CSR rows: no canonical-edge roots, no bit matrices, no
 * pivots, no trussness -- nothing of the library's decomposition.  PINNED by tests/test_oracle_cliques.py against the Python
 * restatements under tests/, networkx and one recorded run. */

/* Clique census by plain ordered enumeration (a node at depth d is one d-clique; a candidate set of >= 20 vertices that is
 * itself a clique is closed by binomials, which is what lets K_70 through).  total[k_cap + 1]: total[k] = min(the k-cliques,
 * 2^64 - 1) for 2 <= k <= k_cap, entries 0 and 1 are 0; k_local != 0: local[nv] = the k_local-cliques through every vertex,
 * saturating alike.  *saturated = some entry is 2^64 - 1; *n_nodes = the cliques visited one by one.  Returns the size of the largest
 * clique (0 without an edge), -1 for bad arguments. */
int32_t orc_clique_census(int64_t nv, const int64_t *rowptr, const int32_t *col, int32_t k_cap, int32_t k_local,
                          uint64_t *total, uint64_t *local, int32_t *saturated, uint64_t *n_nodes);

/* Maximal cliques, pivot-free: the same enumeration carrying the intersection of the members' full neighbourhoods; a clique
 * is maximal when that is empty.  hist[k_cap + 1]: hist[k] = the maximal cliques of k >= 2 vertices (every size, whatever
 * k_min); count[nv], largest[nv], *omega and the list cover those of >= k_min vertices.  The list (only with both pointers
 * given) is malloc'ed here and the caller's to orc_free: clique i is verts[offset[i] .. offset[i + 1]), ascending, the
 * cliques in lexicographic order.  Returns the cliques of >= k_min vertices, -1 for bad arguments or a clique above k_cap. */
int64_t orc_maximal_cliques(int64_t nv, const int64_t *rowptr, const int32_t *col, int32_t k_min, int32_t k_cap,
                            int64_t *hist, int32_t *count, int32_t *largest, int32_t *omega, uint64_t *n_nodes,
                            int64_t **offset_out, int32_t **verts_out, int64_t *n_verts);
void orc_free(void *p);

/* (3,4)-nucleus decomposition.  orc_nucleus_count returns the triangles and writes the 4-cliques; orc_nucleus, given both,
 * fills a, b, c, key0, theta [n_triangles] (triangles in ascending (a, b, c) order), edge_theta [ne] (canonical order, -1
 * without a triangle), vertex_theta [nv] and quads [4 * n_cliques4]: clique a < b < c < d as the triangle ids of (a,b,c),
 * (a,b,d), (a,c,d), (b,c,d), the cliques in (triangle (a,b,c), d) order.  theta by a sequential bucket peel.  Returns the
 * largest theta, -1 without a triangle, -2 when the counts given are not the graph's. */
int64_t orc_nucleus_count(int64_t nv, const int64_t *rowptr, const int32_t *col, int64_t *n_cliques4);
int32_t orc_nucleus(int64_t nv, const int64_t *rowptr, const int32_t *col, int64_t n_triangles, int64_t n_cliques4,
                    int32_t *a, int32_t *b, int32_t *c, int32_t *key0, int32_t *theta,
                    int32_t *edge_theta, int32_t *vertex_theta, int32_t *quads);

/* ---- references for the distance analysis, the betweenness centrality and the graphlet census (include/komb_accel.h has the
 * definitions).  One queue BFS per list entry from a VERTEX over the sorted CSR rows, one source at a time: no bit-parallel
 * masks, no 64-source batches, no (d, id) order, no hash tables, no canonical-edge roots.  The floating-point results follow
 * the operation order of the definitions with every operation rounded on its own (the build sets -ffp-contract=off).  PINNED
 * by tests/test_oracle_traversals.py against the Python restatements under tests/ and the stored fixtures, bit for bit. */

/* komb_distances_run without its info: per list entry src_reached, src_sum, src_ecc [n_sources]; per vertex n_reached,
 * sum_dist, ecc (-1 where no source reaches it) and harmonic [nv]; pairs [nv] (pairs[L] = the (entry, vertex) pairs at
 * distance L; a distance is below nv).  harmonic[v] literally: per block of 64 consecutive entries the distances of the
 * block's sources are kept, every vertex counts them level by level and adds (double)c / (double)L in ascending L to the
 * block's partial sum; the partial sums are added in block order.  Returns the largest distance, -1 for bad arguments. */
int32_t orc_bfs_sources(int64_t nv, const int64_t *rowptr, const int32_t *col, int64_t n_sources, const int32_t *sources,
                        int64_t *src_reached, int64_t *src_sum, int32_t *src_ecc,
                        int64_t *n_reached, int64_t *sum_dist, int32_t *ecc, double *harmonic, int64_t *pairs);

/* komb_betweenness_run: Brandes from the listed sources in the order given -- sigma[w] summed over w's row in ascending id,
 * delta[v] summed over v's row in ascending id with the division, the product and the addition rounded one after the other,
 * bc [nv] summed over the sources in list order without the source itself.  src_* [n_sources] as above; *flags has bit 0
 * when a sigma reached 2^53.  Returns 0, -1 for bad arguments, -2 when a sigma reached +inf (the outputs then mean nothing). */
int32_t orc_betweenness(int64_t nv, const int64_t *rowptr, const int32_t *col, int64_t n_sources, const int32_t *sources,
                        double *bc, int64_t *src_reached, int64_t *src_sum, int32_t *src_ecc, int32_t *flags);

/* komb_graphlets_run on the graph given: orbit [15 * nv] orbit-major, cycles4, cliques4 and (unless NULL) sup [ne] in
 * canonical edge order.  4-cycles per edge (u, v) from a dense p[y] = |N(u) & N(y)| filled by walking N(x) for x in N(u):
 * the sum over y in N(v) without u of p[y] - 1; 4-cliques per edge by intersecting sorted rows inside the common
 * neighbourhood; the orbits by the closed forms of tests/graphlets_ref.py census().  Unsigned 64-bit arithmetic.  Returns 0,
 * -1 for bad arguments, -2 when a per-vertex sum that must divide does not. */
int32_t orc_graphlets(int64_t nv, const int64_t *rowptr, const int32_t *col, uint64_t *orbit, uint64_t *cycles4, uint64_t *cliques4,
                      int64_t *sup);

/* The orbit vector out[15] of ONE vertex straight from the definition: every connected set of three and of four vertices
 * that holds v is formed once (they lie within three hops) and classified by its edges and the degrees inside it.  Returns
 * the number of vertices within three hops of v; with ball_limit > 0 and more than that many, -1 and out is left alone
 * (the sets of a vertex near a hub are too many to list).  -2 for bad arguments. */
int64_t orc_orbits_by_definition(int64_t nv, const int64_t *rowptr, const int32_t *col, int32_t v, int64_t ball_limit, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif
