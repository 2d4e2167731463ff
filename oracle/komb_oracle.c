/*
 * komb_oracle.c -- CPU restatement (plain C, single thread) of KOMB's
 * k-core / k-truss / CoreA hot path.  TEST INFRASTRUCTURE ONLY: see the
 * header for who may use it and for the parity status ("parity unpinned" for
 * the igraph half, pinned by oracle/_ref/corea_ref for the CoreA half).
 *
 * Every function names the reference call site (file:line under
 * /root/reference) whose observable result it restates.
 */
#include "komb_oracle.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------ utils */

static void radix_sort_u64(uint64_t *a, uint64_t *tmp, int64_t n)
{
    /* LSD radix sort, 16-bit digits, skips digits that are constant. */
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = pass * 16;
        int64_t *cnt = (int64_t *)calloc(65537, sizeof(int64_t));
        for (int64_t i = 0; i < n; ++i) cnt[((a[i] >> shift) & 0xFFFF) + 1]++;
        int trivial = 0;
        for (int d = 0; d < 65536; ++d)
            if (cnt[d + 1] == n) { trivial = 1; break; }
        if (!trivial) {
            for (int d = 0; d < 65536; ++d) cnt[d + 1] += cnt[d];
            for (int64_t i = 0; i < n; ++i) tmp[cnt[(a[i] >> shift) & 0xFFFF]++] = a[i];
            memcpy(a, tmp, (size_t)n * sizeof(uint64_t));
        }
        free(cnt);
    }
}

/* position of x in the ascending range col[lo,hi), or -1 */
static inline int64_t find_sorted(const int32_t *col, int64_t lo, int64_t hi, int32_t x)
{
    while (lo < hi) {
        int64_t mid = lo + ((hi - lo) >> 1);
        int32_t c = col[mid];
        if (c < x) lo = mid + 1;
        else if (c > x) hi = mid;
        else return mid;
    }
    return -1;
}

/* --------------------------------------------------------------- a1 simplify
 * Reference: igraph_simplify(&graph, true, true, NULL) at src/graph.cpp:438 on
 * the graph igraph_create()d (src/graph.cpp:418) from the raw clique-expanded
 * pairs (src/graph.cpp:379-389).  Observable result: a simple undirected graph
 * on the same nv vertices; |E| printed at src/graph.cpp:444. */
int64_t orc_simplify(int64_t nv, int64_t n_raw, const int64_t *uv,
                     int64_t *rowptr, int32_t *col)
{
    if (nv < 0 || n_raw < 0 || nv > INT32_MAX) return -1;
    uint64_t *keys = (uint64_t *)malloc((size_t)(n_raw > 0 ? n_raw : 1) * sizeof(uint64_t));
    uint64_t *tmp = (uint64_t *)malloc((size_t)(n_raw > 0 ? n_raw : 1) * sizeof(uint64_t));
    int64_t nk = 0;
    for (int64_t i = 0; i < n_raw; ++i) {
        int64_t u = uv[2 * i], v = uv[2 * i + 1];
        if (u < 0 || v < 0 || u >= nv || v >= nv) { free(keys); free(tmp); return -1; }
        if (u == v) continue;                         /* loops=true */
        uint64_t lo = (uint64_t)(u < v ? u : v), hi = (uint64_t)(u < v ? v : u);
        keys[nk++] = (lo << 32) | hi;
    }
    radix_sort_u64(keys, tmp, nk);
    int64_t ne = 0;
    for (int64_t i = 0; i < nk; ++i)                  /* multiple=true */
        if (i == 0 || keys[i] != keys[i - 1]) keys[ne++] = keys[i];

    memset(rowptr, 0, (size_t)(nv + 1) * sizeof(int64_t));
    for (int64_t i = 0; i < ne; ++i) {
        rowptr[(keys[i] >> 32) + 1]++;
        rowptr[(keys[i] & 0xFFFFFFFFu) + 1]++;
    }
    for (int64_t v = 0; v < nv; ++v) rowptr[v + 1] += rowptr[v];
    int64_t *cur = (int64_t *)malloc((size_t)(nv + 1) * sizeof(int64_t));
    memcpy(cur, rowptr, (size_t)(nv + 1) * sizeof(int64_t));
    /* lower neighbours first (ascending because keys are sorted by min), then
     * upper neighbours (ascending max within one min): rows come out sorted. */
    for (int64_t i = 0; i < ne; ++i) {
        int32_t lo = (int32_t)(keys[i] >> 32), hi = (int32_t)(keys[i] & 0xFFFFFFFFu);
        col[cur[hi]++] = lo;
    }
    for (int64_t i = 0; i < ne; ++i) {
        int32_t lo = (int32_t)(keys[i] >> 32), hi = (int32_t)(keys[i] & 0xFFFFFFFFu);
        col[cur[lo]++] = hi;
    }
    free(cur); free(keys); free(tmp);
    return ne;
}

/* ---------------------------------------------------------------- a2 degree
 * Reference: igraph_degree(&graph,&deg,igraph_vss_all(),IGRAPH_ALL,
 * IGRAPH_NO_LOOPS) at src/graph.cpp:462, after simplify: distinct neighbours. */
void orc_degree(int64_t nv, const int64_t *rowptr, int32_t *degree)
{
    for (int64_t v = 0; v < nv; ++v) degree[v] = (int32_t)(rowptr[v + 1] - rowptr[v]);
}

/* -------------------------------------------------------------- a3 coreness
 * Reference: igraph_coreness(&graph,&coreness,IGRAPH_ALL) at src/graph.cpp:463.
 * igraph implements Batagelj & Zaversnik (2003): bin-sort vertices by degree,
 * sweep in that order, and for every neighbour u of the swept vertex v with
 * cores[u] > cores[v] move u one bin down (swap with the first vertex of its
 * bin) and decrement cores[u]. */
int32_t orc_coreness(int64_t nv, const int64_t *rowptr, const int32_t *col,
                     int32_t *cores)
{
    if (nv == 0) return 0;
    int32_t maxdeg = 0;
    for (int64_t v = 0; v < nv; ++v) {
        cores[v] = (int32_t)(rowptr[v + 1] - rowptr[v]);
        if (cores[v] > maxdeg) maxdeg = cores[v];
    }
    int64_t *bin = (int64_t *)calloc((size_t)maxdeg + 2, sizeof(int64_t));
    int64_t *pos = (int64_t *)malloc((size_t)nv * sizeof(int64_t));
    int32_t *vert = (int32_t *)malloc((size_t)nv * sizeof(int32_t));
    for (int64_t v = 0; v < nv; ++v) bin[cores[v]]++;
    int64_t start = 0;
    for (int32_t d = 0; d <= maxdeg; ++d) { int64_t c = bin[d]; bin[d] = start; start += c; }
    for (int64_t v = 0; v < nv; ++v) { pos[v] = bin[cores[v]]; vert[pos[v]] = (int32_t)v; bin[cores[v]]++; }
    for (int32_t d = maxdeg; d > 0; --d) bin[d] = bin[d - 1];
    bin[0] = 0;
    for (int64_t i = 0; i < nv; ++i) {
        int32_t v = vert[i];
        for (int64_t j = rowptr[v]; j < rowptr[v + 1]; ++j) {
            int32_t u = col[j];
            if (cores[u] > cores[v]) {
                int32_t du = cores[u];
                int64_t pu = pos[u], pw = bin[du];
                int32_t w = vert[pw];
                if (u != w) { pos[u] = pw; pos[w] = pu; vert[pu] = w; vert[pw] = u; }
                bin[du]++;
                cores[u]--;
            }
        }
    }
    int32_t mx = 0;
    for (int64_t v = 0; v < nv; ++v) if (cores[v] > mx) mx = cores[v];
    free(bin); free(pos); free(vert);
    return mx;
}

/* ------------------------------------------------------ a5 induced subgraph
 * Reference: igraph_induced_subgraph_map(&graph,&subgraph,vids,
 * IGRAPH_SUBGRAPH_AUTO,&map,&invmap) at src/graph.cpp:502; vids are the
 * max-coreness vertices collected in ascending vid order at
 * src/graph.cpp:468-473, so new ids keep the old relative order and
 * invmap[new] = old (read at src/graph.cpp:531-532). */
int64_t orc_induced_subgraph(int64_t nv, const int64_t *rowptr, const int32_t *col,
                             const uint8_t *vmask, int64_t *sub_rowptr,
                             int32_t *sub_col, int32_t *invmap)
{
    int32_t *map = (int32_t *)malloc((size_t)(nv > 0 ? nv : 1) * sizeof(int32_t));
    int64_t ns = 0;
    for (int64_t v = 0; v < nv; ++v) {
        if (vmask[v]) { map[v] = (int32_t)ns; invmap[ns] = (int32_t)v; ns++; }
        else map[v] = -1;
    }
    int64_t out = 0;
    sub_rowptr[0] = 0;
    for (int64_t s = 0; s < ns; ++s) {
        int32_t v = invmap[s];
        for (int64_t j = rowptr[v]; j < rowptr[v + 1]; ++j)
            if (map[col[j]] >= 0) sub_col[out++] = map[col[j]];
        sub_rowptr[s + 1] = out;
    }
    free(map);
    return ns;
}

/* ------------------------------------------------------- canonical edge ids
 * Edge identity across the C-ABI is the pair (min,max) in lexicographic
 * order; igraph's internal edge ids are never observable
 * in KOMB's outputs.  ebase[u] = id of u's first upper edge, ustart[u] = slot
 * of u's first neighbour > u. */
static void upper_index(int64_t nv, const int64_t *rowptr, const int32_t *col,
                        int64_t *ustart, int64_t *ebase)
{
    int64_t e = 0;
    for (int64_t u = 0; u < nv; ++u) {
        int64_t lo = rowptr[u], hi = rowptr[u + 1];
        while (lo < hi) {                       /* first slot with col > u */
            int64_t mid = lo + ((hi - lo) >> 1);
            if (col[mid] > (int32_t)u) hi = mid; else lo = mid + 1;
        }
        ustart[u] = lo;
        ebase[u] = e;
        e += rowptr[u + 1] - lo;
    }
    ebase[nv] = e;
}

int64_t orc_edge_list(int64_t nv, const int64_t *rowptr, const int32_t *col,
                      int32_t *eu, int32_t *ev)
{
    int64_t e = 0;
    for (int64_t u = 0; u < nv; ++u)
        for (int64_t j = rowptr[u]; j < rowptr[u + 1]; ++j)
            if (col[j] > (int32_t)u) { eu[e] = (int32_t)u; ev[e] = col[j]; e++; }
    return e;
}

/* slot -> canonical edge id for every one of the 2*ne CSR slots */
static int32_t *slot_edge_ids(int64_t nv, const int64_t *rowptr, const int32_t *col,
                              const int64_t *ustart, const int64_t *ebase)
{
    int64_t ns = rowptr[nv];
    int32_t *eid = (int32_t *)malloc((size_t)(ns > 0 ? ns : 1) * sizeof(int32_t));
    for (int64_t u = 0; u < nv; ++u) {
        for (int64_t j = rowptr[u]; j < rowptr[u + 1]; ++j) {
            int32_t x = col[j];
            if (x > (int32_t)u) eid[j] = (int32_t)(ebase[u] + (j - ustart[u]));
            else {
                int64_t p = find_sorted(col, ustart[x], rowptr[x + 1], (int32_t)u);
                eid[j] = (int32_t)(ebase[x] + (p - ustart[x]));
            }
        }
    }
    return eid;
}

/* For every common neighbour w of u and v call
 *   f(ctx, eid of (u,w), eid of (v,w)).
 * Iterates the shorter row and binary-searches the longer one (igraph's
 * sorted intersection switches to the same strategy for skewed sizes). */
typedef void (*tri_fn)(void *ctx, int32_t e1, int32_t e2);
static void for_common(const int64_t *rowptr, const int32_t *col, const int32_t *eid,
                       int32_t u, int32_t v, tri_fn f, void *ctx)
{
    int64_t du = rowptr[u + 1] - rowptr[u], dv = rowptr[v + 1] - rowptr[v];
    int32_t s = du <= dv ? u : v, l = du <= dv ? v : u;
    for (int64_t j = rowptr[s]; j < rowptr[s + 1]; ++j) {
        int32_t w = col[j];
        if (w == l) continue;
        int64_t p = find_sorted(col, rowptr[l], rowptr[l + 1], w);
        if (p >= 0) {
            if (s == u) f(ctx, eid[j], eid[p]); else f(ctx, eid[p], eid[j]);
        }
    }
}

/* ---------------------------------------------------------------- support
 * igraph_trussness (called at src/graph.cpp:508) starts by listing every
 * triangle and counting, per edge, the triangles through it.
 * Restated as: support[(u,v)] = |N(u) & N(v)|. */
struct cnt_ctx { int64_t n; };
static void cnt_cb(void *c, int32_t e1, int32_t e2) { (void)e1; (void)e2; ((struct cnt_ctx *)c)->n++; }

int64_t orc_support(int64_t nv, const int64_t *rowptr, const int32_t *col,
                    int32_t *support)
{
    int64_t *ustart = (int64_t *)malloc((size_t)(nv + 1) * sizeof(int64_t));
    int64_t *ebase = (int64_t *)malloc((size_t)(nv + 1) * sizeof(int64_t));
    upper_index(nv, rowptr, col, ustart, ebase);
    int32_t *eid = slot_edge_ids(nv, rowptr, col, ustart, ebase);
    int64_t tri3 = 0;
    for (int64_t u = 0; u < nv; ++u) {
        for (int64_t j = ustart[u]; j < rowptr[u + 1]; ++j) {
            struct cnt_ctx c = {0};
            for_common(rowptr, col, eid, (int32_t)u, col[j], cnt_cb, &c);
            support[eid[j]] = (int32_t)c.n;
            tri3 += c.n;
        }
    }
    free(ustart); free(ebase); free(eid);
    return tri3 / 3;
}

/* -------------------------------------------------------------- a6 trussness
 * Reference: igraph_trussness(&subgraph,&trussness) at src/graph.cpp:508.
 * igraph: support per edge; buckets of edges by support; for level = 0..max,
 * while the level's bucket is non-empty take an edge (a,b), and for every
 * common neighbour n whose two edges (a,n),(b,n) are both not yet completed,
 * move each of them that has support > level one bucket down; then
 * trussness[(a,b)] = level + 2 and the edge is completed.
 * Restated with the bin-sorted array + position index of Batagelj-Zaversnik
 * applied to edges (same peel order class, same results; the result is the
 * unique trussness of a simple graph). */
struct peel_ctx {
    int32_t *sup; uint8_t *done; int64_t *bin; int64_t *pos; int32_t *ord; int32_t k;
};
static inline void peel_lower(struct peel_ctx *p, int32_t e)
{
    if (p->sup[e] > p->k) {
        int32_t s = p->sup[e];
        int64_t pe = p->pos[e], pw = p->bin[s];
        int32_t w = p->ord[pw];
        if (e != w) { p->pos[e] = pw; p->pos[w] = pe; p->ord[pe] = w; p->ord[pw] = e; }
        p->bin[s]++;
        p->sup[e]--;
    }
}
static void peel_cb(void *c, int32_t e1, int32_t e2)
{
    struct peel_ctx *p = (struct peel_ctx *)c;
    if (p->done[e1] || p->done[e2]) return;
    peel_lower(p, e1);
    peel_lower(p, e2);
}

int32_t orc_trussness(int64_t nv, const int64_t *rowptr, const int32_t *col,
                      int32_t *truss)
{
    int64_t ne = rowptr[nv] / 2;
    if (ne == 0) return 0;
    int64_t *ustart = (int64_t *)malloc((size_t)(nv + 1) * sizeof(int64_t));
    int64_t *ebase = (int64_t *)malloc((size_t)(nv + 1) * sizeof(int64_t));
    upper_index(nv, rowptr, col, ustart, ebase);
    int32_t *eid = slot_edge_ids(nv, rowptr, col, ustart, ebase);
    int32_t *eu = (int32_t *)malloc((size_t)ne * sizeof(int32_t));
    int32_t *ev = (int32_t *)malloc((size_t)ne * sizeof(int32_t));
    orc_edge_list(nv, rowptr, col, eu, ev);

    int32_t *sup = (int32_t *)malloc((size_t)ne * sizeof(int32_t));
    int32_t maxs = 0;
    for (int64_t e = 0; e < ne; ++e) {
        struct cnt_ctx c = {0};
        for_common(rowptr, col, eid, eu[e], ev[e], cnt_cb, &c);
        sup[e] = (int32_t)c.n;
        if (sup[e] > maxs) maxs = sup[e];
    }
    int64_t *bin = (int64_t *)calloc((size_t)maxs + 2, sizeof(int64_t));
    int64_t *pos = (int64_t *)malloc((size_t)ne * sizeof(int64_t));
    int32_t *ord = (int32_t *)malloc((size_t)ne * sizeof(int32_t));
    uint8_t *done = (uint8_t *)calloc((size_t)ne, 1);
    for (int64_t e = 0; e < ne; ++e) bin[sup[e]]++;
    int64_t start = 0;
    for (int32_t s = 0; s <= maxs; ++s) { int64_t c = bin[s]; bin[s] = start; start += c; }
    for (int64_t e = 0; e < ne; ++e) { pos[e] = bin[sup[e]]; ord[pos[e]] = (int32_t)e; bin[sup[e]]++; }
    for (int32_t s = maxs; s > 0; --s) bin[s] = bin[s - 1];
    bin[0] = 0;

    struct peel_ctx p = { sup, done, bin, pos, ord, 0 };
    int32_t mx = 0;
    for (int64_t i = 0; i < ne; ++i) {
        int32_t e = ord[i];
        p.k = sup[e];
        truss[e] = p.k + 2;
        if (truss[e] > mx) mx = truss[e];
        if (p.k > 0) for_common(rowptr, col, eid, eu[e], ev[e], peel_cb, &p);
        done[e] = 1;
    }
    free(ustart); free(ebase); free(eid); free(eu); free(ev);
    free(sup); free(bin); free(pos); free(ord); free(done);
    return mx;
}

/* ------------------------------------------------- a6, all-cores variant
 * The same trussness with every host core: supports by a parallel loop over the
 * edges, then a level-synchronous parallel peel in the manner of Kabir & Madduri's
 * PKT (2017): level l's edges form the current set; every thread takes edges of
 * the set, and a triangle whose other two edges are both unprocessed loses one
 * support on each edge that is above the level -- on one edge only, by the smaller
 * edge id, when the other one is in the current set too; an edge that lands on the
 * level joins the next set.  Trussness is unique, so the values equal
 * orc_trussness's (tests/test_oracle.py).  This is NOT how the reference runs
 * (igraph is single-threaded, src/graph.cpp:508 is called from one thread): it
 * is the "fairer CPU ceiling" of SURVEY section 8(d), reported next to the
 * single-thread figure.  Built only with OpenMP (oracle/Makefile target native). */
#ifdef _OPENMP
#include <omp.h>
struct pkt_ctx { int32_t *S; const uint8_t *processed; const uint8_t *in_curr; int32_t *next; int64_t *next_n; uint8_t *in_next; int32_t e, l; };
static inline void pkt_dec(struct pkt_ctx *p, int32_t x)
{
    int32_t old = __atomic_fetch_sub(&p->S[x], 1, __ATOMIC_RELAXED);
    if (old == p->l + 1) { int64_t i = __atomic_fetch_add(p->next_n, 1, __ATOMIC_RELAXED); p->next[i] = x; p->in_next[x] = 1; }
    else if (old <= p->l) __atomic_fetch_add(&p->S[x], 1, __ATOMIC_RELAXED);       /* it was on the level already */
}
static void pkt_cb(void *c, int32_t e1, int32_t e2)
{
    struct pkt_ctx *p = (struct pkt_ctx *)c;
    if (p->processed[e1] || p->processed[e2]) return;
    const int32_t s1 = __atomic_load_n(&p->S[e1], __ATOMIC_RELAXED), s2 = __atomic_load_n(&p->S[e2], __ATOMIC_RELAXED);
    if (s1 > p->l && s2 > p->l) { pkt_dec(p, e1); pkt_dec(p, e2); }
    else if (s1 > p->l) { if (!p->in_curr[e2] || p->e < e2) pkt_dec(p, e1); }
    else if (s2 > p->l) { if (!p->in_curr[e1] || p->e < e1) pkt_dec(p, e2); }
}
int32_t orc_trussness_omp(int64_t nv, const int64_t *rowptr, const int32_t *col, int32_t *truss, int nthreads)
{
    int64_t ne = rowptr[nv] / 2;
    if (ne == 0) return 0;
    if (nthreads > 0) omp_set_num_threads(nthreads);
    int64_t *ustart = (int64_t *)malloc((size_t)(nv + 1) * sizeof(int64_t));
    int64_t *ebase = (int64_t *)malloc((size_t)(nv + 1) * sizeof(int64_t));
    upper_index(nv, rowptr, col, ustart, ebase);
    int32_t *eid = slot_edge_ids(nv, rowptr, col, ustart, ebase);
    int32_t *eu = (int32_t *)malloc((size_t)ne * sizeof(int32_t));
    int32_t *ev = (int32_t *)malloc((size_t)ne * sizeof(int32_t));
    orc_edge_list(nv, rowptr, col, eu, ev);
    int32_t *S = (int32_t *)malloc((size_t)ne * sizeof(int32_t));
    uint8_t *processed = (uint8_t *)calloc((size_t)ne, 1), *in_curr = (uint8_t *)calloc((size_t)ne, 1), *in_next = (uint8_t *)calloc((size_t)ne, 1);
    int32_t *curr = (int32_t *)malloc((size_t)ne * sizeof(int32_t)), *next = (int32_t *)malloc((size_t)ne * sizeof(int32_t));
#pragma omp parallel for schedule(dynamic, 4096)
    for (int64_t e = 0; e < ne; ++e) {
        struct cnt_ctx c = {0};
        for_common(rowptr, col, eid, eu[e], ev[e], cnt_cb, &c);
        S[e] = (int32_t)c.n;
    }
    int64_t todo = ne;
    int32_t mx = 0;
    for (int32_t l = 0; todo > 0; ++l) {
        int64_t curr_n = 0;
#pragma omp parallel for schedule(static)
        for (int64_t e = 0; e < ne; ++e)
            if (!processed[e] && S[e] == l) { int64_t i = __atomic_fetch_add(&curr_n, 1, __ATOMIC_RELAXED); curr[i] = (int32_t)e; in_curr[e] = 1; }
        while (curr_n > 0) {
            todo -= curr_n;
            mx = l + 2;
            int64_t next_n = 0;
#pragma omp parallel for schedule(dynamic, 64)
            for (int64_t i = 0; i < curr_n; ++i) {
                struct pkt_ctx p = { S, processed, in_curr, next, &next_n, in_next, curr[i], l };
                if (l > 0) for_common(rowptr, col, eid, eu[p.e], ev[p.e], pkt_cb, &p);
            }
#pragma omp parallel for schedule(static)
            for (int64_t i = 0; i < curr_n; ++i) { const int32_t e = curr[i]; processed[e] = 1; in_curr[e] = 0; truss[e] = l + 2; }
            int32_t *t = curr; curr = next; next = t;
            uint8_t *tf = in_curr; in_curr = in_next; in_next = tf;
            curr_n = next_n;
        }
    }
    free(ustart); free(ebase); free(eid); free(eu); free(ev); free(S); free(processed); free(in_curr); free(in_next); free(curr); free(next);
    return mx;
}
#endif

/* ------------------------------------------------------ a10 fractionalRank
 * Reference: CoreA::fractionalRank, src/CoreA.h:142-187.  Scores truncated to
 * int (:149), sorted descending (:152), uniqued (:154); then for every unique
 * value one pass that advances an int rank counter over the matching entries
 * and sums the ranks in a double (:164-172), avg /= cnt (:174), and a second
 * pass that assigns avg (:176-182). */
static int cmp_int_desc(const void *a, const void *b)
{
    int x = *(const int *)a, y = *(const int *)b;
    return (x < y) - (x > y);
}
void orc_fractional_rank_faithful(const double *scores, int64_t n, double *out)
{
    int *list = (int *)malloc((size_t)(n > 0 ? n : 1) * sizeof(int));
    for (int64_t i = 0; i < n; ++i) list[i] = (int)scores[i];
    qsort(list, (size_t)n, sizeof(int), cmp_int_desc);
    int64_t nu = 0;
    for (int64_t i = 0; i < n; ++i)
        if (i == 0 || list[i] != list[i - 1]) list[nu++] = list[i];
    int rank = 0;
    for (int64_t t = 0; t < nu; ++t) {
        int value = list[t];
        double avg = 0.0;
        int cnt = 0;
        for (int64_t i = 0; i < n; ++i)
            if (scores[i] == value) { rank++; cnt++; avg += rank; }
        avg /= cnt;
        for (int64_t i = 0; i < n; ++i)
            if (scores[i] == value) out[i] = avg;
    }
    free(list);
}

struct kv { int64_t key; int64_t idx; };
static int cmp_kv_desc(const void *a, const void *b)
{
    const struct kv *x = (const struct kv *)a, *y = (const struct kv *)b;
    return (x->key < y->key) - (x->key > y->key);
}
void orc_fractional_rank_fast(const int64_t *keys, int64_t n, double *out)
{
    struct kv *a = (struct kv *)malloc((size_t)(n > 0 ? n : 1) * sizeof(struct kv));
    for (int64_t i = 0; i < n; ++i) { a[i].key = keys[i]; a[i].idx = i; }
    qsort(a, (size_t)n, sizeof(struct kv), cmp_kv_desc);
    int64_t i = 0;
    while (i < n) {
        int64_t j = i;
        while (j + 1 < n && a[j + 1].key == a[i].key) ++j;
        /* positions i+1 .. j+1 (1-based): mean = (first+last)/2, exact */
        double avg = (double)((i + 1) + (j + 1)) / 2.0;
        for (int64_t t = i; t <= j; ++t) out[a[t].idx] = avg;
        i = j + 1;
    }
    free(a);
}

/* ------------------------------------------------------ a9 getAnomalyScore
 * Reference: CoreA::getAnomalyScore, src/CoreA.h:109-140:
 *   corenessWithDegree[i] = coreness[i] * n + degree[i]   (int arithmetic, :122)
 *   anomaly[i] = |log(degreeRank[i]) - log(corenessRank[i])|            (:131) */
void orc_corea_scores(const int32_t *degree, const int32_t *coreness, int64_t n,
                      int faithful, double *score)
{
    double *rd = (double *)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
    double *rc = (double *)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
    if (faithful) {
        double *kd = (double *)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
        double *kc = (double *)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
        int ni = (int)n;
        for (int64_t i = 0; i < n; ++i) {
            kd[i] = degree[i];
            kc[i] = coreness[i] * ni + degree[i];      /* int, as src/CoreA.h:122 */
        }
        orc_fractional_rank_faithful(kc, n, rc);
        orc_fractional_rank_faithful(kd, n, rd);
        free(kd); free(kc);
    } else {
        int64_t *kd = (int64_t *)malloc((size_t)(n > 0 ? n : 1) * sizeof(int64_t));
        int64_t *kc = (int64_t *)malloc((size_t)(n > 0 ? n : 1) * sizeof(int64_t));
        for (int64_t i = 0; i < n; ++i) {
            kd[i] = degree[i];
            kc[i] = (int64_t)coreness[i] * n + degree[i];
        }
        orc_fractional_rank_fast(kc, n, rc);
        orc_fractional_rank_fast(kd, n, rd);
        free(kd); free(kc);
    }
    for (int64_t i = 0; i < n; ++i) score[i] = fabs(log(rd[i]) - log(rc[i]));
    free(rd); free(rc);
}

/* ------------------------------------------- a12 + a13 HashIndexedMinHeap, runMerge
 * Reference: src/HashIndexedMinHeap.h:10-238 (array-backed binary min-heap over int ids with a position index:
 * insert = append + refreshPriority; poll = move the last id to the root + sift down; refreshPriority = sift down,
 * and only if nothing moved, sift up while the parent's value is GREATER) and its only user,
 * CombineCoreA::runMerge, src/CombineCoreA.h:45-219 (dead code in the reference: no caller): a greedy
 * densest-block peel over a "row" copy and a "column" copy of the graph.  Every node starts on both sides with
 * priority = suspiciousness + degree; each step polls the smaller of the two heap minima (the row side only when
 * strictly smaller, or the column side is empty), subtracts its priority from the running sum, records
 * density = sum / nodes left, and lowers by one the priority of the node's neighbours on the OTHER side that are
 * still there.  Output: removal order and sides (filled from the back, as :137-138), the number of nodes of the
 * densest block and its density (:140-145).  Which of several equal priorities is polled first is decided by
 * the heap's array layout, so the heap is restated operation for operation; tests/ pin this against the
 * reference's own class compiled in place (oracle/_ref/merge_ref).  removed[][] is zero-initialised (the
 * reference reads it uninitialised, :104-108), and the reference's `cols` vector sized by the number of rows
 * (:191) is not modelled: rows / cols of the block are order[i] for i < n_block with side[i] == 0 / 1. */
struct mheap { int32_t *arr; int32_t *pos; double *val; int32_t size; };
static int mh_down(struct mheap *h, int32_t p)                /* minHeapfy, :171-217 (iterative; same moves) */
{
    int moved = 0;
    for (;;) {
        const int32_t l = 2 * (p + 1) - 1, r = 2 * (p + 1);
        const int32_t cur = h->arr[p];
        int32_t sp = p, sk = cur;
        if (l < h->size && h->val[h->arr[l]] < h->val[cur]) { sp = l; sk = h->arr[l]; }
        if (r < h->size && h->val[h->arr[r]] < h->val[sk]) { sp = r; sk = h->arr[r]; }
        if (sp == p) return moved;
        h->arr[p] = sk; h->pos[sk] = p;
        h->arr[sp] = cur; h->pos[cur] = sp;
        p = sp; moved = 1;
    }
}
static void mh_refresh(struct mheap *h, int32_t key, double v)   /* refreshPriority, :138-167 */
{
    h->val[key] = v;
    int32_t p = h->pos[key];
    if (mh_down(h, p) || p <= 0) return;
    int32_t pp = (p + 1) / 2 - 1;
    while (p > 0 && h->val[h->arr[pp]] > h->val[key]) {
        const int32_t pe = h->arr[pp];
        h->arr[pp] = key; h->pos[key] = pp;
        h->arr[p] = pe; h->pos[pe] = p;
        p = pp; pp = (p + 1) / 2 - 1;
    }
}
static void mh_insert(struct mheap *h, int32_t key, double v)    /* insert, :83-98 */
{
    const int32_t p = h->size++;
    h->arr[p] = key; h->pos[key] = p; h->val[key] = v;
    mh_refresh(h, key, v);
}
static int32_t mh_poll(struct mheap *h, double *v)               /* poll, :55-81 (size > 0) */
{
    const int32_t top = h->arr[0];
    *v = h->val[top];
    h->pos[top] = -1;
    if (h->size != 1) {
        const int32_t last = h->arr[h->size - 1];
        h->arr[0] = last; h->pos[last] = 0;
        h->size--;
        mh_down(h, 0);
    } else h->size--;
    h->arr[h->size] = 0;
    return top;
}
int32_t orc_run_merge(int64_t nv, const int64_t *rowptr, const int32_t *col, const double *susp,
                      int32_t *order, int32_t *side, double *max_density)
{
    const int32_t n = (int32_t)nv;
    struct mheap h[2];
    for (int s = 0; s < 2; ++s) {
        h[s].arr = (int32_t *)malloc((size_t)(n > 0 ? n : 1) * sizeof(int32_t));
        h[s].pos = (int32_t *)malloc((size_t)(n > 0 ? n : 1) * sizeof(int32_t));
        h[s].val = (double *)calloc((size_t)(n > 0 ? n : 1), sizeof(double));
        h[s].size = 0;
        for (int32_t v = 0; v < n; ++v) h[s].pos[v] = -1;
    }
    double *p0 = (double *)calloc((size_t)(n > 0 ? n : 1), sizeof(double)), *p1 = (double *)calloc((size_t)(n > 0 ? n : 1), sizeof(double));
    double sum = 0;
    if (susp) for (int32_t v = 0; v < n; ++v) { p0[v] = susp[v]; p1[v] = susp[v]; sum += 2 * susp[v]; }   /* :58-67 */
    long slots = 0;
    for (int32_t v = 0; v < n; ++v)                                                                       /* :71-85 */
        for (int64_t j = rowptr[v]; j < rowptr[v + 1]; ++j) { p0[v] += 1; p1[col[j]] += 1; ++slots; }
    sum += (double)slots;                                                                                   /* :87 */
    for (int32_t v = 0; v < n; ++v) mh_insert(&h[0], v, p0[v]);                                            /* :89-93 */
    for (int32_t v = 0; v < n; ++v) mh_insert(&h[1], v, p1[v]);                                            /* :95-99 */
    uint8_t *gone = (uint8_t *)calloc((size_t)2 * (size_t)(n > 0 ? n : 1), 1);
    double best = 0;
    int32_t best_left = 0;
    for (int32_t left = 2 * n; left >= 1;) {                                                                /* :114-174 */
        const int s = (h[0].size > 0 && (h[1].size == 0 || h[0].val[h[0].arr[0]] < h[1].val[h[1].arr[0]])) ? 0 : 1;
        double pv;
        const int32_t node = mh_poll(&h[s], &pv);
        sum -= pv;
        --left;
        order[left] = node; side[left] = s;
        if (left >= 1) { const double d = sum / left; if (d > best) { best = d; best_left = left; } }
        gone[(size_t)s * (size_t)(n > 0 ? n : 1) + node] = 1;
        struct mheap *o = &h[s ^ 1];
        for (int64_t j = rowptr[node]; j < rowptr[node + 1]; ++j) {
            const int32_t w = col[j];
            if (!gone[(size_t)(s ^ 1) * (size_t)(n > 0 ? n : 1) + w]) mh_refresh(o, w, o->val[w] - 1);
        }
    }
    for (int s = 0; s < 2; ++s) { free(h[s].arr); free(h[s].pos); free(h[s].val); }
    free(p0); free(p1); free(gone);
    if (max_density) *max_density = best;
    return best_left;
}

/* ============================================================ cliques and nuclei
 * References for the analyses that walk cliques on the GPU (the clique census, the maximal cliques and, through them, the
 * maximum cliques) and for the (3,4)-nucleus decomposition.  They restate DEFINITIONS (include/komb_accel.h), not the
 * library's decomposition: the walks start at a VERTEX, not at a canonical edge; every set is a sorted array and every step a
 * sorted-array intersection over the CSR rows; there is no bit matrix, no pivot and no trussness anywhere (t_max, which only
 * sizes the library's windows, comes from orc_trussness in oracle.py).  tests/test_oracle_cliques.py ties them to the Python
 * restatements, to networkx and to one recorded run. */

struct arena { int32_t *p; int64_t cap; };
static void arena_need(struct arena *A, int64_t n)
{
    if (n <= A->cap) return;
    int64_t cap = A->cap ? A->cap : 1024;
    while (cap < n) cap *= 2;
    A->p = (int32_t *)realloc(A->p, (size_t)cap * sizeof(int32_t));
    A->cap = cap;
}

/* out = a & b, both ascending; the shorter one is walked, the longer one bisected when it is much longer, else merged */
static int32_t isect(const int32_t *a, int64_t na, const int32_t *b, int64_t nb, int32_t *out)
{
    if (na > nb) { const int32_t *t = a; a = b; b = t; int64_t tn = na; na = nb; nb = tn; }
    int32_t n = 0;
    if (na * 4 < nb) {
        int64_t lo = 0;
        for (int64_t i = 0; i < na && lo < nb; ++i) {
            int64_t l = lo, h = nb;
            while (l < h) { int64_t mid = l + ((h - l) >> 1); if (b[mid] < a[i]) l = mid + 1; else h = mid; }
            lo = l;
            if (l < nb && b[l] == a[i]) { out[n++] = a[i]; lo = l + 1; }
        }
        return n;
    }
    int64_t i = 0, j = 0;
    while (i < na && j < nb) {
        if (a[i] < b[j]) ++i;
        else if (a[i] > b[j]) ++j;
        else { out[n++] = a[i]; ++i; ++j; }
    }
    return n;
}

static inline uint64_t sat_add(uint64_t a, uint64_t b) { const uint64_t s = a + b; return s < a ? UINT64_MAX : s; }

/* row[j] = min(C(n, j), 2^64 - 1), j = 0 .. n: Pascal's rule with saturating adds (adds of non-negative numbers, so exact) */
static void binom_row(int32_t n, uint64_t *row)
{
    row[0] = 1;
    for (int32_t j = 1; j <= n; ++j) row[j] = 0;
    for (int32_t i = 1; i <= n; ++i)
        for (int32_t j = i; j >= 1; --j) row[j] = sat_add(row[j], row[j - 1]);
}

static int32_t max_upper_degree(int64_t nv, const int64_t *rowptr, const int64_t *ustart)
{
    int64_t mx = 0;
    for (int64_t v = 0; v < nv; ++v) if (rowptr[v + 1] - ustart[v] > mx) mx = rowptr[v + 1] - ustart[v];
    return (int32_t)mx;
}

/* ---------------------------------------------------------------- clique census
 * Definition: total[k] = the k-cliques, local[v] = the k_local-cliques through v (include/komb_accel.h, "clique census").
 * Plain ordered enumeration: a clique is visited once, as its ascending tuple; the node of the tuple (v_1 .. v_d) holds
 * P = the common neighbours above v_d and has one child per member of P.  Every node at depth d is one d-clique.
 * One exception, for inputs like K_70 whose 2^70 cliques nothing enumerates: a node whose P has ORC_CLOSED_FROM or more
 * vertices and is itself a clique is closed by binomials (the tuples below it are the subsets of P).  The graphs the
 * mid-size tests use have omega <= 16, so there every clique is visited, and *n_nodes (the cliques visited) says so: it
 * equals the sum of the totals exactly when nothing was closed. */
#define ORC_CLOSED_FROM 20

struct cc {
    const int64_t *rowptr, *ustart; const int32_t *col;
    int32_t k_cap, k_local, omega;
    uint64_t *total, *local, *row, *row1, nodes;
    int32_t *held;
    struct arena A;
};

static int cc_complete(struct cc *C, int64_t off, int32_t p)
{
    for (int32_t i = 0; i + 1 < p; ++i) {
        const int32_t x = C->A.p[off + i];
        if (isect(C->A.p + off + i + 1, p - i - 1, C->col + C->ustart[x], C->rowptr[x + 1] - C->ustart[x], C->A.p + off + p) != p - i - 1) return 0;
    }
    return 1;
}

static void cc_node(struct cc *C, int32_t d, int64_t off, int32_t p)
{
    if (d >= 2) {
        C->nodes++;
        if (d <= C->k_cap) C->total[d] = sat_add(C->total[d], 1);
        if (d > C->omega) C->omega = d;
        if (d == C->k_local) for (int32_t i = 0; i < d; ++i) C->local[C->held[i]] = sat_add(C->local[C->held[i]], 1);
    }
    if (p == 0) return;
    arena_need(&C->A, off + 2 * (int64_t)p);
    if (p >= ORC_CLOSED_FROM && cc_complete(C, off, p)) {
        binom_row(p - 1, C->row1);
        binom_row(p, C->row);
        for (int32_t j = 1; j <= p; ++j) if (d + j <= C->k_cap) C->total[d + j] = sat_add(C->total[d + j], C->row[j]);
        if (d + p > C->omega) C->omega = d + p;
        const int32_t j = C->k_local - d;
        if (C->k_local && j >= 1 && j <= p) {
            for (int32_t i = 0; i < d; ++i) C->local[C->held[i]] = sat_add(C->local[C->held[i]], C->row[j]);
            for (int32_t i = 0; i < p; ++i) C->local[C->A.p[off + i]] = sat_add(C->local[C->A.p[off + i]], C->row1[j - 1]);
        }
        return;
    }
    for (int32_t i = 0; i < p; ++i) {
        const int32_t x = C->A.p[off + i];
        const int32_t n = isect(C->A.p + off + i + 1, p - i - 1, C->col + C->ustart[x], C->rowptr[x + 1] - C->ustart[x], C->A.p + off + p);
        C->held[d] = x;
        cc_node(C, d + 1, off + p, n);
    }
}

int32_t orc_clique_census(int64_t nv, const int64_t *rowptr, const int32_t *col, int32_t k_cap, int32_t k_local,
                          uint64_t *total, uint64_t *local, int32_t *saturated, uint64_t *n_nodes)
{
    if (nv < 0 || k_cap < 2 || k_local < 0 || (k_local && !local)) return -1;
    int64_t *ustart = (int64_t *)malloc((size_t)(nv + 1) * sizeof(int64_t));
    int64_t *ebase = (int64_t *)malloc((size_t)(nv + 1) * sizeof(int64_t));
    upper_index(nv, rowptr, col, ustart, ebase);
    const int32_t mud = max_upper_degree(nv, rowptr, ustart);
    struct cc C = { rowptr, ustart, col, k_cap, k_local, 0, total, local, NULL, NULL, 0, NULL, { NULL, 0 } };
    C.row = (uint64_t *)malloc((size_t)(mud + 2) * sizeof(uint64_t));
    C.row1 = (uint64_t *)malloc((size_t)(mud + 2) * sizeof(uint64_t));
    C.held = (int32_t *)malloc((size_t)(mud + 3) * sizeof(int32_t));
    memset(total, 0, (size_t)(k_cap + 1) * sizeof(uint64_t));
    if (local) memset(local, 0, (size_t)(nv > 0 ? nv : 1) * sizeof(uint64_t));
    for (int64_t v = 0; v < nv; ++v) {
        const int32_t p = (int32_t)(rowptr[v + 1] - ustart[v]);
        if (!p) continue;
        arena_need(&C.A, p);
        memcpy(C.A.p, col + ustart[v], (size_t)p * sizeof(int32_t));
        C.held[0] = (int32_t)v;
        cc_node(&C, 1, 0, p);
    }
    int sat = 0;
    for (int32_t k = 0; k <= k_cap; ++k) sat |= total[k] == UINT64_MAX;
    if (k_local) for (int64_t v = 0; v < nv; ++v) sat |= local[v] == UINT64_MAX;
    if (saturated) *saturated = sat;
    if (n_nodes) *n_nodes = C.nodes;
    free(ustart); free(ebase); free(C.row); free(C.row1); free(C.held); free(C.A.p);
    return C.omega;
}

/* --------------------------------------------------------------- maximal cliques
 * Definition: a clique contained in no larger one (include/komb_accel.h, "maximal cliques"); those of >= k_min vertices are
 * reported.  The PIVOT-FREE form: the same ordered enumeration of every clique as above, the node of (v_1 .. v_d) carrying
 * C = the intersection of its members' FULL neighbourhoods; its children are the members of C above v_d, and the clique is
 * maximal exactly when C is empty.  Ascending tuples in depth-first order come out in lexicographic order (no maximal clique
 * is a prefix of another), so the list needs no sort. */
struct mx {
    const int64_t *rowptr; const int32_t *col;
    int32_t k_cap, k_min, omega, want_list, bad;
    int64_t *hist; int32_t *count, *largest, *held;
    int64_t n_c, n_v, cap_c, cap_v, *off; int32_t *verts;
    uint64_t nodes;
    struct arena A;
};

static void mx_node(struct mx *M, int32_t d, int64_t off, int32_t c, int32_t last)
{
    M->nodes++;
    if (c == 0) {
        if (d < 2) return;
        if (d <= M->k_cap) M->hist[d]++; else M->bad = 1;
        if (d < M->k_min) return;
        if (d > M->omega) M->omega = d;
        for (int32_t i = 0; i < d; ++i) { const int32_t v = M->held[i]; M->count[v]++; if (M->largest[v] < d) M->largest[v] = d; }
        if (M->want_list) {
            if (M->n_c + 2 > M->cap_c) { M->cap_c *= 2; M->off = (int64_t *)realloc(M->off, (size_t)M->cap_c * sizeof(int64_t)); }
            if (M->n_v + d > M->cap_v) { while (M->n_v + d > M->cap_v) M->cap_v *= 2; M->verts = (int32_t *)realloc(M->verts, (size_t)M->cap_v * sizeof(int32_t)); }
            memcpy(M->verts + M->n_v, M->held, (size_t)d * sizeof(int32_t));
            M->n_v += d;
            M->off[M->n_c + 1] = M->n_v;
        }
        M->n_c++;
        return;
    }
    arena_need(&M->A, off + 2 * (int64_t)c);
    for (int32_t i = 0; i < c; ++i) {
        const int32_t x = M->A.p[off + i];
        if (x <= last) continue;
        const int32_t n = isect(M->A.p + off, c, M->col + M->rowptr[x], M->rowptr[x + 1] - M->rowptr[x], M->A.p + off + c);
        M->held[d] = x;
        mx_node(M, d + 1, off + c, n, x);
    }
}

int64_t orc_maximal_cliques(int64_t nv, const int64_t *rowptr, const int32_t *col, int32_t k_min, int32_t k_cap,
                            int64_t *hist, int32_t *count, int32_t *largest, int32_t *omega, uint64_t *n_nodes,
                            int64_t **offset_out, int32_t **verts_out, int64_t *n_verts)
{
    if (nv < 0 || k_min < 2 || k_cap < 2) return -1;
    int64_t mdeg = 0;
    for (int64_t v = 0; v < nv; ++v) if (rowptr[v + 1] - rowptr[v] > mdeg) mdeg = rowptr[v + 1] - rowptr[v];
    struct mx M = { rowptr, col, k_cap, k_min, 0, offset_out && verts_out, 0, hist, count, largest, NULL, 0, 0, 0, 0, NULL, NULL, 0, { NULL, 0 } };
    M.held = (int32_t *)malloc((size_t)(mdeg + 3) * sizeof(int32_t));
    memset(hist, 0, (size_t)(k_cap + 1) * sizeof(int64_t));
    memset(count, 0, (size_t)(nv > 0 ? nv : 1) * sizeof(int32_t));
    memset(largest, 0, (size_t)(nv > 0 ? nv : 1) * sizeof(int32_t));
    if (M.want_list) { M.cap_c = 4096; M.off = (int64_t *)malloc((size_t)M.cap_c * sizeof(int64_t)); M.off[0] = 0; M.cap_v = 16384; M.verts = (int32_t *)malloc((size_t)M.cap_v * sizeof(int32_t)); }
    for (int64_t v = 0; v < nv; ++v) {
        const int32_t c = (int32_t)(rowptr[v + 1] - rowptr[v]);
        if (!c) continue;
        arena_need(&M.A, c);
        memcpy(M.A.p, col + rowptr[v], (size_t)c * sizeof(int32_t));
        M.held[0] = (int32_t)v;
        mx_node(&M, 1, 0, c, (int32_t)v);
    }
    free(M.held); free(M.A.p);
    if (omega) *omega = M.omega;
    if (n_nodes) *n_nodes = M.nodes;
    if (n_verts) *n_verts = M.n_v;
    if (M.want_list) { *offset_out = M.off; *verts_out = M.verts; }
    return M.bad ? -1 : M.n_c;
}

void orc_free(void *p) { free(p); }

/* ------------------------------------------------------- (3,4)-nucleus decomposition
 * Definition: include/komb_accel.h, "(3,4)-nucleus decomposition".  Triangles a < b < c in ascending (a, b, c) order, which is
 * the order tests/nucleus_ref.py lists them in (canonical edge (a, b), then c); the 4-cliques a < b < c < d in the order
 * (triangle (a, b, c), d), each as the ids of its four triangles (a,b,c), (a,b,d), (a,c,d), (b,c,d); key0 = the cliques per
 * triangle; theta by a sequential bucket peel (Batagelj-Zaversnik's bins over the triangles: the triangle with the fewest
 * cliques left goes next, takes that number as theta and retires its cliques, each of which costs its other unprocessed
 * triangles above the level one).  The GPU's peel is level-synchronous over frontiers; theta is unique. */
struct nuc {
    int64_t nv; const int64_t *rowptr; const int32_t *col; int64_t *ustart, *ebase;
    int64_t ne, *tri_base; int32_t *tc;
};

static int64_t nuc_edge(const struct nuc *N, int32_t a, int32_t b)
{
    return N->ebase[a] + (find_sorted(N->col, N->ustart[a], N->rowptr[a + 1], b) - N->ustart[a]);
}

static int64_t nuc_tid(const struct nuc *N, int32_t a, int32_t b, int32_t c)
{
    const int64_t e = nuc_edge(N, a, b);
    return find_sorted(N->tc, N->tri_base[e], N->tri_base[e + 1], c);
}

/* the triangles: tri_base[e] .. tri_base[e + 1] are those of canonical edge e, tc their third vertices ascending */
static int64_t nuc_triangles(struct nuc *N)
{
    N->ustart = (int64_t *)malloc((size_t)(N->nv + 1) * sizeof(int64_t));
    N->ebase = (int64_t *)malloc((size_t)(N->nv + 1) * sizeof(int64_t));
    upper_index(N->nv, N->rowptr, N->col, N->ustart, N->ebase);
    N->ne = N->ebase[N->nv];
    N->tri_base = (int64_t *)calloc((size_t)N->ne + 1, sizeof(int64_t));
    const int32_t mud = max_upper_degree(N->nv, N->rowptr, N->ustart);
    int32_t *tmp = (int32_t *)malloc((size_t)(mud + 1) * sizeof(int32_t));
    int64_t cap = 1024, nt = 0;
    N->tc = (int32_t *)malloc((size_t)cap * sizeof(int32_t));
    for (int64_t a = 0; a < N->nv; ++a)
        for (int64_t j = N->ustart[a]; j < N->rowptr[a + 1]; ++j) {
            const int32_t b = N->col[j];
            const int32_t n = isect(N->col + j + 1, N->rowptr[a + 1] - j - 1, N->col + N->ustart[b], N->rowptr[b + 1] - N->ustart[b], tmp);
            if (nt + n > cap) { while (nt + n > cap) cap *= 2; N->tc = (int32_t *)realloc(N->tc, (size_t)cap * sizeof(int32_t)); }
            memcpy(N->tc + nt, tmp, (size_t)n * sizeof(int32_t));
            nt += n;
            N->tri_base[N->ebase[a] + (j - N->ustart[a]) + 1] = nt;
        }
    free(tmp);
    return nt;
}

static void nuc_free(struct nuc *N) { free(N->ustart); free(N->ebase); free(N->tri_base); free(N->tc); }

/* every 4-clique once, in (triangle, d) order; quads == NULL only counts */
static int64_t nuc_cliques(const struct nuc *N, int32_t *ta, int32_t *tb, int32_t *quads)
{
    int64_t nq = 0;
    for (int64_t a = 0; a < N->nv; ++a)
        for (int64_t j = N->ustart[a]; j < N->rowptr[a + 1]; ++j) {
            const int32_t b = N->col[j];
            const int64_t e = N->ebase[a] + (j - N->ustart[a]);
            for (int64_t t = N->tri_base[e]; t < N->tri_base[e + 1]; ++t) {
                const int32_t c = N->tc[t];
                if (ta) { ta[t] = (int32_t)a; tb[t] = b; }
                for (int64_t t2 = t + 1; t2 < N->tri_base[e + 1]; ++t2) {          /* d > c next to a and b */
                    const int32_t d = N->tc[t2];
                    if (find_sorted(N->col, N->ustart[c], N->rowptr[c + 1], d) < 0) continue;
                    if (quads) {
                        quads[4 * nq] = (int32_t)t; quads[4 * nq + 1] = (int32_t)t2;
                        quads[4 * nq + 2] = (int32_t)nuc_tid(N, (int32_t)a, c, d); quads[4 * nq + 3] = (int32_t)nuc_tid(N, b, c, d);
                    }
                    nq++;
                }
            }
        }
    return nq;
}

int64_t orc_nucleus_count(int64_t nv, const int64_t *rowptr, const int32_t *col, int64_t *n_cliques4)
{
    struct nuc N = { nv, rowptr, col, NULL, NULL, 0, NULL, NULL };
    const int64_t nt = nuc_triangles(&N);
    if (n_cliques4) *n_cliques4 = nuc_cliques(&N, NULL, NULL, NULL);
    nuc_free(&N);
    return nt;
}

int32_t orc_nucleus(int64_t nv, const int64_t *rowptr, const int32_t *col, int64_t n_triangles, int64_t n_cliques4,
                    int32_t *a, int32_t *b, int32_t *c, int32_t *key0, int32_t *theta,
                    int32_t *edge_theta, int32_t *vertex_theta, int32_t *quads)
{
    struct nuc N = { nv, rowptr, col, NULL, NULL, 0, NULL, NULL };
    const int64_t nt = nuc_triangles(&N);
    if (nt != n_triangles || nt > INT32_MAX) { nuc_free(&N); return -2; }
    const int64_t nq = nuc_cliques(&N, a, b, NULL);
    if (nq != n_cliques4 || nq > INT32_MAX / 4) { nuc_free(&N); return -2; }
    nuc_cliques(&N, a, b, quads);
    memcpy(c, N.tc, (size_t)nt * sizeof(int32_t));
    for (int64_t v = 0; v < nv; ++v) vertex_theta[v] = -1;
    for (int64_t e = 0; e < N.ne; ++e) edge_theta[e] = -1;
    if (nt == 0) { nuc_free(&N); return -1; }

    /* incidences: inc[ip[t] .. ip[t + 1]) = the cliques of triangle t */
    int64_t *ip = (int64_t *)calloc((size_t)nt + 1, sizeof(int64_t));
    for (int64_t i = 0; i < 4 * nq; ++i) ip[quads[i] + 1]++;
    int32_t maxk = 0;
    for (int64_t t = 0; t < nt; ++t) { key0[t] = (int32_t)ip[t + 1]; if (key0[t] > maxk) maxk = key0[t]; ip[t + 1] += ip[t]; }
    int32_t *inc = (int32_t *)malloc((size_t)(nq > 0 ? 4 * nq : 1) * sizeof(int32_t));
    int64_t *cur = (int64_t *)malloc((size_t)(nt + 1) * sizeof(int64_t));
    memcpy(cur, ip, (size_t)(nt + 1) * sizeof(int64_t));
    for (int64_t q = 0; q < nq; ++q) for (int r = 0; r < 4; ++r) inc[cur[quads[4 * q + r]]++] = (int32_t)q;
    free(cur);

    /* the peel */
    int32_t *key = (int32_t *)malloc((size_t)nt * sizeof(int32_t));
    memcpy(key, key0, (size_t)nt * sizeof(int32_t));
    int64_t *bin = (int64_t *)calloc((size_t)maxk + 2, sizeof(int64_t));
    int64_t *pos = (int64_t *)malloc((size_t)nt * sizeof(int64_t));
    int32_t *ord = (int32_t *)malloc((size_t)nt * sizeof(int32_t));
    uint8_t *done = (uint8_t *)calloc((size_t)nt, 1), *gone = (uint8_t *)calloc((size_t)(nq > 0 ? nq : 1), 1);
    for (int64_t t = 0; t < nt; ++t) bin[key[t]]++;
    int64_t start = 0;
    for (int32_t k = 0; k <= maxk; ++k) { const int64_t n = bin[k]; bin[k] = start; start += n; }
    for (int64_t t = 0; t < nt; ++t) { pos[t] = bin[key[t]]; ord[pos[t]] = (int32_t)t; bin[key[t]]++; }
    for (int32_t k = maxk; k > 0; --k) bin[k] = bin[k - 1];
    bin[0] = 0;
    int32_t tmax = 0;
    for (int64_t i = 0; i < nt; ++i) {
        const int32_t t = ord[i], k = key[t];
        theta[t] = k;
        if (k > tmax) tmax = k;
        done[t] = 1;
        for (int64_t x = ip[t]; x < ip[t + 1]; ++x) {
            const int32_t q = inc[x];
            if (gone[q]) continue;
            gone[q] = 1;
            for (int r = 0; r < 4; ++r) {
                const int32_t u = quads[4 * (int64_t)q + r];
                if (done[u] || key[u] <= k) continue;
                const int32_t ku = key[u];
                const int64_t pu = pos[u], pw = bin[ku];
                const int32_t w = ord[pw];
                if (u != w) { pos[u] = pw; pos[w] = pu; ord[pu] = w; ord[pw] = u; }
                bin[ku]++;
                key[u]--;
            }
        }
    }
    for (int64_t t = 0; t < nt; ++t) {
        const int64_t e3[3] = { nuc_edge(&N, a[t], b[t]), nuc_edge(&N, a[t], c[t]), nuc_edge(&N, b[t], c[t]) };
        const int32_t v3[3] = { a[t], b[t], c[t] };
        for (int r = 0; r < 3; ++r) {
            if (edge_theta[e3[r]] < theta[t]) edge_theta[e3[r]] = theta[t];
            if (vertex_theta[v3[r]] < theta[t]) vertex_theta[v3[r]] = theta[t];
        }
    }
    free(ip); free(inc); free(key); free(bin); free(pos); free(ord); free(done); free(gone);
    nuc_free(&N);
    return tmax;
}

/* ============================================================ traversals and graphlets
 * References for the distance analysis, the betweenness centrality and the graphlet census (include/komb_accel.h has the
 * definitions).  Each starts at a VERTEX and walks the sorted CSR rows: one queue BFS per source, one source at a time -- no
 * bit-parallel masks, no batches of 64 sources, no (d, id) order, no hash tables, no canonical-edge roots.  This file is
 * built with -ffp-contract=off (oracle/Makefile): every +, * and / below is one IEEE-754 binary64 operation that rounds once,
 * in the order written.  tests/test_oracle_traversals.py ties them to the Python restatements under tests/ and to the stored
 * fixtures bit for bit. */

/* one queue BFS from s: dist[] (-1: unreached; the caller hands it in all -1 and gets it back so), queue[] = the reached
 * vertices in the order found (distances never descend along it).  Returns how many. */
static int64_t bfs_queue(const int64_t *rowptr, const int32_t *col, int32_t s, int32_t *dist, int32_t *queue)
{
    int64_t head = 0, tail = 0;
    dist[s] = 0;
    queue[tail++] = s;
    while (head < tail) {
        const int32_t v = queue[head++], d = dist[v] + 1;
        for (int64_t j = rowptr[v]; j < rowptr[v + 1]; ++j) {
            const int32_t w = col[j];
            if (dist[w] < 0) { dist[w] = d; queue[tail++] = w; }
        }
    }
    return tail;
}

static int sources_ok(int64_t nv, int64_t n_sources, const int32_t *sources)
{
    if (nv < 0 || n_sources < 0 || (n_sources > 0 && !sources)) return 0;
    for (int64_t i = 0; i < n_sources; ++i) if (sources[i] < 0 || sources[i] >= nv) return 0;
    return 1;
}

int32_t orc_bfs_sources(int64_t nv, const int64_t *rowptr, const int32_t *col, int64_t n_sources, const int32_t *sources,
                        int64_t *src_reached, int64_t *src_sum, int32_t *src_ecc,
                        int64_t *n_reached, int64_t *sum_dist, int32_t *ecc, double *harmonic, int64_t *pairs)
{
    if (!sources_ok(nv, n_sources, sources)) return -1;
    for (int64_t v = 0; v < nv; ++v) { n_reached[v] = 0; sum_dist[v] = 0; ecc[v] = -1; harmonic[v] = 0.0; pairs[v] = 0; }
    if (nv == 0) return 0;
    int32_t *block = (int32_t *)malloc((size_t)64 * (size_t)nv * sizeof(int32_t));      /* block[k * nv + v] = d(entry k of the block, v) */
    int32_t *queue = (int32_t *)malloc((size_t)nv * sizeof(int32_t));
    int64_t *count = (int64_t *)calloc((size_t)nv, sizeof(int64_t));                  /* count[L]: the block's sources at distance L from one vertex */
    int32_t depth_max = 0;
    for (int64_t first = 0; first < n_sources; first += 64) {
        const int64_t in_block = n_sources - first < 64 ? n_sources - first : 64;
        memset(block, 0xFF, (size_t)in_block * (size_t)nv * sizeof(int32_t));
        for (int64_t k = 0; k < in_block; ++k) {
            int32_t *dist = block + k * nv;
            const int64_t n = bfs_queue(rowptr, col, sources[first + k], dist, queue);
            int64_t total = 0;
            for (int64_t i = 0; i < n; ++i) {
                const int32_t v = queue[i], d = dist[v];
                total += d;
                n_reached[v]++;
                sum_dist[v] += d;
                if (d > ecc[v]) ecc[v] = d;
                pairs[d]++;
            }
            src_reached[first + k] = n;
            src_sum[first + k] = total;
            src_ecc[first + k] = dist[queue[n - 1]];
            if (src_ecc[first + k] > depth_max) depth_max = src_ecc[first + k];
        }
        for (int64_t v = 0; v < nv; ++v) {
            int32_t top = 0;
            for (int64_t k = 0; k < in_block; ++k) {
                const int32_t d = block[k * nv + v];
                if (d > 0) { count[d]++; if (d > top) top = d; }
            }
            double h = 0.0;
            for (int32_t L = 1; L <= top; ++L)
                if (count[L] > 0) {
                    const double q = (double)count[L] / (double)L;
                    h = h + q;
                    count[L] = 0;
                }
            harmonic[v] = harmonic[v] + h;
        }
    }
    free(block); free(queue); free(count);
    return depth_max;
}

int32_t orc_betweenness(int64_t nv, const int64_t *rowptr, const int32_t *col, int64_t n_sources, const int32_t *sources,
                        double *bc, int64_t *src_reached, int64_t *src_sum, int32_t *src_ecc, int32_t *flags)
{
    if (!sources_ok(nv, n_sources, sources)) return -1;
    for (int64_t v = 0; v < nv; ++v) bc[v] = 0.0;
    *flags = 0;
    if (nv == 0) return 0;
    int32_t *dist = (int32_t *)malloc((size_t)nv * sizeof(int32_t));
    int32_t *queue = (int32_t *)malloc((size_t)nv * sizeof(int32_t));
    double *sigma = (double *)malloc((size_t)nv * sizeof(double));
    double *delta = (double *)malloc((size_t)nv * sizeof(double));
    memset(dist, 0xFF, (size_t)nv * sizeof(int32_t));
    int32_t rc = 0;
    for (int64_t i = 0; i < n_sources && rc == 0; ++i) {
        const int32_t s = sources[i];
        /* the queue BFS; a vertex sums its sigma when it leaves the queue: the queue ascends by level, so every vertex of the
         * level below has left it before and its sigma is final */
        int64_t head = 0, n = 0, total = 0;
        dist[s] = 0;
        queue[n++] = s;
        while (head < n) {
            const int32_t w = queue[head++], level = dist[w];
            double acc = 0.0;
            for (int64_t j = rowptr[w]; j < rowptr[w + 1]; ++j) {
                const int32_t x = col[j];
                if (dist[x] < 0) { dist[x] = level + 1; queue[n++] = x; }
                else if (dist[x] == level - 1) acc = acc + sigma[x];
            }
            sigma[w] = w == s ? 1.0 : acc;
            total += level;
            if (sigma[w] >= 9007199254740992.0) *flags |= 1;
            if (sigma[w] == INFINITY) rc = -2;
        }
        src_reached[i] = n;
        src_sum[i] = total;
        src_ecc[i] = dist[queue[n - 1]];
        for (int64_t k = n - 1; k >= 0 && rc == 0; --k) {
            const int32_t v = queue[k], above = dist[v] + 1;
            double acc = 0.0;
            for (int64_t j = rowptr[v]; j < rowptr[v + 1]; ++j) {
                const int32_t w = col[j];
                if (dist[w] == above) {
                    const double c = (1.0 + delta[w]) / sigma[w];
                    const double p = sigma[v] * c;
                    acc = acc + p;
                }
            }
            delta[v] = acc;
        }
        for (int64_t k = 0; k < n; ++k) {
            const int32_t v = queue[k];
            if (rc == 0 && v != s) bc[v] = bc[v] + delta[v];
            dist[v] = -1;
        }
    }
    free(dist); free(queue); free(sigma); free(delta);
    return rc;
}

static inline uint64_t comb2_u64(uint64_t x) { return x * (x - 1) / 2; }       /* (0 for x = 0: the product is 0) */

int32_t orc_graphlets(int64_t nv, const int64_t *rowptr, const int32_t *col, uint64_t *orbit, uint64_t *cycles4, uint64_t *cliques4,
                      int64_t *sup_out)
{
    if (nv < 0) return -1;
    if (nv == 0) return 0;
    const int64_t ne = rowptr[nv] / 2;
    const size_t nz = (size_t)nv;
    int64_t *ustart = (int64_t *)malloc((nz + 1) * sizeof(int64_t)), *ebase = (int64_t *)malloc((nz + 1) * sizeof(int64_t));
    upper_index(nv, rowptr, col, ustart, ebase);
    uint64_t *sup = (uint64_t *)calloc((size_t)(ne > 0 ? ne : 1), sizeof(uint64_t));
    uint64_t *p = (uint64_t *)calloc(nz, sizeof(uint64_t));
    uint64_t *acc = (uint64_t *)calloc(11 * nz, sizeof(uint64_t));
    uint64_t *d = acc, *t = acc + nz, *K4 = acc + 2 * nz, *C4 = acc + 3 * nz, *D2 = acc + 4 * nz, *D3 = acc + 5 * nz, *S = acc + 6 * nz,
             *W10 = acc + 7 * nz, *N9 = acc + 8 * nz, *B6 = acc + 9 * nz, *SS = acc + 10 * nz;
    int64_t dmax = 0;
    for (int64_t v = 0; v < nv; ++v) { d[v] = (uint64_t)(rowptr[v + 1] - rowptr[v]); if ((int64_t)d[v] > dmax) dmax = (int64_t)d[v]; }
    int32_t *common = (int32_t *)malloc((size_t)(dmax > 0 ? dmax : 1) * sizeof(int32_t)), *inner = (int32_t *)malloc((size_t)(dmax > 0 ? dmax : 1) * sizeof(int32_t));

    /* per canonical edge (u, v): the 4-cycles u - x - y - v from p[y] = |N(u) & N(y)| (v is always one of those x); the common
     * neighbourhood, its size and the edges inside it */
    for (int64_t u = 0; u < nv; ++u) {
        for (int64_t j = rowptr[u]; j < rowptr[u + 1]; ++j) {
            const int32_t x = col[j];
            for (int64_t i = rowptr[x]; i < rowptr[x + 1]; ++i) p[col[i]]++;
        }
        for (int64_t j = ustart[u]; j < rowptr[u + 1]; ++j) {
            const int32_t v = col[j];
            const int64_t e = ebase[u] + (j - ustart[u]);
            uint64_t cyc = 0;
            for (int64_t i = rowptr[v]; i < rowptr[v + 1]; ++i) if (col[i] != (int32_t)u) cyc += p[col[i]] - 1;
            cycles4[e] = cyc;
            const int32_t nc = isect(col + rowptr[u], rowptr[u + 1] - rowptr[u], col + rowptr[v], rowptr[v + 1] - rowptr[v], common);
            uint64_t inside = 0;
            for (int32_t a = 0; a < nc; ++a) {
                const int32_t w = common[a];
                inside += (uint64_t)isect(col + ustart[w], rowptr[w + 1] - ustart[w], common + a + 1, nc - a - 1, inner);
                D2[w] += (uint64_t)nc - 1;                                       /* the triangle (w, u, v): its edge opposite w */
            }
            sup[e] = (uint64_t)nc;
            cliques4[e] = inside;
            if (sup_out) sup_out[e] = nc;
        }
        for (int64_t j = rowptr[u]; j < rowptr[u + 1]; ++j) {
            const int32_t x = col[j];
            for (int64_t i = rowptr[x]; i < rowptr[x + 1]; ++i) p[col[i]] = 0;
        }
    }

    /* the sums over the edges at a vertex, then the closed forms (tests/graphlets_ref.py census(); unsigned 64-bit throughout:
     * every final value is below 2^63 for degrees below 2^20, and an intermediate that wraps wraps back) */
    for (int64_t u = 0; u < nv; ++u)
        for (int64_t j = ustart[u]; j < rowptr[u + 1]; ++j) {
            const int32_t v = col[j];
            const int64_t e = ebase[u] + (j - ustart[u]);
            t[u] += sup[e]; t[v] += sup[e];
            K4[u] += cliques4[e]; K4[v] += cliques4[e];
            C4[u] += cycles4[e]; C4[v] += cycles4[e];
            D3[u] += comb2_u64(sup[e]); D3[v] += comb2_u64(sup[e]);
            S[u] += d[v] - 1; S[v] += d[u] - 1;
            W10[u] += sup[e] * (d[v] - 2); W10[v] += sup[e] * (d[u] - 2);
            B6[u] += comb2_u64(d[v] - 1); B6[v] += comb2_u64(d[u] - 1);
        }
    int32_t rc = 0;
    for (int64_t v = 0; v < nv; ++v) {                  /* a triangle has two edges at v, a 4-clique three, a 4-cycle two */
        if (t[v] % 2 || K4[v] % 3 || C4[v] % 2) rc = -2;
        t[v] /= 2; K4[v] /= 3; C4[v] /= 2;
    }
    for (int64_t u = 0; u < nv; ++u)
        for (int64_t j = ustart[u]; j < rowptr[u + 1]; ++j) {
            const int32_t v = col[j];
            const int64_t e = ebase[u] + (j - ustart[u]);
            N9[u] += t[v] - sup[e]; N9[v] += t[u] - sup[e];
            SS[u] += S[v]; SS[v] += S[u];
        }
    for (int64_t v = 0; v < nv; ++v) {
        uint64_t o[15];
        const uint64_t dv = d[v], tv = t[v], k4 = K4[v];
        o[0] = dv;
        o[3] = tv;
        o[2] = comb2_u64(dv) - tv;
        o[1] = S[v] - 2 * tv;
        o[14] = k4;
        o[13] = D3[v] - 3 * k4;
        o[12] = D2[v] - 3 * k4;
        o[8] = C4[v] - o[12] - o[13] - 3 * k4;
        o[11] = tv * (dv - 2) - 2 * o[13] - 3 * k4;
        o[10] = W10[v] - 2 * o[13] - 2 * o[12] - 6 * k4;
        o[9] = N9[v] - 2 * o[12] - 3 * k4;
        o[7] = dv * (dv - 1) * (dv - 2) / 6 - o[11] - o[13] - k4;              /* (a product with a factor 0 below three) */
        o[6] = B6[v] - o[9] - o[10] - o[13] - 2 * o[12] - 3 * k4;
        o[4] = SS[v] - dv * (dv - 1) - 2 * tv - 2 * o[8] - 2 * o[9] - o[10] - 2 * o[13] - 4 * o[12] - 6 * k4;
        o[5] = (dv - 1) * S[v] - 2 * tv - 2 * o[8] - o[10] - 2 * o[11] - 4 * o[13] - 2 * o[12] - 6 * k4;
        for (int k = 0; k < 15; ++k) orbit[(size_t)k * nz + (size_t)v] = o[k];
    }
    free(ustart); free(ebase); free(sup); free(p); free(acc); free(common); free(inner);
    return rc;
}

/* the orbit of v in the induced subgraph on set[0 .. n) (n = 3 or 4, connected, set[0] = v): by the number of edges and the
 * degrees inside the set, which tell the connected 3- and 4-vertex graphs and their orbits apart */
static int orbit_in_set(const int64_t *rowptr, const int32_t *col, const int32_t *set, int n)
{
    int deg[4] = { 0, 0, 0, 0 }, edges = 0, top = 0;
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b)
            if (find_sorted(col, rowptr[set[a]], rowptr[set[a] + 1], set[b]) >= 0) { deg[a]++; deg[b]++; edges++; }
    for (int a = 0; a < n; ++a) if (deg[a] > top) top = deg[a];
    const int mine = deg[0];
    if (n == 3) return edges == 3 ? 3 : (mine == 1 ? 1 : 2);
    switch (edges) {
    case 3: return top == 3 ? (mine == 3 ? 7 : 6) : (mine == 1 ? 4 : 5);
    case 4: return top == 3 ? (mine == 1 ? 9 : mine == 2 ? 10 : 11) : 8;
    case 5: return mine == 2 ? 12 : 13;
    default: return 14;
    }
}

/* every connected set of up to four vertices that holds set[0], each once: the set grows by one vertex of ext[] at a time;
 * a vertex enters ext[] when the set first touches it (near[] counts the members of the set it is, or is adjacent to), and a
 * vertex taken from ext[] stays out of the branches of the vertices taken after it. */
struct byd { const int64_t *rowptr; const int32_t *col; int32_t *near; uint64_t *out; int32_t set[4]; };

static void byd_grow(struct byd *B, int n, const int32_t *ext, int64_t n_ext)
{
    for (int64_t i = n_ext - 1; i >= 0; --i) {
        const int32_t w = ext[i];
        B->set[n] = w;
        if (n + 1 >= 3) B->out[orbit_in_set(B->rowptr, B->col, B->set, n + 1)]++;
        if (n + 1 == 4) continue;
        int64_t room = i;
        for (int64_t j = B->rowptr[w]; j < B->rowptr[w + 1]; ++j) if (B->near[B->col[j]] == 0) room++;
        int32_t *next = (int32_t *)malloc((size_t)(room > 0 ? room : 1) * sizeof(int32_t));
        memcpy(next, ext, (size_t)i * sizeof(int32_t));
        int64_t n_next = i;
        for (int64_t j = B->rowptr[w]; j < B->rowptr[w + 1]; ++j) {
            const int32_t x = B->col[j];
            if (B->near[x]++ == 0) next[n_next++] = x;
        }
        byd_grow(B, n + 1, next, n_next);
        for (int64_t j = B->rowptr[w]; j < B->rowptr[w + 1]; ++j) B->near[B->col[j]]--;
        free(next);
    }
}

int64_t orc_orbits_by_definition(int64_t nv, const int64_t *rowptr, const int32_t *col, int32_t v, int64_t ball_limit, uint64_t *out)
{
    if (nv <= 0 || v < 0 || v >= nv) return -2;
    int32_t *near = (int32_t *)calloc((size_t)nv, sizeof(int32_t));
    int32_t *queue = (int32_t *)malloc((size_t)nv * sizeof(int32_t));
    /* the ball: the vertices within three hops (near[] is the distance + 1 while it is measured) */
    int64_t head = 0, tail = 0;
    near[v] = 1;
    queue[tail++] = v;
    while (head < tail && !(ball_limit > 0 && tail > ball_limit)) {
        const int32_t x = queue[head++];
        if (near[x] == 4) break;
        for (int64_t j = rowptr[x]; j < rowptr[x + 1]; ++j)
            if (near[col[j]] == 0) { near[col[j]] = near[x] + 1; queue[tail++] = col[j]; }
    }
    const int64_t ball = tail;
    for (int64_t i = 0; i < tail; ++i) near[queue[i]] = 0;
    free(queue);
    if (ball_limit > 0 && ball > ball_limit) { free(near); return -1; }
    for (int k = 0; k < 15; ++k) out[k] = 0;
    out[0] = (uint64_t)(rowptr[v + 1] - rowptr[v]);
    struct byd B = { rowptr, col, near, out, { v, 0, 0, 0 } };
    near[v] = 1;
    for (int64_t j = rowptr[v]; j < rowptr[v + 1]; ++j) near[col[j]]++;
    byd_grow(&B, 1, col + rowptr[v], rowptr[v + 1] - rowptr[v]);
    free(near);
    return ball;
}
