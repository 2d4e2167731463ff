// common.h -- shared host-side definitions of libkomb_accel (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "komb_accel.h"

#include <roctracer/roctx.h>

namespace komb {

// roctx range around a phase of the path (rocprofv3 --marker-trace shows them)
struct Range {
    explicit Range(const char *name) { (void)roctxRangePushA(name); }
    ~Range() { (void)roctxRangePop(); }
    void next(const char *name) { (void)roctxRangePop(); (void)roctxRangePushA(name); }   // one phase ends, the next begins
    Range(const Range &) = delete;
    Range &operator=(const Range &) = delete;
};

constexpr int kBlock = 256;                 // 4 wave64 per workgroup
constexpr int kWave = 64;
inline int tiles_of(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }   // workgroups of kBlock lanes, one lane per item
// stamp / core value of a live edge / vertex: kAlive - c, where c = 0 for a unit with a short slice
// ("light") and c = its number of kChunk-item chunks otherwise.  Whoever reads the marker to test
// liveness (the SCAN sweep, the item that decrements the unit) learns the unit's class for free,
// instead of fetching its slice bounds.
constexpr int32_t kAlive = 0x7FFFFFFF;
constexpr int32_t kAliveMin = 0x40000000;   // every alive marker is >= this; every round / level number is below it

// sum / maximum over the lanes of a wave, in every lane; every lane of the wave calls them
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int o = kWave / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int32_t)v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (int o = kWave / 2; o > 0; o >>= 1) { const uint32_t other = (uint32_t)__shfl_xor((int32_t)v, o); v = other > v ? other : v; }
    return v;
}

// Device-side control block of a peel loop.  One 128-byte record; the fields a
// launch reads at entry are written only by the workgroup that finalises a step.
// `seq` is the index of the launch the state is meant for: every launch carries its
// own index, a workgroup acts only when the two agree before AND after it has read
// the state, and a finaliser moves `seq` on before it touches anything else -- so a
// workgroup that is dispatched late (another process shares the GPU, say), after the
// state has already been rewritten for the next launch, leaves instead of taking part
// in a step that is not its launch's.
struct PeelCtrl {
    // ---- first 64-byte line: the state a launch reads at entry (one coalesced load = one snapshot) and its sequence word.
    // Written by the finalising workgroup only; the counters in it are statistics.
    int32_t  mode;          // 0 = SCAN, 1 = PROCESS
    int32_t  level;         // current peel level (degree k / support L)
    int32_t  round;         // sub-round id stamped on the current frontier
    int32_t  done;          // 1 once every unit is peeled (2 = inconsistent state, 3 = handed over, see tail_limit)
    uint32_t cur_light;     // entries in the current light queue (unit ids)
    uint32_t cur_heavy;     // entries in the current heavy queue ((unit, chunk) pairs)
    int32_t  cur_sel;       // which of the two queue pairs is current
    uint32_t remaining;     // units that have not entered a frontier yet
    int32_t  n_levels;      // stats: populated levels
    int32_t  n_rounds;      // stats: PROCESS launches
    int32_t  n_scans;       // stats: SCAN launches
    int32_t  max_level;     // stats: highest populated level
    uint32_t live_count;    // entries of the compacted live list (live_mode 1)
    int32_t  live_sel;      // which live-list buffer is current
    int32_t  live_mode;     // 0: SCAN sweeps all units; 1: SCAN sweeps the live list
    int32_t  seq;           // index of the launch this state is for (see above)
    // ---- second line: modified with atomics during a launch
    uint32_t tail_l[2];     // append cursors of the light queues
    uint32_t tail_h[2];     // append cursors of the heavy queues
    int32_t  next_min;      // min live key above the scanned level
    uint32_t live_tail;     // survivors appended by the running SCAN
    int32_t  last_retire;   // problems with one-byte states: the sub-round the last RETIRE step ran before (finaliser only)
    // ---- hand-over to a finish (local_dev.h, truss_tail.h, core_tail.h); constant while launches are queued
    uint32_t tail_limit;    // a level that starts with at most this many units left sets done = 3 (0: never)
    uint32_t pad1[7];       // (-DKOMB_STEP_TIMERS: stopwatch sums)
    int32_t  max_retire_gap;    // the most sub-rounds that ever passed without a RETIRE step: the host checks it against the period
};
static_assert(offsetof(PeelCtrl, seq) == 60 && offsetof(PeelCtrl, tail_l) == 64, "PeelCtrl: the entry state is one 64-byte line");
static_assert(sizeof(PeelCtrl) == 128, "PeelCtrl layout");

// Device-side control block of the local finish (local_dev.h): an h-index fixed point on the remainder
// the peel hands over.  64 bytes, device resident; the host keeps two pinned mirrors.
struct LocalCtrl {
    int32_t  done;           // 1 once a sweep changed nothing
    int32_t  iters;          // sweeps run (including the one that changed nothing)
    uint32_t spare[3];       // [0]: the sweep that is running (progress word for the host's guard); the per-sweep change counters live in their own array
    uint32_t bad;            // consistency failures (a compact slice whose fill differs from the live key, ...)
    int32_t  max_val;        // largest final value (k_local_finish)
    uint32_t levels;         // distinct final values (k_local_levels)
    uint32_t evals;          // unit evaluations, all sweeps
    uint32_t n_light, n_heavy;   // numbering counters (k_local_number)
    uint32_t n_giant;        // heavy units with more than kMedMax items
    uint32_t n_chunk;        // chunks of kGiantChunk items they are counted in
    uint32_t pad0;
    unsigned long long key_sum;  // sum of the live keys = items of the remainder (k_local_number)
};
static_assert(sizeof(LocalCtrl) == 64, "LocalCtrl layout");

// How a peel ends (option FINISH, komb_set_option): "local" hands the remainder to the h-index fixed point of local_dev.h
// once at most LOCAL_LIMIT units (default: a fraction of all units) are left at a level boundary and it has at most
// LOCAL_ITEMS items (else it is refused and offered again later); "lds" uses the single-workgroup LDS tails
// (truss_tail.h, core_tail.h; thresholds TAIL / CORE_TAIL); "none" keeps the whole peel in the general
// engine.  None of them changes a result.  Default for both peels: "local" (MI355X: k-core |V| = 1M 5.3 -> 3.0 ms,
// |V| = 10M 16.8 -> 10.7 ms; k-truss peel |E| = 10M 3.7 -> 2.9 ms, |E| = 100M 13.0 -> 11.1 ms against "lds").
enum FinishMode : int { FIN_LOCAL = 0, FIN_LDS = 1, FIN_NONE = 2 };

struct Timer {                               // HIP-event stopwatch on one stream
    hipEvent_t a = nullptr, b = nullptr;
    bool init() { return hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess; }
    void start(hipStream_t s) { (void)hipEventRecord(a, s); }
    double stop(hipStream_t s)
    {
        (void)hipEventRecord(b, s);
        (void)hipEventSynchronize(b);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, a, b);
        return (double)ms;
    }
    void destroy() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); a = b = nullptr; }
};

// HIP events that are destroyed on every way out of the scope that made them (error returns included)
struct EventSet {
    std::vector<hipEvent_t> v;
    EventSet() = default;
    EventSet(const EventSet &) = delete;
    EventSet &operator=(const EventSet &) = delete;
    hipError_t make(hipEvent_t *out, unsigned flags = 0)
    {
        hipEvent_t e = nullptr;
        const hipError_t rc = flags ? hipEventCreateWithFlags(&e, flags) : hipEventCreate(&e);
        if (rc == hipSuccess) { v.push_back(e); *out = e; }
        return rc;
    }
    ~EventSet() { for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e); }
};

} // namespace komb

// Option POISON (komb_set_option(ctx, "POISON", "0xWWWWWWWW")): while it is set, every device allocation the context hands
// out -- new and reused pool blocks, the resident graph, the k-core results, the graph build's scratch -- is filled with that
// 32-bit word before it is returned, so a kernel or host step that reads memory it never wrote sees garbage instead of the
// zeros of a fresh page or the previous run's values (tests only; off, it costs one branch per allocation).  The fill is
// waited for: the graph upload writes on the staging streams, not on the context's.
// Options ALLOC_FAIL_AT / ALLOC_TRIM_AT (komb_set_option; tests only): one counter over every device allocation request of the
// context -- DevPool::get and Poison::malloc, the two places all of them pass through -- and two one-shot triggers on it.
// Request number fail_at (1-based, counted from the moment the option was set) returns hipErrorOutOfMemory before anything is
// done: no hipMalloc, no trim(), nothing on the device.  Request number trim_at, when it is a pool request, gives the cached
// blocks back to the driver first (trim(), what a real near-out-of-memory request does before it retries) and is then served
// normally.  Both disarm when they fire.  `armed` is the one branch a request pays with neither option set.
struct AllocHook {
    bool armed = false;                              // counting, or a trigger waits
    int64_t requests = 0, fail_at = 0, trim_at = 0;  // 0: no trigger
    int32_t fired = 0;                               // the fail trigger has fired since it was last set
    enum Act { PASS, FAIL, TRIM };
    Act step()                                       // one request (called only while armed)
    {
        ++requests;
        if (fail_at && requests == fail_at) { fail_at = 0; fired = 1; return FAIL; }
        if (trim_at && requests == trim_at) { trim_at = 0; return TRIM; }
        return PASS;
    }
};

struct Poison {
    bool on = false;
    uint32_t word = 0;
    hipStream_t stream = nullptr;                    // the context's stream
    AllocHook *hook = nullptr;                       // the pool's (DevPool::hook): the allocations outside the pool count on it too
    hipError_t fill(void *p, size_t bytes) const
    {
        if (!on || !p || !bytes) return hipSuccess;
        const size_t words = bytes / 4, rest = bytes % 4;
        hipError_t e = hipSuccess;
        if (words) e = hipMemsetD32Async((hipDeviceptr_t)p, (int)word, words, stream);
        if (e == hipSuccess && rest) e = hipMemsetAsync((char *)p + 4 * words, (int)(word & 0xFFu), rest, stream);
        return e == hipSuccess ? hipStreamSynchronize(stream) : e;
    }
    hipError_t malloc(void **out, size_t bytes) const  // hipMalloc, then the fill (the one allocation path outside the pool)
    {
        if (hook && hook->armed && hook->step() == AllocHook::FAIL) return hipErrorOutOfMemory;
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return e;
        e = fill(q, bytes);
        if (e != hipSuccess) { (void)hipFree(q); return e; }
        *out = q;
        return hipSuccess;
    }
};

// Caching device allocator: a step's scratch buffers are returned to the pool,
// not to the driver, so steady-state steps perform no hipMalloc / hipFree.
struct DevPool {
    struct Block { void *p; size_t bytes; bool used; };
    std::vector<Block> blocks;
    size_t n_malloc = 0, n_trim = 0;                 // statistics (KOMB_POOL_DEBUG)
    double ms_malloc = 0.0;                          // host time inside hipMalloc
    Poison poison;                                   // option POISON (above); also what the allocations outside the pool use
    AllocHook hook;                                  // options ALLOC_FAIL_AT / ALLOC_TRIM_AT (above)
    DevPool() { poison.hook = &hook; }
    DevPool(const DevPool &) = delete;               // (poison.hook points into this object)
    DevPool &operator=(const DevPool &) = delete;
    hipError_t get(void **out, size_t bytes)
    {
        if (hook.armed) {
            const AllocHook::Act a = hook.step();
            if (a == AllocHook::FAIL) return hipErrorOutOfMemory;
            if (a == AllocHook::TRIM) { ++n_trim; trim(); }
        }
        if (bytes == 0) bytes = 16;
        int best = -1;
        for (int i = 0; i < (int)blocks.size(); ++i)
            if (!blocks[i].used && blocks[i].bytes >= bytes && blocks[i].bytes <= bytes + bytes / 4 + 4096 &&
                (best < 0 || blocks[i].bytes < blocks[best].bytes)) best = i;
        if (best >= 0) {
            if (poison.on) { const hipError_t e = poison.fill(blocks[best].p, blocks[best].bytes); if (e != hipSuccess) return e; }
            blocks[best].used = true; *out = blocks[best].p; return hipSuccess;
        }
        void *q = nullptr;
        ++n_malloc;
        const auto t0 = std::chrono::steady_clock::now();
        hipError_t e = hipMalloc(&q, bytes);
        ms_malloc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (e != hipSuccess) {                       // give cached blocks back and retry once
            ++n_trim;
            trim();
            e = hipMalloc(&q, bytes);
            if (e != hipSuccess) return e;
        }
        blocks.push_back({q, bytes, true});
        if (poison.on) { e = poison.fill(q, bytes); if (e != hipSuccess) { put(q); return e; } }
        *out = q;
        return hipSuccess;
    }
    void put(void *p)
    {
        if (!p) return;
        for (auto &b : blocks) if (b.p == p) { b.used = false; return; }
    }
    size_t unused_bytes() const                      // cached blocks nobody holds: a large request gets them back (trim) before it fails
    {
        size_t t = 0;
        for (const auto &b : blocks) if (!b.used) t += b.bytes;
        return t;
    }
    void trim()                                      // free every unused block
    {
        std::vector<Block> keep;
        for (auto &b : blocks) { if (b.used) keep.push_back(b); else (void)hipFree(b.p); }
        blocks.swap(keep);
    }
    void clear()
    {
        for (auto &b : blocks) (void)hipFree(b.p);
        blocks.clear();
    }
};

// One device array of a result and where it came from: a block of a pool, or (pool == nullptr) a hipMalloc made through
// dev_malloc.  Move-only; it allocates nothing: an allocation call fills slot(), and whatever the handle holds goes back where
// it came from when the handle is reset, assigned to or destroyed.  A result is a struct of these (komb_ctx), so dropping it
// is `ctx->x = {}` and installing a finished one is one move.
template <class T> struct DevArr {
    T *p = nullptr;
    DevPool *pool = nullptr;
    DevArr() = default;
    DevArr(DevArr &&o) noexcept : p(o.p), pool(o.pool) { o.p = nullptr; }
    DevArr &operator=(DevArr &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; pool = o.pool; o.p = nullptr; }
        return *this;
    }
    ~DevArr() { reset(); }
    void reset()
    {
        if (p) { if (pool) pool->put(p); else (void)hipFree(p); }
        p = nullptr;
    }
    T **slot(DevPool *from) { reset(); pool = from; return &p; }   // what `from`->get() or (null) dev_malloc writes the array to
    T *get() const { return p; }
    operator T *() const { return p; }
};

// Everything the k-truss path derives from a symmetric CSR before it enumerates a triangle (truss_prep.hip): the
// (degree,id) renumbering, the oriented CSR in those INTERNAL ids, the canonical edge list and the internal edge id of
// every canonical edge, the per-vertex lines and the task table of the enumeration.  Built on the first k-truss call
// of a graph (or by komb_truss_prepare), kept until the graph goes (or komb_truss_unprepare); an induced subgraph
// gets a temporary one of its own.  Every array is a block of the context's pool.
struct TrussPrep {
    bool valid = false;
    int64_t nv = 0, ne = 0;
    int32_t  *o2i = nullptr, *i2o = nullptr; // [nv] original -> internal id (rank in (degree, original id) order) and back
    uint32_t *orow = nullptr;                // [nv+1]  oriented CSR, INTERNAL ids, rows ascending (source below target): internal edge id = oriented slot
    int32_t  *ocol = nullptr, *osrc = nullptr;   // [ne + 8] target of every oriented slot; [ne] its source -- only once prep_sources was asked (LDS tail, moments)
    uint32_t *e2k = nullptr;                 // [ne] canonical edge id of every internal edge (oriented slot)
    uint4    *vline = nullptr;               // [4*nv] one 64-byte line per vertex: start, length, pivots and signature of its oriented row (truss_line.h)
    void     *wtasks = nullptr;              // [n_wtasks] task descriptors of the triangle enumeration (truss_line.h)
    int64_t   n_wtasks = 0;
    int64_t   own_bound = 0;                 // sum over the vertices of d+ (d+ - 1): bound on the own-role index entries (capacities of a k-truss run)
    double    ms = 0.0;                      // device time of the build (HIP events) ...
    double    ms_part[4] = {0, 0, 0, 0};     // ... and of its parts: vertex order | edges to rows + row pointers | row sort + lines + canonical map | tasks
};

struct komb_ctx {
    komb_opts opts{};
    DevPool pool;                            // (declared before every result record: it outlives their handles when the context is deleted)
    std::string err;
    bool device_ok = false;
    int device = 0;
    hipStream_t stream = nullptr;            // the context's own blocking stream (api.cpp)
    bool own_stream = false;
    komb::Timer timer;
    std::map<std::string, std::string> options;   // komb_set_option: tuning / test switches (none changes a result)

    // ---- resident simple graph: the symmetric CSR in the caller's (ORIGINAL) vertex ids, rows ascending -- what every result
    // is reported in, what k-core peels on, what komb_graph_get_csr returns
    int64_t nv = -1, ne = 0;
    uint32_t *d_o_rowptr = nullptr;          // [nv+1]
    int32_t  *d_o_col = nullptr;             // [2*ne]
    // ---- the k-truss side of the graph, made when a k-truss call first needs it
    TrussPrep prep;

    // ---- the results of the analyses: one record each -- its device arrays (DevArr: they go back where they came from when the
    // record is dropped, `ctx->x = {}`, or replaced), its summary and host vectors, and `done`.  DESIGN.md section 3 says who
    // drops whom.

    // ---- k-core results
    struct Core {
        DevArr<int32_t> deg;                 // [nv] degree (a2), ORIGINAL ids
        DevArr<int32_t> core;                // [nv] coreness (a3), ORIGINAL ids
        bool done = false;
    } core;

    // ---- onion decomposition results (onion.hip): arrays of their own, none of k-core's
    struct Onion {
        DevArr<int32_t> layer;               // [nv] layer, ORIGINAL ids
        DevArr<int32_t> core;                // [nv] coreness the vertex left at
        int64_t n_layers = 0;                // largest layer number of the last run
        int32_t max_core = 0;
        double ms = 0.0;                     // device time of the last run (HIP events)
        bool done = false;
    } onion;

    // ---- connected components of a k-core / k-truss subgraph (components.hip): a snapshot in arrays of its own
    struct Components {
        DevArr<int32_t> label;               // [nv] smallest ORIGINAL id of the vertex' component, -1 for a non-member
        DevArr<int32_t> size;                // [nv] vertices of that component, 0 for a non-member
        int32_t kind = 0, k = 0;             // what the last run was asked for (k resolved)
        int64_t members = 0, count = 0, largest = 0;
        double ms = 0.0;                     // device time of the last run (HIP events)
        bool done = false;
    } comp;

    // ---- component hierarchy (hierarchy.hip): the nesting forest of the k-core / k-truss components, a snapshot in arrays of its own
    struct Hierarchy {
        DevArr<int32_t> nodes;               // [5 * max(nv, 1)] k | rep | parent | size | shell, each a block of max(nv, 1) words with n_nodes in use
        DevArr<int32_t> vnode;               // [nv] the node of every vertex, -1 for a non-member
        int32_t kind = 0, kmax = 0, depth = 0;
        int64_t n_nodes = 0, n_roots = 0;
        double ms = 0.0;                     // device time of the last run (HIP events)
        bool done = false;
    } hier;

    // ---- densest-subgraph search (densest.hip): a snapshot in arrays of its own (pool blocks), dropped with the graph
    struct Densest {
        DevArr<int32_t> member;              // [nv] 1 for a vertex of the result, 0 otherwise
        DevArr<int32_t> load;                // [nv] Frank-Wolfe load of the vertex, 0 outside the pruned set
        int32_t source = 0, k_best = 0, k_prune = 0, iters = 0, k_max = 0;
        int64_t n_pruned = 0, m_pruned = 0, n_sub = 0, m_sub = 0, load_max = 0;
        double ms = 0.0;                     // device time of the last run (HIP events)
        bool local = false;                  // the rounds ran in the single-workgroup LDS kernel
        std::vector<int64_t> profile;        // n_k[k_max + 1] | m_k[k_max + 1] of the last run
        bool done = false;
    } dens;

    // ---- k-truss communities (communities.hip): arrays of their own (pool blocks), indexed like the k-truss result they were
    // computed from and dropped with it (truss_free)
    struct Communities {
        DevArr<int32_t> label;               // [t_ne] smallest canonical edge index of the edge's community, -1 for a non-member
        DevArr<int32_t> size;                // [t_ne] edges of that community, 0 for a non-member
        DevArr<int32_t> ncomm;               // [nv] distinct communities at the vertex: made by the first fetch_vertices / info after a run
        int32_t k = 0;                       // the threshold of the last run (resolved)
        int64_t members = 0, count = 0, largest = 0, multi = 0;
        double ms = 0.0, ms_vertices = 0.0;  // device time of the run | of the vertex pass (HIP events)
        bool done = false, v_ready = false;
    } comm;

    // ---- biconnected components (biconnected.hip): arrays of their own (pool blocks), indexed like the k-truss result they were
    // computed from and dropped with it (truss_free)
    struct Biconnected {
        DevArr<int32_t> block;               // [t_ne] smallest canonical edge index of the edge's block, -1 for a non-member
        DevArr<int32_t> size;                // [t_ne] edges of that block, 0 for a non-member (1: a bridge)
        DevArr<int32_t> nblocks;             // [nv] blocks that contain the vertex (>= 2: an articulation point)
        DevArr<int32_t> ecc_label;           // [nv] smallest ORIGINAL id of the vertex' 2-edge-connected component, -1 for a non-member
        DevArr<int32_t> ecc_size;            // [nv] vertices of that component, 0 for a non-member
        DevArr<int32_t> list;                // [3 * n_blocks] rep | n_edges | n_verts of the blocks in ascending rep order
        int32_t k = 0, depth = 0;            // the threshold of the last run (resolved) | the levels of its spanning forest
        int64_t n_member_edges = 0, n_member_vertices = 0, n_blocks = 0, n_bridges = 0, n_articulation = 0, largest_block = 0,
                n_ecc = 0, largest_ecc = 0;
        double ms = 0.0;                     // device time of the last run (HIP events)
        bool done = false;
    } bc;

    // ---- k-truss community hierarchy (community_hierarchy.hip): the nesting forest of the communities over all k, in pool blocks
    // of its own, indexed like the k-truss result it was computed from and dropped with it (truss_free)
    struct CommunityHierarchy {
        DevArr<int32_t> nodes;               // [5 * cap] k | rep | parent | size | shell, each a block of cap words with n_nodes in use
        DevArr<int32_t> enode;               // [t_ne] the node of every canonical edge, -1 for a non-member
        int64_t cap = 1, n_nodes = 0, n_roots = 0, members = 0;
        int32_t kmax = 2, depth = 0;
        double ms = 0.0;                     // device time of the last run (HIP events)
        bool done = false;
    } ch;

    // ---- structural clustering (structural.hip): arrays of their own (pool blocks), indexed like the k-truss result they were
    // computed from and dropped with it (truss_free)
    struct Structural {
        DevArr<int32_t> label;               // [nv] the cluster of the vertex (smallest ORIGINAL id of its cores' class), -1 for a hub / an outlier
        DevArr<int32_t> size;                // [nv] vertices that carry that label, 0 for label -1
        DevArr<int32_t> role;                // [nv] KOMB_SC_*
        DevArr<int32_t> simdeg;              // [nv] similar edges at the vertex
        DevArr<uint8_t> similar;             // [t_ne] 1 for a similar edge
        int32_t eps_num = 0, eps_den = 0, mu = 0;
        int64_t n_similar = 0, n_cores = 0, n_borders = 0, n_hubs = 0, n_outliers = 0, n_clusters = 0, largest = 0;
        double ms = 0.0, ms_similar = 0.0;   // device time of the last run | of its similarity pass (HIP events)
        bool done = false;
    } sc;

    // ---- graphlet census (graphlets.hip): arrays of their own (pool blocks), indexed like the k-truss result they were
    // computed from and dropped with it (truss_free)
    struct Graphlets {
        DevArr<unsigned long long> orbit;    // [15 * nv] orbit-major: orbit[o * nv + v], ORIGINAL ids
        DevArr<unsigned long long> cycles4;  // [t_ne] 4-cycles (induced or not) through the canonical edge
        DevArr<unsigned long long> cliques4; // [t_ne] 4-cliques through the canonical edge
        uint64_t total[KOMB_GRAPHLET_TYPES] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // induced graphlet counts, saturating
        int32_t flags = 0, max_degree = 0;
        int64_t cycle_items = 0, n_triangles = 0, n_cliques4 = 0;
        int64_t n_wave = 0, n_lds = 0, n_heavy = 0;      // roots of the 4-cycle pass by tier (option GRAPHLET_DEBUG prints them)
        double ms = 0.0, ms_cycles = 0.0, ms_tri = 0.0, ms_vertex = 0.0;   // device time of the last run | of its passes (HIP events)
        bool done = false;
    } gl;

    // ---- betweenness centrality from chosen sources (betweenness.hip): a snapshot in arrays of its own, dropped with the graph
    // (graph_free) and by nothing else
    struct Betweenness {
        DevArr<double> bc;                   // [nv] raw betweenness, ORIGINAL ids (pool block)
        std::vector<int32_t> source;         // [n_sources] the sources of the last run, in the order given
        std::vector<int64_t> n_reached, sum_dist;   // [n_sources] vertices reached (the source included) | sum of their distances
        std::vector<int32_t> ecc;            // [n_sources] the largest distance
        int32_t flags = 0, depth_max = 0;    // KOMB_BETWEENNESS_ROUNDED | the largest ecc
        int64_t n_batches = 0, n_level_steps = 0;
        int64_t visits = 0, needed = 0;      // row entries the sweeps looked at | those some lane needed (option BTW_DEBUG prints them)
        double ms = 0.0;                     // device time of the last run (HIP events)
        bool done = false;
    } btw;

    // ---- distance analysis from chosen sources (distances.hip): a snapshot in arrays of its own, dropped with the graph
    // (graph_free) and by nothing else
    struct Distances {
        DevArr<int64_t> n_reached, sum_dist; // [nv] sources that reach the vertex | sum of their distances, ORIGINAL ids (pool blocks)
        DevArr<int32_t> ecc;                 // [nv] the largest of those distances, -1 where no source reaches the vertex
        DevArr<double> harmonic;             // [nv] the harmonic sum in the order of the definition
        std::vector<int32_t> source;         // [n_sources] the sources of the last run, in the order given
        std::vector<int64_t> s_reached, s_sum_dist;   // [n_sources] vertices reached (the source included) | sum of their distances
        std::vector<int32_t> s_ecc;          // [n_sources] the largest distance
        std::vector<int64_t> pairs;          // [depth_max + 1] (source, vertex) pairs at every distance
        int32_t flags = 0, depth_max = 0, depth_min = 0;   // KOMB_DISTANCES_ALL | the largest | the smallest per-source ecc
        int64_t n_pairs = 0, sum_all = 0;    // the sum of pairs[] | of L * pairs[L]
        int64_t n_batches = 0, n_level_steps = 0;
        int64_t visits = 0, rows = 0;        // row entries the level steps looked at | the lengths of the rows they walked (option DIST_DEBUG prints them)
        int32_t words = 0;                   // 64-bit words per vertex and mask of the run (option DIST_WORDS)
        double ms = 0.0;                     // device time of the last run (HIP events)
        bool done = false;
    } dist;

    // ---- (3,4)-nucleus decomposition (nucleus.hip): arrays of their own (pool blocks), indexed like the k-truss result they were
    // computed from and dropped with it (truss_free)
    struct Nucleus {
        DevArr<int32_t> a, b, c;             // [n_tri] the triangles a < b < c in ascending (a, b, c) order, ORIGINAL ids
        DevArr<int32_t> key0;                // [n_tri + 1] the 4-cliques of the result the triangle lies in
        DevArr<int32_t> theta;               // [n_tri] its nucleus number
        DevArr<int32_t> edge;                // [t_ne] largest theta over the triangles through the canonical edge, -1 without one
        DevArr<int32_t> vertex;              // [nv] the same per vertex
        int64_t n_tri = 0, n_clq = 0, n_subrounds = 0;
        int32_t theta_max = -1, n_levels = 0;
        double ms = 0.0, ms_tri = 0.0, ms_clq = 0.0, ms_peel = 0.0;   // device time of the last run | of its passes (HIP events; option NUC_DEBUG prints them)
        bool done = false;
    } nuc;

    // ---- (3,4)-nucleus hierarchy (nucleus_hierarchy.hip): the k-nuclei as connected classes and their nesting forest over all k,
    // in pool blocks of its own, indexed like the nucleus result it was computed from and dropped with it (nucleus_drop)
    struct NucleusHierarchy {
        DevArr<int32_t> nodes;               // [5 * cap] k | rep | parent | size | shell, each a block of cap words with n_nodes in use
        DevArr<int32_t> tnode;               // [n_tri] the node of every triangle, -1 where theta == 0
        int64_t cap = 1, n_nodes = 0, n_roots = 0, n_members = 0;
        int32_t theta_max = -1, depth = 0;
        double ms = 0.0;                     // device time of the last run (HIP events)
        bool done = false;
    } nh;

    // ---- maximum-clique search (max_clique.hip): the per-vertex counts in a pool block of their own, the witness and the sorted list
    // on the host; they describe the k-truss result they were computed from and are dropped with it (truss_free)
    struct MaxClique {
        DevArr<int32_t> count;               // [nv] maximum cliques through the vertex (not enumerated: 1 on the witness)
        int32_t omega = 0, upper = 0, flags = 0, t_max = 0;
        int64_t n_max = -1, n_roots = 0, nodes = 0;
        double ms = 0.0;                     // device time of the last run (HIP events)
        std::vector<int32_t> witness;        // [omega] ascending
        std::vector<int32_t> list;           // [n_max * omega] with KOMB_MAXCLQ_LISTED: ascending tuples in lexicographic order
        bool done = false;
    } mc;

    // ---- clique census (clique_census.hip): the per-vertex counts in a pool block of their own (only with a k_local), the totals on
    // the host; they describe the k-truss result they were computed from and are dropped with it (truss_free)
    struct CliqueCensus {
        DevArr<unsigned long long> local;    // [nv] k_local-cliques through the vertex, saturating
        int32_t k_lo = 0, k_hi = 0, k_local = 0, t_max = 0, omega = 0, flags = 0, max_p = 0;
        int64_t n_roots = 0, nodes = 0;
        double ms = 0.0;                     // device time of the last run (HIP events)
        std::vector<uint64_t> total;         // [k_hi - k_lo + 1] k-cliques, saturating
        bool done = false;
    } cc;

    // ---- maximal cliques (maximal_cliques.hip): the per-vertex counts in a pool block of their own, the histogram and the sorted
    // list on the host; they describe the k-truss result they were computed from and are dropped with it (truss_free)
    struct MaximalCliques {
        DevArr<int32_t> count;               // [2 * nv] reported cliques through the vertex | the size of the largest one
        int32_t k_min = 0, k_hi = 0, t_max = 0, omega = 0, flags = 0, max_q = 0;
        int64_t n_cliques = 0, n_roots = 0, nodes = 0;
        double ms = 0.0;                     // device time of the last run (HIP events)
        std::vector<int64_t> hist;           // [k_hi - k_min + 1] maximal cliques of k_min + i vertices
        std::vector<int64_t> offset;         // [n_cliques + 1] with KOMB_MAXIMAL_LISTED: clique i is verts[offset[i], offset[i + 1])
        std::vector<int32_t> verts;          // ascending tuples in lexicographic order
        bool done = false;
    } mx;

    // ---- k-clique communities (clique_communities.hip): computed on the device, kept on the host; they describe the held list
    // of maximal cliques and are dropped with it (maximal_cliques_drop)
    struct CliqueCommunities {
        int32_t k = 0, k_min = 0;
        int64_t n_member = 0, n_comm = 0, largest = 0, n_covered = 0, n_overlap = 0, pair_tests = 0;
        double ms = 0.0;                     // device time of the last run (HIP events)
        std::vector<int32_t> label, size;    // [n_cliques of the list] the rep of the clique's community (-1) | its cliques (0)
        std::vector<int32_t> rep, n_cliques; // [n_comm] ascending reps | the cliques of the community
        std::vector<int64_t> offset;         // [n_comm + 1] community c is verts[offset[c], offset[c + 1]), ascending and distinct
        std::vector<int32_t> verts;
        std::vector<int32_t> v_comm, v_first;   // [nv] the communities through the vertex | the smallest of them (-1)
        bool done = false;
    } pc;

    // ---- k-truss results (canonical order)
    int64_t t_ne = -1;                      // edges of the (sub)graph last run
    int32_t *d_t_eu = nullptr, *d_t_ev = nullptr, *d_t_truss = nullptr, *d_t_sup = nullptr;
    uint2 *d_t_slice = nullptr;              // [t_ne] (start, length) of every internal edge's index slice: the length is the support the peel started from; komb_truss_fetch_support puts them in canonical
    uint32_t t_k_lo = 0, t_k_hi = 0;         // the canonical edges the last run materialised (komb_truss_run_slice: this rank's slice)
    bool t_sup_ready = false;                // order on its first call (d_t_sup; igraph_trussness has no such output, and the timed step does not make it)
    bool t_own_edges = false;                // d_t_eu / d_t_ev are pool blocks of this result (induced subgraph), not the graph's cached list
    int32_t *d_ceu = nullptr, *d_cev = nullptr;   // the resident graph's canonical edge list, made by the first komb_truss_fetch that asks for endpoints (pool blocks)
    bool truss_done = false;
    int slice_rank = 0, slice_world = 1;     // komb_truss_run_slice: the canonical edges whose results this run materialises
    bool shard_peel = false;                 // komb_set_shard_peel: sharded runs split the peel too (shard_dev.h)
    // what the record stream of the last k-truss run on a graph of this size turned out to need (ktruss.hip): a graph with more
    // than two triangles per edge pays the second enumeration once per graph, not once per run
    struct { int64_t nv = -1, m = -1; unsigned long long own_cap = 0, rec_cap = 0; } cap_hint;

    // ---- pinned host mirrors of the control blocks (double buffered)
    komb::PeelCtrl *h_ctrl = nullptr;        // [2]
    komb::LocalCtrl *h_local = nullptr;      // [2]
    void *h_stage = nullptr;                 // pinned landing area of the small device-to-host reads (kStageBytes)
    struct H2DStager *stager = nullptr;      // pinned staging buffers + streams of the graph upload (graph_build.hip), made on first use

    komb_stats stats{};
};

// what depends on what: the nucleus hierarchy indexes the nucleus result's triangles, the k-clique communities describe the
// held list of maximal cliques -- either goes with what it was computed from (truss_free in ktruss.hip drops both pairs and
// the other results of a k-truss result; graph_free in graph_build.hip those of the graph)
inline void nucleus_drop(komb_ctx *ctx) { ctx->nh = {}; ctx->nuc = {}; }
inline void maximal_cliques_drop(komb_ctx *ctx) { ctx->pc = {}; ctx->mx = {}; }

// every device allocation outside the pool (the resident graph, the k-core results, the graph build's scratch): hipMalloc,
// then the POISON fill when that option is set
inline hipError_t dev_malloc(komb_ctx *ctx, void **out, size_t bytes) { return ctx->pool.poison.malloc(out, bytes); }
// two arrays that only make sense together (a result's two halves, made on its first run): both or neither.  The pointers are
// published only when both exist -- a run that finds the first one set takes the second for granted.
template <class A, class B> inline hipError_t dev_malloc_pair(komb_ctx *ctx, A **a, size_t a_bytes, B **b, size_t b_bytes)
{
    void *pa = nullptr, *pb = nullptr;
    hipError_t e = dev_malloc(ctx, &pa, a_bytes);
    if (e != hipSuccess) return e;
    e = dev_malloc(ctx, &pb, b_bytes);
    if (e != hipSuccess) { (void)hipFree(pa); return e; }
    *a = (A *)pa; *b = (B *)pb;
    return hipSuccess;
}

// ---- options (komb_set_option): what the library used to read from KOMB_* environment variables.  The drop-in never sets
// any; tests and measurements do, explicitly, per context.
inline const char *ctx_opt(const komb_ctx *ctx, const char *name)
{
    const auto it = ctx->options.find(name);
    return it == ctx->options.end() ? nullptr : it->second.c_str();
}
inline bool ctx_flag(const komb_ctx *ctx, const char *name)
{
    const char *v = ctx_opt(ctx, name);
    return v && strcmp(v, "0") != 0;
}
inline uint32_t ctx_opt_u32(const komb_ctx *ctx, const char *name, uint32_t dflt)      // a count or a length: 1 .. 2^31 - 1
{
    const char *e = ctx_opt(ctx, name);
    if (!e) return dflt;
    const unsigned long v = strtoul(e, nullptr, 10);
    return v < 1 ? 1u : (v > 0x7FFFFFFFul ? 0x7FFFFFFFu : (uint32_t)v);
}
namespace komb {
inline FinishMode finish_mode(const komb_ctx *ctx, FinishMode dflt)
{
    const char *e = ctx_opt(ctx, "FINISH");
    if (e && !strcmp(e, "local")) return FIN_LOCAL;
    if (e && !strcmp(e, "lds")) return FIN_LDS;
    if (e && !strcmp(e, "none")) return FIN_NONE;
    return dflt;
}
// The fixed point costs ~ sweeps x items, the peel ~ its items once + a latency per sub-round: a remainder with more items
// than this is not handed over (the peel goes on and offers a smaller one).  Option LOCAL_ITEMS overrides.
inline uint64_t local_item_limit(const komb_ctx *ctx, uint64_t dflt)
{
    if (const char *e = ctx_opt(ctx, "LOCAL_ITEMS")) return strtoull(e, nullptr, 10);
    return dflt;
}
inline uint32_t local_density_limit(const komb_ctx *ctx, uint32_t dflt)          // items per unit above which a remainder stays with the peel (0 = no rule)
{
    if (const char *e = ctx_opt(ctx, "LOCAL_DENSITY")) return (uint32_t)strtoul(e, nullptr, 10);
    return dflt;
}
inline uint32_t local_limit(const komb_ctx *ctx, uint64_t units, uint64_t divisor)
{
    uint64_t l = units / divisor;
    if (l < 4096) l = 4096;                  // small inputs go to the fixed point whole
    if (const char *e = ctx_opt(ctx, "LOCAL_LIMIT")) l = strtoull(e, nullptr, 10);
    if (l > units) l = units;
    return (uint32_t)l;
}
} // namespace komb

// Scratch buffers of one stage: everything still owned goes back to the context's pool on scope exit.
struct DevBufs {
    komb_ctx *ctx;
    std::vector<void *> owned;
    explicit DevBufs(komb_ctx *c) : ctx(c) {}
    DevBufs(const DevBufs &) = delete;
    DevBufs &operator=(const DevBufs &) = delete;
    template <class T> hipError_t alloc(T **out, size_t count)
    {
        void *q = nullptr;
        hipError_t e = ctx->pool.get(&q, (count ? count : 1) * sizeof(T));
        if (e == hipSuccess) { owned.push_back(q); *out = (T *)q; }
        return e;
    }
    void detach(void *q)                             // the caller keeps q (a pool block it will put() back itself)
    {
        for (auto &p : owned) if (p == q) p = nullptr;
    }
    void release(void *q)
    {
        for (auto &p : owned) if (p == q && q) { ctx->pool.put(q); p = nullptr; }
    }
    ~DevBufs() { for (void *p : owned) if (p) ctx->pool.put(p); }
};

// ---- error plumbing -------------------------------------------------------
#define KOMB_FAIL(ctx, code, ...)                                   \
    do {                                                            \
        char _b[512];                                               \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                      \
        (ctx)->err = _b;                                            \
        return (code);                                              \
    } while (0)

#define KOMB_HIP(ctx, call)                                                          \
    do {                                                                             \
        hipError_t _e = (call);                                                      \
        if (_e != hipSuccess) {                                                      \
            hipError_t _nomem = hipErrorOutOfMemory;                                 \
            KOMB_FAIL(ctx, _e == _nomem ? KOMB_ERR_NOMEM : KOMB_ERR_DEVICE,          \
                      "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e),         \
                      __FILE__, __LINE__);                                           \
        }                                                                            \
    } while (0)

#define KOMB_TRY(expr)                         \
    do {                                       \
        int _s = (expr);                       \
        if (_s != KOMB_OK) return _s;          \
    } while (0)

// small blocking device-to-host read, ordered on the context's stream.  It lands in pinned memory: a copy into pageable
// memory (a variable on the caller's stack) costs 50-100 us in the runtime alone, and a step makes a dozen of them while
// the GPU waits for the host's next decision.
constexpr size_t kStageBytes = 64 << 10;
inline hipError_t d2h(komb_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (ctx->h_stage && bytes <= kStageBytes && dst != ctx->h_stage) {
        hipError_t e = hipMemcpyAsync(ctx->h_stage, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) memcpy(dst, ctx->h_stage, bytes);
        return e;
    }
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
    return e == hipSuccess ? hipStreamSynchronize(ctx->stream) : e;
}

// ---- primitives implemented in prims.hip (rocPRIM/hipCUB behind plain signatures)
namespace komb {
int prim_sort_u64(komb_ctx *ctx, uint64_t *keys, uint64_t *tmp_keys, int64_t n, int end_bit, uint64_t **sorted);
inline int key_bits(int64_t n)                            // bits that hold every value below n: the end_bit of a sort by such a field
{
    int b = 1;
    while (b < 31 && (1ll << b) < n) ++b;
    return b;
}
int prim_unique_u64(komb_ctx *ctx, const uint64_t *in, uint64_t *out, int64_t n, int64_t *n_out);
int prim_exclusive_sum_u32(komb_ctx *ctx, const uint32_t *in, uint32_t *out, int64_t n);   // out[n-1] valid; in/out may alias
int prim_exclusive_sum_u32_u64(komb_ctx *ctx, const uint32_t *in, unsigned long long *out, int64_t n);
// flag[i] = i < m && val[i] >= k for i <= m, pos[] = its exclusive sum over m + 1: pos[i] places member i, pos[m] is their number
int prim_flag_ge_scan(komb_ctx *ctx, const int32_t *val, int64_t m, int32_t k, uint32_t *flag, uint32_t *pos);
int prim_sort_pairs_desc_i64(komb_ctx *ctx, int64_t *keys, int64_t *keys_tmp, uint32_t *vals, uint32_t *vals_tmp,
                             int64_t n, int end_bit, int64_t **sorted_keys, uint32_t **sorted_vals);

int prim_sort_pairs_u32_u64(komb_ctx *ctx, uint32_t *keys, uint32_t *keys_alt, unsigned long long *vals, unsigned long long *vals_alt,
                            int64_t n, int begin_bit, int end_bit, uint32_t **sorted_keys, unsigned long long **sorted_vals);
int prim_sort_pairs_u32_u32(komb_ctx *ctx, uint32_t *keys, uint32_t *keys_alt, uint32_t *vals, uint32_t *vals_alt,
                            int64_t n, int end_bit, uint32_t **sorted_keys, uint32_t **sorted_vals);
int prim_sort_pairs_u64_u32(komb_ctx *ctx, uint64_t *keys, uint64_t *keys_alt, uint32_t *vals, uint32_t *vals_alt,
                            int64_t n, int end_bit, uint64_t **sorted_keys, uint32_t **sorted_vals);

// ---- the forest builder (forest.hip): what the three nesting forests share -- hierarchy.hip, community_hierarchy.hip and
// nucleus_hierarchy.hip.  Each brings its items, its LINK kernels and its output kernels; the header comment of forest.hip
// has the rest.
struct ForestNodes { int32_t *k, *rep, *par; uint32_t *size, *shell; };   // nodes in the order they were made / in final order
struct ForestCtl {                           // the first 16 bytes of a forest's control block (64 bytes, zeroed before every run)
    uint32_t log_n;                          // hooked items so far
    uint32_t n_nodes;                        // nodes so far
    uint32_t n_roots;                        // tail: nodes without a parent
    int32_t  depth;                          // tail: most nodes on a path from a root down
};
struct ForestState {                         // the working arrays of a run, one word per item (pool blocks of the caller)
    int32_t *parent, *log, *claimk, *cur;    // the union-find | the hook log | the level a root's node was made at | that node
    uint32_t *cnt, *seg;                     // items per root | seg[i]: where the i-th populated level's hooks start in the log
    int32_t *node;                           // out: the node of every item, in the numbering of `made`
    ForestNodes made;                        // the nodes in the order they were made
    ForestCtl *ctl;
    uint32_t cap;                            // items = entries of the log = the most nodes there can be
};
constexpr int kForestStepGrid = 2048;        // CLAIM / ADOPT: at most this many workgroups, each striding
inline int forest_bits(uint32_t levels) { int b = 1; while (b < 32 && (1u << b) < levels) ++b; return b; }
// off[k] = the first position of the ascending keys[n] with a key >= k, for k = 0 .. levels (queued; reads nothing back)
void forest_offsets(komb_ctx *ctx, uint32_t n, const uint32_t *keys, uint32_t levels, uint32_t *off);
// CLAIM + ADOPT of the li-th populated level k, queued behind its LINK launches: order[sh_b .. sh_b + sh_n) are the level's
// items, `hooks` bounds what LINK can have logged; isolated: nothing was linked, every item of the level makes its own node
void forest_level(komb_ctx *ctx, const ForestState &f, int32_t k, uint32_t li, bool isolated, const uint32_t *order, uint32_t sh_b,
                  uint32_t sh_n, uint64_t hooks);
// the tail: the n nodes of f.made into (k, rep) order in `out` (rep through rep_map when it is given), rank[made] = final
// number, roots and depth into f.ctl.  vals / vals_alt: n words each that have served.  Queued; reads nothing back.
int forest_tail(komb_ctx *ctx, DevBufs &bufs, const ForestState &f, uint32_t n, int bits, ForestNodes out, int32_t *rank,
                const int32_t *rep_map, uint32_t *vals, uint32_t *vals_alt);

// ---- stages (each in its own translation unit)
int core_run(komb_ctx *ctx, int rank = 0, int world = 1, komb_allreduce_fn fn = nullptr, void *user = nullptr, bool sharded = false);
int onion_run(komb_ctx *ctx);
int components_run(komb_ctx *ctx, int32_t kind, int32_t k);   // components.hip: kind checked, k resolved by the caller
int hierarchy_run(komb_ctx *ctx, int32_t kind);               // hierarchy.hip: kind and the results it needs checked by the caller
int communities_run(komb_ctx *ctx, int32_t k);                // communities.hip: k checked and resolved by the caller
int communities_vertices(komb_ctx *ctx);                      // communities.hip: n_comm[] and the multi-community count, made on first request
int biconnected_run(komb_ctx *ctx, int32_t k);                // biconnected.hip: k checked and resolved by the caller
int community_hierarchy_run(komb_ctx *ctx);                   // community_hierarchy.hip: the k-truss result it needs checked by the caller
int community_hierarchy_labels(komb_ctx *ctx, int32_t k, int32_t *label, int32_t *size);   // k checked and resolved by the caller; host outputs, either may be null
int structural_run(komb_ctx *ctx, int32_t eps_num, int32_t eps_den, int32_t mu);   // structural.hip: the parameters and the k-truss result it needs checked by the caller
int structural_fetch_edges(komb_ctx *ctx, int32_t *similar);  // structural.hip: similar[] of the last run as 0 | 1 words (host output)
int graphlets_run(komb_ctx *ctx);                             // graphlets.hip: the k-truss result it needs checked by the caller
int betweenness_run(komb_ctx *ctx, int64_t n_sources, const int32_t *sources);   // betweenness.hip: sources null = every vertex; checks its arguments itself
int distances_run(komb_ctx *ctx, int64_t n_sources, const int32_t *sources);     // distances.hip: sources null = every vertex; checks its arguments itself
int nucleus_run(komb_ctx *ctx);                               // nucleus.hip: the k-truss result it needs checked by the caller
int nucleus_hierarchy_run(komb_ctx *ctx);                     // nucleus_hierarchy.hip: the nucleus result it needs checked by the caller
int nucleus_hierarchy_labels(komb_ctx *ctx, int32_t k, int32_t *label, int32_t *size);   // k checked and resolved by the caller; host outputs, either may be null
int nucleus_hierarchy_nuclei(komb_ctx *ctx, int32_t k, int64_t cap, int64_t *n_nuclei, int32_t *rep, int32_t *n_triangles,
                             int32_t *n_edges, int32_t *n_vertices);   // k checked and resolved by the caller; host outputs
int max_clique_run(komb_ctx *ctx, int64_t budget);            // max_clique.hip: the k-truss result it needs and the budget checked by the caller
// clique_census.hip: the k-truss result it needs, the budget's sign and 2 <= k_lo checked by the caller, the rest of the window here (it needs t_max)
int clique_census_run(komb_ctx *ctx, int32_t k_lo, int32_t k_hi, int32_t k_local, int64_t budget);
int maximal_cliques_run(komb_ctx *ctx, int32_t k_min, int64_t budget);   // maximal_cliques.hip: the k-truss result it needs, the budget's sign and 2 <= k_min checked by the caller
// clique_communities.hip: the held list of maximal cliques (listed, k_min <= k), 2 <= k and the budget's sign checked by the caller
int clique_communities_run(komb_ctx *ctx, int32_t k, int64_t budget);
int densest_run(komb_ctx *ctx, int32_t iters);               // densest.hip: the graph, iters and the k-core result checked by the caller
int truss_run(komb_ctx *ctx, const uint8_t *vmask_host, int rank, int world, komb_allreduce_fn fn, void *user);
int merge_run(komb_ctx *ctx, const double *susp_host, int32_t *order, int32_t *side, int64_t *n_block, double *max_density);
int corea_ranks(komb_ctx *ctx, const int32_t *deg, const int32_t *core, int64_t n, double *rank_deg, double *rank_key);
int graph_from_edges(komb_ctx *ctx, int64_t nv, int64_t n_raw, const int64_t *uv);
int graph_from_csr(komb_ctx *ctx, int64_t nv, const int64_t *rowptr, const int32_t *col);
void graph_free(komb_ctx *ctx);
void stager_free(komb_ctx *ctx);
// graph_build.hip: blocking copy pageable host memory <-> device through pinned staging buffers and a few host threads (>= 32 MB; else a plain copy)
hipError_t staged_copy(komb_ctx *ctx, void *dst, const void *src, size_t bytes, bool to_device);
void warm_up(komb_ctx *ctx);                 // graph_build.hip: first kernel launch of the library + the upload's staging buffers
// truss_prep.hip: the k-truss side of a symmetric CSR (device pointers; nv vertices, ns = 2 |E| slots)
int prep_build(komb_ctx *ctx, const uint32_t *rowptr, const int32_t *col, int64_t nv, int64_t ns, TrussPrep *out);
void prep_free(komb_ctx *ctx, TrussPrep *p);
int prep_ensure(komb_ctx *ctx);              // the resident graph's preparation, built if absent (ctx->prep)
int prep_sources(komb_ctx *ctx, TrussPrep *p);   // p->osrc, made on first use
// sum d^2, sum min(d,d), max d, (unused), sum d+ + d+ of the resident graph: the roofline model's inputs (measurement only)
int graph_moments(komb_ctx *ctx, int64_t out[5]);
// the subgraph induced by a vertex mask as a symmetric CSR of its own (new ids = ranks among the kept vertices)
struct InducedCsr { int64_t nv = 0, ns = 0; uint32_t *rowptr = nullptr; int32_t *col = nullptr; int32_t *vold = nullptr; };
int induce_csr(komb_ctx *ctx, const uint8_t *vmask_host, InducedCsr *out);
void induced_free(komb_ctx *ctx, InducedCsr *g);
// the canonical edge list (eu[k], ev[k]) of a symmetric CSR, through vold (new -> original ids) when it is an induced subgraph's
int edge_list(komb_ctx *ctx, const uint32_t *rowptr, const int32_t *col, int64_t nv, const int32_t *vold, int32_t *eu, int32_t *ev);
int truss_edges_canonical(komb_ctx *ctx);      // ktruss.hip: d_t_eu / d_t_ev of the last whole-graph run (komb_truss_fetch: on the first request per graph)
void truss_free(komb_ctx *ctx);
int truss_support_canonical(komb_ctx *ctx);    // ktruss.hip: d_t_sup from d_t_slice (whole-graph runs: on the first komb_truss_fetch_support)
void peel_ctrl_pre(hipStream_t s, uint32_t *d_grp_done);
void peel_collect_ctrl(hipStream_t s, PeelCtrl *d_collect, const PeelCtrl *d_from);
void peel_ctrl_init(hipStream_t s, PeelCtrl *d_ctrl, uint32_t *d_grp_done, uint32_t units, uint32_t tail_limit = 0);
int peel_grid(int64_t units);

// Issue `launch()` in batches until the device control block reports done.
// The host never decides what a launch does: every launch reads the control
// block its predecessor finalised (SCAN or PROCESS, or nothing once done), so
// there is no host round trip per sub-round; the host only polls a copy of the
// control block one batch behind the launches it keeps queued.
template <typename F>
int drive_peel(komb_ctx *ctx, PeelCtrl *d_ctrl, int64_t units, F &&launch, int *launches_out)
{
    // launch(i) issues the launch with index i; the state says which index it expects (PeelCtrl::seq)
    // Launches per batch.  What is queued behind the launch that finishes the peel is wasted (a launch that finds nothing to do
    // is ~5 us, and the host sees `done` one batch late): on average 1.5 batches.  The first batch is long (the giant steps of
    // the first levels keep the GPU busy while the host queues); the next few are short, because the graphs this path is
    // measured on hand over to a finish after 35-50 launches (C3: 37 of 72 launches did something with batches of 24; C2
    // k-core: 41 of 72); a peel that is still running after those has thousands of sub-rounds to go and gets long batches.
#ifndef KOMB_PEEL_BATCH
#define KOMB_PEEL_BATCH 24
#endif
#ifndef KOMB_PEEL_BATCH_SHORT
#define KOMB_PEEL_BATCH_SHORT 6
#endif
    constexpr int kBatch = KOMB_PEEL_BATCH, kBatchShort = KOMB_PEEL_BATCH_SHORT, kShortBatches = 6;
    PeelCtrl first;
    KOMB_HIP(ctx, d2h(ctx, &first, d_ctrl, sizeof(PeelCtrl)));
    int32_t next = first.seq;
#ifdef KOMB_DEBUG_SWITCHES
    if (const char *tr = getenv("KOMB_PEEL_TRACE")) {
        // debug: one launch at a time; append "mode level round light heavy live_mode live_count remaining us" per step
        FILE *f = fopen(tr, "a");
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
            if (f) fclose(f);
            if (a) (void)hipEventDestroy(a);
            KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "peel trace: hipEventCreate failed");
        }
        int launches = 0;
        if (f) fprintf(f, "# peel units=%lld\n", (long long)units);
        for (int64_t i = 0; i < 4 * units + 4096; ++i) {
            PeelCtrl before;
            if (d2h(ctx, &before, d_ctrl, sizeof(PeelCtrl)) != hipSuccess) break;
            if (before.done) break;
            (void)hipEventRecord(a, ctx->stream);
            launch(before.seq); ++launches;
            (void)hipEventRecord(b, ctx->stream);
            (void)hipEventSynchronize(b);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, a, b);
            if (f) fprintf(f, "%d %d %d %u %u %d %u %u %.1f\n", before.mode, before.level, before.round, before.cur_light,
                           before.cur_heavy, before.live_mode, before.live_count, before.remaining, ms * 1000.f);
        }
        if (f) fclose(f);
        (void)hipEventDestroy(a); (void)hipEventDestroy(b);
        if (launches_out) *launches_out = launches;
        KOMB_HIP(ctx, d2h(ctx, &ctx->h_ctrl[0], d_ctrl, sizeof(PeelCtrl)));
        return KOMB_OK;
    }
#endif
    EventSet evs;
    hipEvent_t ev[2] = {nullptr, nullptr};
    KOMB_HIP(ctx, evs.make(&ev[0], hipEventDisableTiming));
    KOMB_HIP(ctx, evs.make(&ev[1], hipEventDisableTiming));
    const int64_t max_batches = (4 * units + 4096) / kBatch + 16 + kShortBatches;   // > 2 launches per unit: cannot be reached
    int launches = 0, slot = 0, status = KOMB_OK;
    bool have_prev = false, finished = false, stuck = false;
    int32_t seen_seq = first.seq - 1;
    for (int64_t batch = 0; batch < max_batches && !finished; ++batch) {
        const int nb = (batch >= 1 && batch <= kShortBatches) ? kBatchShort : kBatch;
        for (int i = 0; i < nb; ++i) { launch(next); ++next; ++launches; }
        if (hipMemcpyAsync(&ctx->h_ctrl[slot], d_ctrl, sizeof(PeelCtrl), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipEventRecord(ev[slot], ctx->stream) != hipSuccess) { status = KOMB_ERR_DEVICE; break; }
        if (have_prev) {
            if (hipEventSynchronize(ev[slot ^ 1]) != hipSuccess) { status = KOMB_ERR_DEVICE; break; }
            const PeelCtrl &h = ctx->h_ctrl[slot ^ 1];
            if (h.done) finished = true;
            else if (h.seq == seen_seq) { stuck = true; finished = true; }   // a whole batch of launches moved nothing
            seen_seq = h.seq;
        }
        have_prev = true;
        slot ^= 1;
    }
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (launches_out) *launches_out = launches;
    if (status != KOMB_OK || e != hipSuccess)
        KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "peel driver: HIP failure (%s)", hipGetErrorString(e));
    if (d2h(ctx, &ctx->h_ctrl[0], d_ctrl, sizeof(PeelCtrl)) != hipSuccess)
        KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "peel driver: control block readback failed");
    if (!ctx->h_ctrl[0].done)
        KOMB_FAIL(ctx, KOMB_ERR_DEVICE, "peel driver: %s (level %d, remaining %u, launch %d of state %d)",
                  stuck ? "the launches make no progress" : "launch budget exhausted before completion",
                  ctx->h_ctrl[0].level, ctx->h_ctrl[0].remaining, (int)next, (int)ctx->h_ctrl[0].seq);
    return KOMB_OK;
}
} // namespace komb
