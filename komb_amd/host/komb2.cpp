// komb2.cpp -- drop-in `komb2` for KOMB.py (reference CLI: src/komb2.cpp:16-150).
//
// Same flags, same stdout lines, same files in -o (edgelist.txt, kcore.tsv,
// CoreA_anomaly.txt, optionally truss_unitigs.fasta), same exit codes, so
// KOMB.py's RunKOMB (KOMB.py:435-462) drives it unchanged.  The host builds the
// unitig graph from the two SAM files the way the reference does
// (src/graph.cpp:166-393) and hands the raw vertex pairs to the MI355X library
// through the C ABI of include/komb_accel.h; all decomposition arithmetic
// (simplify, degree, coreness, trussness, CoreA ranks) runs in HIP kernels.
// There is no CPU fallback: without a GPU the program exits non-zero.
//
// Environment knobs (KOMB.py passes a fixed argv, so extras are env vars):
//   KOMB_V1_OUTPUTS=1   re-enable combineFile and splitAnomalousUnitigs (commented out at
//                       src/komb2.cpp:126,139): combined.fasta, top_/low_scoring_anomalous_unitigs.txt,
//                       reference quirks kept; "fixed" = per-vertex decision and unitig names
//   KOMB_V1_ONLY=1      only those two stages, from the kcore.tsv + CoreA_anomaly.txt already in -o
//   KOMB_TRUSS=1        re-enable the runTruss stage the reference has commented
//                       out at src/graph.cpp:478 (writes truss_unitigs.fasta)
//   KOMB_ONION=1        also write onion.tsv after kcore.tsv: #VID, Name, Coreness, Layer (the onion decomposition's
//                       peel layer of every unitig, include/komb_accel.h); nothing else changes
//   KOMB_COMPONENTS=<k>|max   also write core_components.tsv after kcore.tsv (and onion.tsv): #VID, Name, Coreness,
//                       Component, Size -- one row per unitig of coreness >= k (max: the largest coreness) in VID
//                       order; Component is the Name of the member with the smallest VID of the unitig's connected
//                       component in that k-core, Size its number of unitigs (komb_components_run).  VIDs depend on
//                       -t, so only the partition by Name compares between runs.  With KOMB_TRUSS=1 also
//                       truss_components.tsv (Trussness = the threshold in place of Coreness): the records of
//                       truss_unitigs.fasta split into components.  Nothing else changes.
//   KOMB_COMMUNITIES=<k>|max  with KOMB_TRUSS=1: also write, after the truss stage, the k-truss communities of its result
//                       (komb_truss_communities_run: the classes of the edges of trussness >= k, max: the largest
//                       trussness, under "two sides of a triangle of such edges").  truss_communities.tsv: #VID_U,
//                       Name_U, VID_V, Name_V, Trussness, Community, Size -- one row per member edge in canonical
//                       order, Community numbering the communities from 0 in the order of their first edge, Size the
//                       community's number of edges.  truss_community_vertices.tsv: #VID, Name, Communities -- the
//                       unitigs with a member edge and the number of communities they belong to (more than one: a
//                       unitig shared between dense regions).  Nothing else changes.
//   KOMB_BICONNECTED=<k>|max  with KOMB_TRUSS=1: also write, after the truss stage, the biconnected components of the WHOLE
//                       graph's k-truss (a k-truss run of its own, made once the stage and its tables are done, and
//                       komb_biconnected_run on its edges of trussness >= k, max: the largest trussness; the stage's own
//                       subject is the max core, one dense piece; what holds the assembly graph together shows on the
//                       whole graph).
//                       truss_blocks.tsv: #VID_U, Name_U, VID_V, Name_V, Trussness, Block, Size, Bridge -- one row per
//                       member edge in canonical order, Block numbering the blocks from 0 in the order of their first
//                       edge, Size the block's number of edges, Bridge 1 for an adjacency whose loss separates its two
//                       unitigs (a block of one edge), else 0.  truss_articulation.tsv: #VID, Name, Blocks, Articulation,
//                       Component2E, Size2E -- one row per unitig with a member edge in VID order: the blocks it lies in,
//                       1 when its loss separates the graph (more than one block), the Name of the smallest-VID unitig of
//                       its 2-edge-connected component (what stays connected once the bridges are removed) and that
//                       component's number of unitigs.  VIDs depend on -t, so only the tables by Name compare between
//                       runs.  Nothing else changes.
//   KOMB_DENSEST=<rounds>   also write, after kcore.tsv, the densest subgraph komb_densest_subgraph_run(rounds) finds on
//                       the coreness: densest_subgraph.tsv -- #VID, Name, Coreness, Load, members only, in VID order -- and
//                       core_density.tsv -- #K, Vertices, Edges, the vertices of coreness >= K and the edges between two
//                       of them, one row per K.
//   KOMB_HIERARCHY=1    also write, after kcore.tsv, the nesting forest of the k-core components over all k
//                       (komb_hierarchy_run).  core_hierarchy.tsv: #Node, K, Rep, Parent, Size, Shell -- one row per node
//                       in node order (ascending K, then the VID of Rep); Rep is the Name of the unitig with the smallest
//                       VID in the node, Parent a node index or -1, Size the node's number of unitigs, Shell those of
//                       coreness exactly K among them.  core_hierarchy_vertices.tsv: #VID, Name, Coreness, Node -- every
//                       unitig in VID order with the node it belongs to at its own coreness.  With KOMB_TRUSS=1 also
//                       truss_hierarchy.tsv and truss_hierarchy_vertices.tsv (#VID, Name, Trussness, Node) for the truss
//                       stage's result: the unitigs with an edge in it, Trussness the largest of their edges.  VIDs depend
//                       on -t, so only the forest by Name compares between runs.  Nothing else changes.
//   KOMB_COMMUNITY_HIERARCHY=1  with KOMB_TRUSS=1: also write, after the truss stage, the nesting forest of the k-truss
//                       communities of its result over all k (komb_community_hierarchy_run).
//                       truss_community_hierarchy.tsv: #Node, K, Rep_U, Rep_V, Parent, Size, Shell -- one row per node in
//                       node order; Rep_U and Rep_V are the Names of the unitigs of the node's first edge in canonical
//                       order, Parent a node index or -1, Size the node's number of edges, Shell those of trussness exactly
//                       K among them.  truss_community_hierarchy_edges.tsv: #VID_U, Name_U, VID_V, Name_V, Trussness, Node
//                       -- one row per edge of trussness >= 3 in canonical order with the node it belongs to at its own
//                       trussness.  VIDs depend on -t, so only the forest by Name compares between runs.  Nothing else
//                       changes.
//   KOMB_STRUCTURAL=<num>/<den>,<mu>  (for example 7/10,3) also write structural_clusters.tsv: the structural clustering
//                       (komb_structural_clusters_run, eps = num/den, mu) of a whole-graph k-truss run of its own, made
//                       before the KOMB_TRUSS stage, which then runs on the max core exactly as without it.  #VID, Name,
//                       Role, Cluster, ClusterSize, SimilarNeighbours -- one row per unitig in VID order; Role is core,
//                       border, hub or outlier; Cluster the Name of the unitig with the smallest VID among the cluster's
//                       cores, or - for a hub / an outlier; ClusterSize its number of unitigs (0 then);
//                       SimilarNeighbours the unitig's number of similar edges.  VIDs depend on -t, so only the
//                       partition by Name compares between runs.  Nothing else changes.
//   KOMB_GRAPHLETS=1|edges  also write the graphlet census (komb_graphlets_run) of a whole-graph k-truss run of its own, made
//                       before the KOMB_TRUSS stage, which then runs on the max core exactly as without it.
//                       graphlet_orbits.tsv: #VID, Name, O0 .. O14 -- one row per unitig in VID order, the induced 3- and
//                       4-vertex subgraphs it lies in by orbit (Przulj's numbering).  graphlet_census.tsv: #Graphlet, Count
//                       -- edge, wedge, triangle, path4, claw, cycle4, paw, diamond, clique4.  With edges also
//                       graphlet_edges.tsv: #U, V, Triangles, Cycles4, Cliques4 -- one row per edge in canonical order, the
//                       unitigs by Name.  Any other value is a usage error.  VIDs depend on -t, so only the tables by Name
//                       compare between runs.  Nothing else changes.
//   KOMB_BETWEENNESS=all|<n>[:<seed>]  also write the betweenness centrality (komb_betweenness_run, Brandes' algorithm) of the
//                       whole graph from every unitig, or from a sample: the n unitigs with the smallest
//                       splitmix64(seed ^ VID), ties by VID, passed in ascending VID (seed defaults to 1; n >= the number of
//                       unitigs is all).  betweenness.tsv: #VID, Name, Betweenness -- one row per unitig in VID order, the raw
//                       value (neither halved nor normalised; from every unitig it is twice igraph's) printed with %.17g, which
//                       reads back to the same binary64.  betweenness_sources.tsv: #VID, Name, Reached, SumDist, Ecc -- one
//                       row per source in the order passed: the unitigs it reaches (itself included), the sum of their
//                       distances and the largest.  Any other value is a usage error.  Nothing else changes.
//   KOMB_DISTANCES=all|<n>[:<seed>]  also write the distance analysis (komb_distances_run) of the whole graph from every
//                       unitig, or from the sample that the same value of KOMB_BETWEENNESS names.  distances.tsv: #VID, Name,
//                       Reached, SumDist, Ecc, Harmonic -- one row per unitig in VID order: the sources that reach it, the sum
//                       of their distances, the largest (-1 when none reaches it) and the harmonic sum, printed with %.17g,
//                       which reads back to the same binary64.  distance_sources.tsv: #VID, Name, Reached, SumDist, Ecc -- one
//                       row per source in the order passed, as in betweenness_sources.tsv.  distance_histogram.tsv: #Distance,
//                       Pairs -- the (source, unitig) pairs at every distance from 0 to the largest.  Any other value is a
//                       usage error.  Nothing else changes.
//   KOMB_NUCLEUS=1      with KOMB_TRUSS=1: also write, after the truss stage, the (3,4)-nucleus decomposition of its result
//                       (komb_nucleus_run: triangles peeled by the 4-cliques they lie in).  nucleus_triangles.tsv:
//                       #Name_A, Name_B, Name_C, Cliques, Theta -- one row per triangle in triangle order (ascending VIDs),
//                       Cliques the 4-cliques it lies in, Theta its nucleus number.  nucleus_unitigs.tsv: #VID, Name, Theta
//                       -- the unitigs of the result in VID order with the largest Theta among their triangles (-1 without
//                       one).  0 is off; any other value than 0 or 1 is a usage error.  VIDs depend on -t, so only the tables
//                       by Name compare between runs.  Nothing else changes.
//   KOMB_NUCLEUS_HIERARCHY=1  with KOMB_TRUSS=1: also write, after the truss stage, the (3,4)-nuclei of its result as connected
//                       classes and their nesting forest over all k (komb_nucleus_hierarchy_run; it runs komb_nucleus_run
//                       itself when KOMB_NUCLEUS=1 has not).  nucleus_hierarchy.tsv: #Node, Theta, Rep_A, Rep_B, Rep_C, Parent,
//                       Triangles, Shell, Edges, Vertices -- one row per node in node order; Rep_A, Rep_B, Rep_C are the Names
//                       of the unitigs of the node's first triangle in triangle order, Parent a node index or -1, Triangles
//                       the node's number of triangles, Shell those of nucleus number exactly Theta among them, Edges and
//                       Vertices the distinct edges and unitigs of its triangles (komb_nucleus_hierarchy_nuclei, one call per
//                       populated level).  nucleus_hierarchy_triangles.tsv: #Name_A, Name_B, Name_C, Theta, Node -- one row
//                       per triangle of nucleus number >= 1 in triangle order with the node it belongs to at its own Theta.
//                       0 is off; any other value than 0 or 1 is a usage error.  VIDs depend on -t, so only the forest by
//                       Name compares between runs.  Nothing else changes.
//   KOMB_MAX_CLIQUE=1|<budget>  with KOMB_TRUSS=1: also write, after the truss stage, the maximum cliques of its result
//                       (komb_max_clique_run; 1 is the default node budget, a larger number is the budget itself).
//                       max_cliques.tsv: a header comment "# omega <n> upper <n> flags <n> cliques <n>", then one line per
//                       maximum clique in list order, the Names of its unitigs in ascending VID order, tab separated -- or
//                       the witness alone when the list is not held (flags without 4).  max_clique_unitigs.tsv: #Name, Count
//                       -- the unitigs in VID order that lie in at least one maximum clique, with their number (1 on the
//                       witness when the cliques were not enumerated).  0 is off; anything else is a usage error.  VIDs depend
//                       on -t, so only the cliques as sets of Names compare between runs.  Nothing else changes.
//   KOMB_CLIQUE_CENSUS=<k_lo>:<k_hi>[:<k_local>]  with KOMB_TRUSS=1: also write, after the truss stage, the clique census of its
//                       result (komb_clique_census_run with the default node budget): the number of k-cliques for every k of
//                       the window; <k_hi> may be "max" (the largest trussness).  clique_census.tsv: a header comment
//                       "# k_lo <n> k_hi <n> k_local <n> flags <n> omega <n> nodes <n> roots <n>" (k_hi as used), then one
//                       line k<TAB>count per k.  With a <k_local> also clique_census_unitigs.tsv: #Name, Count -- every unitig
//                       in VID order with the number of k_local-cliques it lies in.  Counts saturate at 2^64 - 1 (flags 2).
//                       0 or empty is off; anything else that is not of that form is a usage error.  Nothing else changes.
//   KOMB_MAXIMAL_CLIQUES=<k_min>[:<budget>]  with KOMB_TRUSS=1: also write, after the truss stage, the maximal cliques of at least
//                       <k_min> >= 2 unitigs of its result (komb_maximal_cliques_run; without <budget> the default node budget).
//                       maximal_cliques.tsv: a header comment "# k_min <n> flags <n> omega <n> cliques <n> nodes <n> roots <n>",
//                       then one line per clique in list order: its size and the Names of its unitigs in ascending VID order,
//                       tab separated -- the header alone when the list is not held (flags without 2).
//                       maximal_clique_sizes.tsv: one line size<TAB>count per size from k_min to max(k_min, the largest
//                       trussness).  maximal_clique_unitigs.tsv: #Name, Count, Largest -- the unitigs in VID order that lie in
//                       at least one reported clique, with their number and the size of the largest.  0 or empty is off;
//                       anything else that is not of that form is a usage error.  VIDs depend on -t, so only the cliques as
//                       sets of Names compare between runs.  Nothing else changes.
//   KOMB_CLIQUE_COMMUNITIES=<k>[:<budget>]  with KOMB_TRUSS=1: also write, after the truss stage, the k-clique communities of its
//                       result, k >= 2 (komb_clique_communities_run: clique percolation over the maximal cliques of at least
//                       <k> unitigs; without <budget> the default cap on pair tests).  The maximal cliques are those of
//                       KOMB_MAXIMAL_CLIQUES when that ran with a k_min <= k, else of a komb_maximal_cliques_run(k, default
//                       budget) made for this.  clique_communities.tsv: a header comment "# k <n> communities <n>
//                       member_cliques <n> covered <n> overlap <n> pair_tests <n>", then one line per community: its number,
//                       its cliques, its unitigs and the Names of its unitigs in ascending VID order, tab separated.
//                       clique_community_unitigs.tsv: #Name, Communities, First -- the unitigs in VID order that lie in at
//                       least one community, with their number of communities and the smallest community number.  0 or empty
//                       is off; anything else that is not of that form is a usage error.  Nothing else changes.
//   KOMB_STRICT_SAM=1   parse every SAM line (the reference drops the line that
//                       straddles each OpenMP byte-chunk boundary, see readSAM)
//   KOMB_DEVICE=<n>     HIP device ordinal (default 0)
//   KOMB_HOST_TIMES=1   stage times of the SAM -> edge list pipeline on stderr
//   KOMB_STOP_AFTER_EDGES=1  write edgelist.txt + vertex_names.txt and stop
//                       before touching the device (host-logic tests)
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <ctime>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include <omp.h>
#include <parallel/algorithm>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "komb_accel.h"

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t0) { return std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - t0).count() / 1000000.0; }

// The HIP context is created on a second thread beside the SAM parse.  A fatal exit on the main thread first waits for
// that thread (and drops the context): exit() runs the static destructors, and the HIP runtime must not be torn down
// under a thread that is still initialising it.
std::future<komb_ctx *> *g_ctx_early = nullptr;
[[noreturn]] void leave(int code)
{
    if (g_ctx_early && g_ctx_early->valid()) {
        komb_ctx *c = g_ctx_early->get();
        if (c) komb_destroy(c);
    }
    exit(code);
}

[[noreturn]] void file_not_found(const std::string &path)
{
    // src/graph.cpp:58-61
    fprintf(stderr, "File %s could not be opened. Exiting...\n", path.c_str());
    leave(EXIT_FAILURE);
}

[[noreturn]] void parse_error(const char *prog, const std::string &what)
{
    // TCLAP StdOutput::failure (external/tclap/StdOutput.h:131-153): message on stderr, exit(1)
    fprintf(stderr, "PARSE ERROR: %s\n\nBrief USAGE: \n   %s  -i <string> -j <string> -u <string> [-l <int>] [-t <int>] [-o <string>] [-f] [--] [--version] [-h]\n\nFor complete USAGE and HELP type: \n   %s --help\n\n",
            what.c_str(), prog, prog);
    exit(1);
}

void usage(const char *prog)
{
    printf("\nUSAGE: \n\n   %s  -i <string> -j <string> -u <string> [-l <int>] [-t <int>] [-o <string>] [-f]\n"
           "          [--] [--version] [-h]\n\nWhere: \n\n"
           "   -i <string>,  --input <string>\n     (required)  Input SAM file [Default: alingment1.sam]\n\n"
           "   -j <string>,  --input2 <string>\n     (required)  Second input SAM file [Default: alignment2.sam]\n\n"
           "   -u <string>,  --input-unitigs <string>\n     (required)  FASTA file containing unitigs [Default: unitigs.fa]\n\n"
           "   -l <int>,  --readlen <int>\n     Read Length (can be average) [Default: 151]\n\n"
           "   -t <int>,  --threads <int>\n     Number of Threads [Default: Max]\n\n"
           "   -o <string>,  --output <string>\n     Output directory [Default: output_yyyymmdd_hhmmss]\n\n"
           "   -f,  --fulgor\n     Use Fulgor pseudoalignments instead of SAM files\n\n"
           "   --,  --ignore_rest\n     Ignores the rest of the labeled arguments following this flag.\n\n"
           "   --version\n     Displays version information and exits.\n\n"
           "   -h,  --help\n     Displays usage information and exits.\n\n\n"
           "   KOMB: Taxonomy-oblivious characterization of metagenome dynamics\n\n", prog);
}

struct Args {
    std::string input, input2, unitigs, outdir;
    int readlen = 151, threads = 1;
    bool fulgor = false;
};

Args parse_args(int argc, const char **argv)
{
    Args a;
    a.threads = omp_get_max_threads();                     // src/komb2.cpp:24
    time_t now = time(nullptr);
    tm *t = localtime(&now);                               // src/komb2.cpp:27-32: unpadded fields
    a.outdir = "output_" + std::to_string(1900 + t->tm_year) + std::to_string(1 + t->tm_mon) + std::to_string(t->tm_mday) +
               "_" + std::to_string(t->tm_hour) + std::to_string(t->tm_min) + std::to_string(t->tm_sec);
    const char *prog = "komb2";
    bool have_i = false, have_j = false, have_u = false;
    auto need_value = [&](int &k, const std::string &flag) -> std::string {
        if (k + 1 >= argc) parse_error(prog, "Argument: " + flag + "\n             Missing a value for this argument!");
        return argv[++k];
    };
    auto to_int = [&](const std::string &v, const std::string &flag) -> int {
        char *end = nullptr;
        long x = strtol(v.c_str(), &end, 10);
        if (v.empty() || *end != '\0') parse_error(prog, "Argument: " + flag + "\n             Couldn't read argument value from string '" + v + "'");
        return (int)x;
    };
    for (int k = 1; k < argc; ++k) {
        std::string s = argv[k];
        if (s == "--") break;                              // --ignore_rest
        if (s == "-h" || s == "--help") { usage(prog); exit(0); }            // HelpVisitor.h:70
        if (s == "--version") { printf("\n%s  version: 2.0\n\n", prog); exit(0); } // VersionVisitor.h:74
        if (s == "-i" || s == "--input") { a.input = need_value(k, "-i (--input)"); have_i = true; }
        else if (s == "-j" || s == "--input2") { a.input2 = need_value(k, "-j (--input2)"); have_j = true; }
        else if (s == "-u" || s == "--input-unitigs") { a.unitigs = need_value(k, "-u (--input-unitigs)"); have_u = true; }
        else if (s == "-l" || s == "--readlen") a.readlen = to_int(need_value(k, "-l (--readlen)"), "-l (--readlen)");   // "-l -1" is a value
        else if (s == "-t" || s == "--threads") a.threads = to_int(need_value(k, "-t (--threads)"), "-t (--threads)");
        else if (s == "-o" || s == "--output") a.outdir = need_value(k, "-o (--output)");
        else if (s == "-f" || s == "--fulgor") a.fulgor = true;
        else parse_error(prog, "Argument: " + s + "\n             Couldn't find match for argument");
    }
    if (!have_i) parse_error(prog, "Required argument missing: input");
    if (!have_j) parse_error(prog, "Required argument missing: input2");
    if (!have_u) parse_error(prog, "Required argument missing: input-unitigs");
    if (a.threads < 1) a.threads = 1;
    return a;
}

// ---------------------------------------------------------------------- SAM
// SAM -> graph pipeline (reference: readSAM src/graph.cpp:166-257, getEdgeInfo :259-285,
// generateGraph :287-393).  Same observable result -- vertex = unitig name seen on a parsed
// line, edge = two unitigs sharing a read key in either file -- built without per-read string
// hash sets: both files are mmap'ed, every thread parses the lines of its own byte chunk into
// (read-key view, unitig id) records, records are sorted by read key (64-bit hash first,
// bytes on a tie, so grouping is exact), each run of equal keys is one clique, and the
// expanded pairs are deduplicated by sort + unique.
struct Mapped {
    const char *data = nullptr;
    size_t size = 0;
    std::string fallback;                                  // used when mmap is not possible
    void open(const std::string &path)
    {
        int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) file_not_found(path);
        struct stat st;
        if (fstat(fd, &st) != 0) { ::close(fd); file_not_found(path); }
        size = (size_t)st.st_size;
        if (size == 0) { ::close(fd); data = ""; return; }
        void *p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (p == MAP_FAILED) {
            fallback.resize(size);
            size_t got = 0;
            while (got < size) {
                ssize_t r = ::read(fd, &fallback[got], size - got);
                if (r <= 0) { fprintf(stderr, "Encountered error while reading %s\n", path.c_str()); leave(EXIT_FAILURE); }   // src/graph.cpp:188-192
                got += (size_t)r;
            }
            data = fallback.data();
        } else {
            data = (const char *)p;
            madvise(p, size, MADV_SEQUENTIAL);
        }
        ::close(fd);
    }
    ~Mapped() { if (data && fallback.empty() && size) munmap((void *)data, size); }
};

struct View { const char *p; uint32_t n; };
inline bool operator==(const View &a, const View &b) { return a.n == b.n && memcmp(a.p, b.p, a.n) == 0; }
struct ViewHash {
    size_t operator()(const View &v) const
    {
        uint64_t h = 0xCBF29CE484222325ull;                // FNV-1a, then a final mix
        for (uint32_t i = 0; i < v.n; ++i) { h ^= (unsigned char)v.p[i]; h *= 0x100000001B3ull; }
        h ^= h >> 32; h *= 0x9E3779B97F4A7C15ull; h ^= h >> 29;
        return (size_t)h;
    }
};

struct Names {                                             // unitig name <-> vid (src/graph.cpp:242-256)
    std::vector<std::string> name;                         // vid order = first appearance (file, then byte offset)
};

struct Rec {                                               // one parsed alignment line
    uint64_t hash;                                         // of the read key
    View key;                                              // read.substr(1, read.find('/')) (src/graph.cpp:235)
    int32_t vid;                                           // thread-local unitig id, later the global vid
};

// Which lines does the reference parse?  readSAM (src/graph.cpp:195-238) splits the BYTES of the
// file over T OpenMP threads (static schedule: the first n mod T threads get ceil(n/T) bytes, the
// rest floor(n/T)); each thread records the newlines inside its own chunk and parses only the lines
// that lie between two of its own newlines (thread 0 also gets a synthetic newline before byte 0).
// The line that starts after a chunk's last newline is parsed by nobody, and neither is a final
// line without '\n'.  strict = every line.  Calls f(begin, end) for every parsed line of chunk t.
template <class F>
void for_lines_of_chunk(const char *buf, size_t n, int T, int t, bool strict, F &&f)
{
    const size_t q = n / (size_t)T, r = n % (size_t)T;
    const size_t lo = (size_t)t * q + std::min((size_t)t, r), hi = lo + q + ((size_t)t < r ? 1 : 0);
    if (strict) {
        // every line belongs to the chunk that holds its first byte
        size_t b = lo;
        if (lo > 0) { while (b < n && buf[b - 1] != '\n' && buf[b - 1] != '\0') ++b; }
        while (b < hi && b < n) {
            size_t e = b;
            while (e < n && buf[e] != '\n' && buf[e] != '\0') ++e;
            if (e > b) f(b, e);
            b = e + 1;
        }
        return;
    }
    bool have_prev = (t == 0);                             // thread 0: position[0] = {0}
    size_t prev = 0;
    for (size_t i = lo; i < hi; ++i) {
        if (buf[i] == '\n' || buf[i] == '\0') {
            if (have_prev) {
                size_t start = prev + 1;
                if (start == 1) start = 0;                 // src/graph.cpp:218-219
                f(start, i);
            }
            prev = i; have_prev = true;
        }
    }
}

struct ThreadParse {
    std::vector<Rec> recs;
    std::unordered_map<View, int32_t, ViewHash> local;     // unitig name -> local id
    std::vector<View> local_names;
    std::vector<uint64_t> local_hash;                      // ViewHash of local_names[i]
    std::vector<uint64_t> first_pos;                       // (file << 48 | byte offset) of the first line naming it
};

void parse_sam(const Mapped &m, int file_idx, int threads, bool strict, std::vector<ThreadParse> &tp)
{
#pragma omp parallel for num_threads(threads) schedule(static, 1)
    for (int t = 0; t < threads; ++t) {
        ThreadParse &me = tp[(size_t)t];
        for_lines_of_chunk(m.data, m.size, threads, t, strict, [&](size_t b, size_t e) {
            const char *line = m.data + b;
            const size_t len = e - b;
            if (len == 0 || line[0] == '@') return;        // header (src/graph.cpp:221)
            // strtok_r(line, "\t"): empty fields are skipped; field 0 = QNAME, field 2 = RNAME
            size_t pos = 0;
            const char *tok[3] = {nullptr, nullptr, nullptr};
            size_t tlen[3] = {0, 0, 0};
            int nt = 0;
            while (nt < 3 && pos < len) {
                while (pos < len && line[pos] == '\t') ++pos;
                if (pos >= len) break;
                const char *tb = line + pos;
                const char *te = (const char *)memchr(tb, '\t', len - pos);
                const size_t l = te ? (size_t)(te - tb) : len - pos;
                tok[nt] = tb; tlen[nt] = l; ++nt;
                pos += l;
            }
            if (nt < 3) return;                            // the reference would dereference NULL here
            if (tlen[2] == 1 && tok[2][0] == '*') return;  // unmapped (src/graph.cpp:233)
            // key = read.substr(1, read.find('/')): drop the first char, keep through the first '/'
            View key{tok[0], 0};
            if (tlen[0] >= 1) {
                const char *sl = (const char *)memchr(tok[0], '/', tlen[0]);
                const size_t cnt = sl ? (size_t)(sl - tok[0]) : std::string::npos;        // find('/')
                const size_t avail = tlen[0] - 1;
                key.p = tok[0] + 1;
                key.n = (uint32_t)std::min(avail, cnt);
            }
            const View nm{tok[2], (uint32_t)tlen[2]};
            auto it = me.local.find(nm);
            int32_t lid;
            if (it == me.local.end()) {
                lid = (int32_t)me.local_names.size();
                me.local.emplace(nm, lid);
                me.local_names.push_back(nm);
                me.local_hash.push_back((uint64_t)ViewHash{}(nm));
                me.first_pos.push_back(((uint64_t)file_idx << 48) | (uint64_t)b);
            } else lid = it->second;
            me.recs.push_back(Rec{(uint64_t)ViewHash{}(key), key, lid});
        });
    }
}

// Parses both files and returns the raw (u,v) vertex pairs of all cliques, deduplicated.
std::vector<int64_t> build_edges(const std::string &path1, const std::string &path2, int threads, bool strict, Names &names,
                                 double *t_sam, double *t_merge, double *t_expand)
{
    const auto t0 = clk::now();
    Mapped m1, m2;
    m1.open(path1);                                        // src/komb2.cpp:93
    m2.open(path2);                                        // src/komb2.cpp:95
    std::vector<ThreadParse> tp1((size_t)threads), tp2((size_t)threads);
    const bool host_times = getenv("KOMB_HOST_TIMES") != nullptr;
    auto lap = [&, last = clk::now()](const char *what) mutable {
        if (host_times) fprintf(stderr, "komb2 host: %-28s %.3f s\n", what, since(last));
        last = clk::now();
    };
    lap("mmap");
    parse_sam(m1, 0, threads, strict, tp1);
    parse_sam(m2, 1, threads, strict, tp2);
    lap("parse both SAM files");
    // global vid = order of first appearance (file 1 before file 2, then byte offset): independent of T in strict mode.
    // Every thread has met most of the unitigs, so the per-thread dictionaries hold T x |V| names in total;
    // merging them serially was the largest single cost of the pipeline.  The names are partitioned by hash
    // instead: bucket b takes the names with hash % B == b from every dictionary, all buckets in parallel.
    std::vector<ThreadParse *> all;
    for (auto *tp : {&tp1, &tp2}) for (auto &th : *tp) all.push_back(&th);
    const size_t B = (size_t)threads * 4;
    std::vector<std::unordered_map<View, uint64_t, ViewHash>> bucket(B);      // name -> first position, later -> vid
#pragma omp parallel for num_threads(threads) schedule(dynamic, 1)
    for (size_t b = 0; b < B; ++b) {
        auto &m = bucket[b];
        for (ThreadParse *th : all)
            for (size_t i = 0; i < th->local_names.size(); ++i) {
                if (th->local_hash[i] % B != b) continue;
                auto ins = m.emplace(th->local_names[i], th->first_pos[i]);
                if (!ins.second && th->first_pos[i] < ins.first->second) ins.first->second = th->first_pos[i];
            }
    }
    lap("merge unitig dictionaries");
    std::vector<size_t> boff(B + 1, 0);
    for (size_t b = 0; b < B; ++b) boff[b + 1] = boff[b] + bucket[b].size();
    std::vector<std::pair<uint64_t, View>> order(boff[B]);
#pragma omp parallel for num_threads(threads) schedule(dynamic, 1)
    for (size_t b = 0; b < B; ++b) {
        size_t k = boff[b];
        for (auto &kv : bucket[b]) order[k++] = std::make_pair(kv.second, kv.first);
    }
    __gnu_parallel::sort(order.begin(), order.end(), [](const auto &x, const auto &y) { return x.first < y.first; },
                         __gnu_parallel::default_parallel_tag((unsigned)threads));
    names.name.clear();
    names.name.resize(order.size());
#pragma omp parallel for num_threads(threads) schedule(static)
    for (size_t i = 0; i < order.size(); ++i) {
        const View &nm = order[i].second;
        bucket[(size_t)ViewHash{}(nm) % B].find(nm)->second = (uint64_t)i;      // no insertion: elements are written in place
        names.name[i].assign(nm.p, nm.n);
    }
    lap("number the vertices");
    // gather all records, local id -> global vid
    size_t total = 0;
    std::vector<size_t> offs;
    for (auto *tp : {&tp1, &tp2}) for (auto &th : *tp) { offs.push_back(total); total += th.recs.size(); }
    std::vector<Rec> recs(total);
    {
#pragma omp parallel for num_threads(threads) schedule(dynamic, 1)
        for (size_t k = 0; k < all.size(); ++k) {
            ThreadParse &th = *all[k];
            std::vector<int32_t> remap(th.local_names.size());
            for (size_t i = 0; i < remap.size(); ++i) remap[i] = (int32_t)bucket[th.local_hash[i] % B].find(th.local_names[i])->second;
            for (size_t i = 0; i < th.recs.size(); ++i) { Rec r = th.recs[i]; r.vid = remap[(size_t)r.vid]; recs[offs[k] + i] = r; }
            std::vector<Rec>().swap(th.recs);
        }
    }
    lap("gather records");
    *t_sam = since(t0);

    // getEdgeInfo: one group per read key over both files -- sort by (hash, key bytes, vid)
    const auto t1 = clk::now();
    auto less = [](const Rec &a, const Rec &b) {
        if (a.hash != b.hash) return a.hash < b.hash;
        if (a.key.n != b.key.n) return a.key.n < b.key.n;
        const int c = memcmp(a.key.p, b.key.p, a.key.n);
        if (c != 0) return c < 0;
        return a.vid < b.vid;
    };
    __gnu_parallel::sort(recs.begin(), recs.end(), less, __gnu_parallel::default_parallel_tag((unsigned)threads));
    *t_merge = since(t1);

    // generateGraph: every run of equal keys is a clique over its distinct vids
    const auto t2 = clk::now();
    std::vector<std::vector<uint64_t>> parts((size_t)threads);
#pragma omp parallel num_threads(threads)
    {
        const int t = omp_get_thread_num();
        size_t lo = recs.size() * (size_t)t / (size_t)threads, hi = recs.size() * (size_t)(t + 1) / (size_t)threads;
        auto same = [&](size_t i, size_t j) { return recs[i].hash == recs[j].hash && recs[i].key == recs[j].key; };
        while (lo > 0 && lo < recs.size() && same(lo - 1, lo)) ++lo;          // start at a run boundary
        while (hi > 0 && hi < recs.size() && same(hi - 1, hi)) ++hi;
        std::vector<uint64_t> &out = parts[(size_t)t];
        std::vector<int32_t> clique;
        for (size_t i = lo; i < hi;) {
            size_t j = i;
            clique.clear();
            while (j < hi && same(i, j)) { if (clique.empty() || clique.back() != recs[j].vid) clique.push_back(recs[j].vid); ++j; }
            for (size_t x = 0; x < clique.size(); ++x)
                for (size_t y = x + 1; y < clique.size(); ++y)
                    out.push_back(((uint64_t)(uint32_t)clique[x] << 32) | (uint32_t)clique[y]);   // vids ascending: x < y
            i = j;
        }
    }
    std::vector<Rec>().swap(recs);
    size_t npairs = 0;
    for (auto &v : parts) npairs += v.size();
    std::vector<uint64_t> keys;
    keys.reserve(npairs);
    for (auto &v : parts) { keys.insert(keys.end(), v.begin(), v.end()); std::vector<uint64_t>().swap(v); }
    __gnu_parallel::sort(keys.begin(), keys.end(), std::less<uint64_t>(), __gnu_parallel::default_parallel_tag((unsigned)threads));
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    std::vector<int64_t> edges(keys.size() * 2);
#pragma omp parallel for num_threads(threads)
    for (size_t i = 0; i < keys.size(); ++i) { edges[2 * i] = (int64_t)(keys[i] >> 32); edges[2 * i + 1] = (int64_t)(keys[i] & 0xFFFFFFFFu); }
    *t_expand = since(t2);
    return edges;
}

// readUnitigsFile (src/graph.cpp:565-589): name = text between '>' and the first
// space; sequence lines concatenated, last character of each line dropped.
std::unordered_map<std::string, std::string> read_unitigs(const std::string &path)
{
    std::unordered_map<std::string, std::string> u;
    FILE *fp = fopen(path.c_str(), "r");
    if (!fp) file_not_found(path);
    char *line = nullptr;
    size_t cap = 0;
    ssize_t n;
    std::string cur;
    while ((n = getline(&line, &cap, fp)) != -1) {
        std::string s(line, (size_t)n);
        if (!s.empty() && s[0] == '>') {
            const size_t sp = s.find(' ');
            cur = s.substr(1, sp == std::string::npos ? std::string::npos : sp - 1);
            u[cur] = std::string();
        } else if (!s.empty()) {
            u[cur] += s.substr(0, s.size() - 1);
        }
    }
    free(line);
    fclose(fp);
    return u;
}

// CoreA::readKOMBOutput (src/CoreA.h:24-56): field 2 = coreness, field 3 = degree; '#' lines skipped
bool read_kcore_tsv(const std::string &path, std::vector<int32_t> &core, std::vector<int32_t> &deg, std::vector<std::string> *name = nullptr)
{
    FILE *fp = fopen(path.c_str(), "r");
    if (!fp) return false;
    char *line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, fp) != -1) {
        if (line[0] == '#') continue;
        int i = 0;
        char *save = nullptr;
        for (char *tok = strtok_r(line, "\t", &save); tok; tok = strtok_r(nullptr, "\t", &save), ++i) {
            if (i == 1 && name) name->emplace_back(tok);
            if (i == 2) core.push_back(atoi(tok));
            if (i == 3) deg.push_back(atoi(tok));
        }
    }
    free(line);
    fclose(fp);
    return true;
}

// Writes rows 0..n-1 to fp: rows are formatted by all threads into per-thread buffers (row(i, buf)
// appends the text of row i, exactly what the reference's fprintf would print) and the buffers are
// written in order -- the 10^7..10^8 fprintf calls of src/graph.cpp:468-475 and
// src/CombineCoreA.h:36-39 are the floor of the reference's own timed region.
template <class RowFn>
void write_rows(FILE *fp, int64_t n, int threads, RowFn &&row)
{
    const int64_t kBlockRows = 1 << 16;
    const int64_t nblocks = (n + kBlockRows - 1) / kBlockRows;
    for (int64_t b0 = 0; b0 < nblocks; b0 += threads) {
        const int64_t nb = std::min<int64_t>(threads, nblocks - b0);
        std::vector<std::string> out((size_t)nb);
#pragma omp parallel for num_threads(threads) schedule(static, 1)
        for (int64_t k = 0; k < nb; ++k) {
            std::string &buf = out[(size_t)k];
            const int64_t lo = (b0 + k) * kBlockRows, hi = std::min(n, lo + kBlockRows);
            buf.reserve((size_t)(hi - lo) * 24);
            for (int64_t i = lo; i < hi; ++i) row(i, buf);
        }
        for (auto &buf : out) fwrite(buf.data(), 1, buf.size(), fp);
    }
}

[[noreturn]] void die_accel(komb_ctx *ctx, const char *what, int rc)
{
    fprintf(stderr, "komb2: %s failed (%d): %s\n", what, rc, ctx ? komb_last_error(ctx) : "no context");
    leave(EXIT_FAILURE);
}

bool env_on(const char *name)
{
    const char *v = getenv(name);
    return v && *v && strcmp(v, "0") != 0;
}

// KOMB_COMPONENTS: the last komb_components_run as a table, one row per member vertex in VID order
template <class ValueFn>
void write_components(komb_ctx *ctx, const std::string &path, const char *third, const Names &names, int64_t nv, int threads,
                      ValueFn &&value)
{
    std::vector<int32_t> label((size_t)nv), size((size_t)nv);
    const int rc = komb_components_fetch(ctx, label.data(), size.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_components_fetch", rc);
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID\tName\t%s\tComponent\tSize\n", third);
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        if (label[(size_t)i] < 0) return;
        char tmp[48];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)i);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)i]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t", value(i));
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)label[(size_t)i]]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\n", size[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_DENSEST: komb_densest_subgraph_run(iters) as two tables: densest_subgraph.tsv, one row per member vertex in VID order,
// and core_density.tsv, one row per k
void write_densest(komb_ctx *ctx, int32_t iters, const std::string &outdir, const Names &names, int64_t nv, int threads,
                   const std::vector<int32_t> &core)
{
    int rc = komb_densest_subgraph_run(ctx, iters);
    if (rc != KOMB_OK) die_accel(ctx, "komb_densest_subgraph_run", rc);
    std::vector<int32_t> member((size_t)nv), load((size_t)nv);
    rc = komb_densest_subgraph_fetch(ctx, member.data(), load.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_densest_subgraph_fetch", rc);
    int32_t k_max = 0;
    rc = komb_densest_subgraph_info(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &k_max, nullptr);
    if (rc != KOMB_OK) die_accel(ctx, "komb_densest_subgraph_info", rc);
    std::vector<int64_t> n_k((size_t)k_max + 1), m_k((size_t)k_max + 1);
    rc = komb_densest_subgraph_profile(ctx, n_k.data(), m_k.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_densest_subgraph_profile", rc);
    std::string path = outdir + "/densest_subgraph.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID\tName\tCoreness\tLoad\n");
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        if (!member[(size_t)i]) return;
        char tmp[48];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)i);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)i]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\n", (int)core[(size_t)i], (int)load[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
    path = outdir + "/core_density.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#K\tVertices\tEdges\n");
    for (int32_t k = 0; k <= k_max; ++k) fprintf(fp, "%d\t%lld\t%lld\n", (int)k, (long long)n_k[(size_t)k], (long long)m_k[(size_t)k]);
    fclose(fp);
}

// KOMB_STRUCTURAL: a whole-graph k-truss run of its own and komb_structural_clusters_run on it as one table, one row per vertex
// in VID order
void write_structural(komb_ctx *ctx, int32_t eps_num, int32_t eps_den, int32_t mu, const std::string &outdir, const Names &names,
                      int64_t nv, int threads)
{
    std::vector<int32_t> label((size_t)nv), size((size_t)nv), role((size_t)nv), simdeg((size_t)nv);
    if (nv > 0) {
        int rc = komb_truss_run(ctx, nullptr);
        if (rc != KOMB_OK) die_accel(ctx, "komb_truss_run", rc);
        rc = komb_structural_clusters_run(ctx, eps_num, eps_den, mu);
        if (rc != KOMB_OK) die_accel(ctx, "komb_structural_clusters_run", rc);
        rc = komb_structural_clusters_fetch(ctx, label.data(), size.data(), role.data(), simdeg.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_structural_clusters_fetch", rc);
    }
    const std::string path = outdir + "/structural_clusters.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID\tName\tRole\tCluster\tClusterSize\tSimilarNeighbours\n");
    static const char *const kRole[4] = {"outlier", "hub", "border", "core"};
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        char tmp[48];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)i);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)i]);
        buf.push_back('\t');
        buf.append(kRole[role[(size_t)i] & 3]);
        buf.push_back('\t');
        if (label[(size_t)i] >= 0) buf.append(names.name[(size_t)label[(size_t)i]]); else buf.push_back('-');
        len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\n", (int)size[(size_t)i], (int)simdeg[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_GRAPHLETS: a whole-graph k-truss run of its own and komb_graphlets_run on it: the orbits, one row per vertex in VID order,
// the nine totals and, with with_edges, the three per-edge counts in canonical order
void write_graphlets(komb_ctx *ctx, bool with_edges, const std::string &outdir, const Names &names, int64_t nv, int threads)
{
    static const char *const kType[KOMB_GRAPHLET_TYPES] = {"edge", "wedge", "triangle", "path4", "claw", "cycle4", "paw", "diamond", "clique4"};
    std::vector<uint64_t> orbit((size_t)KOMB_GRAPHLET_ORBITS * (size_t)nv), cyc, clq;
    std::vector<int32_t> eu, ev, sup;
    uint64_t total[KOMB_GRAPHLET_TYPES] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int64_t ne = 0;
    if (nv > 0) {
        int rc = komb_truss_run(ctx, nullptr);
        if (rc != KOMB_OK) die_accel(ctx, "komb_truss_run", rc);
        rc = komb_graphlets_run(ctx);
        if (rc != KOMB_OK) die_accel(ctx, "komb_graphlets_run", rc);
        rc = komb_graphlets_fetch_vertices(ctx, orbit.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_graphlets_fetch_vertices", rc);
        rc = komb_graphlets_info(ctx, total, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        if (rc != KOMB_OK) die_accel(ctx, "komb_graphlets_info", rc);
        if (with_edges) {
            komb_truss_count(ctx, &ne);
            eu.resize((size_t)ne); ev.resize((size_t)ne); sup.resize((size_t)ne); cyc.resize((size_t)ne); clq.resize((size_t)ne);
            rc = komb_truss_fetch(ctx, eu.data(), ev.data(), nullptr);
            if (rc != KOMB_OK) die_accel(ctx, "komb_truss_fetch", rc);
            rc = komb_truss_fetch_support(ctx, sup.data());
            if (rc != KOMB_OK) die_accel(ctx, "komb_truss_fetch_support", rc);
            rc = komb_graphlets_fetch_edges(ctx, cyc.data(), clq.data());
            if (rc != KOMB_OK) die_accel(ctx, "komb_graphlets_fetch_edges", rc);
        }
    }
    std::string path = outdir + "/graphlet_orbits.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID\tName");
    for (int o = 0; o < KOMB_GRAPHLET_ORBITS; ++o) fprintf(fp, "\tO%d", o);
    fprintf(fp, "\n");
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        char tmp[48];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)i);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)i]);
        for (int o = 0; o < KOMB_GRAPHLET_ORBITS; ++o) {
            len = snprintf(tmp, sizeof(tmp), "\t%llu", (unsigned long long)orbit[(size_t)o * (size_t)nv + (size_t)i]);
            buf.append(tmp, (size_t)len);
        }
        buf.push_back('\n');
    });
    fclose(fp);
    path = outdir + "/graphlet_census.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#Graphlet\tCount\n");
    for (int i = 0; i < KOMB_GRAPHLET_TYPES; ++i) fprintf(fp, "%s\t%llu\n", kType[i], (unsigned long long)total[i]);
    fclose(fp);
    if (!with_edges) return;
    path = outdir + "/graphlet_edges.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#U\tV\tTriangles\tCycles4\tCliques4\n");
    write_rows(fp, ne, threads, [&](int64_t i, std::string &buf) {
        char tmp[96];
        buf.append(names.name[(size_t)eu[(size_t)i]]);
        buf.push_back('\t');
        buf.append(names.name[(size_t)ev[(size_t)i]]);
        const int len = snprintf(tmp, sizeof(tmp), "\t%d\t%llu\t%llu\n", (int)sup[(size_t)i], (unsigned long long)cyc[(size_t)i],
                                 (unsigned long long)clq[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_BETWEENNESS and KOMB_DISTANCES name their sources the same way: every vertex (n < 0 or n >= nv), or the n vertices with the
// smallest splitmix64(seed ^ vid), ties by id, passed in ascending id -- so the same value analyses the same sources
uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

struct SourceChoice {
    int64_t n = -1;                          // < 0: all
    uint64_t seed = 1;
};

// all | <n>[:<seed>]; anything else ends the program with the usage line of switch `name`
SourceChoice parse_source_choice(const char *name, const char *value)
{
    SourceChoice c;
    long long n = -1;
    unsigned long long seed = 1;
    bool ok = !strcmp(value, "all");
    if (!ok && *value >= '0' && *value <= '9') {
        char *end = nullptr;
        errno = 0;
        n = strtoll(value, &end, 10);
        ok = errno == 0 && n >= 0;
        if (ok && *end == ':' && end[1] >= '0' && end[1] <= '9') {
            seed = strtoull(end + 1, &end, 10);
            ok = errno == 0;
        }
        ok = ok && *end == 0;
    }
    if (!ok) {
        fprintf(stderr, "komb2: %s=%s: expected all or <n>[:<seed>]\n", name, value);
        leave(EXIT_FAILURE);
    }
    c.n = (int64_t)n; c.seed = (uint64_t)seed;
    return c;
}

// the list a run is given: false = every vertex (pass NULL), true = src (which may be empty)
bool sample_sources(const SourceChoice &c, int64_t nv, std::vector<int32_t> &src)
{
    if (c.n < 0 || c.n >= nv) return false;
    std::vector<std::pair<uint64_t, int32_t>> key((size_t)nv);
    for (int64_t v = 0; v < nv; ++v) key[(size_t)v] = {splitmix64(c.seed ^ (uint64_t)v), (int32_t)v};
    std::partial_sort(key.begin(), key.begin() + c.n, key.end());
    for (int64_t i = 0; i < c.n; ++i) src.push_back(key[(size_t)i].second);
    std::sort(src.begin(), src.end());
    return true;
}

// #VID, Name, Reached, SumDist, Ecc: one row per source in the order passed
void write_source_table(const std::string &path, const Names &names, int threads, const std::vector<int32_t> &source,
                        const std::vector<int64_t> &reached, const std::vector<int64_t> &sumd, const std::vector<int32_t> &ecc)
{
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID\tName\tReached\tSumDist\tEcc\n");
    write_rows(fp, (int64_t)source.size(), threads, [&](int64_t i, std::string &buf) {
        char tmp[96];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)source[(size_t)i]);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)source[(size_t)i]]);
        len = snprintf(tmp, sizeof(tmp), "\t%lld\t%lld\t%d\n", (long long)reached[(size_t)i], (long long)sumd[(size_t)i], (int)ecc[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_BETWEENNESS: komb_betweenness_run on the resident graph, as two tables: one row per vertex in VID order, one row per source
void write_betweenness(komb_ctx *ctx, const SourceChoice &choice, const std::string &outdir, const Names &names, int64_t nv, int threads)
{
    std::vector<int32_t> src;
    const bool all = !sample_sources(choice, nv, src);
    int64_t n_src = 0;
    std::vector<double> bc((size_t)nv);
    std::vector<int32_t> source, ecc;
    std::vector<int64_t> reached, sumd;
    if (nv > 0) {
        int32_t none = 0;
        int rc = komb_betweenness_run(ctx, all ? 0 : (int64_t)src.size(), all ? nullptr : (src.empty() ? &none : src.data()));
        if (rc != KOMB_OK) die_accel(ctx, "komb_betweenness_run", rc);
        rc = komb_betweenness_info(ctx, &n_src, nullptr, nullptr, nullptr, nullptr, nullptr);
        if (rc != KOMB_OK) die_accel(ctx, "komb_betweenness_info", rc);
        source.resize((size_t)n_src); ecc.resize((size_t)n_src); reached.resize((size_t)n_src); sumd.resize((size_t)n_src);
        rc = komb_betweenness_fetch(ctx, bc.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_betweenness_fetch", rc);
        rc = komb_betweenness_fetch_sources(ctx, source.data(), reached.data(), sumd.data(), ecc.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_betweenness_fetch_sources", rc);
    }
    std::string path = outdir + "/betweenness.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID\tName\tBetweenness\n");
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        char tmp[64];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)i);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)i]);
        len = snprintf(tmp, sizeof(tmp), "\t%.17g\n", bc[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
    write_source_table(outdir + "/betweenness_sources.tsv", names, threads, source, reached, sumd, ecc);
}

// KOMB_DISTANCES: komb_distances_run on the resident graph, as three tables: one row per vertex in VID order, one row per source,
// one row per distance
void write_distances(komb_ctx *ctx, const SourceChoice &choice, const std::string &outdir, const Names &names, int64_t nv, int threads)
{
    std::vector<int32_t> src;
    const bool all = !sample_sources(choice, nv, src);
    int64_t n_src = 0;
    int32_t depth = 0;
    std::vector<double> harmonic((size_t)nv);
    std::vector<int32_t> v_ecc((size_t)nv), source, ecc;
    std::vector<int64_t> v_reached((size_t)nv), v_sumd((size_t)nv), reached, sumd, pairs(1, 0);
    if (nv > 0) {
        int32_t none = 0;
        int rc = komb_distances_run(ctx, all ? 0 : (int64_t)src.size(), all ? nullptr : (src.empty() ? &none : src.data()));
        if (rc != KOMB_OK) die_accel(ctx, "komb_distances_run", rc);
        rc = komb_distances_info(ctx, &n_src, nullptr, &depth, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        if (rc != KOMB_OK) die_accel(ctx, "komb_distances_info", rc);
        source.resize((size_t)n_src); ecc.resize((size_t)n_src); reached.resize((size_t)n_src); sumd.resize((size_t)n_src);
        pairs.resize((size_t)depth + 1);
        rc = komb_distances_fetch(ctx, v_reached.data(), v_sumd.data(), v_ecc.data(), harmonic.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_distances_fetch", rc);
        rc = komb_distances_fetch_sources(ctx, source.data(), reached.data(), sumd.data(), ecc.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_distances_fetch_sources", rc);
        rc = komb_distances_histogram(ctx, pairs.data(), (int64_t)pairs.size());
        if (rc != KOMB_OK) die_accel(ctx, "komb_distances_histogram", rc);
    }
    std::string path = outdir + "/distances.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID\tName\tReached\tSumDist\tEcc\tHarmonic\n");
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        char tmp[128];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)i);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)i]);
        len = snprintf(tmp, sizeof(tmp), "\t%lld\t%lld\t%d\t%.17g\n", (long long)v_reached[(size_t)i], (long long)v_sumd[(size_t)i],
                       (int)v_ecc[(size_t)i], harmonic[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
    write_source_table(outdir + "/distance_sources.tsv", names, threads, source, reached, sumd, ecc);
    path = outdir + "/distance_histogram.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#Distance\tPairs\n");
    for (size_t L = 0; L < pairs.size(); ++L) fprintf(fp, "%d\t%lld\n", (int)L, (long long)pairs[L]);
    fclose(fp);
}

// KOMB_HIERARCHY: komb_hierarchy_run of `kind` as two tables: <prefix>_hierarchy.tsv, one row per node in node order, and
// <prefix>_hierarchy_vertices.tsv, one row per member vertex in VID order (level(v): its coreness / its largest trussness)
template <class LevelFn>
void write_hierarchy(komb_ctx *ctx, int32_t kind, const std::string &outdir, const char *prefix, const char *third, const Names &names,
                     int64_t nv, int threads, LevelFn &&level)
{
    int rc = komb_hierarchy_run(ctx, kind);
    if (rc != KOMB_OK) die_accel(ctx, "komb_hierarchy_run", rc);
    int64_t n = 0;
    komb_hierarchy_count(ctx, &n);
    std::vector<int32_t> k((size_t)n), rep((size_t)n), parent((size_t)n), size((size_t)n), shell((size_t)n), node((size_t)nv);
    rc = komb_hierarchy_fetch_nodes(ctx, k.data(), rep.data(), parent.data(), size.data(), shell.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_hierarchy_fetch_nodes", rc);
    rc = komb_hierarchy_fetch_vertices(ctx, node.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_hierarchy_fetch_vertices", rc);
    std::string path = outdir + "/" + prefix + "_hierarchy.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#Node\tK\tRep\tParent\tSize\tShell\n");
    write_rows(fp, n, threads, [&](int64_t i, std::string &buf) {
        char tmp[64];
        int len = snprintf(tmp, sizeof(tmp), "%d\t%d\t", (int)i, (int)k[(size_t)i]);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)rep[(size_t)i]]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\t%d\n", (int)parent[(size_t)i], (int)size[(size_t)i], (int)shell[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
    path = outdir + "/" + prefix + "_hierarchy_vertices.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID\tName\t%s\tNode\n", third);
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        if (node[(size_t)i] < 0) return;
        char tmp[48];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)i);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)i]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\n", level(i), (int)node[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_COMMUNITIES: the last komb_truss_communities_run as two tables (edges in canonical order, vertices in VID order)
void write_communities(komb_ctx *ctx, const std::string &outdir, const Names &names, int64_t nv, int threads,
                       const std::vector<int32_t> &eu, const std::vector<int32_t> &ev, const std::vector<int32_t> &tr)
{
    const int64_t ne = (int64_t)tr.size();
    std::vector<int32_t> label((size_t)ne), size((size_t)ne), rank((size_t)ne, -1), n_comm((size_t)nv);
    int rc = komb_truss_communities_fetch(ctx, label.data(), size.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_truss_communities_fetch", rc);
    rc = komb_truss_communities_fetch_vertices(ctx, n_comm.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_truss_communities_fetch_vertices", rc);
    int32_t next = 0;
    for (int64_t i = 0; i < ne; ++i)                       // a label is the community's first edge: ranks in ascending label order
        if (label[(size_t)i] == (int32_t)i) rank[(size_t)i] = next++;
    std::string path = outdir + "/truss_communities.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID_U\tName_U\tVID_V\tName_V\tTrussness\tCommunity\tSize\n");
    write_rows(fp, ne, threads, [&](int64_t i, std::string &buf) {
        if (label[(size_t)i] < 0) return;
        char tmp[64];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)eu[(size_t)i]);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)eu[(size_t)i]]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t", (int)ev[(size_t)i]);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)ev[(size_t)i]]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\t%d\n", (int)tr[(size_t)i], (int)rank[(size_t)label[(size_t)i]], (int)size[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
    path = outdir + "/truss_community_vertices.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID\tName\tCommunities\n");
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        if (n_comm[(size_t)i] < 1) return;
        char tmp[48];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)i);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)i]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\n", (int)n_comm[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_BICONNECTED: a whole-graph k-truss run of its own (the max core, the truss stage's subject, is one dense piece) and
// komb_biconnected_run on it as two tables (edges in canonical order, vertices in VID order)
void write_biconnected(komb_ctx *ctx, int32_t k, const std::string &outdir, const Names &names, int64_t nv, int threads)
{
    int rc = komb_truss_run(ctx, nullptr);
    if (rc != KOMB_OK) die_accel(ctx, "komb_truss_run", rc);
    int64_t ne = 0;
    komb_truss_count(ctx, &ne);
    std::vector<int32_t> eu((size_t)ne), ev((size_t)ne), tr((size_t)ne);
    rc = komb_truss_fetch(ctx, eu.data(), ev.data(), tr.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_truss_fetch", rc);
    rc = komb_biconnected_run(ctx, k);
    if (rc != KOMB_OK) die_accel(ctx, "komb_biconnected_run", rc);
    std::vector<int32_t> block((size_t)ne), size((size_t)ne), rank((size_t)ne, -1), n_blocks((size_t)nv), ecc((size_t)nv), ecc_size((size_t)nv);
    rc = komb_biconnected_fetch_edges(ctx, block.data(), size.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_biconnected_fetch_edges", rc);
    rc = komb_biconnected_fetch_vertices(ctx, n_blocks.data(), ecc.data(), ecc_size.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_biconnected_fetch_vertices", rc);
    int32_t next = 0;
    for (int64_t i = 0; i < ne; ++i)                       // a label is the block's first edge: ranks in ascending label order
        if (block[(size_t)i] == (int32_t)i) rank[(size_t)i] = next++;
    std::string path = outdir + "/truss_blocks.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID_U\tName_U\tVID_V\tName_V\tTrussness\tBlock\tSize\tBridge\n");
    write_rows(fp, ne, threads, [&](int64_t i, std::string &buf) {
        if (block[(size_t)i] < 0) return;
        char tmp[80];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)eu[(size_t)i]);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)eu[(size_t)i]]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t", (int)ev[(size_t)i]);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)ev[(size_t)i]]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\t%d\t%d\n", (int)tr[(size_t)i], (int)rank[(size_t)block[(size_t)i]], (int)size[(size_t)i],
                       size[(size_t)i] == 1 ? 1 : 0);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
    path = outdir + "/truss_articulation.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID\tName\tBlocks\tArticulation\tComponent2E\tSize2E\n");
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        if (ecc[(size_t)i] < 0) return;
        char tmp[64];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)i);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)i]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\t", (int)n_blocks[(size_t)i], n_blocks[(size_t)i] >= 2 ? 1 : 0);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)ecc[(size_t)i]]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\n", (int)ecc_size[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_NUCLEUS: komb_nucleus_run on the truss stage's result as two tables (triangles in triangle order, the result's unitigs in VID order)
void write_nucleus(komb_ctx *ctx, const std::string &outdir, const Names &names, int64_t nv, int threads,
                   const std::vector<int32_t> &eu, const std::vector<int32_t> &ev)
{
    int rc = komb_nucleus_run(ctx);
    if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_run", rc);
    int64_t n = 0;
    rc = komb_nucleus_count(ctx, &n);
    if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_count", rc);
    std::vector<int32_t> a((size_t)n), b((size_t)n), c((size_t)n), key0((size_t)n), theta((size_t)n), vtheta((size_t)nv);
    rc = komb_nucleus_fetch(ctx, a.data(), b.data(), c.data(), key0.data(), theta.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_fetch", rc);
    rc = komb_nucleus_fetch_vertices(ctx, vtheta.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_fetch_vertices", rc);
    std::string path = outdir + "/nucleus_triangles.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#Name_A\tName_B\tName_C\tCliques\tTheta\n");
    write_rows(fp, n, threads, [&](int64_t i, std::string &buf) {
        buf.append(names.name[(size_t)a[(size_t)i]]);
        buf.push_back('\t');
        buf.append(names.name[(size_t)b[(size_t)i]]);
        buf.push_back('\t');
        buf.append(names.name[(size_t)c[(size_t)i]]);
        char tmp[48];
        const int len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\n", (int)key0[(size_t)i], (int)theta[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
    std::vector<uint8_t> in((size_t)nv, 0);                // the vertices of the result: the ends of its edges
    for (size_t e = 0; e < eu.size(); ++e) { in[(size_t)eu[e]] = 1; in[(size_t)ev[e]] = 1; }
    path = outdir + "/nucleus_unitigs.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID\tName\tTheta\n");
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        if (!in[(size_t)i]) return;
        char tmp[48];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)i);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)i]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\n", (int)vtheta[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_MAX_CLIQUE: komb_max_clique_run on the truss stage's result as two tables (the cliques in list order, the unitigs in VID order)
void write_max_clique(komb_ctx *ctx, int64_t budget, const std::string &outdir, const Names &names, int64_t nv, int threads)
{
    int rc = komb_max_clique_run(ctx, budget);
    if (rc != KOMB_OK) die_accel(ctx, "komb_max_clique_run", rc);
    int32_t omega = 0, upper = 0, flags = 0;
    int64_t n_max = 0;
    rc = komb_max_clique_info(ctx, &omega, &upper, &flags, nullptr, &n_max, nullptr, nullptr, nullptr);
    if (rc != KOMB_OK) die_accel(ctx, "komb_max_clique_info", rc);
    std::vector<int32_t> count((size_t)nv), verts;
    int64_t rows = 0;
    if (flags & KOMB_MAXCLQ_LISTED) {
        rows = n_max;
        verts.resize((size_t)rows * (size_t)omega);
        rc = komb_max_clique_fetch(ctx, count.data(), nullptr);
        if (rc != KOMB_OK) die_accel(ctx, "komb_max_clique_fetch", rc);
        rc = komb_max_clique_list(ctx, rows, &rows, verts.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_max_clique_list", rc);
    } else {
        rows = omega > 0 ? 1 : 0;
        verts.resize((size_t)omega);
        rc = komb_max_clique_fetch(ctx, count.data(), verts.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_max_clique_fetch", rc);
    }
    std::string path = outdir + "/max_cliques.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "# omega %d upper %d flags %d cliques %lld\n", (int)omega, (int)upper, (int)flags, (long long)n_max);
    write_rows(fp, rows, threads, [&](int64_t i, std::string &buf) {
        for (int32_t k = 0; k < omega; ++k) {
            if (k) buf.push_back('\t');
            buf.append(names.name[(size_t)verts[(size_t)i * (size_t)omega + (size_t)k]]);
        }
        buf.push_back('\n');
    });
    fclose(fp);
    path = outdir + "/max_clique_unitigs.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#Name\tCount\n");
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        if (count[(size_t)i] <= 0) return;
        buf.append(names.name[(size_t)i]);
        char tmp[32];
        const int len = snprintf(tmp, sizeof(tmp), "\t%d\n", (int)count[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_CLIQUE_CENSUS: komb_clique_census_run on the truss stage's result as one or two tables (the sizes ascending, the unitigs in VID order)
void write_clique_census(komb_ctx *ctx, const int32_t window[3], const std::string &outdir, const Names &names, int64_t nv, int threads)
{
    int rc = komb_clique_census_run(ctx, window[0], window[1], window[2], 0);
    if (rc != KOMB_OK) die_accel(ctx, "komb_clique_census_run", rc);
    int32_t k_lo = 0, k_hi = 0, k_local = 0, omega = 0, flags = 0;
    int64_t roots = 0, nodes = 0;
    rc = komb_clique_census_info(ctx, &k_lo, &k_hi, &k_local, nullptr, &omega, &flags, nullptr, &roots, &nodes, nullptr);
    if (rc != KOMB_OK) die_accel(ctx, "komb_clique_census_info", rc);
    std::vector<uint64_t> total((size_t)(k_hi - k_lo + 1)), local(k_local ? (size_t)nv : 0);
    rc = komb_clique_census_fetch(ctx, total.data(), k_local ? local.data() : nullptr);
    if (rc != KOMB_OK) die_accel(ctx, "komb_clique_census_fetch", rc);
    std::string path = outdir + "/clique_census.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "# k_lo %d k_hi %d k_local %d flags %d omega %d nodes %lld roots %lld\n", (int)k_lo, (int)k_hi, (int)k_local, (int)flags, (int)omega,
            (long long)nodes, (long long)roots);
    for (size_t i = 0; i < total.size(); ++i) fprintf(fp, "%d\t%llu\n", (int)k_lo + (int)i, (unsigned long long)total[i]);
    fclose(fp);
    if (!k_local) return;
    path = outdir + "/clique_census_unitigs.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#Name\tCount\n");
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        buf.append(names.name[(size_t)i]);
        char tmp[32];
        const int len = snprintf(tmp, sizeof(tmp), "\t%llu\n", (unsigned long long)local[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_MAXIMAL_CLIQUES: komb_maximal_cliques_run on the truss stage's result as three tables (the cliques in list order, the sizes
// ascending, the unitigs in VID order)
void write_maximal_cliques(komb_ctx *ctx, int32_t k_min_arg, int64_t budget, const std::string &outdir, const Names &names, int64_t nv, int threads)
{
    int rc = komb_maximal_cliques_run(ctx, k_min_arg, budget);
    if (rc != KOMB_OK) die_accel(ctx, "komb_maximal_cliques_run", rc);
    int32_t k_min = 0, k_hi = 0, omega = 0, flags = 0;
    int64_t n_cliques = 0, roots = 0, nodes = 0;
    rc = komb_maximal_cliques_info(ctx, &k_min, &k_hi, nullptr, &omega, &flags, &n_cliques, nullptr, &roots, &nodes, nullptr);
    if (rc != KOMB_OK) die_accel(ctx, "komb_maximal_cliques_info", rc);
    std::vector<int64_t> hist((size_t)(k_hi - k_min + 1)), offset(1, 0);
    std::vector<int32_t> count((size_t)nv), largest((size_t)nv), verts;
    rc = komb_maximal_cliques_fetch(ctx, hist.data(), count.data(), largest.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_maximal_cliques_fetch", rc);
    int64_t rows = 0;
    if (flags & KOMB_MAXIMAL_LISTED) {
        int64_t n_verts = 0;
        rc = komb_maximal_cliques_list(ctx, 0, 0, &rows, &n_verts, nullptr, nullptr);
        if (rc != KOMB_OK) die_accel(ctx, "komb_maximal_cliques_list", rc);
        offset.resize((size_t)rows + 1);
        verts.resize((size_t)n_verts);
        rc = komb_maximal_cliques_list(ctx, rows, n_verts, nullptr, nullptr, offset.data(), verts.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_maximal_cliques_list", rc);
    }
    std::string path = outdir + "/maximal_cliques.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "# k_min %d flags %d omega %d cliques %lld nodes %lld roots %lld\n", (int)k_min, (int)flags, (int)omega, (long long)n_cliques,
            (long long)nodes, (long long)roots);
    write_rows(fp, rows, threads, [&](int64_t i, std::string &buf) {
        buf.append(std::to_string(offset[(size_t)i + 1] - offset[(size_t)i]));
        for (int64_t k = offset[(size_t)i]; k < offset[(size_t)i + 1]; ++k) {
            buf.push_back('\t');
            buf.append(names.name[(size_t)verts[(size_t)k]]);
        }
        buf.push_back('\n');
    });
    fclose(fp);
    path = outdir + "/maximal_clique_sizes.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    for (size_t i = 0; i < hist.size(); ++i) fprintf(fp, "%d\t%lld\n", (int)k_min + (int)i, (long long)hist[i]);
    fclose(fp);
    path = outdir + "/maximal_clique_unitigs.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#Name\tCount\tLargest\n");
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        if (count[(size_t)i] <= 0) return;
        buf.append(names.name[(size_t)i]);
        char tmp[48];
        const int len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\n", (int)count[(size_t)i], (int)largest[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_CLIQUE_COMMUNITIES: komb_clique_communities_run on the maximal cliques of the truss stage's result as two tables (the
// communities in community order, the unitigs in VID order).  have_list: KOMB_MAXIMAL_CLIQUES left a list with a k_min <= k.
void write_clique_communities(komb_ctx *ctx, int32_t k_arg, int64_t budget, bool have_list, const std::string &outdir, const Names &names, int64_t nv,
                              int threads)
{
    int rc = KOMB_OK;
    if (!have_list) {
        rc = komb_maximal_cliques_run(ctx, k_arg, 0);
        if (rc != KOMB_OK) die_accel(ctx, "komb_maximal_cliques_run", rc);
    }
    rc = komb_clique_communities_run(ctx, k_arg, budget);
    if (rc != KOMB_OK) die_accel(ctx, "komb_clique_communities_run", rc);
    int32_t k = 0;
    int64_t n_member = 0, n_comm = 0, covered = 0, overlap = 0, pair_tests = 0, n_verts = 0;
    rc = komb_clique_communities_info(ctx, &k, nullptr, &n_member, &n_comm, nullptr, &covered, &overlap, &pair_tests, nullptr);
    if (rc != KOMB_OK) die_accel(ctx, "komb_clique_communities_info", rc);
    rc = komb_clique_communities_count(ctx, nullptr, &n_verts);
    if (rc != KOMB_OK) die_accel(ctx, "komb_clique_communities_count", rc);
    std::vector<int32_t> n_cliques((size_t)n_comm), verts((size_t)n_verts), v_comm((size_t)nv), v_first((size_t)nv);
    std::vector<int64_t> offset((size_t)n_comm + 1, 0);
    rc = komb_clique_communities_fetch_communities(ctx, nullptr, n_cliques.data(), offset.data(), verts.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_clique_communities_fetch_communities", rc);
    rc = komb_clique_communities_fetch_vertices(ctx, v_comm.data(), v_first.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_clique_communities_fetch_vertices", rc);
    std::string path = outdir + "/clique_communities.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "# k %d communities %lld member_cliques %lld covered %lld overlap %lld pair_tests %lld\n", (int)k, (long long)n_comm, (long long)n_member,
            (long long)covered, (long long)overlap, (long long)pair_tests);
    write_rows(fp, n_comm, threads, [&](int64_t c, std::string &buf) {
        char tmp[64];
        const int len = snprintf(tmp, sizeof(tmp), "%lld\t%d\t%lld", (long long)c, (int)n_cliques[(size_t)c],
                                 (long long)(offset[(size_t)c + 1] - offset[(size_t)c]));
        buf.append(tmp, (size_t)len);
        for (int64_t i = offset[(size_t)c]; i < offset[(size_t)c + 1]; ++i) {
            buf.push_back('\t');
            buf.append(names.name[(size_t)verts[(size_t)i]]);
        }
        buf.push_back('\n');
    });
    fclose(fp);
    path = outdir + "/clique_community_unitigs.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#Name\tCommunities\tFirst\n");
    write_rows(fp, nv, threads, [&](int64_t i, std::string &buf) {
        if (v_comm[(size_t)i] <= 0) return;
        buf.append(names.name[(size_t)i]);
        char tmp[48];
        const int len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\n", (int)v_comm[(size_t)i], (int)v_first[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_NUCLEUS_HIERARCHY: komb_nucleus_hierarchy_run on the nucleus decomposition of the truss stage's result as two tables (nodes in
// node order, member triangles in triangle order)
void write_nucleus_hierarchy(komb_ctx *ctx, const std::string &outdir, const Names &names, int threads, bool have_nucleus)
{
    int rc = have_nucleus ? KOMB_OK : komb_nucleus_run(ctx);
    if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_run", rc);
    rc = komb_nucleus_hierarchy_run(ctx);
    if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_hierarchy_run", rc);
    int64_t nt = 0, n = 0;
    rc = komb_nucleus_count(ctx, &nt);
    if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_count", rc);
    rc = komb_nucleus_hierarchy_count(ctx, &n);
    if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_hierarchy_count", rc);
    std::vector<int32_t> a((size_t)nt), b((size_t)nt), c((size_t)nt), theta((size_t)nt), node((size_t)nt);
    std::vector<int32_t> k((size_t)n), rep((size_t)n), parent((size_t)n), size((size_t)n), shell((size_t)n), edges((size_t)n, 0), verts((size_t)n, 0);
    rc = komb_nucleus_fetch(ctx, a.data(), b.data(), c.data(), nullptr, theta.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_fetch", rc);
    rc = komb_nucleus_hierarchy_fetch_nodes(ctx, k.data(), rep.data(), parent.data(), size.data(), shell.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_hierarchy_fetch_nodes", rc);
    rc = komb_nucleus_hierarchy_fetch_triangles(ctx, node.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_hierarchy_fetch_triangles", rc);
    // Edges and Vertices: the nodes of level K are among the K-nuclei, matched by rep (both lists ascend in rep)
    for (int64_t lo = 0; lo < n;) {
        int64_t hi = lo;
        while (hi < n && k[(size_t)hi] == k[(size_t)lo]) ++hi;
        int64_t cnt = 0;
        rc = komb_nucleus_hierarchy_nuclei(ctx, k[(size_t)lo], 0, &cnt, nullptr, nullptr, nullptr, nullptr);
        if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_hierarchy_nuclei", rc);
        std::vector<int32_t> nrep((size_t)cnt), nedge((size_t)cnt), nvert((size_t)cnt);
        rc = komb_nucleus_hierarchy_nuclei(ctx, k[(size_t)lo], cnt, &cnt, nrep.data(), nullptr, nedge.data(), nvert.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_nucleus_hierarchy_nuclei", rc);
        for (int64_t i = lo, j = 0; i < hi; ++i) {
            while (j < cnt && nrep[(size_t)j] < rep[(size_t)i]) ++j;
            if (j < cnt && nrep[(size_t)j] == rep[(size_t)i]) { edges[(size_t)i] = nedge[(size_t)j]; verts[(size_t)i] = nvert[(size_t)j]; }
        }
        lo = hi;
    }
    std::string path = outdir + "/nucleus_hierarchy.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#Node\tTheta\tRep_A\tRep_B\tRep_C\tParent\tTriangles\tShell\tEdges\tVertices\n");
    write_rows(fp, n, threads, [&](int64_t i, std::string &buf) {
        const size_t r = (size_t)rep[(size_t)i];
        char tmp[96];
        int len = snprintf(tmp, sizeof(tmp), "%d\t%d\t", (int)i, (int)k[(size_t)i]);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)a[r]]);
        buf.push_back('\t');
        buf.append(names.name[(size_t)b[r]]);
        buf.push_back('\t');
        buf.append(names.name[(size_t)c[r]]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\t%d\t%d\t%d\n", (int)parent[(size_t)i], (int)size[(size_t)i], (int)shell[(size_t)i],
                       (int)edges[(size_t)i], (int)verts[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
    path = outdir + "/nucleus_hierarchy_triangles.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#Name_A\tName_B\tName_C\tTheta\tNode\n");
    write_rows(fp, nt, threads, [&](int64_t i, std::string &buf) {
        if (theta[(size_t)i] < 1) return;
        buf.append(names.name[(size_t)a[(size_t)i]]);
        buf.push_back('\t');
        buf.append(names.name[(size_t)b[(size_t)i]]);
        buf.push_back('\t');
        buf.append(names.name[(size_t)c[(size_t)i]]);
        char tmp[48];
        const int len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\n", (int)theta[(size_t)i], (int)node[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// KOMB_COMMUNITY_HIERARCHY: komb_community_hierarchy_run as two tables (nodes in node order, member edges in canonical order)
void write_community_hierarchy(komb_ctx *ctx, const std::string &outdir, const Names &names, int threads,
                               const std::vector<int32_t> &eu, const std::vector<int32_t> &ev, const std::vector<int32_t> &tr)
{
    const int64_t ne = (int64_t)tr.size();
    int rc = komb_community_hierarchy_run(ctx);
    if (rc != KOMB_OK) die_accel(ctx, "komb_community_hierarchy_run", rc);
    int64_t n = 0;
    komb_community_hierarchy_count(ctx, &n);
    std::vector<int32_t> k((size_t)n), rep((size_t)n), parent((size_t)n), size((size_t)n), shell((size_t)n), node((size_t)ne);
    rc = komb_community_hierarchy_fetch_nodes(ctx, k.data(), rep.data(), parent.data(), size.data(), shell.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_community_hierarchy_fetch_nodes", rc);
    rc = komb_community_hierarchy_fetch_edges(ctx, node.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_community_hierarchy_fetch_edges", rc);
    std::string path = outdir + "/truss_community_hierarchy.tsv";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#Node\tK\tRep_U\tRep_V\tParent\tSize\tShell\n");
    write_rows(fp, n, threads, [&](int64_t i, std::string &buf) {
        char tmp[64];
        int len = snprintf(tmp, sizeof(tmp), "%d\t%d\t", (int)i, (int)k[(size_t)i]);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)eu[(size_t)rep[(size_t)i]]]);
        buf.push_back('\t');
        buf.append(names.name[(size_t)ev[(size_t)rep[(size_t)i]]]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\t%d\n", (int)parent[(size_t)i], (int)size[(size_t)i], (int)shell[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
    path = outdir + "/truss_community_hierarchy_edges.tsv";
    fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    fprintf(fp, "#VID_U\tName_U\tVID_V\tName_V\tTrussness\tNode\n");
    write_rows(fp, ne, threads, [&](int64_t i, std::string &buf) {
        if (node[(size_t)i] < 0) return;
        char tmp[64];
        int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)eu[(size_t)i]);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)eu[(size_t)i]]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t", (int)ev[(size_t)i]);
        buf.append(tmp, (size_t)len);
        buf.append(names.name[(size_t)ev[(size_t)i]]);
        len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\n", (int)tr[(size_t)i], (int)node[(size_t)i]);
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// CombineCoreA::run (src/CombineCoreA.h:16-43)
void corea_stage(komb_ctx *ctx, const std::string &outdir, const std::vector<int32_t> &deg, const std::vector<int32_t> &core, int threads)
{
    const int n = (int)deg.size();
    const double dense_ratio = n ? (double)(*std::max_element(core.begin(), core.end()) / 2) : 0.0;   // integer division (:24)
    fprintf(stdout, "Dense Ratio: %f\n", dense_ratio);
    std::vector<double> score((size_t)n);
    int rc = komb_corea_scores(ctx, deg.data(), core.data(), n, score.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_corea_scores", rc);
    if ((int64_t)(n ? *std::max_element(core.begin(), core.end()) : 0) * n + (n ? *std::max_element(deg.begin(), deg.end()) : 0) > 2147483647LL)
        fprintf(stderr, "komb2: note: coreness*n+degree exceeds 2^31-1; the reference's int key (src/CoreA.h:122) would overflow here, 64-bit keys used\n");
    const double max_dmp = n ? *std::max_element(score.begin(), score.end()) : 0.0;
    fprintf(stdout, "Max CoreA score: %f\n", max_dmp);
    const std::string path = outdir + "/CoreA_anomaly.txt";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    write_rows(fp, n, threads, [&](int64_t i, std::string &buf) {
        char tmp[64];
        const int len = snprintf(tmp, sizeof(tmp), "%d\t%f\n", (int)i, score[(size_t)i]);      // src/CombineCoreA.h:38
        buf.append(tmp, (size_t)len);
    });
    fclose(fp);
}

// combineFile (src/graph.cpp:591-635; call commented out at src/komb2.cpp:126): one FASTA record per
// kcore.tsv row, header ">Unitig_<name>|<coreness>", sequence only when the unitig file has that name.
// The reference re-parses kcore.tsv for the fields; the same values are still in memory here.
void combine_file(const std::string &outdir, const Names &names, const std::vector<int32_t> &core,
                  const std::unordered_map<std::string, std::string> &unitigs, int threads)
{
    const std::string path = outdir + "/combined.fasta";
    FILE *fp = fopen(path.c_str(), "w+");
    if (!fp) file_not_found(path);
    write_rows(fp, (int64_t)core.size(), threads, [&](int64_t i, std::string &buf) {
        const std::string &nm = names.name[(size_t)i];
        buf.append(">Unitig_").append(nm).append("|").append(std::to_string(core[(size_t)i])).append("\n");
        auto it = unitigs.find(nm);
        if (it != unitigs.end()) buf.append(it->second).append("\n");
    });
    fclose(fp);
}

// getMedian (src/graph.cpp:650-665), including its window: size = end - start - 1
double v1_median(const std::vector<double> &v, int start, int end)
{
    const int size = end - start - 1;
    if (size % 2 == 0) return (v[(size_t)(start + size / 2 - 1)] + v[(size_t)(start + size / 2)]) / 2;
    return v[(size_t)(start + (size - 1) / 2)];
}

// splitAnomalousUnitigs (src/graph.cpp:667-749; call commented out at src/komb2.cpp:139). Kept as the
// reference has it, quirks included: scores are the six-decimal text of CoreA_anomaly.txt read back;
// row i of the output is decided by the i-th SMALLEST score (the sorted copy is what :725 indexes), is
// labelled "Unitig_<i>" and looks the sequence up under the name "<i>". mode "fixed" instead decides
// row i by vertex i's own score and uses the vertex's unitig name.
// The quartile windows read outside the vector for fewer than 6 scores (undefined in the reference):
// refused with a note.
bool split_anomalous(const std::string &outdir, const Names &names, const std::unordered_map<std::string, std::string> &unitigs,
                     bool fixed, int threads)
{
    const std::string in_path = outdir + "/CoreA_anomaly.txt";
    FILE *in = fopen(in_path.c_str(), "r");
    if (!in) file_not_found(in_path);
    std::vector<double> score;
    char *line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, in) != -1) {
        const char *tab = strchr(line, '\t');
        if (tab) score.push_back(strtod(tab + 1, nullptr));
    }
    free(line);
    fclose(in);
    const int size = (int)score.size();
    if (size < 6) {
        fprintf(stderr, "komb2: note: %d CoreA scores; the reference's quartile windows (src/graph.cpp:714-724) need at least 6, split skipped\n", size);
        return false;
    }
    std::vector<double> sorted(score);
    std::sort(sorted.begin(), sorted.end());
    const double q1 = v1_median(sorted, 0, size / 2 - 1);
    const double q3 = size % 2 == 0 ? v1_median(sorted, size / 2, size - 1) : v1_median(sorted, size / 2 + 1, size - 1);
    const double cutoff = q3 + 1.5 * (q3 - q1);
    const std::vector<double> &decide = fixed ? score : sorted;

    const std::string top_path = outdir + "/top_scoring_anomalous_unitigs.txt", low_path = outdir + "/low_scoring_anomalous_unitigs.txt";
    FILE *top = fopen(top_path.c_str(), "w+"), *low = fopen(low_path.c_str(), "w+");
    if (!top) file_not_found(top_path);
    if (!low) file_not_found(low_path);
    for (int pass = 0; pass < 2; ++pass) {
        write_rows(pass == 0 ? top : low, size, threads, [&](int64_t i, std::string &buf) {
            if ((decide[(size_t)i] >= cutoff) != (pass == 0)) return;
            const std::string key = fixed && (size_t)i < names.name.size() ? names.name[(size_t)i] : std::to_string(i);
            buf.append("Unitig_").append(key).append("\n");
            auto it = unitigs.find(key);
            if (it != unitigs.end()) buf.append(it->second).append("\n");
        });
    }
    fclose(top);
    fclose(low);
    return true;
}

} // namespace

int main(int argc, const char **argv)
{
    const Args args = parse_args(argc, argv);
    const auto begin = clk::now();

    // standalone use: the reference needs -o to exist (KOMB.py creates it, KOMB.py:41-52)
    mkdir(args.outdir.c_str(), 0777);

    // --corea-only mode: resume from an existing kcore.tsv, like CoreA itself does
    if (env_on("KOMB_COREA_ONLY")) {
        std::vector<int32_t> core, deg;
        if (!read_kcore_tsv(args.outdir + "/kcore.tsv", core, deg)) file_not_found(args.outdir + "/kcore.tsv");
        komb_opts o{};
        o.device = getenv("KOMB_DEVICE") ? atoi(getenv("KOMB_DEVICE")) : 0;
        komb_ctx *ctx = komb_create(&o);
        corea_stage(ctx, args.outdir, deg, core, args.threads);
        komb_destroy(ctx);
        return 0;
    }

    // v1-outputs-only mode: combined.fasta and the split from an existing kcore.tsv + CoreA_anomaly.txt (no device)
    if (env_on("KOMB_V1_ONLY")) {
        std::vector<int32_t> core, deg;
        Names names;
        if (!read_kcore_tsv(args.outdir + "/kcore.tsv", core, deg, &names.name)) file_not_found(args.outdir + "/kcore.tsv");
        const auto unitigs = read_unitigs(args.unitigs);
        const char *mode = getenv("KOMB_V1_OUTPUTS");
        combine_file(args.outdir, names, core, unitigs, args.threads);
        split_anomalous(args.outdir, names, unitigs, mode && strcmp(mode, "fixed") == 0, args.threads);
        return 0;
    }

    // Creating the HIP context takes ~0.6 s; it runs beside the SAM parse (never in the host-only test mode).
    komb_opts opts{};
    opts.device = getenv("KOMB_DEVICE") ? atoi(getenv("KOMB_DEVICE")) : 0;
    opts.reserved[0] = KOMB_CREATE_WARM_UPLOAD;          // the upload's pinned staging buffers are made beside the SAM parse, off the critical path
    std::future<komb_ctx *> ctx_early;
    g_ctx_early = &ctx_early;
    for (const std::string *path : {&args.input, &args.input2})          // fail on a missing input before a second thread exists
        if (access(path->c_str(), R_OK) != 0) file_not_found(*path);
    if (!env_on("KOMB_STOP_AFTER_EDGES")) ctx_early = std::async(std::launch::async, [&opts]() { return komb_create(&opts); });

    const bool strict = env_on("KOMB_STRICT_SAM");
    const auto begin_komb = clk::now();
    Names names;
    double t_sam_s = 0, t_merge_s = 0, t_expand_s = 0;
    std::vector<int64_t> edges = build_edges(args.input, args.input2, args.threads, strict, names, &t_sam_s, &t_merge_s, &t_expand_s);
    fprintf(stdout, "\nTime elapsed for reading SAMs: %.3f s\n", t_sam_s);
    fprintf(stdout, "\nTime elapsed for edgeInfo: %.3f s\n", t_merge_s);
    fprintf(stdout, "\nTime elapsed for converting umapset to vec<vec>: %.3f s\n", 0.0);
    fprintf(stdout, "\nTime elapsed for constructing local edges: %.3f s\n", t_expand_s);
    auto t_generate = clk::now();
    fprintf(stdout, "\nTime elapsed for generateGraph: %.3f s\n", t_expand_s);
    auto t0 = clk::now();

    // readEdgeList (src/graph.cpp:395-453): edgelist.txt = the raw pairs
    const int64_t nv = (int64_t)names.name.size();
    t0 = clk::now();
    {
        const std::string path = args.outdir + "/edgelist.txt";
        FILE *f = fopen(path.c_str(), "w");
        if (!f) file_not_found(path);
        write_rows(f, (int64_t)(edges.size() / 2), args.threads, [&](int64_t i, std::string &buf) {
            char tmp[48];
            const int len = snprintf(tmp, sizeof(tmp), "%ld\t%ld\n", (long)edges[2 * (size_t)i], (long)edges[2 * (size_t)i + 1]);   // src/graph.cpp:425
            buf.append(tmp, (size_t)len);
        });
        fclose(f);
    }
    if (env_on("KOMB_STOP_AFTER_EDGES")) {
        const std::string path = args.outdir + "/vertex_names.txt";
        FILE *f = fopen(path.c_str(), "w");
        if (!f) file_not_found(path);
        for (int64_t v = 0; v < nv; ++v) fprintf(f, "%ld\t%s\n", (long)v, names.name[(size_t)v].c_str());
        fclose(f);
        return 0;
    }

    komb_ctx *ctx = ctx_early.get();
    if (!ctx) die_accel(nullptr, "komb_create", KOMB_ERR_NOMEM);
    fprintf(stdout, "\nTime elapsed for initializing igraph graph: %.3f s\n", since(t0));
    t0 = clk::now();
    int rc = komb_graph_from_edges(ctx, nv, (int64_t)(edges.size() / 2), edges.data());   // igraph_create + igraph_simplify
    if (rc != KOMB_OK) die_accel(ctx, "komb_graph_from_edges", rc);
    std::vector<int64_t>().swap(edges);
    fprintf(stdout, "\nTime elapsed for simplifying graph: %.3f s\n", since(t0));
    int64_t gnv = 0, gne = 0;
    komb_graph_info(ctx, &gnv, &gne);
    fprintf(stdout, "GraphInfo...\n\tNumber of vertices: %d\n", (int)gnv);
    fprintf(stdout, "\tNumber of edges: %d\n", (int)gne);

    // src/graph.cpp:446 reads the unitig FASTA here; only the (disabled) truss / v1 stages use it, so it is
    // opened now -- a missing file must fail at this point, as in the reference -- and parsed only when needed
    if (access(args.unitigs.c_str(), R_OK) != 0) file_not_found(args.unitigs);
    const bool need_unitigs = env_on("KOMB_TRUSS") || env_on("KOMB_V1_OUTPUTS");
    const auto unitigs = need_unitigs ? read_unitigs(args.unitigs) : std::unordered_map<std::string, std::string>();

    // runCore (src/graph.cpp:455-484)
    t0 = clk::now();
    std::vector<int32_t> deg((size_t)nv), core((size_t)nv);
    rc = komb_degree_coreness(ctx, deg.data(), core.data());
    if (rc != KOMB_OK) die_accel(ctx, "komb_degree_coreness", rc);
    const int max_coreness = nv ? *std::max_element(core.begin(), core.end()) : 0;
    std::vector<uint8_t> maxcore((size_t)nv, 0);
    {
        const std::string path = args.outdir + "/kcore.tsv";
        FILE *kcf = fopen(path.c_str(), "w+");
        if (!kcf) file_not_found(path);
        fprintf(kcf, "#VID\tName\tCoreness\tDegree\n");
        for (int64_t i = 0; i < nv; ++i)
            if (core[(size_t)i] == max_coreness) maxcore[(size_t)i] = 1;       // subgraph_nodes (:470-473)
        write_rows(kcf, nv, args.threads, [&](int64_t i, std::string &buf) {
            char tmp[48];
            int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)i);
            buf.append(tmp, (size_t)len);
            buf.append(names.name[(size_t)i]);
            len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\n", core[(size_t)i], deg[(size_t)i]);   // src/graph.cpp:474
            buf.append(tmp, (size_t)len);
        });
        fclose(kcf);
    }

    // onion decomposition (no counterpart in the reference; opt-in): onion.tsv beside kcore.tsv, one row per vertex in VID order
    if (env_on("KOMB_ONION")) {
        rc = komb_onion_run(ctx);
        if (rc != KOMB_OK) die_accel(ctx, "komb_onion_run", rc);
        std::vector<int32_t> layer((size_t)nv), ocore((size_t)nv);
        rc = komb_onion_fetch(ctx, layer.data(), ocore.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_onion_fetch", rc);
        const std::string path = args.outdir + "/onion.tsv";
        FILE *of = fopen(path.c_str(), "w+");
        if (!of) file_not_found(path);
        fprintf(of, "#VID\tName\tCoreness\tLayer\n");
        write_rows(of, nv, args.threads, [&](int64_t i, std::string &buf) {
            char tmp[48];
            int len = snprintf(tmp, sizeof(tmp), "%d\t", (int)i);
            buf.append(tmp, (size_t)len);
            buf.append(names.name[(size_t)i]);
            len = snprintf(tmp, sizeof(tmp), "\t%d\t%d\n", ocore[(size_t)i], layer[(size_t)i]);
            buf.append(tmp, (size_t)len);
        });
        fclose(of);
    }

    // connected components of a k-core (no counterpart in the reference; opt-in): core_components.tsv
    const char *comp_env = getenv("KOMB_COMPONENTS");
    const bool comp_on = comp_env && *comp_env;
    if (comp_on) {
        char *end = nullptr;
        const bool comp_max = strcmp(comp_env, "max") == 0;
        const long kc = comp_max ? (long)KOMB_COMP_K_MAX : strtol(comp_env, &end, 10);
        if (!comp_max && (*end || kc < 0 || kc > 2147483647L)) {
            fprintf(stderr, "komb2: KOMB_COMPONENTS=%s: expected a coreness threshold >= 0 or max\n", comp_env);
            leave(EXIT_FAILURE);
        }
        rc = komb_components_run(ctx, KOMB_COMP_CORE, (int32_t)kc);
        if (rc != KOMB_OK) die_accel(ctx, "komb_components_run", rc);
        write_components(ctx, args.outdir + "/core_components.tsv", "Coreness", names, nv, args.threads,
                         [&](int64_t i) { return (int)core[(size_t)i]; });
    }

    // the nesting forest of the k-core components over all k (no counterpart in the reference; opt-in): core_hierarchy*.tsv
    const bool hier_on = env_on("KOMB_HIERARCHY");
    if (hier_on)
        write_hierarchy(ctx, KOMB_COMP_CORE, args.outdir, "core", "Coreness", names, nv, args.threads,
                        [&](int64_t i) { return (int)core[(size_t)i]; });

    // densest-subgraph search on the coreness just computed (no counterpart in the reference; opt-in): KOMB_DENSEST=<rounds>
    const char *dens_env = getenv("KOMB_DENSEST");
    if (dens_env && *dens_env) {
        char *end = nullptr;
        const long it = strtol(dens_env, &end, 10);
        if (*end || it < 0 || it > 2147483647L) {
            fprintf(stderr, "komb2: KOMB_DENSEST=%s: expected a number of rounds >= 0\n", dens_env);
            leave(EXIT_FAILURE);
        }
        write_densest(ctx, (int32_t)it, args.outdir, names, nv, args.threads, core);
    }

    // k-truss communities of the truss stage's result (no counterpart in the reference; opt-in, needs KOMB_TRUSS=1)
    const char *comm_env = getenv("KOMB_COMMUNITIES");
    const bool comm_on = comm_env && *comm_env;
    long comm_k = (long)KOMB_COMM_K_MAX;
    if (comm_on && strcmp(comm_env, "max") != 0) {
        char *end = nullptr;
        comm_k = strtol(comm_env, &end, 10);
        if (*end || comm_k < 0 || comm_k > 2147483647L) {
            fprintf(stderr, "komb2: KOMB_COMMUNITIES=%s: expected a trussness threshold >= 0 or max\n", comm_env);
            leave(EXIT_FAILURE);
        }
    }

    // biconnected components of the truss stage's result (no counterpart in the reference; opt-in, needs KOMB_TRUSS=1)
    const char *bc_env = getenv("KOMB_BICONNECTED");
    const bool bc_on = bc_env && *bc_env;
    long bc_k = (long)KOMB_BICONN_K_MAX;
    if (bc_on && strcmp(bc_env, "max") != 0) {
        char *end = nullptr;
        bc_k = strtol(bc_env, &end, 10);
        if (*end || bc_k < 0 || bc_k > 2147483647L) {
            fprintf(stderr, "komb2: KOMB_BICONNECTED=%s: expected a trussness threshold >= 0 or max\n", bc_env);
            leave(EXIT_FAILURE);
        }
    }

    // (3,4)-nucleus decomposition of the truss stage's result (no counterpart in the reference; opt-in, needs KOMB_TRUSS=1)
    const char *nuc_env = getenv("KOMB_NUCLEUS");
    const bool nuc_on = nuc_env && !strcmp(nuc_env, "1");
    if (nuc_env && *nuc_env && !nuc_on && strcmp(nuc_env, "0") != 0) {
        fprintf(stderr, "komb2: KOMB_NUCLEUS=%s: expected 0 or 1\n", nuc_env);
        leave(EXIT_FAILURE);
    }

    // the nuclei of that decomposition and their forest (no counterpart in the reference; opt-in, needs KOMB_TRUSS=1)
    const char *nh_env = getenv("KOMB_NUCLEUS_HIERARCHY");
    const bool nh_on = nh_env && !strcmp(nh_env, "1");
    if (nh_env && *nh_env && !nh_on && strcmp(nh_env, "0") != 0) {
        fprintf(stderr, "komb2: KOMB_NUCLEUS_HIERARCHY=%s: expected 0 or 1\n", nh_env);
        leave(EXIT_FAILURE);
    }

    // the maximum cliques of the truss stage's result (no counterpart in the reference; opt-in, needs KOMB_TRUSS=1)
    const char *mc_env = getenv("KOMB_MAX_CLIQUE");
    const bool mc_on = mc_env && *mc_env && strcmp(mc_env, "0") != 0;
    long long mc_budget = 0;
    if (mc_on) {
        char *end = nullptr;
        errno = 0;
        mc_budget = strtoll(mc_env, &end, 10);
        if (*end || mc_budget < 1 || errno) {
            fprintf(stderr, "komb2: KOMB_MAX_CLIQUE=%s: expected 0, 1 or a node budget\n", mc_env);
            leave(EXIT_FAILURE);
        }
        if (mc_budget == 1) mc_budget = 0;                 // (1: on, with the library's default budget)
    }

    // the clique census of the truss stage's result (no counterpart in the reference; opt-in, needs KOMB_TRUSS=1):
    // KOMB_CLIQUE_CENSUS=<k_lo>:<k_hi>[:<k_local>], <k_hi> a number or "max"
    const char *cc_env = getenv("KOMB_CLIQUE_CENSUS");
    const bool cc_on = cc_env && *cc_env && strcmp(cc_env, "0") != 0;
    int32_t cc_window[3] = {0, 0, 0};
    if (cc_on) {
        auto number = [](const char *&q) -> long long {   // a decimal number of at least 2 at q, -2 if there is none
            if (*q < '0' || *q > '9') return -2;
            char *end = nullptr;
            errno = 0;
            const long long v = strtoll(q, &end, 10);
            q = end;
            return errno || v < 2 || v > 0x7FFFFFFF ? -2 : v;
        };
        const char *q = cc_env;
        const long long lo = number(q);
        long long hi = -2, loc = 0;
        if (*q == ':') {
            ++q;
            if (strncmp(q, "max", 3) == 0) { hi = -1; q += 3; }
            else hi = number(q);
            if (*q == ':') { ++q; loc = number(q); }
        }
        if (*q || lo == -2 || hi == -2 || (hi != -1 && hi < lo) || (loc != 0 && (loc < lo || (hi != -1 && loc > hi)))) {
            fprintf(stderr, "komb2: KOMB_CLIQUE_CENSUS=%s: expected 0 or <k_lo>:<k_hi>[:<k_local>] with 2 <= k_lo <= k_hi, k_hi a number or max, k_local inside\n", cc_env);
            leave(EXIT_FAILURE);
        }
        cc_window[0] = (int32_t)lo; cc_window[1] = (int32_t)hi; cc_window[2] = (int32_t)loc;
    }

    // the maximal cliques of the truss stage's result (no counterpart in the reference; opt-in, needs KOMB_TRUSS=1):
    // KOMB_MAXIMAL_CLIQUES=<k_min>[:<budget>]
    const char *mx_env = getenv("KOMB_MAXIMAL_CLIQUES");
    const bool mx_on = mx_env && *mx_env && strcmp(mx_env, "0") != 0;
    long long mx_k_min = 0, mx_budget = 0;
    if (mx_on) {
        auto number = [](const char *&q, long long lo, long long hi) -> long long {   // a decimal number of [lo, hi] at q, -1 if there is none
            if (*q < '0' || *q > '9') return -1;
            char *end = nullptr;
            errno = 0;
            const long long v = strtoll(q, &end, 10);
            q = end;
            return errno || v < lo || v > hi ? -1 : v;
        };
        const char *q = mx_env;
        mx_k_min = number(q, 2, 0x7FFFFFFF);
        if (*q == ':') { ++q; mx_budget = number(q, 1, 0x7FFFFFFFFFFFFFFFll); }
        if (*q || mx_k_min < 0 || mx_budget < 0) {
            fprintf(stderr, "komb2: KOMB_MAXIMAL_CLIQUES=%s: expected 0 or <k_min>[:<budget>] with k_min >= 2 and a node budget >= 1\n", mx_env);
            leave(EXIT_FAILURE);
        }
    }

    // the k-clique communities of the truss stage's result (no counterpart in the reference; opt-in, needs KOMB_TRUSS=1):
    // KOMB_CLIQUE_COMMUNITIES=<k>[:<budget>]
    const char *pc_env = getenv("KOMB_CLIQUE_COMMUNITIES");
    const bool pc_on = pc_env && *pc_env && strcmp(pc_env, "0") != 0;
    long long pc_k = 0, pc_budget = 0;
    if (pc_on) {
        auto number = [](const char *&q, long long lo, long long hi) -> long long {   // a decimal number of [lo, hi] at q, -1 if there is none
            if (*q < '0' || *q > '9') return -1;
            char *end = nullptr;
            errno = 0;
            const long long v = strtoll(q, &end, 10);
            q = end;
            return errno || v < lo || v > hi ? -1 : v;
        };
        const char *q = pc_env;
        pc_k = number(q, 2, 0x7FFFFFFF);
        if (*q == ':') { ++q; pc_budget = number(q, 1, 0x7FFFFFFFFFFFFFFFll); }
        if (*q || pc_k < 0 || pc_budget < 0) {
            fprintf(stderr, "komb2: KOMB_CLIQUE_COMMUNITIES=%s: expected 0 or <k>[:<budget>] with k >= 2 and a pair-test budget >= 1\n", pc_env);
            leave(EXIT_FAILURE);
        }
    }

    // structural clustering of the whole graph (no counterpart in the reference; opt-in): KOMB_STRUCTURAL=<num>/<den>,<mu>.  It
    // makes a whole-graph k-truss run of its own, before the truss stage below replaces that result with the max core's.
    const char *sc_env = getenv("KOMB_STRUCTURAL");
    if (sc_env && *sc_env) {
        char *end = nullptr;
        const long num = strtol(sc_env, &end, 10);
        const long den = end != sc_env && *end == '/' && end[1] >= '0' && end[1] <= '9' ? strtol(end + 1, &end, 10) : -1;
        const long mu = den >= 0 && *end == ',' && end[1] >= '0' && end[1] <= '9' ? strtol(end + 1, &end, 10) : -1;
        if (mu < 2 || *end || num < 1 || num > den || den > 1000000L || mu > 2147483647L) {
            fprintf(stderr, "komb2: KOMB_STRUCTURAL=%s: expected <num>/<den>,<mu> with 1 <= num <= den <= 1000000 and mu >= 2\n", sc_env);
            leave(EXIT_FAILURE);
        }
        write_structural(ctx, (int32_t)num, (int32_t)den, (int32_t)mu, args.outdir, names, nv, args.threads);
    }

    // graphlet census of the whole graph (no counterpart in the reference; opt-in): KOMB_GRAPHLETS=1 | edges.  Like the
    // structural clustering it makes a whole-graph k-truss run of its own before the truss stage below.
    const char *gl_env = getenv("KOMB_GRAPHLETS");
    if (gl_env && *gl_env) {
        const bool gl_edges = !strcmp(gl_env, "edges");
        if (!gl_edges && strcmp(gl_env, "1") != 0) {
            fprintf(stderr, "komb2: KOMB_GRAPHLETS=%s: expected 1 or edges\n", gl_env);
            leave(EXIT_FAILURE);
        }
        write_graphlets(ctx, gl_edges, args.outdir, names, nv, args.threads);
    }

    // betweenness centrality of the whole graph (no counterpart in the reference; opt-in): KOMB_BETWEENNESS=all | <n>[:<seed>]
    const char *btw_env = getenv("KOMB_BETWEENNESS");
    if (btw_env && *btw_env) write_betweenness(ctx, parse_source_choice("KOMB_BETWEENNESS", btw_env), args.outdir, names, nv, args.threads);

    // distance analysis of the whole graph (no counterpart in the reference; opt-in): KOMB_DISTANCES=all | <n>[:<seed>]
    const char *dist_env = getenv("KOMB_DISTANCES");
    if (dist_env && *dist_env) write_distances(ctx, parse_source_choice("KOMB_DISTANCES", dist_env), args.outdir, names, nv, args.threads);

    // runTruss (src/graph.cpp:486-563) -- disabled in the reference at :478, opt-in here
    if (env_on("KOMB_TRUSS") && nv > 0) {
        fprintf(stdout, "BUILDING K-TRUSS:\n");
        fprintf(stdout, "Selected unitigs in maximal core.\n");
        rc = komb_truss_run(ctx, maxcore.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_truss_run", rc);
        int64_t ne_sub = 0;
        komb_truss_count(ctx, &ne_sub);
        fprintf(stdout, "Succesfully created a %d-core subgraph, with %d edges.\n", max_coreness, (int)ne_sub);
        std::vector<int32_t> eu((size_t)ne_sub), ev((size_t)ne_sub), tr((size_t)ne_sub);
        rc = komb_truss_fetch(ctx, eu.data(), ev.data(), tr.data());
        if (rc != KOMB_OK) die_accel(ctx, "komb_truss_fetch", rc);
        fprintf(stdout, "Computed trussness of edges.\n");
        const std::string path = args.outdir + "/truss_unitigs.fasta";
        FILE *tf = fopen(path.c_str(), "w+");
        if (!tf) file_not_found(path);
        const int threshold = ne_sub ? *std::max_element(tr.begin(), tr.end()) : 0;
        std::vector<uint8_t> in((size_t)nv, 0);
        int count = 0;
        for (int64_t e = 0; e < ne_sub; ++e)
            if (tr[(size_t)e] >= threshold) { in[(size_t)eu[(size_t)e]] = 1; in[(size_t)ev[(size_t)e]] = 1; }
        for (int64_t v = 0; v < nv; ++v) {                 // the reference iterates an unordered_set<int>: order unspecified
            if (!in[(size_t)v]) continue;
            ++count;
            fprintf(tf, ">Unitig_%s\n", names.name[(size_t)v].c_str());
            auto it = unitigs.find(names.name[(size_t)v]);
            if (it != unitigs.end()) fprintf(tf, "%s\n", it->second.c_str());
        }
        fclose(tf);
        fprintf(stdout, "Found %d unitigs in %d-truss, saved at %s\n", count, threshold + 1, path.c_str());   // "+1" as src/graph.cpp:557
        if (comp_on) {                                     // the records of truss_unitigs.fasta, split into components
            rc = komb_components_run(ctx, KOMB_COMP_TRUSS, KOMB_COMP_K_MAX);
            if (rc != KOMB_OK) die_accel(ctx, "komb_components_run", rc);
            int32_t k_used = 0;
            komb_components_info(ctx, nullptr, &k_used, nullptr, nullptr, nullptr, nullptr);
            write_components(ctx, args.outdir + "/truss_components.tsv", "Trussness", names, nv, args.threads,
                             [&](int64_t) { return (int)k_used; });
        }
        if (comm_on) {
            rc = komb_truss_communities_run(ctx, (int32_t)comm_k);
            if (rc != KOMB_OK) die_accel(ctx, "komb_truss_communities_run", rc);
            write_communities(ctx, args.outdir, names, nv, args.threads, eu, ev, tr);
        }
        if (env_on("KOMB_COMMUNITY_HIERARCHY"))            // the forest of the communities of the truss stage's result
            write_community_hierarchy(ctx, args.outdir, names, args.threads, eu, ev, tr);
        if (nuc_on) write_nucleus(ctx, args.outdir, names, nv, args.threads, eu, ev);
        if (nh_on) write_nucleus_hierarchy(ctx, args.outdir, names, args.threads, nuc_on);
        if (mc_on) write_max_clique(ctx, (int64_t)mc_budget, args.outdir, names, nv, args.threads);
        if (cc_on) write_clique_census(ctx, cc_window, args.outdir, names, nv, args.threads);
        if (mx_on) write_maximal_cliques(ctx, (int32_t)mx_k_min, (int64_t)mx_budget, args.outdir, names, nv, args.threads);
        if (pc_on) write_clique_communities(ctx, (int32_t)pc_k, (int64_t)pc_budget, mx_on && mx_k_min <= pc_k, args.outdir, names, nv, args.threads);
        if (hier_on) {                                     // the forest of the truss stage's result
            std::vector<int32_t> lvl((size_t)nv, 0);
            for (int64_t e = 0; e < ne_sub; ++e) {
                lvl[(size_t)eu[(size_t)e]] = std::max(lvl[(size_t)eu[(size_t)e]], tr[(size_t)e]);
                lvl[(size_t)ev[(size_t)e]] = std::max(lvl[(size_t)ev[(size_t)e]], tr[(size_t)e]);
            }
            write_hierarchy(ctx, KOMB_COMP_TRUSS, args.outdir, "truss", "Trussness", names, nv, args.threads,
                            [&](int64_t i) { return (int)lvl[(size_t)i]; });
        }
        if (bc_on) write_biconnected(ctx, (int32_t)bc_k, args.outdir, names, nv, args.threads);   // (last: it replaces the stage's k-truss result)
    }
    fprintf(stdout, "\nTime elapsed doing K-core decomposition: %.3f s\n", since(t0));
    fprintf(stdout, "Created Kcore\n");
    auto t_core = clk::now();
    fprintf(stdout, "\nTime elapsed for edgeInfo: %.3f s\n", std::chrono::duration<double>(t_core - t_generate).count());   // sic (src/komb2.cpp:124)
    const char *v1 = getenv("KOMB_V1_OUTPUTS");
    const bool v1_on = env_on("KOMB_V1_OUTPUTS");
    if (v1_on) combine_file(args.outdir, names, core, unitigs, args.threads);
    auto t_combine = clk::now();
    fprintf(stdout, "\nTime elapsed for combineFile: %.3f s\n", std::chrono::duration<double>(t_combine - t_core).count());

    corea_stage(ctx, args.outdir, deg, core, args.threads);  // anomalyDetection (src/graph.cpp:637-648)
    fprintf(stdout, "\nTime elapsed for anomalyDetection: %.3f s\n", since(t_combine));
    fprintf(stdout, "Identified anomalous unitigs\n");
    if (v1_on) split_anomalous(args.outdir, names, unitigs, strcmp(v1, "fixed") == 0, args.threads);
    fprintf(stdout, "Created anomalouss unitigs file\n");
    fprintf(stdout, "\nTime elapsed for KOMB: %.3f s\n", since(begin_komb));
    fprintf(stdout, "\nTime elapsed for analysis (sec) = %.3f \n", since(begin));
    komb_destroy(ctx);
    return 0;
}
