// smp_prep.cpp -- see smp_prep.h.  Pure host C++; every routine cites the reference lines whose RESULT it must
// reproduce exactly (tie-breaking included: the reference's exchange sorts are not stable, so they are restated
// swap for swap rather than replaced by std::sort).
#include "smp_prep.h"

#include <algorithm>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>

namespace gfsmp {

static void *default_alloc(size_t bytes) { return std::malloc(bytes ? bytes : 1); }
static void default_free(void *p) { std::free(p); }
void *(*table_alloc)(size_t) = default_alloc;
void (*table_free)(void *) = default_free;

namespace {

constexpr int kMaxVertices = 4096;  // per molecule, for the stack-resident vertex tables of the batch builder

// fn(i) for i in [0, n) on up to GF_PREP_THREADS (default: hardware concurrency, at most 32) host threads; every
// iteration writes disjoint memory, so the result does not depend on the thread count or on the schedule.  Iterations
// are handed out in small blocks from a shared counter: molecules differ a lot in cost (O(V^3) each).
// Worker threads are kept between calls (a training loop prepares a batch per step: spawning 31 threads for each of the
// seven parallel sections cost ~3 ms of a 24 ms preparation).  One job at a time; the caller takes part in it.
class WorkerPool {
public:
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        wake_.notify_all();
        for (size_t t = 0; t < threads_.size(); ++t) threads_[t].join();
    }
    // runs job() on `helpers` pool threads and on the calling thread; returns when all of them have finished
    void run(int helpers, const std::function<void()> &job) {
        std::lock_guard<std::mutex> one_job(run_);
        {
            std::lock_guard<std::mutex> lk(m_);
            while ((int)threads_.size() < helpers) {
                const int id = (int)threads_.size();
                threads_.emplace_back([this, id]() { loop(id); });
            }
            job_ = &job;
            want_ = helpers;
            pending_ = helpers;
            ++generation_;
        }
        wake_.notify_all();
        job();
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this]() { return pending_ == 0; });
        job_ = nullptr;
    }

private:
    void loop(int id) {
        unsigned seen = 0;
        for (;;) {
            const std::function<void()> *job;
            {
                std::unique_lock<std::mutex> lk(m_);
                wake_.wait(lk, [&]() { return stop_ || (generation_ != seen && id < want_); });
                if (stop_) return;
                seen = generation_;
                job = job_;
            }
            (*job)();
            std::lock_guard<std::mutex> lk(m_);
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::mutex run_, m_;
    std::condition_variable wake_, done_;
    std::vector<std::thread> threads_;
    const std::function<void()> *job_ = nullptr;
    unsigned generation_ = 0;
    int want_ = 0, pending_ = 0;
    bool stop_ = false;
};
// One pool per CALLING thread: a loop that prepares two batches at once on two host threads (the graph preparation of a batch
// takes longer than its device step since round 2) gets two sets of workers instead of queueing on one.
WorkerPool &pool() {
    static thread_local WorkerPool p;
    return p;
}

template <typename Fn>
void parallel_for(int n, const Fn &fn) {
    int nt = (int)std::thread::hardware_concurrency();
    if (const char *e = std::getenv("GF_PREP_THREADS")) nt = std::atoi(e);
    nt = std::max(1, std::min(nt, std::getenv("GF_PREP_THREADS") ? 128 : 32));
    if (n < 64 || nt == 1) {
        for (int i = 0; i < n; ++i) fn(i);
        return;
    }
    const int block = std::max(1, std::min(16, n / (nt * 8)));
    std::atomic<int> next(0);
    const std::function<void()> worker = [&]() {
        for (;;) {
            const int lo = next.fetch_add(block);
            if (lo >= n) return;
            const int hi = std::min(n, lo + block);
            for (int i = lo; i < hi; ++i) fn(i);
        }
    };
    pool().run(nt - 1, worker);
}

// a handful of independent tasks (one per level), each on its own thread
template <typename Fn>
void parallel_tasks(int n, const Fn &fn) {
    if (std::getenv("GF_PREP_THREADS") && std::atoi(std::getenv("GF_PREP_THREADS")) <= 1) {
        for (int i = 0; i < n; ++i) fn(i);
        return;
    }
    std::atomic<int> next(0);
    const std::function<void()> worker = [&]() {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= n) return;
            fn(i);
        }
    };
    pool().run(n - 1, worker);
}

const int kInf = 1000000000;  // SMP_omega.h:1064

// SMP_omega.h:358-380.  The initialisation visits (i,j) in row-major order and, on an edge, writes BOTH [i][j] and
// [j][i]; a later visit of (j,i) overwrites [j][i] again.  Restated literally so asymmetric inputs behave the same.
void hop_distances(int V, const int *adj, std::vector<int> *out) {
    std::vector<int> &sp = *out;
    sp.assign((size_t)V * V, 0);
    for (int i = 0; i < V; ++i)
        for (int j = 0; j < V; ++j) {
            sp[i * V + j] = (i == j) ? 0 : kInf;
            if (i != j && adj[i * V + j] > 0) {
                sp[i * V + j] = 1;
                sp[j * V + i] = 1;
            }
        }
    for (int k = 0; k < V; ++k)
        for (int i = 0; i < V; ++i)
            for (int j = 0; j < V; ++j) sp[i * V + j] = std::min(sp[i * V + j], sp[i * V + k] + sp[k * V + j]);
}

// SMP_omega.h:382-404: histogram[v][d*F + f] = sum of the raw feature f over vertices at hop distance exactly d.
void wl_features(const Config &cfg, int V, const double *feature, const std::vector<int> &sp, std::vector<double> *out) {
    const int F = cfg.nFeatures, FD = cfg.fdim();
    out->assign((size_t)V * FD, 0.0);
    for (int v = 0; v < V; ++v)
        for (int d = 0; d <= cfg.nDepth; ++d)
            for (int u = 0; u < V; ++u)
                if (sp[u * V + v] == d)
                    for (int f = 0; f < F; ++f) (*out)[(size_t)v * FD + d * F + f] += feature[(size_t)u * F + f];
}

// SMP_omega.h:406-434: lexicographic compare of the histograms, exchange sort into DESCENDING order, rank = position.
int compare_wl(const std::vector<double> &wl, int FD, int u, int v) {
    for (int f = 0; f < FD; ++f) {
        if (wl[(size_t)u * FD + f] < wl[(size_t)v * FD + f]) return -1;
        if (wl[(size_t)u * FD + f] > wl[(size_t)v * FD + f]) return 1;
    }
    return 0;
}

void rank_vertices(int V, int FD, const std::vector<double> &wl, std::vector<int> *rank) {
    std::vector<int> order(V);
    for (int v = 0; v < V; ++v) order[v] = v;
    for (int i = 0; i < V; ++i)
        for (int j = i + 1; j < V; ++j)
            if (compare_wl(wl, FD, order[i], order[j]) < 0) std::swap(order[i], order[j]);
    rank->assign(V, 0);
    for (int i = 0; i < V; ++i) (*rank)[order[i]] = i;
}

// SMP_omega.h:476-507: order by (hop distance from v, rank) with the reference's exchange sort, then drop whole
// farthest hop shells until the field fits.
// use_rank = false: the `_physics` variant of limit_receptive_field (SMP_omega_physics.h:436-450) swaps on distance only.
void cap_field(int v, int V, int cap, const std::vector<int> &sp, const std::vector<int> &rank, std::vector<int> *field, bool use_rank) {
    std::vector<int> &A = *field;
    for (size_t i = 0; i < A.size(); ++i)
        for (size_t j = i + 1; j < A.size(); ++j) {
            const int di = sp[v * V + A[i]], dj = sp[v * V + A[j]];
            if (di > dj) {
                std::swap(A[i], A[j]);
            } else if (use_rank && di == dj && rank[A[i]] > rank[A[j]]) {
                std::swap(A[i], A[j]);
            }
        }
    while ((int)A.size() > cap) {
        const int d = sp[v * V + A.back()];
        while (!A.empty() && sp[v * V + A.back()] == d) A.pop_back();
    }
}

}  // namespace

void prepare_molecule(const Config &cfg, int V, const int *adj, const double *feature, Molecule *out) {
    out->V = V;
    hop_distances(V, adj, &out->hops);
    wl_features(cfg, V, feature, out->hops, &out->wl);
    rank_vertices(V, cfg.fdim(), out->wl, &out->rank);
    // receptive fields, SMP_omega.h:509-537
    out->phi.resize(cfg.nLevels + 1);
    for (int l = 0; l <= cfg.nLevels; ++l) {  // reused storage: clear, keep capacity
        out->phi[l].resize(V);
        for (int v = 0; v < V; ++v) out->phi[l][v].clear();
    }
    for (int v = 0; v < V; ++v) out->phi[0][v].assign(1, v);
    for (int l = 1; l <= cfg.nLevels; ++l)
        for (int v = 0; v < V; ++v) {
            std::vector<int> &field = out->phi[l][v];
            for (int u = 0; u < V; ++u) {
                if (out->hops[u * V + v] > 1) continue;
                const std::vector<int> &B = out->phi[l - 1][u];  // union_set (:436-449): append unseen, keep order
                for (size_t i = 0; i < B.size(); ++i)
                    if (std::find(field.begin(), field.end(), B[i]) == field.end()) field.push_back(B[i]);
            }
            if ((int)field.size() > cfg.max_receptive_field)
                cap_field(v, V, cfg.max_receptive_field, out->hops, out->rank, &field, !cfg.physics);
            if (cfg.has_WL_ordering && !cfg.physics)  // sort() at :451-459: exchange sort by ascending rank
                for (size_t i = 0; i < field.size(); ++i)
                    for (size_t j = i + 1; j < field.size(); ++j)
                        if (out->rank[field[i]] > out->rank[field[j]]) std::swap(field[i], field[j]);
        }
}

void build_batch(const Config &cfg, int nMol, const int *nVertices, const int *adj, const double *feature,
                 const double *coulomb, BatchLayout *out) {
    const int L = cfg.nLevels, FD = cfg.fdim(), F = cfg.nFeatures;
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    out->nMol = nMol;
    out->mols.resize(nMol);  // (the molecules of the previous batch keep their vectors: no allocator traffic in steady state)
    out->mol_first_vertex.assign(nMol + 1, 0);
    std::vector<size_t> adj_off(nMol + 1, 0);
    for (int m = 0; m < nMol; ++m) {
        out->mol_first_vertex[m + 1] = out->mol_first_vertex[m] + nVertices[m];
        adj_off[m + 1] = adj_off[m] + (size_t)nVertices[m] * nVertices[m];
    }
    const int totalV = out->mol_first_vertex[nMol];
    out->x.assign((size_t)totalV * FD, 0.f);
    if (out->device_tables) {
        out->mol_nv.assign(nVertices, nVertices + nMol);
        out->mol_adj_off.resize((size_t)nMol + 1);
        out->max_vertices = 1;
        for (int m = 0; m <= nMol; ++m) out->mol_adj_off[(size_t)m] = (int64_t)adj_off[m];
        for (int m = 0; m < nMol; ++m) out->max_vertices = std::max(out->max_vertices, nVertices[m]);
        out->mol_adj.assign(adj, adj + adj_off[nMol]);
        if (coulomb)
            out->mol_coul.assign(coulomb, coulomb + adj_off[nMol]);
        else
            out->mol_coul.clear();
    }
    parallel_for(nMol, [&](int m) {
        const int V = nVertices[m], v0 = out->mol_first_vertex[m];
        prepare_molecule(cfg, V, adj + adj_off[m], feature + (size_t)v0 * F, &out->mols[m]);
        for (size_t i = 0; i < (size_t)V * FD; ++i) out->x[(size_t)v0 * FD + i] = (float)out->mols[m].wl[i];
    });

    const bool timing = std::getenv("GF_PREP_TIMING") != nullptr;
    const std::chrono::steady_clock::time_point t_mol = std::chrono::steady_clock::now();
    // keep the vectors of a previous batch (their capacity): re-faulting ~50 MB of fresh pages costs more than the work
    out->level.resize(L + 1);
    for (int l = 0; l <= L; ++l) out->level[l].buckets.clear();
    // node numbering per level: level 0 in (molecule, vertex) order; level >= 1 bucketed by field size (stable)
    std::vector<std::vector<int> > node_of(L + 1, std::vector<int>(totalV, -1));  // [level][global vertex] -> node
    parallel_tasks(L + 1, [&](int l) {  // the levels are independent here
        LevelLayout &lv = out->level[l];
        std::vector<std::pair<int, int> > order;  // (size, global vertex)
        order.reserve(totalV);
        for (int m = 0; m < nMol; ++m)
            for (int v = 0; v < nVertices[m]; ++v)
                order.push_back(std::make_pair((int)out->mols[m].phi[l][v].size(), out->mol_first_vertex[m] + v));
        if (l > 0) std::stable_sort(order.begin(), order.end(),
                                    [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first < b.first; });
        lv.nNodes = totalV;
        lv.node_s.resize(totalV);
        lv.node_mol.resize(totalV);
        lv.node_vertex.resize(totalV);
        lv.node_row.resize(totalV);
        lv.node_p.resize(totalV);
        lv.node_pair.resize(totalV);
        int64_t row = 0, pp = 0, pair = 0;
        for (int n = 0; n < totalV; ++n) {
            const int s = order[n].first, gv = order[n].second;
            const int m = (int)(std::upper_bound(out->mol_first_vertex.begin(), out->mol_first_vertex.end(), gv) -
                                out->mol_first_vertex.begin()) - 1;
            node_of[l][gv] = n;
            lv.node_s[n] = s;
            lv.node_mol[n] = m;
            lv.node_vertex[n] = gv - out->mol_first_vertex[m];
            lv.node_row[n] = row;
            lv.node_p[n] = pp;
            lv.node_pair[n] = pair;
            if (lv.buckets.empty() || lv.buckets.back().s != s) {
                Bucket b = {s, 0, n, row, pp};
                lv.buckets.push_back(b);
            }
            lv.buckets.back().count += 1;
            row += (int64_t)s * s;
            pp += (int64_t)s * s * s;
            pair += s;
        }
        lv.rows = row;
        lv.ppos = pp;
        lv.pairs = pair;
        if (l == 0) {  // (a level-0 field is the vertex itself: the sources of level 1)
            lv.field.resize((size_t)totalV);
            for (int n = 0; n < totalV; ++n) lv.field[(size_t)n] = lv.node_vertex[n];
        }
        lv.node_center.assign(totalV, 0);
        {  // counting sort of the nodes by (register class of s, molecule); stable, so size-major order survives inside a key
            // (a class of their own for the nodes above 32 positions: tables-forward launches per register class over ranges of this
            //  order, and those nodes run another kernel)
            auto cls = [](int s) { return s <= 1 ? 0 : s <= 4 ? 1 : s <= 8 ? 2 : s <= 16 ? 3 : s <= 32 ? 4 : 5; };
            std::vector<int> start((size_t)6 * nMol + 1, 0);
            for (int n = 0; n < totalV; ++n) start[(size_t)cls(lv.node_s[n]) * nMol + lv.node_mol[n] + 1] += 1;
            for (size_t k = 0; k + 1 < start.size(); ++k) start[k + 1] += start[k];
            lv.mol_order.assign(totalV, 0);
            for (int n = 0; n < totalV; ++n) lv.mol_order[(size_t)start[(size_t)cls(lv.node_s[n]) * nMol + lv.node_mol[n]]++] = n;
        }
        {  // work items of the one-launch gather (smp_prep.h), molecule-major: (source, 64-lane chunk of its (p, channel quad) rows,
           // eight positions q) -- a source of more than eight positions is several items (round 4: eight accumulators per item)
            const int nl = std::max(1, cfg.nChanels / 4);
            std::vector<int> start((size_t)nMol + 1, 0);
            for (int n = 0; n < totalV; ++n) start[(size_t)lv.node_mol[n] + 1] += 1;
            for (size_t k = 0; k + 1 < start.size(); ++k) start[k + 1] += start[k];
            std::vector<int> order((size_t)totalV);
            for (int n = 0; n < totalV; ++n) order[(size_t)start[(size_t)lv.node_mol[n]]++] = n;
            lv.gather_items.clear();
            for (size_t i = 0; i < order.size(); ++i) {
                const int n = order[i], s = lv.node_s[n], chunks = (s * nl + 63) / 64;
                const int qchunks = s <= 8 ? 1 : (gather_pad(s) + 7) / 8;
                for (int h = 0; h < qchunks; ++h)
                    for (int c = 0; c < chunks; ++c) {
                        lv.gather_items.push_back(n);
                        lv.gather_items.push_back(c | (h << 16));
                    }
            }
        }
        for (int n = 0; n < totalV; ++n) {
            const std::vector<int> &fld = out->mols[lv.node_mol[n]].phi[l][lv.node_vertex[n]];
            const int v = lv.node_vertex[n];
            int c = -1;
            for (size_t i = 0; i < fld.size(); ++i)
                if (fld[i] == v) c = (int)i;
            lv.node_center[n] = c;  // always found: the centre survives the cap (SMP_omega.h:476-507)
        }
    });
    out->top_node_of_vertex = node_of[L];
    out->node_of_vertex = node_of;
    const std::chrono::steady_clock::time_point t_order = std::chrono::steady_clock::now();

    // The levels' tables are independent of each other (they only read node_of and the previous level's node bookkeeping), so
    // the serial parts of all levels run side by side (one task per level) and the node loops of all levels share one
    // parallel_for: four phases instead of four per level.
    std::vector<std::vector<int> > src_node_of_pair(L + 1);
    parallel_tasks(L, [&](int li) {   // phase A: sizes, quad tables and their launch order
        const int l = li + 1;
        LevelLayout &lv = out->level[l];
        const LevelLayout &prev = out->level[l - 1];
        std::vector<int> &pair_src_node = src_node_of_pair[l];
        (void)prev;
        (void)pair_src_node;
        // every element of these is written by the node loop below: resize only (no fill pass over ~50 MB per batch)
        const bool dev = out->device_tables;
        lv.adj.resize(dev ? 0 : (size_t)lv.rows);
        lv.rsum.resize(dev ? 0 : (size_t)lv.pairs);
        lv.rowscale.resize(dev ? 0 : (size_t)lv.nNodes * 2);
        lv.field.resize((size_t)lv.pairs);
        lv.quad_node.clear();
        lv.quad_b0.clear();
        lv.pair_node.resize((size_t)lv.pairs);
        lv.pair_src_row.resize((size_t)lv.pairs);
        lv.pair_src_pair.resize((size_t)lv.pairs);
        lv.pair_src_s.resize((size_t)lv.pairs);
        lv.pi.resize(dev ? 0 : (size_t)lv.rows);
        pair_src_node.assign((size_t)lv.pairs, 0);
        {
            lv.node_panel.resize((size_t)lv.nNodes);
            int np = 0;
            for (int n = 0; n < lv.nNodes; ++n) {
                lv.node_panel[(size_t)n] = np;
                const int sz = lv.node_s[n], gpp = sz >= 32 ? 1 : std::min(8, 32 / (sz < 1 ? 1 : sz));
                // (a node of more than 32 positions has no row panels: its row groups do not fit the 32-row tiles of the panel kernels --
                //  the workgroup kernels take it, smp_fused.hip: big_part; nodes are numbered by size, so those nodes come last)
                if (sz <= 32) np += (sz + gpp - 1) / gpp;
            }
            lv.npanels = np;
        }
        for (int n = 0; n < lv.nNodes; ++n)
            for (int b0 = 0; b0 < lv.node_s[n]; b0 += 4) {
                lv.quad_node.push_back(n);
                lv.quad_b0.push_back(b0);
            }
        {  // launch order of tables-forward: the consumers of one molecule's source tensors run together (stable counting sort)
            auto cls = [](int s) { return s <= 4 ? 0 : s <= 8 ? 1 : s <= 16 ? 2 : 3; };
            const size_t nq = lv.quad_node.size();
            std::vector<int> start((size_t)4 * nMol + 1, 0);
            for (size_t q = 0; q < nq; ++q) {
                const int n = lv.quad_node[q];
                start[(size_t)cls(lv.node_s[n]) * nMol + lv.node_mol[n] + 1] += 1;
            }
            for (size_t k = 0; k + 1 < start.size(); ++k) start[k + 1] += start[k];
            lv.quad_order.assign(nq, 0);
            for (size_t q = 0; q < nq; ++q) {
                const int n = lv.quad_node[q];
                lv.quad_order[(size_t)start[(size_t)cls(lv.node_s[n]) * nMol + lv.node_mol[n]]++] = (int)q;
            }
        }
    });
    const std::chrono::steady_clock::time_point t_A = std::chrono::steady_clock::now();
    parallel_for(L * totalV, [&](int k) {   // phase B: per node -- reduced adjacency, row sums, selection maps
        const int l = 1 + k / totalV, n = k % totalV;
        LevelLayout &lv = out->level[l];
        const LevelLayout &prev = out->level[l - 1];
        std::vector<int> &pair_src_node = src_node_of_pair[l];
        (void)prev;
        (void)pair_src_node;
            const int m = lv.node_mol[n], v = lv.node_vertex[n], s = lv.node_s[n];
            const int V = nVertices[m], v0 = out->mol_first_vertex[m];
            const int *madj = adj + adj_off[m];
            const std::vector<int> &field = out->mols[m].phi[l][v];
            for (int i = 0; i < s; ++i) lv.field[(size_t)lv.node_pair[n] + i] = field[i];
            const bool dev = out->device_tables;
            // reduced adjacency (:556-581): 1 on the diagonal and adj[v1][v2] elsewhere, or the Coulomb entries
            const double *mcoul = coulomb ? coulomb + adj_off[m] : nullptr;
            if (!dev) {
            for (int i = 0; i < s; ++i)
                for (int j = 0; j < s; ++j)
                    lv.adj[(size_t)lv.node_row[n] + (size_t)i * s + j] =
                        mcoul ? (float)mcoul[field[i] * V + field[j]]
                              : ((field[i] == field[j]) ? 1.f : (float)madj[field[i] * V + field[j]]);
            for (int i = 0; i < s; ++i) {  // gated row sums (RisiContraction_18.h:90: entries with A <= 0 are skipped)
                float rs = 0.f;
                for (int j = 0; j < s; ++j) {
                    const float av = lv.adj[(size_t)lv.node_row[n] + (size_t)i * s + j];
                    if (av > 0.f) rs += av;
                }
                lv.rsum[(size_t)lv.node_pair[n] + i] = rs;
            }
            {  // tot = sum of the gated adjacency, tr = its trace: the factors of contraction cases 1/3 and 7 (Appendix A.2)
                float tot = 0.f, tr = 0.f;
                for (int i = 0; i < s; ++i) {
                    tot += lv.rsum[(size_t)lv.node_pair[n] + i];
                    const float av = lv.adj[(size_t)lv.node_row[n] + (size_t)i * s + i];
                    if (av > 0.f) tr += av;
                }
                lv.rowscale[2 * (size_t)n] = tot;      // (expanded to one pair per row on the device: gf_smp_prepare)
                lv.rowscale[2 * (size_t)n + 1] = tr;
            }
            }
            int16_t pos[kMaxVertices];  // position of a vertex inside phi_{l-1}(w), -1 outside; reset after each neighbour
            if (V > kMaxVertices) std::abort();  // (gf_smp_prepare rejects such molecules before it gets here)
            for (int i = 0; i < V; ++i) pos[i] = -1;
            for (int a = 0; a < s; ++a) {
                const int w = field[a];
                const int64_t e = lv.node_pair[n] + a;
                const int src = node_of[l - 1][v0 + w];
                const std::vector<int> &wf = out->mols[m].phi[l - 1][w];
                lv.pair_node[(size_t)e] = n;
                pair_src_node[(size_t)e] = src;
                lv.pair_src_row[(size_t)e] = prev.node_row[src];
                lv.pair_src_pair[(size_t)e] = prev.node_pair[src];
                lv.pair_src_s[(size_t)e] = (int)wf.size();
                if (dev) continue;
                // selection map: X[i][k] = [phi_l(v)[i] == phi_{l-1}(w)[k]]   (:461-474)
                for (size_t k = 0; k < wf.size(); ++k) pos[wf[k]] = (int16_t)k;
                for (int p = 0; p < s; ++p) lv.pi[(size_t)lv.node_row[n] + (size_t)a * s + p] = pos[field[p]];
                for (size_t k = 0; k < wf.size(); ++k) pos[wf[k]] = -1;
            }
            });
    const std::chrono::steady_clock::time_point t_B = std::chrono::steady_clock::now();
    parallel_tasks(L, [&](int li) {   // phase C: consumer lists of the backward gather (prefix sums: serial per level)
        const int l = li + 1;
        LevelLayout &lv = out->level[l];
        const LevelLayout &prev = out->level[l - 1];
        std::vector<int> &pair_src_node = src_node_of_pair[l];
        (void)prev;
        (void)pair_src_node;
        // inverse index for the backward gather: consumers of a source node in increasing pair order (= fixed
        // summation order on the device), offsets by prefix sums, then a parallel fill
        lv.cons_ptr.assign((size_t)prev.nNodes + 1, 0);
        for (int64_t e = 0; e < lv.pairs; ++e) lv.cons_ptr[(size_t)pair_src_node[(size_t)e] + 1] += 1;
        for (int w = 0; w < prev.nNodes; ++w) lv.cons_ptr[(size_t)w + 1] += lv.cons_ptr[(size_t)w];
        std::vector<int64_t> cursor(lv.cons_ptr.begin(), lv.cons_ptr.end() - 1);
        tvec<int64_t> &cons_pair = lv.cons_pair;
        cons_pair.assign((size_t)lv.pairs, 0);
        for (int64_t e = 0; e < lv.pairs; ++e) cons_pair[(size_t)cursor[(size_t)pair_src_node[(size_t)e]]++] = e;
        if (out->device_tables) {   // (the device derives the per-consumer entries from cons_pair: smp_prepare.hip, build_consumer_entries)
            lv.cons_slab.clear();
            lv.cons_s.clear();
            lv.cons_row.clear();
            lv.cons_a.clear();
        } else {
            lv.cons_slab.assign((size_t)lv.pairs, 0);
            lv.cons_s.assign((size_t)lv.pairs, 0);
            lv.cons_row.assign((size_t)lv.pairs, 0);
            lv.cons_a.assign((size_t)lv.pairs, 0);
        }
        lv.cons_inv_off.assign((size_t)lv.pairs, 0);
        int64_t inv_total = 0;
        for (int w = 0; w < prev.nNodes; ++w)
            for (int64_t c = lv.cons_ptr[(size_t)w]; c < lv.cons_ptr[(size_t)w + 1]; ++c) {
                lv.cons_inv_off[(size_t)c] = inv_total;
                inv_total += prev.node_s[w];
            }
        lv.inv_count = inv_total;
        if (out->device_tables)
            lv.inv.clear();
        else
            lv.inv.assign((size_t)inv_total, (int16_t)-1);
        lv.cons_qbase.assign((size_t)prev.nNodes, 0);
        int64_t q = 0;
        for (int w = 0; w < prev.nNodes; ++w) {
            lv.cons_qbase[(size_t)w] = q;
            q += (lv.cons_ptr[(size_t)w + 1] - lv.cons_ptr[(size_t)w]) * gather_pad(prev.node_s[w]);
        }
        lv.qrec_total = q;
    });
    const std::chrono::steady_clock::time_point t_C = std::chrono::steady_clock::now();
    if (!out->device_tables)
    parallel_for(L * totalV, [&](int k) {   // phase D: per source node -- its consumers' entries and inverse maps (host-built tables only)
        const int l = 1 + k / totalV, w = k % totalV;
        LevelLayout &lv = out->level[l];
        const LevelLayout &prev = out->level[l - 1];
        std::vector<int> &pair_src_node = src_node_of_pair[l];
        (void)prev;
        (void)pair_src_node;
            for (int64_t c = lv.cons_ptr[(size_t)w]; c < lv.cons_ptr[(size_t)w + 1]; ++c) {
                const int64_t e = lv.cons_pair[(size_t)c];
                const int n = lv.pair_node[(size_t)e];
                const int s = lv.node_s[n], a = (int)(e - lv.node_pair[n]);
                lv.cons_slab[(size_t)c] = lv.node_p[n] + (int64_t)a * s * s;
                lv.cons_s[(size_t)c] = s;
                lv.cons_row[(size_t)c] = lv.node_row[n];
                lv.cons_a[(size_t)c] = a;
                if (out->device_tables) continue;
                int16_t *iv = &lv.inv[(size_t)lv.cons_inv_off[(size_t)c]];
                for (int p = 0; p < s; ++p) {
                    const int16_t k = lv.pi[(size_t)lv.node_row[n] + (size_t)a * s + p];
                    if (k >= 0) iv[k] = (int16_t)p;
                }
            }
            });
    if (timing) {
        const std::chrono::steady_clock::time_point t_end = std::chrono::steady_clock::now();
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
            return std::chrono::duration<double, std::milli>(b - a).count();
        };
        std::fprintf(stderr, "build_batch: molecules %.1f ms, node order %.1f ms, level tables %.1f ms (sizes / quads %.1f, per node %.1f, "
                             "consumer lists %.1f, inverse maps %.1f)\n",
                     ms(t_begin, t_mol), ms(t_mol, t_order), ms(t_order, t_end), ms(t_order, t_A), ms(t_A, t_B), ms(t_B, t_C), ms(t_C, t_end));
    }
}

// ---- first-order models (GraphFlow/SMP_theta.h) ---------------------------------------------------------------------------------
// The molecules are prepared as for SMP_omega (the two classes share Floyd-Warshall, the WL features, the ranking and the receptive
// fields, SMP_theta.h:327-507).  Per level: nodes in bucket (size) order, rows = the field positions, and the level's own (node, child)
// pairs -- the children of v are the vertices at hop distance <= 1 (:577-583), which under a cap need not lie inside phi_l(v).
void build_batch_theta(const Config &cfg, int nMol, const int *nVertices, const int *adj, const double *feature, BatchLayout *out) {
    const int L = cfg.nLevels, FD = cfg.fdim(), F = cfg.nFeatures;
    out->device_tables = false;
    out->nMol = nMol;
    out->mols.resize(nMol);
    out->mol_first_vertex.assign(nMol + 1, 0);
    std::vector<size_t> adj_off(nMol + 1, 0);
    out->max_vertices = 1;
    for (int m = 0; m < nMol; ++m) {
        out->mol_first_vertex[m + 1] = out->mol_first_vertex[m] + nVertices[m];
        adj_off[m + 1] = adj_off[m] + (size_t)nVertices[m] * nVertices[m];
        out->max_vertices = std::max(out->max_vertices, nVertices[m]);
    }
    const int totalV = out->mol_first_vertex[nMol];
    out->x.assign((size_t)totalV * FD, 0.f);
    parallel_for(nMol, [&](int m) {
        const int V = nVertices[m], v0 = out->mol_first_vertex[m];
        prepare_molecule(cfg, V, adj + adj_off[m], feature + (size_t)v0 * F, &out->mols[m]);
        for (size_t i = 0; i < (size_t)V * FD; ++i) out->x[(size_t)v0 * FD + i] = (float)out->mols[m].wl[i];
    });
    out->level.assign(L + 1, LevelLayout());
    std::vector<std::vector<int> > node_of(L + 1, std::vector<int>(totalV, -1));
    parallel_tasks(L + 1, [&](int l) {   // node numbering: level 0 in (molecule, vertex) order, levels >= 1 by field size (stable)
        LevelLayout &lv = out->level[l];
        std::vector<std::pair<int, int> > order;
        order.reserve(totalV);
        for (int m = 0; m < nMol; ++m)
            for (int v = 0; v < nVertices[m]; ++v)
                order.push_back(std::make_pair((int)out->mols[m].phi[l][v].size(), out->mol_first_vertex[m] + v));
        if (l > 0) std::stable_sort(order.begin(), order.end(),
                                    [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first < b.first; });
        lv.nNodes = totalV;
        lv.node_s.resize(totalV);
        lv.node_mol.resize(totalV);
        lv.node_vertex.resize(totalV);
        lv.node_row.resize(totalV);
        const bool sq = cfg.steerable_2d != 0 && l > 0;   // SMP_2D / ver4: f_l[v] is [s][s][C]; node_pair = the node's first column
        if (cfg.steerable_2d) lv.node_pair.resize(totalV);
        int64_t row = 0, col = 0;
        for (int n = 0; n < totalV; ++n) {
            const int s = order[n].first, gv = order[n].second;
            const int m = (int)(std::upper_bound(out->mol_first_vertex.begin(), out->mol_first_vertex.end(), gv) -
                                out->mol_first_vertex.begin()) - 1;
            node_of[l][gv] = n;
            lv.node_s[n] = s;
            lv.node_mol[n] = m;
            lv.node_vertex[n] = gv - out->mol_first_vertex[m];
            lv.node_row[n] = row;
            if (lv.buckets.empty() || lv.buckets.back().s != s) {
                Bucket b = {s, 0, n, row, 0};
                lv.buckets.push_back(b);
            }
            lv.buckets.back().count += 1;
            if (cfg.steerable_2d) lv.node_pair[n] = col;
            row += sq ? (int64_t)s * s : s;
            col += s;
        }
        lv.rows = row;   // sum s: f_l[v] is [s][C] (sum s^2 for a steerable second-order level)
        lv.ppos = 0;
        lv.th_bucket.clear();
        for (const Bucket &b : lv.buckets) {
            lv.th_bucket.push_back(b.s);
            lv.th_bucket.push_back(b.first_node);
            lv.th_bucket.push_back(b.count);
        }
    });
    out->top_node_of_vertex = node_of[L];
    out->node_of_vertex = node_of;
    for (int l = 1; l <= L; ++l) {   // (the nodes of a level in parallel below)
        LevelLayout &lv = out->level[l];
        const LevelLayout &pv = out->level[l - 1];
        // offsets first (serial prefix sums), then the maps of every node in parallel
        lv.th_child_ptr.assign((size_t)totalV + 1, 0);
        lv.th_cons_ptr.assign((size_t)totalV + 1, 0);
        for (int n = 0; n < totalV; ++n) {
            const int m = lv.node_mol[n], v = lv.node_vertex[n], V = nVertices[m];
            const std::vector<int> &hops = out->mols[m].hops;
            int nc = 0;
            for (int w = 0; w < V; ++w) nc += hops[(size_t)v * V + w] <= 1;
            lv.th_child_ptr[(size_t)n + 1] = nc;
        }
        for (int n = 0; n < totalV; ++n) lv.th_child_ptr[(size_t)n + 1] += lv.th_child_ptr[(size_t)n];
        const int64_t pairs = lv.th_child_ptr[(size_t)totalV];
        lv.pairs = pairs;
        lv.th_src_row.resize((size_t)pairs);
        lv.th_src_s.resize((size_t)pairs);
        lv.th_pi_off.resize((size_t)pairs);
        int64_t pi_total = 0;
        for (int n = 0; n < totalV; ++n) {
            const int64_t e0 = lv.th_child_ptr[(size_t)n], e1 = lv.th_child_ptr[(size_t)n + 1];
            for (int64_t e = e0; e < e1; ++e) {
                lv.th_pi_off[(size_t)e] = pi_total;
                pi_total += lv.node_s[n];
            }
        }
        lv.th_pi.resize((size_t)pi_total);
        // consumers of a source node w of level l - 1: the vertices v with hops[v][w] <= 1, ascending
        for (int w = 0; w < totalV; ++w) {
            const int m = pv.node_mol[w], u = pv.node_vertex[w], V = nVertices[m];
            const std::vector<int> &hops = out->mols[m].hops;
            int nc = 0;
            for (int v = 0; v < V; ++v) nc += hops[(size_t)v * V + u] <= 1;
            lv.th_cons_ptr[(size_t)w + 1] = nc;
        }
        for (int w = 0; w < totalV; ++w) lv.th_cons_ptr[(size_t)w + 1] += lv.th_cons_ptr[(size_t)w];
        lv.un_part_off.clear();
        if (cfg.unrestricted) {
            int64_t o = 0;
            for (const Bucket &b : lv.buckets) {
                lv.un_part_off.push_back(o);
                o += (int64_t)kUnrestrictedSplit * ((int64_t)cfg.filter_floats(l) * b.s * b.s + cfg.level_channels(l) +
                                                     (cfg.unrestricted == 3 ? cfg.level_channels(l - 1) : 0));
            }
            lv.un_part_off.push_back(o);
        }
        lv.th_weight.assign((size_t)totalV, 0);
        for (int m = 0; m < nMol; ++m) {   // the j-th vertex of its size in the molecule, ascending v (see th_weight)
            const int V = nVertices[m], g0 = out->mol_first_vertex[m];
            for (int v = 0; v < V; ++v) {
                const size_t sv = out->mols[m].phi[l][v].size();
                int j = 1;
                for (int u = 0; u < v; ++u) j += out->mols[m].phi[l][u].size() == sv;
                lv.th_weight[(size_t)node_of[l][g0 + v]] = cfg.unrestricted ? 1 : cfg.first_order == 2 ? (int)((long long)j * (j + 1) * (j + 2) / 6)   // (SMP_1D: see th_weight)
                                                           : cfg.steerable_2d == 1 ? (int)((long long)j * (j + 1) / 2) : j;   // (SMP_2D)
            }
        }
        lv.th_cons_row.resize((size_t)pairs);
        lv.th_cons_s.resize((size_t)pairs);
        lv.th_cons_node.resize((size_t)pairs);
        lv.th_inv_off.resize((size_t)pairs);
        int64_t inv_total = 0;
        for (int w = 0; w < totalV; ++w)
            for (int64_t c = lv.th_cons_ptr[(size_t)w]; c < lv.th_cons_ptr[(size_t)w + 1]; ++c) {
                lv.th_inv_off[(size_t)c] = inv_total;
                inv_total += pv.node_s[w];
            }
        lv.th_inv.resize((size_t)inv_total);
        lv.inv_count = inv_total;
        if (cfg.steerable_2d) lv.adj.resize((size_t)lv.rows);
        parallel_for(totalV, [&](int n) {
            if (cfg.steerable_2d) {   // the reduced adjacency of phi_l(v) (SMP_2D.h:459-470; SMP_2D_ver4.h:478-503: unit diagonal, rows / their sums)
                const int m = lv.node_mol[n], v = lv.node_vertex[n], V = nVertices[m];
                const int *A = adj + adj_off[m];
                const std::vector<int> &fv = out->mols[m].phi[l][v];
                const size_t s = fv.size();
                float *a = &lv.adj[(size_t)lv.node_row[n]];
                for (size_t i = 0; i < s; ++i) {
                    double degree = 0.0;
                    for (size_t j = 0; j < s; ++j) {
                        const double x = cfg.steerable_2d >= 2 && fv[i] == fv[j] ? 1.0 : (double)A[(size_t)fv[i] * V + fv[j]];
                        a[i * s + j] = (float)x;
                        degree += x;
                    }
                    if (cfg.steerable_2d >= 2)   // (ver4, ver5)
                        for (size_t j = 0; j < s; ++j) a[i * s + j] = (float)((double)a[i * s + j] / degree);
                }
            }
            {   // node n of level l as a consumer: its children
                const int m = lv.node_mol[n], v = lv.node_vertex[n], V = nVertices[m], g0 = out->mol_first_vertex[m];
                const Molecule &M = out->mols[m];
                const std::vector<int> &fv = M.phi[l][v];
                int64_t e = lv.th_child_ptr[(size_t)n];
                for (int w = 0; w < V; ++w) {
                    if (M.hops[(size_t)v * V + w] > 1) continue;
                    const int wn = node_of[l - 1][g0 + w];
                    const std::vector<int> &fw = M.phi[l - 1][w];
                    lv.th_src_row[(size_t)e] = pv.node_row[wn];
                    lv.th_src_s[(size_t)e] = (int)fw.size();
                    int16_t *pi = &lv.th_pi[(size_t)lv.th_pi_off[(size_t)e]];
                    for (size_t i = 0; i < fv.size(); ++i) {
                        const std::vector<int>::const_iterator it = std::find(fw.begin(), fw.end(), fv[i]);
                        pi[i] = it == fw.end() ? (int16_t)-1 : (int16_t)(it - fw.begin());
                    }
                    ++e;
                }
            }
            {   // node n of level l - 1 as a source: its consumers
                const int w = n, m = pv.node_mol[w], u = pv.node_vertex[w], V = nVertices[m], g0 = out->mol_first_vertex[m];
                const Molecule &M = out->mols[m];
                const std::vector<int> &fw = M.phi[l - 1][u];
                int64_t c = lv.th_cons_ptr[(size_t)w];
                for (int v = 0; v < V; ++v) {
                    if (M.hops[(size_t)v * V + u] > 1) continue;
                    const int vn = node_of[l][g0 + v];
                    const std::vector<int> &fv = M.phi[l][v];
                    lv.th_cons_row[(size_t)c] = lv.node_row[vn];
                    lv.th_cons_s[(size_t)c] = (int)fv.size();
                    lv.th_cons_node[(size_t)c] = vn;
                    int16_t *inv = &lv.th_inv[(size_t)lv.th_inv_off[(size_t)c]];
                    for (size_t j = 0; j < fw.size(); ++j) {
                        const std::vector<int>::const_iterator it = std::find(fv.begin(), fv.end(), fw[j]);
                        inv[j] = it == fv.end() ? (int16_t)-1 : (int16_t)(it - fv.begin());
                    }
                    ++c;
                }
            }
        });
    }
}

// NeuralFingerprint, GCN_1D, GCN_2D (Config::neighbourhood).  Per molecule: the hop distances and x (wl_features: the classes' shell sums;
// nDepth = 0 in form 1, where block 0 is the vertex's own feature).  Per distinct list: member (v, u) iff adj[v][u] > 0 (form 1, as
// NeuralFingerprint.h:186-190 writes it: no self loop, one-sided) or hops[v][u] <= radius (GCN_1D.h:230, GCN_2D.h:230), u ascending.
void build_batch_neighbourhood(const Config &cfg, int nMol, const int *nVertices, const int *adj, const double *feature, BatchLayout *out) {
    const int L = cfg.nLevels, FD = cfg.fdim(), F = cfg.nFeatures;
    out->device_tables = false;
    out->nMol = nMol;
    out->mols.assign(nMol, Molecule());
    out->mol_first_vertex.assign(nMol + 1, 0);
    std::vector<size_t> adj_off(nMol + 1, 0);
    out->max_vertices = 1;
    for (int m = 0; m < nMol; ++m) {
        out->mol_first_vertex[m + 1] = out->mol_first_vertex[m] + nVertices[m];
        adj_off[m + 1] = adj_off[m] + (size_t)nVertices[m] * nVertices[m];
        out->max_vertices = std::max(out->max_vertices, nVertices[m]);
    }
    const int totalV = out->mol_first_vertex[nMol];
    out->x.assign((size_t)totalV * FD, 0.f);
    out->nb_vertex_mol.assign((size_t)totalV, 0);
    parallel_for(nMol, [&](int m) {
        const int V = nVertices[m], v0 = out->mol_first_vertex[m];
        Molecule &M = out->mols[m];
        M.V = V;
        hop_distances(V, adj + adj_off[m], &M.hops);
        wl_features(cfg, V, feature + (size_t)v0 * F, M.hops, &M.wl);
        for (size_t i = 0; i < (size_t)V * FD; ++i) out->x[(size_t)v0 * FD + i] = (float)M.wl[i];
        for (int v = 0; v < V; ++v) out->nb_vertex_mol[(size_t)v0 + v] = m;
    });
    out->level.assign(L + 1, LevelLayout());
    for (int l = 0; l <= L; ++l) {
        out->level[l].nNodes = totalV;
        out->level[l].rows = totalV;
    }
    out->top_node_of_vertex.clear();
    out->node_of_vertex.clear();
    // the distinct lists: form 1 one (the adjacency), else one per radius that occurs
    std::vector<int> radius;
    out->nb_list_of_level.assign(L + 1, -1);
    for (int l = 1; l <= L; ++l) {
        const int r = cfg.nb_radius(l);
        size_t k = std::find(radius.begin(), radius.end(), r) - radius.begin();
        if (k == radius.size()) radius.push_back(r);
        out->nb_list_of_level[l] = (int)k;
    }
    out->nb_lists.assign(radius.size(), BatchLayout::NeighbourList());
    for (size_t k = 0; k < radius.size(); ++k) {
        BatchLayout::NeighbourList &nl = out->nb_lists[k];
        const int r = radius[k];
        nl.ptr.assign((size_t)totalV + 1, 0);
        nl.tptr.assign((size_t)totalV + 1, 0);
        auto member = [&](int m, int v, int u) {
            const int V = nVertices[m];
            return cfg.neighbourhood == 1 ? adj[adj_off[m] + (size_t)v * V + u] > 0 : out->mols[m].hops[(size_t)v * V + u] <= r;
        };
        for (int m = 0; m < nMol; ++m) {
            const int V = nVertices[m], v0 = out->mol_first_vertex[m];
            for (int v = 0; v < V; ++v)
                for (int u = 0; u < V; ++u)
                    if (member(m, v, u)) {
                        nl.ptr[(size_t)v0 + v + 1] += 1;
                        nl.tptr[(size_t)v0 + u + 1] += 1;
                    }
        }
        for (int g = 0; g < totalV; ++g) {
            nl.ptr[(size_t)g + 1] += nl.ptr[(size_t)g];
            nl.tptr[(size_t)g + 1] += nl.tptr[(size_t)g];
        }
        nl.idx.assign((size_t)nl.ptr[(size_t)totalV], 0);
        nl.tidx.assign((size_t)nl.ptr[(size_t)totalV], 0);
        parallel_for(nMol, [&](int m) {   // (a molecule's vertices own disjoint ranges of both tables)
            const int V = nVertices[m], v0 = out->mol_first_vertex[m];
            for (int v = 0; v < V; ++v) {
                int64_t e = nl.ptr[(size_t)v0 + v], t = nl.tptr[(size_t)v0 + v];
                for (int u = 0; u < V; ++u) {
                    if (member(m, v, u)) nl.idx[(size_t)e++] = v0 + u;
                    if (member(m, u, v)) nl.tidx[(size_t)t++] = v0 + u;   // (consumer u of source v)
                }
            }
        });
    }
}

// CGCN_1D, CGCN_2D (Config::covariant).  Per molecule: the hop distances (CGCN_1D.h:156-176, the text of GCN_1D.h's), x (:179-193, the
// shell sums), the masks' hop counts transposed -- cov_hop[v][i] = sp[i][v] (:203-209 reads shortest_paths[u][v]) -- and ONE list:
// member (v, u) iff adj[u][v] > 0 (:225-229: column v, the diagonal included), u ascending; its transpose for the reverse gather.
void build_batch_covariant(const Config &cfg, int nMol, const int *nVertices, const int *adj, const double *feature, BatchLayout *out) {
    const int L = cfg.nLevels, FD = cfg.fdim(), F = cfg.nFeatures, M = cfg.max_nVertices;
    out->device_tables = false;
    out->nMol = nMol;
    out->mols.assign(nMol, Molecule());
    out->mol_first_vertex.assign(nMol + 1, 0);
    std::vector<size_t> adj_off(nMol + 1, 0);
    out->max_vertices = 1;
    for (int m = 0; m < nMol; ++m) {
        out->mol_first_vertex[m + 1] = out->mol_first_vertex[m] + nVertices[m];
        adj_off[m + 1] = adj_off[m] + (size_t)nVertices[m] * nVertices[m];
        out->max_vertices = std::max(out->max_vertices, nVertices[m]);
    }
    const int totalV = out->mol_first_vertex[nMol];
    out->x.assign((size_t)totalV * FD, 0.f);
    out->nb_vertex_mol.assign((size_t)totalV, 0);
    out->cov_hop.assign((size_t)totalV * M, (unsigned char)255);
    out->nb_lists.assign(1, BatchLayout::NeighbourList());
    BatchLayout::NeighbourList &nl = out->nb_lists[0];
    nl.ptr.assign((size_t)totalV + 1, 0);
    nl.tptr.assign((size_t)totalV + 1, 0);
    parallel_for(nMol, [&](int m) {
        const int V = nVertices[m], v0 = out->mol_first_vertex[m];
        const int *A = adj + adj_off[m];
        Molecule &mol = out->mols[m];
        mol.V = V;
        hop_distances(V, A, &mol.hops);
        wl_features(cfg, V, feature + (size_t)v0 * F, mol.hops, &mol.wl);
        for (size_t i = 0; i < (size_t)V * FD; ++i) out->x[(size_t)v0 * FD + i] = (float)mol.wl[i];
        for (int v = 0; v < V; ++v) {
            out->nb_vertex_mol[(size_t)v0 + v] = m;
            for (int i = 0; i < V && i < M; ++i) {
                const int h = mol.hops[(size_t)i * V + v];
                out->cov_hop[((size_t)v0 + v) * M + i] = (unsigned char)(h < 0 || h > 255 ? 255 : h);
            }
            for (int u = 0; u < V; ++u) {   // (counts; the prefix sums follow)
                if (A[(size_t)u * V + v] > 0) nl.ptr[(size_t)v0 + v + 1] += 1;    // u in N(v)
                if (A[(size_t)v * V + u] > 0) nl.tptr[(size_t)v0 + v + 1] += 1;   // v in N(u): u consumes v
            }
        }
    });
    for (int g = 0; g < totalV; ++g) {
        nl.ptr[(size_t)g + 1] += nl.ptr[(size_t)g];
        nl.tptr[(size_t)g + 1] += nl.tptr[(size_t)g];
    }
    nl.idx.assign((size_t)nl.ptr[(size_t)totalV], 0);
    nl.tidx.assign((size_t)nl.tptr[(size_t)totalV], 0);
    parallel_for(nMol, [&](int m) {   // (a molecule's vertices own disjoint ranges of both tables)
        const int V = nVertices[m], v0 = out->mol_first_vertex[m];
        const int *A = adj + adj_off[m];
        for (int v = 0; v < V; ++v) {
            int64_t e = nl.ptr[(size_t)v0 + v], t = nl.tptr[(size_t)v0 + v];
            for (int u = 0; u < V; ++u) {
                if (A[(size_t)u * V + v] > 0) nl.idx[(size_t)e++] = v0 + u;
                if (A[(size_t)v * V + u] > 0) nl.tidx[(size_t)t++] = v0 + u;
            }
        }
    });
    out->nb_list_of_level.assign(L + 1, 0);
    out->level.assign(L + 1, LevelLayout());
    for (int l = 0; l <= L; ++l) {
        out->level[l].nNodes = totalV;
        out->level[l].rows = totalV;
    }
    out->top_node_of_vertex.clear();
    out->node_of_vertex.clear();
}

// GCN_*D_Kernel (Config::readout = 1): X_0, Y_0, X_1, Y_1, ..
void interleave_pairs(int nFeatures, int nPairs, const int *nVertices1, const int *adj1, const double *feature1, const int *nVertices2,
                      const int *adj2, const double *feature2, PairBatch *out) {
    size_t nv = 0, na = 0;
    for (int p = 0; p < nPairs; ++p)
        for (const int V : {nVertices1[p], nVertices2[p]}) {
            nv += (size_t)V;
            na += (size_t)V * (size_t)V;
        }
    out->nVertices.clear();
    out->adj.clear();
    out->feature.clear();
    out->nVertices.reserve(2 * (size_t)nPairs);
    out->adj.reserve(na);
    out->feature.reserve(nv * (size_t)nFeatures);
    size_t a1 = 0, a2 = 0, f1 = 0, f2 = 0;
    for (int p = 0; p < nPairs; ++p) {
        const size_t V1 = (size_t)nVertices1[p], V2 = (size_t)nVertices2[p];
        out->nVertices.push_back(nVertices1[p]);
        out->nVertices.push_back(nVertices2[p]);
        out->adj.insert(out->adj.end(), adj1 + a1, adj1 + a1 + V1 * V1);
        out->adj.insert(out->adj.end(), adj2 + a2, adj2 + a2 + V2 * V2);
        out->feature.insert(out->feature.end(), feature1 + f1, feature1 + f1 + V1 * (size_t)nFeatures);
        out->feature.insert(out->feature.end(), feature2 + f2, feature2 + f2 + V2 * (size_t)nFeatures);
        a1 += V1 * V1, a2 += V2 * V2;
        f1 += V1 * (size_t)nFeatures, f2 += V2 * (size_t)nFeatures;
    }
}

// LCNN, GCN_MW (Config::matrix_form).
void matrix_form_molecule(const Config &cfg, int molV, const int *adj, const double *feature, MatrixFormMolecule *out) {
    const int F = cfg.nFeatures;
    if (cfg.matrix_form == 2) {
        hop_distances(molV, adj, &out->hops);
        wl_features(cfg, molV, feature, out->hops, &out->wl);
        // create_norm_adj: D = the row sums of A + I, d = 1 / sqrt(D) where D > 0 (else D itself), P = D (A + I), A-hat = P D
        std::vector<double> d((size_t)molV, 0.0);
        auto a1 = [&](int i, int j) { return (double)adj[(size_t)i * molV + j] + (i == j ? 1.0 : 0.0); };
        for (int i = 0; i < molV; ++i) {
            for (int j = 0; j < molV; ++j) d[i] += a1(i, j);
            if (d[i] > 0.0) d[i] = 1.0 / std::sqrt(d[i]);
        }
        out->norm_adj.assign((size_t)molV * molV, 0.0);
        for (int i = 0; i < molV; ++i)
            for (int j = 0; j < molV; ++j) out->norm_adj[(size_t)i * molV + j] = (d[i] * a1(i, j)) * d[j];
        return;
    }
    // update_adjacency, update_feature: dummy vertices have no edges and zero features
    const int V = cfg.max_nVertices, FD = cfg.fdim(), k = cfg.nNeighbors;
    std::vector<int> padj((size_t)V * V, 0);
    std::vector<double> pfeat((size_t)V * F, 0.0);
    for (int i = 0; i < molV; ++i) {
        for (int j = 0; j < molV; ++j) padj[(size_t)i * V + j] = adj[(size_t)i * molV + j];
        for (int f = 0; f < F; ++f) pfeat[(size_t)i * F + f] = feature[(size_t)i * F + f];
    }
    hop_distances(V, padj.data(), &out->hops);
    wl_features(cfg, V, pfeat.data(), out->hops, &out->wl);
    // rank_vertices (LCNN.h:276-292): the exchange sort, descending
    std::vector<int> &order = out->order;
    order.resize((size_t)V);
    for (int v = 0; v < V; ++v) order[v] = v;
    for (int i = 0; i < V; ++i)
        for (int j = i + 1; j < V; ++j)
            if (compare_wl(out->wl, FD, order[i], order[j]) < 0) std::swap(order[i], order[j]);
    // find_sequence (LCNN.h:294-320)
    out->seq.assign((size_t)V * k, molV);
    for (int i = 0; i < V; ++i) {
        int j = 0;
        for (int dd = 0; dd < V && j < k; ++dd)
            for (int v = 0; v < V && j < k; ++v)
                if (out->hops[(size_t)order[i] * V + order[v]] == dd && order[v] < molV) out->seq[(size_t)i * k + j++] = order[v];
    }
}

bool lcnn_reads_past(const Config &cfg, int molV, const std::vector<int> &seq) {
    if (molV < cfg.max_nVertices) return false;
    for (size_t i = 0; i < seq.size(); ++i)
        if (seq[i] >= cfg.max_nVertices) return true;
    return false;
}

int build_batch_matrix_form(const Config &cfg, int nMol, const int *nVertices, const int *adj, const double *feature, BatchLayout *out) {
    const int L = cfg.nLevels, FD = cfg.fdim(), F = cfg.nFeatures;
    const bool lcnn = cfg.matrix_form == 1;
    const int V = cfg.max_nVertices, k = lcnn ? cfg.nNeighbors : 1;
    out->device_tables = false;
    out->nMol = nMol;
    out->mols.assign(nMol, Molecule());
    out->mol_first_vertex.assign(nMol + 1, 0);   // (the first ROW of a molecule: LCNN's molecules have V rows each)
    std::vector<size_t> adj_off(nMol + 1, 0), feat_off(nMol + 1, 0);
    out->max_vertices = 1;
    for (int m = 0; m < nMol; ++m) {
        out->mol_first_vertex[m + 1] = out->mol_first_vertex[m] + (lcnn ? V : nVertices[m]);
        adj_off[m + 1] = adj_off[m] + (size_t)nVertices[m] * nVertices[m];
        feat_off[m + 1] = feat_off[m] + (size_t)nVertices[m] * F;
        out->max_vertices = std::max(out->max_vertices, nVertices[m]);
    }
    const int rows = out->mol_first_vertex[nMol];
    out->x.assign((size_t)rows * FD, 0.f);
    out->nb_vertex_mol.assign((size_t)rows, 0);
    BatchLayout::RowLists &rl = out->rl;
    rl.order.assign(lcnn ? (size_t)nMol * V : 0, 0);
    rl.seq.assign(lcnn ? (size_t)nMol * V * k : 0, 0);
    rl.ptr.assign((size_t)rows + 1, 0);
    rl.tptr.assign((size_t)rows + 1, 0);
    std::vector<MatrixFormMolecule> mf((size_t)nMol);
    std::atomic<int> bad(nMol);
    parallel_for(nMol, [&](int m) {
        const int molV = nVertices[m], r0 = out->mol_first_vertex[m], nr = out->mol_first_vertex[m + 1] - r0;
        MatrixFormMolecule &M = mf[(size_t)m];
        matrix_form_molecule(cfg, molV, adj + adj_off[m], feature + feat_off[m], &M);
        out->mols[m].V = molV;
        out->mols[m].hops = M.hops;
        for (size_t i = 0; i < (size_t)nr * FD; ++i) out->x[(size_t)r0 * FD + i] = (float)M.wl[i];
        for (int r = 0; r < nr; ++r) out->nb_vertex_mol[(size_t)r0 + r] = m;
        if (lcnn) {
            if (lcnn_reads_past(cfg, molV, M.seq)) {
                int seen = bad.load();
                while (m < seen && !bad.compare_exchange_weak(seen, m)) {}
                return;
            }
            for (int i = 0; i < V; ++i) rl.order[(size_t)m * V + i] = M.order[i];
            for (size_t i = 0; i < (size_t)V * k; ++i) rl.seq[(size_t)m * V * k + i] = M.seq[i];
            for (int i = 0; i < V; ++i) {   // k entries per row, one per slot; the transposed row of u counts the (i, j) that read u
                rl.ptr[(size_t)r0 + i + 1] = k;
                for (int j = 0; j < k; ++j) rl.tptr[(size_t)r0 + M.seq[(size_t)i * k + j] + 1] += 1;
            }
        } else {
            for (int i = 0; i < molV; ++i)
                for (int j = 0; j < molV; ++j)
                    if (M.norm_adj[(size_t)i * molV + j] != 0.0) {
                        rl.ptr[(size_t)r0 + i + 1] += 1;
                        rl.tptr[(size_t)r0 + j + 1] += 1;
                    }
        }
    });
    if (bad.load() < nMol) return bad.load();
    for (int r = 0; r < rows; ++r) {
        rl.ptr[(size_t)r + 1] += rl.ptr[(size_t)r];
        rl.tptr[(size_t)r + 1] += rl.tptr[(size_t)r];
    }
    const size_t ne = (size_t)rl.ptr[(size_t)rows];
    rl.src.assign(ne, 0), rl.slot.assign(ne, 0), rl.coef.assign(ne, 1.f);
    rl.tsrc.assign(ne, 0), rl.tslot.assign(ne, 0), rl.tcoef.assign(ne, 1.f);
    parallel_for(nMol, [&](int m) {   // (a molecule's rows own disjoint ranges of both lists)
        const int molV = nVertices[m], r0 = out->mol_first_vertex[m];
        const MatrixFormMolecule &M = mf[(size_t)m];
        if (lcnn) {
            for (int i = 0; i < V; ++i)
                for (int j = 0; j < k; ++j) {
                    const size_t e = (size_t)rl.ptr[(size_t)r0 + i] + j;
                    rl.src[e] = r0 + M.seq[(size_t)i * k + j];
                    rl.slot[e] = j;
                }
            std::vector<int64_t> fill((size_t)V);
            for (int u = 0; u < V; ++u) fill[u] = rl.tptr[(size_t)r0 + u];
            for (int j = 0; j < k; ++j)   // slot-major, then ascending row: the fixed order of the reverse gather
                for (int i = 0; i < V; ++i) {
                    const size_t e = (size_t)fill[M.seq[(size_t)i * k + j]]++;
                    rl.tsrc[e] = r0 + i;
                    rl.tslot[e] = j;
                }
        } else {
            for (int i = 0; i < molV; ++i) {
                int64_t e = rl.ptr[(size_t)r0 + i], t = rl.tptr[(size_t)r0 + i];
                for (int j = 0; j < molV; ++j) {
                    const double a = M.norm_adj[(size_t)i * molV + j], at = M.norm_adj[(size_t)j * molV + i];
                    if (a != 0.0) rl.src[(size_t)e] = r0 + j, rl.coef[(size_t)e++] = (float)a;
                    if (at != 0.0) rl.tsrc[(size_t)t] = r0 + j, rl.tcoef[(size_t)t++] = (float)at;   // (consumer j of source i)
                }
            }
        }
    });
    rl.sptr.clear(), rl.tsptr.clear();
    if (lcnn) {   // the entries are ordered by (row, slot): counts per (row, slot), then their prefix sums
        auto offsets = [&](const tvec<int64_t> &ptr, const tvec<int> &slot, tvec<int64_t> *sp) {
            sp->assign((size_t)rows * k + 1, 0);
            for (int r = 0; r < rows; ++r)
                for (int64_t e = ptr[(size_t)r]; e < ptr[(size_t)r + 1]; ++e) (*sp)[(size_t)r * k + slot[(size_t)e] + 1] += 1;
            for (size_t i = 0; i < (size_t)rows * k; ++i) (*sp)[i + 1] += (*sp)[i];
        };
        offsets(rl.ptr, rl.slot, &rl.sptr);
        offsets(rl.tptr, rl.tslot, &rl.tsptr);
    }
    out->level.assign(L + 1, LevelLayout());
    for (int l = 0; l <= L; ++l) {
        out->level[l].nNodes = rows;
        out->level[l].rows = rows;
    }
    out->top_node_of_vertex.clear();
    out->node_of_vertex.clear();
    out->nb_lists.clear();
    out->nb_list_of_level.clear();
    return -1;
}

}  // namespace gfsmp
