// solver_setup.hip -- Solver::setup: the hierarchy (host, distributed; device hooks), the device
// formats of its levels and their cycle-order copies, the work vectors and the smoothers' own
// structures.  A sequence of stages over one SolverSetup.  SURVEY.md 8a rows a6-a10.
#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <thread>

#include "device.hpp"

namespace amg {

namespace {

// One worker thread that builds device formats (DevMatrix::build_view: host C++ format
// builds + uploads) in FIFO order while the setup thread coarsens the next level: level l's
// P and R and A_{l+1} are final once build_hierarchy reports level l done.  One rank only:
// a multi-rank build_view runs host collectives (the halo plan), which must not interleave
// with the hierarchy's.
class FormatWorker {
  public:
    explicit FormatWorker(int device) : th_([this, device] { run(device); }) {}
    ~FormatWorker() {
        if (th_.joinable()) stop();
    }
    void push(std::function<void()> job) {
        {
            std::lock_guard<std::mutex> g(mu_);
            q_.push_back(std::move(job));
        }
        cv_.notify_one();
    }
    // waits for every queued job; rethrows the first failure
    void finish() {
        stop();
        if (err_) std::rethrow_exception(err_);
    }

  private:
    void stop() {
        {
            std::lock_guard<std::mutex> g(mu_);
            done_ = true;
        }
        cv_.notify_one();
        th_.join();
    }
    void run(int device) {
        const hipError_t e = hipSetDevice(device);
        omp_quiet_thread();
        for (;;) {
            std::function<void()> job;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [this] { return done_ || !q_.empty(); });
                if (q_.empty()) return;
                job = std::move(q_.front());
                q_.pop_front();
            }
            if (err_) continue;  // after a failure: drain, report the first one
            try {
                HIP_CHECK(e);
                job();
            } catch (...) {
                err_ = std::current_exception();
            }
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
    bool done_ = false;
    std::exception_ptr err_;
    std::thread th_;
};

// Cycle order.  A Jacobi-smoothed level's kernels form each row's products
// and sum them in the row's stored order; neither depends on where the row sits or on the
// numbering of its columns.  So the cycle may run a level's points in any order Pi, as long as
// every operator touching the level carries the same Pi: A_l (rows and columns), P_l (rows),
// R_l (columns), R_{l-1} (rows) and P_{l-1} (columns).  Each row keeps its entries in the
// hierarchy's order, so every sum is the hierarchy's, bit for bit.  The order chosen is 8x8x8
// bricks of the fine grid: a level point sits at the fine point of its restriction row's
// first local column (for PMIS / RS its C point; for SA a fine point at its aggregate).  A
// block of consecutive rows is then a compact piece of space, and its x tile holds fewer
// lines than a block of a lexicographic slab (tests/analysis_brick_cut.py).  Grid-built
// operators (stencil constructors: each rank knows its box or slab), Jacobi levels only
// (hybrid-GS chunks are defined on the hierarchy's order), distributed levels only (not the
// coarsest, not replicated ones).  On N ranks each rank orders its own points; its send lists
// index its vectors through that order (DevMatrix::send_map), halo columns keep their global
// ids.  AMG_CYCLE_ORDER=0 turns it off.
//
// rows: new row -> old row, cols: old local column -> new (either empty: identity); halo
// columns (other ranks' points) keep their global ids
HostCSR permuted_csr(const HostCSR& M, int rank, const std::vector<int64_t>& rows, const std::vector<int64_t>& cols) {
    const int64_t clo = M.col_starts[rank], chi = M.col_starts[rank + 1];
    HostCSR B;
    B.n_global_rows = M.n_global_rows;
    B.n_global_cols = M.n_global_cols;
    B.row_starts = M.row_starts;
    B.col_starts = M.col_starts;
    const int64_t n = M.nrows();
    B.rp.assign((size_t)n + 1, 0);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
        const int64_t o = rows.empty() ? i : rows[i];
        B.rp[i + 1] = M.rp[o + 1] - M.rp[o];
    }
    for (int64_t i = 0; i < n; ++i) B.rp[i + 1] += B.rp[i];
    B.col.resize((size_t)M.nnz());
    B.val.resize((size_t)M.nnz());
#pragma omp parallel for schedule(dynamic, 4096)
    for (int64_t i = 0; i < n; ++i) {
        const int64_t o = rows.empty() ? i : rows[i];
        int64_t d = B.rp[i];
        for (int64_t k = M.rp[o]; k < M.rp[o + 1]; ++k, ++d) {
            const int64_t c = M.col[k];
            B.col[d] = cols.empty() || c < clo || c >= chi ? c : clo + cols[c - clo];
            B.val[d] = M.val[k];
        }
    }
    return B;
}

// the brick orders of a hierarchy's levels, one level at a time as the setup produces them
struct CycleOrder {
    static constexpr int64_t kB = 8, kMinRows = 4096;
    bool open = false;                             // the next level may still be permuted
    int64_t g[3] = {0, 0, 0};                      // level-0 local grid extents
    std::vector<char> on;                          // per level: permuted (the same on every rank)
    std::vector<std::vector<int64_t>> perm, inv;   // this rank's points: new -> old, old -> new
    std::vector<int64_t> at;                       // fine point of each point of the last level seen
    // AMG_P0_ROWMAP = 0 / 8 / 16 / 32: segment length S of the row order P_0's cycle copy is
    // stored in while level 0 itself stays in the hierarchy's order (0: none)
    static constexpr int kP0Seg = 16;
    int p0_seg = kP0Seg;
    int64_t n0 = 0;  // level-0 local rows

    // The stored row order of P_0's cycle copy: S x 8 x 8 bricks of this rank's grid in level 1's
    // brick sequence, inside a brick z, then y, then x.  Returns the level-0 row of every run of
    // S stored rows (a segment: S consecutive points of one grid line); empty: no map (level 1
    // not permuted, or the x extent no multiple of S).
    std::vector<int> p0_segments() const {
        std::vector<int> seg;
        const int64_t S = p0_seg, gz = std::max<int64_t>(g[2], 1);
        if (S <= 0 || !any(1) || any(0) || g[0] % S != 0 || g[0] * g[1] * gz != n0) return seg;
        seg.reserve((size_t)(n0 / S));
        for (int64_t bz = 0; bz < gz; bz += kB)
            for (int64_t by = 0; by < g[1]; by += kB)
                for (int64_t bx = 0; bx < g[0]; bx += S)
                    for (int64_t z = bz; z < std::min(bz + kB, gz); ++z)
                        for (int64_t y = by; y < std::min(by + kB, g[1]); ++y)
                            seg.push_back((int)((z * g[1] + y) * g[0] + bx));
        return seg;
    }

    void init(const DevMatrix& A, const amg_options& opt, const HostComm& comm, size_t maxl) {
        const char* e = std::getenv("AMG_CYCLE_ORDER");  // read per setup (tests compare both)
        if (const char* r = std::getenv("AMG_P0_ROWMAP")) {
            p0_seg = std::atoi(r);
            AMG_CHECK(p0_seg == 0 || p0_seg == 8 || p0_seg == 16 || p0_seg == 32, "AMG_P0_ROWMAP must be 0, 8, 16 or 32");
        }
        n0 = A.n_rows;
        std::copy(A.grid_local, A.grid_local + 3, g);
        const bool mine = g[0] > 0 && g[1] > 0 && g[0] * g[1] * std::max<int64_t>(g[2], 1) >= A.n_rows;
        open = !(e && std::atoi(e) == 0) && opt.smoother == AMG_SMOOTH_JACOBI &&
               comm.allreduce_sum(mine ? 0 : 1) == 0;  // every rank's operator came from a grid
        on.assign(maxl, 0);
        perm.assign(maxl, {});
        inv.assign(maxl, {});
        if (!open) return;
        at.resize((size_t)A.n_rows);
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < A.n_rows; ++i) at[i] = i;
    }
    bool any(size_t l) const { return l < on.size() && on[l]; }
    // level l + 1's order, from R_l (its rows are level l + 1's points, ascending fine columns)
    void next(size_t l, const HostCSR& R, const amg_options& opt, const HostComm& comm) {
        if (!open) return;
        const int64_t n = R.nrows(), ng = R.n_global_rows;
        const int64_t flo = R.col_starts[comm.rank], fhi = R.col_starts[comm.rank + 1];
        // large enough, not the coarsest level (dense-solved in the hierarchy's order) and not
        // replicated (multi-rank coarse levels held whole on every rank)
        if (ng < kMinRows || ng <= opt.max_coarse || (int)l + 2 >= opt.max_levels || l + 1 >= perm.size() ||
            (comm.nranks > 1 && opt.replicate_below > 0 && ng <= opt.replicate_below)) {
            open = false;
            return;
        }
        on[l + 1] = 1;
        std::vector<int64_t> up((size_t)n), key((size_t)n);
        const int64_t nbx = (g[0] + kB - 1) / kB, nby = (g[1] + kB - 1) / kB, nbz = (g[2] + kB - 1) / kB;
#pragma omp parallel for schedule(static)
        for (int64_t c = 0; c < n; ++c) {
            int64_t f = 0;  // the fine point of the row's first local column
            for (int64_t k = R.rp[c]; k < R.rp[c + 1]; ++k)
                if (R.col[k] >= flo && R.col[k] < fhi) {
                    f = at[R.col[k] - flo];
                    break;
                }
            const int64_t x = f % g[0], y = (f / g[0]) % g[1], z = f / (g[0] * g[1]);
            up[c] = f;
            key[c] = ((z / kB) * nby + y / kB) * nbx + x / kB;
        }
        at.swap(up);
        // stable counting sort by brick
        std::vector<int64_t> cnt((size_t)(nbx * nby * nbz) + 1, 0);
        for (int64_t c = 0; c < n; ++c) ++cnt[key[c] + 1];
        for (size_t b = 1; b < cnt.size(); ++b) cnt[b] += cnt[b - 1];
        std::vector<int64_t>& p = perm[l + 1];
        std::vector<int64_t>& q = inv[l + 1];
        p.resize((size_t)n);
        q.resize((size_t)n);
        for (int64_t c = 0; c < n; ++c) {
            const int64_t t = cnt[key[c]]++;
            p[t] = c;
            q[c] = t;
        }
    }
};

// What the stages of Solver::setup share.  Built in place and never copied: the device hooks
// and the worker jobs keep pointers into it.
struct SolverSetup {
    SolverSetup(Solver& s, DevMatrix& a)
        : S(s), A(a), comm(s.ctx->host), overlap(comm.nranks == 1), hgs(s.opt.smoother == AMG_SMOOTH_HYBRID_GS),
          mcgs(s.opt.smoother == AMG_SMOOTH_MC_GS), maxl((size_t)std::max(s.opt.max_levels, 1) + 1),
          im(s.opt.setup_device ? &images : nullptr), preA(maxl), preP(maxl), preR(maxl), preAc(maxl), prePc(maxl),
          preRc(maxl), mc_pre(maxl), tm(comm) {}
    SolverSetup(const SolverSetup&) = delete;
    SolverSetup& operator=(const SolverSetup&) = delete;

    Solver& S;
    DevMatrix& A;  // the caller's level-0 operator
    const HostComm& comm;
    // device formats of finished levels are built on worker threads during the hierarchy
    const bool overlap, hgs, mcgs;
    const size_t maxl;
    HostHierarchy H;
    // the level operators, P and R stay on the device between the setup steps that read them
    // (SetupImages); only the next level's operator is carried over
    SetupImages images;
    SetupImages* const im;
    SpgemmFn galerkin = nullptr;
    RapFn rap_fn = nullptr;
    LevelSetupFn level_fn = nullptr;
    TransposeFn transpose_fn = nullptr;
    // cycle order: the brick order of level l + 1 is fixed once R_l exists; the operators that
    // touch a permuted level are built as cycle-order copies (their hierarchy-order formats wait
    // for a caller that asks for them: DevMatrix::defer)
    CycleOrder co;
    std::vector<std::unique_ptr<DevMatrix>> preA, preP, preR, preAc, prePc, preRc;
    // multicolour GS: a level is coloured while the setup's images hold its operator (one rank:
    // level 0 before the hierarchy, A_{l+1} when level l is done); the levels left over are
    // coloured on their own once the operators are built (setup_mc_gs)
    std::vector<std::unique_ptr<Colouring>> mc_pre;
    PhaseTimer tm;
    // r5: a second worker builds each operator's GS structures as soon as its formats
    // exist (level 0 from the start), beside the format worker (sa27: 0.9 s of GS builds
    // after the hierarchy before)
    // gs_worker first, and the workers after everything their jobs touch: members are
    // destroyed in reverse order, so when build_hierarchy throws, worker and worker2 drain
    // (their A_{l+1} jobs push onto gs_worker) before gs_worker itself is joined and freed
    // 
    std::unique_ptr<FormatWorker> gs_worker, worker, worker2;

    void mc_colour(size_t l, const HostCSR& M) {
        if (mcgs && im && comm.nranks == 1)
            mc_pre[l].reset(new Colouring(colour_device(*S.ctx, comm, M, S.opt.seed + (uint64_t)l, im)));
    }
    // a level operator's hybrid-GS structures: l1 diagonals, slabs, templates,
    // the split sweep's old-value pass (built by ensure_gs_blocks), level 0's sliced ELL
    void gs_build(DevMatrix& Al, int l) {
        const amg_options& opt = S.opt;
        if (mcgs) {  // the format of the level's colouring (the coarsest level's goes unused)
            if (mc_pre[l]) Al.build_mc_gs(std::move(*mc_pre[l]), opt.seed + (uint64_t)l);
            mc_pre[l].reset();
            return;
        }
        Al.ensure_gs_blocks(opt.gs_block);
        // level 0's norm-carrying forward sweep runs the one-kernel form, inside captured
        // cycles: its sliced ELL is built now even where the other sweeps run split
        if (l == 0) Al.ensure_gs_ell();
        // a forward split sweep on x != 0: level 0's (tol > 0 solves), a second pre-sweep
        if (Al.gs.split.on && (l == 0 || opt.pre_sweeps >= 2)) Al.ensure_gs_pass(0);
    }

    // which operators of level l the cycle runs as cycle-order copies: A_l, and P_l with R_l
    // (they touch level l + 1 too)
    struct Copies {
        bool a, pr;
    };
    Copies cycle_copies(size_t l) const { return {l > 0 && co.any(l), co.any(l) || co.any(l + 1)}; }
    // segs (P_0 only): the operator's rows stay in the hierarchy's order for its callers, and the
    // formats store them by CycleOrder::p0_segments (DevMatrix::row_seg)
    std::unique_ptr<DevMatrix> copy(const HostCSR& M, const std::vector<int64_t>& rows,
                                    const std::vector<int64_t>& cols, int seg_len = 0, std::vector<int> segs = {}) {
        std::unique_ptr<DevMatrix> d(new DevMatrix());
        d->blocks_only = true;  // row templates assume ascending offsets
        if (!segs.empty()) {
            d->row_seg = seg_len;
            d->seg_rows = std::move(segs);
        }
        // what this rank sends of its column level: positions in that level's order
        d->send_map = cols.empty() ? nullptr : &cols;
        d->build(S.ctx, permuted_csr(M, comm.rank, rows, cols));
        d->send_map = nullptr;
        return d;
    }
    // the cycle-order copies of level l's operators from their hierarchy-order CSRs
    std::unique_ptr<DevMatrix> copy_A(size_t l, const HostCSR& M) { return copy(M, co.perm[l], co.inv[l]); }
    std::unique_ptr<DevMatrix> copy_P(size_t l, const HostCSR& M) {
        return l == 0 ? copy(M, co.perm[l], co.inv[l + 1], co.p0_seg, co.p0_segments())
                      : copy(M, co.perm[l], co.inv[l + 1]);
    }
    std::unique_ptr<DevMatrix> copy_R(size_t l, const HostCSR& M) { return copy(M, co.perm[l + 1], co.inv[l]); }
};

void check_options(const DevMatrix& A, const amg_options& o) {
    AMG_CHECK(A.square, "AMG setup needs a square matrix");
    AMG_CHECK(o.pre_sweeps >= 0 && o.post_sweeps >= 0, "negative sweep count");
    AMG_CHECK(o.max_levels >= 1, "max_levels must be >= 1");
    AMG_CHECK(o.smoother == AMG_SMOOTH_JACOBI || o.smoother == AMG_SMOOTH_HYBRID_GS ||
                  o.smoother == AMG_SMOOTH_CHEBYSHEV || o.smoother == AMG_SMOOTH_MC_GS, "bad smoother");
    if (o.smoother == AMG_SMOOTH_CHEBYSHEV) {  // read only here: other callers may leave them zero
        AMG_CHECK(o.cheby_degree >= 1 && o.cheby_degree <= 16, "cheby_degree must be 1 .. 16");
        AMG_CHECK(o.cheby_fraction > 0.0 && o.cheby_fraction < 1.0, "cheby_fraction must lie in (0, 1)");
    }
}

// build_hierarchy's device steps (setup_device != 0): Galerkin products, and with setup_device
// == 1 the level setup and the transpose
void device_hooks(SolverSetup& st) {
    // the level-0 operator's CSR left on the device by its format build (one rank)
    // (a host-side setup has no use for it: freed here either way)
    if (st.im && st.A.setup_csr) st.images.put(st.A.host, std::move(st.A.setup_csr));
    st.A.setup_csr.reset();
    if (!st.S.opt.setup_device) return;
    st.galerkin = [&st](const HostCSR& X, const HostCSR& Y) { return spgemm_device(*st.S.ctx, st.comm, X, Y); };
    st.rap_fn = [&st](const HostCSR& R, const HostCSR& Am, const HostCSR& P) {
        HostCSR Ac = galerkin_device(*st.S.ctx, st.comm, R, Am, P, st.im);
        // the drop tolerance before keep_only: the Galerkin product's device image goes
        // (images are keyed by the host arrays' address)
        if (st.S.opt.drop_tol > 0.0) Ac = sparsify_device(*st.S.ctx, st.comm, Ac, st.S.opt.drop_tol, st.im);
        if (st.im) st.im->keep_only(Ac);
        return Ac;
    };
    // setup_device == 1: the whole level setup on the GPU where it applies;
    // 2: Galerkin products only (the round-1 split, for A/B and tests)
    if (st.S.opt.setup_device != 1) return;
    st.level_fn = [&st](int l, const HostCSR& A, HostCSR& P, std::vector<int32_t>& split) {
        Solver& S = st.S;
        int64_t stats[2] = {0, 0};
        const bool dev = level_setup_device(*S.ctx, st.comm, A, S.opt, l, P, split, st.im, stats);
        if (S.level_on_device.size() <= (size_t)l) {
            S.level_on_device.resize((size_t)l + 1, 0);
            S.level_ext_stats.resize((size_t)l + 1, {0, 0});
        }
        S.level_on_device[l] = dev ? 1 : 0;
        S.level_ext_stats[l] = {stats[0], stats[1]};
        return dev;
    };
    st.transpose_fn = [&st](const HostCSR& P, HostCSR& R) { return transpose_device(*st.S.ctx, st.comm, P, R, st.im); };
}

// the three workers of an overlapped setup; level 0's colouring and GS structures start now
void start_workers(SolverSetup& st) {
    const int device = st.S.ctx->device;
    st.worker.reset(new FormatWorker(device));
    st.worker2.reset(new FormatWorker(device));
    if (!st.hgs && !st.mcgs) return;
    st.gs_worker.reset(new FormatWorker(device));
    st.mc_colour(0, st.A.host);
    st.gs_worker->push([&st] { st.gs_build(st.A, 0); });
}

// a worker job: M's hierarchy-order formats into slot; gs_level >= 0: its GS structures follow
// on the GS worker
std::function<void()> view_job(SolverSetup& st, std::unique_ptr<DevMatrix>& slot, const HostCSR& M, int gs_level) {
    return [&st, &slot, &M, gs_level] {
        std::unique_ptr<DevMatrix> d(new DevMatrix());
        d->build_view(st.S.ctx, M);
        if (gs_level >= 0 && st.gs_worker) {
            DevMatrix* dm = d.get();
            dm->host_view = &M;
            st.gs_worker->push([&st, dm, gs_level] { st.gs_build(*dm, gs_level); });
        }
        slot = std::move(d);
    };
}

// Overlapped setups, once build_hierarchy reports level l done: level l + 1's brick order and
// colouring, and the worker jobs of A_{l+1}, P_l and R_l
void level_done(SolverSetup& st, int l) {
    // A_{l+1} first: its GS structures start on the second worker while P_l and
    // R_l are built
    // (r5: P_l and R_l on a second format worker beside A_{l+1})
    st.co.next((size_t)l, st.H.levels[l].R, st.S.opt, st.comm);
    const size_t a = (size_t)l + 1, p = (size_t)l;
    st.mc_colour(a, st.H.levels[a].A);
    const HostCSR *Ah = &st.H.levels[a].A, *Ph = &st.H.levels[p].P, *Rh = &st.H.levels[p].R;
    if (st.cycle_copies(a).a) st.worker->push([&st, a, Ah] { st.preAc[a] = st.copy_A(a, *Ah); });
    else st.worker->push(view_job(st, st.preA[a], *Ah, (int)a));
    if (st.cycle_copies(p).pr) {
        st.worker2->push([&st, p, Ph] { st.prePc[p] = st.copy_P(p, *Ph); });
        st.worker2->push([&st, p, Rh] { st.preRc[p] = st.copy_R(p, *Rh); });
    } else {
        st.worker2->push(view_job(st, st.preP[p], *Ph, -1));
        st.worker2->push(view_job(st, st.preR[p], *Rh, -1));
    }
}

void hierarchy(SolverSetup& st) {
    RoctxRange r("setup: hierarchy (strength, split / aggregates, P, R, Galerkin)");
    LevelDoneFn done = nullptr;
    if (st.overlap) {
        start_workers(st);
        done = [&st](int l) { level_done(st, l); };
    }
    build_hierarchy(st.comm, st.A.host, st.S.opt, st.H, st.galerkin, st.level_fn, st.transpose_fn, done, st.rap_fn);
    st.images.e.clear();
    st.tm.lap("hierarchy (host + SpGEMM)");
    if (st.worker) st.worker->finish();  // before gs_worker: its jobs push GS jobs
    if (st.worker2) st.worker2->finish();
    if (st.gs_worker) st.gs_worker->finish();
    if (st.overlap) st.tm.lap("format builds still running after the hierarchy");
}

// the DevMatrix of one hierarchy operator: the worker's pre-built one, else built here (a
// replicated level from the gathered operator; deferred where the cycle runs its copy)
std::unique_ptr<DevMatrix> adopt(SolverSetup& st, HostCSR& M, std::unique_ptr<DevMatrix>& pre, bool rep, bool defer) {
    std::unique_ptr<DevMatrix> d(std::move(pre));
    if (d) {
        d->host = std::move(M);  // built from M on the worker
        d->host_view = nullptr;
        return d;
    }
    d.reset(new DevMatrix());
    if (rep) d->build(st.S.ctx, gather_global(st.comm, M), true);
    else if (defer) d->defer(st.S.ctx, std::move(M));  // the cycle runs its copy
    else d->build(st.S.ctx, std::move(M));
    return d;
}

// the hierarchy's levels into Solver::levels
void adopt_levels(SolverSetup& st) {
    Solver& S = st.S;
    const HostComm& comm = st.comm;
    HostHierarchy& H = st.H;
    // replicated coarse levels (multi-rank): from the first level with <= replicate_below
    // global rows on, every rank holds the whole operators and cycles them locally
    S.rep_level = -1;
    if (comm.nranks > 1 && S.opt.replicate_below > 0)
        for (size_t l = 1; l < H.levels.size(); ++l)
            if (H.A(l).n_global_rows <= S.opt.replicate_below) {
                S.rep_level = (int)l;
                break;
            }
    if (!st.overlap)  // the brick orders (overlapped setups fixed them level by level)
        for (size_t l = 0; l + 1 < H.levels.size(); ++l) st.co.next(l, H.levels[l].R, S.opt, comm);
    S.levels.clear();
    S.levels.resize(H.levels.size());
    for (size_t l = 0; l < H.levels.size(); ++l) {
        HostLevel& hl = H.levels[l];
        Level& L = S.levels[l];
        const bool rep = S.rep_level >= 0 && (int)l >= S.rep_level;
        const SolverSetup::Copies cc = st.cycle_copies(l);
        if (l > 0) L.A = adopt(st, hl.A, st.preA[l], rep, cc.a);
        if (!st.overlap) st.tm.lap("L" + std::to_string(l) + " device A build");
        if (l + 1 == H.levels.size()) continue;
        L.split = std::move(hl.split);
        if (rep) {  // a replicated level is whole on every rank: so is its splitting
            const std::vector<std::vector<int32_t>> all =
                comm.exchange(std::vector<std::vector<int32_t>>(comm.nranks, L.split));
            L.split.clear();
            for (const auto& v : all) L.split.insert(L.split.end(), v.begin(), v.end());
        }
        L.P = adopt(st, hl.P, st.preP[l], rep, cc.pr);
        L.R = adopt(st, hl.R, st.preR[l], rep, cc.pr);
        if (!st.overlap) st.tm.lap("L" + std::to_string(l) + " device P/R build");
    }
}

// cycle-order copies (built on the workers where the setup overlaps, here otherwise)
void cycle_order_copies(SolverSetup& st) {
    std::vector<Level>& levels = st.S.levels;
    if (st.co.any(levels.size() - 1)) {
        // the coarsening stalled on a permuted level, which became the (dense-solved) coarsest:
        // the cycle runs the hierarchy's order
        for (auto& L : levels)
            for (DevMatrix* m : {L.A.get(), L.P.get(), L.R.get()})
                if (m) m->ensure_built();
        return;
    }
    for (size_t l = 0; l < levels.size(); ++l) {
        Level& L = levels[l];
        const SolverSetup::Copies cc = st.cycle_copies(l);
        if (cc.a) L.Ac = st.preAc[l] ? std::move(st.preAc[l]) : st.copy_A(l, L.A->host);
        if (l + 1 < levels.size() && cc.pr) {
            L.Pc = st.prePc[l] ? std::move(st.prePc[l]) : st.copy_P(l, L.P->host);
            L.Rc = st.preRc[l] ? std::move(st.preRc[l]) : st.copy_R(l, L.R->host);
        }
    }
    if (!st.overlap) st.tm.lap("cycle-order copies");
}

// transition to the replicated levels: distributed R output -> whole vector on every rank
void replicated_transition(SolverSetup& st) {
    Solver& S = st.S;
    if (S.rep_level <= 0) return;
    const int nranks = st.comm.nranks;
    S.rep_starts = S.levels[S.rep_level - 1].R->host.row_starts;
    S.rep_cmax = 0;
    for (int r = 0; r < nranks; ++r) S.rep_cmax = std::max(S.rep_cmax, S.rep_starts[r + 1] - S.rep_starts[r]);
    S.rep_pad.alloc((size_t)S.rep_cmax * (nranks + 1));
    HIP_CHECK(hipMemset(S.rep_pad.p, 0, S.rep_pad.n * sizeof(double)));
}

// per-level work vectors and (hybrid GS) the levels' GS structures; returns the largest number
// of norm partials any level's kernels leave
size_t work_vectors_and_gs(SolverSetup& st) {
    Solver& S = st.S;
    size_t max_blocks = 0;
    for (size_t l = 0; l < S.levels.size(); ++l) {
        Level& L = S.levels[l];
        DevMatrix& Al = S.Amat(l);
        const size_t n = (size_t)Al.n_rows;
        if (l > 0) {
            L.x.alloc(n);
            L.b.alloc(n);
        }
        L.r.alloc(n);
        L.t.alloc(n);
        max_blocks = std::max({max_blocks, (size_t)Al.norm_parts_max(), (size_t)S.CA(l).norm_parts_max()});
        if (st.hgs) {
            st.gs_build(Al, (int)l);  // done on the GS worker already where the setup overlaps
            st.tm.lap("L" + std::to_string(l) + " GS structures");
            max_blocks = std::max(max_blocks, (size_t)Al.gs.norm_parts());
        }
    }
    return max_blocks;
}

// norm plumbing: partials | reduction scratch | gathered rank sums
void norm_plumbing(SolverSetup& st, size_t max_blocks) {
    Solver& S = st.S;
    const size_t tmpn = max_blocks / 4096 + 64;
    S.norm_scratch.alloc(max_blocks + tmpn + (size_t)st.comm.nranks + 8);
    S.sink.partial = S.norm_scratch.p;
    S.sink.tmp = S.sink.partial + max_blocks;
    S.sink.gathered = S.sink.tmp + tmpn;
    S.hist_counter.alloc(1);
    S.sink.counter = S.hist_counter.p;
    S.norm_done.alloc(1);
    HIP_CHECK(hipMemset(S.norm_done.p, 0, sizeof(unsigned)));
    S.sink.done = S.norm_done.p;
    S.ensure_hist(1024);
}

// coarsest level: this rank's rows of the gathered dense inverse, row-major (one
// wavefront per row reads its row coalesced).  With several ranks b is
// allgathered into a padded [nranks x cmax] layout and unpadded into the global order
// before the solve (the lanes' interleaving is defined on the global index j).
void coarse_inverse(SolverSetup& st) {
    Solver& S = st.S;
    const HostComm& comm = st.comm;
    DevMatrix& Ac = S.Amat(S.levels.size() - 1);
    S.coarse_n = Ac.host.n_global_rows;
    const int64_t nl = Ac.n_rows, f = Ac.first_row;
    const bool serial_coarse = comm.nranks == 1 || Ac.replicated;
    const int nparts = serial_coarse ? 1 : comm.nranks;
    int64_t cmax = 0;
    S.coarse_starts.assign(Ac.host.row_starts.begin(), Ac.host.row_starts.end());
    for (int r = 0; r < nparts; ++r) cmax = std::max(cmax, Ac.host.row_starts[r + 1] - Ac.host.row_starts[r]);
    S.invT.upload(st.H.coarse_inv.data() + (size_t)(f * S.coarse_n), (size_t)std::max<int64_t>(nl * S.coarse_n, 0));
    if (nl * S.coarse_n == 0) S.invT.alloc(1);
    st.tm.lap("coarse inverse upload");
    S.coarse_counts.assign(1, (int)cmax);
    if (serial_coarse) return;
    // gathered (nranks x cmax) + local padded send slot + the unpadded global vector
    S.bfull.alloc((size_t)cmax * comm.nranks + (size_t)cmax + (size_t)S.coarse_n);
    HIP_CHECK(hipMemset(S.bfull.p, 0, S.bfull.n * sizeof(double)));
}
}  // namespace

void Solver::setup(DevMatrix& A, const amg_options& o) {
    RoctxRange range("ParMultilevel::setup");
    check_options(A, o);
    ctx = A.ctx;
    opt = o;
    A0 = &A;
    level_on_device.clear();
    level_ext_stats.clear();
    SolverSetup st(*this, A);
    device_hooks(st);
    st.co.init(A, opt, st.comm, st.maxl);
    hierarchy(st);
    RoctxRange rbuild("setup: device level formats");
    adopt_levels(st);
    cycle_order_copies(st);
    replicated_transition(st);
    norm_plumbing(st, work_vectors_and_gs(st));
    coarse_inverse(st);
    // multi-rank cycles: loopback ranks meet at host barriers, which a graph cannot replay;
    // RCCL ranks capture whole cycles where the runtime is the one capture was validated on
    use_graph = st.comm.nranks == 1 || (ctx->transport == TR_RCCL && rccl_graph_allowed());
    cheby.clear();
    if (opt.smoother == AMG_SMOOTH_CHEBYSHEV) {
        setup_cheby();
        st.tm.lap("Chebyshev eigenvalue estimates");
    }
    if (st.mcgs) {
        setup_mc_gs();
        st.tm.lap("multicolour GS colourings and formats");
    }
}

// Every smoothed level that the overlapped setup has not coloured already: the colouring of
// seed + l (collective on a distributed level; a replicated level is whole on every rank and
// coloured as one rank's) and its format
void Solver::setup_mc_gs() {
    static const HostComm serial;
    for (size_t l = 0; l + 1 < levels.size(); ++l) {
        DevMatrix& A = Amat(l);
        A.ensure_built();
        // (level 0 is the caller's matrix: a colouring of another seed is replaced)
        if (A.mc.built && A.mc.seed == opt.seed + (uint64_t)l) continue;
        A.build_mc_gs(colour_device(*ctx, A.replicated ? serial : ctx->host, A.host_image(), opt.seed + (uint64_t)l),
                      opt.seed + (uint64_t)l);
    }
}

namespace {
constexpr int kChebyEigIters = 10;  // power steps of lambda_l (SA's rho: DESIGN.md 3)

// y_i = (A x)_i / a_ii (the division by the diagonal itself) and max |y_i|
__global__ __launch_bounds__(kTPB) void eig_div_max_kernel(int n, const double* d, double* y, unsigned long long* m) {
    const int i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= n) return;
    const double v = y[i] / d[i];
    y[i] = v;
    dmax_abs(m, v);
}
}  // namespace

// lambda_l = rho(D^-1 A_l) of every level but the coarsest by the power iteration DESIGN.md 3
// defines for SA's rho (power_iteration, setup_device.hip), on A_l itself: the seeded vector of
// the global ids (seed + l), kChebyEigIters times y = (A x) / a_ii.  Then the coefficients, on the
// host in the order the definition writes them.
void Solver::setup_cheby() {
    const HostComm& comm = ctx->host;
    hipStream_t s = ctx->stream;
    cheby.assign(levels.size(), Cheby{});
    for (size_t l = 0; l + 1 < levels.size(); ++l) {
        DevMatrix& A = Amat(l);
        A.ensure_built();
        const int n = (int)A.n_rows;
        const int g = (n + kTPB - 1) / kTPB;
        const bool dist = comm.nranks > 1 && !A.replicated;  // a replicated level is whole here
        // a_ii of the local rows from the host image (global column ids)
        const HostCSR& H = A.host_image();
        std::vector<double> dh((size_t)std::max(n, 1), 0.0);
#pragma omp parallel for schedule(static)
        for (int i = 0; i < n; ++i)
            for (int64_t k = H.rp[i]; k < H.rp[i + 1]; ++k)
                if (H.col[k] == A.first_row + i) dh[i] = H.val[k];
        DevBuf<double> d;
        d.upload(dh.data(), dh.size());
        double* x = levels[l].r.p;  // the level's work vectors: free until the first cycle
        double* y = levels[l].t.p;
        auto step = [&](unsigned long long* mx) {  // y = (A x) / a_ii, max |y_i| into mx
            par_apply(A, KM_SPMV, x, nullptr, y, 0.0, nullptr);
            if (n) hipLaunchKernelGGL(eig_div_max_kernel, dim3(g), dim3(kTPB), 0, s, n, d.p, y, mx);
        };
        const double lam =
            power_iteration(s, comm, dist, n, A.first_row, opt.seed + (uint64_t)l, kChebyEigIters, x, y, step);
        HIP_CHECK(hipStreamSynchronize(s));  // d is freed here
        Cheby& c = cheby[l];
        const int m = opt.cheby_degree;
        c.lambda = lam;
        c.c1.assign((size_t)m, 0.0);
        c.c2.assign((size_t)m, 0.0);
        if (lam == 0.0) continue;  // every coefficient 0.0
        const double hi = 1.1 * lam;
        const double lo = opt.cheby_fraction * hi;
        const double theta = 0.5 * (hi + lo);
        const double delta = 0.5 * (hi - lo);
        const double sigma = theta / delta;
        c.w0 = 1.0 / theta;
        double rho = 1.0 / sigma;
        for (int k = 1; k < m; ++k) {
            const double rk = 1.0 / (2.0 * sigma - rho);
            c.c1[k] = rk * rho;
            c.c2[k] = (2.0 * rk) / delta;
            rho = rk;
        }
    }
}

// Whole-cycle capture with RCCL groups inside: on HIP 7.0.51831 + RCCL 2.26.6
// (the copies torch bundles, which a torch-first process binds) hipStreamEndCapture segfaults;
// on ROCm 7.2's HIP 7.2.26015 + RCCL 2.27.7 (torch-free callers) captured cycles replay
// bit-exact.  AMG_RCCL_GRAPH=0 / 1 overrides the version check either way.
bool Solver::rccl_graph_allowed(std::string* why) {
    static const int forced = [] {
        const char* e = std::getenv("AMG_RCCL_GRAPH");
        return e && *e ? (std::atoi(e) != 0 ? 1 : 0) : -1;
    }();
    int hv = 0, nv = 0;
    (void)hipRuntimeGetVersion(&hv);
    (void)ncclGetVersion(&nv);
    const bool ok = forced >= 0 ? forced == 1 : hv >= 70200000 && nv >= 22707;
    if (!ok && why)
        *why = "multi-rank hipGraph capture of RCCL cycles is validated on HIP >= 7.2 with RCCL >= "
               "2.27.7; this process runs HIP " + std::to_string(hv) + " with RCCL " +
               std::to_string(nv) + (forced == 0 ? " (AMG_RCCL_GRAPH=0)" : " (AMG_RCCL_GRAPH=1 overrides)");
    return ok;
}

}  // namespace amg
