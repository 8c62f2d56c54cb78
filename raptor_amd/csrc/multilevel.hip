// multilevel.hip -- ParMultilevel on the GPU: the V-cycle, its captured graphs and timeline, and
// the solve / PCG / BiCGStab drivers (the setup half: solver_setup.hip).  SURVEY.md 8a rows
// a6-a10.  The cycle mirrors oracle/amg_oracle.c cycle_rec() operation for operation, so the
// iterates are bit-identical to the oracle's.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "device.hpp"

namespace amg {

Solver::~Solver() {
    for (auto& g : graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    for (hipEvent_t e : tl_ev) (void)hipEventDestroy(e);
}

void Solver::ensure_hist(int32_t n) {
    if (hist.n >= (size_t)n) return;
    hist.alloc((size_t)n);
    sink.hist = hist.p;
    destroy_graphs();  // captured graphs baked the old pointer (collective: every rank's solve
                       // sizes the history from the same max_iter)
}

// In place: forward before the coarse correction, backward after it.  From zero the sweep runs
// as it is on a zeroed x (no shortcut: the bits of the definition)
void Solver::smooth_mc_gs(size_t l, double* x, const double* b, const Sweep& w) {
    DevMatrix& A = CA(l);
    AMG_ASSERT(!w.with_norm && !w.x0_in_t);
    if (w.from_zero) launch_zero(ctx->stream, A.n_rows, x);
    par_mc_gs(A, x, b, w.post, 0);
    mark(l, w.post ? "post-smooth mc sweep" : w.from_zero ? "pre-smooth mc sweep from 0" : "pre-smooth mc sweep");
}

// One application of the degree-m polynomial: step 0 is a Jacobi step with omega = w0 on
// Jacobi's paths; step k >= 1 writes x_{k+1} over x_{k-1} (y aliases xprev), so the two
// buffers keep alternating.  After a step 0 from zero x_{k-1} is zeros: no operand
void Solver::smooth_cheby(size_t l, double*& x, const double* b, double*& tmp, const Sweep& w) {
    DevMatrix& A = CA(l);
    const Cheby& c = cheby[l];
    if (w.x0_in_t) {  // step 0 fused into the restriction above (par_restrict_j0)
        AMG_ASSERT(w.from_zero && !w.with_norm);
    } else if (w.with_norm) {
        AMG_ASSERT(!w.from_zero);
        par_apply(A, KM_JACOBI, x, b, tmp, c.w0, sink.partial);
        norm_finish(A, sink);
    } else if (w.from_zero) {
        launch_jacobi_zero(ctx->stream, A.n_rows, b, A.dinv.p, tmp, c.w0);
    } else {
        par_apply(A, KM_JACOBI, x, b, tmp, c.w0, nullptr);
    }
    std::swap(x, tmp);
    if (!w.x0_in_t)
        mark(l, w.post ? "post-smooth step 0" : w.with_norm ? "pre-smooth step 0 + norm"
                                            : w.from_zero ? "pre-smooth step 0 from 0" : "pre-smooth step 0");
    bool prev_zero = w.from_zero;
    for (int k = 1; k < opt.cheby_degree; ++k) {
        par_apply(A, KM_CHEBY, x, b, tmp, c.c2[k], nullptr, prev_zero ? nullptr : tmp, c.c1[k]);
        std::swap(x, tmp);
        prev_zero = false;
        mark(l, w.post ? "post-smooth step" : "pre-smooth step");
    }
}

static const char* sweep_label(const Solver::Sweep& w) {
    return w.post ? "post-smooth" : w.with_norm ? "pre-smooth + norm" : w.from_zero ? "pre-smooth from 0" : "pre-smooth";
}

// Hybrid GS sweeps forward before the coarse correction and backward after it (post):
// the V-cycle is then a symmetric operator, as CG requires (oracle smooth()).
void Solver::smooth_hybrid_gs(size_t l, double*& x, const double* b, double*& tmp, const Sweep& w) {
    DevMatrix& A = CA(l);
    AMG_ASSERT(!w.x0_in_t);
    if (w.with_norm) {  // forward GS sweep that also leaves the partials of ||b - A x|| (old x)
        AMG_ASSERT(!w.from_zero && !w.post);
        par_hybrid_gs(A, x, b, tmp, opt.gs_block, false, sink.partial);
        norm_finish(A, sink, A.gs.norm_parts());
    } else {
        if (w.from_zero) launch_zero(ctx->stream, A.n_rows, x);
        if (w.from_zero && !w.post) par_hybrid_gs_from_zero(A, x, b, tmp, opt.gs_block);
        else par_hybrid_gs(A, x, b, tmp, opt.gs_block, w.post);
    }
    std::swap(x, tmp);
    mark(l, sweep_label(w));
}

void Solver::smooth_jacobi(size_t l, double*& x, const double* b, double*& tmp, const Sweep& w) {
    DevMatrix& A = CA(l);
    if (w.x0_in_t) return std::swap(x, tmp);  // the sweep from zero is in tmp already (par_restrict_j0)
    if (w.with_norm) {  // Jacobi sweep that also leaves the partials of ||b - A x||
        AMG_ASSERT(opt.smoother == AMG_SMOOTH_JACOBI && !w.from_zero);
        par_apply(A, KM_JACOBI, x, b, tmp, opt.jacobi_omega, sink.partial);
        norm_finish(A, sink);
    } else if (w.from_zero) {
        launch_jacobi_zero(ctx->stream, A.n_rows, b, A.dinv.p, tmp, opt.jacobi_omega);
    } else {
        par_apply(A, KM_JACOBI, x, b, tmp, opt.jacobi_omega, nullptr);
    }
    std::swap(x, tmp);
    mark(l, sweep_label(w));
}

void Solver::smooth(size_t l, double*& x, const double* b, double*& tmp, const Sweep& w) {
    switch (opt.smoother) {
        case AMG_SMOOTH_JACOBI: return smooth_jacobi(l, x, b, tmp, w);
        case AMG_SMOOTH_CHEBYSHEV: return smooth_cheby(l, x, b, tmp, w);
        case AMG_SMOOTH_HYBRID_GS: return smooth_hybrid_gs(l, x, b, tmp, w);
        case AMG_SMOOTH_MC_GS: return smooth_mc_gs(l, x, b, w);
    }
    AMG_ASSERT(false);
}

// Timeline marks (amg_solver_cycle_timeline).  tl_mode 2, inside the timeline's capture: an
// event-record node is added behind the capture's current tail and becomes the new tail, so one
// graph of the whole cycle timestamps every operation as it replays (HIP captures a plain
// event record only as a dependency marker).  tl_mode 1, inside the capture: the capture is
// closed there and reopened (one graph per operation, replayed back to back with timing events
// between them; each time then includes a graph launch).  Eager: a timing event.
static void ensure_events(std::vector<hipEvent_t>& ev, size_t n) {
    while (ev.size() < n) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));  // timing enabled
        ev.push_back(e);
    }
}

void Solver::mark(size_t l, const char* what) {
    if (!tl_on) return;
    hipStream_t s = ctx->stream;
    const std::string label = "L" + std::to_string(l) + " " + what;
    if (ctx->capturing && tl_mode == 1) {
        hipGraph_t g = nullptr;
        HIP_CHECK(hipStreamEndCapture(s, &g));
        tl_graphs.push_back(g);
        tl_label.push_back(label);
        HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        return;
    }
    ensure_events(tl_ev, tl_n + 1);
    if (tl_label.size() <= tl_n) tl_label.resize(tl_n + 1);
    tl_label[tl_n] = label;
    if (ctx->capturing) {  // tl_mode 2
        hipStreamCaptureStatus st;
        hipGraph_t g = nullptr;
        const hipGraphNode_t* deps = nullptr;
        size_t nd = 0;
        HIP_CHECK(hipStreamGetCaptureInfo_v2(s, &st, nullptr, &g, &deps, &nd));
        hipGraphNode_t en;
        HIP_CHECK(hipGraphAddEventRecordNode(&en, g, deps, nd, tl_ev[tl_n]));
        HIP_CHECK(hipStreamUpdateCaptureDependencies(s, &en, 1, hipStreamSetCaptureDependencies));
    } else {
        HIP_CHECK(hipEventRecord(tl_ev[tl_n], s));
    }
    ++tl_n;
}

int Solver::cycle_timeline(double* x, const double* b, int reps, std::vector<std::string>& labels,
                           std::vector<double>& us) {
    AMG_CHECK(ctx->host.nranks == 1, "cycle timeline: one rank");
    AMG_CHECK(reps >= 1, "cycle timeline: reps must be >= 1");
    hipStream_t s = ctx->stream;
    std::vector<hipGraphExec_t> execs;
    std::vector<std::string> seg_label;
    auto capture_marked = [&](int m, const std::function<void()>& body) {  // marks on, in mode m
        tl_mode = m;
        tl_graphs.clear();
        tl_label.clear();
        tl_n = 0;
        tl_on = true;
        const Captured c = capture(body);
        tl_on = false;
        return c;
    };
    // capture the cycle with marks in mode m; the instantiated graphs (one, or one per
    // operation) and their labels; false where the runtime refuses
    auto capture_cycle = [&](int m) {
        const Captured c = capture_marked(m, [&] {
            if (m == 2) mark(0, "begin");
            cycle_rec(0, x, b, false, false);
        });
        (void)hipGetLastError();
        bool ok = c.err.empty() && c.end == hipSuccess;
        if (m == 2) {
            if (c.graph) tl_graphs.push_back(c.graph);
            seg_label.assign(tl_label.begin() + (tl_n > 0 ? 1 : 0), tl_label.begin() + tl_n);
        } else {
            if (c.graph) (void)hipGraphDestroy(c.graph);  // after the last mark: nothing
            seg_label = tl_label;
        }
        for (hipGraph_t g : tl_graphs) {
            hipGraphExec_t e = nullptr;
            if (ok && hipGraphInstantiate(&e, g, nullptr, nullptr, 0) == hipSuccess) execs.push_back(e);
            else ok = false;
            (void)hipGraphDestroy(g);
        }
        tl_graphs.clear();
        (void)hipGetLastError();
        if (!ok) {
            for (hipGraphExec_t e : execs) (void)hipGraphExecDestroy(e);
            execs.clear();
        }
        return ok;
    };
    // one replay: a vector of event-to-event times (ms), empty where the runtime did not time them
    auto replay = [&](int m) {
        std::vector<float> t;
        size_t n = 0;
        if (m == 2) {
            HIP_CHECK(hipGraphLaunch(execs[0], s));
            n = tl_n;
        } else if (m == 1) {
            ensure_events(tl_ev, execs.size() + 1);
            HIP_CHECK(hipEventRecord(tl_ev[0], s));
            for (size_t k = 0; k < execs.size(); ++k) {
                HIP_CHECK(hipGraphLaunch(execs[k], s));
                HIP_CHECK(hipEventRecord(tl_ev[k + 1], s));
            }
            n = execs.size() + 1;
        } else {
            tl_mode = 0;
            tl_on = true;
            tl_n = 0;
            try {
                mark(0, "begin");
                cycle_rec(0, x, b, false, false);
            } catch (...) {
                tl_on = false;
                throw;
            }
            tl_on = false;
            n = tl_n;
            seg_label.assign(tl_label.begin() + 1, tl_label.begin() + (n > 0 ? n : 1));
        }
        HIP_CHECK(hipStreamSynchronize(s));
        for (size_t k = 1; k < n; ++k) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, tl_ev[k - 1], tl_ev[k]) != hipSuccess) {
                (void)hipGetLastError();
                return std::vector<float>();
            }
            t.push_back(ms);
        }
        return t;
    };
    int mode = 0;
    std::vector<std::vector<float>> t;
    for (int m = use_graph ? 2 : 0; m >= 0 && mode == 0; --m) {
        if (m > 0 && !capture_cycle(m)) continue;
        std::vector<float> first = replay(m);
        if (first.empty() && m > 0) {  // not timed: the next mode
            for (hipGraphExec_t e : execs) (void)hipGraphExecDestroy(e);
            execs.clear();
            continue;
        }
        mode = m > 0 ? m : -1;
        t.assign(first.size(), {});
        for (size_t k = 0; k < first.size(); ++k) t[k].push_back(first[k]);
        for (int r = 1; r < reps; ++r) {
            const std::vector<float> v = replay(m);
            for (size_t k = 0; k < v.size() && k < t.size(); ++k) t[k].push_back(v[k]);
        }
    }
    for (hipGraphExec_t e : execs) HIP_CHECK(hipGraphExecDestroy(e));
    execs.clear();
    labels = seg_label;
    labels.resize(t.size());
    if (mode == 2) {
        // calibration: two event-record nodes with nothing between them -- the time a node adds
        // to the operation before it (reported as a last pseudo-operation "event-node gap")
        const Captured c = capture_marked(2, [&] {
            mark(0, "gap a");
            mark(0, "gap b");
        });
        hipGraphExec_t e = nullptr;
        if (c.err.empty() && c.end == hipSuccess && c.graph &&
            hipGraphInstantiate(&e, c.graph, nullptr, nullptr, 0) == hipSuccess) {
            std::vector<float> gv;
            for (int r = 0; r < reps; ++r) {
                HIP_CHECK(hipGraphLaunch(e, s));
                HIP_CHECK(hipStreamSynchronize(s));
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, tl_ev[0], tl_ev[1]) == hipSuccess) gv.push_back(ms);
            }
            if (!gv.empty()) {
                labels.push_back("event-node gap");
                t.push_back(gv);
            }
            HIP_CHECK(hipGraphExecDestroy(e));
        }
        if (c.graph) (void)hipGraphDestroy(c.graph);
        (void)hipGetLastError();
    }
    tl_mode = 0;
    us.clear();
    for (auto& v : t) {
        std::sort(v.begin(), v.end());
        us.push_back(1e3 * (double)v[v.size() / 2]);
    }
    return mode > 0 ? mode : 0;
}

void Solver::allgather_unpad(const double* slot, double* pad, int64_t cmax, const std::vector<int64_t>& starts,
                             double* dst) {
    ctx->allgather(slot, pad, (size_t)cmax);
    for (int q = 0; q < ctx->host.nranks; ++q) {
        const int64_t c = starts[q + 1] - starts[q];
        if (c)
            HIP_CHECK(hipMemcpyAsync(dst + starts[q], pad + q * cmax, c * sizeof(double), hipMemcpyDeviceToDevice,
                                     ctx->stream));
    }
}

void Solver::cycle_rec(size_t l, double* x, const double* b, bool x_zero, bool with_norm, bool x0_in_t) {
    DevMatrix& A = CA(l);
    hipStream_t s = ctx->stream;
    const HostComm& comm = ctx->host;
    if (l + 1 == levels.size()) {
        const double* bf = b;
        if (comm.nranks > 1 && !A.replicated) {
            const int64_t cmax = coarse_counts[0];
            double* slot = bfull.p + cmax * comm.nranks;
            if (A.n_rows > 0)
                HIP_CHECK(hipMemcpyAsync(slot, b, A.n_rows * sizeof(double), hipMemcpyDeviceToDevice, s));
            double* glob = bfull.p + cmax * (comm.nranks + 1);
            allgather_unpad(slot, bfull.p, cmax, coarse_starts, glob);
            bf = glob;
        }
        launch_dense_gemv(s, A.n_rows, coarse_n, invT.p, bf, x);
        mark(l, "coarse solve");
        return;
    }
    Level& L = levels[l];
    double* cur = x;
    double* tmp = L.t.p;
    bool zero = x_zero;
    for (int k = 0; k < opt.pre_sweeps; ++k) {
        smooth(l, cur, b, tmp, {zero, with_norm && k == 0, false, k == 0 && x0_in_t});
        zero = false;
    }
    if (zero) launch_zero(s, A.n_rows, cur);
    par_apply(A, KM_RESID, cur, b, L.r.p, 0.0, nullptr);
    mark(l, "residual");
    Level& C = levels[l + 1];
    if ((int)l + 1 == rep_level) {
        // distributed R output -> whole b_{l+1} on every rank (padded allgather + unpad)
        double* slot = rep_pad.p + rep_cmax * comm.nranks;
        par_apply(CR(l), KM_SPMV, L.r.p, nullptr, slot, 0.0, nullptr);
        allgather_unpad(slot, rep_pad.p, rep_cmax, rep_starts, C.b.p);
        mark(l, "restrict + allgather");
        cycle_rec(l + 1, C.x.p, C.b.p, true, false);
        // this rank's slice of the whole correction feeds the distributed interpolation
        par_apply(CP(l), KM_SPMV_ADD, C.x.p + L.P->first_col, nullptr, cur, 0.0, nullptr);
    } else {
        // Jacobi: the coarse level's first sweep from x = 0 (omega dinv b) rides along with
        // the restriction that produces b (one pass over b and a launch fewer per level)
        // (Chebyshev: its step 0, omega = the next level's w0)
        const bool j0 = jacobi_like() && opt.pre_sweeps >= 1 && l + 2 < levels.size() &&
                        par_restrict_j0(CR(l), L.r.p, C.b.p, C.t.p, CA(l + 1).dinv.p, omega0(l + 1));
        if (!j0) par_apply(CR(l), KM_SPMV, L.r.p, nullptr, C.b.p, 0.0, nullptr);
        mark(l, j0 ? "restrict + next pre-smooth from 0" : "restrict");
        cycle_rec(l + 1, C.x.p, C.b.p, true, false, j0);
        par_apply(CP(l), KM_SPMV_ADD, C.x.p, nullptr, cur, 0.0, nullptr);
    }
    mark(l, "interp");
    for (int k = 0; k < opt.post_sweeps; ++k) smooth(l, cur, b, tmp, {false, false, true, false});
    if (cur != x) {
        HIP_CHECK(hipMemcpyAsync(x, cur, A.n_rows * sizeof(double), hipMemcpyDeviceToDevice, s));
        mark(l, "copy");
    }
}

bool Solver::can_fuse_norm() const {
    return (jacobi_like() || opt.smoother == AMG_SMOOTH_HYBRID_GS) && opt.pre_sweeps >= 1 && levels.size() >= 2;
}

// An exec is destroyed only once the stream has drained: a replay enqueued without a host
// wait (graph_launch) may still be running, and HIP does not document a deferred free of an
// executing graph the way CUDA does.  Recaptures are rare, so one wait is cheap.
void Solver::drop_graph(Graph& G) {
    if (!G.exec) return;
    if (!ctx->capturing) HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->graph_inflight = false;
    HIP_CHECK(hipGraphExecDestroy(G.exec));
    G.exec = nullptr;
}

void Solver::destroy_graphs() {
    for (auto& g : graphs) drop_graph(g);
}

Solver::Captured Solver::capture(const std::function<void()>& body) {
    Captured c;
    HIP_CHECK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    ctx->capturing = true;
    try {
        body();
    } catch (const Error& e) {
        c.err = e.what();
        c.err_code = e.code;
    } catch (const std::exception& e) {
        c.err = e.what();
    }
    ctx->capturing = false;
    c.end = hipStreamEndCapture(ctx->stream, &c.graph);
    return c;
}

// true where `mine` holds on any rank (host allgather: collective)
static bool any_rank(const HostComm& comm, bool mine) {
    bool any = false;
    for (int64_t v : comm.allgather((int64_t)(mine ? 1 : 0))) any = any || v != 0;
    return any;
}

// Capture `body` (enqueues on ctx->stream, RCCL groups included) into graphs[slot] unless the
// graph for (x, b) and the current formats exists.  Multi-rank, the decision is collective:
//  1. with `agree`, every rank's stale flag goes through the host exchange and all ranks
//     recapture if any must (a caching allocator handing x a new address on one rank only
//     would otherwise leave that rank capturing -- and waiting in the host exchange below --
//     while its peers replay RCCL groups it never joins);
//  2. the capture + instantiate status is exchanged: one rank's failure sends every rank to
//     eager launches (an exception during capture raises on every rank).
bool Solver::graph_ready(int slot, const double* x, const double* b, const std::function<void()>& body,
                         bool agree) {
    Graph& G = graphs[slot];
    const HostComm& comm = ctx->host;
    const bool multi = comm.nranks > 1;
    bool stale = !G.exec || G.x != x || G.b != b || G.fmt_gen != DevMatrix::format_generation;
    if (multi && agree) stale = any_rank(comm, stale);
    if (!stale) return true;
    drop_graph(G);
    static const bool trace = std::getenv("AMG_TRACE_RCCL") != nullptr;
    if (trace) std::fprintf(stderr, "[amg] rank %d capture begin (slot %d)\n", comm.rank, slot);
    RoctxRange r("cycle: hipGraph capture");
    install_crash_handler();
    // a capture starts from an idle stream: RCCL work of earlier replays still in flight
    // stays ordered before the captured groups by the stream, and nothing eager is pending
    if (multi) ctx->eager_rccl_fence();
    Captured c = capture(body);  // c.err_code: the amg::Error code of a failing body, rethrown below
    std::string& err = c.err;
    if (c.end != hipSuccess && err.empty()) err = std::string("hipStreamEndCapture: ") + hipGetErrorString(c.end);
    if (trace) std::fprintf(stderr, "[amg] rank %d capture end\n", comm.rank);
    hipError_t ie = hipErrorUnknown;
    if (err.empty() && c.graph) ie = hipGraphInstantiate(&G.exec, c.graph, nullptr, nullptr, 0);
    if (c.graph) (void)hipGraphDestroy(c.graph);
    if (ie != hipSuccess) {
        (void)hipGetLastError();
        G.exec = nullptr;
    }
    // 1 = ready, 0 = instantiate refused, -1 = the capture itself failed
    const int64_t mine = !err.empty() ? -1 : ie == hipSuccess ? 1 : 0;
    int64_t worst = mine;
    if (multi)
        for (int64_t v : comm.allgather(mine)) worst = std::min(worst, v);
    if (worst == -1) {
        destroy_graphs();
        use_graph = false;
        // the failing rank keeps its own error code (NOMEM, INVALID, ...); its peers report
        // the generic failure
        throw Error(err.empty() ? AMG_ERR_INTERNAL : c.err_code,
                    "V-cycle capture failed" + (err.empty() ? std::string(" on another rank") : ": " + err));
    }
    if (worst == 0) {
        // a graph some rank's runtime cannot instantiate: every rank runs eagerly from now on
        // (identical results; only the launch overhead differs)
        AMG_CHECK(multi, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
        destroy_graphs();
        use_graph = false;
        return false;
    }
    G.x = x;
    G.b = b;
    G.fmt_gen = DevMatrix::format_generation;
    return true;
}

// One collective staleness decision for every graph slot a call will replay (multi-rank): a
// slot stale on any rank is dropped on every rank, so the later graph_ready(.., agree = false)
// calls capture -- and meet in the capture's status exchange -- on all ranks or on none.
// (Deciding per slot inside the loop hung: solve's last-norm graph was stale on the rank whose
// x had moved and fresh on the others, so one rank waited in the status exchange.)
void Solver::agree_stale(std::initializer_list<int> slots, const double* x, const double* b) {
    const HostComm& comm = ctx->host;
    if (!use_graph || comm.nranks <= 1) return;
    bool stale = false;
    for (int slot : slots) {
        const Graph& G = graphs[slot];
        stale = stale || !G.exec || G.x != x || G.b != b || G.fmt_gen != DevMatrix::format_generation;
    }
    if (!any_rank(comm, stale)) return;
    if (ctx->graph_inflight) ctx->eager_rccl_fence();  // replays of the graphs dropped below
    for (int slot : slots) drop_graph(graphs[slot]);
}

void Solver::graph_launch(int slot) {
    RoctxRange r("cycle: hipGraph replay");
    HIP_CHECK(hipGraphLaunch(graphs[slot].exec, ctx->stream));
    static const bool trace = std::getenv("AMG_TRACE_RCCL") != nullptr;
    if (trace) std::fprintf(stderr, "[amg] rank %d graph launched (slot %d)\n", ctx->host.rank, slot);
    // no host wait: the next replay orders behind this one on the stream, and the next eager
    // RCCL enqueue waits once (Context::eager_rccl_fence)
    if (ctx->host.nranks > 1) ctx->graph_inflight = true;
}

void Solver::run(int slot, const double* x, const double* b, const std::function<void()>& body, bool agree,
                 const char* eager_range) {
    if (use_graph && graph_ready(slot, x, b, body, agree)) return graph_launch(slot);
    if (!eager_range) return body();
    RoctxRange r(eager_range);
    body();
}

void Solver::cycle(double* x, const double* b, bool with_norm, bool agree) {
    AMG_ASSERT(!with_norm || can_fuse_norm());
    run(with_norm ? G_CYCLE_NORM : G_CYCLE, x, b, [&] { cycle_rec(0, x, b, false, with_norm); }, agree, "cycle: eager");
}

void Solver::residual_norm(double* x, const double* b, bool agree) {
    // AMG_RCCL_NORM_GRAPH=0: the norm eager after graph-replayed cycles (probe of the eager
    // fence)
    static const bool norm_graph = [] {
        const char* e = std::getenv("AMG_RCCL_NORM_GRAPH");
        return !(e && *e && std::atoi(e) == 0);
    }();
    auto body = [&] { par_residual_norm(*A0, x, b, levels[0].r.p, sink); };
    if (norm_graph || ctx->host.nranks == 1) run(G_NORM, x, b, body, agree);
    else body();
}

void Solver::begin_history(int32_t max_iter) {
    ensure_hist(max_iter + 1);
    if (ctx->host.nranks > 1) ctx->eager_rccl_fence();  // replays of earlier calls
    HIP_CHECK(hipMemsetAsync(hist_counter.p, 0, sizeof(int), ctx->stream));
}

double Solver::read_scalar(const double* dev) {
    double v = 0.0;
    HIP_CHECK(hipMemcpyAsync(&v, dev, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->graph_inflight = false;
    return v;
}

void Solver::download_history(double* hist_host, size_t n) {
    HIP_CHECK(hipMemcpyAsync(hist_host, hist.p, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->graph_inflight = false;
}

bool Solver::grow_work(DevBuf<double>& a, size_t na, DevBuf<double>& b, size_t nb, std::initializer_list<int> slots) {
    const bool ga = a.n < na, gb = b.n < nb;
    if (ga || gb)
        for (int slot : slots) drop_graph(graphs[slot]);  // the captured graphs hold these addresses
    if (ga) a.alloc(na);
    if (gb) b.alloc(nb);
    return gb;
}

int32_t Solver::solve(double* x, const double* b, int32_t max_iter, double tol, double* hist_host) {
    AMG_CHECK(max_iter >= 0, "max_iter must be >= 0");
    RoctxRange range("ParMultilevel::solve");
    begin_history(max_iter);
    int32_t it = 0;
    // one collective graph decision per solve, over every slot it replays (x and b stay put
    // for its cycles)
    if (tol <= 0.0 && can_fuse_norm()) {
        // ||b - A x_k|| comes out of cycle k+1's first Jacobi sweep (same b - Ax values);
        // only the last norm needs its own residual pass.  No host sync in the loop, and with
        // graphs on, no eager work at all: cycles and the last norm replay captured graphs.
        agree_stale({G_CYCLE_NORM, G_NORM}, x, b);
        for (; it < max_iter; ++it) cycle(x, b, true, false);
        residual_norm(x, b, false);
    } else {
        agree_stale({G_CYCLE, G_NORM}, x, b);
        residual_norm(x, b, false);
        const double r0 = tol > 0.0 ? read_scalar(hist.p) : 0.0;
        while (it < max_iter) {
            cycle(x, b, false, false);
            residual_norm(x, b, false);
            ++it;
            if (tol > 0.0) {
                const double rn = read_scalar(hist.p + it);
                if (r0 > 0.0 && rn / r0 < tol) break;
            }
        }
    }
    download_history(hist_host, (size_t)(it + 1));
    return it;
}

// ---- AMG-preconditioned CG ------------------------------------
// Scalars never leave the device (alpha/beta are formed inside the update kernels), so an
// iteration has no host synchronisation unless a tolerance is requested.  Dot products use
// a fixed block span + fixed trees + rank-ordered sums: deterministic for a given partition.
enum { SC_RZ = 0, SC_RZN, SC_PQ, SC_RN, SC_N };

void Solver::dot(const double* a, const double* b, double* dst, bool take_sqrt) {
    DevMatrix& A = *A0;
    const int g = dot_partial_count(A.n_rows);
    double* partial = pcg_scratch.p;
    double* tmp = partial + g;
    double* gathered = tmp + g / 4096 + 64;
    double* local = gathered + ctx->host.nranks;
    launch_dot_partials(ctx->stream, A.n_rows, a, b, partial);
    launch_reduce_partials(ctx->stream, g, partial, tmp, local);
    if (ctx->host.nranks > 1) {
        ctx->allgather(local, gathered, 1);
        launch_finish_sum(ctx->stream, ctx->host.nranks, gathered, dst, take_sqrt);
    } else {
        launch_finish_sum(ctx->stream, 1, local, dst, take_sqrt);
    }
}

// With graphs on, an iteration is two captured graphs: G_PCG_STEP (q = A p, p.q, the x / r
// update, ||r|| appended) and G_PCG_PREC (z = M^-1 r by one V-cycle from z = 0, r.z, the p
// update).  Multi-rank, their RCCL halo groups and dot allgathers replay inside the graphs, so
// nothing eager follows a replay inside the loop and Context::eager_rccl_fence never waits
// there (the eager dot allgathers synchronised the host once per
// iteration).  The set-up (r = b - A x, ||r||, the first z, r.z) runs eagerly, before any
// replay.  tol > 0 waits for the norm each iteration anyway.
int32_t Solver::pcg(double* x, const double* b, int32_t max_iter, double tol, double* hist_host) {
    AMG_CHECK(max_iter >= 0, "max_iter must be >= 0");
    RoctxRange range("ParMultilevel::pcg");
    DevMatrix& A = *A0;
    const int64_t n = A.n_rows;
    hipStream_t s = ctx->stream;
    const int g = dot_partial_count(n);
    const size_t need = (size_t)g + g / 4096 + 64 + ctx->host.nranks + 2 + SC_N;
    grow_work(pcg_vec, (size_t)(4 * n + 4), pcg_scratch, need, {G_PCG_STEP, G_PCG_PREC});
    double* r = pcg_vec.p;
    double* z = r + n;
    double* p = z + n;
    double* q = p + n;
    double* sc = pcg_scratch.p + (need - SC_N);
    begin_history(max_iter);
    auto record_norm = [&] {
        dot(r, r, sc + SC_RN, true);
        launch_append(s, sc + SC_RN, hist.p, hist_counter.p);
    };
    auto step = [&] {  // q = A p; alpha = rz / pq; x += alpha p; r -= alpha q; ||r||
        par_apply(A, KM_SPMV, p, nullptr, q, 0.0, nullptr);
        dot(p, q, sc + SC_PQ, false);
        launch_pcg_xr(s, n, sc + SC_RZ, sc + SC_PQ, p, q, x, r);
        record_norm();
    };
    auto prec = [&] {  // z = M^-1 r (one V-cycle from z = 0); beta = rz_new / rz; p = z + beta p
        launch_zero(s, n, z);
        cycle_rec(0, z, r, false, false);
        dot(r, z, sc + SC_RZN, false);
        launch_pcg_p(s, n, sc + SC_RZN, sc + SC_RZ, z, p);
        HIP_CHECK(hipMemcpyAsync(sc + SC_RZ, sc + SC_RZN, sizeof(double), hipMemcpyDeviceToDevice, s));
    };
    par_apply(A, KM_RESID, x, b, r, 0.0, nullptr);
    record_norm();
    const double r0 = tol > 0.0 ? read_scalar(hist.p) : 0.0;
    launch_zero(s, n, z);
    cycle_rec(0, z, r, false, false);
    if (n) HIP_CHECK(hipMemcpyAsync(p, z, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    dot(r, z, sc + SC_RZ, false);
    // one collective graph decision for both iteration graphs (keyed by the caller's x, b)
    agree_stale({G_PCG_STEP, G_PCG_PREC}, x, b);
    int32_t it = 0;
    while (it < max_iter) {
        run(G_PCG_STEP, x, b, step);
        ++it;
        if (tol > 0.0) {
            const double rn = read_scalar(hist.p + it);
            if (r0 > 0.0 && rn / r0 < tol) break;
        }
        if (it == max_iter) break;
        run(G_PCG_PREC, x, b, prec);
    }
    download_history(hist_host, (size_t)(it + 1));
    return it;
}

// ---- AMG-preconditioned BiCGStab --------------------------------------------
// Right-preconditioned BiCGStab for nonsymmetric operators, M = one V-cycle from zero.  alpha,
// omega, beta, rho, the stop flag and the history counter stay on the device: single-thread
// finishing launches form them after each dot product, and every vector kernel of the iteration
// returns at once when the flag is set, so with tol == 0 the loop never waits for the host and
// the replays after a breakdown change nothing.  With graphs on an iteration is two captured
// graphs, as in pcg: G_BICG_S (phat = M p, v = A phat, rhat.v, alpha, s) and G_BICG_XR (shat =
// M s, t = A shat, t.s and t.t, omega, the x / r update with r.r and rhat.r, beta, p).
int32_t Solver::bicgstab(double* x, const double* b, int32_t max_iter, double tol, double* hist_host,
                         int32_t* status) {
    AMG_CHECK(max_iter >= 0, "max_iter must be >= 0");
    RoctxRange range("ParMultilevel::bicgstab");
    DevMatrix& A = *A0;
    const int64_t n = A.n_rows;
    hipStream_t s = ctx->stream;
    const int nr = ctx->host.nranks;
    const int g = dot_partial_count(n);
    const size_t ntmp = (size_t)g / 4096 + 64;
    const size_t need = 2 * (size_t)g + ntmp + 2 * (size_t)nr + 2 + BS_N;
    // a fresh scratch is zeroed: after a stop the gated kernels leave the partials unwritten
    // and the reductions still read them
    if (grow_work(bicg_vec, (size_t)(8 * n + 8), bicg_scratch, need, {G_BICG_S, G_BICG_XR}))
        HIP_CHECK(hipMemsetAsync(bicg_scratch.p, 0, need * sizeof(double), s));
    double* r = bicg_vec.p;
    double* rhat = r + n;
    double* p = rhat + n;
    double* v = p + n;
    double* sv = v + n;
    double* t = sv + n;
    double* ph = t + n;
    double* sh = ph + n;
    double* part0 = bicg_scratch.p;
    double* part1 = part0 + g;
    double* tmp = part1 + g;
    double* gathered = tmp + ntmp;
    double* local = gathered + 2 * (size_t)nr;
    double* sc = local + 2;
    begin_history(max_iter);
    // the rank sums of `count` dot products whose partials sit in part0 (and part1): one
    // reduction each, one allgather of `count` values per rank
    auto rank_sums = [&](int count) -> const double* {
        launch_reduce_partials(s, g, part0, tmp, local);
        if (count == 2) launch_reduce_partials(s, g, part1, tmp, local + 1);
        if (nr == 1) return local;
        ctx->allgather(local, gathered, (size_t)count);
        return gathered;
    };
    auto apply_m = [&](const double* in, double* out) {  // out = M(in): one V-cycle from zero
        launch_zero(s, n, out);
        cycle_rec(0, out, in, false, false);
    };
    auto first = [&] {  // phat = M p; v = A phat; alpha = rho / rhat.v; s = r - alpha v
        apply_m(p, ph);
        par_apply(A, KM_SPMV, ph, nullptr, v, 0.0, nullptr);
        launch_dot_partials(s, n, rhat, v, part0);
        launch_bicg_alpha(s, nr, rank_sums(1), sc);
        launch_bicg_s(s, n, sc, r, v, sv);
    };
    auto second = [&] {  // shat = M s; t = A shat; omega; x, r; ||r|| appended; beta; p
        apply_m(sv, sh);
        par_apply(A, KM_SPMV, sh, nullptr, t, 0.0, nullptr);
        launch_bicg_tsdot(s, n, sc, t, sv, part0, part1);
        launch_bicg_omega(s, nr, rank_sums(2), sc);
        launch_bicg_xr(s, n, sc, ph, sh, sv, t, rhat, x, r, part0, part1);
        launch_bicg_step(s, nr, rank_sums(2), sc, hist.p, hist_counter.p);
        launch_bicg_p(s, n, sc, r, v, p);
    };
    par_apply(A, KM_RESID, x, b, r, 0.0, nullptr);
    if (n) {
        HIP_CHECK(hipMemcpyAsync(rhat, r, n * sizeof(double), hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpyAsync(p, r, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    launch_dot_partials(s, n, r, r, part0);
    launch_bicg_start(s, nr, rank_sums(1), sc, tol, hist.p, hist_counter.p);
    // one collective graph decision for both iteration graphs (keyed by the caller's x, b)
    agree_stale({G_BICG_S, G_BICG_XR}, x, b);
    double flag = BICG_RUN;
    for (int32_t it = 0; it < max_iter; ++it) {
        run(G_BICG_S, x, b, first);
        run(G_BICG_XR, x, b, second);
        if (tol > 0.0) {  // the device applied the stopping rules: the host only learns of it
            flag = read_scalar(sc + BS_FLAG);
            if (flag != BICG_RUN) break;
        }
    }
    int count = 0;
    HIP_CHECK(hipMemcpyAsync(&count, hist_counter.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&flag, sc + BS_FLAG, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    ctx->graph_inflight = false;
    AMG_ASSERT(count >= 1 && count <= max_iter + 1);
    download_history(hist_host, (size_t)count);
    *status = flag == BICG_BREAKDOWN ? AMG_KRYLOV_BREAKDOWN : AMG_KRYLOV_OK;
    return count - 1;
}

// ---- AMG-preconditioned restarted FGMRES --------------------------------------
// Right-preconditioned flexible GMRES, M = one V-cycle from zero, one-pass classical
// Gram-Schmidt.  The column index j, the iteration count, the stop flag, g, cs, sn, the packed
// H, c and y stay on the device (sc[FG_*]): the kernels read j there and take the basis base
// pointers, so one launch sequence -- one captured graph, G_FGMRES_STEP -- serves every Arnoldi
// step, and G_FGMRES_RESTART (back substitution, the x update over the J columns completed, r =
// b - A x, beta, v_0) opens every cycle and closes the call.  The x update zeroes J, so the
// closing launch after a mid-cycle stop applies exactly the completed columns once.  With tol ==
// 0 nothing waits for the host before the history download.  The cycle is captured on fixed
// addresses: v_j is also written to `vin`, and the cycle's output `zout` is copied to Z's slot j.
int32_t Solver::fgmres(double* x, const double* b, int32_t restart, int32_t max_iter, double tol,
                       double* hist_host, int32_t* status) {
    AMG_CHECK(max_iter >= 0, "max_iter must be >= 0");
    AMG_CHECK(restart >= 1 && restart <= kFgMax, "restart must be 1 .. AMG_FGMRES_MAX_RESTART");
    RoctxRange range("ParMultilevel::fgmres");
    DevMatrix& A = *A0;
    const int64_t n = A.n_rows;
    hipStream_t s = ctx->stream;
    const int nr = ctx->host.nranks;
    const int g = dot_partial_count(n);
    const size_t ntmp = (size_t)kFgMax * ((size_t)g / 4096 + 1) + 64;
    // both grow with restart only: a smaller restart runs in the same buffers and graphs (the
    // basis pairs sit behind the three fixed vectors, restart is read from the device)
    const size_t m = (size_t)std::max(restart, fgmres_room);
    const size_t need = m * (size_t)g + ntmp + (size_t)kFgMax * (size_t)nr + kFgMax + FG_N;
    // a fresh scratch is zeroed: after a stop the gated kernels leave partials unwritten and
    // the reductions and allgathers still read them
    if (grow_work(fgmres_vec, (2 * m + 3) * (size_t)n + 1, fgmres_scratch, need, {G_FGMRES_STEP, G_FGMRES_RESTART}))
        HIP_CHECK(hipMemsetAsync(fgmres_scratch.p, 0, need * sizeof(double), s));
    fgmres_room = (int32_t)m;
    double* w = fgmres_vec.p;
    double* vin = w + n;
    double* zout = vin + n;
    double* V = zout + n;
    double* Z = V + n;
    const int64_t stride = 2 * n;
    double* part = fgmres_scratch.p;
    double* tmp = part + m * (size_t)g;
    double* gathered = tmp + ntmp;
    double* local = gathered + (size_t)kFgMax * (size_t)nr;
    double* sc = local + kFgMax;
    begin_history(max_iter);
    launch_fgmres_init(s, sc, tol, restart, max_iter);
    // the rank sums of the dot product whose partials sit in part's first row
    auto rank_sums = [&]() -> const double* {
        launch_reduce_partials(s, g, part, tmp, local);
        if (nr == 1) return local;
        ctx->allgather(local, gathered, 1);
        return gathered;
    };
    auto step = [&] {  // column j: z_j = M(v_j); w = A z_j; c; w -= sum c_i v_i; eta; rotations; v_{j+1}
        launch_zero(s, n, zout);
        cycle_rec(0, zout, vin, false, false);
        par_apply(A, KM_SPMV, zout, nullptr, w, 0.0, nullptr);
        launch_fgmres_keep(s, n, sc, zout, Z, stride);
        launch_fgmres_dots(s, n, sc, w, V, stride, part);
        launch_fgmres_reduce(s, g, sc, part, tmp, local);
        if (nr > 1) ctx->allgather(local, gathered, (size_t)kFgMax);  // the j + 1 sums in one exchange
        launch_fgmres_c(s, nr, nr > 1 ? gathered : local, sc);
        launch_fgmres_update(s, n, sc, V, stride, w, part);
        launch_fgmres_column(s, nr, rank_sums(), sc, hist.p, hist_counter.p);
        launch_fgmres_scale(s, n, sc, w, V, stride, vin);
    };
    auto cycle_start = [&] {  // x += Z y over the columns completed; r = b - A x; beta; v_0
        launch_fgmres_y(s, sc);
        launch_fgmres_x(s, n, sc, Z, stride, x);
        par_apply(A, KM_RESID, x, b, w, 0.0, nullptr);
        launch_dot_partials(s, n, w, w, part);
        launch_fgmres_begin(s, nr, rank_sums(), sc, hist.p, hist_counter.p);
        launch_fgmres_scale(s, n, sc, w, V, stride, vin);
    };
    // one collective graph decision for both graphs (keyed by the caller's x, b)
    agree_stale({G_FGMRES_STEP, G_FGMRES_RESTART}, x, b);
    run(G_FGMRES_RESTART, x, b, cycle_start);
    double flag = FG_RUN;
    bool open = false;  // columns completed and not yet applied to x
    for (int32_t it = 0; it < max_iter; ++it) {
        run(G_FGMRES_STEP, x, b, step);
        open = true;
        if ((it + 1) % restart == 0 || it + 1 == max_iter) {
            run(G_FGMRES_RESTART, x, b, cycle_start);
            open = false;
        }
        if (tol > 0.0) {  // the device applied the stopping rules: the host only learns of it
            flag = read_scalar(sc + FG_FLAG);
            if (flag != FG_RUN) break;
        }
    }
    if (open) run(G_FGMRES_RESTART, x, b, cycle_start);  // a stop inside a cycle: its columns
    int count = 0;
    HIP_CHECK(hipMemcpyAsync(&count, hist_counter.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&flag, sc + FG_FLAG, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    ctx->graph_inflight = false;
    AMG_ASSERT(count >= 1 && count <= max_iter + 1);
    download_history(hist_host, (size_t)count);
    *status = flag == FG_BREAKDOWN ? AMG_KRYLOV_BREAKDOWN : AMG_KRYLOV_OK;
    return count - 1;
}

static int64_t spmv_bytes(const DevMatrix& M) {
    // a segment row map is one more index stream of the operator: 4 B per segment
    const int64_t map = M.row_seg > 0 ? 4 * (M.n_rows / M.row_seg) : 0;
    return 12 * M.nnz + 4 * (M.n_rows + 1) + 8 * M.n_cols_local + 8 * M.n_rows + map;
}

int64_t Solver::bytes_per_cycle(size_t l) const {
    const DevMatrix& A = CA(l);
    const int64_t n = A.n_rows;
    if (l + 1 == levels.size()) return 8 * coarse_n * n + 8 * coarse_n + 8 * n;
    const int64_t base = 12 * A.nnz + 4 * (n + 1);
    const int64_t jac = base + 32 * n;
    // Chebyshev: step 0 costs what a Jacobi sweep costs there, each later step + xprev
    const int64_t later = (sweep_steps() - 1) * (base + 40 * n);
    int64_t b = 0;
    bool zero = l > 0;
    int64_t sweeps = 0;
    for (int k = 0; k < opt.pre_sweeps; ++k, ++sweeps) {
        if (zero && jacobi_like()) b += 24 * n;
        else b += jac + (zero ? 8 * n : 0);
        b += later;
        zero = false;
    }
    if (zero) b += 8 * n;
    b += base + 24 * n;                                   // residual
    b += spmv_bytes(CR(l));                            // restriction
    b += spmv_bytes(CP(l)) + 8 * n;                    // interpolation (reads x)
    b += opt.post_sweeps * (jac + later);
    sweeps += opt.post_sweeps;
    // (multicolour GS sweeps in place: priced as a GS sweep, never copied back)
    if (opt.smoother != AMG_SMOOTH_MC_GS && sweeps * sweep_steps() % 2 == 1) b += 16 * n;  // copy back
    return b;
}

// Mirrors cycle_rec(): per operation the stored-format bytes of the kernel that runs it
// (DevMatrix::mode_bytes, the sliced-ELL stream for hybrid GS), plus the vector-only passes.
int64_t Solver::stored_bytes_per_cycle(size_t l) const {
    const DevMatrix& A = CA(l);  // the operators the cycle runs
    const int64_t n = A.n_rows;
    if (l + 1 == levels.size()) return 8 * coarse_n * n + 8 * coarse_n + 8 * n;
    // multicolour GS: its own format's byte model per sweep, in place (no fused sweep from zero,
    // no copy back)
    const bool mc = opt.smoother == AMG_SMOOTH_MC_GS;
    const bool gs = opt.smoother == AMG_SMOOTH_HYBRID_GS || mc;
    const int64_t sweep = mc ? A.mc.bytes : gs ? A.gs.bytes : A.mode_bytes(KM_JACOBI);
    const int64_t later = (sweep_steps() - 1) * A.mode_bytes(KM_CHEBY);  // Chebyshev steps k >= 1
    int64_t b = 0;
    bool zero = l > 0;
    int64_t sweeps = 0;
    // the sweep from zero fused into the restriction above (cycle_rec): dinv read + x write
    const DevMatrix* Rup = l > 0 ? &CR(l - 1) : nullptr;
    const bool j0 = !gs && Rup && (int)l != rep_level && Rup->format != AMG_FORMAT_CSR &&
                    !Rup->tpl_on();
    // a split GS sweep from zero is its chain walk alone (par_hybrid_gs_from_zero)
    const int64_t sweep0 = gs && !mc && A.gs.split.on ? sweep - A.gs.split.old[1]->mode_bytes(KM_RESID) - 8 * n : sweep;
    for (int k = 0; k < opt.pre_sweeps; ++k, ++sweeps) {
        if (zero && !gs) b += (j0 ? 16 : 24) * n;  // omega * dinv * b
        else b += (zero ? sweep0 : sweep) + (zero ? 8 * n : 0);  // (zero fill of x first)
        b += later;
        zero = false;
    }
    if (zero) b += 8 * n;
    b += A.mode_bytes(KM_RESID);
    b += CR(l).mode_bytes(KM_SPMV);
    b += CP(l).mode_bytes(KM_SPMV_ADD);
    b += opt.post_sweeps * (sweep + later);
    sweeps += opt.post_sweeps;
    if (!mc && sweeps * sweep_steps() % 2 == 1) b += 16 * n;  // copy back
    return b;
}

}  // namespace amg
