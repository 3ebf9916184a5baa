// Stand-alone check of the solver chain's buffer lifetimes (df-vo_amd/csrc/dev_mem.h, solver_buffers.hip): this program is
// linked with solver_buffers.hip compiled as plain C++ and with no HIP library -- the few HIP entry points that unit calls
// are defined in hip_stub.h on malloc / free, with a "fail the k-th allocation" counter, call counters and a registry of the
// live blocks, streams and events.  Built with -fsanitize=address,undefined and run by tests/test_solver_buffers_cpu.py:
// solver_buffers_check <case> ; exit status 0 = the case holds.
#include "hip_stub.h"

#include "../../df-vo_amd/csrc/tracker.h"

// ---- what the cases look at: every owning member of a buffer set as (pointer, elements, bytes per element) ----
struct Arr {
    const void* p;
    size_t n, elem;
};
template <class T>
static Arr arr(const DevArr<T>& a) {
    return Arr{a.p, a.n, sizeof(T)};
}
static std::vector<Arr> members(const RansacWorkspace& w) {
    return {arr(w.state), arr(w.pts_a), arr(w.pts_b), arr(w.norm_a), arr(w.norm_b), arr(w.f_a), arr(w.f_b), arr(w.idx), arr(w.ws),
            arr(w.ok), arr(w.models), arr(w.nmodels), arr(w.counts), arr(w.mask), arr(w.out), arr(w.lm), arr(w.cidx)};
}
static std::vector<Arr> members(const PnpBuffers& b) {
    return {arr(b.info), arr(b.fk1), arr(b.fk2), arr(b.xyz), arr(b.perm), arr(b.obj), arr(b.img), arr(b.state), arr(b.idx),
            arr(b.models), arr(b.nmodels), arr(b.counts), arr(b.mask), arr(b.keep), arr(b.pts5), arr(b.rep_out), arr(b.result)};
}
static std::vector<Arr> members(const BestNBuffers& b) {
    return {arr(b.key_base), arr(b.tosort), arr(b.map), arr(b.Lpos), arr(b.Rpos), arr(b.count), arr(b.kp)};
}
static std::vector<Arr> members(const RigidKpBuffers& b) {
    return {arr(b.depth32), arr(b.rdiff), arr(b.mats), arr(b.cell_count), arr(b.cell_sel), arr(b.cell_sel_uni), arr(b.info),
            arr(b.zero), arr(b.lidx), arr(b.kp)};
}
static std::vector<Arr> members(const TrackerBuffers& t) {  // the keypoint-sized set of ensure_kp
    return {arr(t.kp_ref), arr(t.kp_cur), arr(t.pa), arr(t.pb), arr(t.perm), arr(t.res), arr(t.best_inliers), arr(t.cell_count),
            arr(t.cell_sel), arr(t.z2), arr(t.pix), arr(t.ratios), arr(t.inl_a), arr(t.inl_b), arr(t.scratch)};
}
// the capacities that are parameters of a set, and an array (index into members()) each of them bounds, with its elements per unit
struct Cap {
    size_t value;
    int member;
    size_t per_unit;
};
static std::vector<Cap> caps(const RansacWorkspace& w) { return {{(size_t)w.cap_n, 1, 2}, {(size_t)w.cap_n, 13, 1}, {(size_t)w.cap_iters, 7, 5}}; }
static std::vector<Cap> caps(const PnpBuffers& b) { return {{(size_t)b.cap, 13, 1}, {(size_t)b.cap, 3, 3}, {(size_t)b.iters_cap, 8, 5}}; }
static std::vector<Cap> caps(const BestNBuffers& b) { return {{b.cap, 1, 1}, {b.cap, 2, 1}, {b.cap, 0, 1}}; }
static std::vector<Cap> caps(const RigidKpBuffers& b) { return {{(size_t)b.sel_cap, 4, 1}, {(size_t)b.sel_cap, 5, 1}, {(size_t)b.sel_cap, 9, 8}}; }
static std::vector<Cap> caps(const TrackerBuffers& t) { return {{(size_t)t.kp_cap, 0, 2}, {(size_t)t.kp_cap, 14, 1}, {(size_t)t.sel_cap, 8, 1}}; }

// the rule: every pointer null or a live block that holds its `n` elements, no capacity beyond what is allocated
template <class W>
static bool sound(const W& w) {
    const std::vector<Arr> m = members(w);
    for (const Arr& a : m) {
        if (!a.p && a.n) return false;
        if (a.p) {
            auto it = g_blocks.find((void*)a.p);
            if (it == g_blocks.end() || it->second < a.n * a.elem) return false;
        }
    }
    for (const Cap& c : caps(w))
        if (c.value * c.per_unit > m[c.member].n) return false;
    return true;
}
template <class W>
static bool empty(const W& w) {
    for (const Arr& a : members(w))
        if (a.p || a.n) return false;
    for (const Cap& c : caps(w))
        if (c.value) return false;
    return true;
}
template <class W>
static bool full(const W& w) {
    for (const Arr& a : members(w))
        if (!a.p) return false;
    return true;
}

// (a) .. (d) of a buffer set: `small` and `large` are two ensure calls, the second of which grows every dimension.  The k-th
// allocation fails, of `large` on an empty set and of `large` on a set that holds `small`
template <class W>
static void fail_each(const std::function<int(W&)>& small, const std::function<int(W&)>& large) {
    for (int from_small = 0; from_small < 2; ++from_small) {
        int n_empty = 0, n_allocs = 0;  // allocations of `large` on an empty set, and from the state the failures start at
        {
            W w;
            arm(-1);
            CHECK(large(w) == DFVO_OK && full(w) && sound(w));
            n_empty = n_allocs = g_allocs;
            w.release();
            CHECK(empty(w));
            if (from_small) {
                CHECK(small(w) == DFVO_OK);
                arm(-1);
                CHECK(large(w) == DFVO_OK && full(w) && sound(w));
                n_allocs = g_allocs;
                w.release();
            }
        }
        CHECK(n_allocs >= 6 && n_allocs <= n_empty);
        for (int k = 0; k < n_allocs; ++k) {
            W w;
            arm(-1);
            if (from_small) CHECK(small(w) == DFVO_OK && full(w) && sound(w));
            arm(k);
            CHECK(large(w) == DFVO_ERR_HIP);  // (a)
            CHECK(g_last_error.find("hipMalloc") != std::string::npos);
            CHECK(sound(w) && empty(w));  // (b)
            arm(-1);
            CHECK(large(w) == DFVO_OK && full(w) && sound(w));  // (c)
            CHECK(g_allocs == n_empty);
            arm(0);
            CHECK(large(w) == DFVO_OK && g_hip_calls == 0);
            w.release();  // (d), with the sanitizers and the registry
            CHECK(empty(w));
            CHECK(g_blocks.empty());
        }
    }
}

static void ransac_fail_each() {
    fail_each<RansacWorkspace>([](RansacWorkspace& w) { return w.ensure(8, 100); }, [](RansacWorkspace& w) { return w.ensure(500, 1000); });
}
static void pnp_fail_each() {
    fail_each<PnpBuffers>([](PnpBuffers& b) { return b.ensure(16, 20); }, [](PnpBuffers& b) { return b.ensure(2008, 100); });
}
static void bestn_fail_each() {
    fail_each<BestNBuffers>([](BestNBuffers& b) { return b.ensure(100, 10); }, [](BestNBuffers& b) { return b.ensure(1000, 50); });
}
static void rigid_fail_each() {
    fail_each<RigidKpBuffers>([](RigidKpBuffers& b) { return b.ensure(10, 13, 4, 2, 30); },
                              [](RigidKpBuffers& b) { return b.ensure(40, 50, 10, 20, 300); });
}
static void tracker_kp_fail_each() {
    fail_each<TrackerBuffers>([](TrackerBuffers& t) { return t.ensure_kp(16, 1, 1); }, [](TrackerBuffers& t) { return t.ensure_kp(100, 4, 4); });
}

// a failure in one of the later, independent parts of the two sets that grow by parts: everything is released, not that part alone
static void parts_fail_releases_all() {
    BestNBuffers b;
    arm(-1);
    CHECK(b.ensure(100, 10) == DFVO_OK);
    arm(0);
    CHECK(b.ensure(100, 20) == DFVO_ERR_HIP && sound(b) && empty(b));  // only kp grows, and fails
    RigidKpBuffers r;
    arm(-1);
    CHECK(r.ensure(10, 13, 4, 2, 30) == DFVO_OK);
    arm(0);
    CHECK(r.ensure(10, 13, 4, 2, 60) == DFVO_ERR_HIP && sound(r) && empty(r));  // only lidx
    arm(-1);
    CHECK(r.ensure(10, 13, 4, 2, 30) == DFVO_OK);
    arm(1);
    CHECK(r.ensure(10, 13, 4, 4, 30) == DFVO_ERR_HIP && sound(r) && empty(r));  // the selection lists, the second of them
    CHECK(g_blocks.empty());
}

static void fits_no_calls() {
    RansacWorkspace w;
    PnpBuffers p;
    BestNBuffers b;
    RigidKpBuffers r;
    TrackerBuffers t;
    arm(-1);
    CHECK(w.ensure(500, 1000) == DFVO_OK && p.ensure(200, 100) == DFVO_OK && b.ensure(1000, 50) == DFVO_OK &&
          r.ensure(40, 50, 10, 20, 300) == DFVO_OK && t.ensure_kp(100, 4, 4) == DFVO_OK);
    CHECK(t.grow_winner(40, 50) == DFVO_OK && t.grow_lidx(10, 300) == DFVO_OK && t.grow_ratio_map(40, 50) == DFVO_OK);
    arm(0);  // any allocation would fail
    CHECK(w.ensure(500, 1000) == DFVO_OK && w.ensure(8, 1000) == DFVO_OK && w.ensure(500, 1) == DFVO_OK);
    CHECK(p.ensure(200, 100) == DFVO_OK && p.ensure(1, 1) == DFVO_OK);
    CHECK(b.ensure(1000, 50) == DFVO_OK && b.ensure(10, 0) == DFVO_OK);
    CHECK(r.ensure(40, 50, 10, 20, 300) == DFVO_OK && r.ensure(20, 100, 20, 10, 150) == DFVO_OK);
    CHECK(t.ensure_kp(100, 4, 4) == DFVO_OK && t.ensure_kp(16, 1, 1) == DFVO_OK && t.ensure_kp(100, 16, 1) == DFVO_OK);
    CHECK(t.grow_winner(50, 40) == DFVO_OK && t.grow_lidx(300, 10) == DFVO_OK && t.grow_ratio_map(1, 1) == DFVO_OK);
    CHECK(g_hip_calls == 0);
    t.release();  // (the other sets go with their members' destructors)
}

static void grow_one_dimension() {
    RansacWorkspace w;
    arm(-1);
    CHECK(w.ensure(500, 100) == DFVO_OK && w.ensure(8, 1000) == DFVO_OK);
    CHECK(w.cap_n == 500 && w.cap_iters == 1000 && sound(w) && full(w));
    CHECK(w.ensure(600, 10) == DFVO_OK && w.cap_n == 600 && w.cap_iters == 1000 && sound(w));
    PnpBuffers p;
    CHECK(p.ensure(200, 10) == DFVO_OK && p.ensure(10, 100) == DFVO_OK && p.cap == 200 && p.iters_cap == 100 && sound(p));
    TrackerBuffers t;
    CHECK(t.ensure_kp(100, 4, 4) == DFVO_OK && t.ensure_kp(200, 1, 1) == DFVO_OK && t.kp_cap == 200 && t.sel_cap == 16 && sound(t));
    CHECK(t.ensure_kp(16, 5, 5) == DFVO_OK && t.kp_cap == 200 && t.sel_cap == 25 && sound(t));
    t.release();
    BestNBuffers b;
    CHECK(b.ensure(100, 50) == DFVO_OK);
    const double* kp = b.kp;
    CHECK(b.ensure(1000, 10) == DFVO_OK && b.cap == 1000 && b.kp == kp && b.kp.n == 200 && sound(b));  // the picks stay
    RigidKpBuffers r;
    CHECK(r.ensure(40, 50, 10, 20, 300) == DFVO_OK);
    const float* d32 = r.depth32;
    CHECK(r.ensure(10, 10, 30, 20, 10) == DFVO_OK && r.depth32 == d32 && r.sel_cap == 600 && r.lidx.n == 3000 && sound(r));
}

static void grow_on_demand_fail() {
    TrackerBuffers t;
    DevArr<int>& w = t.winner;
    arm(-1);
    CHECK(t.grow_winner(10, 13) == DFVO_OK && t.grow_lidx(4, 30) == DFVO_OK && t.grow_ratio_map(10, 13) == DFVO_OK);
    CHECK(w.n == 130 && t.lidx.n == 120 && t.ratio_map.n == 130);
    arm(0);
    CHECK(t.grow_winner(40, 50) == DFVO_ERR_HIP && !w.p && w.n == 0);
    arm(0);
    CHECK(t.grow_lidx(10, 300) == DFVO_ERR_HIP && !t.lidx.p && t.lidx.n == 0);
    arm(0);
    CHECK(t.grow_ratio_map(40, 50) == DFVO_ERR_HIP && !t.ratio_map.p && t.ratio_map.n == 0);
    CHECK(g_blocks.empty());
    arm(-1);
    CHECK(t.grow_winner(40, 50) == DFVO_OK && t.grow_lidx(10, 300) == DFVO_OK && t.grow_ratio_map(40, 50) == DFVO_OK);
    CHECK(w.p && w.n == 2000 && t.lidx.p && t.lidx.n == 3000 && t.ratio_map.p && t.ratio_map.n == 2000);
    t.release();
    CHECK(!w.p && !t.lidx.p && !t.ratio_map.p && g_blocks.empty());
}

// DevArr itself: moves hand the block over, the destructor releases
static void devarr_moves() {
    arm(-1);
    {
        DevArr<double> a, b;
        CHECK(a.alloc(10) == DFVO_OK && a.n == 10 && g_blocks.size() == 1);
        double* p = a;
        b = std::move(a);
        CHECK(!a.p && a.n == 0 && b.p == p && b.n == 10);
        DevArr<double> c(std::move(b));
        CHECK(!b.p && c.p == p && g_blocks.size() == 1);
        PinnedArr<int> h;
        CHECK(h.alloc(4) == DFVO_OK && h.grow(3) == DFVO_OK && g_allocs == 2);
        arm(0);
        CHECK(h.grow(5) == DFVO_ERR_HIP && !h.p && h.n == 0 && g_last_error.find("hipHostMalloc") != std::string::npos);
    }
    CHECK(g_blocks.empty());
}

// ---- side streams and events of TrackerBuffers: what the object created is destroyed once, what it was lent never ----
static hipStream_t lend_stream() {
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, 0) == hipSuccess);
    return s;
}
static void streams_init_own() {
    TrackerBuffers t;
    CHECK(t.init() == DFVO_OK);
    CHECK(g_streams.size() == (size_t)NUM_REP_STREAMS && t.n_rep_owned == NUM_REP_STREAMS);
    CHECK(t.enable_stage_timing() == DFVO_OK && t.mark(3, t.s_rep[0]) == DFVO_OK);
    CHECK(g_events.size() == (size_t)MAX_REP + 3 + TrackerBuffers::N_SEG);
    t.release();
    CHECK(g_streams.empty() && g_events.empty() && g_blocks.empty());
    t.release();  // a second release is harmless
}
static void streams_init_given() {
    hipStream_t a = lend_stream(), b = lend_stream();
    TrackerBuffers t;
    CHECK(t.init(a, b) == DFVO_OK && g_streams.size() == 2 && t.n_rep_owned == 2);  // handed over: the object destroys them
    CHECK(t.s_rep[0] == a && t.s_rep[1] == b && t.s_rep[2] == a && t.s_rep[3] == b);
    t.release();
    CHECK(g_streams.empty() && g_events.empty() && g_blocks.empty());
}
static void streams_borrowed_aliased() {
    hipStream_t s = lend_stream();
    TrackerBuffers t;
    CHECK(t.init(nullptr, nullptr, true) == DFVO_ERR_ARG);
    CHECK(t.init(s, s, true) == DFVO_OK && g_streams.size() == 1 && t.n_rep_owned == 0);
    for (int r = 0; r < MAX_REP; ++r) CHECK(t.s_rep[r] == s);
    t.release();
    CHECK(g_streams.count(s) == 1 && g_events.empty() && g_blocks.empty());
    CHECK(hipStreamDestroy(s) == hipSuccess && g_streams.empty());
}
static void streams_rebind() {
    TrackerBuffers t;
    CHECK(t.init() == DFVO_OK);
    hipStream_t a = lend_stream(), b = lend_stream();
    CHECK(t.rebind_streams(a, b) == DFVO_OK && g_streams.size() == 2 && t.n_rep_owned == 2);  // its own four are gone
    hipStream_t s = lend_stream();
    CHECK(t.rebind_streams(s, s, true) == DFVO_OK && g_streams.size() == 1 && t.n_rep_owned == 0);  // a and b were its own by then
    hipStream_t c = lend_stream();
    CHECK(t.rebind_streams(c, c) == DFVO_OK && g_streams.size() == 2 && g_streams.count(s) == 1);  // an owned, aliased pair
    t.release();
    CHECK(g_streams.size() == 1 && g_streams.count(s) == 1 && g_events.empty() && g_blocks.empty());
    CHECK(hipStreamDestroy(s) == hipSuccess);
}
static void streams_shared() {
    TrackerBuffers first, second;
    CHECK(first.init() == DFVO_OK);
    const size_t n_events = g_events.size(), n_blocks = g_blocks.size();
    CHECK(second.init_shared(first) == DFVO_OK && second.mt_state == first.mt_state && !second.mt_own.p);
    CHECK(g_streams.size() == (size_t)NUM_REP_STREAMS && g_events.size() == n_events + 2 && g_blocks.size() == n_blocks + 5);
    CHECK(second.rebind_streams(first.s_rep[0], first.s_rep[1]) == DFVO_ERR_ARG);
    CHECK(second.ensure_kp(16, 1, 1) == DFVO_OK);
    second.release();
    CHECK(g_streams.size() == (size_t)NUM_REP_STREAMS && g_events.size() == n_events && g_blocks.size() == n_blocks);
    CHECK(g_blocks.count(first.mt_state) == 1 && g_events.count(first.ev_fork) == 1 && g_events.count(first.ev_rep[0]) == 1);
    first.release();
    CHECK(g_streams.empty() && g_events.empty() && g_blocks.empty());
}

int main(int argc, char** argv) {
    const std::map<std::string, std::function<void()>> cases = {
        {"ransac_fail_each", ransac_fail_each},
        {"pnp_fail_each", pnp_fail_each},
        {"bestn_fail_each", bestn_fail_each},
        {"rigid_fail_each", rigid_fail_each},
        {"tracker_kp_fail_each", tracker_kp_fail_each},
        {"parts_fail_releases_all", parts_fail_releases_all},
        {"fits_no_calls", fits_no_calls},
        {"grow_one_dimension", grow_one_dimension},
        {"grow_on_demand_fail", grow_on_demand_fail},
        {"devarr_moves", devarr_moves},
        {"streams_init_own", streams_init_own},
        {"streams_init_given", streams_init_given},
        {"streams_borrowed_aliased", streams_borrowed_aliased},
        {"streams_rebind", streams_rebind},
        {"streams_shared", streams_shared},
    };
    if (argc == 2 && !strcmp(argv[1], "--list")) {
        for (const auto& c : cases) printf("%s\n", c.first.c_str());
        return 0;
    }
    auto it = argc == 2 ? cases.find(argv[1]) : cases.end();
    if (it == cases.end()) {
        fprintf(stderr, "usage: solver_buffers_check --list | <case>\n");
        return 2;
    }
    it->second();
    // whatever a case left behind is a leak (the leak checker of the sanitizer sees the same at exit)
    CHECK(g_blocks.empty() && g_streams.empty() && g_events.empty());
    if (g_failed) return 1;
    printf("%s: ok\n", it->first.c_str());
    return 0;
}
