// Stand-alone check of the host-only stream logic (df-vo_amd/csrc/stream_layout.h): the pool's classification of probe times
// into pipe groups / hardware queues, and the fused pipeline's role -> stream plan.  Built with -fsanitize=address,undefined
// and run by tests/test_stream_layout_cpu.py:  stream_layout_check <case> ; exit status 0 = the case holds.
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../df-vo_amd/csrc/stream_layout.h"

using namespace dfvo;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

// Synthetic probe times of n candidates with the given pipe and queue of each: base 40 us, spinning 160 us.  The chain
// starts ~30 us into the spinning (the host's eight launches): alone it ends 90 us before the spinning does, next to a
// busy stream of its pipe it takes 100 us and ends 30 us before it, behind one of its own queue it runs after it.
struct Probe {
    int n;
    std::vector<float> base;
    std::vector<PoolSample> m1, m2;
    Probe(const std::vector<int>& pipe, const std::vector<int>& queue) : n((int)pipe.size()), base(n, 40.f), m1((size_t)n * n), m2(m1) {
        for (int a = 0; a < n; ++a)
            for (int b = a + 1; b < n; ++b) set(a, b, queue[a] == queue[b] ? POOL_REL_QUEUE : pipe[a] == pipe[b] ? POOL_REL_PIPE : POOL_REL_NONE);
    }
    static PoolSample sample(int rel) {
        if (rel == POOL_REL_QUEUE) return PoolSample{41.f, 44.f};
        if (rel == POOL_REL_PIPE) return PoolSample{100.f, -30.f};
        return PoolSample{42.f, -88.f};
    }
    void set(int a, int b, int rel) { m1[(size_t)a * n + b] = m2[(size_t)a * n + b] = sample(rel); }
    void set_first_only(int a, int b, int rel) {  // a positive that does not repeat
        m1[(size_t)a * n + b] = sample(rel);
        m2[(size_t)a * n + b] = sample(POOL_REL_NONE);
    }
    bool classify(PoolClasses* c) const { return pool_classify(n, base.data(), m1.data(), m2.data(), c); }
};

static std::vector<int> iota_mod(int n, int m) {
    std::vector<int> v(n);
    for (int i = 0; i < n; ++i) v[i] = i % m;
    return v;
}

static void twelve_on_four_queues() {
    // queue membership as the hardware hands it out when candidates outnumber the queues (not i mod 4), a pipe per queue
    const std::vector<int> q = {0, 1, 2, 3, 3, 2, 1, 0, 3, 2, 1, 0};
    Probe p(q, q);
    PoolClasses c;
    CHECK(p.classify(&c));
    CHECK(c.nqueues == 4 && c.ngroups == 4);
    CHECK(c.queue_group == q && c.group == q);
    CHECK(pool_expected_shape(c));
    int pick[4];
    CHECK(pick_lane_candidates(c, pick));
    CHECK(pick[0] == 0 && pick[1] == 1 && pick[2] == 2 && pick[3] == 3);
}

static void twelve_queues_four_pipes() {
    std::vector<int> q(12);
    for (int i = 0; i < 12; ++i) q[i] = i;
    Probe p(iota_mod(12, 4), q);
    PoolClasses c;
    CHECK(p.classify(&c));
    CHECK(c.nqueues == 12 && c.ngroups == 4);
    CHECK(c.group == iota_mod(12, 4) && c.queue_group == q);
    CHECK(pool_expected_shape(c));
    int pick[4];
    CHECK(pick_lane_candidates(c, pick));
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j) CHECK(c.group[pick[i]] != c.group[pick[j]]);
}

static void five_queues_uneven() {
    // a process that already owns streams: five queues behind twelve candidates, 3 3 2 2 2, two of the queues on one pipe
    const std::vector<int> q = {0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1};
    const std::vector<int> pipe = {0, 1, 2, 3, 0, 0, 1, 2, 3, 0, 0, 1};
    Probe p(pipe, q);
    PoolClasses c;
    CHECK(p.classify(&c));
    CHECK(c.nqueues == 5 && c.ngroups == 4);
    CHECK(c.queue_group == q && c.group == pipe);
    CHECK(!pool_expected_shape(c));  // accepted only when a second pass repeats it
    int pick[4];
    CHECK(pick_lane_candidates(c, pick));
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j) CHECK(c.queue_group[pick[i]] != c.queue_group[pick[j]] && c.group[pick[i]] != c.group[pick[j]]);
}

static void positive_not_repeated() {
    std::vector<int> q(12);
    for (int i = 0; i < 12; ++i) q[i] = i;
    Probe p(iota_mod(12, 4), q);
    p.set_first_only(0, 1, POOL_REL_PIPE);   // different pipes: one slow measurement
    p.set_first_only(2, 3, POOL_REL_QUEUE);  // different queues: one late chain
    PoolClasses c;
    CHECK(p.classify(&c));
    CHECK(c.group == iota_mod(12, 4) && c.queue_group == q);
    // a queue positive whose repeat only shows the pipe: one pipe, two queues
    Probe p2(iota_mod(12, 4), q);
    p2.m1[0 * 12 + 4] = Probe::sample(POOL_REL_QUEUE);
    PoolClasses c2;
    CHECK(p2.classify(&c2));
    CHECK(c2.group == iota_mod(12, 4) && c2.queue_group == q);
}

static void inconsistent() {
    std::vector<int> q(12);
    for (int i = 0; i < 12; ++i) q[i] = i;
    Probe p(iota_mod(12, 4), q);
    p.set(0, 8, POOL_REL_NONE);  // 0 ~ 4 and 4 ~ 8 share a pipe, 0 and 8 do not
    PoolClasses c;
    CHECK(!p.classify(&c));
    CHECK(c.group.size() == 12 && c.queue_group.size() == 12);  // filled in all the same (the probe prints them)
    const std::vector<int> q4 = {0, 1, 2, 3, 3, 2, 1, 0, 3, 2, 1, 0};
    Probe p4(q4, q4);
    p4.set(0, 11, POOL_REL_PIPE);  // 0 ~ 7 and 7 ~ 11 share a queue, 0 and 11 only a pipe
    CHECK(!p4.classify(&c));
    CHECK(c.group.size() == 12 && c.queue_group.size() == 12);
}

static void thresholds() {
    CHECK(pool_rel_of(40.f, PoolSample{40.f, -100.f}) == POOL_REL_NONE);
    CHECK(pool_rel_of(40.f, PoolSample{63.f, -60.f}) == POOL_REL_NONE);
    CHECK(pool_rel_of(40.f, PoolSample{66.f, -60.f}) == POOL_REL_PIPE);
    CHECK(pool_rel_of(40.f, PoolSample{160.f, 20.f}) == POOL_REL_PIPE);  // a slow chain that outlasts the spinning a little
    CHECK(pool_rel_of(40.f, PoolSample{40.f, 24.f}) == POOL_REL_QUEUE);
    CHECK(pool_rel_of(40.f, PoolSample{40.f, 45.f}) == POOL_REL_QUEUE);
}

static void plan_for(int nqueues) {
    // what the pool reports with nqueues hardware queues: a pipe group per queue up to the four pipes
    const int ngroups = nqueues < 4 ? nqueues : 4;
    const StreamPlan p = plan_stream_layout(ngroups, nqueues, LAYOUT_CHOICE_AUTO);
    static const int wide[ROLE_COUNT] = {0, 0, 0, 1, 1, 1, 2, 3};  // the role table R of the twelve-queue layout
    if (nqueues < 4) {
        CHECK(p.layout == LAYOUT_CREATION);
        for (int r = 0; r < ROLE_COUNT; ++r) CHECK(p.lane[r] == -1);
        CHECK(plan_stream_layout(ngroups, nqueues, LAYOUT_CHOICE_LANES).layout == LAYOUT_CREATION);
        CHECK(plan_stream_layout(ngroups, nqueues, LAYOUT_CHOICE_WIDE).layout == LAYOUT_CREATION);
    } else if (nqueues < 8) {
        CHECK(p.layout == LAYOUT_LANES);
        bool used[4] = {false, false, false, false};
        for (int r = 0; r < ROLE_COUNT; ++r) {
            CHECK(p.lane[r] >= 0 && p.lane[r] < 4);  // every role mapped
            if (p.lane[r] >= 0 && p.lane[r] < 4) used[p.lane[r]] = true;
        }
        CHECK(used[0] && used[1] && used[2] && used[3]);
        CHECK(p.lane[ROLE_TRK] != p.lane[ROLE_FLOW] && p.lane[ROLE_TRK] != p.lane[ROLE_FLOW_X]);
        CHECK(p.lane[ROLE_REP0] == p.lane[ROLE_TRK] && p.lane[ROLE_REP1] == p.lane[ROLE_TRK]);
        // the measured winner (profiles/lanes_ab.txt): both pre-parts behind the depth net, not behind the flow net of their
        // parity -- a homography chain on a flow lane keeps that lane's net from the machine for its 1.4 ms of one-workgroup kernels
        CHECK(p.lane[ROLE_PRE0] == p.lane[ROLE_DEPTH] && p.lane[ROLE_PRE1] == p.lane[ROLE_DEPTH]);
        CHECK(p.lane[ROLE_FLOW] != p.lane[ROLE_FLOW_X]);
        CHECK(p.lane[ROLE_DEPTH] != p.lane[ROLE_TRK] && p.lane[ROLE_DEPTH] != p.lane[ROLE_FLOW] && p.lane[ROLE_DEPTH] != p.lane[ROLE_FLOW_X]);
        const StreamPlan w = plan_stream_layout(ngroups, nqueues, LAYOUT_CHOICE_WIDE);
        CHECK(w.layout == LAYOUT_WIDE);
        for (int r = 0; r < ROLE_COUNT; ++r) CHECK(w.lane[r] == wide[r]);
    } else {
        CHECK(p.layout == LAYOUT_WIDE);
        for (int r = 0; r < ROLE_COUNT; ++r) CHECK(p.lane[r] == wide[r]);
        CHECK(plan_stream_layout(ngroups, nqueues, LAYOUT_CHOICE_LANES).layout == LAYOUT_LANES);
    }
    CHECK(plan_stream_layout(0, 0, LAYOUT_CHOICE_AUTO).layout == LAYOUT_CREATION);  // the probe failed
    CHECK(std::string(stream_layout_name(p.layout)) == (nqueues < 4 ? "creation" : nqueues < 8 ? "lanes" : "wide"));
}

static void too_few_queues_to_pick() {
    const std::vector<int> q = {0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2};
    Probe p(q, q);
    PoolClasses c;
    CHECK(p.classify(&c));
    CHECK(c.nqueues == 3);
    int pick[4];
    CHECK(!pick_lane_candidates(c, pick));
}

int main(int argc, char** argv) {
    std::map<std::string, std::function<void()>> cases = {
        {"classify_twelve_on_four_queues", twelve_on_four_queues},
        {"classify_twelve_queues_four_pipes", twelve_queues_four_pipes},
        {"classify_five_queues_uneven", five_queues_uneven},
        {"classify_positive_not_repeated", positive_not_repeated},
        {"classify_inconsistent", inconsistent},
        {"classify_thresholds", thresholds},
        {"pick_too_few_queues", too_few_queues_to_pick},
    };
    for (int nq : {1, 2, 3, 4, 5, 7, 8, 12}) cases["plan_nqueues_" + std::to_string(nq)] = [nq] { plan_for(nq); };
    if (argc == 2 && !strcmp(argv[1], "--list")) {
        for (auto& kv : cases) printf("%s\n", kv.first.c_str());
        return 0;
    }
    if (argc != 2 || !cases.count(argv[1])) {
        fprintf(stderr, "usage: stream_layout_check <case> | --list\n");
        return 2;
    }
    cases[argv[1]]();
    printf("%s: %s\n", argv[1], g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
