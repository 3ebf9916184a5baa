// Host-only decision logic of the stream pool and of the fused pipeline's stream layout: no HIP call, no device type, so a
// plain C++ program can test it (tests/host_harness/stream_layout_check.cpp).
//
// 1. pool_classify: the probe's times -> which candidate streams share a dispatch PIPE and which share a hardware QUEUE.
//    The probe (stream_pool.hip) keeps stream a busy with back-to-back spinning kernels and meanwhile runs a chain of
//    dependent empty launches on stream b.  It reports the chain's own time (event in front of it -> event behind it) and
//    its LAG: the time from the end of the spinning on a to the end of the chain on b.
//      other pipe   the chain takes what it takes alone (base[b]) and ends long before the spinning: lag < 0
//      same pipe    its launches are dispatched ~2.5x slower while a is busy: chain > 1.6 base; it still ends before the
//                   spinning does, or -- a slow chain -- soon after it: lag well below base
//      same queue   one in-order queue: the chain STARTS when the spinning has drained.  Its own time is then the unloaded
//                   one (both of its events sit behind the spinning), which is why the chain time alone cannot see a
//                   shared queue; its lag is its whole length: lag >= base
//    A positive has to show in both of two measurements (a hiccup slows ONE measurement).  The relation has to be an
//    equivalence: a with b and b with c but not a with c is a measurement gone wrong, and the pass is not consistent.
// 2. plan_stream_layout: queue count -> which role of the pipeline runs on which stream.
#pragma once
#include <vector>

namespace dfvo {

enum PoolRel { POOL_REL_NONE = 0, POOL_REL_PIPE = 1, POOL_REL_QUEUE = 2 };

struct PoolSample {
    float chain_us;  // the chain on b while a spins
    float lag_us;    // end of the chain on b - end of the spinning on a
};

// one loaded measurement of the chain on a stream whose unloaded time is base_us
static inline int pool_rel_of(float base_us, PoolSample m) {
    if (m.lag_us >= 0.6f * base_us) return POOL_REL_QUEUE;
    return m.chain_us > 1.6f * base_us ? POOL_REL_PIPE : POOL_REL_NONE;
}

struct PoolClasses {
    std::vector<int> group;        // pipe group of candidate i; ids are canonical (order of first appearance)
    std::vector<int> queue_group;  // hardware queue of candidate i, likewise
    int ngroups = 0, nqueues = 0;
};

// first-appearance group ids of the relation rel(a, b) >= level over n candidates; false when it is no equivalence
static inline bool pool_groups_of(int n, const std::vector<int>& rel, int level, std::vector<int>* group, int* ngroups) {
    group->assign(n, -1);
    *ngroups = 0;
    auto R = [&](int a, int b) { return rel[(size_t)(a < b ? a : b) * n + (a < b ? b : a)] >= level; };
    for (int a = 0; a < n; ++a) {
        if ((*group)[a] >= 0) continue;
        (*group)[a] = *ngroups;
        for (int b = a + 1; b < n; ++b)
            if ((*group)[b] < 0 && R(a, b)) (*group)[b] = *ngroups;
        ++*ngroups;
    }
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b)
            if (R(a, b) != ((*group)[a] == (*group)[b])) return false;
    return true;
}

// base[n]; m1 / m2 [n * n], entry [a * n + b] with a < b: the chain on b while a spins, first and second measurement (m2 is
// only read where m1 is a positive; the probe measures it only there).  Returns false when the result is not consistent.
static inline bool pool_classify(int n, const float* base, const PoolSample* m1, const PoolSample* m2, PoolClasses* out) {
    std::vector<int> rel((size_t)n * n, POOL_REL_NONE);
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b) {
            const size_t i = (size_t)a * n + b;
            int r = pool_rel_of(base[b], m1[i]);
            if (r != POOL_REL_NONE) {
                const int r2 = pool_rel_of(base[b], m2[i]);
                r = r2 < r ? r2 : r;
            }
            rel[i] = r;
        }
    const bool pipes = pool_groups_of(n, rel, POOL_REL_PIPE, &out->group, &out->ngroups);
    const bool queues = pool_groups_of(n, rel, POOL_REL_QUEUE, &out->queue_group, &out->nqueues);
    return pipes && queues;  // (both filled in either way: the probe's verbose line prints them)
}

// The shape a process whose hardware queues are all its own must see with n = 4 m candidates created back to back: the
// queues go round the four pipes, so four pipe groups of m; and either every candidate has a queue of its own or the
// candidates went round q < n queues, n / q on each.
static inline bool pool_expected_shape(const PoolClasses& c) {
    const int n = (int)c.group.size();
    if (n == 0 || n % 4 != 0 || c.ngroups != 4 || c.nqueues < 4 || n % c.nqueues != 0) return false;
    std::vector<int> cg(c.ngroups, 0), cq(c.nqueues, 0);
    for (int i = 0; i < n; ++i) {
        ++cg[c.group[i]];
        ++cq[c.queue_group[i]];
    }
    for (int v : cg)
        if (v != n / 4) return false;
    for (int v : cq)
        if (v != n / c.nqueues) return false;
    return true;
}

// ---- the fused pipeline's roles and their streams -------------------------------------------------------------------
enum StreamRole { ROLE_TRK = 0, ROLE_REP0, ROLE_REP1, ROLE_DEPTH, ROLE_PRE0, ROLE_PRE1, ROLE_FLOW, ROLE_FLOW_X, ROLE_COUNT };
enum StreamLayout {
    LAYOUT_CREATION = 0,  // no usable measurement: freshly created streams, the runtime's creation order decides
    LAYOUT_WIDE = 1,      // a stream per role, placed by dispatch pipe (needs the hardware queues to back eight busy streams)
    LAYOUT_LANES = 2      // four streams, one per hardware queue; the roles of a lane share its stream
};
enum StreamLayoutChoice { LAYOUT_CHOICE_AUTO = 0, LAYOUT_CHOICE_WIDE, LAYOUT_CHOICE_LANES };

static inline const char* stream_role_name(int r) {
    static const char* const names[ROLE_COUNT] = {"trk", "rep0", "rep1", "depth", "pre0", "pre1", "flow", "flow_x"};
    return r >= 0 && r < ROLE_COUNT ? names[r] : "?";
}
static inline const char* stream_layout_name(int l) { return l == LAYOUT_WIDE ? "wide" : l == LAYOUT_LANES ? "lanes" : "creation"; }

struct StreamPlan {
    int layout = LAYOUT_CREATION;
    // WIDE: the pipe group (0 = largest .. 3) the role's own stream is taken from; LANES: the lane (0 .. 3) whose one stream
    // the role uses; CREATION: -1
    int lane[ROLE_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1};
};

// ngroups / nqueues: what the pool found (0: the probe failed).
//   wide   trk rep0 rep1 | depth pre0 pre1 | flow | flow_x: measured on twelve queues (profiles/r3k_layouts.txt)
//   lanes  Streams of one hardware queue execute in host enqueue order whatever their events say, so with fewer queues than
//          busy streams the pipeline takes ONE stream per queue and puts on it the roles the wide layout puts on one pipe:
//          flow | flow_x | depth + both pre-parts (keypoints, homography chain) | the RandomState-ordered chain and its side
//          streams.  Which queue a role shares is then the pipeline's decision, not the accident of which queue the runtime
//          dealt its stream onto (creation order on four queues: 249 frames/s against 305, profiles/lanes_ab.txt).
//          Measured against it: the pre-part of pair j right behind flow(j) on the flow lane of its parity, where it waits
//          for nothing -- 287-294 frames/s: 1.4 ms of one-workgroup kernels per pair keep that lane's net from the machine.
//          Its keypoint stage and start group alone there (0.2 ms), the homography part left on the depth lane: no gain over
//          the lanes as they are -- the homography part then ends behind the five-point batch (profiles/lanes_chain_ab.txt).
// auto: lanes with 4 .. 7 queues, wide with 8 or more (8 streams), creation order below four.
static inline StreamPlan plan_stream_layout(int ngroups, int nqueues, int choice) {
    StreamPlan p;
    const bool wide_ok = ngroups >= 4, lanes_ok = nqueues >= 4;
    int layout = LAYOUT_CREATION;
    if (choice == LAYOUT_CHOICE_WIDE)
        layout = wide_ok ? LAYOUT_WIDE : LAYOUT_CREATION;
    else if (choice == LAYOUT_CHOICE_LANES)
        layout = lanes_ok ? LAYOUT_LANES : LAYOUT_CREATION;
    else if (nqueues >= 8 && wide_ok)
        layout = LAYOUT_WIDE;
    else if (lanes_ok)
        layout = LAYOUT_LANES;
    p.layout = layout;
    static const int wide[ROLE_COUNT] = {0, 0, 0, 1, 1, 1, 2, 3};
    static const int lanes[ROLE_COUNT] = {3, 3, 3, 2, 2, 2, 0, 1};
    for (int r = 0; r < ROLE_COUNT; ++r) p.lane[r] = layout == LAYOUT_WIDE ? wide[r] : layout == LAYOUT_LANES ? lanes[r] : -1;
    return p;
}

// LANES: four candidates on four different hardware queues, on different pipes as far as the pipes go.  pick[l] = the
// candidate of lane l; false when there are fewer than four queues.
static inline bool pick_lane_candidates(const PoolClasses& c, int pick[4]) {
    const int n = (int)c.group.size();
    int np = 0;
    std::vector<char> queue_used(c.nqueues > 0 ? c.nqueues : 1, 0), pipe_used(c.ngroups > 0 ? c.ngroups : 1, 0);
    for (int pass = 0; pass < 2 && np < 4; ++pass)  // pass 0: a new pipe and a new queue; pass 1: a new queue
        for (int i = 0; i < n && np < 4; ++i) {
            if (queue_used[c.queue_group[i]] || (pass == 0 && pipe_used[c.group[i]])) continue;
            queue_used[c.queue_group[i]] = pipe_used[c.group[i]] = 1;
            pick[np++] = i;
        }
    return np == 4;
}

}  // namespace dfvo
