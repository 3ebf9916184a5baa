// Stand-alone check of the keypoint refinement's host-side pieces, compiled for the host:
//   pipeline_refine_check                 the rules of dfvo_pipeline_set_refine (df-vo_amd/csrc/pipeline_setup.h): the five setters
//                                         played in every order over the combinations of tracking method, pose net, iterative scale
//                                         recovery, depth source and refinement block, against the verdicts written out below from
//                                         the rules; then the edge values of the new range checks
//   pipeline_refine_check <in> <out>      sm::rigid_pose_f32 (df-vo_amd/csrc/np_legacy.h), the PnP refinement's rigid_flow_pose:
//                                         in: int32 n, then n records of 12 float64 (R row-major 3x3, t); out: n x 16 float32
// No HIP.  Built with -fsanitize=address,undefined and run by tests/test_pipeline_refine_cpu.py; exit status 0 = every check holds.
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../df-vo_amd/csrc/np_legacy.h"
#include "../../df-vo_amd/csrc/pipeline_setup.h"

using namespace dfvo;

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
            ++g_failed;                                                      \
        }                                                                    \
    } while (0)

static bool has(const char* msg, const char* word) { return word ? (msg && strstr(msg, word)) : msg == nullptr; }

// the setters as pipeline_options.hip plays them (see pipeline_setup_check.cpp): the argument beside the committed blocks
struct Setup {
    dfvo_pipeline_cfg cfg;
    dfvo_pipeline_opts opts;
    dfvo_pipeline_iter_opts iter;
    dfvo_pipeline_depth_src dsrc;
    dfvo_pipeline_pose_opts pose;
    dfvo_pipeline_refine_opts refine;
};
static const char* const T_KP = "dfvo_pipeline_set_refine: more kp_depth keypoints than the depth-ratio kernel holds in 64 KB of LDS (16384)";
static const char* set_options(Setup& c, const dfvo_pipeline_opts& o) {
    const char* why = options_refusal(c.cfg, o, c.iter, c.pose);
    if (!why) why = options_refine_refusal(o, c.refine);
    if (!why) c.opts = o;
    return why;
}
static const char* set_pose(Setup& c, const dfvo_pipeline_pose_opts& o) {
    const char* why = pose_net_refusal(c.opts, o);
    if (!why) c.pose = o.enable ? o : dfvo_pipeline_pose_opts{};
    return why;
}
static const char* set_iter(Setup& c, const dfvo_pipeline_iter_opts& o) {
    const char* why = o.enable ? iter_opts_refusal(o, c.cfg.scale_min_samples) : nullptr;
    if (!why && o.enable) why = iter_refine_refusal(o, c.refine);
    if (!why) c.iter = o.enable ? o : dfvo_pipeline_iter_opts{};
    return why;
}
static const char* set_dsrc(Setup& c, const dfvo_pipeline_depth_src& d) {
    const char* why = depth_source_refusal(d);
    if (!why) c.dsrc = d.source == DFVO_DEPTH_NET ? dfvo_pipeline_depth_src{} : d;
    return why;
}
static const char* set_refine(Setup& c, const dfvo_pipeline_refine_opts& r) {
    const char* why = refine_opts_refusal(r, c.opts, c.iter);
    if (!why && refine_on(r)) {  // (the launcher's geometry comes here: cells x floor(num_bestN / cells) keypoints at most)
        const int cells = r.num_row * r.num_col;
        if (!refine_kp_count_ok(r, cells * (r.num_bestN / cells))) why = T_KP;
    }
    if (!why) c.refine = refine_on(r) ? r : dfvo_pipeline_refine_opts{};
    return why;
}

enum Step { OPT, POSE, ITER, DSRC, REFINE };
enum Kind { OFF, E, E_SCALE, PNP, ALL, SCALE_ALONE, N_KIND };
struct Combo {
    int tracking, pose_on, iter, external, kind;
};

static Setup fresh() {
    Setup s = {};
    s.cfg.img_h = 192, s.cfg.img_w = 640;
    s.cfg.kp_num_row = 10, s.cfg.kp_num_col = 10, s.cfg.kp_num_bestN = 2000;
    s.cfg.scale_min_samples = 3;
    return s;
}
static dfvo_pipeline_opts opts_of(int tracking) {
    dfvo_pipeline_opts o = {};
    o.tracking_method = tracking, o.kp_sampled_num = 2000;
    o.flow_crop[1] = o.flow_crop[3] = 1.0;
    return o;
}
static dfvo_pipeline_iter_opts iter_of(int on) {
    dfvo_pipeline_iter_opts o = {};
    o.enable = on, o.kp_src = DFVO_ITER_KP_DEPTH;
    o.num_row = 10, o.num_col = 10, o.num_bestN = 2000, o.rigid_flow_thre = 5.0, o.optical_flow_thre = 0.1;
    return o;
}
static dfvo_pipeline_refine_opts refine_of(int kind) {
    dfvo_pipeline_refine_opts r = {};
    if (kind == OFF) return r;
    r.e_enable = kind == E || kind == E_SCALE || kind == ALL;
    r.scale_enable = kind == E_SCALE || kind == ALL || kind == SCALE_ALONE;
    r.pnp_enable = kind == PNP || kind == ALL;
    r.e_score_rigid = 0, r.pnp_score_rigid = 1;
    r.num_row = 10, r.num_col = 10, r.num_bestN = 2000, r.rigid_flow_thre = 5.0, r.optical_flow_thre = 0.1;
    return r;
}

// The verdict of a play by the rules, as a word of the refusal (null: accepted), with what is committed when each setter comes:
//   deep_pose needs the pose net, and the net cannot be taken away under it; the refinement excludes the iterative scale method
//   and deep_pose, whichever setter comes second; its E half needs an E-tracker (not tracking_method PnP); scale_enable needs
//   e_enable.  The first refusal ends the play.
static const char* expected(const Step* order, const Combo& c) {
    int tracking = DFVO_TRACKING_HYBRID;
    bool pose_net = false, iter_on = false, ref_on = false, ref_e = false;
    const bool want_e = c.kind == E || c.kind == E_SCALE || c.kind == ALL;
    for (int k = 0; k < 5; ++k) {
        switch (order[k]) {
        case OPT:
            if (c.tracking == DFVO_TRACKING_DEEP_POSE && !pose_net) return "tracking_method is";
            if (ref_on && c.tracking == DFVO_TRACKING_DEEP_POSE) return "DFVO_TRACKING_DEEP_POSE beside dfvo_pipeline_set_refine";
            if (ref_e && c.tracking == DFVO_TRACKING_PNP) return "DFVO_TRACKING_PNP beside dfvo_pipeline_set_refine's e_enable";
            tracking = c.tracking;
            break;
        case POSE:
            if (!c.pose_on && tracking == DFVO_TRACKING_DEEP_POSE) return "needs the pose net";
            pose_net = c.pose_on;
            break;
        case ITER:
            if (c.iter && ref_on) return "dfvo_pipeline_set_iterative: not beside dfvo_pipeline_set_refine";
            iter_on = c.iter;
            break;
        case DSRC:
            break;
        case REFINE:
            if (c.kind == OFF) break;
            if (c.kind == SCALE_ALONE) return "scale_enable without e_enable";
            if (iter_on) return "dfvo_pipeline_set_refine: not beside dfvo_pipeline_set_iterative";
            if (tracking == DFVO_TRACKING_DEEP_POSE) return "runs no tracker to refine";
            if (want_e && tracking == DFVO_TRACKING_PNP) return "e_enable under tracking_method DFVO_TRACKING_PNP";
            ref_on = true, ref_e = want_e;
            break;
        }
    }
    return nullptr;
}

static void walk_product() {
    int accepted = 0, refused = 0, orders = 0;
    Step order[5] = {OPT, POSE, ITER, DSRC, REFINE};
    do {
        ++orders;
        for (int tracking = 0; tracking < 3; ++tracking)
            for (int pose_on = 0; pose_on < 2; ++pose_on)
                for (int iter = 0; iter < 2; ++iter)
                    for (int external = 0; external < 2; ++external)
                        for (int kind = 0; kind < N_KIND; ++kind) {
                            const Combo c = {tracking, pose_on, iter, external, kind};
                            Setup st = fresh();
                            const char* got = nullptr;
                            for (int k = 0; k < 5 && !got; ++k) {
                                dfvo_pipeline_depth_src d = {};
                                if (external) d.source = DFVO_DEPTH_EXTERNAL, d.scale = 500.0, d.src_h = 376, d.src_w = 1241;
                                if (order[k] == OPT) got = set_options(st, opts_of(tracking));
                                if (order[k] == POSE) got = set_pose(st, dfvo_pipeline_pose_opts{pose_on, 0, 0.05f});
                                if (order[k] == ITER) got = set_iter(st, iter_of(iter));
                                if (order[k] == DSRC) got = set_dsrc(st, d);
                                if (order[k] == REFINE) got = set_refine(st, refine_of(kind));
                            }
                            const char* want = expected(order, c);
                            if (!has(got, want)) {
                                fprintf(stderr, "tracking %d pose %d iter %d external %d kind %d order %d%d%d%d%d:\n  got  %s\n  want %s\n", tracking, pose_on,
                                        iter, external, kind, order[0], order[1], order[2], order[3], order[4], got ? got : "accepted",
                                        want ? want : "accepted");
                                ++g_failed;
                            }
                            ++(want ? refused : accepted);
                            if (!want) {  // an accepted play committed exactly the combination, and never the two methods together
                                const dfvo_pipeline_refine_opts r = refine_of(kind);
                                CHECK(st.opts.tracking_method == tracking && st.pose.enable == pose_on && st.iter.enable == iter);
                                CHECK(st.dsrc.source == external && !memcmp(&st.refine, &r, sizeof(r)));
                                CHECK(!(st.iter.enable && refine_on(st.refine)));
                                CHECK(!(refine_on(st.refine) && st.opts.tracking_method == DFVO_TRACKING_DEEP_POSE));
                                CHECK(!(st.refine.e_enable && st.opts.tracking_method == DFVO_TRACKING_PNP));
                                // an all-zero block switches the refinement off again, after which the iterative method is accepted
                                CHECK(set_refine(st, refine_of(OFF)) == nullptr && !refine_on(st.refine));
                                CHECK(set_iter(st, iter_of(1)) == nullptr);
                            }
                        }
    } while (std::next_permutation(order, order + 5));
    CHECK(orders == 120 && accepted > 0 && refused > 0 && accepted + refused == 120 * 3 * 2 * 2 * 2 * N_KIND);
}

static void edge_values() {
    const double nan = std::nan(""), inf = INFINITY;
    const struct {
        int dfvo_pipeline_refine_opts::*field;
    } flags[] = {{&dfvo_pipeline_refine_opts::e_enable}, {&dfvo_pipeline_refine_opts::scale_enable}, {&dfvo_pipeline_refine_opts::pnp_enable},
                 {&dfvo_pipeline_refine_opts::e_score_rigid}, {&dfvo_pipeline_refine_opts::pnp_score_rigid}};
    for (const auto& f : flags)
        for (int v : {-1, 2}) {
            Setup st = fresh();
            dfvo_pipeline_refine_opts r = refine_of(ALL);
            r.*f.field = v;
            CHECK(has(set_refine(st, r), "the enables are 0 or 1"));
        }
    for (int e_score = 0; e_score < 2; ++e_score)
        for (int p_score = 0; p_score < 2; ++p_score) {
            Setup st = fresh();
            dfvo_pipeline_refine_opts r = refine_of(ALL);
            r.e_score_rigid = e_score, r.pnp_score_rigid = p_score;
            CHECK(set_refine(st, r) == nullptr && st.refine.e_score_rigid == e_score && st.refine.pnp_score_rigid == p_score);
        }
    {  // nothing enabled: the block is all zero, or a mistake
        Setup st = fresh();
        dfvo_pipeline_refine_opts r = refine_of(ALL);
        r.e_enable = r.scale_enable = r.pnp_enable = 0;
        CHECK(has(set_refine(st, r), "nothing enabled"));
        r = {};
        r.optical_flow_thre = 0.1;
        CHECK(has(set_refine(st, r), "nothing enabled"));
        r = {};
        r.rigid_flow_thre = -0.0;  // (compares equal to zero)
        CHECK(set_refine(st, r) == nullptr);
    }
    for (int dim = 0; dim < 3; ++dim)
        for (int v : {-1, 0, 1}) {
            Setup st = fresh();
            dfvo_pipeline_refine_opts r = refine_of(E);
            r.num_row = r.num_col = 1, r.num_bestN = 1;
            (dim == 0 ? r.num_row : dim == 1 ? r.num_col : r.num_bestN) = v;
            CHECK(v >= 1 ? set_refine(st, r) == nullptr : has(set_refine(st, r), "are positive"));
        }
    for (int which = 0; which < 2; ++which) {
        Setup st = fresh();
        dfvo_pipeline_refine_opts r = refine_of(PNP);
        (which ? r.rigid_flow_thre : r.optical_flow_thre) = nan;
        CHECK(has(set_refine(st, r), "a threshold is NaN"));
        (which ? r.rigid_flow_thre : r.optical_flow_thre) = inf;
        CHECK(set_refine(st, r) == nullptr);
        (which ? r.rigid_flow_thre : r.optical_flow_thre) = -inf;
        CHECK(set_refine(st, r) == nullptr);
    }
    // the second scale stage's bound, read with scale_enable only: 128 cells x 129 > 16384 >= 128 x 128
    for (int kind : {E, E_SCALE, PNP, ALL}) {
        Setup st = fresh();
        dfvo_pipeline_refine_opts r = refine_of(kind);
        r.num_row = 8, r.num_col = 16, r.num_bestN = 128 * 129;
        const bool scale = kind == E_SCALE || kind == ALL;
        CHECK(scale ? set_refine(st, r) == T_KP : set_refine(st, r) == nullptr);
        r.num_bestN = 128 * 129 - 1;
        CHECK(set_refine(st, r) == nullptr);
    }
    CHECK(refine_kp_count_ok(refine_of(E_SCALE), 16384) && !refine_kp_count_ok(refine_of(E_SCALE), 16385) && refine_kp_count_ok(refine_of(E), 1 << 30));
    CHECK(refine_all_zero(refine_of(OFF)) && !refine_all_zero(refine_of(PNP)) && !refine_on(refine_of(OFF)) && refine_on(refine_of(SCALE_ALONE)));
}

static int poses(const char* src, const char* dst) {
    FILE* f = fopen(src, "rb");
    if (!f) return 2;
    int32_t n = 0;
    if (fread(&n, sizeof(n), 1, f) != 1 || n < 0) return 2;
    std::vector<double> in((size_t)n * 12);
    if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
    fclose(f);
    std::vector<float> out((size_t)n * 16);
    for (int i = 0; i < n; ++i) sm::rigid_pose_f32(&in[(size_t)i * 12], &in[(size_t)i * 12 + 9], &out[(size_t)i * 16]);
    f = fopen(dst, "wb");
    if (!f) return 2;
    if (fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) return 2;
    fclose(f);
    printf("refine_pose: %d poses\n", (int)n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return poses(argv[1], argv[2]);
    if (argc != 1) return 2;
    walk_product();
    edge_values();
    if (g_failed) return 1;
    printf("pipeline_refine: ok\n");
    return 0;
}
