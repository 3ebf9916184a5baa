// Device buffers, small state blocks and enqueue functions of the tracker stages around the RANSAC solvers:
//   solver_kp.hip               keypoint selection (local_bestN, bestN_flow_kp, rigid-flow and sampled keypoints)
//   solver_rng.hip              numpy's MT19937 seeding and shuffle on the device
//   solver_pose2d2d.hip         EssTracker.compute_pose_2d2d: GRIC, the repeated shuffled five-point RANSAC, bookkeeping
//   solver_scale.hip            depth-ratio scale recovery (find_scale_from_depth) and the iterative loop around it as one enqueue
//   solver_trajectory.hip       update_global_pose over a gathered sequence
//   solver_buffers.hip          lifetime of every buffer set declared here and in solver.h (host only)
// Sequential semantics that leak into the results (argpartition order, python-loop summation order, the global
// np.random stream, last-writer-wins scatter) are kept by giving each sequential chain to one lane and spreading
// independent chains over lanes / workgroups.  All solver_*.hip units are built with -ffp-contract=off.
#pragma once
#include <stddef.h>

#include "solver.h"

namespace dfvo {

struct PoseState {
    int n;
    int best_cnt;
    int num_valid;
    int have_best;
    int major_valid;
    int cheirality;
    int valid_case;
    int h_found;
    double h_gric;
    double best_E[9];
    double R[9];
    double t[3];
    int rep_cnt[8];
    int rep_valid[8];
    double rep_gric[8];
};

struct ScaleResult {
    double scale;
    int n_valid;
    int n_trials;
    int n_inliers;
    int status;  // 1 ok, 0 too few valid points (scale -1), -1 no consensus set (sklearn raises)
    int best_is_a;
};

struct PoseConfig {
    double fx, cx, cy;
    double reproj_thre;
    int repeat;
    int max_iters;
    double KinvT[9], Kinv[9];
    int validity = 0;           // e_tracker.validity.method: 0 GRIC, 1 flow, 2 homo_ratio (E_tracker.py:182-194, 243-250)
    double validity_thre = 0;   // flow: mean keypoint displacement [px] above which the pair is tracked at all;
                                // homo_ratio: a repeat is valid while H inliers / (H + E inliers) stays below it
};

struct ScaleConfig {
    double cx, cy, fx, fy;
    int min_samples, max_trials;
    double stop_prob, thre;
    int method = 0;  // scale_recovery.ransac.method: 0 depth_ratio, 1 abs_diff (E_tracker.py:626-635)
};

constexpr int MAX_REP = 8;
// TrackerBuffers::mt_state holds the RandomState (624 key words + position) followed by MAX_REP + 1 snapshots of it
constexpr int MT_SNAP_STRIDE = 640;
inline uint32_t* mt_snapshots(uint32_t* mt_state) { return mt_state + MT_SNAP_STRIDE; }
// TrackerBuffers::kp_total, ints: small device counters of the stages
constexpr int KP_CNT_BLOCKS = 64;     // counting blocks of k_kp_cell (solver_kp.hip)
constexpr int KPT_GOOD = 0;           // k_kp_gather's count when it is given no partial counts ([1..3] unused)
constexpr int KPT_SCALE_VALID = 4;    // number of valid depth ratios of the scale stage
constexpr int KPT_FLOW_GATE = 5;      // "flow" validity: [5] the keypoint count the shuffles see, [6] valid_case ([7] unused)
constexpr int KPT_CELL_PARTIAL = 8;   // [8..71] the counting blocks' partial counts
constexpr int KPT_E_RNG = KPT_CELL_PARTIAL + KP_CNT_BLOCKS;  // [72..73] the five-point sampler's 64-bit state behind its prefetched subsets
constexpr int KPT_SIZE = KPT_E_RNG + 2;
// TrackerBuffers::small, doubles
constexpr int SMALL_KINVT = 0;    // [0..8] K^-T
constexpr int SMALL_KINV = 9;     // [9..17] K^-1
constexpr int SMALL_H_GRIC = 18;  // GRIC of the homography ("flow" validity: the mean keypoint displacement)
constexpr int SMALL_E_GRIC = 19;  // [19 .. 19 + MAX_REP) GRIC of each repeat's E ("flow" validity: its cheirality count)
constexpr int SMALL_SIZE = 128;
constexpr int NUM_REP_STREAMS = 4;  // side streams created per tracker; two are used (see TrackerBuffers::init)
static inline int rep_stream_count() { return NUM_REP_STREAMS; }

// PnpTracker.compute_pose_3d2d (solver_pnp.hip)
struct PnpConfig {
    double fx, fy, cx, cy;
    double inv_K[9];  // Intrinsics.inv_mat, row-major
    double min_depth, max_depth;
    int repeat;  // number of shuffled solvePnPRansac runs (cfg.pnp_tracker.ransac.repeat, or 3)
    int iters;   // iterationsCount
    double reproj_thre;
};
struct PnpRepOut {
    int flag;       // solvePnPRansac returned true
    int n_inliers;  // inlier.shape[0]
    int status;     // 1 ok, 0 no model, -2 planar initialisation branch (not implemented)
    int lm_iters;
    double rvec[3], tvec[3];
};
struct PnpResult {
    int found;         // len(best_rt) != 0
    int best_inliers;
    int n_filtered;    // keypoints that survived the in-image / depth-range masks
    int status;        // 0, or -2 when a repeat met the planar branch
    double rvec[3], tvec[3];
    double R[9];       // cv2.Rodrigues(rvec)
};
struct PnpBuffers {
    int cap = 0, iters_cap = 0;
    DevArr<int> info;
    DevArr<double> fk1, fk2, xyz;
    DevArr<int> perm;
    DevArr<float> obj, img;
    DevArr<RansacState> state;
    DevArr<int> idx;
    DevArr<double> models;
    DevArr<int> nmodels, counts;
    DevArr<uint8_t> mask, keep;  // keep[i]: input keypoint i survived the filters
    DevArr<float> pts5;
    DevArr<PnpRepOut> rep_out;
    DevArr<PnpResult> result;
    int ensure(int n, int iters);
    void release();
};

struct TrackerBuffers {
    RansacWorkspace ws_h, ws_e;          // ws_e: stand-alone findEssentialMat / recoverPose calls
    RansacWorkspace ws_rep[MAX_REP];     // one workspace per repeated findEssentialMat (run concurrently)
    hipStream_t s_rep[MAX_REP] = {};
    int n_rep_owned = 0;  // s_rep[0 .. n_rep_owned) are distinct streams this object destroys
    hipEvent_t ev_rep[MAX_REP] = {};
    hipEvent_t ev_fork = nullptr, ev_start = nullptr, ev_h = nullptr;
    // DFVO_TRACK_TRACE: device-side timestamps of the RNG-ordered chain (start of the shuffles, end of the five-point batch,
    // end of recoverPose, end of the scale stage), and of the homography half on its stream ([4] beside ev_start, [5] beside
    // ev_h; ev_t_half: recorded for the pair at hand); null unless tracing
    static constexpr int N_EV_T = 6;
    hipEvent_t ev_t[N_EV_T] = {};
    bool ev_t_half = false;
    // Stage timestamps for the reference's Timer sub-keys (E_tracker.py:197-296,597-638), created on demand by
    // enable_stage_timing() (the drop-in mirrors' tracker; the fused pipeline leaves them null).  Marks: 0 start of the
    // homography part | 1 findHomography done | 2 GRIC-H done | 3 first shuffle | 4 five-point batch done | 5 GRIC-E done |
    // 6 validity bookkeeping done | 7 recoverPose done | 8 scale stage start | 9 triangulation + depth ratios done |
    // 10 scale RANSAC done.  seg_mask: the marks recorded since the last homography part / scale stage began.
    static constexpr int N_SEG = 11;
    hipEvent_t ev_seg[N_SEG] = {};
    unsigned seg_mask = 0;
    int enable_stage_timing();
    int mark(int i, hipStream_t s);
    bool shared = false;  // streams / events / RandomState borrowed from another TrackerBuffers (see share_from)
    uint32_t* mt_state = nullptr;  // numpy RandomState: key[624], pos (mt_own's, or the first set's when `shared`)
    DevArr<uint32_t> mt_own;
    DevArr<int> kp_info;           // [n, good_kp_found, regions]
    DevArr<int> kp_total;          // [KPT_SIZE], layout: KPT_* above
    int e_pre_iters = 0;  // > 0: enqueue_pose_h_part drew the five-point sampler's first chunk ahead, for this iteration budget
    DevArr<PoseState> pose;
    DevArr<double> small;          // [SMALL_SIZE], layout: SMALL_* above
    double h_small[18] = {};       // host copy of the 18 intrinsics doubles held in `small` (uploaded only when they change)
    bool small_valid = false;
    DevArr<ScaleResult> scale_out;
    // grown on demand by the stages that use them
    DevArr<int> winner;            // per pixel (the scale stage)
    DevArr<unsigned short> lidx;   // cells x pixels of a cell (local_bestN)
    DevArr<float> ratio_map;       // flow_diff / |flow| per pixel (local_bestN score_method 'flow_ratio')
    int grow_winner(int H, int W) { return winner.grow((size_t)H * W); }
    int grow_lidx(int cells, int cap) { return lidx.grow((size_t)cells * cap); }
    int grow_ratio_map(int H, int W) { return ratio_map.grow((size_t)H * W); }
    // keypoint-sized buffers
    DevArr<double> kp_ref, kp_cur, pa, pb, res, z2, ratios;
    DevArr<int> perm, cell_count, cell_sel, pix, scratch;
    DevArr<uint8_t> best_inliers, inl_a, inl_b;
    int kp_cap = 0, sel_cap = 0;
    // rep0 / rep1: side streams chosen by the caller (the fused pipeline hands out streams by dispatch pipe); null = create.
    // They may be the same stream.  borrowed: the caller keeps and destroys them -- they may then also be the stream the
    // chain itself is enqueued on (the lane layout of the fused pipeline: one stream per hardware queue)
    int init(hipStream_t rep0 = nullptr, hipStream_t rep1 = nullptr, bool borrowed = false);
    // replaces the side streams of an idle, non-shared buffer set by two streams the caller chose by dispatch pipe (the frame
    // session, session.hip); this object owns and destroys them from then on, unless they are `borrowed` (see init).  The
    // two may be one stream
    int rebind_streams(hipStream_t rep0, hipStream_t rep1, bool borrowed = false);
    // second and further buffer sets of the fused pipeline: own keypoint / RANSAC workspaces, but the numpy
    // RandomState and the (serialised anyway) RNG-side streams and events of `first`
    int init_shared(const TrackerBuffers& first);
    int ensure_kp(int cap, int cells, int n_best);
    void release_kp();
    void release();

private:
    int init_own();  // the buffers and events every set owns, shared or not
};

// score_method: 0 'flow' (the consistency map itself), 1 'flow_ratio' (map / |flow|), kp_selection.py:137-141,151-156
// d_depth_diff (kp_selection.depth_consistency, :145-148; null: off): a cell's candidates must also lie under depth_thre in it
int enqueue_local_bestn(TrackerBuffers& tb, const float* d_flow, const float* d_diff, int H, int W, int num_row,
                        int num_col, int num_bestN, float thre, hipStream_t s, int score_method = 0,
                        const float* d_depth_diff = nullptr, float depth_thre = 0.f);
// bestN_flow_kp (kp_selection.py:33-71): whole-image argpartition
struct BestNBuffers {
    DevArr<float> key_base;      // keys carried along with the index array, with slack on either side
    DevArr<int> tosort, map, Lpos, Rpos, count;  // count[1] = result size
    DevArr<double> kp;           // [kp1 | kp2], N x 2 doubles each
    size_t cap = 0;              // pixels the six selection arrays hold (kp holds kp.n / 4 picks)
    int ensure(size_t px, int N);  // allocates (hipMalloc / hipFree: not for a per-pair path once the sizes are final)
    void release();
};
// d_kp1 / d_kp2 / d_info (all three or none): the picks go straight to these [N][2] arrays instead of bb.kp, and d_info
// receives a tracker's kp_info triple [n, good_kp_found, 0] (n = 0 and good_kp_found = 0 where numpy would raise)
int enqueue_bestn_flow_kp(BestNBuffers& bb, const float* d_flow, const float* d_diff, int H, int W, int N, hipStream_t s,
                          double* d_kp1 = nullptr, double* d_kp2 = nullptr, int* d_info = nullptr);

// rigid-flow keypoints (E_tracker.py:645-705 kp_selection_good_depth)
struct RigidKpConfig {
    int num_row, num_col, num_bestN;
    float rigid_thre, opt_thre;
    int score_rigid;              // 1: score = rigid-flow distance, 0: forward-backward distance
    float K[9], Kinv[9], T[16];   // float32 intrinsics, their inverse, the ref -> cur motion (row-major)
};
// scale_recovery_iterative (E_tracker.py:509-569) as one enqueue: the loop's state on the device.  Every kernel of a round
// reads `done` as its skip flag, so the rounds behind the last executed one draw nothing and overwrite nothing.
constexpr int ITER_ROUNDS = 5;
constexpr int ITER_RUNNING = 0;       // status
constexpr int ITER_EMPTY = 1;         // opt_rigid_flow_kp selected nothing (the reference's assertion) in round n_iter
constexpr int ITER_NO_CONSENSUS = 2;  // sklearn's "could not find a valid consensus set" in round n_iter
constexpr int ITER_NOT_RUN = 3;       // the gate was closed (IterDevice::gate: ||t|| == 0, dfvo.py:182): no round, no draw, no write
struct IterCtl {
    double scale;   // in: prev_scale; out: the last round's scale
    int done;       // the skip flag of every later kernel
    int n_iter;     // rounds completed (find_scale_from_depth returned)
    int status;     // ITER_*
    int sel_round;  // last round whose selection was not empty (-1: none); its distance map is rdiff_of(sel_round)
    double scale_in[ITER_ROUNDS], scale_out[ITER_ROUNDS];
    int n_kp[ITER_ROUNDS];  // uniform keypoints of each round (-1: round not run)
    int pad;
};
struct RigidKpBuffers {
    DevArr<float> depth32, rdiff, mats;  // depth32: one float per pixel; rdiff: two maps (iterative rounds alternate)
    DevArr<IterCtl> ctl;
    float* rdiff_of(int round, int H, int W) const { return rdiff.p + (size_t)(round & 1) * H * W; }
    DevArr<int> cell_count, cell_sel, cell_sel_uni, info, zero;
    DevArr<unsigned short> lidx;
    DevArr<double> kp;            // [4][sel_cap][2]: kp1 best, kp2 best, kp1 uniform, kp2 uniform
    int sel_cap = 0;
    int ensure(int H, int W, int cells, int n_best, int cap);
    void release();
};
int enqueue_rigid_flow_kp(RigidKpBuffers& rb, const float* d_flow, const float* d_odiff, const float* d_depth32, int H,
                          int W, const RigidKpConfig& cfg, const float* d_rdiff_override, hipStream_t s);
// one round of the iterative loop: rb.mats already holds Kinv | T | K on the device (k_iter_begin), the distance map goes
// to d_rdiff_out, only the uniform set is selected (rb.kp + 2 * sel_cap * 2, count in rb.info[4]); nothing runs when *d_skip
int enqueue_rigid_flow_kp_round(RigidKpBuffers& rb, const float* d_flow, const float* d_odiff, const float* d_depth32, int H,
                                int W, const RigidKpConfig& cfg, float* d_rdiff_out, const int* d_skip, hipStream_t s);
// launch geometry of the rigid-flow keypoint kernels for this size (the refusals shared by every entry point)
int rigid_flow_kp_geometry(int H, int W, const RigidKpConfig& cfg, int* cells, int* n_best, int* cap, size_t* lds, int* par);
// d_info (optional): receives a tracker's kp_info triple [n, 1, 0] (keypoint_sampler.py:96: good_kp_found stays True)
int enqueue_kp_sampled(const float* d_flow, int H, int W, int y0, int y1, int x0, int x1, const int* d_idx, int n,
                       double* d_kp1, double* d_kp2, hipStream_t s, int* d_info = nullptr);
// generate_kp_samples (keypoint_sampler.py:52-74): np.linspace(0, (y1 - y0) * (x1 - x0) - 1, n, dtype=int) into h_idx[n]
void generate_kp_samples(int y0, int y1, int x0, int x1, int n, int* h_idx);
int enqueue_mt_seed(TrackerBuffers& tb, uint32_t seed, hipStream_t s);
// d_T21 (optional): 16 doubles that receive the inverse of the accepted pose (input of the scale stage)
int enqueue_compute_pose_2d2d(TrackerBuffers& tb, int n_host, const PoseConfig& cfg, hipStream_t s,
                              double* d_T21 = nullptr);
// update_global_pose over a gathered sequence in one launch (rows [n][17] -> poses [n+1][16]); d_bad[0] = first status-2 row or -1
int enqueue_compose_trajectory(const double* d_rows, int n, const double* d_first, double* d_poses, int* d_bad, hipStream_t s);
int enqueue_pose_h_part(TrackerBuffers& tb, int n_bound, const PoseConfig& cfg, hipStream_t sh);
// d_E_pose (optional): 16 doubles that receive the accepted pose itself, [R t; 0 0 0 1] (cur -> ref, unit translation: the
// E_pose of scale_recovery_iterative), from a one-lane kernel behind recoverPose
int enqueue_pose_e_part(TrackerBuffers& tb, int n_host, const PoseConfig& cfg, hipStream_t s, double* d_T21,
                        double* d_E_pose = nullptr);
// snap (optional): mt_snapshots(tb.mt_state) -- the state before the first and behind every shuffle
int enqueue_mt_shuffle(uint32_t* mt_state, const int* d_n, int n_host, int repeat, int perm_stride, int* perm,
                       hipStream_t s, uint32_t* snap = nullptr);
// depth_per_kp: d_depth holds, per keypoint, the depth map's value at that keypoint's kp1 pixel (truncated, negative indices
// wrapped as numpy does) -- [n_host] doubles instead of the H x W map
int enqueue_compute_pose_3d2d(PnpBuffers& pb, uint32_t* mt_state, const double* d_kp1, const double* d_kp2,
                              const int* d_n, int n_host, const double* d_depth, int H, int W, const PnpConfig& cfg,
                              hipStream_t s, bool depth_per_kp = false);
// d_gate (optional): device PoseState whose zero translation suppresses the whole stage (no RandomState draws)
// depth_per_kp: d_depth holds, per keypoint, the depth map's value at that keypoint's (truncated) kp2 pixel -- [n_host]
// doubles instead of the H x W map (only those pixels are ever read)
int enqueue_find_scale(TrackerBuffers& tb, int n_host, const double* d_T21, const double* d_depth, int H, int W,
                       const ScaleConfig& cfg, hipStream_t s, const PoseState* d_gate = nullptr, bool prepared = false,
                       bool depth_per_kp = false);
int enqueue_scale_prepare(TrackerBuffers& tb, int H, int W);
// EssTracker.scale_recovery_iterative, all ITER_ROUNDS rounds enqueued back to back on `s` with no host wait between them.
// d_E_pose: 16 doubles, cur -> ref with unit translation; d_T21: 16 doubles, its inverse (what find_scale_from_depth takes);
// cfg.T is not read.  kp_src 0 "kp_depth": the scale of a round is taken from that round's uniform keypoints; 1 "kp_best":
// from tb.kp_ref / tb.kp_cur (n_kp_best of them).  rb.ctl holds the outcome; the last selected round's uniform keypoints stay
// in rb.kp, its distance map in rb.rdiff_of(ctl.sel_round).  Consumes tb.mt_state.
// k_scale_ratios keeps one int per keypoint in dynamic LDS: at most ITER_MAX_KP keypoints (64 KB, the size a kernel gets
// without asking for more).
constexpr int ITER_MAX_KP = 16384;
// dev (the fused pipeline): the loop starts and ends on the device.  prev_scale: a device double read by the loop's first
// kernel in place of the host value and written back behind the last round when at least one round completed (self.prev_scale,
// E_tracker.py:559; the scale -1 included); gate: the E-tracker's PoseState -- a zero translation ends the call in its first
// kernel with ITER_NOT_RUN, and every later kernel returns through the skip pointer.
struct IterDevice {
    double* prev_scale = nullptr;
    const PoseState* gate = nullptr;
};
int enqueue_scale_recovery_iterative(TrackerBuffers& tb, RigidKpBuffers& rb, const float* d_flow, const float* d_odiff,
                                     const float* d_depth32_ref, const double* d_depth64_cur, int H, int W,
                                     const RigidKpConfig& cfg, const ScaleConfig& scfg, const double* d_E_pose,
                                     const double* d_T21, double prev_scale, int kp_src, int n_kp_best, hipStream_t s,
                                     const IterDevice* dev = nullptr);
// The trackers' iterative keypoint refinement (dfvo.py:194-222, 236-244; solver_refine.hip): the device-side hand-over between a
// first pass and the second pass on kp_depth.  Each builds Kinv | T | K in rb.mats from the first pass's device results and
// sets the skip flag of the selection behind it, rb.ctl->done (status ITER_NOT_RUN when set); a skipped hand-over writes
// d_kp_info2 = [0, 0, 0], the second pass's keypoint triple.
//   e_mats:   T = inv([R | t * scale]) (scale -1: inv([R | 0])) of the E-tracker's pose; skipped when ||t|| == 0
//   pnp_mats: T = [Rodrigues(r) | t] of the PnP tracker's result, the identity when no repeat found a model; never skipped
int enqueue_refine_e_mats(RigidKpBuffers& rb, const PoseState* d_pose, const ScaleResult* d_scale, const RigidKpConfig& cfg,
                          int* d_kp_info2, hipStream_t s);
int enqueue_refine_pnp_mats(RigidKpBuffers& rb, const PnpResult* d_pnp, const RigidKpConfig& cfg, int* d_kp_info2, hipStream_t s);
// enqueue_rigid_flow_kp with the matrices already in rb.mats and a device skip flag (null: none): the distance map goes to
// rb.rdiff, the best set and its kp_info triple [n, 1, regions] to d_kp1 / d_kp2 / d_info (the second pass's buffers, at least
// cells * n_best keypoints), the uniform set to rb.kp as before.  rb is ensured by the caller: nothing allocates here.
int enqueue_rigid_flow_kp_dev(RigidKpBuffers& rb, const float* d_flow, const float* d_odiff, const float* d_depth32, int H, int W,
                              const RigidKpConfig& cfg, const int* d_skip, double* d_kp1, double* d_kp2, int* d_info, hipStream_t s);
// the bookkeeping of dfvo.py:206-221 behind the second E pass (and, scale_ran, the second scale stage), one lane
struct RefineFinal {
    double R[9], t[3];  // the second pass's
    double scale;       // the last scale assigned (pass one's, or the second stage's when it ran)
    double scale2;      // the second stage's result (0: it did not run)
    int t2_zero;        // the second pass was rejected
    int scale_ran;
    int needs_pnp;      // dfvo.py:227
    int pad;
};
int enqueue_refine_final(const PoseState* d_pose1, const ScaleResult* d_scale1, const PoseState* d_pose2, const ScaleResult* d_scale2,
                         int scale_enable, RefineFinal* d_out, hipStream_t s);

int enqueue_ransac_regressor(TrackerBuffers& tb, int n, bool y_is_ones, const ScaleConfig& cfg, hipStream_t s);
int set_sklearn_compat(const char* version);  // "0.20" (the reference's pin, default) | "0.22" and later

}  // namespace dfvo
