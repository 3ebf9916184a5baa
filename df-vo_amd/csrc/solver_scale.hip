// Depth-ratio scale recovery.  Reference call sites (paths relative to /root/reference):
//   libs/tracker/E_tracker.py:571-643             find_scale_from_depth (+ libs/geometry/ops_3d.py:15-67)
//   sklearn RANSACRegressor.fit (third party)     subset draws from the global numpy RandomState
//   libs/tracker/E_tracker.py:509-569             scale_recovery_iterative (enqueue_scale_recovery_iterative, at the end)
// See tracker.h on sequential semantics.  Built with -ffp-contract=off.
#include <atomic>
#include <cstdio>  // sscanf

#include "np_legacy.h"    // sm::Mt19937, sm::mt_sample_without_replacement
#include "ransac_dev.h"   // wave_sum, wave_sum_d
#include "solver_math.h"  // sm::triangulate_point
#include "tracker.h"

namespace dfvo {

// per keypoint: normalise, triangulate with [I|0] / T_21, X2 = T_21[:3] @ (X / X[3]); target pixel of kp2
__global__ void k_scale_triangulate(const int* __restrict__ n_ptr, const double* __restrict__ kp1,
                                    const double* __restrict__ kp2, const double* __restrict__ T21, double cx, double cy,
                                    double fx, double fy, int H, int W, double* __restrict__ z2,
                                    int* __restrict__ pix, int* __restrict__ winner, const int* __restrict__ skip) {
    if (skip && *skip) return;  // (the iterative scale loop's rounds behind its last one)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *n_ptr) return;
    const double P1[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    double P2[12];
    for (int k = 0; k < 12; k++) P2[k] = T21[k];
    const double x1 = (kp1[i * 2] - cx) / fx, y1 = (kp1[i * 2 + 1] - cy) / fy;
    const double x2 = (kp2[i * 2] - cx) / fx, y2 = (kp2[i * 2 + 1] - cy) / fy;
    double X[4];
    sm::triangulate_point(P1, P2, x1, y1, x2, y2, X);
    const double w = X[3];
    const double Xn[4] = {X[0] / w, X[1] / w, X[2] / w, X[3] / w};
    double z = 0;
    z = P2[8] * Xn[0] + P2[9] * Xn[1] + P2[10] * Xn[2] + P2[11] * Xn[3];
    z2[i] = z;
    // kp.astype(np.int): truncation toward zero
    const double kx = kp2[i * 2], ky = kp2[i * 2 + 1];
    const int ix = (int)kx, iy = (int)ky;
    int p = -1;
    if (ix >= 0 && ix < W && iy >= 0 && iy < H && kx == kx && ky == ky) p = iy * W + ix;
    pix[i] = p;
    if (p >= 0) atomicMax(&winner[p], i);  // numpy fancy assignment: the last index wins
}

// ordered list of depth ratios: pixels (row-major) whose winning keypoint has tri > 0 and CNN depth > 0
__global__ __launch_bounds__(256) void k_scale_ratios(const int* __restrict__ n_ptr, const double* __restrict__ z2,
                                                       const int* __restrict__ pix, const int* __restrict__ winner,
                                                       const double* __restrict__ depth, double* __restrict__ ratios,
                                                       int* __restrict__ n_valid, double* __restrict__ tri_list,
                                                       double* __restrict__ pred_list, int depth_per_kp,
                                                       const int* __restrict__ skip) {
    // single block: n <= a few thousand.  rank = number of valid entries with a smaller pixel index.
    // depth_per_kp: `depth` holds the depth map's value at keypoint i's pixel, [n], instead of the map (the only pixels read)
    extern __shared__ int s_pix[];
    if (skip && *skip) return;
    const int n = *n_ptr;
    const int t = threadIdx.x;
    for (int i = t; i < n; i += blockDim.x) {
        const int p = pix[i];
        bool ok = p >= 0 && winner[p] == i;
        if (ok) {
            double tri = z2[i];
            if (tri < 0) tri = 0;  // depth2_tri[depth2_tri < 0] = 0 (NaN stays NaN and fails > 0)
            ok = (tri > 0) && (depth[depth_per_kp ? i : p] > 0);
        }
        s_pix[i] = ok ? p : -1;
    }
    __syncthreads();
    int local = 0;
    for (int i = t; i < n; i += blockDim.x) {
        const int p = s_pix[i];
        if (p < 0) continue;
        int rank = 0;
        for (int j = 0; j < n; j++) rank += (s_pix[j] >= 0 && s_pix[j] < p) ? 1 : 0;
        const double dp = depth[depth_per_kp ? i : p];
        ratios[rank] = z2[i] / dp;
        if (tri_list) {  // ransac.method 'abs_diff': the regression runs on the two depths themselves
            tri_list[rank] = z2[i];
            pred_list[rank] = dp;
        }
        local++;
    }
    const int s = wave_sum(local);
    if ((t & 63) == 0 && s) atomicAdd(n_valid, s);
}

// sklearn RANSACRegressor(LinearRegression(fit_intercept=False), min_samples, max_trials, stop_probability,
// residual_threshold).fit(ratio.reshape(-1,1), ones) -> estimator_.coef_[0,0]; one 256-thread block.
// yv != nullptr (ransac.method 'abs_diff', E_tracker.py:631-635): .fit(depth_tri, depth_pred) -- the same loop with a
// general target: least squares through the origin sum(xy)/sum(xx), residual |y - x coef|, and the tie-break score is
// the real r2_score of the inlier set (1 - ss_res / ss_tot; constant target: 1 when ss_res == 0, else 0).
__global__ __launch_bounds__(256) void k_scale_ransac(uint32_t* __restrict__ mt_state, const double* __restrict__ x,
                                                       const double* __restrict__ yv, const int* __restrict__ n_valid, int min_valid, int min_samples,
                                                       int max_trials, double stop_prob, double thr,
                                                       uint8_t* __restrict__ inl_a, uint8_t* __restrict__ inl_b,
                                                       int* __restrict__ scratch, ScaleResult* __restrict__ out,
                                                       const PoseState* __restrict__ gate, int r2_nan_below_two,
                                                       const int* __restrict__ skip) {
    __shared__ sm::Mt19937 s;
    __shared__ double s_coef;
    __shared__ int s_cnt[4], s_nz[4];
    __shared__ double s_red[3][4];
    __shared__ int s_ctl;  // 0 continue, 1 stop
    __shared__ int s_best_is_a;
    if (skip && *skip) return;  // before the RandomState is read: a skipped round draws nothing
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = *n_valid;
    // fused pipeline: scale recovery only runs when ||t|| != 0 (dfvo.py:198); a rejected E-tracker pose must not
    // draw from the numpy stream
    const bool gated = gate && gate->t[0] == 0 && gate->t[1] == 0 && gate->t[2] == 0;
    if (gated || !(n > min_valid)) {  // valid_mask2.sum() > 10
        if (t == 0) {
            out->scale = -1.0;
            out->n_valid = n;
            out->n_trials = 0;
            out->n_inliers = 0;
            out->status = 0;
        }
        return;
    }
    for (int i = t; i < 624; i += 256) s.key[i] = mt_state[i];
    if (t == 0) s.pos = (int)mt_state[624];
    __syncthreads();
    int n_inliers_best = 1, n_trials = 0, trials_cap = max_trials;
    double score_best = -INFINITY;
    bool have_best = false;
    int best_is_a = 0;
    for (;;) {
        if (!(n_trials < trials_cap)) break;
        n_trials++;
        if (t == 0) {
            int idx[8];
            sm::mt_sample_without_replacement(s, n, min_samples, idx, scratch);
            // LinearRegression(fit_intercept=False) on (x_subset, ones): least squares through the origin
            double sx = 0, sxx = 0;
            for (int k = 0; k < min_samples; k++) {
                sx += x[idx[k]] * (yv ? yv[idx[k]] : 1.0);
                sxx += x[idx[k]] * x[idx[k]];
            }
            s_coef = sx / sxx;
        }
        __syncthreads();
        const double coef = s_coef;
        uint8_t* cur = best_is_a ? inl_b : inl_a;  // write the candidate mask into the non-best buffer
        int c = 0, nz = 0;
        double sy = 0;
        for (int i = t; i < n; i += 256) {
            const double pred = x[i] * coef;
            const double yi = yv ? yv[i] : 1.0;
            const double r = fabs(yi - pred);
            const int f = r <= thr ? 1 : 0;
            cur[i] = (uint8_t)f;
            c += f;
            nz += (f && (yi - pred) != 0.0) ? 1 : 0;  // r2_score numerator != 0 on the inlier set
            if (f) sy += yi;
        }
        c = wave_sum(c);
        nz = wave_sum(nz);
        if (yv) sy = wave_sum_d(sy);
        if (lane == 0) {
            s_cnt[wave] = c;
            s_nz[wave] = nz;
            s_red[0][wave] = sy;
        }
        __syncthreads();
        const int n_in = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        const int nzs = s_nz[0] + s_nz[1] + s_nz[2] + s_nz[3];
        const double mean_y = (s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3]) / (double)n_in;
        __syncthreads();
        if (n_in < n_inliers_best) continue;  // n_skips_no_inliers_
        // r2_score with constant y_true: 1.0 when the residual sum is zero, else 0.0
        double score = nzs == 0 ? 1.0 : 0.0;
        if (yv) {
            double res = 0, tot = 0;
            for (int i = t; i < n; i += 256)
                if (cur[i]) {
                    const double d = yv[i] - x[i] * coef, e = yv[i] - mean_y;
                    res += d * d;
                    tot += e * e;
                }
            res = wave_sum_d(res);
            tot = wave_sum_d(tot);
            if (lane == 0) {
                s_red[1][wave] = res;
                s_red[2][wave] = tot;
            }
            __syncthreads();
            res = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
            tot = s_red[2][0] + s_red[2][1] + s_red[2][2] + s_red[2][3];
            __syncthreads();
            if (tot != 0.0) score = 1.0 - res / tot;  // else: the constant-target rule above (force_finite)
        }
        // sklearn >= 0.22: r2_score of fewer than two samples is nan, which loses no comparison below.  scikit-learn 0.20.3
        // (the reference's pin, envs/requirement.yml:233) has no such rule: one sample is a constant target, scored 1.0 /
        // 0.0 by the rule above.  dfvo_set_sklearn_compat selects (default: the reference's pin).
        if (r2_nan_below_two && n_in < 2) score = NAN;
        if (n_in == n_inliers_best && score < score_best) continue;
        n_inliers_best = n_in;
        score_best = score;
        have_best = true;
        best_is_a = best_is_a ? 0 : 1;  // the buffer just written becomes the best
        // _dynamic_max_trials
        {
            const double eps = 2.220446049250313e-16;
            const double ratio = (double)n_in / (double)n;
            double nom = 1 - stop_prob;
            nom = nom > eps ? nom : eps;
            double denom = 1 - pow(ratio, (double)min_samples);
            denom = denom > eps ? denom : eps;
            double dyn;
            if (nom == 1)
                dyn = 0;
            else if (denom == 1)
                dyn = INFINITY;
            else
                dyn = fabs(ceil(log(nom) / log(denom)));
            if (dyn < (double)trials_cap) trials_cap = (int)dyn;
        }
    }
    // final fit on the best inliers (in index order)
    if (t == 0) {
        double scale = -1.0;
        int status = 0;
        if (have_best) {
            const uint8_t* best = best_is_a ? inl_a : inl_b;
            double sx = 0, sxx = 0;
            for (int i = 0; i < n; i++)
                if (best[i]) {
                    sx += x[i] * (yv ? yv[i] : 1.0);
                    sxx += x[i] * x[i];
                }
            scale = sx / sxx;
            status = 1;
        } else {
            status = -1;  // sklearn raises ValueError: no valid consensus set
        }
        out->scale = scale;
        out->n_valid = n;
        out->n_trials = n_trials;
        out->n_inliers = have_best ? n_inliers_best : 0;
        out->status = status;
        out->best_is_a = best_is_a;
    }
    __syncthreads();
    for (int i = t; i < 624; i += 256) mt_state[i] = s.key[i];
    if (t == 0) mt_state[624] = (uint32_t)s.pos;
    (void)s_ctl;
    (void)s_best_is_a;
}

// find_scale_from_depth on tb.kp_ref (kp1) / tb.kp_cur (kp2); d_T21: 16 doubles; d_depth: H x W doubles
// clears the scatter map and the ratio counter of the scale stage on a side stream (tb.s_rep[1]) and records
// tb.ev_rep[1]; enqueue_find_scale(prepared = true) then only waits for that event, so the two fills leave the
// solver's chain of dependent launches
int enqueue_scale_prepare(TrackerBuffers& tb, int H, int W) {
    if (int rc = tb.grow_winner(H, W)) return rc;
    hipStream_t side = tb.s_rep[1];
    DFVO_HIP_CHECK(hipMemsetAsync(tb.winner, 0xff, sizeof(int) * (size_t)H * W, side));
    DFVO_HIP_CHECK(hipMemsetAsync(tb.kp_total + KPT_SCALE_VALID, 0, sizeof(int), side));
    DFVO_HIP_CHECK(hipEventRecord(tb.ev_rep[1], side));
    return DFVO_OK;
}

// which scikit-learn the depth-ratio RANSAC reproduces where the versions differ (dfvo_set_sklearn_compat)
std::atomic<int> g_sklearn_r2_nan_below_two{0};
int set_sklearn_compat(const char* version) {
    DFVO_ARG_CHECK(version, "dfvo_set_sklearn_compat: null version");
    int major = 0, minor = 0;
    DFVO_ARG_CHECK(sscanf(version, "%d.%d", &major, &minor) == 2, "dfvo_set_sklearn_compat: expected \"<major>.<minor>[...]\"");
    // r2_score's "fewer than two samples -> nan" rule exists from scikit-learn 0.22 on
    g_sklearn_r2_nan_below_two.store((major > 0 || minor >= 22) ? 1 : 0);
    return DFVO_OK;
}

// sklearn.linear_model.RANSACRegressor(LinearRegression(fit_intercept=False), min_samples, max_trials, stop_probability,
// residual_threshold).fit(x[:, None], y) on raw arrays already in tb.ratios (x at [0, n), y at [kp_cap, kp_cap + n), or
// d_y_is_ones: y = 1): the regression stage of find_scale_from_depth on its own (no "more than 10 valid points" gate)
int enqueue_ransac_regressor(TrackerBuffers& tb, int n, bool y_is_ones, const ScaleConfig& cfg, hipStream_t s) {
    DFVO_ARG_CHECK(n >= 1 && n <= tb.kp_cap, "ransac_regressor: capacity");
    DFVO_HIP_CHECK(hipMemcpyAsync(tb.kp_total + KPT_SCALE_VALID, &n, sizeof(int), hipMemcpyHostToDevice, s));
    DFVO_HIP_CHECK(hipStreamSynchronize(s));  // (n is a stack value)
    hipLaunchKernelGGL(k_scale_ransac, dim3(1), dim3(256), 0, s, tb.mt_state, tb.ratios,
                       y_is_ones ? (const double*)nullptr : tb.ratios + tb.kp_cap, tb.kp_total + KPT_SCALE_VALID, -1, cfg.min_samples,
                       cfg.max_trials, cfg.stop_prob, cfg.thre, tb.inl_a, tb.inl_b, tb.scratch, tb.scale_out,
                       (const PoseState*)nullptr, g_sklearn_r2_nan_below_two.load(), (const int*)nullptr);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

int enqueue_find_scale(TrackerBuffers& tb, int n_host, const double* d_T21, const double* d_depth, int H, int W,
                       const ScaleConfig& cfg, hipStream_t s, const PoseState* d_gate, bool prepared, bool depth_per_kp) {
    DFVO_ARG_CHECK(n_host >= 0 && n_host <= tb.kp_cap, "find_scale: keypoint capacity");
    if (prepared) {
        DFVO_ARG_CHECK((size_t)H * W <= tb.winner.n, "find_scale: enqueue_scale_prepare was not called for this size");
        DFVO_HIP_CHECK(hipStreamWaitEvent(s, tb.ev_rep[1], 0));
    } else {
        if (int rc = tb.grow_winner(H, W)) return rc;
        DFVO_HIP_CHECK(hipMemsetAsync(tb.winner, 0xff, sizeof(int) * (size_t)H * W, s));
        DFVO_HIP_CHECK(hipMemsetAsync(tb.kp_total + KPT_SCALE_VALID, 0, sizeof(int), s));
    }
    const int nb = cdiv(n_host > 0 ? n_host : 1, 256);
    const bool abs_diff = cfg.method == 1;
    tb.seg_mask &= ~0x700u;
    if (tb.mark(8, s) != DFVO_OK) return DFVO_ERR_HIP;
    hipLaunchKernelGGL(k_scale_triangulate, dim3(nb), dim3(256), 0, s, tb.kp_info, tb.kp_ref, tb.kp_cur, d_T21, cfg.cx,
                       cfg.cy, cfg.fx, cfg.fy, H, W, tb.z2, tb.pix, tb.winner, (const int*)nullptr);
    hipLaunchKernelGGL(k_scale_ratios, dim3(1), dim3(256), sizeof(int) * (size_t)(n_host > 0 ? n_host : 1), s, tb.kp_info,
                       tb.z2, tb.pix, tb.winner, d_depth, tb.ratios, tb.kp_total + KPT_SCALE_VALID, abs_diff ? tb.ratios + tb.kp_cap : nullptr,
                       abs_diff ? tb.ratios + 2 * (size_t)tb.kp_cap : nullptr, depth_per_kp ? 1 : 0, (const int*)nullptr);
    if (tb.mark(9, s) != DFVO_OK) return DFVO_ERR_HIP;
    hipLaunchKernelGGL(k_scale_ransac, dim3(1), dim3(256), 0, s, tb.mt_state, abs_diff ? tb.ratios + tb.kp_cap : tb.ratios,
                       abs_diff ? tb.ratios + 2 * (size_t)tb.kp_cap : (const double*)nullptr, tb.kp_total + KPT_SCALE_VALID, 10,
                       cfg.min_samples, cfg.max_trials, cfg.stop_prob, cfg.thre, tb.inl_a, tb.inl_b, tb.scratch,
                       tb.scale_out, d_gate, g_sklearn_r2_nan_below_two.load(), (const int*)nullptr);
    if (tb.mark(10, s) != DFVO_OK) return DFVO_ERR_HIP;
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

// ================================================================================================
// EssTracker.scale_recovery_iterative (E_tracker.py:509-569) as one enqueue
// ================================================================================================
struct IterMats {
    float Kinv[9], K[9];
};

// d_prev_scale (optional): the carried scale on the device, read instead of the host value; gate (optional): the E-tracker's
// pose -- scale recovery runs only when ||t|| != 0 (dfvo.py:182)
__global__ void k_iter_init(IterCtl* __restrict__ ctl, double prev_scale, const double* __restrict__ d_prev_scale,
                            const PoseState* __restrict__ gate) {
    if (threadIdx.x != 0) return;
    const bool gated = gate && gate->t[0] == 0 && gate->t[1] == 0 && gate->t[2] == 0;
    ctl->scale = d_prev_scale ? *d_prev_scale : prev_scale;
    ctl->done = gated ? 1 : 0;
    ctl->n_iter = 0;
    ctl->status = gated ? ITER_NOT_RUN : ITER_RUNNING;
    ctl->sel_round = -1;
    for (int r = 0; r < ITER_ROUNDS; ++r) {
        ctl->scale_in[r] = 0.0;
        ctl->scale_out[r] = 0.0;
        ctl->n_kp[r] = -1;
    }
    ctl->pad = 0;
}

// end of a round (E_tracker.py:557-568; the scale -1 of "too few valid points" gets no special case there either)
__device__ void iter_end(IterCtl* __restrict__ ctl, int round, const ScaleResult* __restrict__ res) {
    if (ctl->done) return;
    if (res->status < 0) {  // sklearn raised inside find_scale_from_depth
        ctl->done = 1;
        ctl->status = ITER_NO_CONSENSUS;
        return;
    }
    const double new_scale = res->scale;
    const double delta = fabs(new_scale - ctl->scale);
    ctl->scale_out[round] = new_scale;
    ctl->scale = new_scale;
    ctl->n_iter = round + 1;
    if (delta < 0.001) ctl->done = 1;
}

// start of a round, one lane: closes the round before it, then builds rigid_flow_pose = inv([R | t * scale]) of this round in
// float32, beside Kinv and K (the matrices come as a kernel argument: no host buffer has to outlive the enqueue)
__global__ void k_iter_begin(IterCtl* __restrict__ ctl, int round, const ScaleResult* __restrict__ res,
                             const double* __restrict__ E_pose, IterMats m, float* __restrict__ mats /*Kinv[9] | T[16] | K[9]*/) {
    if (threadIdx.x != 0) return;
    if (round > 0) iter_end(ctl, round - 1, res);
    if (ctl->done) return;
    const double scale = ctl->scale;
    ctl->scale_in[round] = scale;
    for (int i = 0; i < 9; ++i) {
        mats[i] = m.Kinv[i];
        mats[25 + i] = m.K[i];
    }
    sm::rigid_pose_inv_f32(E_pose, scale, mats + 9);
}

// behind the selection.  Lane 0 of block 0: the reference asserts a non-empty selection before it looks for the scale.  Every
// thread: the two fills of the scale stage (see enqueue_scale_prepare).  A block that reads `done` while lane 0 sets it for an
// empty selection may still clear its part of the map: nothing reads the map before the next call clears all of it.
__global__ void k_iter_selected(IterCtl* __restrict__ ctl, int round, const int* __restrict__ n_uniform, int* __restrict__ winner,
                                int px, int* __restrict__ n_valid) {
    if (ctl->done) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < px) winner[i] = -1;
    if (i != 0) return;
    *n_valid = 0;
    const int n = *n_uniform;
    ctl->n_kp[round] = n;
    if (n == 0) {
        ctl->done = 1;
        ctl->status = ITER_EMPTY;
    } else {
        ctl->sel_round = round;
    }
}

// behind the last round, one lane
__global__ void k_iter_end(IterCtl* __restrict__ ctl, int round, const ScaleResult* __restrict__ res) {
    if (threadIdx.x == 0) iter_end(ctl, round, res);
}

// behind k_iter_end, one lane: self.prev_scale = new_scale of the last completed round (E_tracker.py:559); a call that
// completed no round (gated, an empty first selection, no consensus set in round 0) leaves it as it was
__global__ void k_iter_store_prev(const IterCtl* __restrict__ ctl, double* __restrict__ d_prev_scale) {
    if (threadIdx.x == 0 && ctl->n_iter > 0) *d_prev_scale = ctl->scale;
}

int enqueue_scale_recovery_iterative(TrackerBuffers& tb, RigidKpBuffers& rb, const float* d_flow, const float* d_odiff,
                                     const float* d_depth32_ref, const double* d_depth64_cur, int H, int W,
                                     const RigidKpConfig& cfg, const ScaleConfig& scfg, const double* d_E_pose,
                                     const double* d_T21, double prev_scale, int kp_src, int n_kp_best, hipStream_t s,
                                     const IterDevice* dev) {
    DFVO_ARG_CHECK(d_flow && d_odiff && d_depth32_ref && d_depth64_cur && d_E_pose && d_T21 && H > 0 && W > 0,
                   "scale_recovery_iterative: bad argument");
    DFVO_ARG_CHECK(kp_src == 0 || kp_src == 1, "scale_recovery_iterative: kp_src is 0 (kp_depth) or 1 (kp_best)");
    DFVO_ARG_CHECK(scfg.min_samples >= 1 && scfg.min_samples <= 8, "scale_recovery_iterative: min_samples in [1,8]");
    int cells, n_best, cap, par;
    size_t lds;
    if (int rc_g = rigid_flow_kp_geometry(H, W, cfg, &cells, &n_best, &cap, &lds, &par)) return rc_g;
    // the keypoints the scale stage may see: a round's uniform set (at most cells * n_best) or the caller's fixed set
    const int n_sel = cells * n_best;
    const int n_scale = kp_src == 0 ? n_sel : n_kp_best;
    DFVO_ARG_CHECK(n_scale >= 0 && n_scale <= ITER_MAX_KP,
                   "scale_recovery_iterative: more keypoints than k_scale_ratios holds in 64 KB of LDS (16384)");
    DFVO_ARG_CHECK(kp_src == 0 || n_kp_best <= tb.kp_cap, "scale_recovery_iterative: kp_best exceeds the keypoint capacity");
    if (int rc_e = rb.ensure(H, W, cells, n_best, cap)) return rc_e;
    if (kp_src == 0)
        if (int rc_k = tb.ensure_kp(n_sel > 16 ? n_sel : 16, 1, 1)) return rc_k;
    if (int rc_w = tb.grow_winner(H, W)) return rc_w;
    IterMats m;
    for (int i = 0; i < 9; ++i) m.Kinv[i] = cfg.Kinv[i], m.K[i] = cfg.K[i];
    IterCtl* ctl = rb.ctl;
    const int* skip = &ctl->done;
    const size_t sc = (size_t)rb.sel_cap * 2;
    const double* kp1 = kp_src == 0 ? rb.kp + 2 * sc : tb.kp_ref.p;
    const double* kp2 = kp_src == 0 ? rb.kp + 3 * sc : tb.kp_cur.p;
    const int* n_ptr = kp_src == 0 ? rb.info + 4 : tb.kp_info.p;  // (kp_best: the caller set tb.kp_info[0] with the keypoints)
    const int nb = cdiv(n_scale > 0 ? n_scale : 1, 256);
    const size_t ratios_lds = sizeof(int) * (size_t)(n_scale > 0 ? n_scale : 1);
    const bool abs_diff = scfg.method == 1;
    const int px = H * W;
    tb.seg_mask &= ~0x700u;  // no stage marks between the rounds: dfvo_tracker_stage_ms reports none for the scale stage
    hipLaunchKernelGGL(k_iter_init, dim3(1), dim3(64), 0, s, ctl, prev_scale, (const double*)(dev ? dev->prev_scale : nullptr),
                       dev ? dev->gate : (const PoseState*)nullptr);
    for (int r = 0; r < ITER_ROUNDS; ++r) {
        hipLaunchKernelGGL(k_iter_begin, dim3(1), dim3(64), 0, s, ctl, r, (const ScaleResult*)tb.scale_out.p, d_E_pose, m,
                           rb.mats.p);
        if (int rc_r = enqueue_rigid_flow_kp_round(rb, d_flow, d_odiff, d_depth32_ref, H, W, cfg, rb.rdiff_of(r, H, W), skip, s))
            return rc_r;
        hipLaunchKernelGGL(k_iter_selected, dim3(cdiv(px, 256)), dim3(256), 0, s, ctl, r, (const int*)(rb.info + 4), tb.winner.p, px,
                           tb.kp_total + KPT_SCALE_VALID);
        hipLaunchKernelGGL(k_scale_triangulate, dim3(nb), dim3(256), 0, s, n_ptr, kp1, kp2, d_T21, scfg.cx, scfg.cy, scfg.fx,
                           scfg.fy, H, W, tb.z2.p, tb.pix.p, tb.winner.p, skip);
        hipLaunchKernelGGL(k_scale_ratios, dim3(1), dim3(256), ratios_lds, s, n_ptr, (const double*)tb.z2.p, (const int*)tb.pix.p,
                           (const int*)tb.winner.p, d_depth64_cur, tb.ratios.p, tb.kp_total + KPT_SCALE_VALID,
                           abs_diff ? tb.ratios + tb.kp_cap : (double*)nullptr,
                           abs_diff ? tb.ratios + 2 * (size_t)tb.kp_cap : (double*)nullptr, 0, skip);
        hipLaunchKernelGGL(k_scale_ransac, dim3(1), dim3(256), 0, s, tb.mt_state,
                           (const double*)(abs_diff ? tb.ratios + tb.kp_cap : tb.ratios.p),
                           (const double*)(abs_diff ? tb.ratios + 2 * (size_t)tb.kp_cap : nullptr),
                           (const int*)(tb.kp_total + KPT_SCALE_VALID), 10, scfg.min_samples, scfg.max_trials, scfg.stop_prob,
                           scfg.thre, tb.inl_a.p, tb.inl_b.p, tb.scratch.p, tb.scale_out.p, (const PoseState*)nullptr,
                           g_sklearn_r2_nan_below_two.load(), skip);
    }
    hipLaunchKernelGGL(k_iter_end, dim3(1), dim3(64), 0, s, ctl, ITER_ROUNDS - 1, (const ScaleResult*)tb.scale_out.p);
    if (dev && dev->prev_scale)
        hipLaunchKernelGGL(k_iter_store_prev, dim3(1), dim3(64), 0, s, (const IterCtl*)ctl, dev->prev_scale);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

}  // namespace dfvo
