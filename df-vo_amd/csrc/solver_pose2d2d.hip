// EssTracker.compute_pose_2d2d around the RANSAC solvers of solver_ransac.hip: GRIC model selection, the repeated
// shuffled five-point RANSAC and the validity bookkeeping.  Reference call sites (paths relative to /root/reference):
//   libs/tracker/gric.py:14-132                   Sampson / homography residuals + GRIC
//   libs/tracker/E_tracker.py:154-307             compute_pose_2d2d
// See tracker.h on sequential semantics.  Built with -ffp-contract=off.
#include <cstring>  // memcmp, memcpy: the host copy of the intrinsics

#include "np_legacy.h"    // sm::np_add_reduce
#include "solver_math.h"  // sm::mul33
#include "tracker.h"

namespace dfvo {

// blockIdx.y = repeat: perm / pa / pb advance by perm_stride / pts_stride elements per repeat
__global__ void k_permute_points(const int* __restrict__ n_ptr, const int* __restrict__ perm, int perm_stride,
                                 const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ pa,
                                 double* __restrict__ pb, int pts_stride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *n_ptr) return;
    perm += (size_t)blockIdx.y * perm_stride;
    pa += (size_t)blockIdx.y * pts_stride;
    pb += (size_t)blockIdx.y * pts_stride;
    const int p = perm[i];
    pa[i * 2] = a[p * 2];
    pa[i * 2 + 1] = a[p * 2 + 1];
    pb[i * 2] = b[p * 2];
    pb[i * 2 + 1] = b[p * 2 + 1];
}

// ================================================================================================
// GRIC
// ================================================================================================
// residual + calc_GRIC in one launch, blockIdx.x = problem (kp1 / kp2 advance by pts_stride, out by one element per
// problem).  mode 0: res = compute_fundamental_residual(F, kp1, kp2) with F = KinvT @ E @ Kinv (gric.py:14-37); mode 1:
// res = compute_homography_residual(H, kp1, kp2) (gric.py:40-92).  The residual of point i is produced by all threads
// straight into the LDS staging buffer; calc_GRIC (gric.py:95-132) then sums the clamped terms on one lane in the
// reference's sequential np.sum order, batched by eight so that LDS latency overlaps.
struct GricFusedBatch {
    const double* M[MAX_E_BATCH];  // E (mode 0) or H (mode 1) per problem
};
__global__ __launch_bounds__(256) void k_gric_fused(const GricFusedBatch G, int mode, const double* __restrict__ KinvT,
                                                     const double* __restrict__ Kinv, const int* __restrict__ n_ptr,
                                                     const double* __restrict__ kp1, const double* __restrict__ kp2,
                                                     int pts_stride, double sigma, int Kp, int D,
                                                     double* __restrict__ out) {
    __shared__ double s_res[2048];
    __shared__ double s_M[9];
    const int n = *n_ptr;
    const double* Min = G.M[blockIdx.x];
    kp1 += (size_t)blockIdx.x * pts_stride;
    kp2 += (size_t)blockIdx.x * pts_stride;
    out += blockIdx.x;
    if (threadIdx.x == 0) {
        if (mode == 0) {  // F = K^-T E K^-1
            double T[9], F[9];
            sm::mul33(KinvT, Min, T);
            sm::mul33(T, Kinv, F);
            for (int k = 0; k < 9; k++) s_M[k] = F[k];
        } else {
            for (int k = 0; k < 9; k++) s_M[k] = Min[k];
        }
    }
    __syncthreads();
    const double R = 4, sigmasq1 = 1. / (sigma * sigma);
    const double lam3RD = 2.0 * (R - D);
    double sum = 0;
    for (int c0 = 0; c0 < n; c0 += 2048) {
        const int cnt = n - c0 < 2048 ? n - c0 : 2048;
        for (int k = threadIdx.x; k < cnt; k += 256) {
            const int i = c0 + k;
            double r;
            if (mode == 0) {
                const double* F = s_M;
                const double m0[3] = {kp1[i * 2], kp1[i * 2 + 1], 1.0}, m1[3] = {kp2[i * 2], kp2[i * 2 + 1], 1.0};
                double Fm0[3], Ftm1[3];
                for (int q = 0; q < 3; q++) {
                    Fm0[q] = F[q * 3] * m0[0] + F[q * 3 + 1] * m0[1] + F[q * 3 + 2] * m0[2];
                    Ftm1[q] = F[q] * m1[0] + F[3 + q] * m1[1] + F[6 + q] * m1[2];
                }
                const double m1Fm0 = Fm0[0] * m1[0] + Fm0[1] * m1[1] + Fm0[2] * m1[2];
                r = m1Fm0 * m1Fm0 / ((Fm0[0] * Fm0[0] + Fm0[1] * Fm0[1]) + (Ftm1[0] * Ftm1[0] + Ftm1[1] * Ftm1[1]));
            } else {
                const double* H = s_M;
                const double m0x = kp1[i * 2], m0y = kp1[i * 2 + 1], m1x = kp2[i * 2], m1y = kp2[i * 2 + 1];
                const double G00 = H[0] - m1x * H[6], G01 = H[1] - m1x * H[7], G02 = -m0x * H[6] - m0y * H[7] - H[8];
                const double G10 = H[3] - m1y * H[6], G11 = H[4] - m1y * H[7], G12 = -m0x * H[6] - m0y * H[7] - H[8];
                const double magG0 = sqrt(G00 * G00 + G01 * G01 + G02 * G02);
                const double magG1 = sqrt(G10 * G10 + G11 * G11 + G12 * G12);
                const double magG0G1 = G00 * G10 + G01 * G11;
                const double alpha = acos(magG0G1 / (magG0 * magG1));
                const double alg0 = m0x * H[0] + m0y * H[1] + H[2] - m1x * (m0x * H[6] + m0y * H[7] + H[8]);
                const double alg1 = m0x * H[3] + m0y * H[4] + H[5] - m1y * (m0x * H[6] + m0y * H[7] + H[8]);
                const double D1 = alg0 / magG0, D2 = alg1 / magG1;
                r = (D1 * D1 + D2 * D2 - 2.0 * D1 * D2 * cos(alpha)) / sin(alpha);
            }
            s_res[k] = r;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int i = 0;
            for (; i + 8 <= cnt; i += 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double tmp = s_res[i + u] * sigmasq1;
                    v[u] = tmp <= lam3RD ? tmp : lam3RD;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) sum += v[u];
            }
            for (; i < cnt; i++) {
                const double tmp = s_res[i] * sigmasq1;
                sum += tmp <= lam3RD ? tmp : lam3RD;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sum += n * D * log(R) + Kp * log(R * n);
        *out = sum;
    }
}

// ================================================================================================
// compute_pose_2d2d bookkeeping
// ================================================================================================
__global__ void k_pose_state_init(PoseState* ps, const int* __restrict__ n_ptr, uint8_t* __restrict__ best_inliers,
                                  int cap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) best_inliers[i] = 1;  // np.ones((N,1)) == 1
    if (i == 0) {
        ps->best_cnt = 0;
        ps->num_valid = 0;
        ps->have_best = 0;
        ps->h_gric = 0;
        ps->n = *n_ptr;
        for (int k = 0; k < 9; k++) ps->best_E[k] = 0;
        for (int k = 0; k < 9; k++) ps->R[k] = (k % 4 == 0) ? 1.0 : 0.0;
        ps->t[0] = ps->t[1] = ps->t[2] = 0;
        ps->cheirality = 0;
        ps->valid_case = 1;
        ps->major_valid = 0;
        ps->h_found = 0;
        for (int k = 0; k < 8; k++) {
            ps->rep_cnt[k] = 0;
            ps->rep_valid[k] = 0;
            ps->rep_gric[k] = 0;
        }
    }
}

// Where the REFERENCE raises inside its repeat loop, the device answers with a fixed contract (include/dfvo_hip.h): identity /
// zero pose, no valid repeat, the all-ones inlier mask, and the RandomState the reference left behind: `shuffles` draws
// after the call's start (0: findHomography found nothing under GRIC validity, homography_residual(None) raises before the
// loop; rep + 1: findEssentialMat returned None in repeat `rep`).  Called by every thread of the one-block bookkeeping kernel.
__device__ void pose_after_raise(PoseState* ps, int shuffles, uint32_t* __restrict__ mt_state, const uint32_t* __restrict__ snap,
                                 uint8_t* __restrict__ best_inliers, int repeat) {
    const int n = ps->n;
    __syncthreads();
    if (mt_state && snap)
        for (int i = threadIdx.x; i < 625; i += blockDim.x) mt_state[i] = snap[(size_t)shuffles * MT_SNAP_STRIDE + i];
    for (int c = threadIdx.x; c < n; c += blockDim.x) best_inliers[c] = 1;
    if (threadIdx.x == 0) {
        ps->best_cnt = 0;
        ps->num_valid = 0;
        ps->have_best = 0;
        ps->major_valid = 0;
        for (int k = 0; k < repeat; k++) ps->rep_valid[k] = 0;
    }
}

// the whole post-RANSAC bookkeeping of compute_pose_2d2d in one launch (E_tracker.py:258-285): H validity (h_found,
// h_gric = the homography's GRIC, inf without a model), then per repeat, in order: valid_case, the inlier check and, for
// the repeat with the most inliers so far, best_E and its un-permuted mask; last
// major_valid = num_valid_case > (max_ransac_iter / 2).  recoverPose's tail (PoseFinish, solver_ransac.hip) consumes it.
struct RepBatch {
    const RansacState* st[MAX_REP];
    const double* E[MAX_REP];
    const uint8_t* mask[MAX_REP];
};
// the steps k_rep_update_all and k_rep_update_flow share.  A repeat becomes the best model so far (one thread) ...
__device__ __forceinline__ void rep_take_model(PoseState* ps, int cnt, const double* E) {
    ps->best_cnt = cnt;
    ps->have_best = 1;
    for (int k = 0; k < 9; k++) ps->best_E[k] = E[k];
}
// ... and its mask, computed on the shuffled points, goes back to keypoint order (every thread of the block)
__device__ __forceinline__ void rep_take_mask(const uint8_t* mask, const int* perm, int n,
                                              uint8_t* best_inliers) {
    for (int c = threadIdx.x; c < n; c += blockDim.x) best_inliers[perm[c]] = mask[c];
}
// major_valid = num_valid_case > (max_ransac_iter / 2)
__device__ __forceinline__ void pose_set_major_valid(PoseState* ps, int repeat) {
    ps->major_valid = ((double)ps->num_valid > (double)repeat / 2.0 && ps->have_best) ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_rep_update_all(PoseState* ps, const RansacState* hst, const double* __restrict__ h_gric,
                                                         const RepBatch B, const double* __restrict__ e_gric,
                                                         const int* __restrict__ perm, int perm_stride,
                                                         uint8_t* __restrict__ best_inliers, int repeat,
                                                         int by_ratio, double ratio_thre, uint32_t* __restrict__ mt_state,
                                                         const uint32_t* __restrict__ snap) {
    // by_ratio (validity.method 'homo_ratio', E_tracker.py:186-194,243-250): a repeat is valid while
    // H_inliers.sum() / (H_inliers.sum() + inliers.sum()) < thre (0 / 0 = nan compares false, like numpy);
    // h_gric then carries the homography's inlier count and rep_gric[] the ratios
    __shared__ int s_take, s_raise;
    const int n = ps->n;
    if (threadIdx.x == 0) {
        s_raise = -1;
        if (!by_ratio && !hst->found) s_raise = 0;
        for (int rep = 0; rep < repeat && s_raise < 0; ++rep)
            if (!B.st[rep]->found) s_raise = rep + 1;
        ps->h_found = hst->found;
        if (by_ratio)
            ps->h_gric = hst->found ? (double)hst->max_good : 0.0;  // no model: OpenCV returns an all-zero mask
        else
            ps->h_gric = hst->found ? *h_gric : INFINITY;
    }
    __syncthreads();
    for (int rep = 0; rep < repeat; ++rep) {
        if (threadIdx.x == 0) {
            const RansacState* est = B.st[rep];
            const int found = est->found;
            const int cnt = found ? est->max_good : 0;
            bool valid;
            double crit;
            if (by_ratio) {
                crit = ps->h_gric / (ps->h_gric + (double)cnt);
                valid = crit < ratio_thre;
            } else {
                crit = found ? e_gric[rep] : INFINITY;
                valid = found && (ps->h_gric > e_gric[rep]);
            }
            ps->rep_cnt[rep] = cnt;
            ps->rep_valid[rep] = valid ? 1 : 0;
            ps->rep_gric[rep] = crit;
            ps->num_valid += valid ? 1 : 0;
            s_take = (found && cnt > ps->best_cnt) ? 1 : 0;
            if (s_take) rep_take_model(ps, cnt, B.E[rep]);
        }
        __syncthreads();
        if (s_take) rep_take_mask(B.mask[rep], perm + (size_t)rep * perm_stride, n, best_inliers);
        __syncthreads();
    }
    if (threadIdx.x == 0) pose_set_major_valid(ps, repeat);
    if (s_raise >= 0) pose_after_raise(ps, s_raise, mt_state, snap, best_inliers, repeat);
}

// ---- e_tracker.validity.method == "flow" (ablation_model_sel_flow.yml) ------------------------------------------
// valid_case = np.mean(np.linalg.norm(kp_ref - kp_cur, axis=1)) > thre (E_tracker.py:182-185).  gate[0] = the keypoint
// count the shuffles see (n when the pair is tracked, 0 otherwise: a closed gate draws nothing from np.random),
// gate[1] = valid_case; the mean goes to *avg_out
__global__ __launch_bounds__(256) void k_flow_gate(const int* __restrict__ kp_info, const double* __restrict__ kp_ref,
                                                    const double* __restrict__ kp_cur, double thre, double* __restrict__ norms,
                                                    double* __restrict__ avg_out, int* __restrict__ gate) {
    const int n = kp_info[0];
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double dx = kp_ref[i * 2] - kp_cur[i * 2], dy = kp_ref[i * 2 + 1] - kp_cur[i * 2 + 1];
        norms[i] = sqrt(dx * dx + dy * dy);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double avg = sm::np_add_reduce(norms, n) / (double)n;  // n == 0: nan, compares false like numpy's
        *avg_out = avg;
        const int open = avg > thre ? 1 : 0;
        gate[0] = open ? n : 0;
        gate[1] = open;
    }
}

__global__ void k_copy_double(double* __restrict__ dst, const double* __restrict__ src) { *dst = *src; }

// the per-repeat bookkeeping of the "flow" validity: validity of a repeat = its recoverPose cheirality count above
// 10 % of the keypoints, best model = most RANSAC inliers among the repeats whose count is above 5 %
__global__ __launch_bounds__(256) void k_rep_update_flow(PoseState* ps, const int* __restrict__ gate, const double* __restrict__ avg_flow,
                                                          const RepBatch B, const double* __restrict__ cheir,
                                                          const int* __restrict__ perm, int perm_stride,
                                                          uint8_t* __restrict__ best_inliers, int repeat,
                                                          uint32_t* __restrict__ mt_state, const uint32_t* __restrict__ snap) {
    __shared__ int s_take, s_raise;
    const int n = ps->n;
    const int open = gate[1];
    if (threadIdx.x == 0) {
        s_raise = -1;  // recoverPose(None, ...) raises in the repeat whose findEssentialMat found nothing
        for (int rep = 0; open && rep < repeat && s_raise < 0; ++rep)
            if (!B.st[rep]->found) s_raise = rep + 1;
        ps->h_found = 0;
        ps->h_gric = *avg_flow;
    }
    __syncthreads();
    for (int rep = 0; rep < repeat; ++rep) {
        if (threadIdx.x == 0) {
            const RansacState* est = B.st[rep];
            const int found = open && est->found;
            const int cnt = found ? est->max_good : 0;
            const double c = found ? cheir[rep] : 0.0;
            const bool valid = found && c > (double)n * 0.1;
            ps->rep_cnt[rep] = cnt;
            ps->rep_valid[rep] = valid ? 1 : 0;
            ps->rep_gric[rep] = c;
            ps->num_valid += valid ? 1 : 0;
            s_take = (found && cnt > ps->best_cnt && c > (double)n * 0.05) ? 1 : 0;
            if (s_take) rep_take_model(ps, cnt, B.E[rep]);
        }
        __syncthreads();
        if (s_take) rep_take_mask(B.mask[rep], perm + (size_t)rep * perm_stride, n, best_inliers);
        __syncthreads();
    }
    if (threadIdx.x == 0) pose_set_major_valid(ps, repeat);
    if (s_raise >= 0) pose_after_raise(ps, s_raise, mt_state, snap, best_inliers, repeat);
}

// RNG-independent half of compute_pose_2d2d: state reset, findHomography + refinement, GRIC-H.  Everything reads the
// keypoint count from the device (tb.kp_info[0]; n_bound only sizes the launches), so it can be enqueued before the
// host knows that count -- the fused pipeline runs it right behind the nets of a pair, while the solver stage of the
// previous pair is still busy.  Records tb.ev_start (keypoints ready) and tb.ev_h (this half done) on sh.
int enqueue_pose_h_part(TrackerBuffers& tb, int n_bound, const PoseConfig& cfg, hipStream_t sh) {
    DFVO_ARG_CHECK(n_bound >= 0 && n_bound <= tb.kp_cap, "compute_pose_2d2d: keypoint capacity");
    tb.seg_mask &= ~0xffu;
    // the intrinsics are constant for a pipeline / tracker: uploaded (synchronously) only when they differ from what this
    // buffer set already holds, so the per-pair path contains no host-to-device copy at all (a copy queued behind the
    // stream's wait for the nets delayed the whole keypoint stage by milliseconds; a pageable source could be read late)
    double hk[18];
    for (int i = 0; i < 9; i++) {
        hk[i] = cfg.KinvT[i];
        hk[9 + i] = cfg.Kinv[i];
    }
    if (!tb.small_valid || memcmp(tb.h_small, hk, sizeof(hk)) != 0) {
        DFVO_HIP_CHECK(hipDeviceSynchronize());  // nothing in flight may still read the old values
        DFVO_HIP_CHECK(hipMemcpy(tb.small, hk, sizeof(hk), hipMemcpyHostToDevice));
        memcpy(tb.h_small, hk, sizeof(hk));
        tb.small_valid = true;
    }
    hipLaunchKernelGGL(k_pose_state_init, dim3(cdiv(tb.kp_cap, 256)), dim3(256), 0, sh, tb.pose, tb.kp_info,
                       tb.best_inliers, tb.kp_cap);
    // the five-point sampler's first chunk of subsets depends on the keypoint COUNT only: drawn here, beside the homography
    // chain, instead of inside the RandomState-ordered chain (round 6; consumed by enqueue_pose_e_part through tb.e_pre_*)
    tb.e_pre_iters = 0;
    static const bool subsets_ahead = env_flag("DFVO_E_SUBSETS_AHEAD", true);  // (0: A/B hook)
    if (subsets_ahead && cfg.max_iters >= 1) {
        int rc_pre = enqueue_e_subsets_prefetch(tb.ws_rep[0], tb.kp_info, n_bound, cfg.max_iters,
                                                reinterpret_cast<unsigned long long*>(tb.kp_total + KPT_E_RNG), sh);
        if (rc_pre != DFVO_OK) return rc_pre;
        tb.e_pre_iters = cfg.max_iters;
    }
    DFVO_HIP_CHECK(hipEventRecord(tb.ev_start, sh));
    tb.ev_t_half = tb.ev_t[4] != nullptr;
    if (tb.ev_t_half) DFVO_HIP_CHECK(hipEventRecord(tb.ev_t[4], sh));
    if (tb.mark(0, sh) != DFVO_OK) return DFVO_ERR_HIP;
    auto done = [&]() -> int {
        DFVO_HIP_CHECK(hipEventRecord(tb.ev_h, sh));
        if (tb.ev_t_half) DFVO_HIP_CHECK(hipEventRecord(tb.ev_t[5], sh));
        DFVO_HIP_CHECK(hipGetLastError());
        return DFVO_OK;
    };
    if (cfg.validity == 1) {  // "flow": no homography; the mean displacement decides whether the pair is tracked
        hipLaunchKernelGGL(k_flow_gate, dim3(1), dim3(256), 0, sh, tb.kp_info, tb.kp_ref, tb.kp_cur, cfg.validity_thre,
                           tb.pa, tb.small + SMALL_H_GRIC, tb.kp_total + KPT_FLOW_GATE);
        return done();
    }
    // ---- homography + GRIC-H (kp_cur -> kp_ref); with 10 or fewer keypoints the result is never consumed
    // (E_tracker.py:196) and with fewer than 5 the chain marks itself "no model"
    // homo_ratio: the same call with ransacReprojThreshold 0.2, only its inlier count is used (E_tracker.py:188-194)
    int rc = enqueue_find_homography(tb.ws_h, tb.kp_cur, tb.kp_ref, n_bound, cfg.validity == 2 ? 0.2 : 1.0, 2000, 0.99, sh,
                                     tb.kp_info);
    if (rc != DFVO_OK) return rc;
    if (tb.mark(1, sh) != DFVO_OK) return DFVO_ERR_HIP;
    if (cfg.validity != 2) {
        GricFusedBatch GH;
        for (int r = 0; r < MAX_E_BATCH; ++r) GH.M[r] = tb.ws_h.out;
        hipLaunchKernelGGL(k_gric_fused, dim3(1), dim3(256), 0, sh, GH, 1, tb.small + SMALL_KINVT, tb.small + SMALL_KINV, tb.kp_info, tb.kp_cur,
                           tb.kp_ref, 0, 0.8, 8, 2, tb.small + SMALL_H_GRIC);
        if (tb.mark(2, sh) != DFVO_OK) return DFVO_ERR_HIP;
    }
    return done();
}

// RNG-consuming half: `repeat` x (shuffle, findEssentialMat, GRIC-E) as one batch on tb.s_rep[0] (after tb.ev_start),
// then on s (after tb.ev_h): validity bookkeeping, recoverPose, pose / T21.  n_host = the keypoint count.
// s waits for tb.ev_h where the homography half is first read -- in front of k_rep_update_* (ws_h.state, SMALL_H_GRIC) --
// and not at the top: tb.s_rep[0] may be s itself (the fused pipeline's lane layout), and the batch reads nothing of that
// half (keypoints, count and the prefetched subsets are complete at tb.ev_start; pa / pb / perm / ws_rep are its own).
// validity "flow" is the exception: the gate (k_flow_gate, scratch tb.pa) feeds the shuffles, so the batch waits for
// tb.ev_h itself.  A pair with too few keypoints for the batch still leaves s behind tb.ev_h.
// one lane: the accepted pose as a 4 x 4 (E_pose.pose of dfvo.py:172), for the iterative scale loop
__global__ void k_pose_matrix(const PoseState* __restrict__ ps, double* __restrict__ E) {
    if (threadIdx.x != 0) return;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) E[r * 4 + c] = ps->R[r * 3 + c];
        E[r * 4 + 3] = ps->t[r];
    }
    E[12] = E[13] = E[14] = 0;
    E[15] = 1;
}

int enqueue_pose_e_part(TrackerBuffers& tb, int n_host, const PoseConfig& cfg, hipStream_t s, double* d_T21, double* d_E_pose) {
    DFVO_ARG_CHECK(n_host >= 0 && n_host <= tb.kp_cap, "compute_pose_2d2d: keypoint capacity");
    DFVO_ARG_CHECK(cfg.repeat >= 1 && cfg.repeat <= MAX_REP, "compute_pose_2d2d: repeat out of range");
    const bool by_flow = cfg.validity == 1, by_ratio = cfg.validity == 2;
    // GRIC: only when more than 10 keypoints (E_tracker.py:196); flow / homo_ratio: whenever the five-point solver has
    // its 5 points
    if (by_flow || by_ratio ? n_host >= 5 : n_host > 10) {
        const int nb = cdiv(n_host, 256);
        const int cap = tb.kp_cap;
        hipStream_t sr = tb.s_rep[0];
        const unsigned R = (unsigned)cfg.repeat;
        // flow: the shuffles (and with them np.random) only run behind an open gate: their count is gate[0] = n or 0
        const int* d_n = by_flow ? tb.kp_total + KPT_FLOW_GATE : tb.kp_info;
        DFVO_HIP_CHECK(hipStreamWaitEvent(sr, by_flow ? tb.ev_h : tb.ev_start, 0));
        if (tb.ev_t[0]) DFVO_HIP_CHECK(hipEventRecord(tb.ev_t[0], sr));
        if (tb.mark(3, sr) != DFVO_OK) return DFVO_ERR_HIP;
        int rc = enqueue_mt_shuffle(tb.mt_state, d_n, n_host, cfg.repeat, cap + 8, tb.perm, sr, mt_snapshots(tb.mt_state));
        if (rc != DFVO_OK) return rc;
        hipLaunchKernelGGL(k_permute_points, dim3(nb, R), dim3(256), 0, sr, d_n, tb.perm, cap + 8, tb.kp_cur,
                           tb.kp_ref, tb.pa, tb.pb, 2 * cap);
        // the `repeat` five-point RANSACs as one batched launch sequence (blockIdx.y = repeat)
        const double *pas[MAX_REP], *pbs[MAX_REP];
        for (int rep = 0; rep < cfg.repeat; ++rep) {
            pas[rep] = tb.pa + (size_t)rep * 2 * cap;
            pbs[rep] = tb.pb + (size_t)rep * 2 * cap;
        }
        // (the first chunk's subsets were drawn by the homography half for this keypoint count, if it ran with this budget)
        const unsigned long long* rng_pre = tb.e_pre_iters == cfg.max_iters ? reinterpret_cast<const unsigned long long*>(tb.kp_total + KPT_E_RNG) : nullptr;
        tb.e_pre_iters = 0;
        rc = enqueue_find_essential_batch(tb.ws_rep, pas, pbs, cfg.repeat, n_host, cfg.fx, cfg.cx, cfg.cy, 0.99,
                                          cfg.reproj_thre, cfg.max_iters, sr, rng_pre);
        if (rc != DFVO_OK) return rc;
        if (tb.mark(4, sr) != DFVO_OK) return DFVO_ERR_HIP;
        if (by_flow) {
            // cv2.recoverPose(E_rep, shuffled points): only its count is used (E_tracker.py:243-250); the homography
            // workspace, idle in this mode, is the scratch of the `repeat` calls
            for (int rep = 0; rep < cfg.repeat; ++rep) {
                rc = enqueue_recover_pose(tb.ws_h, tb.ws_rep[rep].out, pas[rep], pbs[rep], n_host, cfg.fx, cfg.cx, cfg.cy, sr);
                if (rc != DFVO_OK) return rc;
                hipLaunchKernelGGL(k_copy_double, dim3(1), dim3(1), 0, sr, tb.small + SMALL_E_GRIC + rep, tb.ws_h.out + 16 + 12);
            }
        } else if (!by_ratio) {
            GricFusedBatch GE;
            for (int rep = 0; rep < MAX_E_BATCH; ++rep) GE.M[rep] = rep < cfg.repeat ? tb.ws_rep[rep].out : nullptr;
            hipLaunchKernelGGL(k_gric_fused, dim3(R), dim3(256), 0, sr, GE, 0, tb.small + SMALL_KINVT, tb.small + SMALL_KINV, tb.kp_info, tb.pa, tb.pb,
                               2 * cap, 0.8, 5, 3, tb.small + SMALL_E_GRIC);
        }
        if (tb.ev_t[1]) DFVO_HIP_CHECK(hipEventRecord(tb.ev_t[1], sr));
        if (!by_flow && !by_ratio && tb.mark(5, sr) != DFVO_OK) return DFVO_ERR_HIP;
        DFVO_HIP_CHECK(hipEventRecord(tb.ev_rep[0], sr));
        DFVO_HIP_CHECK(hipStreamWaitEvent(s, tb.ev_rep[0], 0));
        DFVO_HIP_CHECK(hipStreamWaitEvent(s, tb.ev_h, 0));  // the homography half: read from here on
        {
            RepBatch RB;
            for (int rep = 0; rep < MAX_REP; ++rep) {
                RB.st[rep] = rep < cfg.repeat ? tb.ws_rep[rep].state : nullptr;
                RB.E[rep] = rep < cfg.repeat ? tb.ws_rep[rep].out : nullptr;
                RB.mask[rep] = rep < cfg.repeat ? tb.ws_rep[rep].mask : nullptr;
            }
            if (by_flow)
                hipLaunchKernelGGL(k_rep_update_flow, dim3(1), dim3(256), 0, s, tb.pose, tb.kp_total + KPT_FLOW_GATE, tb.small + SMALL_H_GRIC, RB,
                                   tb.small + SMALL_E_GRIC, tb.perm, cap + 8, tb.best_inliers, cfg.repeat, tb.mt_state,
                                   mt_snapshots(tb.mt_state));
            else
                hipLaunchKernelGGL(k_rep_update_all, dim3(1), dim3(256), 0, s, tb.pose, tb.ws_h.state, tb.small + SMALL_H_GRIC, RB,
                                   tb.small + SMALL_E_GRIC, tb.perm, cap + 8, tb.best_inliers, cfg.repeat, by_ratio ? 1 : 0,
                                   cfg.validity_thre, tb.mt_state, mt_snapshots(tb.mt_state));
        }
        if (tb.mark(6, s) != DFVO_OK) return DFVO_ERR_HIP;
        // recoverPose(best_E, kp_cur, kp_ref): always enqueued, consumed only when major_valid; its last kernel also
        // writes the pose bookkeeping and (fused pipeline) the inverse pose for the scale stage
        PoseFinish fin;
        fin.ps = tb.pose;
        fin.T21 = d_T21;
        rc = enqueue_recover_pose(tb.ws_rep[0], (const double*)((const char*)tb.pose.p + offsetof(PoseState, best_E)),
                                  tb.kp_cur, tb.kp_ref, n_host, cfg.fx, cfg.cx, cfg.cy, s, fin);
        if (rc != DFVO_OK) return rc;
        if (d_E_pose) hipLaunchKernelGGL(k_pose_matrix, dim3(1), dim3(64), 0, s, (const PoseState*)tb.pose.p, d_E_pose);
        if (tb.ev_t[2]) DFVO_HIP_CHECK(hipEventRecord(tb.ev_t[2], s));
        if (tb.mark(7, s) != DFVO_OK) return DFVO_ERR_HIP;
    } else {
        DFVO_HIP_CHECK(hipStreamWaitEvent(s, tb.ev_h, 0));  // no batch: whatever follows on s still comes behind that half
    }
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

// EssTracker.compute_pose_2d2d on tb.kp_ref / tb.kp_cur (n = kp_info[0] on the device, n_host = the same count known
// to the host): both halves on one stream
int enqueue_compute_pose_2d2d(TrackerBuffers& tb, int n_host, const PoseConfig& cfg, hipStream_t s, double* d_T21) {
    int rc = enqueue_pose_h_part(tb, n_host, cfg, s);
    if (rc != DFVO_OK) return rc;
    return enqueue_pose_e_part(tb, n_host, cfg, s, d_T21);
}

}  // namespace dfvo
