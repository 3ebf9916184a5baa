// Lifetime of the solver chain's buffer sets (solver.h, tracker.h): allocation, the tracker's side streams and events, its
// stage-timing marks.  Host code only: this unit also builds as plain C++ (tests/host_harness/solver_buffers_check.cpp).
// Every ensure() frees first and allocates then (peak memory stays that of the larger set), each dimension grows to the
// maximum of its old value and the request, a request that fits makes no HIP call, and a failed one leaves the set empty.
#include "tracker.h"

namespace dfvo {

int RansacWorkspace::ensure(int n, int max_iters) {
    if (n <= cap_n && max_iters <= cap_iters) return DFVO_OK;
    const size_t cn = n > cap_n ? n : cap_n, it = max_iters > cap_iters ? max_iters : cap_iters;
    release();
    if (state.alloc(1) || pts_a.alloc(2 * cn) || pts_b.alloc(2 * cn) || norm_a.alloc(2 * cn) || norm_b.alloc(2 * cn) ||
        f_a.alloc(2 * cn) || f_b.alloc(2 * cn) || idx.alloc(5 * it) || ws.alloc(E_WS * it) || ok.alloc(it) ||
        models.alloc(90 * it) || nmodels.alloc(it) || counts.alloc(10 * it) || mask.alloc(cn) || out.alloc(64) ||
        lm.alloc(20 * cn + 512) || cidx.alloc(cn + 16)) {
        release();
        return DFVO_ERR_HIP;
    }
    cap_n = (int)cn;
    cap_iters = (int)it;
    return DFVO_OK;
}

void RansacWorkspace::release() {
    for (DevArr<double>* a : {&pts_a, &pts_b, &norm_a, &norm_b, &ws, &models, &out, &lm}) a->release();
    for (DevArr<int>* a : {&idx, &ok, &nmodels, &counts, &cidx}) a->release();
    state.release(), f_a.release(), f_b.release(), mask.release();
    cap_n = cap_iters = 0;
}

int PnpBuffers::ensure(int n, int iters) {
    if (n <= cap && iters <= iters_cap) return DFVO_OK;
    const size_t c = n > cap ? n : cap, it = iters > iters_cap ? iters : iters_cap, R = MAX_REP;
    release();
    if (info.alloc(4) || fk1.alloc(2 * c) || fk2.alloc(2 * c) || xyz.alloc(3 * c) || perm.alloc(R * (c + 8)) ||
        obj.alloc(R * 3 * c) || img.alloc(R * 2 * c) || state.alloc(R) || idx.alloc(5 * it) || models.alloc(R * 6 * it) ||
        nmodels.alloc(R * it) || counts.alloc(R * it) || mask.alloc(R * c) || keep.alloc(c) || pts5.alloc(R * 5 * c) ||
        rep_out.alloc(R) || result.alloc(1)) {
        release();
        return DFVO_ERR_HIP;
    }
    cap = (int)c;
    iters_cap = (int)it;
    return DFVO_OK;
}

void PnpBuffers::release() {
    for (DevArr<int>* a : {&info, &perm, &idx, &nmodels, &counts}) a->release();
    for (DevArr<double>* a : {&fk1, &fk2, &xyz, &models}) a->release();
    for (DevArr<float>* a : {&obj, &img, &pts5}) a->release();
    state.release(), mask.release(), keep.release(), rep_out.release(), result.release();
    cap = iters_cap = 0;
}

int BestNBuffers::ensure(size_t px, int N) {
    int rc = DFVO_OK;
    if (px > cap) {
        for (DevArr<int>* a : {&tosort, &map, &Lpos, &Rpos, &count}) a->release();
        // key_base: 16 floats of slack, the 4-wide scans over-read
        if (key_base.alloc(px + 16) || tosort.alloc(px) || map.alloc(px) || Lpos.alloc(px + 2) || Rpos.alloc(px + 2) ||
            count.alloc(4))
            rc = DFVO_ERR_HIP;
        else if (hipError_t e = hipMemset(key_base, 0, sizeof(float) * (px + 16))) {
            set_last_error(std::string("BestNBuffers::ensure: hipMemset: ") + hipGetErrorString(e));
            rc = DFVO_ERR_HIP;
        }
        cap = px;
    }
    if (!rc) rc = kp.grow(4 * (size_t)N);
    if (rc) release();
    return rc;
}

void BestNBuffers::release() {
    for (DevArr<int>* a : {&tosort, &map, &Lpos, &Rpos, &count}) a->release();
    key_base.release(), kp.release();
    cap = 0;
}

int RigidKpBuffers::ensure(int H, int W, int cells, int n_best, int cap) {
    const size_t px = (size_t)H * W, sel = (size_t)cells * n_best;
    int rc = DFVO_OK;
    if (px > depth32.n) {
        rdiff.release();
        rc = depth32.alloc(px) || rdiff.alloc(2 * px) ? DFVO_ERR_HIP : DFVO_OK;
    }
    if (!rc && !mats) {
        if (mats.alloc(40) || ctl.alloc(1) || cell_count.alloc(1024) || info.alloc(8) || zero.alloc(2))
            rc = DFVO_ERR_HIP;
        else if (hipError_t e = hipMemset(zero, 0, sizeof(int) * 2)) {
            set_last_error(std::string("RigidKpBuffers::ensure: hipMemset: ") + hipGetErrorString(e));
            rc = DFVO_ERR_HIP;
        }
    }
    if (!rc && sel > (size_t)sel_cap) {
        cell_sel_uni.release(), kp.release();
        rc = cell_sel.alloc(sel) || cell_sel_uni.alloc(sel) || kp.alloc(8 * sel) ? DFVO_ERR_HIP : DFVO_OK;
        sel_cap = (int)sel;
    }
    if (!rc) rc = lidx.grow((size_t)cells * cap);
    if (rc) release();
    return rc;
}

void RigidKpBuffers::release() {
    for (DevArr<int>* a : {&cell_count, &cell_sel, &cell_sel_uni, &info, &zero}) a->release();
    depth32.release(), rdiff.release(), mats.release(), ctl.release(), lidx.release(), kp.release();
    sel_cap = 0;
}

int TrackerBuffers::ensure_kp(int cap, int cells, int n_best) {
    if (cap <= kp_cap && cells * n_best <= sel_cap) return DFVO_OK;
    const size_t kc = cap > kp_cap ? cap : kp_cap, sc = cells * n_best > sel_cap ? cells * n_best : sel_cap, R = MAX_REP;
    release_kp();
    if (kp_ref.alloc(2 * kc) || kp_cur.alloc(2 * kc) || pa.alloc(2 * kc * R) || pb.alloc(2 * kc * R) ||
        perm.alloc((kc + 8) * R) || res.alloc(kc * (R + 1)) || best_inliers.alloc(kc + 8) || cell_count.alloc(1024) ||
        cell_sel.alloc(sc) || z2.alloc(kc) || pix.alloc(kc) ||
        ratios.alloc(kc * 3) ||  // ratio | triangulated | CNN depth lists
        inl_a.alloc(kc + 8) || inl_b.alloc(kc + 8) || scratch.alloc(kc + 8)) {
        release_kp();
        return DFVO_ERR_HIP;
    }
    kp_cap = (int)kc;
    sel_cap = (int)sc;
    return DFVO_OK;
}

void TrackerBuffers::release_kp() {
    for (DevArr<double>* a : {&kp_ref, &kp_cur, &pa, &pb, &res, &z2, &ratios}) a->release();
    for (DevArr<int>* a : {&perm, &cell_count, &cell_sel, &pix, &scratch}) a->release();
    best_inliers.release(), inl_a.release(), inl_b.release();
    kp_cap = sel_cap = 0;
}

int TrackerBuffers::init_own() {
    if (kp_info.alloc(8) || kp_total.alloc(KPT_SIZE) || pose.alloc(1) || small.alloc(SMALL_SIZE) || scale_out.alloc(1))
        return DFVO_ERR_HIP;
    DFVO_HIP_CHECK(hipMemset(kp_info, 0, sizeof(int) * 8));
    DFVO_HIP_CHECK(hipEventCreateWithFlags(&ev_start, hipEventDisableTiming));
    DFVO_HIP_CHECK(hipEventCreateWithFlags(&ev_h, hipEventDisableTiming));
    return DFVO_OK;
}

int TrackerBuffers::init(hipStream_t rep0, hipStream_t rep1, bool borrowed) {
    DFVO_ARG_CHECK(!borrowed || rep0, "TrackerBuffers::init: borrowed side streams have to be given");
    if (int rc = mt_own.alloc((size_t)MT_SNAP_STRIDE * (MAX_REP + 2))) return rc;  // the state + its snapshots (mt_snapshots)
    mt_state = mt_own;
    if (int rc = init_own()) return rc;
    // Side streams: [0] runs the five-point batch, [1] the scale stage's fills; the slots past `n_streams` alias them.
    // How many streams are CREATED here matters although only two are used: the hardware queue a stream gets (and with it
    // the compute pipe that dispatches it) follows the creation order, the fused pipeline creates its two prefetch
    // streams after these, and the pair rate depends on which pipes the prefetch chain shares with the flow nets / the
    // RNG-dependent solver chain.  Measured on MI355X, bench.py order (pipeline created before the process touches the
    // GPU through torch), exact fp32: 2 -> 103, 3 -> 108, 4 -> 133, 5 -> 111, 6 -> 112, 7 -> 116, 8 -> 133 frames/s;
    // with a torch copy issued first the fast settings are 5 .. 7 (126).  DFVO_REP_STREAMS overrides (tuning aid).
    // (The fused pipeline no longer depends on this: it measures which streams share a pipe and passes rep0 / rep1 in,
    // stream_pool.hip.)
    // rep0 / rep1 may be one stream, and with `borrowed` the stream of the chain itself (the fused pipeline's lane layout): a
    // side stream then runs its work in the chain's own order, and the waits between the two are satisfied by stream order.
    const int n_streams = rep0 ? 2 : rep_stream_count();
    n_rep_owned = borrowed ? 0 : n_streams;
    for (int r = 0; r < MAX_REP; r++) {
        if (rep0 && r < 2)
            s_rep[r] = r == 0 ? rep0 : (rep1 ? rep1 : rep0);
        else if (r < n_streams)
            DFVO_HIP_CHECK(create_solver_stream(&s_rep[r], 2));
        else
            s_rep[r] = s_rep[r % n_streams];
        DFVO_HIP_CHECK(hipEventCreateWithFlags(&ev_rep[r], hipEventDisableTiming));
    }
    DFVO_HIP_CHECK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    return DFVO_OK;
}

int TrackerBuffers::rebind_streams(hipStream_t rep0, hipStream_t rep1, bool borrowed) {
    DFVO_ARG_CHECK(!shared && rep0 && rep1, "TrackerBuffers::rebind_streams: bad argument");
    DFVO_HIP_CHECK(hipDeviceSynchronize());
    for (int r = 0; r < n_rep_owned && r < MAX_REP; r++)
        if (s_rep[r] && !(r == 1 && s_rep[1] == s_rep[0])) (void)hipStreamDestroy(s_rep[r]);
    n_rep_owned = borrowed ? 0 : 2;  // (release() destroys an aliased pair once)
    for (int r = 0; r < MAX_REP; r++) s_rep[r] = (r & 1) ? rep1 : rep0;
    return DFVO_OK;
}

int TrackerBuffers::init_shared(const TrackerBuffers& first) {
    shared = true;
    mt_state = first.mt_state;
    for (int r = 0; r < MAX_REP; r++) {
        s_rep[r] = first.s_rep[r];
        ev_rep[r] = first.ev_rep[r];
    }
    ev_fork = first.ev_fork;
    return init_own();
}

void TrackerBuffers::release() {
    release_kp();
    ws_h.release();
    ws_e.release();
    const bool aliased = s_rep[1] == s_rep[0];  // an owned pair that is one stream is destroyed once
    for (int r = 0; r < MAX_REP; r++) {
        ws_rep[r].release();
        if (!shared) {
            if (s_rep[r] && r < n_rep_owned && !(r == 1 && aliased)) (void)hipStreamDestroy(s_rep[r]);
            if (ev_rep[r]) (void)hipEventDestroy(ev_rep[r]);
        }
        s_rep[r] = nullptr;
        ev_rep[r] = nullptr;
    }
    if (ev_fork && !shared) (void)hipEventDestroy(ev_fork);
    if (ev_start) (void)hipEventDestroy(ev_start);
    if (ev_h) (void)hipEventDestroy(ev_h);
    ev_fork = ev_start = ev_h = nullptr;
    for (int i = 0; i < N_EV_T; i++) {
        if (ev_t[i]) (void)hipEventDestroy(ev_t[i]);
        ev_t[i] = nullptr;
    }
    for (int i = 0; i < N_SEG; i++) {
        if (ev_seg[i]) (void)hipEventDestroy(ev_seg[i]);
        ev_seg[i] = nullptr;
    }
    mt_state = nullptr;
    small_valid = false;
    mt_own.release(), kp_info.release(), kp_total.release(), pose.release(), small.release(), scale_out.release();
    winner.release(), lidx.release(), ratio_map.release();
}

int TrackerBuffers::enable_stage_timing() {
    for (int i = 0; i < N_SEG; i++)
        if (!ev_seg[i]) DFVO_HIP_CHECK(hipEventCreate(&ev_seg[i]));
    return DFVO_OK;
}
int TrackerBuffers::mark(int i, hipStream_t s) {
    if (!ev_seg[i]) return DFVO_OK;
    DFVO_HIP_CHECK(hipEventRecord(ev_seg[i], s));
    seg_mask |= 1u << i;
    return DFVO_OK;
}

}  // namespace dfvo
