// Lifetime of TrackerBuffers (tracker.h): allocation, side streams and events, stage-timing marks.  Host code only.
#include "tracker.h"

namespace dfvo {

int TrackerBuffers::ensure_kp(int cap, int cells, int n_best) {
    if (cap <= kp_cap && cells * n_best <= sel_cap) return DFVO_OK;
    release_kp();
    kp_cap = cap > kp_cap ? cap : kp_cap;
    sel_cap = cells * n_best > sel_cap ? cells * n_best : sel_cap;
    DFVO_HIP_CHECK(hipMalloc((void**)&kp_ref, sizeof(double) * 2 * kp_cap));
    DFVO_HIP_CHECK(hipMalloc((void**)&kp_cur, sizeof(double) * 2 * kp_cap));
    DFVO_HIP_CHECK(hipMalloc((void**)&pa, sizeof(double) * 2 * kp_cap * MAX_REP));
    DFVO_HIP_CHECK(hipMalloc((void**)&pb, sizeof(double) * 2 * kp_cap * MAX_REP));
    DFVO_HIP_CHECK(hipMalloc((void**)&perm, sizeof(int) * (size_t)(kp_cap + 8) * MAX_REP));
    DFVO_HIP_CHECK(hipMalloc((void**)&res, sizeof(double) * kp_cap * (MAX_REP + 1)));
    DFVO_HIP_CHECK(hipMalloc((void**)&best_inliers, kp_cap + 8));
    DFVO_HIP_CHECK(hipMalloc((void**)&cell_count, sizeof(int) * 1024));
    DFVO_HIP_CHECK(hipMalloc((void**)&cell_sel, sizeof(int) * sel_cap));
    DFVO_HIP_CHECK(hipMalloc((void**)&z2, sizeof(double) * kp_cap));
    DFVO_HIP_CHECK(hipMalloc((void**)&pix, sizeof(int) * kp_cap));
    DFVO_HIP_CHECK(hipMalloc((void**)&ratios, sizeof(double) * kp_cap * 3));  // ratio | triangulated | CNN depth lists
    DFVO_HIP_CHECK(hipMalloc((void**)&inl_a, kp_cap + 8));
    DFVO_HIP_CHECK(hipMalloc((void**)&inl_b, kp_cap + 8));
    DFVO_HIP_CHECK(hipMalloc((void**)&scratch, sizeof(int) * (kp_cap + 8)));
    return DFVO_OK;
}

void TrackerBuffers::release_kp() {
    void* ptrs[] = {kp_ref, kp_cur, pa, pb, perm, res, best_inliers, cell_count, cell_sel, z2, pix, ratios, inl_a, inl_b, scratch};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    kp_ref = kp_cur = pa = pb = res = z2 = ratios = nullptr;
    perm = cell_count = cell_sel = pix = scratch = nullptr;
    best_inliers = inl_a = inl_b = nullptr;
    kp_cap = sel_cap = 0;
}

int TrackerBuffers::init_own() {
    DFVO_HIP_CHECK(hipMalloc((void**)&kp_info, sizeof(int) * 8));
    DFVO_HIP_CHECK(hipMalloc((void**)&kp_total, sizeof(int) * KPT_SIZE));
    DFVO_HIP_CHECK(hipMalloc((void**)&pose, sizeof(PoseState)));
    DFVO_HIP_CHECK(hipMalloc((void**)&small, sizeof(double) * SMALL_SIZE));
    DFVO_HIP_CHECK(hipMalloc((void**)&scale_out, sizeof(ScaleResult)));
    DFVO_HIP_CHECK(hipMemset(kp_info, 0, sizeof(int) * 8));
    DFVO_HIP_CHECK(hipEventCreateWithFlags(&ev_start, hipEventDisableTiming));
    DFVO_HIP_CHECK(hipEventCreateWithFlags(&ev_h, hipEventDisableTiming));
    return DFVO_OK;
}

int TrackerBuffers::init(hipStream_t rep0, hipStream_t rep1, bool borrowed) {
    DFVO_ARG_CHECK(!borrowed || rep0, "TrackerBuffers::init: borrowed side streams have to be given");
    DFVO_HIP_CHECK(hipMalloc((void**)&mt_state, sizeof(uint32_t) * MT_SNAP_STRIDE * (MAX_REP + 2)));  // the state + its snapshots (mt_snapshots)
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
    for (int r = 0; r < MAX_REP; r++) {
        ws_rep[r].release();
        if (!shared) {
            if (s_rep[r] && r < n_rep_owned && !(r == 1 && s_rep[1] == s_rep[0])) (void)hipStreamDestroy(s_rep[r]);
            if (ev_rep[r]) (void)hipEventDestroy(ev_rep[r]);
        }
        s_rep[r] = nullptr;
        ev_rep[r] = nullptr;
    }
    if (ev_fork && !shared) (void)hipEventDestroy(ev_fork);
    if (ev_start) (void)hipEventDestroy(ev_start);
    if (ev_h) (void)hipEventDestroy(ev_h);
    ev_fork = ev_start = ev_h = nullptr;
    for (int i = 0; i < 4; i++) {
        if (ev_t[i]) (void)hipEventDestroy(ev_t[i]);
        ev_t[i] = nullptr;
    }
    for (int i = 0; i < N_SEG; i++) {
        if (ev_seg[i]) (void)hipEventDestroy(ev_seg[i]);
        ev_seg[i] = nullptr;
    }
    if (shared) mt_state = nullptr;
    small_valid = false;
    if (ratio_map) (void)hipFree(ratio_map);
    ratio_map = nullptr;
    ratio_cap = 0;
    void* ptrs[] = {mt_state, kp_info, kp_total, pose, small, scale_out, winner, lidx};
    lidx = nullptr;
    lidx_cap = 0;
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    mt_state = nullptr;
    kp_info = kp_total = winner = nullptr;
    pose = nullptr;
    small = nullptr;
    scale_out = nullptr;
    winner_cap = 0;
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
