"""GPU: the keypoint-selection kernels (df-vo_amd/csrc/solver_kp.hip: k_kp_cell, k_kp_cell_rigid, k_bestn_select with
kp_introselect_block and sm::kp_introselect_cp_from underneath) on the inputs of tests/select_world.py -- adversarial keys
that exhaust introselect's depth limit (median of medians, recursive selection on the device), sorted / sawtooth /
organ-pipe / constant / two-valued keys with and without ties, +inf, -0.0, denormals, NaN, candidate counts at every
switch of the code, grids other than 10 x 10 -- bit for bit (kp1, kp2, n, good_kp_found) against T.local_bestN,
T.bestN_flow_kp and T.opt_rigid_flow_kp with the C oracle's argpartition.  No tolerance, no excluded case.

Stack: the three selection kernels have a dynamic stack because sm::kp_introselect_cp_from recurses through
kp_median_of_median5_cp.  The compiler's resource remarks (-Rpass-analysis=kernel-resource-usage, gfx950, -O3) give
112 bytes per lane and nesting level (96 for kp_introselect_cp_from + 16 for kp_introselect_cp), the `depth < 4` cap in
kp_select.h bounds the nesting at five levels = 560 bytes; the killers of this module reach level one (224 bytes).  The
runtime's per-lane stack limit (hipDeviceGetLimit(hipLimitStackSize)) is read first and must be >= 560 before any killer is
launched; it is never set from here.  Read on the MI355X test machine: 1024 bytes (HIP's documented default)."""
import ctypes as C

import numpy as np
import pytest

import select_world as S
from oracle import tracker_np as T

pytestmark = pytest.mark.gpu

ERR_ARG = -2
THRE = 0.1
STACK_NEEDED = 560  # 5 nesting levels x 112 bytes, see the module docstring


@pytest.fixture(scope="module")
def trk(gpu):
    lib = gpu.lib()
    t = C.c_void_p()
    gpu.check(lib.dfvo_tracker_create(None, C.byref(t)))
    yield t
    lib.dfvo_tracker_destroy(t)


def _hip_runtime():
    """the HIP runtime the process already has loaded (a query goes to that one, never to a second copy)"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no HIP runtime is loaded"
    return C.CDLL(paths[0])


@pytest.fixture(scope="module")
def stack_ok(gpu, trk):
    """the stack gate: the per-lane stack limit of the runtime, read and asserted before any killer case is launched"""
    hip = _hip_runtime()
    hip.hipDeviceGetLimit.restype = C.c_int
    hip.hipDeviceGetLimit.argtypes = [C.POINTER(C.c_size_t), C.c_int]
    v = C.c_size_t(0)
    rc = hip.hipDeviceGetLimit(C.byref(v), 0)  # hipLimitStackSize
    print("hipLimitStackSize: rc %d, %d bytes per lane" % (rc, v.value))
    assert rc == 0
    assert v.value >= STACK_NEEDED, "per-lane stack limit %d < %d: the recursive fallback may overrun it" % (v.value, STACK_NEEDED)
    return int(v.value)


def test_stack_limit_covers_the_recursive_fallback(stack_ok):
    assert stack_ok >= STACK_NEEDED


# ----------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------
def run_local(gpu, trk, flow, diff, nr, nc, num_bestN, thre=THRE, score=None):
    h, w = diff.shape
    kp1, kp2 = np.full((max(num_bestN, 1), 2), -7.0), np.full((max(num_bestN, 1), 2), -7.0)
    n, good = C.c_int(-7), C.c_int(-7)
    flow, diff = np.ascontiguousarray(flow), np.ascontiguousarray(diff)
    if score is None:
        rc = gpu.lib().dfvo_kp_local_bestn(trk, gpu.as_ptr(flow), gpu.as_ptr(diff), h, w, nr, nc, num_bestN, thre,
                                           gpu.as_ptr(kp1), gpu.as_ptr(kp2), C.byref(n), C.byref(good))
    else:
        rc = gpu.lib().dfvo_kp_local_bestn_ex(trk, gpu.as_ptr(flow), gpu.as_ptr(diff), h, w, nr, nc, num_bestN, thre, score,
                                              gpu.as_ptr(kp1), gpu.as_ptr(kp2), C.byref(n), C.byref(good))
    return rc, n.value, good.value, kp1, kp2


def check_local(gpu, trk, flow, diff, nr, nc, num_bestN, thre=THRE, score=None, must_be_good=True, tag=""):
    """one launch against the oracle; returns the number of keypoints"""
    ref = T.local_bestN(flow, diff[..., None], num_bestN=num_bestN, num_row=nr, num_col=nc, thre=thre,
                        score_method="flow_ratio" if score == 1 else "flow")
    rc, n, good, kp1, kp2 = run_local(gpu, trk, flow, diff, nr, nc, num_bestN, thre, score)
    gpu.check(rc)
    assert bool(good) == bool(ref["good_kp_found"]), tag
    if must_be_good:
        assert ref["good_kp_found"], "%s: the map does not pass local_bestN's gates, nothing would be compared" % tag
    if not ref["good_kp_found"]:
        return 0
    assert n == ref["kp1_best"].shape[1], tag
    assert np.array_equal(kp1[:n], ref["kp1_best"][0]), tag
    assert np.array_equal(kp2[:n], ref["kp2_best"][0]), tag
    return n


def pack(cases, h, w, nr, nc, thre=THRE, first_cell=0):
    """one map with case i in cell first_cell + i; odd cells get their candidates in the first pixels, even cells spread"""
    diff = S.blank_map(h, w, thre)
    for i, c in enumerate(cases):
        S.embed(c[1], h, w, nr, nc, first_cell + i, thre, raw=c[3], into=diff, spread=(i % 2 == 0))
    return diff


def images_of(cases, per_image):
    """deal the cases (sorted by count) round-robin, so that every image has long and short sequences: the gates pass"""
    cases = sorted(cases, key=lambda c: len(c[1]))
    n_img = -(-len(cases) // per_image)
    return [cases[i::n_img] for i in range(n_img)]


G34 = (120, 160, 3, 4)      # 39 x 39 = 1521-pixel cells, parallel selection (par = 1)
G11 = (120, 123, 1, 1)      # one 119 x 122 cell, cap 15250: the largest the parallel selection takes
G22 = (300, 320, 2, 2)      # 149 x 159 cells, cap 24624: single-lane selection (par = 0)


# ----------------------------------------------------------------------------------------------
# local_bestN
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_best", S.N_BEST)
def test_local_bestn_inventory_all_cells(gpu, trk, stack_ok, n_best):
    """every case of the inventory that fits a 3 x 4 cell, twelve per image (all cells), parallel selection"""
    h, w, nr, nc = G34
    flow = S.flow_for(h, w)
    cases = [c for c in S.cases() if c[2] == n_best and len(c[1]) <= S.cell_pixels(h, w, nr, nc, 0)]
    assert len(cases) >= 190
    total = 0
    for img in images_of(cases, nr * nc):
        total += check_local(gpu, trk, flow, pack(img, h, w, nr, nc), nr, nc, n_best * nr * nc, tag=",".join(c[0] for c in img))
    assert total == sum(min(n_best, len(S.selection_keys(c))) for c in cases)


def _one_cell_cases():
    names = {c[0]: c for c in S.cases()}
    keep = [c for c in S.cases() if c[0].startswith("killer") and len(c[1]) <= 1521]
    for n_best in (3, 20, 256):
        for kind in ("saw", "organ-ties", "ends", "two_lo", "const", "desc", "inf_zero_denorm", "nan"):
            for num in (257, 1000):
                keep.append(names["%s-%d-nb%d" % (kind, num, n_best)])
    return keep


def test_local_bestn_one_cell(gpu, trk, stack_ok):
    """killers (one shorter than 256 candidates: thread 0 alone walks into the fallback) and a sample of the structured and
    special cases in ONE cell of the 3 x 4 grid, noise in the others"""
    h, w, nr, nc = G34
    flow = S.flow_for(h, w, 1)
    cases = _one_cell_cases()
    assert any(c[0].startswith("killer") and len(c[1]) < 256 for c in cases)
    for i, c in enumerate(cases):
        cell = (5, 0, 11)[i % 3]
        diff = S.embed(c[1], h, w, nr, nc, cell, THRE, raw=c[3], spread=(i % 2 == 1), filler=300)
        check_local(gpu, trk, flow, diff, nr, nc, c[2] * nr * nc, tag=c[0])


def test_local_bestn_largest_parallel_cell(gpu, trk, stack_ok):
    """14 500 candidates in the one cell of a 1 x 1 grid (cap 15 250 of the 15 355 the parallel selection takes): killer and
    structured keys through many workgroup-parallel passes"""
    h, w, nr, nc = G11
    flow = S.flow_for(h, w, 2)
    cases = [c for c in S.cases() if len(c[1]) == S.BIG_PAR]
    assert len(cases) == 11 and any(c[0].startswith("killer") for c in cases)
    for i, c in enumerate(cases):
        diff = S.embed(c[1], h, w, nr, nc, 0, THRE, raw=c[3], spread=(i % 2 == 0))
        check_local(gpu, trk, flow, diff, nr, nc, c[2], tag=c[0])


def _single_lane_cases():
    big = [c for c in S.cases() if len(c[1]) == S.BIG_SEQ]
    small = [c for c in _one_cell_cases() if c[2] == 20]
    extra = [c for c in S.cases() if c[2] == 20 and len(c[1]) in (1, 2, 19, 20, 21, 255, 256) and ("ties" in c[0] or c[3])]
    return big, small + extra


def test_local_bestn_single_lane_selection(gpu, trk, stack_ok):
    """par = 0 (cells too large for the stopper lists in LDS): 2 x 2 on 300 x 320, the killer of 23 000 keys, long
    structured sequences and the short cases of the inventory, four per image"""
    h, w, nr, nc = G22
    flow = S.flow_for(h, w, 3)
    big, small = _single_lane_cases()
    assert len(big) == 11 and any(c[0].startswith("killer") for c in big)
    for n_best in (3, 20):
        for img in images_of([c for c in big if c[2] == n_best], 4):
            check_local(gpu, trk, flow, pack(img, h, w, nr, nc), nr, nc, n_best * 4, tag=",".join(c[0] for c in img))
    assert len(small) > 40
    for img in images_of(small, 4):
        check_local(gpu, trk, flow, pack(img, h, w, nr, nc), nr, nc, 20 * 4, tag=",".join(c[0] for c in img))


def _smooth_map(h, w, seed, levels=0):
    """a smooth consistency map (a cell read row by row is a sawtooth), most of it under the threshold"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    m = 0.06 + 0.05 * np.sin(x / 7.0 + rng.random() * 6) * np.cos(y / 5.0 + rng.random() * 6) + 0.01 * (x % 13) / 13.0
    if levels:
        m = np.floor(m * levels) / levels
    return m.astype(np.float32)


GRIDS = [  # h, w, rows, cols, n_best, must pass the gates (None: whatever the oracle says)
    (9, 11, 1, 1, 3, True), (40, 300, 1, 7, 20, True), (121, 163, 3, 4, 20, True), (100, 61, 7, 3, 2, True),
    (130, 170, 32, 32, 1, True), (200, 200, 2, 2, 256, True), (97, 89, 5, 6, 256, True), (10, 64, 7, 3, 1, True),
    (5, 64, 7, 3, 1, True), (3, 200, 10, 10, 2, True), (64, 5, 3, 7, 1, True), (4, 6, 9, 8, 1, None), (64, 64, 32, 32, 1, True),
    (2, 64, 7, 3, 1, None)]


@pytest.mark.parametrize("h,w,nr,nc,n_best,good", GRIDS)
def test_local_bestn_grids(gpu, trk, h, w, nr, nc, n_best, good):
    """grids other than 10 x 10: one cell, one row of cells, unequal rows and columns, 1024 cells (the size of k_kp_gather's
    LDS arrays), n_best 1 and 256, sides that the grid does not divide, cells of zero height, and fewer image rows (columns)
    than grid rows (columns): there the reference's slice end int(h / num_row * (row + 1)) - 1 is -1 for the first rows of
    cells, which numpy reads as "all but the last image row" -- those cells overlap and are not empty"""
    flow = S.flow_for(h, w, 4)
    for seed, levels in ((1, 0), (2, 9)):
        diff = _smooth_map(h, w, seed + h, levels)
        n = check_local(gpu, trk, flow, diff, nr, nc, n_best * nr * nc, must_be_good=bool(good), tag="%dx%d %dx%d" % (h, w, nr, nc))
        assert n > 0 or not good
    # no candidate anywhere: "not enough keypoints" on both sides
    assert check_local(gpu, trk, flow, S.blank_map(h, w, THRE), nr, nc, n_best * nr * nc, must_be_good=False) == 0


def test_local_bestn_flow_ratio_killer(gpu, trk, stack_ok):
    """score_method 'flow_ratio': the ratio map is what is ranked, so the consistency map is key * |flow| with power-of-two
    flow magnitudes -- the division is exact and the ranked keys are the killers'"""
    h, w, nr, nc = G34
    flow = S.flow_for(h, w, 5)
    mag = np.abs(flow[0]) + np.abs(flow[1])  # one component is zero
    cases = [c for c in S.cases() if c[0] in ("killer-1000-nb20", "killer-257-nb20", "killer-40-nb20", "killer-distinct-257-nb20")]
    assert len(cases) == 4
    keys = S.blank_map(h, w, THRE)
    rng = np.random.default_rng(5)
    for cell in range(nr * nc):
        if cell < 4:
            S.embed(cases[cell][1], h, w, nr, nc, cell, THRE, into=keys, spread=(cell % 2 == 0))
        else:
            S.embed(rng.permutation(60), h, w, nr, nc, cell, THRE, into=keys)
    diff = (keys * mag).astype(np.float32)
    assert np.array_equal((diff / mag).astype(np.float32), keys)
    n = check_local(gpu, trk, flow, diff, nr, nc, 20 * nr * nc, score=1, tag="flow_ratio killers")
    assert n == 20 * nr * nc


# ----------------------------------------------------------------------------------------------
# bestN_flow_kp
# ----------------------------------------------------------------------------------------------
def run_bestn(gpu, trk, flow, diff, N):
    h, w = diff.shape
    kp1, kp2 = np.full((N, 2), -7.0), np.full((N, 2), -7.0)
    n = C.c_int(-7)
    rc = gpu.lib().dfvo_kp_bestn(trk, gpu.as_ptr(np.ascontiguousarray(flow)), gpu.as_ptr(np.ascontiguousarray(diff)), h, w, N,
                                 gpu.as_ptr(kp1), gpu.as_ptr(kp2), C.byref(n))
    return rc, n.value, kp1, kp2


def check_bestn(gpu, trk, flow, diff, N, tag):
    rc, n, kp1, kp2 = run_bestn(gpu, trk, flow, diff, N)
    gpu.check(rc)
    with np.errstate(invalid="ignore"):
        cnt = int((diff >= 0).sum())
    if cnt <= N:  # numpy raises "kth out of bounds"; the C entry reports zero keypoints
        assert n == 0, tag
        return 0
    o1, o2 = T.bestN_flow_kp(flow, diff[..., None], N)
    assert n == N, tag
    assert np.array_equal(kp1, o1[0]) and np.array_equal(kp2, o2[0]), tag
    return n


BH, BW, BN = 60, 90, 300


def test_bestn_whole_image_sequences(gpu, trk, stack_ok):
    """the killer and the structured / special sequences as whole 60 x 90 images, N = 300 (every pixel a candidate: the
    identity path; int positions, two int scans)"""
    flow = S.flow_for(BH, BW, 6)
    n = BH * BW
    seqs = [("killer", S.killer(n, BN), False), ("killer-distinct", S.killer(n, BN, True), False)]
    seqs += [("%s%s" % (k, "-ties" if t else ""), S.structured(k, n, t, BW), False) for k in S.STRUCTURED for t in (False, True)]
    seqs.append(("inf_zero_denorm", S.special("inf_zero_denorm", n), True))
    for name, seq, raw in seqs:
        assert check_bestn(gpu, trk, flow, S.embed_image(seq, BH, BW, raw=raw), BN, name) == BN


def test_bestn_compaction_and_edge_counts(gpu, trk, stack_ok):
    """NaN and negative pixels force the ordered compaction, with the last candidate in the middle of a 256-chunk; cnt == N
    gives n = 0, cnt == N + 1 takes the find-max shortcut, cnt == N + 300 and a killer of 5000 candidates select"""
    flow = S.flow_for(BH, BW, 7)
    n = BH * BW
    assert n % 256 != 0
    for cnt in (BN, BN + 1, BN + 300):
        for kind in ("saw", "organ-ties", "const"):
            seq = S.structured(kind.split("-")[0], cnt, "ties" in kind, BW)
            got = check_bestn(gpu, trk, flow, S.embed_image(seq, BH, BW), BN, "%s cnt %d" % (kind, cnt))
            assert got == (0 if cnt == BN else BN)
    for seq, name in ((S.killer(5000, BN), "killer 5000"), (S.killer(601, BN), "killer 601")):
        holes = None
        if len(seq) == 601:  # every candidate in the first three chunks, the last one mid-chunk
            holes = np.r_[np.arange(0, 100), np.arange(701, n)]
        assert check_bestn(gpu, trk, flow, S.embed_image(seq, BH, BW, holes=holes), BN, name) == BN
    nan_img = S.special("nan", n).reshape(BH, BW)  # NaN interleaved with noise
    assert check_bestn(gpu, trk, flow, nan_img, BN, "nan") == BN


# ----------------------------------------------------------------------------------------------
# opt_rigid_flow_kp
# ----------------------------------------------------------------------------------------------
def run_rigid(gpu, trk, flow, odiff, rdiff, nr, nc, num_bestN, score, rigid_thre, opt_thre):
    h, w = odiff.shape
    cfg = gpu.RigidKpCfg(num_row=nr, num_col=nc, num_bestN=num_bestN, rigid_flow_thre=rigid_thre, optical_flow_thre=opt_thre,
                         score_method=1 if score == "rigid_flow" else 0)
    for i in range(9):
        cfg.K[i] = cfg.Kinv[i] = float(i % 4 == 0)
    for i in range(16):
        cfg.T_ref_to_cur[i] = float(i % 5 == 0)
    kps = [np.full((num_bestN, 2), -7.0) for _ in range(4)]
    n = C.c_int(-7)
    depth = np.ones((h, w), np.float32)
    rc = gpu.lib().dfvo_kp_rigid_flow(trk, gpu.as_ptr(np.ascontiguousarray(flow)), gpu.as_ptr(np.ascontiguousarray(odiff)),
                                      gpu.as_ptr(depth), h, w, C.byref(cfg), gpu.as_ptr(np.ascontiguousarray(rdiff)),
                                      gpu.as_ptr(kps[0]), gpu.as_ptr(kps[1]), gpu.as_ptr(kps[2]), gpu.as_ptr(kps[3]), C.byref(n), None)
    return rc, n.value, kps


@pytest.mark.parametrize("score", ["rigid_flow", "opt_flow"])
def test_rigid_flow_kp_killers(gpu, trk, stack_ok, score):
    """h_rigid_diff_override: killer keys in the rigid distance under score 'rigid_flow', in the flow distance otherwise;
    the OTHER map passes its threshold at the killer's pixels and fails it at half as many extra pixels that the scored
    map lets through (every third candidate of the first threshold goes: the compaction is not the identity).  "best" and
    "uniform" sets against the oracle."""
    h, w, nr, nc = G34
    rigid_thre, opt_thre = 0.5, THRE
    flow = S.flow_for(h, w, 8)
    names = ("killer-1000-nb20", "killer-257-nb20", "killer-40-nb20", "killer-300-nb20", "saw-1000-nb20", "organ-ties-257-nb20",
             "ends-257-nb20", "const-21-nb20", "asc-20-nb20", "desc-19-nb20", "two_lo-1-nb20", "inf_zero_denorm-1000-nb20")
    by_name = {c[0]: c for c in S.cases()}
    scored = pack([by_name[k] for k in names], h, w, nr, nc)          # candidates < 0.1, everything else 0.4
    other = np.zeros((h, w), np.float32)                               # passes everywhere ...
    rng = np.random.default_rng(8)
    for cell in range(nr * nc):
        y0, y1, x0, x1 = S.cell_bounds(h, w, nr, nc, cell // nc, cell % nc)
        tile_s, tile_o = scored[y0:y1, x0:x1], other[y0:y1, x0:x1]
        free = np.argwhere(~(tile_s < THRE))
        cnt = int((tile_s < THRE).sum())
        extra = free[np.sort(rng.choice(len(free), min(cnt // 2, len(free)), replace=False))]
        tile_s[extra[:, 0], extra[:, 1]] = (rng.integers(0, 4000, len(extra)) * S.KEY_STEP).astype(np.float32)
        tile_o[extra[:, 0], extra[:, 1]] = 1.0                         # ... but at the extra pixels
    rdiff, odiff = (scored, other) if score == "rigid_flow" else (other, scored)
    want = T.opt_rigid_flow_kp(flow, odiff[..., None], rdiff[..., None], score, num_bestN=20 * nr * nc, num_row=nr, num_col=nc,
                               rigid_thre=rigid_thre, opt_thre=opt_thre)
    rc, n, kps = run_rigid(gpu, trk, flow, odiff, rdiff, nr, nc, 20 * nr * nc, score, rigid_thre, opt_thre)
    gpu.check(rc)
    assert n == want["kp1_depth"].shape[1] and n > 150
    for got, key in zip(kps, ("kp1_depth", "kp2_depth", "kp1_depth_uniform", "kp2_depth_uniform")):
        assert np.array_equal(got[:n], want[key][0]), key


@pytest.mark.parametrize("h,w,nr,nc,n_best", [(121, 163, 3, 4, 20), (40, 300, 1, 7, 256), (5, 64, 7, 3, 1), (64, 5, 3, 7, 2), (130, 170, 32, 32, 1)])
def test_rigid_flow_kp_grids(gpu, trk, h, w, nr, nc, n_best):
    """opt_rigid_flow_kp on grids other than 10 x 10, cells wrapped by a negative slice end included; smooth maps"""
    flow = S.flow_for(h, w, 10)
    odiff, rdiff = _smooth_map(h, w, 20 + h, 9), (_smooth_map(h, w, 30 + w) * 4).astype(np.float32)
    for score in ("opt_flow", "rigid_flow"):
        want = T.opt_rigid_flow_kp(flow, odiff[..., None], rdiff[..., None], score, num_bestN=n_best * nr * nc, num_row=nr, num_col=nc,
                                   rigid_thre=0.3, opt_thre=THRE)
        rc, n, kps = run_rigid(gpu, trk, flow, odiff, rdiff, nr, nc, n_best * nr * nc, score, 0.3, THRE)
        gpu.check(rc)
        assert n == want["kp1_depth"].shape[1] and n > 0
        for got, key in zip(kps, ("kp1_depth", "kp2_depth", "kp1_depth_uniform", "kp2_depth_uniform")):
            assert np.array_equal(got[:n], want[key][0]), (score, key)


# ----------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------
def test_launcher_refusals_leave_the_tracker_usable(gpu, trk):
    """more than 1024 cells, num_bestN below the cell count (n_best 0), n_best 257 and a cell too large for LDS return the
    argument error, write nothing to the outputs, and the next call on the same handle still matches the oracle"""
    h, w = 120, 160
    flow, diff = S.flow_for(h, w, 9), _smooth_map(h, w, 9)
    big_flow, big_diff = S.flow_for(300, 320, 9), _smooth_map(300, 320, 10)
    refused = [(flow, diff, 25, 41, 2000), (flow, diff, 3, 4, 11), (flow, diff, 3, 4, 257 * 12), (big_flow, big_diff, 1, 1, 20)]
    for f, d, nr, nc, num_bestN in refused:
        rc, n, good, kp1, kp2 = run_local(gpu, trk, f, d, nr, nc, num_bestN)
        assert rc == ERR_ARG, (nr, nc, num_bestN, rc)
        assert gpu.lib().dfvo_last_error()
        assert n == -7 and good == -7 and (kp1 == -7.0).all() and (kp2 == -7.0).all()
        assert check_local(gpu, trk, flow, diff, 3, 4, 240, tag="after a refusal") > 0
    # the rigid-flow launcher has the same limits
    for nr, nc, num_bestN in ((25, 41, 2000), (3, 4, 11), (3, 4, 257 * 12)):
        rc, n, kps = run_rigid(gpu, trk, flow, diff, diff, nr, nc, num_bestN, "opt_flow", 0.5, THRE)
        assert rc == ERR_ARG and n == -7 and all((k == -7.0).all() for k in kps), (nr, nc, num_bestN, rc)
    want = T.opt_rigid_flow_kp(flow, diff[..., None], diff[..., None], "opt_flow", num_bestN=240, num_row=3, num_col=4, rigid_thre=0.5,
                               opt_thre=THRE)
    rc, n, kps = run_rigid(gpu, trk, flow, diff, diff, 3, 4, 240, "opt_flow", 0.5, THRE)
    gpu.check(rc)
    assert n == want["kp1_depth"].shape[1] > 0 and np.array_equal(kps[0][:n], want["kp1_depth"][0])
    assert np.array_equal(kps[3][:n], want["kp2_depth_uniform"][0])
