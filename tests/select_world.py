"""Case inventory of the keypoint-selection tests (tests/test_oracle_tracker.py, test_host_lanes.py,
test_kp_select_cpu.py, test_kp_select_gpu.py): key sequences on which numpy's introselect goes wrong easily, and the
maps that put such a sequence into one grid cell of local_bestN / opt_rigid_flow_kp or over the image of bestN_flow_kp.
Pure numpy, deterministic.

killer(num, kth)   a McIlroy adversary ("A killer adversary for quicksort", 1999) run against the oracle's pure-Python
                   introselect through its comparison: undecided ("gas") keys compare SMALLER than every frozen key --
                   the mirror image of the paper, because kth is small and the selection follows the low side -- and
                   the key about to become the pivot is frozen just below all frozen ones.  Every median-of-three pass
                   then peels a constant number of keys off the top, the depth limit 2*floor(log2 num) runs out with
                   most of the range left, and the selection enters its median-of-medians branch.
structured(...)    sorted, reversed, sawtooth (a smooth map read row by row through a cell), organ pipe, constant,
                   two-valued, all-equal-but-the-ends; each also quantised to a few levels (heavy ties)
special(...)       +inf, -0.0 / +0.0, denormals, NaN
embed(...)         keys -> consistency map
CASES              the cross product the CPU lanes run in full; the GPU tests pack it into a few images
"""
import functools

import numpy as np

from oracle import tracker_np as T

KEY_STEP = 2.0 ** -20   # dense rank r -> key r * 2^-20: exact in float32, order and ties kept, < 0.1 for r < 104857
CELL_ROW = 39           # candidates per row of a 3 x 4 cell on 120 x 160: the sawtooth period


# ----------------------------------------------------------------------------------------------
# adversary
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _killer(num, kth, distinct_gas):
    gas = num + 1                      # "undecided": below every frozen value once the run is over
    val = [gas] * num
    state = {"next": num, "cand": -1}  # frozen values count DOWN: the next pivot lands below the frozen ones

    def freeze(i):
        val[i] = state["next"]
        state["next"] -= 1

    def lt(a, b):  # a, b: item numbers
        if val[a] == gas and val[b] == gas:
            freeze(a if a == state["cand"] else b)
        if val[a] == gas:
            state["cand"] = a
        elif val[b] == gas:
            state["cand"] = b
        va = -1 if val[a] == gas else val[a]
        vb = -1 if val[b] == gas else val[b]
        return va < vb

    saved = T._lt
    T._lt = lt
    try:
        T._introselect(list(range(num)), list(range(num)), 0, num, kth)
    finally:
        T._lt = saved
    out = np.asarray(val, np.float64)
    still = out == gas
    if distinct_gas:
        rng = np.random.default_rng(num * 7919 + kth)
        out[still] = -1.0 - rng.permutation(int(still.sum()))
    else:
        out[still] = -1.0
    out = (out - out.min()).astype(np.float32)  # small non-negative integers: exact
    before = T.FALLBACK_ENTRIES[0]
    T.argpartition_scalar(out, kth)
    entries = T.FALLBACK_ENTRIES[0] - before
    assert entries >= 1, "killer(%d, %d) did not reach the median-of-medians branch" % (num, kth)
    out.setflags(write=False)
    return out, entries


def killer(num, kth, distinct_gas=False):
    """float32 keys of length num on which introselect(kth) exhausts its depth limit (asserted by a replay)"""
    assert 3 <= kth < num - 1
    return _killer(int(num), int(kth), bool(distinct_gas))[0]


def killer_entries(num, kth, distinct_gas=False):
    """how often the replay of killer(...) entered the median-of-medians branch"""
    return _killer(int(num), int(kth), bool(distinct_gas))[1]


# ----------------------------------------------------------------------------------------------
# structured and special sequences
# ----------------------------------------------------------------------------------------------
STRUCTURED = ("asc", "desc", "saw", "organ", "const", "two_lo", "two_hi", "ends")


def structured(kind, num, ties=False, period=CELL_ROW):
    i = np.arange(num, dtype=np.float64)
    if kind == "asc":
        s = i
    elif kind == "desc":
        s = num - 1 - i
    elif kind == "saw":          # ramps along a row, drifts from row to row
        s = (i % period) * 64 + (i // period)
    elif kind == "organ":
        s = np.minimum(i, num - 1 - i)
    elif kind == "const":
        s = np.zeros(num)
    elif kind == "two_lo":       # a few small keys among equal large ones
        s = np.ones(num)
        s[::7] = 0
    elif kind == "two_hi":
        s = np.zeros(num)
        s[::7] = 1
    elif kind == "ends":         # everything equals the median-of-three pivot except the two ends
        s = np.full(num, 5.0)
        s[0], s[-1] = 0.0, 9.0
    else:
        raise ValueError(kind)
    if ties:
        top = max(float(s.max()), 1.0)
        s = np.floor(s * (6.0 / top))   # seven levels
    return s.astype(np.float32)


SPECIAL = ("inf_zero_denorm", "nan")


def special(kind, num, seed=0):
    """raw float32 keys (embed(..., raw=True)); every finite one lies in [0, 0.05)"""
    rng = np.random.default_rng(1000 + seed + num)
    s = (rng.random(num) * 0.05).astype(np.float32)
    if kind == "inf_zero_denorm":
        pick = rng.integers(0, 6, num)
        s[pick == 0] = np.float32(0.0)
        s[pick == 1] = np.float32(-0.0)
        den = (rng.integers(1, 40, num).astype(np.uint32)).view(np.float32)  # 1 .. 39 units of 2^-149
        s[pick == 2] = den[pick == 2]
        s[::11] = np.inf
    elif kind == "nan":
        s[::3] = np.nan
        s[1::10] = np.nan
        if num > 4:
            s[-2] = np.nan
    else:
        raise ValueError(kind)
    return s


def rank_keys(seq):
    """dense rank * 2^-20: order and ties of seq, exactly representable, inside [0, 0.1)"""
    _, inv = np.unique(np.asarray(seq), return_inverse=True)
    assert inv.max() * KEY_STEP < 0.1
    return (inv.astype(np.float64) * KEY_STEP).astype(np.float32)


# ----------------------------------------------------------------------------------------------
# maps
# ----------------------------------------------------------------------------------------------
def cell_bounds(h, w, num_row, num_col, row, col):
    """the oracle's (= the reference's) expressions"""
    return (int(h / num_row * row), int(h / num_row * (row + 1)) - 1, int(w / num_col * col), int(w / num_col * (col + 1)) - 1)


def cell_pixels(h, w, num_row, num_col, cell):
    y0, y1, x0, x1 = cell_bounds(h, w, num_row, num_col, cell // num_col, cell % num_col)
    return len(range(h)[y0:y1]) * len(range(w)[x0:x1])  # slices, as the reference takes them (an end of -1 wraps)


def blank_map(h, w, thre):
    """no candidate anywhere"""
    return np.full((h, w), np.float32(4.0 * thre), np.float32)


def embed(seq, h, w, num_row, num_col, cell, thre, raw=False, into=None, spread=True, filler=40):
    """Consistency map [h, w] float32 whose cell `cell`, read row-major, has exactly the keys `seq` as its candidates (in
    that order), every other pixel of that cell >= thre.  Keys are the dense ranks of seq unless raw.  With into=None the
    other cells get `filler` noise candidates each so that the mask.sum() and region gates of local_bestN pass; with
    into=<map> only the one cell is written.  spread: the candidates are scattered over the cell (the compaction is not
    the identity) instead of filling its first pixels."""
    keys = np.asarray(seq, np.float32) if raw else rank_keys(seq)
    if into is None:
        out = blank_map(h, w, thre)
        rng = np.random.default_rng(h * 1000 + w)
        for c in range(num_row * num_col):
            n = min(filler, cell_pixels(h, w, num_row, num_col, c))
            if c != cell and n:
                embed(rng.permutation(n), h, w, num_row, num_col, c, thre, into=out)
    else:
        out = into
    y0, y1, x0, x1 = cell_bounds(h, w, num_row, num_col, cell // num_col, cell % num_col)
    th, tw = len(range(h)[y0:y1]), len(range(w)[x0:x1])
    total = th * tw
    assert len(keys) <= total, "cell %d has %d pixels, %d keys" % (cell, total, len(keys))
    if spread and len(keys):
        pos = np.floor(np.arange(len(keys)) * (total / len(keys))).astype(np.int64)  # strictly increasing
    else:
        pos = np.arange(len(keys))
    tile = np.full(total, np.float32(4.0 * thre), np.float32)
    tile[pos] = keys
    # (a raw key that is no candidate -- inf, NaN -- stays where it is: it must not disturb the order of the others)
    out[y0:y0 + th, x0:x0 + tw] = tile.reshape(th, tw)
    return out


def embed_image(seq, h, w, raw=False, holes=None):
    """bestN_flow_kp map [h, w]: the candidates (>= 0), row-major, are `seq`; the h*w - len(seq) other pixels alternate
    between NaN and -1 and are spread evenly unless `holes` gives their flat positions"""
    keys = np.asarray(seq, np.float32) if raw else rank_keys(seq)
    n = h * w
    assert len(keys) <= n
    out = np.empty(n, np.float32)
    nh = n - len(keys)
    if holes is None:
        holes = np.floor(np.arange(nh) * (n / max(nh, 1))).astype(np.int64)
    is_hole = np.zeros(n, bool)
    is_hole[holes] = True
    assert is_hole.sum() == nh
    out[~is_hole] = keys
    fill = np.full(nh, -1.0, np.float32)
    fill[::2] = np.nan
    out[is_hole] = fill
    return out.reshape(h, w)


def flow_for(h, w, seed=0):
    """flow [2, h, w] with power-of-two magnitudes along one axis (|flow| is exact), signs and axes mixed"""
    rng = np.random.default_rng(77 + seed)
    mag = (2.0 ** rng.integers(-1, 3, (h, w))).astype(np.float32) * rng.choice([-1.0, 1.0], (h, w)).astype(np.float32)
    axis = rng.integers(0, 2, (h, w))
    flow = np.zeros((2, h, w), np.float32)
    flow[0] = np.where(axis == 0, mag, 0)
    flow[1] = np.where(axis == 1, mag, 0)
    return flow


# ----------------------------------------------------------------------------------------------
# the inventory
# ----------------------------------------------------------------------------------------------
COUNTS = (1, 2, 3, 19, 20, 21, 255, 256, 257, 1000)
N_BEST = (1, 2, 3, 20, 256)
BIG_PAR = 14500          # fits the 119 x 122 cell of a 1 x 1 grid on 120 x 123 (cap 15250 <= 15355: parallel selection)
BIG_SEQ = 23000          # fits a 149 x 159 cell of a 2 x 2 grid on 300 x 320 (cap 24624: single-lane selection)
KILLERS = ((40, 19), (255, 19), (256, 19), (257, 19), (300, 19), (1000, 19), (1000, 255), (2000, 255), (BIG_PAR, 19),
           (BIG_SEQ, 19))
KILLERS_DISTINCT = ((257, 19), (1000, 255))


def _cases():
    out = []
    counts = COUNTS + tuple(n + d for n in N_BEST for d in (0, 1))  # cnt == n_best, cnt == n_best + 1
    counts = tuple(sorted(set(counts)))
    for n_best in N_BEST:
        for num in counts:
            for kind in STRUCTURED:
                for ties in (False, True):
                    out.append(("%s%s-%d-nb%d" % (kind, "-ties" if ties else "", num, n_best), structured(kind, num, ties), n_best, False))
            for kind in SPECIAL:
                out.append(("%s-%d-nb%d" % (kind, num, n_best), special(kind, num), n_best, True))
    for n_best in (3, 20):
        for kind in ("saw", "organ", "two_lo", "ends", "desc"):
            for num in (BIG_PAR, BIG_SEQ):
                out.append(("%s-%d-nb%d" % (kind, num, n_best), structured(kind, num, False, 122 if num == BIG_PAR else 159), n_best, False))
    return out


_STATIC = _cases()


def killer_cases():
    """(name, keys, n_best, raw) of every killer; generated on first use (pure Python, cached for the process)"""
    out = [("killer-%d-nb%d" % (num, kth + 1), killer(num, kth), kth + 1, False) for num, kth in KILLERS]
    out += [("killer-distinct-%d-nb%d" % (num, kth + 1), killer(num, kth, True), kth + 1, False) for num, kth in KILLERS_DISTINCT]
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """CASES: (name, float32 keys, n_best, raw).  A selection of n_best out of len(keys): kth = min(n_best, len) - 1."""
    return tuple(_STATIC + killer_cases())


def selection_keys(case):
    """what the device ranks for a case: its dense-rank keys, or the raw ones without the non-candidates"""
    name, seq, n_best, raw = case
    if raw:
        keys = np.asarray(seq, np.float32)
        return keys[keys < np.float32(0.1)]
    return rank_keys(seq)
