"""TEST INFRASTRUCTURE: seeded Scan Context cases (CPU only: numpy and the restatement tools/sc_numpy.py, nothing of the library), each built to reach
one branch of lt-mapper_amd/csrc/ltm_k_scancontext.hip that the default 20 x 60 shape and a database of 40 entries do not reach.

The generators of tests/test_gpu_scancontext.py live here (polar_points, away_from, place, session_scans, rotated) and are imported back there.
all_cases() returns every case as a dict: name, family, branch (what it is built to reach), p (the restatement's parameters), the inputs, and `runs`,
the list of parameter sets with the restatement's expected result of each.  Families:

  pair         (shape_case)      `base` / `copies` descriptors and 24 (copy, base) pairs at the shapes of SHAPES; runs: search_ratio with dist, shift and
                                 the two gaps (alignment norms, distances inside the search space) that make the expected shift well-posed
  known        (one_by_one_case) the 1 x 1 shape: known answers
  candidates   (candidate_case)  ltm_sc_detect with num_candidates 1 / 3 / 64 against nd = 63 / 64 / 65 / 130 entries with exact duplicates and a crowd
  exhaustive   (exhaustive_case) num_candidates 0 / nd / nd + 5 against 130 entries: duplicates in different lanes of the reduction, a scaled twin
  nonfinite    (nonfinite_case)  a NaN bin, a 1e30 bin and an all-zero entry in the database, in both index orders
  descriptors  (many_keyframes_case, block_edge_case) ltm_sc_from_scanset with more than 65535 keyframes and on either side of the scatter's LDS limit

Database descriptors are ref.descriptors(session_scans(...)) with max(600, 3 R S / 2) points per keyframe (about three quarters of the bins filled),
queries are `rotated` copies (whole sectors, 1e-3 height noise).  Exact ties are made of exact arithmetic only, never of near-ties:
  * an exact duplicate of an entry ties with it in ring-key distance AND in pair distance, bit for bit: the smaller index has to win;
  * the crowd: three exact duplicates of a descriptor D whose ring key is the query's (D is the query with every row permuted on its own: same
    row means, unrelated columns), while the entry X the query was made of (columns scaled by 0.95 .. 1.05: cosine distance 0, ring key moved) is
    fourth in key order.  With num_candidates = 3 the duplicates fill the list and X must NOT be found; a selection that skips equal key distances
    lets X in;
  * the scaled twin: entry X with every second column doubled.  Doubling a column doubles its dot products and its norm exactly, so every column
    cosine, hence the distance at every shift, is bit-equal to X's, while the ring key is not: with every shift searched the two entries tie exactly
    in distance and the one with the smaller KEY DISTANCE has to win, although its index is the larger one.
The 1e30 entry: its float ring key (1e30 / S) is finite, the SQUARE in the float key distance overflows to +inf; its column norms and cosines are
finite in double, so it is a legitimate winner.  A NaN bin makes the ring key, the key distance and every pair distance of its entry NaN."""
import numpy as np

from tools import sc_numpy as ref

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------ generators (shared with tests/test_gpu_scancontext.py)
def polar_points(rng, n, p, exclude=()):
    """n points in the interior of random bins (never one of `exclude`, 0-based (ring, sector)); z so that z + 2 covers negatives, zero and ordinary heights"""
    R, S = p["num_ring"], p["num_sector"]
    ri, si = rng.integers(0, R, n), rng.integers(0, S, n)
    return place(rng, *away_from(ri, si, S, exclude), p, rng.uniform(-2.9, 9.0, n))


def away_from(ri, si, S, exclude):
    """bin indices moved one sector on where they hit a bin of `exclude` (distinct rings there, so the move never lands in another one)"""
    for (er, es) in exclude:
        hit = (ri == er) & (si == es)
        si[hit] = (si[hit] + 1) % S if S > 1 else si[hit]
    return ri, si


def place(rng, ri, si, p, z):
    R, S = p["num_ring"], p["num_sector"]
    n = len(ri)
    r = (ri + rng.uniform(0.1, 0.9, n)) * (p["max_radius"] / R)
    th = np.deg2rad((si + rng.uniform(0.1, 0.9, n)) * (360.0 / S))
    return np.stack([r * np.cos(th), r * np.sin(th), np.asarray(z, np.float64), np.zeros(n)], axis=1).astype(np.float32)


def session_scans(seed, n_kf, pts_per_kf, p):
    rng = np.random.default_rng(seed)
    scans = np.concatenate([polar_points(rng, pts_per_kf, p) for _ in range(n_kf)])
    return scans, (np.arange(n_kf + 1) * pts_per_kf).astype(np.uint64)


def rotated(rng, desc, rot, noise=1e-3):
    out = np.roll(desc, rot, axis=1)
    return out + np.where(out != 0, rng.uniform(-noise, noise, out.shape), 0.0)


def points_per_keyframe(R, S):
    return max(600, 3 * R * S // 2)


def database(seed, n, p):
    return ref.descriptors(*session_scans(seed, n, points_per_keyframe(p["num_ring"], p["num_sector"]), p), p)


# ------------------------------------------------------------------ pair distance and shift over the shapes
SHAPES = ((3, 64), (5, 65), (7, 128), (64, 57), (64, 58), (40, 120), (64, 256), (20, 60))
SHAPE_BRANCH = {(3, 64): "one full trip of the shift loops", (5, 65): "second trip of one lane", (7, 128): "two full trips",
                (64, 57): "last shape staged in LDS", (64, 58): "first shape not staged", (40, 120): "not staged, two trips",
                (64, 256): "domain corner: not staged, four trips", (20, 60): "anchor: the default shape"}
RATIOS = (0.0, 0.05, 0.1, 0.7, 1.0)
N_BASE = 12


def rotation_choices(S):
    """{0, 1, S/2, S-1, 63, 64, 65} clipped to S - 1: the best shift on both sides of a lane-trip boundary and on the wrap-around"""
    return sorted({min(r, S - 1) for r in (0, 1, S // 2, S - 1, 63, 64, 65)})


def shape_case(R, S):
    return _cached(("pair", R, S), lambda: _shape_case(R, S))


def _shape_case(R, S):
    p = ref.params(num_ring=R, num_sector=S)
    rng = np.random.default_rng(7000 + 1000 * R + S)
    base = database(100 + 1000 * R + S, N_BASE, p)
    choices = rotation_choices(S)
    rots = np.concatenate([rng.permutation(choices), rng.choice(choices, N_BASE)])[:N_BASE].astype(np.int64)      # every choice once, then draws
    copies = np.stack([rotated(rng, base[k], int(rots[k])) for k in range(N_BASE)])
    pairs = np.concatenate([np.stack([np.arange(N_BASE)] * 2, axis=1), rng.integers(0, N_BASE, (N_BASE, 2))]).astype(np.int32)
    # the restatement's distance(), its shift-independent parts evaluated once per pair (tests/test_sc_cases_cpu.py compares with ref.distance itself)
    per_pair = []
    for i, j in pairs:
        norms = ref.align_norms(ref.sector_key(copies[i]), ref.sector_key(base[j]))
        per_pair.append((norms, ref.first_min(norms, range(S))[1], ref.shift_distances(copies[i], base[j])))
    runs = []
    for ratio in RATIOS:
        dist, shift, ngap, dgap, width = [], [], [], [], []
        for norms, a0, d in per_pair:
            space = ref.search_space(a0, S, ratio)
            best, arg = ref.first_min(d, space)
            sn, sd = np.sort(norms), np.sort(d[space])
            dist.append(best), shift.append(arg), width.append(len(space))
            ngap.append(sn[1] - sn[0]), dgap.append(sd[1] - sd[0] if len(sd) > 1 else np.inf)
        runs.append(dict(search_ratio=ratio, dist=np.array(dist), shift=np.array(shift, np.int32), norm_gap=np.array(ngap), dist_gap=np.array(dgap),
                         width=np.array(width)))
    return dict(name=f"pair-{R}x{S}", family="pair", branch=SHAPE_BRANCH[(R, S)], p=p, base=base, copies=copies, rots=rots, pairs=pairs, runs=runs)


def one_by_one_case():
    """1 x 1: the only shift is 0; equal signs give cosine 1, a zero descriptor gives no column to count.  R = 1 stays out of the shape family: with one
    ring every column cosine is +-1 and exact ties are everywhere."""
    descs = np.array([2.0, 3.0, -1.5, 0.0]).reshape(4, 1, 1)
    pairs = np.array([[0, 1], [1, 0], [0, 0], [2, 2], [0, 3], [3, 0], [3, 3]], np.int32)
    return dict(name="known-1x1", family="known", branch="a single sector", p=ref.params(num_ring=1, num_sector=1), descs=descs, pairs=pairs,
                dist=np.array([0.0, 0.0, 0.0, 0.0, 10000000.0, 10000000.0, 10000000.0]), shift=np.zeros(7, np.int32))


# ------------------------------------------------------------------ detect: candidates, exhaustive, non-finite
DETECT_SHAPES = ((5, 65), (20, 60))
CANDIDATE_ND = (63, 64, 65, 130)
CANDIDATE_K = (1, 3, 64)
CANDIDATE_DUPS = {8: 2, 62: 2, 64: 2, 70: 2, 129: 2}      # index -> the entry it copies: lanes 2, 8, 62, then the second and third trip of the row loop
CROWD_SOURCE = 20                                          # X: the entry the crowd query is made of
EXHAUSTIVE_ND = 130
EXHAUSTIVE_DUPS = {66: 2, 129: 5}                          # 2 and 66 meet in lane 2 of the reduction, 5 and 129 in lanes 5 and 1
TWIN_SOURCE, TWIN_AT = 77, 9                               # entry 9 = entry 77 with every second column doubled


def crowd_indices(nd):
    return (3, 67, 128) if nd > 128 else (3, 40, 61)      # lanes 3, 3 (second trip) and 0 (third trip) of the row loop


def _base130(R, S):
    return _cached(("base130", R, S), lambda: database(300 + 1000 * R + S, 130, ref.params(num_ring=R, num_sector=S)))


def _other(R, S):
    return _cached(("other", R, S), lambda: database(400 + 1000 * R + S, 1, ref.params(num_ring=R, num_sector=S)))


def _copies(rng, db, src, S):
    rots = [(0, 1, S // 2, S - 1, 7)[k % 5] for k in range(len(src))]
    return [rotated(rng, db[s], r) for s, r in zip(src, rots)], rots


def candidate_case(R, S, nd):
    return _cached(("cand", R, S, nd), lambda: _candidate_case(R, S, nd))


def _candidate_case(R, S, nd):
    p = ref.params(num_ring=R, num_sector=S)
    rng = np.random.default_rng(9000 + 1000 * R + S + nd)
    db = _base130(R, S)[:nd].copy()
    dups = {i: s for i, s in CANDIDATE_DUPS.items() if i < nd}
    for i, s in dups.items():
        db[i] = db[s]
    crowd_q = db[CROWD_SOURCE] * rng.uniform(0.95, 1.05, S)[None, :]
    crowd_d = np.stack([row[rng.permutation(S)] for row in crowd_q])
    for i in crowd_indices(nd):
        db[i] = crowd_d
    src = [2, 5, CROWD_SOURCE, 33, nd - 1]
    copies, rots = _copies(rng, db, src, S)
    queries = np.stack(copies + [db[2].copy(), crowd_q, _other(R, S)[0]])
    roles = dict(copies=list(range(len(src))), copy_sources=src, copy_rots=rots, equals_duplicated=len(src), crowd=len(src) + 1, unrelated=len(src) + 2)
    runs = [dict(num_candidates=k, search_ratio=p["search_ratio"], want=ref.detect(db, queries, dict(p, num_candidates=k))) for k in CANDIDATE_K]
    return dict(name=f"candidates-{R}x{S}-nd{nd}", family="candidates", branch="row loop past 64 entries" if nd > 64 else "row loop within one trip", p=p,
                db=db, queries=queries, dups=dups, crowd=crowd_indices(nd), roles=roles, runs=runs)


def exhaustive_case(R, S):
    return _cached(("exh", R, S), lambda: _exhaustive_case(R, S))


def _exhaustive_case(R, S):
    p = ref.params(num_ring=R, num_sector=S)
    nd = EXHAUSTIVE_ND
    rng = np.random.default_rng(11000 + 1000 * R + S)
    db = _base130(R, S).copy()
    for i, s in EXHAUSTIVE_DUPS.items():
        db[i] = db[s]
    db[TWIN_AT] = db[TWIN_SOURCE] * np.where(np.arange(S) % 2 == 0, 2.0, 1.0)[None, :]
    src = [2, 5, TWIN_SOURCE, 100]
    copies, rots = _copies(rng, db, src, S)
    queries = np.stack(copies + [db[5].copy(), _other(R, S)[0]])
    roles = dict(copies=list(range(len(src))), copy_sources=src, copy_rots=rots, equals_duplicated=len(src), twin=2, unrelated=len(src) + 1)
    ncs = (0, nd, nd + 5) if (R, S) == DETECT_SHAPES[0] else (0,)
    runs = [dict(num_candidates=nc, search_ratio=ratio, want=ref.detect(db, queries, dict(p, num_candidates=nc, search_ratio=ratio)))
            for nc in ncs for ratio in (0.1, 1.0)]
    return dict(name=f"exhaustive-{R}x{S}", family="exhaustive", branch="reduction over more than 64 pairs per query", p=p, db=db, queries=queries,
                dups=dict(EXHAUSTIVE_DUPS), twin=(TWIN_AT, TWIN_SOURCE), roles=roles, runs=runs)


NONFINITE_ND = 10
NONFINITE_ZERO = 5


def nonfinite_case(nan_at, inf_at):
    return _cached(("nonfinite", nan_at, inf_at), lambda: _nonfinite_case(nan_at, inf_at))


def _nonfinite_case(nan_at, inf_at):
    """(5, 65), 10 entries: entry nan_at holds a NaN bin, entry inf_at a 1e30 bin, entry 5 is all zero.  Of the 10 key distances of the ordinary query 8 are
    finite, one is +inf and one NaN: with num_candidates = 9 those two compete for the last place, and the query is a copy of the 1e30 entry's original,
    so the result says which one got it.  Every shift is searched: the 1e30 sector key swamps the alignment norms, which all tie."""
    R, S = DETECT_SHAPES[0]
    p = ref.params(num_ring=R, num_sector=S, search_ratio=1.0)
    rng = np.random.default_rng(13000 + 10 * nan_at + inf_at)
    db = _base130(R, S)[:NONFINITE_ND].copy()
    plain = db[inf_at].copy()
    db[NONFINITE_ZERO] = 0.0
    db[nan_at][2, 11] = np.nan
    db[inf_at][3, 40] = 1e30
    queries = np.stack([rotated(rng, plain, 7), db[nan_at].copy(), db[inf_at].copy()])
    with np.errstate(all="ignore"):
        runs = [dict(num_candidates=nc, search_ratio=1.0, want=ref.detect(db, queries, dict(p, num_candidates=nc))) for nc in (8, 9, 0)]
    return dict(name=f"nonfinite-nan{nan_at}-inf{inf_at}", family="nonfinite", branch="a NaN and a +inf key distance compete", p=p, db=db, queries=queries,
                nan_at=nan_at, inf_at=inf_at, runs=runs)


# ------------------------------------------------------------------ descriptors from scans
MANY_KF = 65540
MANY_NONEMPTY = (0, 1, 4, 30000, 32768, 65533, 65534, 65535, 65536, 65537, 65538, 65539)


def many_keyframes_case(kf_begin):
    return _cached(("many", kf_begin), lambda: _many_keyframes_case(kf_begin))


def _many_keyframes_case(kf_begin):
    """65540 keyframes at (2, 3), all empty but MANY_NONEMPTY (1 - 3 interior points each): the scatter's second chunk over gridDim.y.  `want` holds the
    restatement's descriptors of the non-empty keyframes only; every other one is zero by definition."""
    p = ref.params(num_ring=2, num_sector=3)
    rng = np.random.default_rng(15000)
    counts = np.zeros(MANY_KF, np.int64)
    kfs = []
    for k in MANY_NONEMPTY:
        n = int(rng.integers(1, 4))
        counts[k] = n
        kfs.append(place(rng, rng.integers(0, 2, n), rng.integers(0, 3, n), p, rng.uniform(-2.9, 9.0, n)))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    want = np.stack([ref.descriptor(k, p) for k in kfs])
    return dict(name=f"descriptors-65540-from{kf_begin}", family="descriptors", branch="more than 65535 keyframes in one call", p=p, scans=np.concatenate(kfs),
                offsets=off, kf_begin=kf_begin, nonempty=np.array(MANY_NONEMPTY), want=want)


BLOCK_EDGE_SHAPES = ((64, 64), (64, 65))      # 4096 bins: the last shape the scatter pre-reduces in LDS; 4160: the first it does not


def block_edge_case(R, S):
    return _cached(("edge", R, S), lambda: _block_edge_case(R, S))


def _block_edge_case(R, S):
    p = ref.params(num_ring=R, num_sector=S)
    scans, off = session_scans(17000 + S, 3, 5000, p)      # three blocks of the scatter per keyframe
    return dict(name=f"descriptors-{R}x{S}", family="descriptors", branch="either side of the scatter's LDS limit", p=p, scans=scans, offsets=off, kf_begin=0,
                nonempty=np.arange(3), want=ref.descriptors(scans, off, p))


def pair_cases():
    return [shape_case(R, S) for R, S in SHAPES]


def detect_cases():
    return ([candidate_case(R, S, nd) for R, S in DETECT_SHAPES for nd in CANDIDATE_ND] + [exhaustive_case(R, S) for R, S in DETECT_SHAPES] +
            [nonfinite_case(3, 7), nonfinite_case(7, 3)])


def descriptor_cases():
    return [many_keyframes_case(0), many_keyframes_case(3)] + [block_edge_case(R, S) for R, S in BLOCK_EDGE_SHAPES]


def all_cases():
    return pair_cases() + [one_by_one_case()] + detect_cases() + descriptor_cases()
