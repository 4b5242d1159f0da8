"""The matrix of tests/walker_cases.py reaches what it is named for, shown on the host alone (no device): the self-queries of every consumer take every
state of the kNN seed on the larger shapes, the tie clouds end most neighbourhoods inside a group of equal distances that the seed does not cover, the
radii "at a tie" have pairs exactly at r2, the cluster cases have clique leaves and plain ones where their names say so, the two tiny-tolerance clouds
satisfy the clique rule as it WAS while the float relation separates them (and the rule as it is does not call them cliques), and the restatements
the device is held against (tools/outlier_numpy.py, tools/cluster_numpy.py, tools/normals_numpy.py) agree with values derived from the one brute force
and stay defined on every cloud."""
import functools

import numpy as np
import pytest

import search_cases as sc
import walker_cases as wc
from tools import cluster_numpy as cref
from tools import normals_numpy as nref
from tools import outlier_numpy as oref


@functools.lru_cache(maxsize=None)
def _model(name):
    return sc.tree_model(wc.CASES[name])


@functools.lru_cache(maxsize=None)
def _self_keys(name):
    fin, _, _ = wc.brute_self(name)
    return _model(name).codes(wc.CASES[name][fin, :3])


def test_the_matrix_is_the_search_matrix_plus_two_clouds():
    assert set(wc.MATRIX) == set(sc.SHAPES) | set(sc.TIES) | set(sc.RANGE)
    assert all(wc.CASES[n] is sc.CASES[n].target for n in wc.MATRIX), "no second copy of a cloud"
    assert set(wc.CASES) - set(wc.MATRIX) == {"tiny_tol_pair", "tiny_tol_40"}
    assert max(len(t) for t in wc.CASES.values()) == 1028
    for name, t in wc.CASES.items():
        assert t.dtype == np.float32 and t.ndim == 2 and t.shape[1] == 4
        fin, bi, bd = wc.brute_self(name)
        assert bi.shape == bd.shape == (len(fin), len(fin)) and not np.isnan(bd).any()
        assert (np.sort(bi, axis=1) == fin[None, :]).all()
        assert (bd[:, 0] == 0).all() and (bd[:, 1:] >= bd[:, :-1]).all()
    assert set(wc.NORMALS_K_ALL) >= {s + d for s in (4, 8, 16, 32, 64) for d in (-1, 0)} | {5, 9, 17, 33}
    assert {k + 1 for k in wc.SOR_MEAN_K_ALL} >= {2, 4, 5, 8, 9, 16, 17, 32, 64}
    assert all(_ks[0] >= 3 and _ks[-1] == 64 for _ks in (wc.NORMALS_K_ALL, wc.NORMALS_K_FEW))
    assert set(wc.FPFH_CLOUDS) <= set(wc.MATRIX) and set(wc.ICP_CLOUDS) == set(wc.MATRIX) - {"overflow"}


# -------------------------------------------------------------------------------------------------------------------- seed
@pytest.mark.parametrize("n", [n for n in sc.SHAPE_SIZES if n >= 97])
def test_self_queries_take_every_seed_clamp_at_each_k(n):
    """a list of two slots (mean_k = 1) cannot take the clamp at the end from a self-query: the lower bound of a point's own key is a position p <= Mf - 1,
    the seed starts at p - 1 and ends at p + 1 <= Mf.  Every other list of the matrix takes all three."""
    name = f"n{n}"
    m, keys = _model(name), _self_keys(name)
    for kk in sorted(set(wc.normals_ks(name)) | {k + 1 for k in wc.sor_mean_ks(name)}):
        seen = {m.seed_leaves(q, min(kk, m.Mf))[2] for q in keys}
        assert seen == ({"zero", "interior"} if kk == 2 else {"zero", "end", "interior"}), (name, kk, seen)


# -------------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("name", ("lattice_x3", "offset_1e7"))
def test_ties_straddle_the_seed(name):
    """a (point, k) pair counts when the neighbourhood ends inside a group of equal distances and a member of that group lies in a leaf the seed did not
    cover: the walk has to find it, and the list has to take it or refuse it by its index"""
    m, keys = _model(name), _self_keys(name)
    fin, bi, bd = wc.brute_self(name)
    pos = np.empty(len(wc.CASES[name]), np.int64)
    pos[m.idx] = np.arange(m.Mf)
    for what, ks in (("normals", wc.normals_ks(name)), ("sor", [k + 1 for k in wc.sor_mean_ks(name)])):
        pairs = straddling = 0
        for kk in ks:
            assert kk < m.Mf
            for i in range(len(fin)):
                pairs += 1
                if bd[i, kk - 1] != bd[i, kk]:
                    continue
                a, b, _ = m.seed_leaves(keys[i], kk)
                leaves = pos[bi[i][bd[i] == bd[i, kk - 1]]] // sc.LEAF
                straddling += bool(((leaves < a) | (leaves > b)).any())
        print(f"{name} {what}: {straddling} of {pairs} (point, k) pairs end inside a tie that straddles the seed")
        assert 4 * straddling >= pairs


def test_radii_at_a_tie_have_pairs_exactly_at_r2():
    for name, radii in wc.RADII_AT_A_TIE.items():
        _, _, bd = wc.brute_self(name)
        for r, above in radii:
            at = bd == sc.r2_of(r)
            assert at.any() and sc.r2_of(above) > sc.r2_of(r)
            assert ((bd < sc.r2_of(above)) == ((bd < sc.r2_of(r)) | at)).all(), "the next float takes exactly the pairs at the tie in"
            assert any((rr == r) for rr, _ in wc.ror_list(name)) and any((rr == above) for rr, _ in wc.ror_list(name))
            assert r in wc.cluster_tolerances(name) and above in wc.cluster_tolerances(name)
    # the counts the lattice's min_neighbors sit around: the three copies at r = 1, with the six neighbours (fewer on the border) at the next float
    c1, cn = wc.self_counts("lattice_x3", np.float32(1.0)), wc.self_counts("lattice_x3", wc.LATTICE_NEXT)
    assert (c1 == 3).all() and cn.max() == 21 and cn.min() == 12
    assert {m for r, m in wc.ror_list("lattice_x3") if r == wc.LATTICE_NEXT} >= {3, 4, 21, 22}
    # float sqrt 2 squares to the float just below 2: the face diagonals, at exactly 2, are outside by one float
    assert sc.r2_of(np.sqrt(np.float32(2.0))) == np.nextafter(np.float32(2.0), np.float32(0.0)) and (wc.brute_self("lattice_x3")[2] == 2.0).any()
    # the tiny-tolerance pair is a pair at the radius too
    assert wc.brute_self("tiny_tol_pair")[2][0, 1] == sc.r2_of(wc.TINY_TOLERANCE) == 8 * sc.DENORM_MIN


def test_ror_parameters_sit_on_both_sides_of_a_count():
    for name in wc.MATRIX:
        fin, _, _ = wc.brute_self(name)
        params = wc.ror_list(name)
        assert params, name
        for r in {r for r, _ in params}:
            assert np.isfinite(r) and r > 0
            ms = {m for rr, m in params if rr == r}
            counts = wc.self_counts(name, r)
            assert ms >= {1, 2, 33, len(fin) + 1} and min(ms) >= 1
            if (counts >= 2).any():
                c = int(counts[np.flatnonzero(counts >= 2)[0]])
                assert {c, c + 1} <= ms
    for name in ("underflow_cube", "partial_underflow", "partial_underflow_1e22"):
        assert [float(sc.r2_of(r)) for r in sorted({r for r, _ in wc.ror_list(name)})] == [sc.DENORM_MIN, 8 * sc.DENORM_MIN, sc.NORMAL_MIN]


# ------------------------------------------------------------------------------------------------------------------ cliques
# what the names say, under the rule as it is: "all" / "none" / "both" of the leaves are cliques
CLIQUES_NAMED = {("coincident_100", 0): "all", ("two_values_140", 0): "both", ("two_values_140", 1): "all", ("lattice_x3", 0): "none",
                 ("lattice_x3", 2): "none", ("underflow_cube", 0): "none", ("underflow_cube", 1): "all", ("underflow_cube", 2): "all",
                 ("partial_underflow", 2): "all", ("partial_underflow_1e22", 1): "both", ("denormal_results", 0): "none", ("overflow", 0): "none",
                 ("overflow", 1): "both", ("offset_1e7", 1): "none", ("n1024", 0): "none", ("n1025", 0): "both", ("tiny_tol_pair", 0): "none",
                 ("tiny_tol_40", 0): "both"}


@pytest.mark.parametrize("name", wc.CLUSTER_CLOUDS)
def test_clique_leaves_are_cliques_and_are_where_the_names_say(name):
    m = _model(name)
    tols = wc.cluster_tolerances(name)
    assert tols, name
    for j, tol in enumerate(tols):
        r2 = sc.r2_of(tol)
        assert np.isfinite(r2) and r2 > 0
        new = wc.clique_leaves(m, r2, "new")
        truth = np.array([wc.leaf_is_all_adjacent(m, l, r2) for l in range(m.L)])
        assert not (new & ~truth).any(), f"{name} at {tol!r}: the rule calls a leaf a clique that has a pair with float d2 >= r2"
        if (name, j) in CLIQUES_NAMED:
            want = CLIQUES_NAMED[(name, j)]
            assert {"all": new.all(), "none": not new.any(), "both": new.any() and not new.all()}[want], (name, tol, new)
        if name not in wc.TINY:      # the rule as it was is wrong nowhere else in the matrix
            assert not (wc.clique_leaves(m, r2, "old") & ~truth).any()


@pytest.mark.parametrize("name", list(wc.TINY))
def test_the_defect_shows_on_the_tiny_tolerance_clouds(name):
    """the leaf that holds both ends of the diagonal satisfies the rule as it was, although its ends are not adjacent under float d2 < r2: the
    restatement has two clusters, and a device that hooks the leaf under one root has one.  The rule as it is does not call it a clique."""
    m = _model(name)
    r2 = sc.r2_of(wc.TINY_TOLERANCE)
    lo, hi = m.lo[m.P].astype(np.float64), m.hi[m.P].astype(np.float64)
    diag2 = float(((hi - lo) ** 2).sum())
    assert diag2 * (1.0 + 1e-6) < float(r2), "the old rule holds for the first leaf"
    assert 7.1 * sc.DENORM_MIN < diag2 < 7.3 * sc.DENORM_MIN and float(r2) == 8 * sc.DENORM_MIN
    assert wc.clique_leaves(m, r2, "old")[0] and not wc.clique_leaves(m, r2, "new")[0]
    assert not wc.leaf_is_all_adjacent(m, 0, r2)
    want = cref.cluster(wc.CASES[name], float(wc.TINY_TOLERANCE), 1, None)
    half = len(wc.CASES[name]) // 2
    assert want["sizes"].tolist() == [half, half], "the restatement separates the two ends"
    if name == "tiny_tol_40":
        assert m.L == 2 and wc.clique_leaves(m, r2, "new")[1], "the second leaf is one end alone: a clique under either rule"


# ------------------------------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("name", wc.MATRIX)
def test_outlier_restatements_follow_the_brute_force(name):
    t = wc.CASES[name]
    fin, _, bd = wc.brute_self(name)
    with np.errstate(all="ignore"):
        for mean_k in wc.sor_mean_ks(name):
            kk = min(mean_k + 1, len(fin))
            want = np.zeros(len(t), np.float32)
            want[fin] = oref._distance_from_sorted_d2(bd[:, :kk], mean_k)
            got = oref.sor_distances(t, mean_k)
            assert not np.isnan(got).any() and (got.view(np.uint32) == want.view(np.uint32)).all(), (name, mean_k)
            if name not in ("overflow", "collapse"):
                assert np.isfinite(got).all(), (name, mean_k)
        for r in sorted({r for r, _ in wc.ror_list(name)}):
            got = oref.radius(t, float(r), len(fin) + 1)["counts"]      # a threshold no count reaches: the counts themselves
            want = np.zeros(len(t), np.uint32)
            want[fin] = wc.self_counts(name, r)
            assert (got == want).all(), (name, r)
            assert sc.r2_of(r) == oref.r2_of(r)


@pytest.mark.parametrize("name", wc.MATRIX)
def test_normals_restatement_follows_the_brute_force(name):
    t = wc.CASES[name]
    fin, bi, _ = wc.brute_self(name)
    pts = np.ascontiguousarray(t[fin, :3])
    for k in wc.normals_ks(name)[::3]:
        kk = min(k, len(fin))
        assert (fin[nref.neighbours(pts, kk)] == bi[:, :kk]).all(), (name, k)
    for k in (3, 9, 17):
        r = nref.estimate(t, k)
        bad = ~np.isfinite(r["normals"][fin]).all(axis=1)
        assert bad.all() if len(fin) < 3 else not bad.any(), f"{name} k={k}: the restatement is not defined on every finite point"
        assert np.isnan(r["normals"][~sc.finite_rows(t)]).all()


@pytest.mark.parametrize("name", wc.CLUSTER_CLOUDS)
def test_cluster_restatement_equals_a_plain_search_over_the_full_matrix(name):
    t = wc.CASES[name]
    fin, _, _ = wc.brute_self(name)
    d2 = wc.self_d2(name)
    for tol in wc.cluster_tolerances(name):
        comp = wc.bfs_components(d2, sc.r2_of(tol))
        want = cref.cluster(t, float(tol), 1, None)
        assert cref.r2_of(tol) == sc.r2_of(tol)
        assert len(want["sizes"]) == comp.max() + 1 and (want["labels"][~sc.finite_rows(t)] == -1).all()
        labels = want["labels"][fin]
        assert (labels >= 0).all()
        # the same partition: every component has one label and every label one component
        pairs = set(zip(comp.tolist(), labels.tolist()))
        assert len(pairs) == comp.max() + 1 == len({c for c, _ in pairs}) == len({l for _, l in pairs}), (name, tol)
        sizes = np.bincount(labels)
        assert (sizes == want["sizes"]).all() and (np.diff(sizes.astype(np.int64)) <= 0).all()
        assert np.isfinite(want["centroids"]).all()
