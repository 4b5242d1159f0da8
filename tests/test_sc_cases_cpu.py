"""The Scan Context cases of tests/sc_cases.py are well-posed and reach the branch each is named for (no GPU needed): the expected shifts do not
hinge on a near-tie, the ties that are meant to be exact are exact in the restatement (tools/sc_numpy.py) and resolved by the smaller index, and the
sizes that select another kernel or another trip of a loop are there -- read from the cases' own numbers and, for the two LDS decisions, from the
library's launch wrappers themselves (ltm_debug_sc_paths).  tests/test_gpu_scancontext_shapes.py runs the same cases on the device."""
import numpy as np
import pytest

import sc_cases as sc
from tools import sc_numpy as ref

bits = lambda a: np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def key_distances(case, q):
    with np.errstate(all="ignore"):
        return ref.key_distances(ref.ring_key(case["queries"][q]), np.stack([ref.ring_key(d) for d in case["db"]]))


# ------------------------------------------------------------------ pair family
@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pair_cases_are_well_posed(shape):
    """every pair of every shape, none left out: the two smallest alignment norms and the two smallest distances inside the search space differ by more
    than 1e-9 (the condition tests/test_gpu_scancontext.py puts on its inputs), and the diagonal pairs come back at their rotation"""
    c = sc.shape_case(*shape)
    R, S = shape
    assert c["base"].shape == (sc.N_BASE, R, S) and c["copies"].shape == (sc.N_BASE, R, S) and len(c["pairs"]) == 2 * sc.N_BASE
    assert (c["pairs"][:sc.N_BASE] == np.arange(sc.N_BASE)[:, None]).all()
    assert sorted(set(c["rots"].tolist())) == sc.rotation_choices(S)                       # every rotation of the family is used
    assert 0.7 < np.mean(c["base"] != 0) < 1.0                                             # about three quarters of the bins and more are filled
    assert [r["search_ratio"] for r in c["runs"]] == list(sc.RATIOS)
    for run in c["runs"]:
        print(c["name"], "ratio", run["search_ratio"], "min alignment-norm gap", float(run["norm_gap"].min()), "min distance gap", float(run["dist_gap"].min()))
        assert (run["norm_gap"] > 1e-9).all(), np.nonzero(run["norm_gap"] <= 1e-9)[0]
        assert (run["dist_gap"] > 1e-9).all(), np.nonzero(run["dist_gap"] <= 1e-9)[0]
        assert (run["shift"][:sc.N_BASE] == c["rots"]).all() and (run["dist"][:sc.N_BASE] < 0.01).all()
    # the builder evaluates the restatement's distance() piecewise: the same numbers as distance() itself
    for k in (0, sc.N_BASE - 1, sc.N_BASE, 2 * sc.N_BASE - 1):
        i, j = c["pairs"][k]
        for run in (c["runs"][0], c["runs"][2]):
            d, s = ref.distance(c["copies"][i], c["base"][j], run["search_ratio"])
            assert d == run["dist"][k] and s == run["shift"][k]
    # the search space: one shift at ratio 0, every shift at ratio 1, and the reference's round(): half-way values go up
    assert (c["runs"][0]["width"] == 1).all() and (c["runs"][-1]["width"] == S).all()
    for run in c["runs"][1:-1]:
        assert (run["width"] == 2 * int(np.floor(0.5 * run["search_ratio"] * S + 0.5)) + 1).all()


def test_pair_shapes_reach_their_branches(ltm):
    paths = {s: ltm.sc_paths(*s) for s in sc.SHAPES}
    assert {p[1] for p in paths.values()} == {True, False}                                 # staged in LDS and not
    assert paths[(64, 57)][1] and not paths[(64, 58)][1]                                   # ... on either side of the limit
    assert not paths[(40, 120)][1] and not paths[(64, 256)][1] and paths[(20, 60)][1] and paths[(5, 65)][1]
    for (R, S), (_, staged) in paths.items():
        assert staged == (5 * S * 8 + 2 * R * S * 8 <= 61440)
    trips = {s: -(-s[1] // 64) for s in sc.SHAPES}                                         # trips of the lanes' shift loops
    assert trips[(3, 64)] == 1 and trips[(5, 65)] == 2 and trips[(7, 128)] == 2 and trips[(64, 256)] == 4 and trips[(20, 60)] == 1
    for s in sc.SHAPES:
        c = sc.shape_case(*s)
        if s[1] > 64:                                                                      # a best shift in the second trip, and the lane boundary itself
            assert (c["rots"] >= 64).any() and (c["rots"] < 64).any()
        assert 0 in c["rots"] and s[1] - 1 in c["rots"]                                    # no shift, and the wrap-around
    assert any(abs(0.5 * r * S % 1 - 0.5) < 1e-12 for r in sc.RATIOS for _, S in sc.SHAPES)  # a radius that ends in .5
    assert ltm.load_library().ltm_debug_sc_paths(65, 60, None, None) == -1 and ltm.load_library().ltm_debug_sc_paths(20, 0, None, None) == -1
    assert ltm.load_library().ltm_debug_sc_paths(64, 256, None, None) == 0


def test_one_by_one_known_answers():
    c = sc.one_by_one_case()
    for (i, j), d, s in zip(c["pairs"], c["dist"], c["shift"]):
        with np.errstate(all="ignore"):
            assert ref.distance(c["descs"][i], c["descs"][j], 1.0) == (d, s)


# ------------------------------------------------------------------ detect families
@pytest.mark.parametrize("shape", sc.DETECT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("nd", sc.CANDIDATE_ND)
def test_candidate_cases_tie_exactly(shape, nd):
    c = sc.candidate_case(*shape, nd)
    roles = c["roles"]
    assert len(c["db"]) == nd and (nd > 64) == (c["branch"] == "row loop past 64 entries")
    assert [r["num_candidates"] for r in c["runs"]] == [1, 3, 64]
    assert c["dups"] and all(i > s for i, s in c["dups"].items())
    if nd > 64:
        assert any(i >= 64 for i in c["dups"]) and any(i < 64 for i in c["dups"])        # ties on both sides of the lane stride
    for q in range(len(c["queries"])):
        kd = key_distances(c, q)
        for i, s in c["dups"].items():
            assert bits(kd)[i] == bits(kd)[s]                                              # bit-equal key distances
    # the query that equals the duplicated entry: key distance 0 to the whole group, which leads the candidate order by index alone
    q = roles["equals_duplicated"]
    group = sorted([2] + [i for i, s in c["dups"].items() if s == 2])
    kd = key_distances(c, q)
    order = np.lexsort((np.arange(nd), kd))
    assert (kd[group] == 0).all() and order[:len(group)].tolist() == group
    for run in c["runs"]:
        w = run["want"]
        assert w["nn_idx"][q] == 2 and w["nn_align"][q] == 0 and w["min_dist"][q] < 1e-12   # the smaller index
        for k, s in zip(roles["copies"], roles["copy_sources"]):                           # a copy of a duplicate finds the original
            assert w["nn_idx"][k] == c["dups"].get(s, s)
    # the crowd: three bit-equal key distances in front, then the entry the query was made of, which is the nearer one by far
    q, crowd = roles["crowd"], list(c["crowd"])
    kd = key_distances(c, q)
    order = np.lexsort((np.arange(nd), kd))
    assert order[:4].tolist() == crowd + [sc.CROWD_SOURCE] and len(set(bits(kd)[crowd].tolist())) == 1 and kd[sc.CROWD_SOURCE] > kd[crowd[0]]
    if nd > 128:
        assert crowd[1] - crowd[0] == 64 and crowd[2] % 64 == 0                            # one lane's two trips, and a third trip
    want = {r["num_candidates"]: r["want"] for r in c["runs"]}
    assert want[1]["nn_idx"][q] == crowd[0] and want[3]["nn_idx"][q] == crowd[0] and want[3]["min_dist"][q] > 0.1
    assert want[64]["nn_idx"][q] == sc.CROWD_SOURCE and want[64]["min_dist"][q] < 1e-12


@pytest.mark.parametrize("shape", sc.DETECT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exhaustive_cases_tie_exactly(shape):
    c = sc.exhaustive_case(*shape)
    nd, S, roles = len(c["db"]), shape[1], c["roles"]
    assert nd > 64                                                                         # K = nd: the reduction's second and third trip
    assert {r["num_candidates"] for r in c["runs"]} >= {0} and {r["search_ratio"] for r in c["runs"]} == {0.1, 1.0}
    if shape == sc.DETECT_SHAPES[0]:
        assert {r["num_candidates"] for r in c["runs"]} == {0, nd, nd + 5}
    lanes = {i: (i % 64, s % 64) for i, s in c["dups"].items()}
    assert lanes[66] == (2, 2) and lanes[129] == (1, 5)                                    # one pair within a lane, one across lanes (the larger index in the lower lane)
    for i, s in c["dups"].items():
        assert (bits(c["db"][i]) == bits(c["db"][s])).all()
    by_params = {(r["num_candidates"], r["search_ratio"]): r["want"] for r in c["runs"]}
    for (nc, ratio), w in by_params.items():
        assert w["nn_idx"][roles["equals_duplicated"]] == 5 and w["nn_idx"][0] == 2 and w["nn_idx"][1] == 5      # the smaller index of each pair
        for k in ("loop_id", "nn_idx", "nn_align", "min_dist", "yaw_diff_rad"):            # 0, nd and nd + 5 mean the same
            assert (bits(w[k]) == bits(by_params[(0, ratio)][k])).all() if w[k].dtype.kind == "f" else (w[k] == by_params[(0, ratio)][k]).all()
    # the scaled twin: bit-equal distance at every shift, a different key distance; the smaller key distance wins against the smaller index
    at, src = c["twin"]
    q = c["queries"][roles["twin"]]
    assert at < src and at % 64 != src % 64
    assert (bits(ref.shift_distances(q, c["db"][at])) == bits(ref.shift_distances(q, c["db"][src]))).all()
    assert ref.distance(q, c["db"][at], 1.0) == ref.distance(q, c["db"][src], 1.0)
    kd = key_distances(c, roles["twin"])
    assert kd[src] < kd[at]
    assert by_params[(0, 1.0)]["nn_idx"][roles["twin"]] == src


@pytest.mark.parametrize("order", [(3, 7), (7, 3)], ids=["nan-first", "inf-first"])
def test_nonfinite_cases_have_a_nan_and_an_inf_key_distance(order):
    c = sc.nonfinite_case(*order)
    nan_at, inf_at, nd = c["nan_at"], c["inf_at"], len(c["db"])
    kd = key_distances(c, 0)
    assert np.isnan(kd[nan_at]) and np.isposinf(kd[inf_at]) and np.isfinite(np.delete(kd, [nan_at, inf_at])).all()
    assert np.isfinite(ref.ring_key(c["db"][inf_at])).all()                                # the key is finite: its square overflows
    assert (c["db"][sc.NONFINITE_ZERO] == 0).all()
    order_ = np.lexsort((np.arange(nd), kd))
    assert order_[-2:].tolist() == [inf_at, nan_at]                                        # +inf before NaN, whatever the indices
    want = {r["num_candidates"]: r["want"] for r in c["runs"]}
    assert want[8]["nn_idx"][0] not in (inf_at, nan_at)                                    # neither is a candidate
    assert want[9]["nn_idx"][0] == inf_at and want[9]["min_dist"][0] < 0.05                # the last place goes to the +inf one, which is the query's original
    assert want[0]["nn_idx"][0] == inf_at
    for w in want.values():
        assert w["min_dist"][1] == 10000000.0 and w["nn_idx"][1] == 0 and w["loop_id"][1] == -1      # the NaN entry as a query finds nothing
    assert np.isnan(key_distances(c, 1)).all()
    kd2 = key_distances(c, 2)                                                              # the 1e30 entry as a query: itself, then +inf everywhere, the NaN last
    assert kd2[inf_at] == 0 and np.isnan(kd2[nan_at]) and np.isposinf(np.delete(kd2, [nan_at, inf_at])).all()
    assert all(w["nn_idx"][2] == inf_at for w in want.values())


# ------------------------------------------------------------------ descriptors
def test_descriptor_cases_reach_their_branches(ltm):
    in_lds = set()
    for c in sc.descriptor_cases():
        R, S = c["p"]["num_ring"], c["p"]["num_sector"]
        in_lds.add(ltm.sc_paths(R, S)[0])
        n_kf = len(c["offsets"]) - 1
        assert len(c["want"]) == len(c["nonempty"])
        sizes = np.diff(c["offsets"].astype(np.int64))
        assert (np.nonzero(sizes)[0] == c["nonempty"]).all()
        assert all(np.count_nonzero(w) > 0 for w in c["want"])
        if "65540" in c["name"]:
            assert n_kf > 65535 and n_kf - c["kf_begin"] > 65535                            # a second chunk over gridDim.y, also from kf_begin
            assert (c["nonempty"] >= c["kf_begin"] + 65535).sum() >= 2 and sizes.max() <= 3
            assert {0, 1} <= set(c["nonempty"].tolist()) and set(range(65533, 65540)) <= set(c["nonempty"].tolist())
            of = lambda k: c["want"][list(c["nonempty"]).index(k)] if k in c["nonempty"] else np.zeros((R, S))
            assert (of(c["kf_begin"] + 65535) != of(c["kf_begin"])).any()                   # the second chunk's first keyframe is not the first chunk's
    assert in_lds == {True, False}
    assert ltm.sc_paths(64, 64) == (True, False) and ltm.sc_paths(64, 65) == (False, False) and sc.many_keyframes_case(3)["kf_begin"] == 3


def test_every_case_names_a_branch():
    cases = sc.all_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    assert all(c["branch"] and c["family"] for c in cases)
    assert {c["family"] for c in cases} == {"pair", "known", "candidates", "exhaustive", "nonfinite", "descriptors"}
