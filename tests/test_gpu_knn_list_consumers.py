"""The kernels that keep a k-best list (csrc/ltm_knn_list.h, and the copies of it that the search and normals kernels write out) agree with
each other on the device, bit for bit: the statistical filter's per-point distance
is the ascending sum over the rows of the index's own kNN search (the list without payload against the list with the index word, registers and LDS), and the
kNN rows of a register form are the head of the rows of the next larger form (k = 4 | 5, 8 | 9, and 16 in registers | 17 in LDS).  Both follow from the tie
rule (smaller distance, then smaller index; equal distances give equal terms of the sum), on clouds of 2, 33 and 300 points and on the integer lattice,
where most distances tie."""
import numpy as np
import pytest

import outlier_cases as oc
from tools import outlier_numpy as oref

pytestmark = pytest.mark.gpu

CLOUDS = {"n2": oc._xyzi(oc.blob(2, 41), 5), "n33": oc._xyzi(oc.blob(33, 42), 5), "n300": oc._xyzi(oc.blob(300, 20), 6), "lattice": oc._xyzi(oc.lattice(), 12)}
MEAN_KS = (1, 3, 4, 7, 8, 15, 16, 17, 63)
HEADS = ((4, 5), (8, 9), (16, 17))


@pytest.fixture(scope="module")
def shared(gpu_ctx):
    """per cloud: the uploaded cloud, its index and the kNN rows of the cloud against itself, made on first use and left unchanged"""
    cache = {"rows": {}}
    for name, pts in CLOUDS.items():
        cloud = gpu_ctx.upload(pts)
        cache[name] = (cloud, gpu_ctx.search_index(cloud))
    yield cache
    for name in CLOUDS:
        cloud, index = cache[name]
        index.close()
        cloud.free()


def _rows(shared, name, k):
    if (name, k) not in shared["rows"]:
        cloud, index = shared[name]
        shared["rows"][(name, k)] = index.knn(cloud, k)
    return shared["rows"][(name, k)]


@pytest.mark.parametrize("mean_k", MEAN_KS)
@pytest.mark.parametrize("name", list(CLOUDS))
def test_filter_distance_is_the_sum_over_the_knn_rows(gpu_ctx, shared, name, mean_k):
    n = len(CLOUDS[name])
    idx, d2 = _rows(shared, name, mean_k + 1)
    kk = min(mean_k + 1, n)
    assert (idx[:, :kk] >= 0).all() and np.isfinite(d2[:, :kk]).all() and (d2[:, 0] == 0.0).all()
    want = oref._distance_from_sorted_d2(d2[:, :kk], mean_k)      # float32(sum over ranks 1 .. kk-1 of sqrt(float64(d2)) / mean_k), terms in ascending rank
    with shared[name][1].statistical_outliers(mean_k, 1.0) as out:
        got = out.distances()
    assert got.dtype == np.float32 and got.shape == (n,)
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), f"{name}, mean_k {mean_k}: {int((got != want).sum())} of {n} distances differ"


@pytest.mark.parametrize("k_head,k_next", HEADS)
@pytest.mark.parametrize("name", list(CLOUDS))
def test_rows_of_a_form_are_the_head_of_the_next_forms_rows(shared, name, k_head, k_next):
    idx_a, d2_a = _rows(shared, name, k_head)
    idx_b, d2_b = _rows(shared, name, k_next)
    assert idx_a.shape == (len(CLOUDS[name]), k_head)
    assert idx_a.tobytes() == np.ascontiguousarray(idx_b[:, :k_head]).tobytes(), f"{name}: indices at k = {k_head} are not the head of those at k = {k_next}"
    assert d2_a.view(np.uint32).tobytes() == np.ascontiguousarray(d2_b[:, :k_head]).view(np.uint32).tobytes(), f"{name}: distances at k = {k_head} / {k_next}"
