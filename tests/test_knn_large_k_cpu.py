"""CPU suite: the long-list kNN bounds (GEOT_KNN_KMAX_HEAP / GEOT_KNN_KMAX_SORTED) and the host-only contracts around
them.  Every call below returns before any launch, so no GPU is needed."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1        # hipErrorInvalidValue


@pytest.fixture(scope="module")
def lib():
    from geot_amd import build, _lib
    build.build()
    return _lib.load()


def _header_define(name):
    text = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


def test_header_states_the_bounds_the_binding_uses():
    from geot_amd import _lib
    assert _header_define("GEOT_KNN_KMAX_HEAP") == _lib.KNN_KMAX_HEAP >= 1000       # the reference's best_dist[1000]
    assert _header_define("GEOT_KNN_KMAX_SORTED") == _lib.KNN_KMAX_SORTED >= 4096


def test_out_of_range_k_is_refused_before_any_launch(lib):
    from geot_amd import _lib
    H, S = _lib.KNN_KMAX_HEAP, _lib.KNN_KMAX_SORTED
    null = None
    for ns in (-1, H + 1, 1 << 20):
        assert lib.geot_knnquery_heap(1, 4, ns, null, null, null, null, null, null, null) == INVALID, ns
        assert lib.geot_knnquery_heap_ws(1, 4, 4, ns, null, null, null, null, null, null, null, 0, null) == INVALID, ns
    for k in (-1, S + 1, 1 << 20):
        assert lib.geot_knn_sorted(1, 4, 4, k, null, null, null, null, null) == INVALID, k
        assert lib.geot_knn_sorted_ws(1, 4, 4, k, null, null, null, null, null, 0, null) == INVALID, k
    # at the bounds, empty problems are accepted (nothing to launch)
    assert lib.geot_knnquery_heap(0, 0, H, null, null, null, null, null, null, null) == 0
    assert lib.geot_knnquery_heap_ws(0, 4, 4, H, null, null, null, null, null, null, null, 0, null) == 0
    assert lib.geot_knn_sorted(0, 4, 4, S, null, null, null, null, null) == 0
    assert lib.geot_knn_sorted_ws(1, 0, 4, S, null, null, null, null, null, 0, null) == 0


def test_heap_ws_bytes_are_o_queries_for_long_lists(lib):
    """From nsample 64 on, pointops.knn's workspace is the list of uncertified queries and its count: 16-byte
    multiples, monotone in the number of queries, the same for every nsample."""
    from geot_amd import _lib
    sizes = []
    for b, m_per in ((1, 1), (1, 1000), (2, 1000), (8, 24000)):
        per_k = {lib.geot_knnquery_heap_ws_bytes(b, 24000, m_per, ns) for ns in (64, 100, 257, 1000, _lib.KNN_KMAX_HEAP)}
        assert len(per_k) == 1, per_k
        w = per_k.pop()
        assert w % 16 == 0 and 4 * b * m_per < w <= 4 * b * m_per + 32
        sizes.append(w)
    assert sizes == sorted(sizes)
    # 8 x 24000 queries at nsample 1000: under 1 MB (the (k+1)-list layout would need ~1.5 GB)
    assert lib.geot_knnquery_heap_ws_bytes(8, 24000, 24000, 1000) < 1 << 20
    assert lib.geot_knnquery_heap_ws_bytes(-1, 24000, 24000, 1000) == -1
    assert lib.geot_knnquery_heap_ws_bytes(1, 24000, 24000, -1) == -1


def test_grid_stays_at_k_64(lib, monkeypatch):
    monkeypatch.delenv("GEOT_NN_IMPL", raising=False)
    assert lib.geot_knn_grid_eligible(1, 24000, 24000, 64) == 1
    for k in (65, 257, 1000, 4096):
        assert lib.geot_knn_grid_eligible(1, 24000, 24000, k) == 0
        assert lib.geot_knn_grid_eligible(8, 24000, 24000, k) == 0
