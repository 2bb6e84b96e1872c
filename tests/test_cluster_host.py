"""not-gpu: the clustering entry points exist at every layer (header, ctypes binding, apply_r's options), and the numpy restatement of the
member selection (tests/cluster_oracle.py) is the list logic of apply_r.createClusterImages."""
import os
import re

import numpy as np
import pytest

import cluster_oracle as clo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gr_kmeans_dev", "gr_cosine_assign_dev", "gr_cluster_members_dev", "gr_cluster_faces_dev")


def test_header_declares_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ganrev.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    lua = open(os.path.join(ROOT, "gan-reverser_amd", "lua", "hipnn.lua")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, lua), name


def test_context_has_the_methods():
    import ganrev._lib as L
    for name in ("kmeans_dev", "cosine_assign_dev", "cluster_members_dev", "cluster_faces_dev"):
        assert callable(getattr(L.Context, name, None)), name
    for name in ENTRY_POINTS:
        assert name in L.EXPORTED_SYMBOLS, name


def test_parse_knows_resident_and_rejects_it_with_host(capsys):
    from ganrev import apply_r
    assert apply_r.parse(["--resident"]).resident is True
    assert apply_r.parse([]).resident is False
    assert apply_r.parse(["--resident", "--render"]).render is True
    with pytest.raises(SystemExit) as e:
        apply_r.parse(["--resident", "--host"])
    assert e.value.code == 2
    assert "--resident" in capsys.readouterr().err


def todays_lists(label, sim, k, m):
    """the lists apply_r.createClusterImages builds (apply_r.lua:218-227): its own selection, apply_r.selectClusterMembers"""
    from ganrev import apply_r
    return [[(int(r), float(sim[r])) for r in keep] for keep in apply_r.selectClusterMembers(label, sim, k, m)]


def same_lists(a, b):
    """lists of (row, similarity) compared exactly: the similarity by its bits (a NaN equals a NaN, -0 differs from +0)"""
    key = lambda cl: [(r, np.float32(v).tobytes()) for r, v in cl]
    return [key(c) for c in a] == [key(c) for c in b]


@pytest.mark.parametrize("n,k,m,nan", [(37, 1, 1, False), (37, 20, 71, False), (600, 20, 71, False), (600, 20, 1, False), (600, 5, 128, True),
                                       (1300, 32, 71, True), (50, 4, 128, False)])
def test_oracle_is_todays_list_logic(n, k, m, nan):
    label, sim = clo.member_case(n, k, m, seed=n + k + m, nan=nan)
    rows, sims, kept, sizes = clo.cluster_members(label, sim, k, m)
    lists = [[(int(r), float(v)) for r, v in zip(rows[j, :kept[j]], sims[j, :kept[j]])] for j in range(k)]
    assert same_lists(lists, todays_lists(label, sim, k, m))
    assert np.array_equal(sizes, np.bincount(label, minlength=k)[:k])
    assert np.array_equal(kept, np.minimum(sizes, m))
    for j in range(k):
        assert (rows[j, kept[j]:] == -1).all() and (sims[j, kept[j]:].view(np.uint32) == 0).all()
    if k > 1:
        assert sizes[k - 1] == 0                                        # an empty cluster
    if n == 50:
        assert (sizes <= m).all()                                       # m larger than every cluster
    if n >= 600 and m > 1:
        j = 0                                                           # exact ties cross the cut-off: the tie rule decided
        left = sim[[r for r in np.nonzero(label == j)[0] if r not in set(rows[j])]]
        assert sizes[j] > m and sims[j, m - 1] == np.nanmax(left)


def test_oracle_duplicate_rows_nan_and_zeros():
    label = np.zeros(8, np.int32)
    sim = np.array([0.5, np.nan, 0.5, -0.0, 0.0, np.nan, 0.9, 0.5], np.float32)
    rows, sims, kept, sizes = clo.cluster_members(label, sim, 2, 6)
    assert list(rows[0]) == [6, 0, 2, 7, 3, 4] and kept[0] == 6 and sizes[0] == 8
    assert list(rows[1]) == [-1] * 6 and kept[1] == 0 and sizes[1] == 0
    rows, _, kept, _ = clo.cluster_members(label, sim, 1, 8)
    assert list(rows[0]) == [6, 0, 2, 7, 3, 4, 1, 5]                    # NaN last, by row
    assert same_lists([[(int(r), float(sim[r])) for r in rows[0]]], todays_lists(label, sim, 1, 8))
