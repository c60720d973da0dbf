"""posfeat_amd.matchers.match_pairs (matchpairs.hip) against the per-pair
matchers (match.hip) on the same device: bit-identical, no tolerance -- both
run the same tile loop and each similarity is one K = 128 fp32 chain whose
bits do not depend on how the A rows are split.

The sets have the sizes [1, 2, 31, 64, 129, 300, 1000, 2049] (below, at and
above the 32-row MFMA block, the 64-row LDS step and the 128-column tile; more
than one column block; a ragged last block).  The list below has ~24 pairs and
far fewer than two rounds of resident workgroups, so the plan cuts the A rows
into ranges of 128: every side whose A set has 129, 300, 1000 or 2049 rows is
split (2, 3, 8 and 17 ranges), the sides over 1..64 rows are not;
test_plan_splits asserts this through posfeat_match_pairs_splits."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import match_ref as mr

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 31, 64, 129, 300, 1000, 2049]
# every size on each side (the ring), set 6 against five others (the HPatches
# pattern), self pairs, (6, 7) in both orders
PAIRS = ([(i, (i + 1) % 8) for i in range(8)] + [(6, j) for j in (2, 3, 4, 5, 1)] +
         [(7, 7), (4, 4), (7, 6), (0, 0), (3, 6), (7, 2)])
_CACHE = {}


def _sets():
    if "sets" not in _CACHE:
        sets = []
        for k in range(4):   # (1, 2), (31, 64), (129, 300), (1000, 2049): true correspondences
            sets += list(mr.seeded_descriptors(50 + k, SIZES[2 * k], SIZES[2 * k + 1]))
        _CACHE["sets"] = sets
    return _CACHE["sets"]


def _per_pair(fn_name, pairs, **kw):
    """the existing per-pair function on each pair, computed once per (function, args)"""
    from posfeat_amd import matchers as M
    key = (fn_name, tuple(pairs), tuple(sorted(kw.items())))
    if key not in _CACHE:
        sets = _sets()
        _CACHE[key] = [getattr(M, fn_name)(sets[i], sets[j], **kw) for i, j in pairs]
    return _CACHE[key]


def test_plan_splits(gpu):
    from posfeat_amd import _lib
    set_off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    pairs = np.asarray(PAIRS, np.int32)
    ns = np.zeros(2 * len(PAIRS), np.int32)
    assert _lib.lib().posfeat_match_pairs_splits(
        ctypes.c_void_p(set_off.ctypes.data), 8, ctypes.c_void_p(pairs.ctypes.data), len(PAIRS),
        ctypes.c_void_p(ns.ctypes.data)) == 0
    want = {1: 1, 2: 1, 31: 1, 64: 1, 129: 2, 300: 3, 1000: 8, 2049: 17}
    for p, (i, j) in enumerate(PAIRS):
        # side 2p streams the rows of set j, side 2p + 1 those of set i
        assert (ns[2 * p], ns[2 * p + 1]) == (want[SIZES[j]], want[SIZES[i]]), (p, i, j)
    assert (ns > 1).sum() >= 1


@pytest.mark.parametrize("matcher,fn,kw", [
    ("mnn", "mnn_matcher", {}),
    ("ratio", "ratio_matcher", {}),                       # the default ratio, 0.95
    ("mnn_ratio", "mutual_nn_ratio_matcher", {}),
    ("ratio", "ratio_matcher", {"ratio": 0.95}),
    ("mnn_ratio", "mutual_nn_ratio_matcher", {"ratio": 0.8}),
])
def test_match_pairs_bit_identical_to_per_pair(gpu, matcher, fn, kw):
    from posfeat_amd import matchers as M
    # the ratio matchers raise for a 1-row side (as the per-pair functions do:
    # test_edge_cases), so their list leaves out the pairs with set 0
    pairs = [p for p in PAIRS if matcher == "mnn" or 0 not in p]
    sets = _sets()
    got = M.match_pairs(sets, pairs, matcher=matcher, **kw)
    ref = _per_pair(fn, pairs, **kw)
    assert len(got) == len(pairs)
    for (i, j), g, r in zip(pairs, got, ref):
        assert g.dtype == np.int64 and g.ndim == 2 and g.shape[1] == 2
        assert np.array_equal(g, r), (matcher, i, j)
        if i == j and matcher == "mnn":                   # a self pair is the identity
            assert np.array_equal(g, np.stack([np.arange(SIZES[i])] * 2, 1))
    assert sum(len(g) for g in got) > 1000                # real matches were compared
    if matcher == "mnn":
        # device tensors give the same; so does a second call (no state)
        dev = [torch.from_numpy(s).to(gpu) for s in sets]
        for g, r in zip(M.match_pairs(dev, pairs), ref):
            assert np.array_equal(g, r)


def test_tie_rule_inside_a_batch(gpu):
    """exact duplicate rows as one pair among others: the first index wins"""
    from posfeat_amd import matchers as M
    rs = np.random.RandomState(5)
    d1 = rs.randn(300, 128).astype(np.float32)
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    d2 = np.concatenate([d1[:100], d1[:100], d1[100:]], 0)   # d2 rows j and j+100 tie
    sets = _sets()
    descs = [sets[5], d1, d2, sets[6]]
    pairs = [(0, 3), (1, 2), (3, 0), (2, 1), (2, 2)]
    got = M.match_pairs(descs, pairs)
    np.testing.assert_array_equal(got[1], mr.mnn_matcher(d1, d2))
    assert got[1][:100, 1].tolist() == list(range(100))      # first occurrence
    assert len(got[1]) == 300
    # d2 x d1: the tie is between rows; rows 100..199 of d2 lose their d1 row to rows 0..99
    keep = np.r_[0:100, 200:400]
    np.testing.assert_array_equal(got[3], np.stack([keep, np.arange(300)], 1))
    # d2 x d2: rows j and j + 100 tie on both sides; the lower index takes both
    np.testing.assert_array_equal(got[4], np.stack([keep, keep], 1))
    for p, (i, j) in enumerate(pairs):
        np.testing.assert_array_equal(got[p], M.mnn_matcher(descs[i], descs[j]))


def test_edge_cases(gpu):
    from posfeat_amd import matchers as M
    sets = _sets()
    empty = np.zeros((0, 128), np.float32)
    assert M.match_pairs(sets, []) == []
    assert M.match_pairs([], []) == []
    # an empty set on either side, among live pairs and alone
    got = M.match_pairs([sets[4], empty, sets[5]], [(0, 1), (0, 2), (1, 2), (1, 1), (2, 0)])
    for g in (got[0], got[2], got[3]):
        assert g.shape == (0, 2) and g.dtype == np.int64
    np.testing.assert_array_equal(got[1], M.mnn_matcher(sets[4], sets[5]))
    np.testing.assert_array_equal(got[4], M.mnn_matcher(sets[5], sets[4]))
    got = M.match_pairs([sets[4], empty], [(0, 1), (1, 0)])
    assert [g.shape for g in got] == [(0, 2), (0, 2)]
    # one descriptor on a side: the ratio matchers raise, mnn does not
    for matcher in ("ratio", "mnn_ratio"):
        for pairs in ([(0, 4)], [(4, 0)], [(4, 5), (5, 0)]):
            with pytest.raises(RuntimeError):
                M.match_pairs(sets, pairs, matcher=matcher)
    assert M.match_pairs(sets, [(0, 4)])[0].shape == (1, 2)
    with pytest.raises(NotImplementedError):
        M.match_pairs([np.zeros((4, 64), np.float32)] * 2, [(0, 1)])
    with pytest.raises(IndexError):
        M.match_pairs(sets, [(0, 8)])
    with pytest.raises(ValueError):
        M.match_pairs(sets, [(0, 1)], matcher="nearest")
