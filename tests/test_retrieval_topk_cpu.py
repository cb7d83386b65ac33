"""CPU: the yardstick of the top-K search (tests/retrieval_topk_reference.py) against a second definition, its interval checker
topk_valid against the results it must accept and the defects it must reject, and the conditions the GPU tests
(tests/test_retrieval_topk_gpu.py) rely on, asserted on the seeded inputs alone."""
import numpy as np
import pytest
import torch

from tests import retrieval_reference as rr
from tests import retrieval_topk_reference as tr

REALISTIC = [(21, 333, 67, 512, 10), (22, 640, 200, 768, 10), (41, 700, 5000, 64, 10), (41, 700, 5000, 64, 64)]


@pytest.mark.parametrize("Nt,Ni,E", [(5, 3, 64), (127, 129, 512), (333, 67, 768)])
@pytest.mark.parametrize("k", [1, 10, 64])
def test_sort_and_selection_agree_where_ties_are_real(Nt, Ni, E, k):
    V, T, _ = rr.exact_case(100 + Nt, Nt, Ni, E)
    for Q, X in ((T, V), (V, T)):
        idx, val = tr.topk(Q, X, k)
        idx2, val2 = tr.topk_by_selection(Q, X, k)
        assert np.array_equal(idx, idx2) and np.array_equal(val, val2)
        kk = min(k, X.shape[0])
        assert (idx[:, kk:] == -1).all() and np.isneginf(val[:, kk:]).all() and (idx[:, :kk] >= 0).all()


def test_exact_case_has_ties_inside_and_at_the_last_place():
    """the index rule is exercised: most rows of (333, 67, 768) have equal scores inside the first 11 places, and a fifth have
    them exactly across the boundary of k = 10"""
    V, T, _ = rr.exact_case(100 + 333, 333, 67, 768)
    _, val = tr.topk(T, V, 11)
    assert np.mean((val[:, :-1] == val[:, 1:]).any(axis=1)) > 0.8
    assert np.mean(val[:, 9] == val[:, 10]) > 0.15


def _fp32_topk(Q, X, k):
    s = torch.from_numpy(Q) @ torch.from_numpy(X).T
    val, idx = torch.sort(s, dim=1, descending=True, stable=True)
    kk = min(k, X.shape[0])
    return idx[:, :kk].numpy(), val[:, :kk].numpy()


@pytest.mark.parametrize("seed,Nt,Ni,E,k", REALISTIC)
def test_realistic_cases_are_determined_and_both_results_are_accepted(seed, Nt, Ni, E, k):
    V, T, _ = rr.realistic_case(seed, Nt, Ni, E)
    b = rr.dot_gap(E) / 2
    for Q, X in ((T, V), (V, T)):
        s64 = tr.scores(Q, X)
        idx, val = tr.topk_of_scores(s64, k)
        bad, share = tr.topk_valid(s64, idx, val, k, b)
        assert bad == [] and share >= 0.9, (bad, share)     # the interval cannot hide a failure
        idx32, val32 = _fp32_topk(Q, X, k)
        assert val32.dtype == np.float32
        bad, _ = tr.topk_valid(s64, idx32, val32, k, b)
        assert bad == [], bad


def test_the_checker_rejects_small_defects():
    seed, Nt, Ni, E, k = REALISTIC[0]
    V, T, _ = rr.realistic_case(seed, Nt, Ni, E)
    b = rr.dot_gap(E) / 2
    s64 = tr.scores(T, V)
    idx, val = _fp32_topk(T, V, k)
    assert tr.topk_valid(s64, idx, val, k, b)[0] == []
    gaps = val[:, :-1].astype(np.float64) - val[:, 1:]
    q, p = (int(x[0]) for x in np.nonzero(gaps > 4 * b))      # two adjacent entries farther apart than the bound

    def rejected(i, v, what):
        bad, _ = tr.topk_valid(s64, i, v, k, b)
        assert bad, f"{what}: accepted"
        return " ".join(bad)

    i, v = idx.copy(), val.copy()
    i[q, [p, p + 1]], v[q, [p, p + 1]] = i[q, [p + 1, p]], v[q, [p + 1, p]]
    assert "order" in rejected(i, v, "two entries swapped")
    i = idx.copy()
    i[q, [p, p + 1]] = i[q, [p + 1, p]]
    assert "score off" in rejected(i, val, "two indices swapped under their scores")
    i = idx.copy()
    i[q, p + 1] = i[q, p]
    assert "duplicated" in rejected(i, val, "a duplicated index")
    i2, v2 = _fp32_topk(T, V, k + 1)
    q0 = int(np.nonzero(v2[:, 0].astype(np.float64) - v2[:, k] > 4 * b)[0][0])
    i, v = idx.copy(), val.copy()
    i[q0], v[q0] = i2[q0, 1:], v2[q0, 1:]
    assert "not returned" in rejected(i, v, "the best entry dropped")
    v = val.copy()
    v[q, p] += np.float32(4 * b)
    assert "score off" in rejected(idx, v, "a score off by 4 b")
    v = val.copy()
    v[q, k - 1] = -np.inf
    assert rejected(idx, v, "a padded place inside the list")


def test_padding_is_checked():
    V, T, _ = rr.exact_case(105, 5, 3, 64)
    s64 = tr.scores(T, V)
    idx, val = tr.topk_of_scores(s64, 5)
    assert tr.topk_valid(s64, idx, val, 5, 0.0)[0] == []
    idx[2, 4] = 0
    assert any("padding" in m for m in tr.topk_valid(s64, idx, val, 5, 0.0)[0])
