"""CPU: the retrieval yardstick (tests/retrieval_reference.py) against a second, independent definition and against cases
worked by hand; metrics_from_hist against the metrics of the rank vectors; image_index_from_cut_off_points; and the
conditions on the seeded inputs of tests/test_retrieval_gpu.py that need no GPU."""
import numpy as np
import pytest
import torch

from segclip_amd.retrieval import image_index_from_cut_off_points, metrics_from_hist
from tests import retrieval_reference as rr


def test_hand_case_with_a_tie():
    """3 images on the axes; caption 0 lies between images 0 and 1 (an exact tie), caption 1 prefers image 2 to its own."""
    V = np.eye(3, 4)
    T = np.array([[1.0, 1.0, 0.0, 0.0],      # g = 0: sim (1, 1, 0): image 1 ties and does not count -> rank 0
                  [0.0, 0.5, 1.0, 0.0],      # g = 1: sim (0, .5, 1): image 2 is above -> rank 1
                  [0.0, 0.0, 2.0, 0.0],      # g = 2: sim (0, 0, 2) -> rank 0
                  [0.0, 0.25, 0.0, 0.0]])    # g = 1: sim (0, .25, 0) -> rank 0
    g = np.array([0, 1, 2, 1])
    rank_t2i, rank_i2t = rr.ranks(V, T, g)
    assert rank_t2i.tolist() == [0, 1, 0, 0]
    # image 0: best 1 (caption 0), nobody above.  image 1: best 0.5; caption 0 has 1 -> rank 1.  image 2: best 2 -> rank 0
    assert rank_i2t.tolist() == [0, 1, 0]
    assert rr.metrics(rank_t2i) == dict(R1=75.0, R5=100.0, R10=100.0, MedianR=1.0, MeanR=1.25)
    m = rr.metrics(rank_i2t)
    assert m["R1"] == pytest.approx(200.0 / 3) and m["MedianR"] == 1.0 and m["MeanR"] == pytest.approx(4.0 / 3)


def test_hand_case_image_without_captions():
    """Image 1 has no caption: rank -1, left out of the metrics; it still competes as a candidate of the captions."""
    V = np.array([[1.0, 0.0], [0.6, 0.8], [0.0, 1.0]])
    T = np.array([[0.6, 0.8],     # g = 0: sim (.6, 1, .8): images 1 and 2 above -> rank 2
                  [0.0, 1.0]])    # g = 2: sim (0, .8, 1) -> rank 0
    g = np.array([0, 2])
    rank_t2i, rank_i2t = rr.ranks(V, T, g)
    assert rank_t2i.tolist() == [2, 0]
    # image 0: best .6, caption 1 has 0 -> 0.  image 2: best 1 (caption 1), caption 0 has .8 -> 0
    assert rank_i2t.tolist() == [0, -1, 0]
    assert rr.metrics(rank_i2t) == dict(R1=100.0, R5=100.0, R10=100.0, MedianR=1.0, MeanR=1.0)
    assert rr.metrics(rank_t2i) == dict(R1=50.0, R5=100.0, R10=100.0, MedianR=2.0, MeanR=2.0)
    h_t, h_i = rr.hists(rank_t2i, rank_i2t)
    assert h_t.tolist() == [1, 0, 1] and h_i.tolist() == [2, 0, 0]


def test_hand_case_one_image():
    """Ni = 1: there is no other image, every caption has rank 0; the image's best caption has nobody above it."""
    V = np.array([[0.0, 1.0]])
    T = np.array([[0.0, -1.0], [1.0, 0.0], [0.0, 0.5]])
    g = np.zeros(3, dtype=np.int64)
    rank_t2i, rank_i2t = rr.ranks(V, T, g)
    assert rank_t2i.tolist() == [0, 0, 0] and rank_i2t.tolist() == [0]
    assert rr.ranks_by_argsort(V, T, g)[0].tolist() == [0, 0, 0]


@pytest.mark.parametrize("seed,Nt,Ni,E", [(0, 1, 1, 32), (1, 5, 3, 64), (2, 40, 9, 32), (3, 127, 129, 32), (4, 90, 17, 64)])
def test_reference_against_argsort_definition_with_ties(seed, Nt, Ni, E):
    V, T, g = rr.exact_case(seed, Nt, Ni, E)
    a, b = rr.ranks(V, T, g), rr.ranks_by_argsort(V, T, g)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    if Ni >= 3:
        assert (a[1] == -1).any()


@pytest.mark.parametrize("seed", [5, 6, 7])
def test_reference_against_argsort_definition_random(seed):
    rng = np.random.default_rng(seed)
    Ni, Nt, E = 23, 61, 16
    V, T = rng.standard_normal((Ni, E)), rng.standard_normal((Nt, E))
    g = rng.integers(0, Ni, size=Nt)
    a, b = rr.ranks(V, T, g), rr.ranks_by_argsort(V, T, g)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_interval_brackets_the_ranks():
    V, T, g = rr.realistic_case(11, 120, 31, 64)
    r_t, r_i = rr.ranks(V, T, g)
    lo_t, hi_t, lo_i, hi_i = rr.rank_intervals(V, T, g, 1e-3)
    assert (lo_t <= r_t).all() and (r_t <= hi_t).all() and (lo_t < hi_t).any()
    assert (lo_i <= r_i).all() and (r_i <= hi_i).all()


@pytest.mark.parametrize("seed", range(6))
def test_metrics_from_hist_equals_metrics_from_ranks(seed):
    rng = np.random.default_rng(seed)
    n, bins = [1, 2, 7, 50, 51, 400][seed], [1, 3, 12, 30, 200, 20][seed]
    rank = rng.integers(0, bins, size=n)
    if seed == 3:
        rank[: n // 2] = 0      # an even count whose two middle ranks differ
    want = rr.metrics(rank)
    got = metrics_from_hist(torch.from_numpy(np.bincount(rank, minlength=bins)))
    assert got == want          # integer sums and one division on both sides: no tolerance


def test_metrics_from_hist_leaves_out_nothing_but_the_absent():
    rank_i2t = np.array([3, -1, 0, 0, -1, 12])
    _, h = rr.hists(np.zeros(20, dtype=np.int64), rank_i2t)
    assert metrics_from_hist(torch.from_numpy(h)) == rr.metrics(rank_i2t)
    empty = metrics_from_hist(torch.zeros(4, dtype=torch.int64))
    assert all(np.isnan(v) for v in empty.values())


def test_image_index_from_cut_off_points():
    g = image_index_from_cut_off_points([5, 5, 7, 12])       # image 1 has no sentence
    assert g.dtype == torch.int32 and g.tolist() == [0] * 5 + [2] * 2 + [3] * 5
    assert image_index_from_cut_off_points([]).numel() == 0
    assert image_index_from_cut_off_points(torch.tensor([0, 0, 1])).tolist() == [2]
    # the loader's own layout: five sentences per image
    assert torch.equal(image_index_from_cut_off_points(np.arange(5, 55, 5)), torch.arange(10, dtype=torch.int32).repeat_interleave(5))
    with pytest.raises(ValueError, match="cut_off_points"):
        image_index_from_cut_off_points([3, 2])


# ---------------------------------------------------------------- conditions on the GPU tests' inputs (the reference alone)
EXACT_SHAPES = [(1, 1, 32), (5, 3, 64), (127, 129, 512), (333, 67, 768), (1300, 260, 512)]
REALISTIC = [(21, 333, 67, 512), (22, 640, 200, 768)]   # seed, Nt, Ni, E


@pytest.mark.parametrize("Nt,Ni,E", EXACT_SHAPES)
def test_exact_cases_have_what_the_gpu_test_needs(Nt, Ni, E):
    V, T, g = rr.exact_case(100 + Nt, Nt, Ni, E)
    assert g.shape == (Nt,) and V.shape == (Ni, E) and T.shape == (Nt, E)
    assert np.abs(V).max() <= 1 and np.array_equal(V * 8, np.round(V * 8)) and np.array_equal(T * 8, np.round(T * 8))
    counts = np.bincount(g, minlength=Ni)
    assert counts.max() <= 7
    assert counts[0] >= 1 and counts[Ni - 1] >= 1            # the ground truth in the first and the last image of a tile
    if Ni > 128:
        assert counts[127] >= 1 and counts[128] >= 1
    if Ni >= 3:
        assert (counts == 0).any()
    if Ni >= 64:   # a row with ties above, at and below its threshold
        sim = rr.similarity(V, T)
        found = False
        for t in range(Nt):
            row, thr = np.delete(sim[t], g[t]), sim[t, g[t]]
            above, below = row[row > thr], row[row < thr]
            if (row == thr).any() and np.unique(above).size < above.size and np.unique(below).size < below.size:
                found = True
                break
        assert found


@pytest.mark.parametrize("seed,Nt,Ni,E", REALISTIC)
def test_realistic_cases_are_spread_and_mostly_decided(seed, Nt, Ni, E):
    V, T, g = rr.realistic_case(seed, Nt, Ni, E)
    assert np.allclose(np.linalg.norm(V.astype(np.float64), axis=1), 1, atol=1e-6)
    r_t, r_i = rr.ranks(V, T, g)
    assert r_t.min() == 0 and r_t.max() > 10 and np.unique(r_t).size > 10
    assert r_i.max() > 10
    lo_t, hi_t, lo_i, hi_i = rr.rank_intervals(V, T, g, rr.dot_gap(E))
    share_t, share_i = np.mean(lo_t == hi_t), np.mean(lo_i == hi_i)
    print(f"decided rows {share_t:.3f}, columns {share_i:.3f}; max ranks {r_t.max()}, {r_i.max()}")
    assert share_t >= 0.9 and share_i >= 0.9
