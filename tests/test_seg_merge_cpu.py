"""The restatement of despeckling by merging (tests/cc_merge_reference.py) checked on its own, without a GPU: against an
independent scipy.ndimage formulation on seeded random maps, the scene identities of the definition (include/segclip_hip.h,
segclip_seg_sieve) that the kernel tests then lean on, the composition of rounds, the Despeckle argument errors and the agreement
of the header's prototypes with the ctypes signatures."""
import numpy as np
import pytest
import torch

from segclip_amd import ops
from segclip_amd.segmentation import Despeckle, despeckle
from tests import cc_merge_reference as cm
from tests import cc_reference as cc
from tests.helpers import header_declaration

TH, TW = ops.SEG_CC_TILE


def scipy_round(L, connectivity, skip_label, min_area):
    """One round, formulated with scipy.ndimage alone: label per class, the cross dilation of every small component to find
    its neighbours, the winner by (largest area, smallest label) as a tuple comparison -> (map, orphan mask)"""
    ndi = pytest.importorskip("scipy.ndimage")
    cross = ndi.generate_binary_structure(2, 1)
    structure = np.ones((3, 3), dtype=int) if connectivity == 8 else cross
    comp = np.zeros(L.shape, dtype=np.int64)          # 0: skipped; components numbered from 1 over all classes
    areas, labels = [0], [-1]
    for v in np.unique(L).tolist():
        if v == skip_label:
            continue
        lab, n = ndi.label(L == v, structure=structure)
        comp[lab > 0] = lab[lab > 0] + len(areas) - 1
        areas += np.bincount(lab.reshape(-1), minlength=n + 1)[1:].tolist()
        labels += [v] * n
    areas, labels = np.asarray(areas), np.asarray(labels)
    out, orphans = L.copy(), np.zeros(L.shape, dtype=bool)
    for k in range(1, len(areas)):
        if areas[k] >= min_area:
            continue
        mask = comp == k
        ring = ndi.binary_dilation(mask, structure=cross) & ~mask
        cand = [c for c in np.unique(comp[ring]).tolist() if c > 0 and areas[c] >= min_area]
        if cand:
            out[mask] = labels[min(cand, key=lambda c: (-areas[c], labels[c]))]
        else:
            orphans[mask] = True
    return out, orphans


def random_map(seed):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(1, 12)), int(rng.integers(1, 16))
    n_labels = int(rng.integers(2, 5))
    side = int(rng.integers(1, 3))
    small = rng.integers(0, n_labels, size=((h + side - 1) // side, (w + side - 1) // side)).astype(np.uint8)
    return np.ascontiguousarray(np.kron(small, np.ones((side, side), dtype=np.uint8))[:h, :w])


@pytest.mark.parametrize("orphan_fill", [None, 77])
@pytest.mark.parametrize("skip", [None, 0])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_against_scipy(connectivity, skip, orphan_fill):
    """30 seeded maps per setting, 240 cases in all, min_area drawn per map, rounds 1 and 2"""
    changed = orphaned = 0
    for seed in range(30):
        L = random_map(1000 + seed)
        min_area = int(np.random.default_rng(seed).integers(2, 9))
        want, orphans = scipy_round(L, connectivity, skip, min_area)
        got, got_orphans = cm.merge_round(L, connectivity, skip, min_area)
        assert np.array_equal(got, want) and np.array_equal(got_orphans, orphans), seed
        filled = want.copy()
        if orphan_fill is not None:
            filled[orphans] = orphan_fill
        assert np.array_equal(cm.merge(L, connectivity, skip, min_area, orphan_fill, 1), filled), seed
        want2, orphans2 = scipy_round(want, connectivity, skip, min_area)     # round 2 runs on round 1's map, orphans unfilled
        if orphan_fill is not None:
            want2[orphans2] = orphan_fill
        assert np.array_equal(cm.merge(L, connectivity, skip, min_area, orphan_fill, 2), want2), seed
        if skip is not None:
            assert np.array_equal(got[L == skip], L[L == skip]) and not orphans[L == skip].any()
        changed += int((want != L).sum())
        orphaned += int(orphans.sum())
    assert changed > 100 and orphaned > 0, "the random maps do not exercise the merge"


def test_merging_restores_the_scene_without_a_background_class():
    scene, speckled = cm.no_background_scene()
    assert scene.shape == (48, 80) and sorted(np.unique(scene).tolist()) == [1, 2, 3] == sorted(np.unique(speckled).tolist())
    assert int((speckled != scene).sum()) == 24
    for connectivity in (4, 8):
        filled = cc.components([speckled], connectivity, None, 16, 0)[3][0]
        assert int((filled == 0).sum()) == 24 and 0 not in scene          # a class that the scene does not contain
        assert np.array_equal(cm.merge(speckled, connectivity, None, 16), scene)


def test_nested_specks_need_two_rounds():
    a = cm.nested_specks()
    for connectivity in (4, 8):
        one, orphans = cm.merge_round(a, connectivity, None, 9)
        assert int(orphans.sum()) == 1 and one[5, 6] == 3 and int((one != 1).sum()) == 1
        assert np.array_equal(cm.merge(a, connectivity, None, 9, None, 2), np.ones_like(a))
        assert cm.merge(a, connectivity, None, 9, 0, 1)[5, 6] == 0            # the orphan rule after a last round of one


def test_a_4_connected_checkerboard_consists_of_orphans():
    a = cm.checkerboard()
    out, orphans = cm.merge_round(a, 4, None, 2)
    assert orphans.all() and np.array_equal(out, a)
    assert bool((cm.merge(a, 4, None, 2, 9, 3) == 9).all())
    out8, orphans8 = cm.merge_round(a, 8, None, 2)                            # 8-connected: two kept components
    assert not orphans8.any() and np.array_equal(out8, a)


def test_equal_areas_give_the_smaller_label():
    a = cm.area_tie()
    assert a.tolist() == [[5, 5, 5, 5, 9, 3, 3, 3, 3]]
    assert cm.merge(a, 8, None, 2).tolist() == [[5, 5, 5, 5, 3, 3, 3, 3, 3]]
    assert cm.merge(a[:, ::-1], 4, None, 2).tolist() == [[3, 3, 3, 3, 3, 5, 5, 5, 5]]
    b = np.asarray([[5, 5, 5, 5, 5, 9, 3, 3, 3, 3]], dtype=np.uint8)             # the larger area beats the smaller label
    assert cm.merge(b, 8, None, 2)[0, 5] == 5


def test_a_diagonal_touch_is_no_contact():
    a = cm.diagonal_only(TH, TW)
    for connectivity in (4, 8):
        out, orphans = cm.merge_round(a, connectivity, None, 2)
        assert orphans[TH, TW] and int(orphans.sum()) == 1 and out[TH, TW] == 9
        assert int((out != 0).sum()) == 1                                     # its four neighbours touched the background
        assert not cm.merge(a, connectivity, None, 2, None, 2).any()


def test_noise_reaches_a_fixed_point():
    a = cm.noise()
    assert a.shape == (24, 70) and sorted(np.unique(a).tolist()) == [0, 1, 2]
    steps = cm.chain(a, 4, None, 6, 3)
    left = [cm.small_left(m, 4, None, 6) for m, _ in steps]
    assert cm.small_left(a, 4, None, 6) > 100 and left[0] > 0 and left[1:] == [0, 0], left      # two rounds, none left
    assert np.array_equal(steps[2][0], steps[1][0]), "a map without small components is a fixed point"
    assert not steps[2][1].any()
    assert not np.array_equal(steps[1][0], steps[0][0])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_rounds_compose(connectivity):
    for L, skip, min_area in ((cm.noise(h=15, w=31), None, 5), (cm.noise(seed=7, h=15, w=31), 0, 7), (cm.frame_and_skip(), 255, 4)):
        cur = L
        for rounds in (1, 2, 3):
            cur, orphans = cm.merge_round(cur, connectivity, skip, min_area)
            assert np.array_equal(cm.merge(L, connectivity, skip, min_area, None, rounds), cur)
            filled = cur.copy()
            filled[orphans] = 200
            assert np.array_equal(cm.merge(L, connectivity, skip, min_area, 200, rounds), filled)
        assert np.array_equal(cm.merge(L, connectivity, skip, 0), L) and np.array_equal(cm.merge(L, connectivity, skip, 1, 9, 3), L)


def test_the_kernel_test_maps_are_what_they_are_there_for():
    a = cm.corner_speck(TH, TW)
    ids = cc.label(a, 4)
    y, x = TH - 1, TW - 1
    around = [(y, x - 1), (y - 1, x), (y, x + 1), (y + 1, x)]
    assert [int(a[p]) for p in around] == [1, 2, 3, 4]
    assert [int((ids == ids[p]).sum()) for p in around] == [TW - 1, TH - 1, 40, TH + TW]
    assert len({(p[0] // TH, p[1] // TW) for p in around}) == 3
    assert cm.merge(a, 4, None, 2)[y, x] == 4
    b = cm.speck_across_tiles(TH, TW)
    assert b.shape == (2, 2 * TW + 10) and bool((cm.merge(b, 8, None, 9)[:, TW - 2:TW + 2] == 2).all())
    s = cm.serpentine_tail(TH, TW)
    assert int((s == 7).sum()) == 1 and len(np.unique(cc.label(s, 4))) == 3
    assert 7 not in cm.merge(s, 4, None, 2)
    k = cm.key_above_bit_16()
    assert k.shape == (272, 272) and int((k == 3).sum()) == 65636 and int((k == 2).sum()) == 5000
    y, x = np.argwhere(k == 9)[0]
    assert (k[y, x - 1], k[y - 1, x], k[y, x + 1], k[y + 1, x]) == (3, 3, 2, 2)
    assert cm.column().shape == (84, 1) and cm.row().shape == (1, 84)
    want = cm.merge(cm.row(), 8, None, 3)
    assert np.array_equal(cm.merge(cm.column(), 4, None, 3).reshape(-1), want.reshape(-1))
    assert sorted(np.unique(want).tolist()) == [1, 3] and cm.small_left(want, 8, None, 3) == 0


def test_despeckle_arguments():
    d = Despeckle(4)
    assert (d.min_area, d.fill, d.connectivity, d.skip_label, d.merge, d.rounds) == (4, 0, 8, None, False, 1)
    d = Despeckle(16, fill=None, connectivity=4, skip_label=255, merge=True, rounds=8)
    assert (d.min_area, d.fill, d.connectivity, d.skip_label, d.merge, d.rounds) == (16, None, 4, 255, True, 8)
    assert Despeckle(3, merge=True).fill == 0 and Despeckle(3, 7, merge=True, rounds=2).fill == 7
    for bad, match in ((dict(rounds=2), "rounds=2 needs merge=True"), (dict(fill=None), "fill=None.*merge=True"),
                       (dict(merge=True, rounds=0), "rounds is an integer in 1 .. 8"), (dict(merge=True, rounds=9), "rounds is an integer"),
                       (dict(merge=True, rounds=2.0), "rounds is an integer"), (dict(merge=True, rounds=True), "rounds is an integer"),
                       (dict(rounds=0), "rounds is an integer"), (dict(merge=1), "merge is True or False"),
                       (dict(merge=True, fill=256), "fill is an integer in 0 .. 255 or None"), (dict(merge=True, fill=-1), "fill"),
                       (dict(merge=True, fill=1.5), "fill"), (dict(fill=256), "fill is an integer in 0 .. 255, got"),
                       (dict(merge=True, connectivity=6), "connectivity"), (dict(merge=True, skip_label=256), "skip_label")):
        with pytest.raises(ValueError, match=match):
            Despeckle(4, **bad)
    with pytest.raises(ValueError, match="min_area"):
        Despeckle(-1, merge=True)
    with pytest.raises(ValueError, match="rounds=3 needs merge=True"):
        despeckle([torch.zeros(2, 2, dtype=torch.uint8)], 2, rounds=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        despeckle([torch.zeros(2, 2, dtype=torch.uint8)], 2, merge=True)
    table, n_blocks, side = ops.seg_components_table([(3, 3)], [0], "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_sieve(table, n_blocks, torch.zeros(9, dtype=torch.uint8), min_area=2)
    assert ops.SEG_SIEVE_MAX_ROUNDS == 8


def test_header_and_ctypes_prototypes_agree():
    args = header_declaration("segclip_seg_sieve")
    assert [a.rsplit(" ", 1)[1].lstrip("*") for a in args] == [
        "images", "B", "n_blocks", "max_side", "labels", "labels_bytes", "connectivity", "skip_label", "min_area", "orphan_fill",
        "rounds", "cleaned", "cleaned_bytes", "ws", "ws_bytes", "stream"]
