"""CPU: the restatements of components, merge rounds and boundary bands for 16-bit label maps (tests/wide_post_reference.py)
tied to scipy.ndimage on seeded 16-bit maps, and, through the order-preserving injection (every value replaced by its rank, a
uint8 map), to the uint8 restatements that the existing kernel tests lean on.  What the C header and the ctypes binding say about
the three wide entries, and what the host layer refuses without a device."""
import numpy as np
import pytest
import torch

from segclip_amd import _lib, ops
from segclip_amd.segmentation import Boundary, Despeckle, boundary_areas, boundary_bands, components, despeckle
from tests import boundary_reference as bd
from tests import cc_merge_reference as cm
from tests import cc_reference as cc
from tests import wide_post_reference as wp
from tests.helpers import header_declaration

VALUE_SETS = [wp.SHARED_LOW_BYTE, wp.TOP_BIT_AND_SENTINEL, (0, 256, 300, 513, 1023, 40000)]


def random_map(seed, values):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(1, 14)), int(rng.integers(1, 18))
    return wp.blocks(rng, h, w, int(rng.integers(1, 3)), values)


@pytest.mark.parametrize("skip", [None, 65535, 255, 257])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_components_against_scipy(connectivity, skip):
    """ndimage.label per value: the same partition, the same areas and boxes; the id is the first pixel in raster order"""
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), dtype=int) if connectivity == 8 else ndi.generate_binary_structure(2, 1)
    n_components = 0
    for seed in range(24):
        L = random_map(seed, VALUE_SETS[seed % 3])
        ids, area, records, cleaned = (r[0] if isinstance(r, list) else r for r in wp.components([L], connectivity, skip, 3, 77))
        want_ids = np.full(L.shape, -1, dtype=np.int64)
        rows = []
        for v in np.unique(L).tolist():
            if v == skip:
                continue
            lab, n = ndi.label(L == v, structure=structure)
            for k, box in zip(range(1, n + 1), ndi.find_objects(lab)):
                m = lab == k
                first = int(np.flatnonzero(m.reshape(-1))[0])
                want_ids[m] = first
                ys, xs = np.nonzero(m)
                rows.append([0, first, v, int(m.sum()), box[0].start, box[1].start, box[0].stop, box[1].stop, int(ys.sum()), int(xs.sum())])
        rows.sort(key=lambda r: r[1])
        assert np.array_equal(ids, want_ids), seed
        assert np.array_equal(records, np.asarray(rows, dtype=np.int64).reshape(-1, 10)), seed
        want_area = np.zeros(L.shape, dtype=np.int32)
        for r in rows:
            want_area[want_ids == r[1]] = r[3]
        assert np.array_equal(area, want_area), seed
        want_cleaned = L.copy()
        want_cleaned[(want_ids >= 0) & (want_area < 3)] = 77
        assert np.array_equal(cleaned, want_cleaned) and cleaned.dtype == np.uint16, seed
        n_components += len(rows)
    assert n_components > 100


def scipy_round(L, connectivity, skip_label, min_area):
    """one merge round with scipy.ndimage alone; the winner by (largest area, smallest label) as a tuple comparison"""
    ndi = pytest.importorskip("scipy.ndimage")
    cross = ndi.generate_binary_structure(2, 1)
    structure = np.ones((3, 3), dtype=int) if connectivity == 8 else cross
    comp = np.zeros(L.shape, dtype=np.int64)
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


@pytest.mark.parametrize("skip", [None, 65535, 513])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_merge_rounds_against_scipy(connectivity, skip):
    changed = orphaned = 0
    for seed in range(24):
        L = random_map(500 + seed, VALUE_SETS[seed % 3])
        min_area = int(np.random.default_rng(seed).integers(2, 9))
        want, orphans = scipy_round(L, connectivity, skip, min_area)
        got, got_orphans = wp.merge_round(L, connectivity, skip, min_area)
        assert np.array_equal(got, want) and np.array_equal(got_orphans, orphans) and got.dtype == np.uint16, seed
        want2, orphans2 = scipy_round(want, connectivity, skip, min_area)
        want2[orphans2] = 65535
        assert np.array_equal(wp.merge(L, connectivity, skip, min_area, 65535, 2), want2), seed
        changed += int((want != L).sum())
        orphaned += int(orphans.sum())
    assert changed > 100 and orphaned > 0, "the random maps do not exercise the merge"


@pytest.mark.parametrize("d", [1, 2, 5])
def test_bands_against_binary_erosion(d):
    """(M == k) & (band != 0) is mask_to_boundary of class k: the mask minus its d-fold 3 x 3 erosion with a ring of zeros"""
    ndi = pytest.importorskip("scipy.ndimage")
    for seed in range(12):
        m = random_map(900 + seed, VALUE_SETS[seed % 3])
        band = wp.band(m, d)
        assert band.dtype == np.uint8 and band.max() <= 3
        for k in np.unique(m).tolist():
            mask = m == k
            eroded = ndi.binary_erosion(mask, np.ones((3, 3), dtype=bool), iterations=d, border_value=0)
            assert np.array_equal(mask & (band != 0), mask & ~eroded), (seed, k)


@pytest.mark.parametrize("values", VALUE_SETS)
def test_the_injection_ties_the_restatements_to_the_uint8_ones(values):
    """ranks instead of values: ids, areas and bands of the 16-bit restatement equal the uint8 restatement's on the relabelled
    maps, the records but for the label column, and the sieve result maps back"""
    maps = [random_map(40 + i, values) for i in range(6)] + [wp.blocks(np.random.default_rng(3), 20, 70, 2, values)]
    ranked, table = wp.rank_relabel(maps)
    assert all(r.dtype == np.uint8 for r in ranked) and all(np.array_equal(table[r], m) for r, m in zip(ranked, maps))
    skip16 = values[-1]
    skip8 = int(np.searchsorted(table, skip16))
    for connectivity in (4, 8):
        for s16, s8 in ((None, None), (skip16, skip8)):
            ids, area, rec, _ = wp.components(maps, connectivity, s16)
            ids8, area8, rec8, _ = cc.components(ranked, connectivity, s8)
            assert all(np.array_equal(a, b) for a, b in zip(ids, ids8)) and all(np.array_equal(a, b) for a, b in zip(area, area8))
            assert np.array_equal(np.delete(rec, 2, axis=1), np.delete(rec8, 2, axis=1))
            assert np.array_equal(rec[:, 2], table[rec8[:, 2]].astype(np.int64))
            for m, r in zip(maps, ranked):
                for rounds in (1, 2):
                    assert np.array_equal(wp.merge(m, connectivity, s16, 5, None, rounds), table[cm.merge(r, connectivity, s8, 5, None, rounds)])
    for m, r in zip(maps, ranked):
        for d in (1, 3):
            assert np.array_equal(wp.band(m, d), bd.band(r, d))


def test_values_that_a_byte_reader_would_merge():
    """what the kernel-test values are there for: as bytes {1, 257, 513} are one label, and as int16 65535 is -1"""
    a = np.asarray([[1, 257, 513, 1]], dtype=np.uint16)
    assert len(wp.components([a])[2]) == 4 and len(cc.components([a.astype(np.uint8)])[2]) == 1
    b = np.asarray([[65535, 65535, 32768, 255]], dtype=np.uint16)
    assert wp.components([b])[2][:, 2].tolist() == [65535, 32768, 255]
    assert wp.components([b], skip_label=65535)[2][:, 2].tolist() == [32768, 255]
    assert wp.components([b.view(np.int16)])[2][:, 2].tolist() == [65535, 32768, 255]   # an int16 array is read as unsigned


def test_merge_scenes():
    """equal areas: the smaller 16-bit label wins, which a byte key (255 - low byte) gets wrong for 300 (44) against 513 (1)"""
    for left, right, winner in ((256, 1, 1), (1, 256, 1), (300, 513, 300), (513, 300, 300), (65535, 32768, 32768)):
        scene = wp.speck_between(left, right)
        ids = cc.label(scene, 4)
        counts = np.bincount(ids.reshape(-1))
        assert sorted(counts[counts > 0].tolist()) == [4, 26, 26]
        out = wp.merge(scene, 4, None, 5)
        assert (out[1:3, 6:8] == winner).all() and set(np.unique(out).tolist()) == {left, right}
    out = wp.merge(wp.speck_between(9, 40000, wider_right=3), 4, None, 5)     # the larger region carries the larger label
    assert (out[1:3, 6:8] == 40000).all()
    nested = wp.nested()
    one, two = wp.merge(nested, 8, None, 9, None, 1), wp.merge(nested, 8, None, 9, None, 2)
    assert one[5, 6] == 40000 and (one != 300).sum() == 1 and (two == 300).all()
    walled = wp.walled_in()
    assert wp.merge(walled, 8, 65535, 4)[3, 4] == 700 and wp.merge(walled, 8, 65535, 4, 65535)[3, 4] == 65535
    assert np.array_equal(wp.merge(walled, 8, 65535, 4, 65535) == 65535, walled >= 700)


def test_boundary_areas_identities():
    """radius >= max(h, w): slot 0 is the plain areas; a uniform ground truth leaves slot 1 empty; classes 256 and 1023 count"""
    rng = np.random.default_rng(11)
    gt = wp.blocks(rng, 20, 30, 5, (0, 256, 1023, 1024, 65535))
    pred = wp.blocks(rng, 20, 30, 4, (0, 256, 1023, 2000))
    for C in (257, 1024):
        for rz in (False, True):
            a = wp.areas([pred], [gt], [30], C, 65535, rz)
            assert np.array_equal(a[0], wp.plain_areas(pred, gt, C, 65535, rz))
            assert a[0, 1, 256] > 0 and (C == 257 or a[0, 1, 1023] > 0)
            small = wp.areas([pred], [gt], [2], C, 65535, rz)
            assert (small <= a[0][None]).all() and small[1].sum() > 0
    uniform = np.full((20, 30), 256, dtype=np.uint16)
    assert wp.areas([pred], [uniform], [3], 1024)[1].sum() == 0
    low = [wp.blocks(rng, 17, 40, 3, tuple(range(21))) for _ in range(2)]
    assert np.array_equal(wp.areas([low[0]], [low[1]], [2], 21, 255), bd.areas([low[0].astype(np.uint8)], [low[1].astype(np.uint8)], [2], 21, 255))


def test_header_and_ctypes_prototypes_agree():
    """the wide entries take the uint8 entries' argument lists with uint16_t labels and outputs"""
    for name, swaps in (("segclip_seg_components", 2), ("segclip_seg_sieve", 2), ("segclip_seg_boundary", 2)):
        narrow, wide = " ".join(header_declaration(name)), " ".join(header_declaration(name + "_wide"))
        assert wide.count("uint16_t*") == swaps and narrow.count("uint8_t*") - wide.count("uint8_t*") == swaps
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name + "_wide"][1])
        assert [a is b for a, b in zip(_lib.SIGNATURES[name][1], _lib.SIGNATURES[name + "_wide"][1])].count(False) <= swaps
    assert "segclip_seg_sieve_wide_ws_bytes" in _lib.SIGNATURES
    assert ops.SEG_WIDE_MAX_CLASSES == 1024


def test_host_side_refusals():
    """Despeckle keeps its byte range whatever the maps' width; CPU tensors are refused by name"""
    with pytest.raises(ValueError, match="fill is an integer in 0 .. 255"):
        Despeckle(4, fill=256)
    with pytest.raises(ValueError, match="skip_label is None or an integer in 0 .. 255"):
        Despeckle(4, skip_label=65535)
    m16 = torch.zeros(4, 5, dtype=torch.int16)
    for call in (lambda: components([m16]), lambda: despeckle([m16], 4), lambda: boundary_bands([m16], Boundary()),
                 lambda: boundary_areas([m16], [m16], 300, Boundary(), ignore_index=65535)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="empty list of label maps"):
        components([])
