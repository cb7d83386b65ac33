"""The restatement of the connected components (tests/cc_reference.py) checked on its own, without a GPU: against
scipy.ndimage where it is installed, the properties of the definition that the kernel tests then lean on, the host-side
refusals that need no device, and the parameter list of the entry in the header (tests/test_abi.py holds the binding to it)."""
import numpy as np
import pytest
import torch

from segclip_amd import ops
from tests import cc_reference as cc
from tests.helpers import header_declaration

TH, TW = ops.SEG_CC_TILE
CASES = cc.cases(TH, TW)
RANDOM = ["noise_3_labels", "blocks_21_labels", "bytes_0_7_255", "mixed_batch", "tall_noise", "1x9", "7x1"]


def test_tile_and_cases():
    assert (TH, TW) == (16, 64)
    sizes = {k: [m.shape for m in v] for k, v in CASES.items()}
    assert sizes["long_row"] == [(1, 8 * TW + 3)] and sizes["long_column"] == [(8 * TH + 3, 1)]
    assert sizes["whole_image"] == [(2 * TH + 1, 2 * TW + 2)] and sizes["checkerboard"] == [(TH + 1, TW + 3)]
    assert sizes["serpentine"] == sizes["spiral"] == [(2 * TH + 3, 2 * TW + 3)]
    assert sizes["noise_3_labels"] == [(2 * TH + 6, 2 * TW + 26)]
    assert sizes["mixed_batch"] == [(5, 7), (9, 11), (13, 3), (2 * TH + 6, 2 * TW + 26)]
    assert sorted(np.unique(CASES["bytes_0_7_255"][0]).tolist()) == [0, 7, 255]
    assert len(np.unique(CASES["blocks_21_labels"][0])) == 21


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", RANDOM + ["serpentine", "spiral", "u_shapes", "checkerboard"])
def test_restatement_against_scipy(name, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), dtype=int) if connectivity == 8 else ndi.generate_binary_structure(2, 1)
    maps = CASES[name]
    ids, area, records, _ = cc.components(maps, connectivity)
    rows = []
    for img, L in enumerate(maps):
        h, w = L.shape
        want_ids = np.full((h, w), -1, dtype=np.int64)
        want_area = np.zeros((h, w), dtype=np.int64)
        flat = np.arange(h * w).reshape(h, w)
        for v in np.unique(L).tolist():                      # scipy labels a binary picture: once per label value
            lab, n = ndi.label(L == v, structure=structure)
            for j, sl in enumerate(ndi.find_objects(lab), start=1):
                m = lab == j
                first = int(flat[m].min())                   # canonical: the first pixel in raster order
                want_ids[m], want_area[m] = first, int(m.sum())
                ys, xs = np.nonzero(m)
                rows.append([img, first, v, int(m.sum()), sl[0].start, sl[1].start, sl[0].stop, sl[1].stop, int(ys.sum()), int(xs.sum())])
        assert np.array_equal(ids[img], want_ids) and np.array_equal(area[img], want_area)
    rows.sort(key=lambda r: (r[0], r[1]))
    assert np.array_equal(records, np.asarray(rows, dtype=np.int64).reshape(-1, 10))


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", RANDOM)
def test_properties(name, connectivity):
    for L in CASES[name]:
        ids, area, records, cleaned = cc.components([L], connectivity, skip_label=0, min_area=3, fill=9)
        ids, area, cleaned = ids[0], area[0], cleaned[0]
        h, w = L.shape
        flat = np.arange(h * w).reshape(h, w)
        kept = L != 0
        assert np.all(ids[~kept] == -1) and np.all(area[~kept] == 0) and np.all(ids[kept] >= 0)
        # an id is the index of one of its own pixels, the smallest, and that pixel carries the component's label
        assert np.all(ids[kept] <= flat[kept])
        roots = ids.reshape(-1)[ids[kept]]
        assert np.array_equal(roots, ids[kept])
        assert np.array_equal(L.reshape(-1)[ids[kept]], L[kept])
        # idempotent: the id map, taken as a label map, has the same components and so the same ids
        assert np.array_equal(cc.label(ids, connectivity, skip_label=-1), ids)
        # the areas sum to the unskipped pixel count, in the records and per pixel
        assert int(records[:, 3].sum()) == int(kept.sum())
        assert sum(int(area.reshape(-1)[i]) for i in records[:, 1]) == int(kept.sum())
        assert np.array_equal(records[:, 1], np.unique(ids[kept])) and np.all(records[:, 2] != 0)
        # the despeckling
        small = kept & (area < 3)
        assert np.all(cleaned[small] == 9) and np.array_equal(cleaned[~small], L[~small])
        assert np.array_equal(cc.components([L], connectivity, min_area=0)[3][0], L)


@pytest.mark.parametrize("name", RANDOM + ["checkerboard"])
def test_8_components_are_unions_of_4_components(name):
    for L in CASES[name]:
        i4, i8 = cc.label(L, 4), cc.label(L, 8)
        # every 4-component lies inside one 8-component, whose id is the smallest id of the 4-components it holds
        pairs = np.unique(np.stack([i4.reshape(-1), i8.reshape(-1)], axis=1), axis=0)
        assert len(pairs) == len(np.unique(i4))
        for i in np.unique(i8).tolist():
            assert pairs[pairs[:, 1] == i, 0].min() == i
    L = CASES["checkerboard"][0]
    assert len(np.unique(cc.label(L, 4))) == L.size and len(np.unique(cc.label(L, 8))) == 2


def test_diagonals_and_long_chains():
    for name in cc.diagonals(TH, TW):
        L = CASES[name][0]
        n4, n8 = len(cc.components([L], 4)[2]), len(cc.components([L], 8)[2])
        assert (n4, n8) == (3, 2), name
    for name in ("serpentine", "spiral"):
        L = CASES[name][0]
        for conn in (4, 8):
            records = cc.components([L], conn)[2]
            assert len(records) == 2 and records[:, 3].min() > L.shape[0] * L.shape[1] // 3, name
    L = CASES["u_shapes"][0]
    ids = cc.label(L, 4)
    assert ids[3, 2] == ids[1, 6] == 1 * L.shape[1] + 6            # the arm that starts later takes the other's id
    assert ids[2 * TH + 1, 20] == ids[2 * TH + 1, 10] == (TH - 4) * L.shape[1] + 10


def test_host_side_refusals():
    from segclip_amd.segmentation import Despeckle, SegInference, SegSweepEvaluator
    d = Despeckle(4)
    assert (d.min_area, d.fill, d.connectivity, d.skip_label) == (4, 0, 8, None)
    for bad, match in ((dict(min_area=-1), "min_area"), (dict(min_area=2.0), "min_area"), (dict(min_area=True), "min_area"),
                       (dict(min_area=1, fill=256), "fill"), (dict(min_area=1, fill=-1), "fill"), (dict(min_area=1, fill=1.0), "fill"),
                       (dict(min_area=1, connectivity=6), "connectivity"), (dict(min_area=1, connectivity="8"), "connectivity"),
                       (dict(min_area=1, skip_label=256), "skip_label"), (dict(min_area=1, skip_label=-1), "skip_label"),
                       (dict(min_area=1, skip_label=0.0), "skip_label")):
        with pytest.raises(ValueError, match=match):
            Despeckle(**bad)
    with pytest.raises(ValueError, match="SegSweepEvaluator.*clean.*SegEvaluator"):
        SegSweepEvaluator.update_raw(object.__new__(SegSweepEvaluator), [], [], None, clean=d)
    with pytest.raises(ValueError, match="render_raw.*clean.*despeckle"):
        SegInference.render_raw(object.__new__(SegInference), [], None, ["pred"], None, clean=d)
    with pytest.raises(ValueError, match="predict_list.*clean.*despeckle"):
        SegInference.predict_list(object.__new__(SegInference), [], clean=d)
    with pytest.raises(ValueError, match="sizes 1 .."):
        ops.seg_components_table([(0, 5)], [0], "cpu")
    table, n_blocks, side = ops.seg_components_table([(TH, TW), (TH + 1, TW + 1), (1, 1)], [0, 2000, 9000], "cpu")
    assert table.tolist() == [[TH, TW, 0, 0, 0, 0, 0, 0], [TH + 1, TW + 1, 2000, 1, 0, 0, 0, 0], [1, 1, 9000, 5, 0, 0, 0, 0]]
    assert (n_blocks, side) == (6, TW + 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_components(table, n_blocks, torch.zeros(9001, dtype=torch.uint8))


def test_header_and_ctypes_prototypes_agree():
    args = header_declaration("segclip_seg_components")
    assert [a.rsplit(" ", 1)[1].lstrip("*") for a in args] == [
        "images", "B", "n_blocks", "max_side", "labels", "labels_bytes", "connectivity", "skip_label", "ids", "area_px", "px_count",
        "records", "K", "count", "min_area", "fill", "cleaned", "cleaned_bytes", "ws", "ws_bytes", "stream"]
