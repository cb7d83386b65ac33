"""The numpy restatement of the superpixels and of the majority vote (tests/superpixel_reference.py) checked on its own, without
a GPU: the snapping-scene numbers the definition was settled on, the empty-cluster rule, the tie rules, the host-side argument
checks and refusals that need no device, and the declarations and constants of the header."""
import numpy as np
import pytest
import torch

from segclip_amd import _lib, ops
from segclip_amd.segmentation import (Segments, SegEvaluator, SegInference, SegSweepEvaluator, Snap, Superpixels, snap_labels,
                                      superpixels)
from tests import pamr_reference as pr
from tests import superpixel_reference as sr
from tests.helpers import header_declaration


def _scene():
    raw, labels, gt = pr.snapping_scene()
    return raw.numpy(), labels.numpy(), gt


def _miou(labels, gt):
    return pr.miou(torch.from_numpy(np.ascontiguousarray(labels)), gt, 3)


def test_snapping_scene_before_any_stage():
    raw, labels, gt = _scene()
    assert raw.shape == (96, 128, 3)
    assert round(_miou(labels, gt), 4) == 0.8664


@pytest.mark.parametrize("step,iters,miou,wrong", [(16, 0, 0.9858, 77), (16, 2, 1.0, 0), (16, 5, 1.0, 0), (16, 10, 1.0, 0),
                                                   (8, 5, 0.9182, 534)])
def test_snapping_scene_numbers(step, iters, miou, wrong):
    raw, labels, gt = _scene()
    ids, cen = sr.slic(raw, step, 10, iters)
    K = cen.shape[0]
    assert K == -(-96 // step) * -(-128 // step) and ids.dtype == np.int32 and 0 <= ids.min() and ids.max() < K
    out = sr.vote(labels, ids, K, 3, 0)
    got, bad = _miou(out, gt), int((out != gt.numpy()).sum())
    print(f"step {step} compactness 10 iters {iters}: mIoU {got:.4f}, {bad} wrong pixels")
    assert round(got, 4) == miou and bad == wrong


def test_empty_clusters_keep_their_values():
    raw = sr.block_picture()
    assert raw.shape == (48, 60, 3) and raw.dtype == np.uint8
    ids, cen, n = sr.slic(raw, 7, 1, 6, with_counts=True)
    empty = np.nonzero(n == 0)[0]
    print(f"block picture at S = 7, m = 1, T = 6: {len(empty)} of {len(n)} centres without a pixel")
    assert len(n) == 63 and len(empty) >= 1
    # a centre that is empty after the last round has the values of the round before: one more update changes nothing of it
    again, _ = sr.update(raw, ids, cen.astype(np.int64))
    assert np.array_equal(again[empty], cen[empty])
    assert set(np.unique(ids).tolist()) == set(np.nonzero(n)[0].tolist())


def test_initial_centres_and_the_index_tie_rule():
    raw = np.full((40, 40, 3), 93, dtype=np.uint8)
    cen = sr.init_centres(raw, 16)
    assert cen[:, 0].reshape(3, 3)[:, 0].tolist() == [8, 24, 39] and cen[:, 1].reshape(3, 3)[0].tolist() == [8, 24, 39]
    ids, _ = sr.slic(raw, 16, 10, 0)
    # one byte value: only the distance in the plane counts; (16, x) is as far from row 8 as from row 24 and goes to the lower index
    assert ids[16, 0] == 0 and ids[17, 0] == 3 and ids[0, 16] == 0 and ids[0, 17] == 1
    small, c1 = sr.slic(np.zeros((3, 5, 3), dtype=np.uint8), 16, 10, 3)
    assert c1.shape == (1, 5) and not small.any() and c1[0].tolist() == [1, 2, 0, 0, 0]


def test_vote_rules():
    lab = np.array([[0, 0, 1, 1], [2, 2, 2, 255], [1, 0, 1, 0], [5, 5, 5, 5]], dtype=np.uint8)
    seg = np.array([[0, 0, 0, 0], [1, 1, 1, 1], [2, 2, 2, 2], [-1, 4, 3, 3]], dtype=np.int32)
    out = sr.vote(lab, seg, 4, 4, 0)
    assert out[0].tolist() == [0, 0, 0, 0]                  # 2 : 2 goes to the smallest class
    assert out[1].tolist() == [2, 2, 2, 255]                # a label >= C does not vote and is kept
    assert out[2].tolist() == [0, 0, 0, 0]
    assert out[3].tolist() == [5, 5, 5, 5]                  # ids -1 and K, and labels >= C in segment 3: nobody votes
    assert sr.vote(lab, seg, 4, 4, 50)[0].tolist() == [0, 0, 0, 0]   # exactly 50 %: >= snaps
    assert sr.vote(lab, seg, 4, 4, 51)[0].tolist() == [0, 0, 1, 1]   # 51 %: does not
    assert sr.vote(lab, seg, 4, 4, 100)[1].tolist() == [2, 2, 2, 255]
    wide = np.array([[1, 257, 257, 65535]], dtype=np.uint16)
    assert sr.vote(wide, np.zeros((1, 4), dtype=np.int32), 1, 300, 0).tolist() == [[257, 257, 257, 65535]]


def test_arguments():
    sp = Superpixels()
    assert (sp.step, sp.compactness, sp.iters) == (16, 10, 5)
    assert sp.grid(96, 128) == (6, 8) and sp.count(96, 128) == 48 and Superpixels(7).grid(48, 60) == (7, 9)
    assert Superpixels(4, 1, 0).count(3, 5) == 2 and Superpixels(7).count(3, 5) == 1 and Superpixels(64, 64, 16).count(65, 64) == 2
    for bad, match in ((dict(step=3), "step"), (dict(step=65), "step"), (dict(step=8.0), "step"), (dict(step=True), "step"),
                       (dict(compactness=0), "compactness"), (dict(compactness=65), "compactness"), (dict(compactness=1.5), "compactness"),
                       (dict(iters=-1), "iters"), (dict(iters=17), "iters"), (dict(iters=None), "iters")):
        with pytest.raises(ValueError, match=match):
            Superpixels(**bad)
    s = Snap()
    assert isinstance(s.superpixels, Superpixels) and s.min_share == 0 and Snap(sp, 60).superpixels is sp
    for bad in (-1, 101, 50.0, True):
        with pytest.raises(ValueError, match="min_share"):
            Snap(min_share=bad)
    with pytest.raises(TypeError, match="Superpixels"):
        Snap(superpixels=16)
    with pytest.raises(TypeError, match="Superpixels"):
        superpixels([torch.zeros(4, 4, 3, dtype=torch.uint8)], sp=16)


def test_cpu_tensors_have_no_fallback():
    raw = torch.zeros(8, 8, 3, dtype=torch.uint8)
    lab, ids = torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        superpixels([raw])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        snap_labels([lab], [ids], 3, counts=[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        snap_labels([lab], Segments([ids], [1]), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_superpixels_table([raw], 16)
    table, n_blocks, total, top = ops.seg_vote_table([(8, 8)], [0], [1], "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_vote(table, n_blocks, lab.view(-1), ids.view(-1), total, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_superpixels(torch.zeros(1, 8, dtype=torch.int64), 1, ids.view(-1), 1)


def test_tables_and_refusals_without_a_device():
    TH, TW = ops.SEG_SP_TILE
    T = ops.SEG_VOTE_TILE
    table, n_blocks, total, top = ops.seg_vote_table([(TH, TW), (3, 5), (1, T + 1)], [0, 4000, 5000], [7, 1, 5000], "cpu")
    assert table.tolist() == [[0, TH * TW, 0, 7, 0, 0, 0, 0], [4000, 15, 7, 1, 1, 0, 0, 0], [5000, T + 1, 8, 5000, 2, 0, 0, 0]]
    assert (n_blocks, total, top) == (4, 5008, 5000)
    for sizes, offs, counts, match in (([(0, 5)], [0], [1], "sizes 1 .."), ([(4, 4)], [0], [0], "segments per image"),
                                       ([(4, 4)], [0], [ops.SEG_VOTE_MAX_SEGMENTS + 1], "segments per image"),
                                       ([(4, 4)], [0, 1], [1], "offsets"), ([], [], [], "0 sizes")):
        with pytest.raises(ValueError, match=match):
            ops.seg_vote_table(sizes, offs, counts, "cpu")
    with pytest.raises(ValueError, match="step"):
        ops.seg_superpixels_table([torch.zeros(4, 4, 3, dtype=torch.uint8)], 3)

    # the checks of snap_labels that come before anything touches the device
    class OnDevice(torch.Tensor):   # a CPU tensor that says it lives on the device: the checks under test read no data
        is_cuda = True
    lab = torch.zeros(6, 7, dtype=torch.uint8).as_subclass(OnDevice)
    ids = torch.zeros(6, 7, dtype=torch.int32).as_subclass(OnDevice)
    with pytest.raises(ValueError, match="needs counts"):
        snap_labels([lab], [ids], 3)
    with pytest.raises(ValueError, match="carries its counts"):
        snap_labels([lab], Segments([ids], [1]), 3, counts=[1])
    with pytest.raises(ValueError, match="1 label maps but 2 segment maps"):
        snap_labels([lab], [ids, ids], 3, counts=[1, 1])
    with pytest.raises(ValueError, match="segment map is an .h, w. int32"):
        snap_labels([lab], [ids.long()], 3, counts=[1])
    with pytest.raises(ValueError, match="segment map is an .h, w. int32"):
        snap_labels([lab], [ids[:5]], 3, counts=[1])
    with pytest.raises(ValueError, match="segment count"):
        snap_labels([lab], [ids], 3, counts=[0])
    with pytest.raises(ValueError, match="min_share"):
        snap_labels([lab], [ids], 3, counts=[1], min_share=101)
    with pytest.raises(ValueError, match="num_classes .uint8 labels."):
        snap_labels([lab], [ids], 257, counts=[1])
    with pytest.raises(ValueError, match="num_classes .int16 labels."):
        snap_labels([lab.to(torch.int16).as_subclass(OnDevice)], [ids], 1025, counts=[1])
    with pytest.raises(ValueError, match="uint8 or int16"):
        snap_labels([lab.float().as_subclass(OnDevice)], [ids], 3, counts=[1])


def test_entry_points_that_refuse_snap():
    s = Snap()
    with pytest.raises(ValueError, match="predict_list.*snap.*predict_raw"):
        SegInference.predict_list(object.__new__(SegInference), [], snap=s)
    with pytest.raises(ValueError, match="render_raw.*snap.*predict_raw"):
        SegInference.render_raw(object.__new__(SegInference), [], None, ["pred"], None, snap=s)
    with pytest.raises(ValueError, match="SegEvaluator.update.*snap.*update_raw"):
        SegEvaluator.update(object.__new__(SegEvaluator), [], [], snap=s)
    with pytest.raises(ValueError, match="SegSweepEvaluator.*snap.*SegEvaluator"):
        SegSweepEvaluator.update_raw(object.__new__(SegSweepEvaluator), [], [], None, snap=s)
    wide = object.__new__(SegInference)
    wide.wide = True
    with pytest.raises(ValueError, match="predict_raw.*snap.*16-bit"):
        wide.predict_raw([], None, snap=s)
    ev = object.__new__(SegEvaluator)
    ev.seg = wide
    with pytest.raises(ValueError, match="update_raw.*snap.*16-bit"):
        ev.update_raw([], [], None, snap=s)
    narrow = object.__new__(SegInference)
    with pytest.raises(TypeError, match="snap is a Snap"):
        narrow.predict_raw([torch.zeros(4, 4, 3, dtype=torch.uint8)], None, snap=Superpixels())
    with pytest.raises(ValueError, match="snap: out_shapes"):
        narrow.predict_raw([torch.zeros(4, 4, 3, dtype=torch.uint8)], None, out_shapes=[(5, 4)], snap=s)
    from segclip_amd.train import eval_epoch
    with pytest.raises(ValueError, match="snap.*transform"):
        eval_epoch(None, None, "cpu", 1, [], None, True, dict(snap=s))


def test_header_declarations_and_constants():
    names = lambda entry: [a.rsplit(" ", 1)[1].lstrip("*") for a in header_declaration(entry)]   # noqa: E731
    assert names("segclip_seg_superpixels_ws_bytes") == ["K_total"]
    assert names("segclip_seg_superpixels") == ["images", "B", "n_blocks", "max_side", "step", "compactness", "iters", "ids", "ids_n",
                                                "K_total", "centres", "ws", "ws_bytes", "stream"]
    assert names("segclip_seg_vote_ws_bytes") == ["K_total", "C"]
    vote = ["images", "B", "n_blocks", "max_k", "labels", "labels_bytes", "segments", "segments_n", "K_total", "C", "min_share", "out",
            "out_bytes", "ws", "ws_bytes", "stream"]
    assert names("segclip_seg_vote") == vote
    assert names("segclip_seg_vote_wide") == [{"labels_bytes": "labels_n", "out_bytes": "out_n"}.get(a, a) for a in vote]
    assert header_declaration("segclip_seg_vote_wide")[4] == "const uint16_t* labels"
    for entry in ("segclip_seg_superpixels", "segclip_seg_superpixels_ws_bytes", "segclip_seg_vote", "segclip_seg_vote_wide",
                  "segclip_seg_vote_ws_bytes"):
        assert entry in _lib.SIGNATURES
    assert ops.SEG_SP_TILE == (32, 64) and ops.SEG_SP_COLS == 8 and ops.SEG_VOTE_COLS == 8 and ops.SEG_VOTE_TILE == 2048
    assert (ops.SEG_SP_MIN_STEP, ops.SEG_SP_MAX_STEP, ops.SEG_SP_MAX_COMPACTNESS, ops.SEG_SP_MAX_ITERS) == (4, 64, 64, 16)
    assert ops.SEG_VOTE_MAX_SEGMENTS == 1 << 20
    # the two bounds the header states beside the limits
    S, m = ops.SEG_SP_MAX_STEP, ops.SEG_SP_MAX_COMPACTNESS
    assert S * S * 3 * 255 * 255 + m * m * 18 * S * S < 2 ** 31
    assert 9 * S * S * (ops.SEG_SOURCE_LIMIT - 1) < 2 ** 32
    # at the smallest step a tile stages the most centres: they fit one lane each and the static LDS
    th, tw = ops.SEG_SP_TILE
    assert (th // 4) * (tw // 4) <= 256 and (th // 4 + 2) * (tw // 4 + 2) * 11 * 4 <= 64 * 1024
