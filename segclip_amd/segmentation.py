"""Zero-shot segmentation inference: an image batch and class prompts in, a label map out.

Replaces seg_segmentation/evaluation of the reference without mmseg / mmcv: build_text_embedding is the text step of
build_seg_inference (evaluation/builder.py:55-66), SegInference is ViTSegInference (evaluation/vit_seg.py:118-256) plus
mmseg's whole / slide inference.  The post-processing runs in three HIP kernels (csrc/segment.hip): the label map is written
as one byte per pixel without the reference's (H, W, G) / (H, W, N) intermediates, and the vision tower sees every window
once, all windows of all images of a call in one batch.

The evaluation (main_seg_zeroshot.py:122-167 and mmseg's single_gpu_test / eval_metrics): SegInference.predict_list takes
images of mixed sizes and writes their label maps at the ground truth's size in one launch (csrc/segment_eval.inc), and
SegEvaluator accumulates mmseg's per-class areas in the same launch and turns them into mIoU / aAcc / mAcc.

The front end (the test pipeline of configs/_base_/datasets/pascal_voc12.py:19-34, mmcv's Resize(keep_ratio=True) and
Normalize there): ImageTransform states it, and predict_raw / update_raw / preprocess take decoded (h, w, 3) uint8 images.
One HIP kernel (csrc/segment_frontend.inc) writes the tower's input windows from the raw bytes, resized bilinearly and
normalised on the way, so the resized image does not exist: decoded image in, mIoU out.  The dataset, the image decoding and
the tokenizer stay with the caller.

The demo (main_seg_vis.py; ViTSegInference.show_result / blend_result / seg2coord, vit_seg.py:100-115, 258-377): blend draws
an index map over decoded images in numpy's fp64 arithmetic and sums the label anchors in the same launch, groups_list /
groups_raw write the group map at each picture's size, and render_raw serves the reference's --vis modes from one pass of the
vision tower (csrc/segment_render.inc).  Encoding the pictures, the palette-mode PNG of vis_mode="pred" and the label text
stay with the caller.

Test-time augmentation (mmseg's MultiScaleFlipAug + aug_test, the wrapper of every test configuration of the reference):
TestAug lists an image's views, predict_raw / update_raw / eval_epoch take aug=, predict_views / update_views take tensors
that are already pre-processed and flipped, and predict_proba_* return the mean probabilities.  Every (image, view) pair is
an entry of the plan, so the windows of all views share the tower calls, and one kernel (csrc/segment_aug.inc) rescales
every view's logits, takes their soft-max, mirrors, averages and takes the first maximum per output pixel.

The threshold sweep (bg_thresh is the one hyperparameter of the evaluation that is tuned per dataset and checkpoint: the
reference's configurations use 0.80, 0.25 and 0.65): SegSweepEvaluator scores up to 16 ascending thresholds in one pass - the
towers, the front end and the group tables run once, and one kernel (csrc/segment_sweep.inc) writes every threshold's label
map and areas, bit for bit those of one SegEvaluator per threshold.  Not swept: the augmented path, the dense logits, the
top-5 mask.

Refinement (not in the reference; the zero-shot systems after SegCLIP report their numbers with it): PAMR states the
pixel-adaptive mask refinement of Araslanov & Roth (CVPR 2020), refine_labels applies it to label maps against the decoded
pictures, and predict_raw / update_raw / eval_epoch take refine=.  The label map is the arg-max of a 14 x 14 assignment blown
up twice, so its borders follow the patch grid; the refinement moves them onto the picture's edges.  It runs on the device
(csrc/segment_refine.inc) without a (C, h, w) tensor and without a host synchronisation, and with a ground truth its last
kernel adds the mIoU areas.  Not covered: the threshold sweep, render_raw, and the entry points without a raw picture.

Objects (not in the reference): components labels the connected components of label maps on the device
(csrc/segment_objects.inc) - ids whose value is the component's first pixel in raster order, so they depend on no scheduling -
and returns them with a compact list of boxes, areas and coordinate sums; despeckle / Despeckle replace components below a
minimum area by a fill label, or with merge=True (csrc/segment_sieve.inc) by the label of their largest neighbour, in up to 8
rounds - the mode for Context-59, COCO-Stuff, ADE and every with_bg=False configuration, where no class is the background and
fill=0 would paint the specks with the first real class.  predict_raw / update_raw / eval_epoch take clean=, applied after
refine=.  Not covered: the threshold sweep, render_raw, predict_list and update (apply despeckle to their maps); merging by
the length of the shared border or by the picture's colours; more than 8 rounds in one call (call again).

Boundary metrics (not in the reference): mIoU counts every pixel alike and hardly sees the borders that refine= and clean=
exist to improve.  Boundary states the band radius of Boundary IoU (Cheng et al., CVPR 2021), boundary_bands returns the
band bytes of label maps, boundary_areas the (2, 3, C) areas of Boundary IoU and of the trimap mIoU of the DeepLab papers,
and SegEvaluator(boundary=) scores the labels of every update path against the ground truths with one more call
(csrc/segment_boundary.inc), without a host synchronisation; compute() adds bIoU, mbIoU, trimap_IoU, trimap_mIoU and
trimap_aAcc.  Not covered: SegSweepEvaluator and render_raw.

Wide vocabularies (the reference evaluates VOC, Context-59 and COCO-80; open-vocabulary work also reports Pascal-Context-459
and ADE20K-847): SegInference(label_dtype=torch.int16) writes 16-bit label maps for up to 1024 classes and SegEvaluator over it
scores int16 ground truths (csrc/segment_wide.inc: 3 x 1024 counters per workgroup, and the pixels that need a scan over the
classes are resolved by their wave, 64 classes at a time).  The uint8 path is unchanged and stays the default.  Not covered for
16-bit maps: test-time augmentation, the threshold sweep, refinement (PAMR's launch plan and presence map stop at 256 classes)
and render_raw, and inside the pipeline (clean=, SegEvaluator(boundary=)) despeckling and the boundary metrics.  The stand-alone
functions do take int16 maps - components, despeckle, boundary_bands, boundary_areas (their kernels are templates on the label
element) - and SegEvaluator.update_maps scores label maps that exist already: predict_raw -> despeckle -> update_maps.

Confusion matrix (not in the reference): the (3, C) areas say how bad a class is, not where its pixels went.
SegEvaluator(confusion=True) counts the labels of every update path, 8- or 16-bit, against the ground truths into a
(C + 1, C + 1) int64 device matrix with one more call (csrc/segment_confusion.inc: wide loads, run-length counting, the matrix
or a table of pairs per workgroup in LDS), without a host synchronisation; compute() adds Dice, Precision, Recall, Fscore,
fwIoU and kappa, and areas_from_confusion, confusion_metrics, confused_pairs and merge_classes work on a host copy without an
evaluator.  Not covered: SegSweepEvaluator.

Per-image areas (mmseg's pre_eval hands them back; the summed (3, C) table cannot): image_areas counts a list of label maps
against their ground truths into a (B, 3, C) int64 device tensor, one (3, C) row per picture, in one launch
(csrc/segment_image_areas.inc: one tile of one picture per workgroup, 16-byte loads at any element offset, run-length counting,
the counters in LDS), and SegEvaluator(per_image=True) does so on every update path, 8- or 16-bit, with one more call on the
maps that leave the chain and without a host synchronisation; `image_areas` is the (n, 3, C) concatenation in the order the
pictures were given.  Three reductions of the rows, static and without an evaluator: fine_grained_from_image_areas (the mean of
per-image mIoU, the per-class mean over the pictures that contain the class, and the means of their lowest q %),
worst_images (the k lowest pictures) and bootstrap_miou (a confidence interval of the data-set mIoU from resampled pictures);
compute() adds the first.  Several ranks gather the rows (all_gather), they are not summed.  Not covered: SegSweepEvaluator,
per-image boundary areas and per-image confusion.

Superpixels and snapping (not in the reference): the third standard answer to borders that follow the patch grid.  Superpixels
states an integer SLIC on the RGB bytes, superpixels cuts a list of decoded pictures into segments on the device
(csrc/segment_superpixel.inc), snap_labels gives every segment the majority label of its pixels (csrc/segment_vote.inc) - the
segments are a Segments, or int32 maps of the caller's own with their counts (Felzenszwalb maps, flattened instance masks), the
labels uint8 or int16 - and Snap is the stage: predict_raw / update_raw / eval_epoch take snap=, applied after refine= and
before clean=.  Everything is integer arithmetic, without soft masks and without a host synchronisation.  No connectivity
pass belongs to the definition (components gives the connected parts of an id map).  Not covered: predict_list, update,
render_raw, SegSweepEvaluator and, inside the pipeline, 16-bit label maps: predict_raw -> snap_labels -> despeckle -> update_maps.

The host layer.  _plan_windows turns the sizes of a call into tower batches and per-entry windows (a pure function: no model,
no device), a source (_BatchImages, _SlicedImages, _RawImages) says where a chunk's tower input comes from, and
SegInference._list_towers is the one loop that runs the towers, for every entry point.  A source is always view-shaped: an
image without augmentation is one view with flags 0.  _list_forward (arg-max of the logits, group maps), _sweep_forward
(the same for a list of thresholds) and _views_forward (soft-max mean, dense twin) are the kernel calls over the same steps.
Behind the label kernel, _Maps owns the layout of a list of maps in one flat buffer (views used where they lie, copies at
multiples of 4, zeroed bytes between the maps of an output, the gapless form that the ground truths have), and
SegInference._post_process is the one chain labels -> refine -> snap -> clean -> areas -> boundary areas for predict_raw and every
update path; its docstring states which kernel counts the mIoU areas.  _refuse words the refusals of the entry points that
do not take a stage, and _check_pictures / _check_maps (here) and ops._seg_pictures (strides, where the addresses are taken)
are the only checks of decoded pictures and index maps.

Deviations from the reference.  mmseg takes a softmax between the resize and the arg-max; without augmentation the arg-max
is taken of the logits here, which can differ only where fp32 exp rounds two different logits to one value (the augmented
path takes the soft-max mmseg takes: the mean over views needs it).  A ground-truth value of 255 stays
ignored whatever reduce_zero_label says.  The resized pixel is kept in fp32 and not rounded back to uint8 as cv2's 8-bit
fixed-point resize does: about one grey level, 0.015 in normalised units (unmeasured: cv2 is not a dependency).  The overlay
is drawn on the decoded image itself, where the reference draws on a de-normalised copy of the network input resized back
to the picture's size.  Text is not drawn: input_pred_label returns the anchor positions beside the overlay.
"""
import collections
import colorsys
import itertools
import math

import torch

from . import config, ops


def slide_windows(H, W, crop, stride):
    """mmseg's sliding-window grid: [(y0, x0)] row by row, the last window of a row / column shifted back inside."""
    (ch, cw), (sh, sw) = crop, stride
    if H < ch or W < cw:
        raise ValueError(f"slide mode: image {H}x{W} is smaller than the crop {ch}x{cw}")
    hg = max(H - ch + sh - 1, 0) // sh + 1
    wg = max(W - cw + sw - 1, 0) // sw + 1
    out = []
    for i in range(hg):
        for j in range(wg):
            y1, x1 = min(i * sh + ch, H), min(j * sw + cw, W)
            out.append((max(y1 - ch, 0), max(x1 - cw, 0)))
    return out


def test_size(h, w, img_scale=(2048, 224)):
    """mmcv's keep-ratio rescale of an (h, w) image to the test pipeline's img_scale -> (H, W): the largest scale that keeps
    the long side within max(img_scale) and the short side within min(img_scale), sizes rounded half up."""
    s = min(max(img_scale) / max(h, w), min(img_scale) / min(h, w))
    return int(h * s + 0.5), int(w * s + 0.5)


test_size.__test__ = False   # a product function, not a test


class ImageTransform:
    """The test pipeline's Resize(keep_ratio=True) at img_scale + Normalize(mean, std) (pascal_voc12.py:19-34).  mean and std
    are per channel in RGB order, in grey levels (the defaults are the VOC config's); channel_order is the order of the
    decoded source's channels: "bgr" sources (cv2.imread) are reversed on the way, as to_rgb=True does."""

    def __init__(self, img_scale=(2048, 224), mean=(122.7709383, 116.7460125, 104.09373615),
                 std=(68.5005327, 66.6321579, 70.32316305), channel_order="rgb"):
        if channel_order not in ("rgb", "bgr"):
            raise ValueError(f"channel_order must be 'rgb' or 'bgr', got {channel_order!r}")
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("mean and std have one entry per channel")
        self.img_scale, self.channel_order = tuple(img_scale), channel_order
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(v) for v in std)
        # 1 / std in fp64, rounded to fp32 once: the kernel multiplies by exactly this number
        self.inv_std = tuple(torch.tensor([1.0 / v for v in self.std], dtype=torch.float64).float().tolist())

    def net_size(self, h, w):
        """The (H, W) an (h, w) image is resized to."""
        return test_size(h, w, self.img_scale)


_Plan = collections.namedtuple("_Plan", "batches entries image_windows")


def _entry_name(view_counts, e):
    """Entry e of a plan, for a message: the views of an image are consecutive entries."""
    for i, n in enumerate(view_counts):
        if e < n:
            return f"image {i} view {e}"
        e -= n


def _plan_windows(mode, crop_size, stride, sizes, view_counts=None):
    """The windows of a call, from sizes alone.  sizes[e] = (H, W) of entry e; image i owns view_counts[i] consecutive
    entries, its views (one each unless given).  -> _Plan(batches [(win size, [(entry, y0, x0)])] in tower order, entries
    [(first window, window count, win size)], image_windows [windows of an image over its views]).  Slide mode: one batch of
    all windows; whole mode: one batch per distinct size, sizes and their entries in first-seen order.  What exceeds the
    limits of the kernels' device-side lists would be silently ignored there, so it raises here, image and view named."""
    counts = [1] * len(sizes) if view_counts is None else list(view_counts)
    if sum(counts) != len(sizes):
        raise ValueError(f"{len(sizes)} entries but the view counts sum to {sum(counts)}")
    entries = [None] * len(sizes)
    if mode == "slide":
        crop, wins = tuple(crop_size), []
        for e, (H, W) in enumerate(sizes):
            try:
                per = slide_windows(H, W, crop, stride)
            except ValueError as err:
                raise ValueError(f"{_entry_name(counts, e)}: {err}") from None
            if len(per) > ops.SEG_MAX_IMAGE_WINDOWS:
                raise ValueError(f"{_entry_name(counts, e)}: slide mode: {len(per)} windows, at most "
                                 f"{ops.SEG_MAX_IMAGE_WINDOWS} supported")
            entries[e] = (len(wins), len(per), crop)
            wins += [(e, y, x) for (y, x) in per]
        batches = [(crop, wins)]
    else:
        by_size = {}
        for e, hw in enumerate(sizes):
            by_size.setdefault(tuple(hw), []).append(e)
        batches, n = [], 0
        for hw, members in by_size.items():
            for k, e in enumerate(members):
                entries[e] = (n + k, 1, hw)
            batches.append((hw, [(e, 0, 0) for e in members]))
            n += len(members)
    image_windows, e0 = [], 0
    for i, V in enumerate(counts):
        if V > ops.SEG_MAX_VIEWS:
            raise ValueError(f"image {i}: {V} views, at most {ops.SEG_MAX_VIEWS} supported")
        image_windows.append(sum(count for _, count, _ in entries[e0:e0 + V]))
        if image_windows[i] > ops.SEG_MAX_IMAGE_WINDOWS:
            raise ValueError(f"image {i}: {image_windows[i]} windows over its {V} views, at most {ops.SEG_MAX_IMAGE_WINDOWS} "
                             "supported")
        e0 += V
    return _Plan(batches, entries, image_windows)


def _check_tower_windows(plan, name, patch, base):
    """What the vision tower requires of a plan's window sizes, before anything runs.  name(e): entry e for the message;
    base: the tokens of the training resolution."""
    for (wh, ww), wins in plan.batches:
        if wh % patch or ww % patch:
            raise ValueError(f"{name(wins[0][0])}: window {wh}x{ww} is not a multiple of the patch size {patch}")
        if (wh // patch) * (ww // patch) not in (base, 4 * base):
            raise ValueError(f"{name(wins[0][0])}: window {wh}x{ww}: the vision tower takes its segmentation branch only at 1x "
                             f"or 4x the training token count ({base}; modules/module_seg_vit.py:423)")


class _Source:
    """The tower input of a call, always view-shaped: image i has view_counts[i] consecutive entries, its views; sizes[e] is
    the network size of entry e and flags[e] its flip word.  default_out: the output sizes when the caller names
    none; augmented: the call takes mmseg's aug_test (_views_forward) - an image without augmentation is one view, flags 0.
    windows(chunk, dwin, wh, ww): the (n, 3, wh, ww) tower input of a chunk of the plan's windows, dwin its device rows."""

    augmented = False

    def name(self, e):
        return _entry_name(self.view_counts, e)


class _BatchImages(_Source):
    """A (B, 3, H, W) batch (predict, group_map, encode_decode).  Whole mode: a chunk is a run of images, so its input is a
    view of the batch; slide mode: one slice per window."""

    def __init__(self, img, whole):
        ops.L.require_cuda(img)
        B, _, H, W = img.shape
        if B == 0:
            raise ValueError("empty image batch")
        self.img, self.whole, self.device = img, whole, img.device
        self.sizes, self.flags, self.view_counts = [(int(H), int(W))] * B, [0] * B, [1] * B

    def windows(self, chunk, dwin, wh, ww):
        if self.whole:
            return self.img[chunk[0][0]:chunk[-1][0] + 1]
        return torch.stack([self.img[b, :, y:y + wh, x0:x0 + ww] for (b, y, x0) in chunk])


class _SlicedImages(_Source):
    """views[i] = [((3, H, W) tensor, flags)]: images already resized and normalised (predict_list: one view each, flags 0) or
    views that are also flipped already (what mmseg hands to aug_test).  One slice per window."""

    def __init__(self, views, augmented=False):
        if len(views) == 0:
            raise ValueError("empty image list")
        self.imgs, self.flags = [], []
        for i, per in enumerate(views):
            if len(per) == 0:
                raise ValueError(f"image {i}: no views")
            for v, (t, flags) in enumerate(per):
                ops.L.require_cuda(t)
                if t.dim() != 3 or t.shape[0] != 3:
                    raise ValueError(f"image {i} view {v}: a view is a (3, H, W) tensor, got {tuple(t.shape)}")
                if int(flags) not in (0, 1, 2, 3):
                    raise ValueError(f"image {i} view {v}: flags {flags}, bit 0 = horizontal flip and bit 1 = vertical flip")
                self.imgs.append(t)
                self.flags.append(int(flags))
        self.view_counts = [len(per) for per in views]
        self.augmented, self.device = augmented, self.imgs[0].device
        self.sizes = [(int(t.shape[1]), int(t.shape[2])) for t in self.imgs]
        self.default_out = None if augmented else self.sizes

    def windows(self, chunk, dwin, wh, ww):
        return torch.stack([self.imgs[e][:, y:y + wh, x0:x0 + ww] for (e, y, x0) in chunk])


class _RawImages(_Source):
    """Decoded (h, w, 3) uint8 images, one unflipped view each or with aug (a TestAug) its views: the front-end kernel resizes,
    normalises and mirrors a chunk's windows; neither a resized nor a flipped image exists.  net_sizes overrides the network
    sizes: one (H, W) per image, with aug one per view of every image in the order of aug.views."""

    def __init__(self, raws, transform, net_sizes=None, aug=None):
        self.pictures, self.default_out = list(raws), _check_pictures(raws)   # the output sizes: mmseg's ori_shape
        if not isinstance(transform, ImageTransform):
            raise TypeError("transform is an ImageTransform")
        if aug is not None and not isinstance(aug, TestAug):
            raise TypeError("aug is a TestAug")
        if aug is None:
            if net_sizes is not None and len(net_sizes) != len(raws):
                raise ValueError(f"{len(raws)} images but {len(net_sizes)} network sizes")
            lists = [[tuple(transform.net_size(h, w) if net_sizes is None else net_sizes[i]) + (0,)]
                     for i, (h, w) in enumerate(self.default_out)]
        else:
            lists = [aug.views(h, w, transform) for (h, w) in self.default_out]
            if net_sizes is not None:
                if len(net_sizes) != len(raws) or any(len(a) != len(b) for a, b in zip(net_sizes, lists)):
                    raise ValueError("with aug, net_sizes holds one (H, W) per view of every image")
                lists = [[(H, W, f) for (H, W), (_, _, f) in zip(a, b)] for a, b in zip(net_sizes, lists)]
        self.view_counts = [len(per) for per in lists]
        self.sizes = [(int(H), int(W)) for per in lists for (H, W, _) in per]
        self.flags = [f for per in lists for (_, _, f) in per]
        self.raws = [t for t, per in zip(raws, lists) for _ in per]
        self.transform, self.augmented, self.device = transform, aug is not None, raws[0].device
        # no flipped view: the plain kernel and its table (the view kernel at flags 0 writes the same bits)
        self.flipped = any(self.flags)
        self.table = ops.seg_view_source_table(self.raws, self.sizes, self.flags) if self.flipped else \
            ops.seg_source_table(self.raws, self.sizes)

    def windows(self, chunk, dwin, wh, ww):
        t = self.transform
        kw = dict(reverse_channels=t.channel_order == "bgr", table=self.table)
        if self.flipped:
            return ops.seg_view_windows_from_u8(self.raws, self.sizes, self.flags, dwin, (wh, ww), t.mean, t.inv_std, **kw)
        return ops.seg_windows_from_u8(self.raws, self.sizes, dwin, (wh, ww), t.mean, t.inv_std, **kw)


@torch.no_grad()
def preprocess(raws, transform, net_sizes=None):
    """[(h_i, w_i, 3) uint8] -> [(3, H_i, W_i) fp32]: every image resized to its network size (transform.net_size, or
    net_sizes) and normalised, by the kernel of predict_raw with one whole-image window per image, one launch per distinct
    size.  predict_list on the result equals predict_raw on the raw images bit for bit; predict_raw does not form it."""
    src = _RawImages(raws, transform, net_sizes)
    out = [None] * len(raws)
    for (H, W), wins in _plan_windows("whole", None, None, src.sizes).batches:
        x = src.windows(wins, wins, H, W)   # the window list as it is: the wrapper copies it to the device
        for k, (i, _, _) in enumerate(wins):
            out[i] = x[k]
    return out


class TestAug:
    """mmseg's MultiScaleFlipAug(img_ratios, flip, flip_direction): the views of one image, in mmseg's order."""

    __test__ = False   # a product class, not a test

    def __init__(self, img_ratios=(1.0,), flip=False, flip_direction="horizontal"):
        ratios = [float(r) for r in ([img_ratios] if isinstance(img_ratios, (int, float)) else img_ratios)]
        if len(ratios) == 0:
            raise ValueError("TestAug: empty ratio list")
        if any(not r > 0.0 for r in ratios):
            raise ValueError(f"TestAug: ratios are positive, got {ratios}")
        if flip_direction not in ("horizontal", "vertical"):   # one direction: a list of them is not taken
            raise ValueError(f"TestAug: flip_direction is 'horizontal' or 'vertical', got {flip_direction!r}")
        self.img_ratios, self.flip, self.flip_direction = tuple(ratios), bool(flip), flip_direction

    def views(self, h, w, transform):
        """[(H, W, flags)] of an (h, w) image: for each ratio the unflipped view, then with flip the flipped one.  (H, W) is
        the keep-ratio test size at (int(s0 * r), int(s1 * r)) of the transform's img_scale; flags: ops.SEG_FLIP_H / _V."""
        out = []
        for r in self.img_ratios:
            H, W = test_size(h, w, (int(transform.img_scale[0] * r), int(transform.img_scale[1] * r)))
            out.append((H, W, 0))
            if self.flip:
                out.append((H, W, ops.SEG_FLIP_H if self.flip_direction == "horizontal" else ops.SEG_FLIP_V))
        return out


def _check_pictures(raws, maps=None, noun="a label map"):
    """Decoded pictures, (h, w, 3) uint8 device tensors, and with `maps` one map of every picture's size -> the sizes
    [(h, w)].  The pictures' strides are checked where their addresses are taken, by the table builders of ops."""
    if len(raws) == 0:
        raise ValueError("empty image list")
    if maps is not None and len(raws) != len(maps):
        raise ValueError(f"{len(raws)} images but {len(maps)} {noun.split(' ', 1)[1]}s")
    ops.L.require_cuda(*raws)
    for t in raws:
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8:
            raise ValueError(f"a decoded image is an (h, w, 3) uint8 tensor, got {t.dtype} {tuple(t.shape)}")
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in raws]
    if maps is not None:
        _check_maps(maps, noun, sizes)
    return sizes


def _check_maps(maps, noun="a label map", sizes=None, wide=False):
    """A list of (h, w) uint8 device maps, `noun` each in the messages.  sizes: those of the pictures they belong to; without
    them any non-empty size.  wide: the caller's kernels take 16-bit label maps too (components, despeckle, the boundary
    functions): uint8 or int16, one dtype per list."""
    plural = noun.split(" ", 1)[1] + "s"
    if len(maps) == 0:
        raise ValueError(f"empty list of {plural}")
    ops.L.require_cuda(*maps)
    dtypes = (torch.uint8, torch.int16) if wide else (torch.uint8,)
    words = "uint8 or int16" if wide else "uint8"
    for i, m in enumerate(maps):
        plain = m.dtype in dtypes and m.dim() == 2
        if sizes is None and not (plain and m.numel() > 0):
            raise ValueError(f"{noun} is a non-empty (h, w) {words} tensor, got {m.dtype} {tuple(m.shape)}")
        if sizes is not None and not (plain and tuple(m.shape) == sizes[i]):
            raise ValueError(f"{noun} is an (h, w) {words} tensor of its image's size {sizes[i]}, got {m.dtype} {tuple(m.shape)}")
        if m.dtype != maps[0].dtype:
            raise ValueError(f"the {plural} are all uint8 or all int16, one dtype per list; {plural[:-1]} 0 is {maps[0].dtype} and "
                             f"{plural[:-1]} {i} is {m.dtype}")
        if m.device != maps[0].device:
            raise ValueError(f"the {plural} are on different devices")


class _Maps:
    """A list of (h_i, w_i) maps of one element type (uint8 labels, groups and bands; int16 labels of the wide path) in one flat
    buffer: map i is the h_i * w_i elements of `flat` from offs[i], sizes[i] = (h_i, w_i); offsets count elements.  The kernels
    take `flat` and a table of the offsets; between two maps there may be elements that belong to none
    (the label kernels start every map at a multiple of 4), and what follows a kernel in the chain reads them as they are: an
    output that is passed on has them zeroed (empty_like)."""

    def __init__(self, flat, offs, sizes):
        self.flat, self.offs, self.sizes = flat, list(offs), [(int(h), int(w)) for (h, w) in sizes]

    @classmethod
    def of(cls, maps):
        """A list of maps of one dtype -> their batch.  Contiguous views of one storage (what predict_raw and groups_raw return) are used where
        they lie, without a copy; anything else is copied into a new zeroed buffer at offsets that are multiples of 4."""
        sizes = [tuple(m.shape) for m in maps]
        store = maps[0].untyped_storage().data_ptr()
        if all(m.is_contiguous() and m.untyped_storage().data_ptr() == store for m in maps):
            lo = min(m.storage_offset() for m in maps)
            hi = max(m.storage_offset() + m.numel() for m in maps)
            return cls(torch.as_strided(maps[0], (hi - lo,), (1,), lo), [m.storage_offset() - lo for m in maps], sizes)
        offs, n = cls._running([(m.numel() + 3) // 4 * 4 for m in maps])
        new = cls(torch.zeros(n, dtype=maps[0].dtype, device=maps[0].device), offs, sizes)
        for v, m in zip(new.views(), maps):
            v.copy_(m)
        return new

    @staticmethod
    def _running(lengths):
        """-> (the running sum before every length, the total)"""
        sums = [0, *itertools.accumulate(lengths)]
        return sums[:-1], sums[-1]

    @classmethod
    def gapless_of(cls, gts):
        """Ground truths laid one after the other, as the kernels that score against them take them -> (flat tensor, offsets);
        (None, None) without ground truths."""
        if gts is None:
            return None, None
        flat = gts[0].reshape(-1) if len(gts) == 1 else torch.cat([g.reshape(-1) for g in gts])
        return flat, cls._running([g.numel() for g in gts])[0]

    def packed(self):
        """The maps lie one after the other in list order and fill the buffer."""
        offs, n = self._running([h * w for h, w in self.sizes])
        return self.offs == offs and self.flat.numel() == n

    def views(self):
        """The per-image (h, w) views of the buffer."""
        return [self.flat[o:o + h * w].view(h, w) for o, (h, w) in zip(self.offs, self.sizes)]

    def empty_like(self):
        """An output buffer of the same layout; the bytes between the maps, which no kernel writes, are zero."""
        out = torch.empty_like(self.flat)
        return _Maps(out if self.packed() else out.zero_(), self.offs, self.sizes)

    def gapless(self):
        """The maps one after the other in a flat tensor: `flat` itself where they lie so already, else a copy."""
        return self.flat if self.packed() else torch.cat([v.reshape(-1) for v in self.views()])


class PAMR:
    """Pixel-adaptive mask refinement (Araslanov & Roth, CVPR 2020) as a post-processing step of the label maps: `iters`
    iterations of an affinity-weighted average over the 8 neighbours at each of `dilations` (csrc/segment_refine.inc; the
    definition stands in include/segclip_hip.h).  The defaults are the paper's.  The reference has no refinement."""

    def __init__(self, iters=10, dilations=(8, 16)):
        if isinstance(iters, bool) or not isinstance(iters, int) or not 0 <= iters <= ops.SEG_REFINE_MAX_ITERS:
            raise ValueError(f"PAMR: iters is an integer in 0 .. {ops.SEG_REFINE_MAX_ITERS}, got {iters!r}")
        try:
            dil = tuple(dilations)
        except TypeError:
            raise ValueError(f"PAMR: dilations is a sequence of integers, got {dilations!r}") from None
        if not 1 <= len(dil) <= ops.SEG_REFINE_MAX_DILATIONS:
            raise ValueError(f"PAMR: dilations holds 1 .. {ops.SEG_REFINE_MAX_DILATIONS} values, got {len(dil)}")
        if any(isinstance(d, bool) or not isinstance(d, int) or not 1 <= d <= ops.SEG_REFINE_MAX_DILATION for d in dil):
            raise ValueError(f"PAMR: dilations are integers in 1 .. {ops.SEG_REFINE_MAX_DILATION}, got {dil}")
        if any(b <= a for a, b in zip(dil, dil[1:])):
            raise ValueError(f"PAMR: dilations must be strictly increasing, got {dil}")
        self.iters, self.dilations = iters, dil


def _refine_maps(raws, maps, num_classes, transform, pamr, gts=None, areas=None, ignore_index=255, reduce_zero_label=False):
    """The refinement of a list call: maps [(h_i, w_i) uint8] of the pictures' own sizes -> the refined maps, views of one new
    buffer; with gts the areas of the refined maps are added to `areas` by the refinement's last kernel."""
    if not isinstance(pamr, PAMR):
        raise TypeError("refine is a PAMR")
    if not isinstance(transform, ImageTransform):
        raise TypeError("transform is an ImageTransform")
    _check_pictures(raws, maps)
    if gts is not None:
        for g, m in zip(gts, maps):
            if tuple(g.shape) != tuple(m.shape):
                raise ValueError(f"refine: a ground truth has its picture's size {tuple(m.shape)}, got {tuple(g.shape)}")
    batch = _Maps.of(maps)
    table, n_blocks, side = ops.seg_refine_table(list(raws), batch.offs)
    out = ops.seg_refine(table, n_blocks, batch.flat, num_classes, pamr.dilations, pamr.iters, transform.mean, transform.inv_std,
                         reverse_channels=transform.channel_order == "bgr", gt=_Maps.gapless_of(gts)[0], areas=areas,
                         ignore_index=ignore_index, reduce_zero_label=reduce_zero_label, max_side=side)
    return _Maps(out, batch.offs, batch.sizes).views()


@torch.no_grad()
def refine_labels(raws, labels, num_classes, transform, pamr):
    """raws [(h_i, w_i, 3) uint8 decoded images, rows possibly strided], labels [(h_i, w_i) uint8 label maps at the pictures'
    own sizes] -> [(h_i, w_i) uint8 refined maps], views of one buffer: `pamr` (a PAMR) applied to every map, all images in one
    call and without a host synchronisation.  transform supplies the normalisation and the pictures' channel order.  The
    inputs stay as they are."""
    return _refine_maps(raws, labels, num_classes, transform, pamr)


class Despeckle:
    """Despeckling as a post-processing step of the label maps: the connected components (`connectivity` 4 or 8) with fewer
    than `min_area` pixels are removed; the pixels of `skip_label` belong to no component and stay.
    merge=False: every such component becomes `fill`.  One pass: what became `fill` is not merged again
    (csrc/segment_objects.inc, segclip_seg_components).  It suits vocabularies whose class 0 is the background.
    merge=True: every such component takes the label of its largest neighbour among the components of at least min_area pixels
    that touch it left, right, up or down (among equal areas the smallest label), `rounds` (1 .. 8) times with the components
    formed anew: a speck nested in a speck needs two.  A small component that touches no such neighbour keeps its label, or
    becomes `fill` after the last round; fill=None keeps it (csrc/segment_sieve.inc, segclip_seg_sieve).  It is for the
    vocabularies without a background class, where a constant fill would paint the specks with a real class.
    The definitions stand in include/segclip_hip.h.  The reference has no such step.
    `fill` and `skip_label` are in 0 .. 255 here whatever the maps' width: through this class a 16-bit map (despeckle on int16
    maps) can be filled with, or skip, one of the first 256 values only; ops.seg_components and ops.seg_sieve take 0 .. 65535."""

    def __init__(self, min_area, fill=0, connectivity=8, skip_label=None, merge=False, rounds=1):
        if isinstance(min_area, bool) or not isinstance(min_area, int) or min_area < 0:
            raise ValueError(f"Despeckle: min_area is a non-negative integer, got {min_area!r}")
        if not isinstance(merge, bool):
            raise ValueError(f"Despeckle: merge is True or False, got {merge!r}")
        if fill is None and not merge:
            raise ValueError("Despeckle: fill=None (orphans keep their label) needs merge=True")
        if fill is not None and (isinstance(fill, bool) or not isinstance(fill, int) or not 0 <= fill <= 255):
            raise ValueError(f"Despeckle: fill is an integer in 0 .. 255{' or None' if merge else ''}, got {fill!r}")
        if isinstance(connectivity, bool) or connectivity not in (4, 8):
            raise ValueError(f"Despeckle: connectivity is 4 or 8, got {connectivity!r}")
        if skip_label is not None and (isinstance(skip_label, bool) or not isinstance(skip_label, int) or not 0 <= skip_label <= 255):
            raise ValueError(f"Despeckle: skip_label is None or an integer in 0 .. 255, got {skip_label!r}")
        if isinstance(rounds, bool) or not isinstance(rounds, int) or not 1 <= rounds <= ops.SEG_SIEVE_MAX_ROUNDS:
            raise ValueError(f"Despeckle: rounds is an integer in 1 .. {ops.SEG_SIEVE_MAX_ROUNDS}, got {rounds!r}")
        if rounds != 1 and not merge:
            raise ValueError(f"Despeckle: rounds={rounds} needs merge=True (the fill mode is one pass)")
        self.min_area, self.fill, self.connectivity, self.skip_label = min_area, fill, connectivity, skip_label
        self.merge, self.rounds = merge, rounds


class Objects:
    """The connected components of a list of label maps (components): ids [(h_i, w_i) int32 maps, views of one buffer: the id
    of a pixel's component = the flat index y * w + x of the component's first pixel in raster order, -1 where the label is
    skipped], records ((n, 10) int64 device tensor, one row per component in ascending (image, id) order: image, id, label,
    area, y0, x0, y1, x1, sum of y, sum of x; y1 and x1 exclusive) and count = n."""

    def __init__(self, ids, records, count):
        self.ids, self.records, self.count = ids, records, count

    def boxes(self):
        """(n, 6) int64: image, label, y0, x0, y1, x1 (y1 and x1 exclusive)"""
        return self.records[:, [0, 2, 4, 5, 6, 7]]

    def centroids(self):
        """(n, 2) fp64: (sum of y / area, sum of x / area)"""
        return self.records[:, 8:10].double() / self.records[:, 3:4].double()


@torch.no_grad()
def components(maps, connectivity=8, skip_label=None, max_objects=None):
    """maps [(h_i, w_i) label maps of any mix of sizes, all uint8 or all int16 (16-bit maps read as unsigned values, those of
    SegInference(label_dtype=torch.int16))] -> Objects: the connected components of every map, labelled on the device in one
    call; the label column of the records carries the 16-bit label.  max_objects bounds the record list (default: one row per
    16 pixels, at least 4096 rows).  Reading the count is the ONE host synchronisation of this function; more components
    than max_objects raise a ValueError that names both numbers (ask again with a larger max_objects)."""
    maps = list(maps)
    _check_maps(maps, wide=True)
    batch = _Maps.of(maps)
    dev = batch.flat.device
    if max_objects is None:
        max_objects = max(4096, sum(h * w for h, w in batch.sizes) // 16)
    if isinstance(max_objects, bool) or not isinstance(max_objects, int) or max_objects < 1:
        raise ValueError(f"components: max_objects is a positive integer, got {max_objects!r}")
    table, n_blocks, side = ops.seg_components_table(batch.sizes, batch.offs, dev)
    ids = torch.empty(batch.flat.numel(), dtype=torch.int32, device=dev)   # only the maps' own entries are ever seen
    records = torch.empty(max_objects, ops.SEG_CC_RECORD, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ops.seg_components(table, n_blocks, batch.flat, connectivity=connectivity, skip_label=skip_label, ids=ids, records=records,
                       count=count, max_side=side)
    n = int(count.item())
    if n > max_objects:
        raise ValueError(f"components: the maps hold {n} components but max_objects is {max_objects}")
    return Objects(_Maps(ids, batch.offs, batch.sizes).views(), records[:n], n)


def _check_clean(clean):
    if not isinstance(clean, Despeckle):
        raise TypeError("clean is a Despeckle")


def _despeckle_maps(maps, clean):
    """-> the cleaned maps, a _Maps over one new buffer"""
    _check_clean(clean)
    maps = list(maps)
    _check_maps(maps, wide=True)
    batch = _Maps.of(maps)
    table, n_blocks, side = ops.seg_components_table(batch.sizes, batch.offs, batch.flat.device)
    out = batch.empty_like()
    if clean.merge:
        ops.seg_sieve(table, n_blocks, batch.flat, connectivity=clean.connectivity, skip_label=clean.skip_label,
                      min_area=clean.min_area, orphan_fill=clean.fill, rounds=clean.rounds, cleaned=out.flat, max_side=side)
    else:
        ops.seg_components(table, n_blocks, batch.flat, connectivity=clean.connectivity, skip_label=clean.skip_label,
                           min_area=clean.min_area, fill=clean.fill, cleaned=out.flat, max_side=side)
    return out


@torch.no_grad()
def despeckle(maps, min_area, fill=0, connectivity=8, skip_label=None, merge=False, rounds=1):
    """maps [(h_i, w_i) label maps, all uint8 or all int16] -> [(h_i, w_i) maps of the same dtype], views of one new buffer:
    every connected component with fewer than min_area pixels replaced by `fill`, or with merge=True merged into its largest
    neighbour in `rounds` rounds (see Despeckle), all maps in one call and without a host synchronisation.  int16 maps are the
    16-bit label maps of SegInference(label_dtype=torch.int16), read as unsigned values; `fill` and `skip_label` stay in
    0 .. 255 (Despeckle).  The inputs stay as they are."""
    return _despeckle_maps(maps, Despeckle(min_area, fill, connectivity, skip_label, merge, rounds)).views()


def _int_in(owner, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{owner}: {name} is an integer in {lo} .. {hi}, got {v!r}")
    return v


class Superpixels:
    """Superpixels of the decoded pictures: an integer SLIC on the RGB bytes (csrc/segment_superpixel.inc; the definition
    stands in include/segclip_hip.h).  step: the side of a grid cell, an image of (h, w) pixels has ceil(h / step) *
    ceil(w / step) centres; compactness: the weight of the distance in the plane against the distance in colour; iters: rounds
    of (assignment, update) before the final assignment.  No connectivity pass belongs to the definition: a segment need not be
    connected (components gives the connected parts of any id map).  The reference has no superpixels."""

    def __init__(self, step=16, compactness=10, iters=5):
        self.step = _int_in("Superpixels", "step", step, ops.SEG_SP_MIN_STEP, ops.SEG_SP_MAX_STEP)
        self.compactness = _int_in("Superpixels", "compactness", compactness, 1, ops.SEG_SP_MAX_COMPACTNESS)
        self.iters = _int_in("Superpixels", "iters", iters, 0, ops.SEG_SP_MAX_ITERS)

    def grid(self, h, w):
        """(rows, columns) of the centres of an (h, w) picture"""
        return -(-int(h) // self.step), -(-int(w) // self.step)

    def count(self, h, w):
        """K of an (h, w) picture: its segment ids are 0 .. K - 1"""
        gh, gw = self.grid(h, w)
        return gh * gw


class Segments:
    """Segment maps of a list of images: maps [(h_i, w_i) int32, views of one flat buffer; the ids of image i are
    0 .. counts[i] - 1, and an id may be unused], counts [K per image].  centres: None, or the (sum of counts, 5) int32 final
    (y, x, r, g, b) of every centre, image after image."""

    def __init__(self, maps, counts, centres=None):
        self.maps, self.counts, self.centres = list(maps), [int(k) for k in counts], centres


def _check_superpixels(sp):
    if not isinstance(sp, Superpixels):
        raise TypeError("superpixels is a Superpixels")


@torch.no_grad()
def superpixels(raws, sp=None, centres=False):
    """raws [(h_i, w_i, 3) uint8 decoded images of any mix of sizes, rows possibly strided] -> Segments: the superpixels of
    every picture under `sp` (a Superpixels; the defaults without one), all pictures in every launch of one call and without a
    host synchronisation.  centres=True also returns the final centres.  The pictures stay as they are."""
    sp = Superpixels() if sp is None else sp
    _check_superpixels(sp)
    raws = list(raws)
    sizes = _check_pictures(raws)
    table, n_blocks, side, counts = ops.seg_superpixels_table(raws, sp.step)
    dev = raws[0].device
    offs, n = _Maps._running([h * w for h, w in sizes])
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    cen = torch.empty(sum(counts), 5, dtype=torch.int32, device=dev) if centres else None
    ops.seg_superpixels(table, n_blocks, ids, sum(counts), sp.step, sp.compactness, sp.iters, centres=cen, max_side=side)
    return Segments(_Maps(ids, offs, sizes).views(), counts, cen)


def _check_min_share(owner, min_share):
    return _int_in(owner, "min_share", min_share, 0, 100)


def _snap_maps(labels, segments, num_classes, counts=None, min_share=0):
    """-> the snapped maps, a _Maps over one new buffer"""
    labels = list(labels)
    _check_maps(labels, wide=True)
    _check_min_share("snap_labels", min_share)
    if isinstance(segments, Segments):
        if counts is not None:
            raise ValueError("snap_labels: a Segments carries its counts; counts= goes with a list of segment maps")
        segments, counts = segments.maps, segments.counts
    else:
        if counts is None:
            raise ValueError("snap_labels: a list of segment maps needs counts, the number of segments of every image (finding "
                             "the largest id would cost a host synchronisation)")
        segments, counts = list(segments), list(counts)
    if len(segments) != len(labels) or len(counts) != len(labels):
        raise ValueError(f"snap_labels: {len(labels)} label maps but {len(segments)} segment maps and {len(counts)} counts")
    ops.L.require_cuda(*segments)
    for m, s in zip(labels, segments):
        if s.dtype != torch.int32 or s.dim() != 2 or tuple(s.shape) != tuple(m.shape):
            raise ValueError(f"snap_labels: a segment map is an (h, w) int32 tensor of its label map's size {tuple(m.shape)}, got "
                             f"{s.dtype} {tuple(s.shape)}")
        if s.device != m.device:
            raise ValueError("snap_labels: the segment maps and the label maps are on different devices")
    for k in counts:
        _int_in("snap_labels", "a segment count", k, 1, ops.SEG_VOTE_MAX_SEGMENTS)
    limit = ops.SEG_WIDE_MAX_CLASSES if labels[0].dtype == torch.int16 else 256
    _int_in("snap_labels", f"num_classes ({'int16' if limit > 256 else 'uint8'} labels)", num_classes, 1, limit)
    batch = _Maps.of(labels)
    # the segment ids at the labels' offsets: where both lists lie packed in list order (predict_raw's maps under
    # out_shapes = the raw sizes never do: the label kernels start every map at a multiple of 4) the ids are read where they are
    store = segments[0].untyped_storage().data_ptr()
    lo = min(s.storage_offset() for s in segments)
    if all(s.is_contiguous() and s.untyped_storage().data_ptr() == store for s in segments) \
            and [s.storage_offset() - lo for s in segments] == batch.offs \
            and max(s.storage_offset() + s.numel() for s in segments) - lo == batch.flat.numel():
        ids = torch.as_strided(segments[0], (batch.flat.numel(),), (1,), lo)
    else:
        ids = torch.zeros(batch.flat.numel(), dtype=torch.int32, device=batch.flat.device)
        for v, s in zip(_Maps(ids, batch.offs, batch.sizes).views(), segments):
            v.copy_(s)
    return _vote(batch, ids, counts, num_classes, min_share)


def _vote(batch, ids, counts, num_classes, min_share):
    """batch: the label maps, ids: flat int32 segment ids at the labels' offsets -> the snapped maps, a _Maps over a new buffer"""
    table, n_blocks, total, top = ops.seg_vote_table(batch.sizes, batch.offs, counts, batch.flat.device)
    out = batch.empty_like()
    ops.seg_vote(table, n_blocks, batch.flat, ids, total, num_classes, min_share=min_share, out=out.flat, max_count=top)
    return out


def _snap_stage(raws, labels, num_classes, snap):
    """The snap stage of the chain: the superpixels of the pictures written at the label maps' own offsets, then the vote
    -> the snapped maps, a _Maps over one new buffer"""
    _check_snap(snap)
    raws = list(raws)
    _check_pictures(raws, labels)
    batch = _Maps.of(labels)
    sp = snap.superpixels
    table, n_blocks, side, counts = ops.seg_superpixels_table(raws, sp.step, batch.offs)
    ids = torch.empty(batch.flat.numel(), dtype=torch.int32, device=batch.flat.device)   # only the maps' own entries are ever read
    ops.seg_superpixels(table, n_blocks, ids, sum(counts), sp.step, sp.compactness, sp.iters, max_side=side)
    return _vote(batch, ids, counts, num_classes, snap.min_share)


@torch.no_grad()
def snap_labels(labels, segments, num_classes, counts=None, min_share=0):
    """labels [(h_i, w_i) label maps, all uint8 or all int16 (16-bit maps read as unsigned values)], segments (a Segments, what
    superpixels returns, or a list of (h_i, w_i) int32 maps of the caller's own - Felzenszwalb maps, flattened instance masks
    - with counts [K_i]: the ids of image i are 0 .. K_i - 1) -> [(h_i, w_i) maps of the labels' dtype], views of one new
    buffer: every segment gives its pixels the label most of them carry (csrc/segment_vote.inc; the definition stands in
    include/segclip_hip.h).  A pixel votes when its label is below num_classes and its id lies in 0 .. K_i - 1; among equal
    counts the smallest class wins; a segment snaps when the winner holds at least min_share percent (an integer, 0 .. 100) of
    its voters; every other pixel keeps its value (a label >= num_classes such as an ignore value, an id outside the range,
    a segment that does not snap).  All maps in one call and without a host synchronisation.  The inputs stay as they are."""
    return _snap_maps(labels, segments, num_classes, counts, min_share).views()


class Snap:
    """Snapping as a post-processing step of the label maps: the superpixels of the decoded picture (`superpixels`, a
    Superpixels) vote, and every superpixel whose most frequent label holds at least `min_share` percent of it takes that label
    (snap_labels).  The third answer, beside PAMR and Despeckle, to label maps whose borders follow the patch grid: it is cheap,
    needs no soft masks and composes with both.  The reference has no such step."""

    def __init__(self, superpixels=None, min_share=0):
        sp = Superpixels() if superpixels is None else superpixels
        if not isinstance(sp, Superpixels):
            raise TypeError("Snap: superpixels is a Superpixels")
        self.superpixels, self.min_share = sp, _check_min_share("Snap", min_share)


def _check_snap(snap):
    if not isinstance(snap, Snap):
        raise TypeError("snap is a Snap")


class Boundary:
    """The band of the boundary metrics: the pixels of a map within `radius` pixels (Chebyshev distance) of a pixel with another
    label or of the picture frame.  ratio: the radius as a share of the map's diagonal, d = max(1, round(ratio * sqrt(h^2 +
    w^2))) - 0.02 is the default of Boundary IoU (Cheng et al., CVPR 2021); radius: a fixed radius in pixels that overrides
    the ratio (the trimap widths of the DeepLab papers).  csrc/segment_boundary.inc; the definition stands in
    include/segclip_hip.h.  The reference has no such measure."""

    def __init__(self, ratio=0.02, radius=None):
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not math.isfinite(ratio) or not ratio > 0:
            raise ValueError(f"Boundary: ratio is a positive number, got {ratio!r}")
        if radius is not None and (isinstance(radius, bool) or not isinstance(radius, int) or
                                   not 1 <= radius <= ops.SEG_BOUNDARY_MAX_RADIUS):
            raise ValueError(f"Boundary: radius is None or an integer in 1 .. {ops.SEG_BOUNDARY_MAX_RADIUS}, got {radius!r}")
        self.ratio, self.radius = float(ratio), radius

    def radius_of(self, h, w, image=None):
        """The radius of an (h, w) map; one above the kernel's limit raises, naming the image."""
        if self.radius is not None:
            return self.radius
        d = max(1, int(round(self.ratio * math.sqrt(h * h + w * w))))
        if d > ops.SEG_BOUNDARY_MAX_RADIUS:
            name = "a map" if image is None else f"image {image}"
            raise ValueError(f"Boundary: {name} of {h}x{w} has the radius {d} at ratio {self.ratio}, at most "
                             f"{ops.SEG_BOUNDARY_MAX_RADIUS} supported (pass a fixed radius)")
        return d


def _check_boundary(boundary):
    if not isinstance(boundary, Boundary):
        raise TypeError("boundary is a Boundary")


def _boundary_call(batch, boundary, gts=None, **kw):
    """ops.seg_boundary over a _Maps and the ground truths of its maps, laid gapless one after the other."""
    radii = [boundary.radius_of(h, w, i) for i, (h, w) in enumerate(batch.sizes)]
    for g, hw in zip(gts or (), batch.sizes):
        if tuple(g.shape) != hw:
            raise ValueError(f"boundary: a ground truth has its label map's size {hw}, got {tuple(g.shape)}")
    gt, gt_offs = _Maps.gapless_of(gts)
    table, n_blocks, side = ops.seg_boundary_table(batch.sizes, batch.offs, gt_offs, radii, batch.flat.device)
    ops.seg_boundary(table, n_blocks, batch.flat, gt=gt, max_side=side, **kw)


@torch.no_grad()
def boundary_bands(maps, boundary):
    """maps [(h_i, w_i) label maps of any mix of sizes, all uint8 or all int16 (16-bit maps read as unsigned values)] ->
    [(h_i, w_i) uint8 band maps, whatever the labels' dtype], views of one new buffer: bit 0 where a pixel within the radius
    (boundary.radius_of(h_i, w_i), Chebyshev distance, inside the map) carries another label, bit 1 where
    the (2d+1)^2 window leaves the map.  (map == k) & (band != 0) is Boundary IoU's mask_to_boundary of class k.
    All maps in one call and without a host synchronisation; the inputs stay as they are."""
    _check_boundary(boundary)
    maps = list(maps)
    _check_maps(maps, wide=True)
    batch = _Maps.of(maps)
    flat = torch.empty(batch.flat.numel(), dtype=torch.uint8, device=batch.flat.device)
    band = _Maps(flat if batch.packed() else flat.zero_(), batch.offs, batch.sizes)   # as empty_like, one byte per label
    _boundary_call(batch, boundary, pred_band=band.flat)
    return band.views()


@torch.no_grad()
def boundary_areas(preds, gts, num_classes, boundary, ignore_index=255, reduce_zero_label=False, areas=None):
    """preds, gts [(h_i, w_i), all uint8 or all int16] -> (2, 3, C) int64 on the device, added to `areas` when given: slot 0 the intersection,
    prediction area and label area of Boundary IoU (each side restricted to its own band), slot 1 those of the trimap (the
    pixels within the radius of a change of the ground truth's label).  The ground-truth rule (ignore_index,
    reduce_zero_label, values >= C) is ops.seg_areas'.  With int16 preds the ground truths are int16 too (16-bit maps read as
    unsigned values), num_classes is at most 1024 and ignore_index is in 0 .. 65535 (65535 is the usual choice).
    SegEvaluator.boundary_metrics_from_areas turns a host copy into figures.  One call, no host synchronisation."""
    _check_boundary(boundary)
    preds, gts = list(preds), list(gts)
    _check_maps(preds, wide=True)
    if len(preds) != len(gts):
        raise ValueError(f"{len(preds)} predictions but {len(gts)} ground truths")
    SegEvaluator._check_gts(preds, gts, preds[0].dtype)
    if areas is None:
        areas = torch.zeros(2, 3, int(num_classes), dtype=torch.int64, device=preds[0].device)
    _boundary_call(_Maps.of(preds), boundary, gts=gts, num_classes=num_classes, ignore_index=ignore_index,
                   reduce_zero_label=reduce_zero_label, areas=areas)
    return areas


def _image_areas_call(batch, gts, num_classes, **rule):
    """ops.seg_image_areas over a _Maps, read where its maps lie (gaps included), and the ground truths of its maps, laid
    gapless one after the other -> (B, 3, C) int64."""
    gt, gt_offs = _Maps.gapless_of(gts)
    table, n_blocks = ops.seg_image_areas_table(batch.offs, gt_offs, [h * w for h, w in batch.sizes], batch.flat.device)
    return ops.seg_image_areas(batch.flat, gt, table, n_blocks, num_classes, **rule)


@torch.no_grad()
def image_areas(preds, gts, num_classes, ignore_index=255, reduce_zero_label=False):
    """preds, gts [(h_i, w_i) maps of any mix of sizes, all uint8 or all int16 (16-bit maps read as unsigned values), sizes equal
    pairwise] -> (B, 3, C) int64 on the device: row i is the intersection, prediction area and label area per class of picture
    i alone, ops.seg_areas of that pair value for value (the same ground-truth rule: ignore_index, reduce_zero_label, values
    >= C), so the sum of the rows is the (3, C) `areas` of the list.  Predictions that are views of one buffer (what predict_raw
    returns) are read where they lie.  One call, no host synchronisation.  SegEvaluator.fine_grained_from_image_areas,
    worst_images and bootstrap_miou turn the rows into figures."""
    preds, gts = list(preds), list(gts)
    _check_maps(preds, wide=True)
    if len(preds) != len(gts):
        raise ValueError(f"{len(preds)} predictions but {len(gts)} ground truths")
    SegEvaluator._check_gts(preds, gts, preds[0].dtype)
    for i, (p, g) in enumerate(zip(preds, gts)):
        if tuple(p.shape) != tuple(g.shape):
            raise ValueError(f"image_areas: a ground truth has its label map's size {tuple(p.shape)}, ground truth {i} is {tuple(g.shape)}")
    return _image_areas_call(_Maps.of(preds), gts, num_classes, ignore_index=ignore_index, reduce_zero_label=reduce_zero_label)


def _check_stages(refine, clean, raws, out_shapes, snap=None):
    """refine=, snap= and clean= of predict_raw / update_raw: a PAMR and a Snap, each with label maps at the pictures' own
    sizes, and a Despeckle.  It runs before the source is built: what the host does between the source's table copy and the
    first launch is not hidden behind the device's work."""
    if clean is not None:
        _check_clean(clean)
    if refine is not None and not isinstance(refine, PAMR):
        raise TypeError("refine is a PAMR")
    if snap is not None:
        _check_snap(snap)
    if (refine is None and snap is None) or out_shapes is None:
        return
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in raws]
    if [(int(a), int(b)) for (a, b) in out_shapes] != sizes:
        if refine is not None:
            raise ValueError(f"refine: out_shapes must be the raw images' own sizes {sizes} (the refinement reads the picture under "
                             f"every label), got {list(out_shapes)}")
        raise ValueError(f"snap: out_shapes must be the raw images' own sizes {sizes} (a superpixel lies in the picture under "
                         f"the labels), got {list(out_shapes)}")


def _refuse(entry, *stages):
    """The entry points that do not take a stage of the chain: stages = (name, what the caller gave, the advice); the first
    one given raises."""
    for name, given, advice in stages:
        if given is not None:
            raise ValueError(f"{entry}: {name} {advice}")


# What an evaluator's call hands to the chain: the ground truths, the (3, C) areas, the ground-truth rule (ignore_index and
# reduce_zero_label, as keyword arguments of every kernel that counts), the Boundary or None and its (2, 3, C) areas, the
# confusion matrix or None, and the list that takes the call's (B, 3, C) per-image areas or None.
_Score = collections.namedtuple("_Score", "gts areas rule boundary boundary_areas confusion per_image", defaults=(None, None))


def _out_shapes(src, out_shapes):
    """The output sizes of a list call, one per image: the caller's, or the source's default."""
    n_img = len(src.view_counts)
    if out_shapes is None:
        out_shapes = src.default_out
    if out_shapes is None or len(out_shapes) != n_img:
        raise ValueError(f"{n_img} images but {0 if out_shapes is None else len(out_shapes)} output shapes")
    return [(int(a), int(b)) for (a, b) in out_shapes]


def _require_eval(model):
    if model.training:
        raise RuntimeError("segclip_amd.segmentation: call model.eval() first (training mode draws Gumbel noise)")


def build_text_embedding(model, text_tokens, chunk=1024):
    """(N, T, L) int64 prompt ids (N classes x T templates) -> (N, C): encode_text, mean over the templates, L2 norm
    (evaluation/builder.py:59-66).  The N * T captions go through the text tower `chunk` rows at a time."""
    ops.L.require_cuda(text_tokens)
    _require_eval(model)
    N, T, Lc = text_tokens.shape
    flat = text_tokens.reshape(N * T, Lc)
    with torch.no_grad():
        feats = [model.clip.encode_text(flat[i:i + chunk].contiguous()).float() for i in range(0, N * T, chunk)]
        emb = (feats[0] if len(feats) == 1 else torch.cat(feats)).view(N, T, -1).mean(dim=1)
        return ops.L2NormFn.apply(emb)


class SegInference:
    """ViTSegInference (evaluation/vit_seg.py:118-256) with mmseg's test modes.

    mode="whole": H and W multiples of the patch size, one window per image.  mode="slide": any H, W >= crop, mmseg's
    window grid; overlapping windows average their logits.  All windows of all images of a call go through one
    encode_image call (at most `max_windows` at a time).

    label_dtype=torch.int16: vocabularies of up to 1024 classes (Pascal-Context-459, ADE20K-847) without the dense logits.
    predict, predict_list and predict_raw then return int16 maps (csrc/segment_wide.inc; below 257 classes they hold the values
    of the uint8 maps), and a SegEvaluator over it takes int16 ground truths.  group_map, groups_list, groups_raw and
    encode_decode do not depend on it.  The in-pipeline stages are not built for 16-bit maps, each refused by name before
    anything is launched: aug= / predict_views / update_views, refine=, clean=, SegEvaluator(boundary=), SegSweepEvaluator and
    render_raw.  The stand-alone functions take the int16 maps these methods return: components, despeckle (fill and merge),
    boundary_bands, boundary_areas, and SegEvaluator.update_maps scores maps that exist already - predict_raw, despeckle,
    update_maps is the chain of a wide vocabulary.  Out of scope: PAMR for more than 256 classes (its ceil(C / 8) x T launch
    plan and its 256-bit presence map need another design) and test-time augmentation of wide maps."""

    label_dtype, wide = torch.uint8, False   # the default path; __init__ sets both

    def __init__(self, model, text_embedding, with_bg, bg_thresh=0.95, mode="whole", crop_size=(224, 224), stride=(224, 224),
                 max_windows=256, label_dtype=torch.uint8):
        if mode not in ("whole", "slide"):
            raise ValueError(f"mode must be 'whole' or 'slide', got {mode!r}")
        if label_dtype not in (torch.uint8, torch.int16):
            raise ValueError(f"label_dtype is torch.uint8 (at most 256 classes) or torch.int16 (at most {ops.SEG_WIDE_MAX_CLASSES}), "
                             f"got {label_dtype!r}")
        self.label_dtype, self.wide = label_dtype, label_dtype == torch.int16
        ops.L.require_cuda(text_embedding)
        self.model = model
        self.text_embedding = text_embedding.detach().float().contiguous()
        self.with_bg, self.bg_thresh, self.mode = bool(with_bg), float(bg_thresh), mode
        self.crop_size, self.stride, self.max_windows = tuple(crop_size), tuple(stride), int(max_windows)
        self.num_classes = self.text_embedding.shape[0] + int(self.with_bg)
        self._memo = {}

    def window_list(self, B, H, W):
        """(windows [(image, y0, x0)], (win_h, win_w)) of a (B, 3, H, W) batch."""
        plan = _plan_windows(self.mode, self.crop_size, self.stride, [(H, W)] * B)
        return [w for _, wins in plan.batches for w in wins], ((H, W) if self.mode == "whole" else self.crop_size)

    def _device_plan(self, src, image_first=False):
        """(_plan_windows of a source, checked against the tower; its windows as (nW, 3) int32 device rows; with image_first
        the (images + 1) int32 device list of every image's first window, for sources of one view per image).  The last
        call shape - sizes, view counts, device - is remembered (a dataset of varying sizes does not accumulate plans)."""
        key = (tuple(src.sizes), tuple(src.view_counts), str(src.device))
        memo = self._memo
        if memo.get("key") != key:
            plan = _plan_windows(self.mode, self.crop_size, self.stride, src.sizes, src.view_counts)
            visual = self.model.clip.visual
            _check_tower_windows(plan, src.name, visual.patch_size, visual.transformer.patch_len ** 2)
            wins = [w for _, ws in plan.batches for w in ws]
            memo = self._memo = dict(key=key, plan=plan, dfirst=None,
                                     dwin=torch.tensor(wins, dtype=torch.int32, device=src.device).view(-1, 3))
        if image_first and memo["dfirst"] is None:
            firsts = [first for first, _, _ in memo["plan"].entries] + [memo["dwin"].shape[0]]
            memo["dfirst"] = torch.tensor(firsts, dtype=torch.int32, device=src.device)
        return memo["plan"], memo["dwin"], memo["dfirst"]

    def _list_towers(self, src, plan, dwin, classes=True):
        """The tower part of every call: every window of the plan through encode_image (max_windows at a time) and, with
        `classes`, segclip_seg_group_table.  -> (flat soft_attn, tables, a window's offset in soft_attn, group count)."""
        _require_eval(self.model)
        N = self.text_embedding.shape[0]
        parts, done, win_off, floats = [], 0, [], 0
        for (wh, ww), wins in plan.batches:
            for s in range(0, len(wins), self.max_windows):
                chunk = wins[s:s + self.max_windows]
                x = src.windows(chunk, dwin[done + s:done + s + len(chunk)], wh, ww)
                # the reference segments one image per call, where the two key layouts of the cross-attention block coincide;
                # in a batch only "intended" keeps every window attending to its own tokens (config.py, SURVEY finding 0.4)
                with config.scope(cross_mode="intended"):
                    feat, hidden, mid = self.model.clip.encode_image(x, return_hidden=True)
                if not mid["attns"]:
                    raise ValueError(f"{src.name(chunk[0][0])}: window {wh}x{ww}: the vision tower takes its segmentation "
                                     "branch only at 1x or 4x the training token count (modules/module_seg_vit.py:423)")
                soft = mid["attns"][-1]["soft_attn"]
                del mid, x
                tables = ()
                if classes:
                    tables = ops.seg_group_table(hidden[:, 1:, :], feat, self.text_embedding, self.model.clip.logit_scale, min(5, N))
                win_off += range(floats, floats + soft.numel(), soft.numel() // soft.shape[0])
                floats += soft.numel()
                n_groups = int(soft.shape[1])
                parts.append((soft.reshape(-1),) + tables)
            done += len(wins)
        if len(parts) == 1:
            soft, tables = parts[0][0], parts[0][1:]
        else:
            cat = [torch.cat([q[i] for q in parts]) for i in range(len(parts[0]))]
            soft, tables = cat[0], tuple(cat[1:])
        return soft, tables, win_off, n_groups

    def _check_classes(self):
        if self.wide:
            if self.num_classes > ops.SEG_WIDE_MAX_CLASSES:
                raise ops.L.Unsupported(f"{self.num_classes} classes: the 16-bit label-map kernels hold at most "
                                        f"{ops.SEG_WIDE_MAX_CLASSES}; use encode_decode")
        elif self.num_classes > 256:
            raise ops.L.Unsupported(f"{self.num_classes} classes: the label-map kernels hold at most 256; use encode_decode or "
                                    "label_dtype=torch.int16")

    def _refuse_wide(self, entry, **stages):
        """The stages that are not built for 16-bit label maps: the first one given raises, by its name."""
        if self.wide:
            _refuse(entry, *((name, given, "is not built for 16-bit label maps (label_dtype=torch.int16)")
                             for name, given in stages.items()))

    def _batch_forward(self, img, classes=True):
        """Vision tower + group tables of every window of a (B, 3, H, W) batch -> the pixel kernels' arguments.
        classes=False (group_map: the groups do not depend on the classes): zero tables of one class."""
        src = _BatchImages(img, self.mode == "whole")
        plan, dwin, dfirst = self._device_plan(src, image_first=True)
        soft, tables, _, G = self._list_towers(src, plan, dwin, classes)
        if not classes:
            n = dwin.shape[0]
            tables = (soft.new_zeros(n, G, 1), soft.new_zeros(n), soft.new_zeros(n, G, dtype=torch.int32), soft.new_zeros(n, G))
        (B, _, H, W), (wh, ww), p = img.shape, plan.entries[0][2], self.model.clip.visual.patch_size
        return soft, tables, dwin, dfirst, (B, H, W), (wh, ww), (wh // p, ww // p)

    @torch.no_grad()
    def predict(self, img):
        """(B, 3, H, W) -> (B, H, W) uint8 labels (class 0 = background when with_bg); int16 with label_dtype=torch.int16: the
        rescaled entry at the identity size, which is by definition the network-size label map."""
        self._check_classes()
        if self.wide:
            src = _BatchImages(img, self.mode == "whole")
            return torch.stack(self._list_forward(src, src.sizes))
        return ops.seg_label_map(*self._batch_forward(img), self.with_bg, self.bg_thresh)[0]

    @torch.no_grad()
    def group_map(self, img):
        """(B, 3, H, W) -> (B, H, W) uint8: the group of every pixel (in its first covering window)."""
        return ops.seg_label_map(*self._batch_forward(img, classes=False), self.with_bg, self.bg_thresh, labels=False, groups=True)[1]

    @torch.no_grad()
    def encode_decode(self, img):
        """(B, 3, H, W) -> (B, N + with_bg, H, W) fp32 logits (vit_seg.py:202-256; any batch size)."""
        return ops.seg_logits(*self._batch_forward(img), self.with_bg, self.bg_thresh)

    # ------------------------------------------------------------------------------------------ images of mixed sizes
    def _image_rows(self, src, plan, win_off, out_shapes, with_gt):
        """The rows of ops.seg_image_table / seg_view_tables: one per entry, with its image's output size and ground-truth
        offset (the ground truths lie flat one after the other)."""
        p = self.model.clip.visual.patch_size
        rows, gt_off = [], 0
        for i, V in enumerate(src.view_counts):
            for e in range(len(rows), len(rows) + V):
                first, count, (wh, ww) = plan.entries[e]
                rows.append(dict(first=first, count=count, net=src.sizes[e], out=out_shapes[i], win=(wh, ww), grid=(wh // p, ww // p),
                                 soft_off=win_off[first], gt_off=gt_off if with_gt else -1, flags=src.flags[e]))
            gt_off += out_shapes[i][0] * out_shapes[i][1]
        return rows

    def _list_forward(self, src, out_shapes, gts=None, areas=None, ignore_index=255, reduce_zero_label=False, want_labels=True,
                      groups=None):
        """The list call without augmentation: the arg-max of the rescaled logits (segclip_seg_label_map_rescaled).
        groups: None, "also" (-> (labels, group maps, G), both at out_shapes, from the same pass of the tower) or "only"
        (-> (None, group maps, G): no class tables, no label map)."""
        out_shapes = _out_shapes(src, out_shapes)
        classes = groups != "only"
        if classes:
            self._check_classes()
        plan, dwin, _ = self._device_plan(src)
        if groups is not None:
            for i, count in enumerate(plan.image_windows):
                if count != 1:
                    raise ValueError(f"group maps are defined for one window per image: image {i} ({src.sizes[i][0]}x"
                                     f"{src.sizes[i][1]}) has {count} windows in slide mode")
        soft, tables, win_off, n_groups = self._list_towers(src, plan, dwin, classes)
        rows = self._image_rows(src, plan, win_off, out_shapes, gts is not None)
        images, offs, nbytes, n_blocks, most = ops.seg_image_table(rows, src.device)
        labels = None
        if classes:
            # the table's offsets count elements: it serves the 16-bit maps as it is
            labels = torch.empty(nbytes, dtype=self.label_dtype, device=src.device) if want_labels else None
            kernel = ops.seg_label_map_rescaled_wide if self.wide else ops.seg_label_map_rescaled
            kernel(soft, tables, dwin, images, n_blocks, most, self.with_bg, self.bg_thresh, labels=labels,
                   gt=_Maps.gapless_of(gts)[0], areas=areas, ignore_index=ignore_index, reduce_zero_label=reduce_zero_label)
            labels = None if labels is None else _Maps(labels, offs, out_shapes).views()
        if groups is None:
            return labels
        # the table's label offsets and workgroup numbers serve the group maps as they are: same sizes, same tile
        gmaps = ops.seg_groups_rescaled(soft, images, n_blocks, n_groups, torch.empty(nbytes, dtype=torch.uint8, device=src.device))
        return labels, _Maps(gmaps, offs, out_shapes).views(), n_groups

    def _sweep_forward(self, src, out_shapes, thresholds, gts=None, areas=None, ignore_index=255, reduce_zero_label=False,
                       want_labels=True):
        """_list_forward for every background threshold of a list at once (segclip_seg_label_map_rescaled_sweep): one pass of
        the towers, -> [(T, oh_i, ow_i) uint8 labels], views of one (T, bytes) buffer, or None."""
        out_shapes = _out_shapes(src, out_shapes)
        self._check_classes()
        plan, dwin, _ = self._device_plan(src)
        soft, tables, win_off, _ = self._list_towers(src, plan, dwin)
        rows = self._image_rows(src, plan, win_off, out_shapes, gts is not None)
        images, offs, nbytes, n_blocks, most = ops.seg_image_table(rows, src.device)
        labels = torch.empty(len(thresholds), nbytes, dtype=torch.uint8, device=src.device) if want_labels else None
        ops.seg_label_map_sweep(soft, tables, dwin, images, n_blocks, most, thresholds, labels=labels, gt=_Maps.gapless_of(gts)[0],
                                areas=areas, ignore_index=ignore_index, reduce_zero_label=reduce_zero_label)
        if labels is None:
            return None
        return [labels[:, o:o + oh * ow].view(-1, oh, ow) for o, (oh, ow) in zip(offs, out_shapes)]

    def _views_forward(self, src, out_shapes, gts=None, areas=None, ignore_index=255, reduce_zero_label=False, want_labels=True,
                       dense=False):
        """The augmented list call: the mean over an image's views of the soft-max of the rescaled logits, its first maximum
        (segclip_seg_label_map_views).  dense: -> the (C, oh, ow) fp32 mean probabilities of the single image instead."""
        out_shapes = _out_shapes(src, out_shapes)
        self._check_classes()
        if dense and len(out_shapes) != 1:
            raise ValueError(f"the dense probabilities are formed for one image per call, got {len(out_shapes)}")
        plan, dwin, _ = self._device_plan(src)
        soft, tables, win_off, _ = self._list_towers(src, plan, dwin)
        rows = self._image_rows(src, plan, win_off, out_shapes, gts is not None)
        images, vtab, offs, nbytes, *limits = ops.seg_view_tables(rows, src.view_counts, src.device)
        args = (soft, tables, dwin, images, vtab, *limits, self.with_bg, self.bg_thresh)
        if dense:
            return ops.seg_view_probs(*args, out_shapes[0])
        labels = torch.empty(nbytes, dtype=torch.uint8, device=src.device) if want_labels else None
        ops.seg_label_map_views(*args, labels=labels, gt=_Maps.gapless_of(gts)[0], areas=areas, ignore_index=ignore_index,
                                reduce_zero_label=reduce_zero_label)
        return None if labels is None else _Maps(labels, offs, out_shapes).views()

    def _post_process(self, src, out_shapes, refine=None, clean=None, score=None, want_labels=True, snap=None):
        """The chain of every list entry point that returns or scores label maps: labels -> refine (a PAMR, against
        src.pictures) -> snap (a Snap, against src.pictures) -> clean (a Despeckle) -> the mIoU areas -> the boundary areas -> the
        confusion matrix -> the per-image areas.  score: None, or the _Score of an
        evaluator's call; the areas are those of the maps that leave the chain, counted once (`counts`), by

            refine   snap   clean       the mIoU areas are counted by
            -        -      -           the label kernel
            PAMR     -      -           the refinement's last kernel; the label kernel only writes the maps
            any      Snap   -           ops.seg_areas on the snapped maps, laid gapless; nothing earlier counts
            any      any    Despeckle   ops.seg_areas on the cleaned maps, gapless; nothing earlier counts

        and with score.boundary one more ops.seg_boundary call on the same maps adds to score.boundary_areas, with
        score.confusion one ops.seg_confusion call on them, laid gapless, to that matrix, with score.per_image one
        ops.seg_image_areas call on them, where they lie, whose (B, 3, C) rows are appended to that list.  The labels are
        formed whenever a later stage reads them, wanted or not.  -> the final maps, or None when they are not wanted."""
        forward = self._views_forward if src.augmented else self._list_forward
        counts = (None if score is None else "clean" if clean is not None else "snap" if snap is not None else
                  "refine" if refine is not None else "labels")
        counting = {} if score is None else dict(gts=score.gts, areas=score.areas, **score.rule)
        reads_labels = score is not None and (score.boundary is not None or score.confusion is not None or score.per_image is not None)
        first = dict(counting, want_labels=want_labels or reads_labels) if counts == "labels" else {}
        labels = forward(src, out_shapes, **first)
        if refine is not None:
            labels = _refine_maps(src.pictures, labels, self.num_classes, src.transform, refine, **(counting if counts == "refine" else {}))
        if snap is not None:
            snapped = _snap_stage(src.pictures, labels, self.num_classes, snap)
            labels = snapped.views()
            if counts == "snap":
                ops.seg_areas(snapped.gapless(), _Maps.gapless_of(score.gts)[0], self.num_classes, areas=score.areas, **score.rule)
        if clean is not None:
            cleaned = _despeckle_maps(labels, clean)
            labels = cleaned.views()
            if counts == "clean":
                ops.seg_areas(cleaned.gapless(), _Maps.gapless_of(score.gts)[0], self.num_classes, areas=score.areas, **score.rule)
        if score is not None and score.boundary is not None:
            _boundary_call(_Maps.of(labels), score.boundary, gts=score.gts, num_classes=self.num_classes, areas=score.boundary_areas,
                           **score.rule)
        if score is not None and score.confusion is not None:
            ops.seg_confusion(_Maps.of(labels).gapless(), _Maps.gapless_of(score.gts)[0], self.num_classes, conf=score.confusion,
                              **score.rule)
        if score is not None and score.per_image is not None:
            score.per_image.append(_image_areas_call(_Maps.of(labels), score.gts, self.num_classes, **score.rule))
        return labels if want_labels else None

    @torch.no_grad()
    def predict_list(self, imgs, out_shapes=None, refine=None, clean=None, snap=None):
        """[(3, H_i, W_i)] of any mix of sizes -> [(oh_i, ow_i) uint8 labels], views of one flat buffer; out_shapes defaults
        to the images' own sizes.  The logits are rescaled bilinearly (align_corners=False) to the output size and the first
        maximum taken there, as mmseg's resize(size=ori_shape) + arg-max, inside one kernel launch for the whole list.
        Slide mode: the windows of all images go through encode_image max_windows at a time; whole mode: one call per size.
        refine and snap are refused: there is no raw picture here (predict_raw has it); clean too: despeckle the maps."""
        _refuse("predict_list", ("refine", refine, "needs the decoded pictures: use predict_raw(refine=) or refine_labels"),
                ("snap", snap, "needs the decoded pictures: use predict_raw(snap=) or snap_labels"),
                ("clean", clean, "is not supported; apply despeckle to the maps it returns"))
        return self._list_forward(_SlicedImages([[(t, 0)] for t in imgs]), out_shapes)

    @torch.no_grad()
    def predict_raw(self, raws, transform, out_shapes=None, net_sizes=None, aug=None, refine=None, clean=None, snap=None):
        """[(h_i, w_i, 3) uint8 decoded images] -> [(oh_i, ow_i) uint8 labels] as predict_list(preprocess(raws, transform,
        net_sizes), out_shapes), bit for bit, without the resized images: the windows of a tower call are written from the
        raw bytes by one launch of segclip_seg_windows_from_u8.  out_shapes defaults to the raw images' own sizes (mmseg's
        ori_shape); net_sizes overrides transform.net_size (whole mode needs multiples of the patch size).
        aug (a TestAug): mmseg's aug_test over the views of aug.views - every view segmented, its logits rescaled to the output
        size and passed through a soft-max, flipped back, the probabilities averaged over the views, first maximum.  net_sizes
        then holds one (H, W) per view of every image.
        refine (a PAMR): the label maps pass through the pixel-adaptive refinement against the raw pictures before they are
        returned, = refine_labels(raws, predict_raw(raws, ...), num_classes, transform, refine) bit for bit.  out_shapes must
        then be the raw sizes (the default).  It composes with aug: the refinement sees only labels.
        snap (a Snap): the maps, after the refinement if there is one, are snapped to the superpixels of the raw pictures,
        = snap_labels(predict_raw(raws, ...), superpixels(raws, snap.superpixels), num_classes, min_share=snap.min_share) bit
        for bit.  out_shapes must then be the raw sizes (the default).
        clean (a Despeckle): the maps, after the refinement and the snapping if there are any, are despeckled before they are
        returned, = despeckle(predict_raw(raws, ...), ...) bit for bit.
        With label_dtype=torch.int16 the maps are int16, and aug, refine, snap and clean are refused (snap_labels and despeckle
        take the int16 maps this returns)."""
        self._refuse_wide("predict_raw", aug=aug, refine=refine, snap=snap, clean=clean)
        _check_stages(refine, clean, raws, out_shapes, snap)
        return self._post_process(_RawImages(raws, transform, net_sizes, aug), out_shapes, refine, clean, snap=snap)

    @torch.no_grad()
    def predict_views(self, views, out_shapes):
        """views[i] = [((3, H, W) tensor, flags)]: the views of image i, pre-processed and ALREADY FLIPPED as mmseg hands imgs
        and img_metas to aug_test (flags: ops.SEG_FLIP_H | ops.SEG_FLIP_V, what img_metas' flip / flip_direction say)
        -> [(oh_i, ow_i) uint8 labels] of the mean probabilities, as predict_raw(aug=)."""
        self._refuse_wide("predict_views", predict_views=views)
        return self._views_forward(_SlicedImages(views, augmented=True), out_shapes)

    @torch.no_grad()
    def predict_proba_views(self, views, out_shape):
        """The views [((3, H, W) tensor, flags)] of ONE image -> (N + with_bg, oh, ow) fp32: the mean over the views of the
        soft-max of the rescaled logits, what aug_test takes the arg-max of (predict_views' label is its first maximum)."""
        return self._views_forward(_SlicedImages([views], augmented=True), [out_shape], dense=True)

    @torch.no_grad()
    def predict_proba_raw(self, raw, transform, aug=None, out_shape=None, net_sizes=None):
        """predict_proba_views from ONE decoded (h, w, 3) uint8 image; aug defaults to the single unflipped view, out_shape to
        the image's own size."""
        src = _RawImages([raw], transform, None if net_sizes is None else [net_sizes], TestAug() if aug is None else aug)
        return self._views_forward(src, None if out_shape is None else [out_shape], dense=True)

    # ------------------------------------------------------------------------------------------ the demo's outputs
    @torch.no_grad()
    def groups_list(self, imgs, out_shapes=None):
        """[(3, H_i, W_i)] -> [(oh_i, ow_i) uint8 group maps], views of one flat buffer: the soft assignment resized to the
        network size and again to the output size, first maximum over the groups (get_attn_maps + show_result's group
        branch, vit_seg.py:144-200, :359-362), one launch for the list.  out_shapes defaults to the images' own sizes, where
        the result equals group_map's.  Every image is one window: a slide-mode image with more raises ValueError."""
        return self._list_forward(_SlicedImages([[(t, 0)] for t in imgs]), out_shapes, groups="only")[1]

    @torch.no_grad()
    def groups_raw(self, raws, transform, out_shapes=None, net_sizes=None):
        """groups_list from decoded (h_i, w_i, 3) uint8 images, as predict_raw; out_shapes defaults to the raw sizes."""
        return self._list_forward(_RawImages(raws, transform, net_sizes), out_shapes, groups="only")[1]

    @torch.no_grad()
    def render_raw(self, raws, transform, vis_modes, palette, group_palette=None, net_sizes=None, refine=None, clean=None,
                   snap=None):
        """The reference's --vis modes (show_result, vit_seg.py:286-377) for decoded images, at their own sizes -> dict
        mode -> result:
          input              the raws
          pred               [(h_i, w_i) uint8 label maps] (predict_raw's)
          input_pred         [(h_i, w_i, 3) uint8]: blend at opacity 0.8, background kept as it is when with_bg (:298)
          input_pred_label   (blend at opacity 0.6, anchors [[(label, y, x)]] without the background when with_bg) (:299-320)
          final_group, first_group   [(h_i, w_i, 3) uint8]: the group map blended at 0.6 with group_palette[:G] (:346-375)
          all_groups         the same as a one-element list per image: this model has one grouping stage
        palette: (P, 3) uint8 RGB class colours (index 0 = background when with_bg); group_palette defaults to
        default_group_palette(G).  Channel order of the pictures: transform.channel_order.  The vision tower runs once per
        call whatever the modes: labels and group maps come from the same encode_image pass.  refine is refused: draw refined
        maps with blend(raws, predict_raw(raws, transform, refine=...), palette).  snap and clean are refused in the same way."""
        self._refuse_wide("SegInference", render_raw=vis_modes)
        _refuse("render_raw", ("refine", refine, "is not supported; blend the maps of predict_raw(refine=) instead"),
                ("snap", snap, "is not supported; blend the maps of predict_raw(snap=) instead"),
                ("clean", clean, "is not supported; blend the maps of despeckle(predict_raw(...)) instead"))
        modes = list(vis_modes)
        for m in modes:
            if m not in VIS_MODES:
                raise ValueError(f"unknown vis mode {m!r}; known: {', '.join(VIS_MODES)}")
        want_labels = any(m in ("pred", "input_pred", "input_pred_label") for m in modes)
        want_groups = any(m in _GROUP_MODES for m in modes)
        src = _RawImages(raws, transform, net_sizes)
        palette = _check_palette(palette, src.device)
        labels = gmaps = None
        if want_groups:
            labels, gmaps, G = self._list_forward(src, None, want_labels=want_labels, groups="also" if want_labels else "only")
        elif want_labels:
            labels = self._list_forward(src, None)
        order = transform.channel_order
        out = {}
        for m in modes:
            if m in out:
                continue
            if m == "input":
                out[m] = list(raws)
            elif m == "pred":
                out[m] = labels
            elif m == "input_pred":
                out[m] = blend(raws, labels, palette, 0.8, skip_zero=self.with_bg, channel_order=order)
            elif m == "input_pred_label":
                imgs, sums = blend(raws, labels, palette, 0.6, skip_zero=self.with_bg, channel_order=order, anchors=True)
                marks = anchors_from_sums(sums.cpu())
                if self.with_bg:
                    marks = [[a for a in per if a[0] != 0] for per in marks]
                out[m] = (imgs, marks)
            else:
                if "_groups" not in out:
                    gp = default_group_palette(G) if group_palette is None else group_palette
                    gp = _check_palette(gp, src.device)
                    if gp.shape[0] < G:
                        raise ValueError(f"the group palette has {gp.shape[0]} colours for {G} groups")
                    out["_groups"] = blend(raws, gmaps, gp[:G], 0.6, channel_order=order)
                out[m] = [[t] for t in out["_groups"]] if m == "all_groups" else out["_groups"]
        out.pop("_groups", None)
        return out


VIS_MODES = ("input", "pred", "input_pred", "all_groups", "first_group", "final_group", "input_pred_label")
_GROUP_MODES = ("all_groups", "first_group", "final_group")


def default_group_palette(G):
    """(G, 3) uint8 RGB colours for group maps: evenly spaced hues at full saturation, two brightness levels in turn so
    that neighbouring hues stay apart.  (The reference's group_palette.txt is its data: a caller who wants it passes it.)"""
    G = int(G)
    if not 1 <= G <= 256:
        raise ValueError(f"a palette has 1 .. 256 colours, got {G}")
    rows = [[int(c * 255.0 + 0.5) for c in colorsys.hsv_to_rgb(i / G, 1.0, 1.0 if i % 2 == 0 else 0.65)] for i in range(G)]
    return torch.tensor(rows, dtype=torch.uint8)


def _check_palette(palette, device):
    """-> (P, 3) uint8 on `device`; a palette is a small host-side setting like the normalisation constants and may come from
    anywhere."""
    palette = torch.as_tensor(palette)
    if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= 256:
        raise ValueError(f"a palette is a (P <= 256, 3) uint8 tensor, got {palette.dtype} {tuple(palette.shape)}")
    return palette.to(device).contiguous()


@torch.no_grad()
def blend(raws, maps, palette, opacity=0.5, skip_zero=False, channel_order="rgb", anchors=False):
    """blend_result (vit_seg.py:258-284) for a list of pictures of mixed sizes in one launch: raws [(h_i, w_i, 3) uint8
    decoded images, rows possibly strided], maps [(h_i, w_i) uint8 palette indices: labels or groups], palette (P <= 256, 3)
    uint8 RGB -> [(h_i, w_i, 3) uint8] in the raws' channel order, views of one flat buffer.  Every byte is numpy's
    (img * (1 - opacity) + color * opacity).astype(uint8), computed in fp64 as numpy does; an index >= P is black; with
    skip_zero the pixels of index 0 stay as they are (the reference's with_bg).  anchors=True: also the (B, P, 3) int64
    device tensor of per-index pixel counts, sums of y and sums of x (anchors_from_sums turns it into positions)."""
    if channel_order not in ("rgb", "bgr"):
        raise ValueError(f"channel_order must be 'rgb' or 'bgr', got {channel_order!r}")
    opacity = float(opacity)
    if not 0.0 < opacity <= 1.0:
        raise ValueError(f"opacity lies in (0, 1], got {opacity}")
    _check_pictures(raws, maps, "an index map")
    dev = raws[0].device
    palette = _check_palette(palette, dev)
    batch = _Maps.of(maps)
    table, offs, nbytes, n_blocks = ops.seg_blend_table(list(raws), batch.offs)
    out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sums = torch.zeros(len(raws), palette.shape[0], 3, dtype=torch.int64, device=dev) if anchors else None
    ops.seg_blend(table, n_blocks, batch.flat, palette, opacity, out, skip_zero=skip_zero, reverse_channels=channel_order == "bgr",
                  sums=sums)
    imgs = [out[o:o + 3 * t.shape[0] * t.shape[1]].view(t.shape[0], t.shape[1], 3) for o, t in zip(offs, raws)]
    return (imgs, sums) if anchors else imgs


def anchors_from_sums(sums):
    """The (B, P, 3) sums of blend(anchors=True), copied to the host -> per image [(index, y, x)] for the indices present:
    y = int(sum_y / count), x = int(sum_x / count) in fp64 = seg2coord(...)[index].astype(np.int32) (vit_seg.py:100-115,
    :320), where the label text is anchored."""
    if sums.is_cuda:
        raise ValueError("anchors_from_sums takes a CPU copy of the sums (sums.cpu())")
    if sums.dim() != 3 or sums.shape[2] != 3 or sums.dtype != torch.int64:
        raise ValueError(f"sums is a (B, P, 3) int64 tensor, got {sums.dtype} {tuple(sums.shape)}")
    out = []
    for per in sums.tolist():
        out.append([(i, int(sy / n), int(sx / n)) for i, (n, sy, sx) in enumerate(per) if n > 0])
    return out


class SegEvaluator:
    """mmseg's mIoU evaluation on the device.  update() adds every image's per-class intersection, prediction area and label
    area (intersect_and_union with ignore_index / reduce_zero_label) to `areas`, a (3, C) int64 device tensor, inside the
    label-map launch and without a host synchronisation; compute() copies it to the host once.  Several ranks: all_reduce
    `areas` (sum) before compute().
    boundary (a Boundary): every update path also scores the labels whose areas it counts - the refined or cleaned ones -
    against the ground truths with one more call (segclip_seg_boundary) that adds to `boundary_areas`, a (2, 3, C) int64
    device tensor (slot 0 Boundary IoU, slot 1 trimap); the labels are then formed even when return_labels is False, and
    compute() adds bIoU, mbIoU, trimap_IoU, trimap_mIoU and trimap_aAcc from the same host copy.  Several ranks: all_reduce
    `boundary_areas` like `areas`.  Without it nothing changes.
    confusion (True): every update path also counts the labels whose areas it counts against the ground truths with one more
    call (segclip_seg_confusion, or its 16-bit entry) that adds to `confusion`, a (C + 1, C + 1) int64 device tensor: row =
    ground-truth class, column = predicted class, index C the out-of-range bin, the ground-truth rule that of `areas`, which
    is a projection of it (areas_from_confusion).  The labels are then formed even when return_labels is False, and
    compute() adds confusion, Dice, Precision, Recall, Fscore, mDice, mFscore, fwIoU and kappa from the same host copy.
    Several ranks: all_reduce `confusion` (sum) like `areas`.  Without it nothing changes.
    per_image (True): every update path also counts the labels whose areas it counts - the refined, snapped or cleaned ones,
    exactly as confusion=True sees them - picture by picture with one more call (segclip_seg_image_areas, or its 16-bit
    entry): one (3, C) row per picture, kept as a list of per-call device tensors.  `image_areas` is their concatenation,
    (n, 3, C) int64, in the order the pictures were given ((0, 3, C) before any update; reset() clears it), and its sum over
    the pictures is `areas`.  The labels are then formed even when return_labels is False, no update synchronises with the
    host, and compute() adds image_mIoU, mIoU_I, IoU_C, mIoU_C, mIoU_I_q and mIoU_C_q (fine_grained_from_image_areas, reduced
    on the device).  Several ranks: the rows are CONCATENATED - all_gather `image_areas`, never all_reduce it - and the
    figures taken from the gathered tensor with the static functions.  Without it nothing changes.
    Over a SegInference with label_dtype=torch.int16 the ground truths are (oh, ow) torch.int16 tensors whose elements are read
    as unsigned 16-bit values (a loader's uint16 array goes in as .view(torch.int16)), ignore_index is an integer in
    0 .. 65535 compared with that value, and boundary= is refused (boundary_areas takes the int16 maps that update_raw returns);
    confusion= works there too.
    update_maps(preds, gts) scores label maps that exist already, of either width, without the towers."""

    def __init__(self, seg, ignore_index=255, reduce_zero_label=False, boundary=None, confusion=False, per_image=False):
        self.gt_dtype = getattr(seg, "label_dtype", torch.uint8)
        if self.gt_dtype == torch.int16:
            _refuse("SegEvaluator", ("boundary", boundary, "is not built for 16-bit label maps (label_dtype=torch.int16)"))
            if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or not 0 <= ignore_index <= 65535:
                raise ValueError(f"SegEvaluator: with 16-bit label maps ignore_index is an integer in 0 .. 65535, got {ignore_index!r}")
        if boundary is not None:
            _check_boundary(boundary)
        self.seg, self.ignore_index, self.reduce_zero_label = seg, int(ignore_index), bool(reduce_zero_label)
        self.areas = torch.zeros(3, seg.num_classes, dtype=torch.int64, device=seg.text_embedding.device)
        self.boundary, self.boundary_areas = boundary, None
        if boundary is not None:
            self.boundary_areas = torch.zeros(2, 3, seg.num_classes, dtype=torch.int64, device=self.areas.device)
        self.confusion = None
        if confusion:
            self.confusion = torch.zeros(seg.num_classes + 1, seg.num_classes + 1, dtype=torch.int64, device=self.areas.device)
        self._image_rows = [] if per_image else None   # one (B, 3, C) device tensor per update call

    @property
    def image_areas(self):
        """(n, 3, C) int64 on the device: one row per picture seen, in the order given; None without per_image=True."""
        if self._image_rows is None:
            return None
        if len(self._image_rows) > 1:   # kept as one tensor from here on
            self._image_rows = [torch.cat(self._image_rows)]
        return self._image_rows[0] if self._image_rows else self.areas.new_zeros(0, 3, self.areas.shape[1])

    def reset(self):
        self.areas.zero_()
        if self.boundary_areas is not None:
            self.boundary_areas.zero_()
        if self.confusion is not None:
            self.confusion.zero_()
        if self._image_rows is not None:
            self._image_rows.clear()

    def _score(self, gts):
        """-> (what the chain, SegInference._post_process, scores a call against; the ground truths' sizes, its out_shapes)"""
        rule = dict(ignore_index=self.ignore_index, reduce_zero_label=self.reduce_zero_label)
        return (_Score(list(gts), self.areas, rule, self.boundary, self.boundary_areas, self.confusion, self._image_rows),
                [tuple(g.shape) for g in gts])

    @torch.no_grad()
    def update(self, imgs, gts, return_labels=False, refine=None, clean=None, snap=None):
        """imgs [(3, H_i, W_i)], gts [(oh_i, ow_i) uint8]: the labels are formed at each ground truth's size.  refine and snap
        are refused: there is no raw picture here (update_raw has it); clean is refused too (update_raw has it)."""
        _refuse("SegEvaluator.update", ("refine", refine, "needs the decoded pictures: use update_raw(refine=)"),
                ("snap", snap, "needs the decoded pictures: use update_raw(snap=)"),
                ("clean", clean, "is not supported; use update_raw(clean=), or despeckle the maps and score them with ops.seg_areas"))
        self._check_gts(imgs, gts, self.gt_dtype)
        score, shapes = self._score(gts)
        return self.seg._post_process(_SlicedImages([[(t, 0)] for t in imgs]), shapes, score=score, want_labels=return_labels)

    @torch.no_grad()
    def update_raw(self, raws, gts, transform, return_labels=False, net_sizes=None, aug=None, refine=None, clean=None, snap=None):
        """raws [(h_i, w_i, 3) uint8 decoded images] instead of pre-processed ones, as SegInference.predict_raw (aug included).
        refine (a PAMR): the areas are those of the refined label maps, added by the refinement's last kernel; the label
        kernel then only writes the maps and counts nothing.  The ground truths must have the pictures' sizes.
        snap (a Snap): the labels are formed (and refined) without counting, snapped to the pictures' superpixels, and
        ops.seg_areas of the snapped maps against the ground truths is added.  The ground truths must have the pictures' sizes.
        clean (a Despeckle): the labels are formed (and refined, and snapped) without counting, despeckled, and ops.seg_areas of
        the cleaned maps against the ground truths is added: the areas are those of the cleaned maps."""
        self.seg._refuse_wide("SegEvaluator.update_raw", aug=aug, refine=refine, snap=snap, clean=clean)
        self._check_gts(raws, gts, self.gt_dtype)
        score, shapes = self._score(gts)
        _check_stages(refine, clean, raws, shapes, snap)
        return self.seg._post_process(_RawImages(raws, transform, net_sizes, aug), shapes, refine, clean, score, return_labels, snap=snap)

    @torch.no_grad()
    def update_maps(self, preds, gts):
        """Scores label maps that exist already - refined elsewhere, read from disk, or what despeckle returned: preds
        [(oh_i, ow_i) maps of the evaluator's label dtype, uint8 or int16], gts [the ground truths, of the same dtype and sizes].
        Adds to `areas` (ops.seg_areas / ops.seg_areas_wide), with confusion=True to `confusion`, with per_image=True one row
        per map to `image_areas`, and on a uint8 evaluator with boundary= to `boundary_areas`: exactly what update / update_raw count for the same maps.  It is how a 16-bit evaluator
        scores despeckled maps, whose in-pipeline stage (update_raw(clean=)) stays refused.  No towers, no host
        synchronisation.  -> None."""
        preds, gts = list(preds), list(gts)
        word = "int16" if self.gt_dtype == torch.int16 else "uint8"
        if len(preds) == 0:
            raise ValueError("SegEvaluator.update_maps: empty list of label maps")
        if len(preds) != len(gts):
            raise ValueError(f"SegEvaluator.update_maps: {len(preds)} label maps but {len(gts)} ground truths")
        ops.L.require_cuda(*preds)
        self._check_gts(preds, gts, self.gt_dtype)
        for i, (p, g) in enumerate(zip(preds, gts)):
            if p.dtype != self.gt_dtype or p.dim() != 2 or p.numel() == 0:
                raise ValueError(f"SegEvaluator.update_maps: label map {i} is a non-empty (oh, ow) {word} tensor (the evaluator's "
                                 f"label dtype), got {p.dtype} {tuple(p.shape)}")
            if tuple(p.shape) != tuple(g.shape):
                raise ValueError(f"SegEvaluator.update_maps: label map {i} has its ground truth's size {tuple(g.shape)}, got "
                                 f"{tuple(p.shape)}")
        batch = _Maps.of(preds)
        flat, gt = batch.gapless(), _Maps.gapless_of(gts)[0]
        C = self.seg.num_classes
        rule = dict(ignore_index=self.ignore_index, reduce_zero_label=self.reduce_zero_label)
        (ops.seg_areas_wide if self.gt_dtype == torch.int16 else ops.seg_areas)(flat, gt, C, areas=self.areas, **rule)
        if self.boundary is not None:
            _boundary_call(batch, self.boundary, gts=gts, num_classes=C, areas=self.boundary_areas, **rule)
        if self.confusion is not None:
            ops.seg_confusion(flat, gt, C, conf=self.confusion, **rule)
        if self._image_rows is not None:
            self._image_rows.append(_image_areas_call(batch, gts, C, **rule))

    @torch.no_grad()
    def update_views(self, views, gts, return_labels=False):
        """views[i] = [((3, H, W) tensor, flags)] as SegInference.predict_views, scored at each ground truth's size."""
        self.seg._refuse_wide("SegEvaluator", update_views=views)
        self._check_gts(views, gts)
        score, shapes = self._score(gts)
        return self.seg._post_process(_SlicedImages(views, augmented=True), shapes, score=score, want_labels=return_labels)

    @staticmethod
    def _check_gts(imgs, gts, dtype=torch.uint8):
        """dtype: torch.uint8, or torch.int16 for an evaluator over 16-bit label maps"""
        if len(imgs) != len(gts):
            raise ValueError(f"{len(imgs)} images but {len(gts)} ground truths")
        ops.L.require_cuda(*gts)
        want = "int16 tensor (label_dtype=torch.int16; a uint16 array goes in as .view(torch.int16))" if dtype == torch.int16 \
            else "uint8 tensor"
        for g in gts:
            if g.dtype != dtype or g.dim() != 2:
                raise ValueError(f"a ground truth is an (oh, ow) {want}, got {g.dtype} {tuple(g.shape)}")

    @staticmethod
    def boundary_metrics_from_areas(areas):
        """(2, 3, C) integer CPU tensor (boundary_areas) -> dict(bIoU, mbIoU, trimap_IoU, trimap_mIoU, trimap_aAcc), each slot
        as metrics_from_areas treats `areas`: IoU = I / (P + L - I) per class, a class absent from both sides of a slot is NaN
        and left out of its mean, trimap_aAcc = sum(I) / sum(L) of the trimap."""
        if areas.dim() != 3 or tuple(areas.shape[:2]) != (2, 3):
            raise ValueError(f"areas is a (2, 3, C) tensor, got {tuple(areas.shape)}")
        a = areas.to(torch.float64)
        biou = a[0, 0] / (a[0, 1] + a[0, 2] - a[0, 0])
        tiou = a[1, 0] / (a[1, 1] + a[1, 2] - a[1, 0])
        return dict(bIoU=biou, mbIoU=float(torch.nanmean(biou)), trimap_IoU=tiou, trimap_mIoU=float(torch.nanmean(tiou)),
                    trimap_aAcc=float(a[1, 0].sum() / a[1, 2].sum()))

    @staticmethod
    def metrics_from_areas(areas):
        """(3, C) integer CPU tensor -> dict(mIoU, aAcc, mAcc, IoU, Acc) as mmseg's eval_metrics: IoU = I / (P + L - I),
        Acc = I / L, aAcc = sum(I) / sum(L); a class absent from prediction and label is NaN and left out of the means."""
        a = areas.to(torch.float64)
        inter, pred, label = a[0], a[1], a[2]
        iou, acc = inter / (pred + label - inter), inter / label
        return dict(mIoU=float(torch.nanmean(iou)), aAcc=float(inter.sum() / label.sum()), mAcc=float(torch.nanmean(acc)),
                    IoU=iou, Acc=acc)

    @staticmethod
    def _check_confusion(conf):
        if conf.dim() != 2 or conf.shape[0] != conf.shape[1] or conf.shape[0] < 2 or conf.is_floating_point():
            raise ValueError(f"conf is a (C + 1, C + 1) integer tensor, got {conf.dtype} {tuple(conf.shape)}")
        return conf.to(torch.int64)

    @staticmethod
    def areas_from_confusion(conf):
        """(C + 1, C + 1) integer CPU tensor (`confusion`) -> the (3, C) int64 `areas` of the same pixels: the diagonal, the
        column sums over all rows and the row sums over all columns, the out-of-range bins included in the sums."""
        conf = SegEvaluator._check_confusion(conf)
        C = conf.shape[0] - 1
        return torch.stack([conf.diagonal()[:C], conf.sum(0)[:C], conf.sum(1)[:C]])

    @staticmethod
    def confusion_metrics(conf):
        """(C + 1, C + 1) integer CPU tensor -> dict, with I, P, L = areas_from_confusion(conf) in fp64:
        Dice = 2 I / (P + L), Precision = I / P, Recall = I / L, Fscore = 2 Precision Recall / (Precision + Recall) (mmseg's
        f_score with beta = 1) per class, NaN for a class absent from prediction and label; mDice and mFscore their means
        over the other classes (as mmseg's nanmean; a class with I = 0 on one side only has an undefined Fscore and is left
        out of mFscore too); fwIoU = sum(L IoU) / sum(L) over the classes with L > 0; kappa = (po - pe) / (1 - pe) over the
        WHOLE matrix, the out-of-range bins being one more class on either axis: po = trace / total,
        pe = sum(row sums x column sums) / total^2; and confusion, the int64 matrix itself."""
        conf = SegEvaluator._check_confusion(conf)
        a = SegEvaluator.areas_from_confusion(conf).to(torch.float64)
        inter, pred, label = a[0], a[1], a[2]
        dice = 2.0 * inter / (pred + label)
        precision, recall = inter / pred, inter / label
        fscore = 2.0 * precision * recall / (precision + recall)
        iou = inter / (pred + label - inter)
        seen = label > 0
        fw = float((label[seen] * iou[seen]).sum() / label.sum())
        m = conf.to(torch.float64)
        total = m.sum()
        po, pe = m.diagonal().sum() / total, (m.sum(1) * m.sum(0)).sum() / (total * total)
        return dict(confusion=conf, Dice=dice, Precision=precision, Recall=recall, Fscore=fscore, mDice=float(torch.nanmean(dice)),
                    mFscore=float(torch.nanmean(fscore)), fwIoU=fw, kappa=float((po - pe) / (1.0 - pe)))

    @staticmethod
    def confused_pairs(conf, k, names=None):
        """The k largest off-diagonal cells among the first C rows and columns of a (C + 1, C + 1) integer CPU tensor, empty
        cells left out -> [(gt, pred, count, share)], share = count / the ground-truth class's pixels (its row sum, the
        out-of-range column included), ordered by falling count and then by rising (gt, pred); with `names` (C strings) the
        two classes are given by name."""
        conf = SegEvaluator._check_confusion(conf)
        C = conf.shape[0] - 1
        if names is not None and len(names) != C:
            raise ValueError(f"names holds {len(names)} entries for {C} classes")
        inner = conf[:C, :C].clone()
        inner.fill_diagonal_(0)
        rows = conf.sum(1).tolist()
        cells = [(-v, i // C, i % C) for i, v in enumerate(inner.reshape(-1).tolist()) if v > 0]
        out = []
        for neg, g, p in sorted(cells)[:max(int(k), 0)]:
            out.append((g if names is None else names[g], p if names is None else names[p], -neg, -neg / rows[g]))
        return out

    @staticmethod
    def merge_classes(conf, mapping):
        """The matrix "if these names were one class": mapping[c] in 0 .. M - 1 is the new class of class c (C entries, every new
        class used at least once) -> the (M + 1, M + 1) int64 matrix whose cell (a, b) sums the cells of the classes mapped
        to a and b; the out-of-range bins are carried over as bin M."""
        conf = SegEvaluator._check_confusion(conf)
        C = conf.shape[0] - 1
        mapping = [int(v) for v in mapping]
        if len(mapping) != C or min(mapping) < 0 or sorted(set(mapping)) != list(range(max(mapping) + 1)):
            raise ValueError(f"mapping holds one new class id per class ({C}), the ids 0 .. M - 1 all used")
        M = max(mapping) + 1
        idx = torch.tensor(mapping + [M], dtype=torch.int64)
        rows = torch.zeros(M + 1, C + 1, dtype=torch.int64).index_add_(0, idx, conf)
        return torch.zeros(M + 1, M + 1, dtype=torch.int64).index_add_(1, idx, rows)

    @staticmethod
    def _check_image_areas(image_areas):
        if not isinstance(image_areas, torch.Tensor) or image_areas.dim() != 3 or image_areas.shape[1] != 3 \
                or image_areas.is_floating_point() or image_areas.is_complex() or image_areas.dtype == torch.bool:
            got = f"{image_areas.dtype} {tuple(image_areas.shape)}" if isinstance(image_areas, torch.Tensor) else repr(type(image_areas))
            raise ValueError(f"image_areas is an (n, 3, C) integer tensor, got {got}")
        return image_areas

    @staticmethod
    def _check_quantiles(quantiles):
        qs = [float(q) for q in quantiles]
        for q in qs:
            if not 0.0 < q <= 1.0:   # NaN fails too
                raise ValueError(f"a quantile q lies in (0, 1], got {q!r}")
        return qs

    @staticmethod
    def _lowest_means(values, qs):
        """values (m_max, K) fp64 with NaN for "no value": per column the mean of its max(1, ceil(q * m)) lowest values, m the
        column's count of values -> [(K,) per q], NaN for a column without a value.  Tensor arithmetic only: no host copy."""
        n = values.shape[0]
        have = ~torch.isnan(values)
        m = have.sum(0)
        if n == 0:
            return [torch.full_like(m, float("nan"), dtype=torch.float64) for _ in qs]
        ordered = torch.sort(values, dim=0).values   # NaN sorts last
        sums = torch.cumsum(torch.nan_to_num(ordered, nan=0.0), dim=0)
        out = []
        for q in qs:
            k = torch.ceil(q * m.to(torch.float64)).to(torch.int64).clamp_(min=1)
            mean = sums.gather(0, (k - 1).clamp_(max=n - 1).unsqueeze(0))[0] / k.to(torch.float64)
            out.append(torch.where(m > 0, mean, torch.full_like(mean, float("nan"))))
        return out

    @staticmethod
    def _fine_grained(image_areas, qs):
        """The figures of fine_grained_from_image_areas as fp64 tensors on the tensor's device:
        -> (image_mIoU (n,), IoU_C (C,), scalars (2 + 2 len(qs),) = mIoU_I, mIoU_C, mIoU_I_q..., mIoU_C_q...)."""
        a = image_areas.to(torch.float64)
        inter, pred, label = a[:, 0], a[:, 1], a[:, 2]
        union = pred + label - inter
        nan = torch.full_like(union, float("nan"))
        iou = torch.where(union > 0, inter / union, nan)
        per_image = torch.nanmean(iou, dim=1)
        in_class = torch.where(label > 0, iou, nan)   # L > 0 implies U > 0
        # the plain means are the means of the lowest 100 %: mIoU_I_q[1.0] == mIoU_I and mIoU_C_q[1.0] == mIoU_C bit for bit
        low_i = SegEvaluator._lowest_means(per_image.unsqueeze(1), [1.0] + qs)
        low_c = SegEvaluator._lowest_means(in_class, [1.0] + qs)
        per_class = low_c[0]
        scalars = [v[0] for v in low_i[:1]] + [torch.nanmean(per_class)] + [v[0] for v in low_i[1:]] + [torch.nanmean(v) for v in low_c[1:]]
        return per_image, per_class, torch.stack(scalars)

    @staticmethod
    def _fine_grained_dict(per_image, per_class, scalars, qs):
        s = scalars.tolist()
        return dict(image_mIoU=per_image, mIoU_I=s[0], IoU_C=per_class, mIoU_C=s[1],
                    mIoU_I_q={q: s[2 + i] for i, q in enumerate(qs)}, mIoU_C_q={q: s[2 + len(qs) + i] for i, q in enumerate(qs)})

    @staticmethod
    def fine_grained_from_image_areas(image_areas, quantiles=(0.05, 0.1)):
        """(n, 3, C) integer tensor (`image_areas`), on the CPU or on a device -> dict of the fine-grained mIoU figures, in fp64.
        Per picture i and class c, with I, P, L the picture's areas: U = P + L - I and iou[i, c] = I / U where U > 0, else NaN.
            image_mIoU  (n,) fp64 CPU tensor: the mean of iou[i] over the classes with a value; NaN for a picture with no class
                        on either side (all its pixels ignored).  A class that is predicted but not labelled counts, as 0.
            mIoU_I      the mean of image_mIoU over the pictures with a score
            IoU_C       (C,) fp64 CPU tensor: for class c the mean of iou[i, c] over the pictures with L[i, c] > 0 - those that
                        contain the class; NaN where there is none
            mIoU_C      the mean of IoU_C over the classes with a value
            mIoU_I_q    {q: the mean of the max(1, ceil(q * m)) lowest of the m picture scores}: the worst q of the pictures
            mIoU_C_q    {q: per class the mean of the max(1, ceil(q * m_c)) lowest of its m_c values, then the mean over the
                        classes with a value}
        q lies in (0, 1]; q = 1 gives mIoU_I and mIoU_C.  The data-set mIoU (metrics_from_areas of the summed rows) is dominated
        by large objects and large pictures; these figures weigh every picture, or every picture of a class, alike.  The
        reduction runs where the tensor lies, and one small copy brings the figures to the host."""
        image_areas = SegEvaluator._check_image_areas(image_areas)
        qs = SegEvaluator._check_quantiles(quantiles)
        per_image, per_class, scalars = SegEvaluator._fine_grained(image_areas, qs)
        n, C = per_image.numel(), per_class.numel()
        host = torch.cat([per_image, per_class, scalars]).cpu()
        return SegEvaluator._fine_grained_dict(host[:n], host[n:n + C], host[n + C:], qs)

    @staticmethod
    def worst_images(image_areas, k):
        """(n, 3, C) integer tensor -> [(index, image_mIoU)] of the k pictures with the lowest score, by rising score and, among
        equal scores, rising index; pictures without a score (all pixels ignored) are left out."""
        scores = SegEvaluator.fine_grained_from_image_areas(image_areas, ())["image_mIoU"].tolist()
        ranked = sorted((s, i) for i, s in enumerate(scores) if not math.isnan(s))
        return [(i, s) for s, i in ranked[:max(int(k), 0)]]

    @staticmethod
    def bootstrap_miou(image_areas, n_boot=1000, alpha=0.05, seed=0):
        """A bootstrap over pictures of the data-set mIoU: (n, 3, C) integer tensor -> dict(lo, hi, std, replicates).  Replicate
        r draws n pictures with replacement, idx = torch.randint(0, n, (n_boot, n), generator=torch.Generator().manual_seed(
        seed)), sums their rows - formed for all replicates at once as the fp64 product of the (n_boot, n) matrix of draw
        counts with the (n, 3 C) areas, exact while the sums stay below 2^53 - and takes metrics_from_areas(...)["mIoU"] of
        the sum.  replicates: (n_boot,) fp64; lo, hi: torch.quantile of them at alpha / 2 and 1 - alpha / 2; std: their
        standard deviation (one less than their number in the denominator; 0 for a single one).  A replicate that drew only
        pictures whose pixels are all ignored has no mIoU: it stays NaN in `replicates` and is left out of lo, hi and std.
        Runs on a CPU copy; the same seed gives the same interval."""
        image_areas = SegEvaluator._check_image_areas(image_areas)
        n, _, C = image_areas.shape
        n_boot = int(n_boot)
        if n < 1 or n_boot < 1:
            raise ValueError(f"bootstrap_miou needs at least one picture and one replicate, got n = {n} and n_boot = {n_boot}")
        if not 0.0 < float(alpha) < 1.0:
            raise ValueError(f"alpha lies in (0, 1), got {alpha!r}")
        rows = image_areas.cpu().to(torch.float64).reshape(n, 3 * C)
        idx = torch.randint(0, n, (n_boot, n), generator=torch.Generator().manual_seed(int(seed)))
        draws = torch.zeros(n_boot, n, dtype=torch.float64).scatter_add_(1, idx, torch.ones(n_boot, n, dtype=torch.float64))
        sums = (draws @ rows).view(n_boot, 3, C)
        replicates = torch.tensor([SegEvaluator.metrics_from_areas(s)["mIoU"] for s in sums], dtype=torch.float64)
        scored = replicates[~torch.isnan(replicates)]   # a replicate that drew all-ignored pictures only has no mIoU
        if scored.numel() == 0:
            return dict(lo=float("nan"), hi=float("nan"), std=float("nan"), replicates=replicates)
        lo, hi = torch.quantile(scored, torch.tensor([alpha / 2.0, 1.0 - alpha / 2.0], dtype=torch.float64)).tolist()
        return dict(lo=lo, hi=hi, std=float(scored.std()) if scored.numel() > 1 else 0.0, replicates=replicates)

    def compute(self, quantiles=(0.05, 0.1)):
        """quantiles: the q of mIoU_I_q and mIoU_C_q, read with per_image=True only."""
        parts = [self.areas.reshape(-1)]
        if self.boundary is not None:
            parts.append(self.boundary_areas.reshape(-1))
        if self.confusion is not None:
            parts.append(self.confusion.reshape(-1))
        fine = None
        if self._image_rows is not None:   # reduced on the device; the figures go to the host beside the areas
            qs = self._check_quantiles(quantiles)
            fine = self._fine_grained(self.image_areas, qs)
        if len(parts) == 1:
            out = self.metrics_from_areas(self.areas.cpu())
        else:
            C = self.areas.shape[1]
            host = torch.cat(parts).cpu()  # the one host copy
            out = self.metrics_from_areas(host[:3 * C].view(3, C))
            if self.boundary is not None:
                out.update(self.boundary_metrics_from_areas(host[3 * C:9 * C].view(2, 3, C)))
            if self.confusion is not None:
                out.update(self.confusion_metrics(host[-(C + 1) * (C + 1):].view(C + 1, C + 1)))
        if fine is not None:
            n, C = fine[0].numel(), fine[1].numel()
            host = torch.cat(fine).cpu()
            out.update(self._fine_grained_dict(host[:n], host[n:n + C], host[n + C:], qs))
        return out


def check_thresholds(thresholds):
    """The background thresholds of a sweep -> a list of floats: 1 .. ops.SEG_MAX_THRESHOLDS finite values, strictly increasing
    (the kernel's switch index needs the order; a duplicate would only repeat a slice)."""
    try:
        thr = [float(v) for v in thresholds]
    except TypeError:
        raise ValueError(f"thresholds is a sequence of numbers, got {thresholds!r}") from None
    if len(thr) < 1:
        raise ValueError("thresholds is empty")
    if len(thr) > ops.SEG_MAX_THRESHOLDS:
        raise ValueError(f"thresholds has {len(thr)} values, at most {ops.SEG_MAX_THRESHOLDS} per sweep (split the list)")
    # what the kernel compares is the fp32 value: two numbers that round to one float are duplicates
    thr = torch.tensor(thr, dtype=torch.float64).float().tolist()
    if any(not math.isfinite(v) for v in thr):
        raise ValueError(f"thresholds must be finite, got {thr}")
    for a, b in zip(thr, thr[1:]):
        if b == a:
            raise ValueError(f"thresholds holds the duplicate {a} (as fp32)")
        if b < a:
            raise ValueError(f"thresholds must be sorted in ascending order, got {b} after {a}")
    return thr


class SegSweepEvaluator:
    """SegEvaluator for a list of background thresholds in ONE pass: towers, front end and group tables run once per update,
    and the fused kernel (csrc/segment_sweep.inc) adds every image's areas to `areas`, a (T, 3, C) int64 device tensor whose
    slice t is, integer for integer, the `areas` of SegEvaluator(SegInference(..., bg_thresh=thresholds[t])).  For tuning
    bg_thresh on a new dataset or checkpoint (the reference's configurations use 0.80, 0.25 and 0.65).

    seg.bg_thresh is IGNORED here: the thresholds of the list take its place.  seg must have with_bg=True (without a background
    class there is no threshold).  Not covered: test-time augmentation (aug= raises: the augmented path takes a soft-max that
    includes the background logit, so it would need accumulators per threshold), the dense logits, more than 16 thresholds per
    sweep (split the list over two evaluators) and a sweep of the top-5 mask."""

    def __init__(self, seg, thresholds, ignore_index=255, reduce_zero_label=False):
        if getattr(seg, "wide", False):
            raise ValueError("SegSweepEvaluator is not built for 16-bit label maps (label_dtype=torch.int16); use one SegEvaluator "
                             "per threshold")
        if not seg.with_bg:
            raise ValueError("SegSweepEvaluator: seg must have with_bg=True (the threshold decides the background class)")
        self.thresholds = check_thresholds(thresholds)
        self.seg, self.ignore_index, self.reduce_zero_label = seg, int(ignore_index), bool(reduce_zero_label)
        self.areas = torch.zeros(len(self.thresholds), 3, seg.num_classes, dtype=torch.int64, device=seg.text_embedding.device)

    def reset(self):
        self.areas.zero_()

    @torch.no_grad()
    def update(self, imgs, gts, return_labels=False):
        """As SegEvaluator.update; with return_labels one (T, oh_i, ow_i) uint8 tensor per image."""
        SegEvaluator._check_gts(imgs, gts)
        return self._forward(_SlicedImages([[(t, 0)] for t in imgs]), gts, return_labels)

    @torch.no_grad()
    def update_raw(self, raws, gts, transform, return_labels=False, net_sizes=None, aug=None, refine=None, clean=None, snap=None):
        """As SegEvaluator.update_raw, without aug, without refine, without snap and without clean."""
        _refuse("SegSweepEvaluator",
                ("snap", snap, "is not supported (every threshold's map would need its own vote); use one SegEvaluator per "
                               "threshold (update_raw(snap=))"),
                ("clean", clean, "is not supported (every threshold's map would need its own pass); despeckle the maps of one "
                                 "SegEvaluator per threshold (update_raw(clean=))"),
                ("refine", refine, "is not supported (every threshold's map would need its own refinement); use one SegEvaluator "
                                   "per threshold"),
                ("aug", aug, "is not supported (the augmented path needs accumulators per threshold); use one SegEvaluator per "
                             "threshold"))
        SegEvaluator._check_gts(raws, gts)
        return self._forward(_RawImages(raws, transform, net_sizes), gts, return_labels)

    def _forward(self, src, gts, return_labels):
        return self.seg._sweep_forward(src, [tuple(g.shape) for g in gts], self.thresholds, gts=list(gts), areas=self.areas,
                                       ignore_index=self.ignore_index, reduce_zero_label=self.reduce_zero_label,
                                       want_labels=return_labels)

    @staticmethod
    def sweep_from_areas(areas, thresholds):
        """(T, 3, C) integer CPU tensor -> dict(thresholds, metrics [SegEvaluator.metrics_from_areas per threshold],
        best=(index, threshold, mIoU)): the highest mIoU, the lowest threshold among equal ones (a NaN mIoU never wins)."""
        thr = [float(v) for v in thresholds]
        if areas.dim() != 3 or areas.shape[0] != len(thr) or areas.shape[1] != 3:
            raise ValueError(f"areas is a (T, 3, C) tensor for {len(thr)} thresholds, got {tuple(areas.shape)}")
        metrics = [SegEvaluator.metrics_from_areas(a) for a in areas]
        best = 0
        for t, m in enumerate(metrics):
            if m["mIoU"] > metrics[best]["mIoU"] or (math.isnan(metrics[best]["mIoU"]) and not math.isnan(m["mIoU"])):
                best = t
        return dict(thresholds=thr, metrics=metrics, best=(best, thr[best], metrics[best]["mIoU"]))

    def compute(self):
        return self.sweep_from_areas(self.areas.cpu(), self.thresholds)
