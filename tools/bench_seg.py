"""Zero-shot segmentation inference (segclip_amd.segmentation), ViT-B/16 synthetic weights, bf16 towers:
  (i)   images/s of SegInference.predict, B = 64 at 224^2, mode "whole"
  (ii)  images/s of SegInference.predict, B = 16 at 448 x 672, mode "slide", the VOC settings (crop = stride = 224,
        20 classes + background, bg_thresh 0.80)
  (iii) for both: the post-processing alone - the three HIP kernels against an eager-torch transcription of the same
        post-processing (written here from tests/seg_reference.py's statement of the math, on the GPU in fp32) on top of
        the SAME encode_image outputs, so the ratio isolates the post-processing.
Every figure: 3 warm-up calls, then `reps` timed repeats of `inner` calls each, device-synchronised; median and min-max of
the repeats.  The shader clock the box held during the timed region is sampled (tools/clock_sampler.py).
The lines are printed and written to `out`.
With --eval instead: the mIoU evaluation of 64 images of mixed VOC-like sizes (21 classes, slide 224 / 224):
  (iv)  images/s of SegEvaluator.update (one call for the list), the time of segclip_seg_label_map_rescaled alone, the time of
        the Python-side window extraction (torch.stack of slices) alone, peak allocation, and the same evaluation done the
        obvious way on the same GPU: encode_decode per image -> F.interpolate -> argmax -> three histc, batch 1.
With --raw instead: the same 64 images as decoded uint8 (h, w, 3) tensors, in ONE command and alternating within every repeat:
  (v)   images/s of SegEvaluator.update_raw (the fused front-end kernel), of segmentation.preprocess + update (the same kernel
        writing the resized images, then torch.stack of slices), and of an eager-torch front end + update (per image a float
        copy, F.interpolate, normalise; then the slices); the front-end kernel's own time from a separate
        `rocprofv3 --kernel-trace --stats` child (--raw-child: five update_raw calls and nothing else) and its bytes per second
        against the HBM peak.
With --aug instead: the same 64 decoded images under test-time augmentation, TestAug(img_ratios=(1.0, 1.5), flip=True) = four
views per image, in ONE command and alternating within every repeat:
  (vi)  images/s of SegEvaluator.update_raw(aug=) (every window of every view through shared tower calls, then one
        segclip_seg_label_map_views launch) and of the eager composition from this library's public pieces (preprocess per view;
        per image and view a flip, encode_decode at batch 1, F.interpolate to the ground truth's size, soft-max, flip back, sum;
        arg-max of the mean; three histc), the areas of the two, peak allocation, and the multi-view kernel's and the view front
        end's own time from a separate `rocprofv3 --kernel-trace --stats` child (--aug-child: five update_raw(aug=) calls and
        nothing else).
With --sweep instead: the same 64 decoded images and a list of 8 background thresholds, in ONE command and alternating within
every repeat:
  (vii) one SegEvaluator.update_raw (the yardstick: the single evaluation, unchanged by the sweep), one
        SegSweepEvaluator.update_raw with the 8 thresholds, and 8 single update_raw calls (one evaluator per threshold): medians,
        spread, the ratios sweep / single and (8 singles) / sweep, peak allocation, the clock held, whether the 8 area slices equal
        the 8 single runs, and the sweep kernel's own time from a separate `rocprofv3 --kernel-trace --stats` child
        (--sweep-child: five sweep and five single update_raw calls and nothing else), beside the single entry's own time.  The
        thresholds are quantiles of the inputs' own best_score: synthetic weights score far below the reference's 0.25-0.80, where
        every threshold is clamped by table_max and all slices are one.
With --refine instead: the same 64 decoded images with pixel-adaptive refinement of the label maps, PAMR() = 10 iterations at
dilations (8, 16), in ONE command and alternating within every repeat:
  (viii) one SegEvaluator.update_raw (the yardstick: unchanged by the refinement), one update_raw(refine=PAMR()), and update_raw's
        label maps refined by an eager fp32 transcription of the definition (replicate pad + F.unfold on the (C, h, w) one-hot,
        per image) and scored by segclip_seg_areas: medians, spread, the refinement's cost over the yardstick both ways and their
        ratio, the share of pixels on which the two agree, peak allocation, the clock held, and the refinement kernels' own time
        from a separate `rocprofv3 --kernel-trace --stats` child (--refine-child: five update_raw(refine=) calls and nothing
        else) with the step kernel's bytes per second against its design traffic.
With --objects instead: the label maps that update_raw forms for the same 64 decoded images, and their connected components
(segmentation.components / despeckle, csrc/segment_objects.inc), in ONE command and alternating within every repeat:
  (ix)  segclip_seg_components with every output (ids, area_px, records, count, cleaned) without a host copy, components() with
        its one host synchronisation, despeckle alone, one SegEvaluator.update_raw (the yardstick: unchanged by the feature), one
        update_raw(clean=Despeckle(16)), and the host route on the same maps: .cpu(), then scipy.ndimage.label per present class
        (without scipy: the numpy restatement of the tests on 4 maps, scaled to 64); then one 500 x 500 map that is one component,
        one 4-connected checkerboard (250 000 components) and one of 3-label noise, every output each: whether the atomics on one
        root or the chains of the merge dominate; and the kernels' own times from a separate `rocprofv3 --kernel-trace --stats`
        child (--objects-child: five calls with every output on the 64 maps and nothing else).
With --boundary instead: the boundary metrics (SegEvaluator(boundary=), csrc/segment_boundary.inc) on the inputs of --raw, in
ONE command and alternating within every repeat:
  (x)   one SegEvaluator.update_raw (the yardstick: the code path without the feature), one update_raw of an evaluator with
        boundary=Boundary(), segclip_seg_boundary alone on update_raw's label maps (areas only, and with both bands written),
        and the host route on the same maps: .cpu(), then scipy.ndimage.binary_erosion per present class of prediction and
        ground truth, then counting (without scipy: unmeasured); peak allocation, the clock held, the run-to-run spread, and the
        kernels' own times from a separate `rocprofv3 --kernel-trace --stats` child (--boundary-child: five calls with every
        output on the 64 maps and nothing else).
With --wide instead: the 16-bit label-map kernel (segclip_seg_label_map_rescaled_wide, csrc/segment_wide.inc) on the inputs of
--eval (64 images of mixed VOC-like sizes, slide 224 / 224, 12.0 M output pixels) with random int16 ground truths, the arguments
of one SegEvaluator.update captured, in ONE command and alternating within every repeat:
  (xi)  at 21 and 151 classes the wide kernel against the uint8 kernel on the same inputs (what the 16-bit path costs where both
        apply), labels and areas compared; at 460 and 848 classes the wide kernel against the composition a user had before it -
        ops.seg_logits per image, F.interpolate to the output size, argmax, three bincounts - with the peak allocation of both,
        and at every class count against two more builds of csrc/segment.hip (made on the spot with hipcc when they are missing):
        -DSEG_WIDE_LANE_SCAN=1, in which every lane scans the classes of its own undecided pixels as the uint8 kernel does, and
        -DSEG_WIDE_LANE_SCAN_CLASSES=0, the wave-cooperative scan at every class count (the kernel switches from the first to
        the second above 32 classes); labels and areas compared.
With --merge instead: despeckling by merging (despeckle(merge=True), csrc/segment_sieve.inc) on the label maps of --objects, in
ONE command and alternating within every repeat:
  (xii) despeckle(min_area=16) as shipped (the yardstick: the fill mode, the same kernels as before the feature), despeckle(...,
        merge=True) at rounds 1 and 2, one SegEvaluator.update_raw and one update_raw(clean=Despeckle(16, merge=True)), and the
        host route on the same maps: .cpu(), scipy.ndimage.label per class and a dilation per small component (without scipy:
        unmeasured); the share of labels each mode changes, the clock held, the run-to-run spread; then one 500 x 500 map that is
        one component, one 4-connected checkerboard (orphans only) and 3-label noise under both connectivities (most pixels
        vote), fill mode against one and two rounds each; and the kernels' own times from a
        separate `rocprofv3 --kernel-trace --stats` child (--merge-child: five one-round calls on the 64 maps and nothing else)
        with the vote and final kernels' bytes per second against their design traffic.
With --confusion instead: the confusion matrix of label maps (ops.seg_confusion, csrc/segment_confusion.inc) on the label maps
that SegEvaluator.update forms for the inputs of --eval (64 images of mixed VOC-like sizes, 12.0 M pixels) at 21 and 151 classes
(uint8 maps) and 460 and 848 classes (int16 maps), in ONE command and alternating within every repeat:
  (xiii) ops.seg_confusion against two yardsticks: the route a user had before it - the ground-truth rule in torch, g * (C + 1) + p
        as int64, torch.bincount - with its peak allocation, and ops.seg_areas / seg_areas_wide, which reads the same bytes and is
        the floor the kernel should sit near; the matrices of the first two compared, the identity with the areas checked.  Three
        inputs per class count: the label maps against themselves shifted by (3, 2) pixels with 40 rectangles per image
        relabelled (piecewise constant, as annotations are), the label maps against independent random labels, and random labels
        on both sides (at 460 and 848 classes more distinct pairs than the sparse table has slots: its overflow path).  Medians,
        spread, the clock held, the route, bytes per second against the HBM peak.
With --wide-post instead: the post-processing of 16-bit label maps (components, despeckle, boundary_areas on int16 maps: the
uint16_t instantiations of csrc/segment_objects.inc, segment_sieve.inc and segment_boundary.inc) on the 64 label maps of
--objects and on their int16 copies - the values are below 256, so both widths give the same result, which is checked - in ONE
command and alternating within every repeat:
  (xiv) components(), despeckle(min_area=16) in fill mode and with merge=True, and boundary_areas against update_raw's ground
        truths, each on the uint8 maps (the yardstick of its int16 twin) and on the int16 copies: medians, min-max, the ratio
        int16 / uint8 of every call, the clock held, and the kernels' own times by instantiation from a separate
        `rocprofv3 --kernel-trace --stats` child (--wide-post-child: five calls of each on both widths and nothing else).
        The output file keeps whatever stands above the line "# ---- tools/bench_seg.py --wide-post" (the kernels' resource
        tables) and replaces what follows it.
With --snap instead: superpixels and majority voting (superpixels, snap_labels, update_raw(snap=); csrc/segment_superpixel.inc
and segment_vote.inc) on the inputs of --raw (64 decoded images of mixed VOC-like sizes, 12.0 M pixels, 21 classes), in ONE
command and alternating within every repeat:
  (xv)  update_raw (the path without the stage: the yardstick), update_raw(snap=Snap()), superpixels alone and snap_labels alone
        on update_raw's label maps: medians, min-max, the clock held, the peak allocation of the two stand-alone calls, the
        share of the labels the stage moves, the host route (the numpy restatement of tests/superpixel_reference.py on .cpu()
        copies of 8 maps, scaled to 64), and the new kernels' own times from a separate `rocprofv3 --kernel-trace --stats`
        child (--snap-child: five calls of superpixels and snap_labels and nothing else) against their design traffic
        (DESIGN.md section 4).
With --per-image instead: the per-image areas (segmentation.image_areas, SegEvaluator(per_image=True);
csrc/segment_image_areas.inc) on the 64 label maps of --objects (12.0 M pixels, views of update_raw's label buffer, read where
they lie) at 21 and 151 classes and on their int16 copies, in the same layout, at 21, 151, 460 and 848 classes, against
two ground truths - update_raw's per-pixel noise, which leaves the run-length counting nothing to merge, and the maps shifted
by (3, 2) pixels with a band ignored, piecewise constant as annotations are - in ONE command and alternating within every repeat:
  (xvi) one image_areas call (checks, the ground truths laid gapless, the table copy, one launch), ops.seg_image_areas alone on the
        same buffers with the table made beforehand, and the only device means there was before: one ops.seg_areas /
        seg_areas_wide call per picture into the rows of a (B, 3, C) tensor; the three results compared; then one
        SegEvaluator.update_raw (the path without the feature: the yardstick) and one update_raw of an evaluator with
        per_image=True.  Medians, min-max, the clock held, bytes per second of the launch alone against the HBM peak, and
        whether the single call is slower than the loop outside the two ways' own min-max.  The output file keeps whatever
        stands above the line "# ---- tools/bench_seg.py --per-image" (the kernels' resources, the tile measurements).
usage: python tools/bench_seg.py [--eval | --raw | --aug | --sweep | --refine | --objects | --boundary | --wide | --merge | --confusion |
                                  --wide-post | --snap | --per-image]
                                 [reps=7] [out=profiles/seg_infer.txt | seg_eval.txt | seg_frontend.txt | seg_aug.txt | seg_sweep.txt |
                                  seg_refine.txt | seg_objects.txt | seg_boundary.txt | seg_wide.txt | seg_merge.txt | seg_confusion.txt |
                                  seg_wide_post.txt | seg_snap.txt | seg_per_image.txt]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import segclip_amd
from segclip_amd import config, ops, synth
from segclip_amd.segmentation import SegInference, _BatchImages
from tools.clock_sampler import ClockSampler

EVAL, RAW, RAW_CHILD = ("--eval" in sys.argv[1:]), ("--raw" in sys.argv[1:]), ("--raw-child" in sys.argv[1:])
AUG, AUG_CHILD = ("--aug" in sys.argv[1:]), ("--aug-child" in sys.argv[1:])
SWEEP, SWEEP_CHILD = ("--sweep" in sys.argv[1:]), ("--sweep-child" in sys.argv[1:])
REFINE, REFINE_CHILD = ("--refine" in sys.argv[1:]), ("--refine-child" in sys.argv[1:])
OBJECTS, OBJECTS_CHILD = ("--objects" in sys.argv[1:]), ("--objects-child" in sys.argv[1:])
BOUNDARY, BOUNDARY_CHILD = ("--boundary" in sys.argv[1:]), ("--boundary-child" in sys.argv[1:])
WIDE = "--wide" in sys.argv[1:]
MERGE, MERGE_CHILD = ("--merge" in sys.argv[1:]), ("--merge-child" in sys.argv[1:])
CONFUSION = "--confusion" in sys.argv[1:]
WIDE_POST, WIDE_POST_CHILD = ("--wide-post" in sys.argv[1:]), ("--wide-post-child" in sys.argv[1:])
WIDE_POST_MARK = "# ---- tools/bench_seg.py --wide-post"
SNAP, SNAP_CHILD = ("--snap" in sys.argv[1:]), ("--snap-child" in sys.argv[1:])
PER_IMAGE = "--per-image" in sys.argv[1:]
PER_IMAGE_MARK = "# ---- tools/bench_seg.py --per-image"
ARGV = [a for a in sys.argv[1:] if a not in ("--eval", "--raw", "--raw-child", "--aug", "--aug-child", "--sweep", "--sweep-child",
                                             "--refine", "--refine-child", "--objects", "--objects-child", "--boundary",
                                             "--boundary-child", "--wide", "--merge", "--merge-child", "--confusion", "--wide-post",
                                             "--wide-post-child", "--snap", "--snap-child", "--per-image")]
REPS = int(ARGV[0]) if len(ARGV) > 0 else 7
OUT = ARGV[1] if len(ARGV) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                 "seg_per_image.txt" if PER_IMAGE else "seg_snap.txt" if SNAP else "seg_wide_post.txt" if WIDE_POST else "seg_confusion.txt" if CONFUSION else "seg_merge.txt" if MERGE else "seg_wide.txt" if WIDE else "seg_boundary.txt" if BOUNDARY else "seg_objects.txt" if OBJECTS else "seg_refine.txt" if REFINE else "seg_sweep.txt" if SWEEP else "seg_aug.txt" if AUG else "seg_frontend.txt" if RAW else
                                                 "seg_eval.txt" if EVAL else "seg_infer.txt")
HBM_PEAK = 8.0e12   # bytes / s, MI355X specification
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, inner):
    with torch.no_grad():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / inner)
    return statistics.median(ts), min(ts), max(ts)


def eager_post(soft, hidden, feat, text, logit_scale, wins, out_size, win, grid, with_bg, bg_thresh):
    """The reference's formulation per window (upsampled soft assignment, one-hot, product with the table, logit volume,
    .item() for the background threshold) and mmseg's slide accumulation, as eager torch on the GPU."""
    B, H, W = out_size
    wh, ww = win
    N = text.shape[0]
    off = int(with_bg)
    preds = soft.new_zeros(B, N + off, H, W)
    count = soft.new_zeros(B, 1, H, W)
    scale = logit_scale.exp().clamp(max=100)
    for k, (b, y0, x0) in enumerate(wins):
        attn = F.interpolate(soft[k].view(1, -1, *grid), size=(wh, ww), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
        onehot = F.one_hot(attn.argmax(dim=-1), num_classes=attn.shape[-1]).to(attn.dtype)
        gt, pf = F.normalize(hidden[k, 1:], dim=-1), F.normalize(feat[k:k + 1], dim=-1)
        aff = gt @ text.t() * scale
        pre = F.softmax(aff, dim=-1)
        avg = F.softmax(pf @ text.t() * scale, dim=-1)
        mask = torch.zeros_like(avg).scatter_(-1, avg.topk(min(5, N), dim=-1).indices, 1.0).bool()
        aff = F.softmax(aff.masked_fill(~mask, float("-inf")), dim=-1) * pre
        logits = soft.new_zeros(N + off, wh, ww)
        prod = onehot @ aff
        logits[off:] = prod.permute(2, 0, 1)
        if with_bg:
            thr = min(bg_thresh, aff.max().item())
            logits[0, prod.max(dim=-1).values < thr] = 1
        preds[b, :, y0:y0 + wh, x0:x0 + ww] += logits
        count[b, :, y0:y0 + wh, x0:x0 + ww] += 1
    return (preds / count).argmax(dim=1).to(torch.uint8)


def case(name, model, text, B, H, W, inner, **kw):
    seg = SegInference(model, text, True, bg_thresh=0.80, **kw)
    img = torch.randn(B, 3, H, W, device="cuda")
    sampler = ClockSampler().start()
    med, lo, hi = timed(lambda: seg.predict(img), inner)
    clk = sampler.stop()
    say(f"{name}: predict {med * 1e3:8.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f}; {REPS} x {inner} calls)  "
        f"{B / med:8.1f} images/s   clock {clk}")
    # the same encoder outputs for both post-processings
    wins, win = seg.window_list(B, H, W)
    with torch.no_grad(), config.scope(cross_mode="intended"):
        x = img if seg.mode == "whole" else torch.stack([img[b, :, y:y + win[0], x0:x0 + win[1]] for (b, y, x0) in wins])
        feat, hidden, mid = model.clip.encode_image(x, return_hidden=True)
    soft = mid["attns"][-1]["soft_attn"]
    _, dwin, dfirst = seg._device_plan(_BatchImages(img, seg.mode == "whole"), image_first=True)
    grid = (win[0] // 16, win[1] // 16)
    ls = model.clip.logit_scale.detach()

    def kernels():
        tables = ops.seg_group_table(hidden[:, 1:, :], feat, text, ls, min(5, text.shape[0]))
        return ops.seg_label_map(soft, tables, dwin, dfirst, (B, H, W), win, grid, True, 0.80)[0]

    def eager():
        return eager_post(soft, hidden, feat, text, ls, wins, (B, H, W), win, grid, True, 0.80)

    same = float((kernels() == eager()).float().mean())
    sampler = ClockSampler().start()
    k_med, k_lo, k_hi = timed(kernels, inner * 40)
    k_clk = sampler.stop()
    sampler = ClockSampler().start()
    e_med, e_lo, e_hi = timed(eager, 1)
    e_clk = sampler.stop()
    say(f"{name}: post-processing, {len(wins)} windows: HIP kernels {k_med * 1e6:9.1f} us (min {k_lo * 1e6:.1f}, max {k_hi * 1e6:.1f})   "
        f"eager torch {e_med * 1e6:10.1f} us (min {e_lo * 1e6:.1f}, max {e_hi * 1e6:.1f})   ratio {e_med / k_med:7.1f}x   "
        f"labels equal at {same:.6f} of the pixels")
    say(f"{name}: clock during the kernels' timing {k_clk}; during the eager timing {e_clk}")
    say(f"{name}: post-processing share of predict: kernels {k_med / med:.4f}, eager would be {e_med / (med - k_med + e_med):.4f}")


# original sizes of the evaluation leg (VOC-like), cycled; the network sizes are their test_size at img_scale (2048, 224)
EVAL_SIZES = [(375, 500), (500, 375), (281, 500), (333, 500), (500, 334), (366, 500), (500, 500), (442, 500)]


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def eval_case(model, text, n_images=64):
    from segclip_amd.segmentation import SegEvaluator, slide_windows, test_size
    name = f"(iv) eval   {n_images} mixed sizes"
    seg = SegInference(model, text, True, bg_thresh=0.80, mode="slide", crop_size=(224, 224), stride=(224, 224))
    C = seg.num_classes
    g = torch.Generator().manual_seed(1)
    outs = [EVAL_SIZES[i % len(EVAL_SIZES)] for i in range(n_images)]
    imgs = [torch.randn(3, *test_size(*o), generator=g).cuda() for o in outs]
    gts = [torch.randint(0, C, o, generator=g).to(torch.uint8).cuda() for o in outs]
    ev = SegEvaluator(seg)
    sampler = ClockSampler().start()
    med, lo, hi = timed(lambda: ev.update(imgs, gts), 2)
    clk = sampler.stop()
    wins = [(i, y, x) for i, t in enumerate(imgs) for (y, x) in slide_windows(t.shape[1], t.shape[2], (224, 224), (224, 224))]
    say(f"{name}: SegEvaluator.update {med * 1e3:8.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f}; {REPS} x 2 calls)  "
        f"{n_images / med:8.1f} images/s   {len(wins)} windows   clock {clk}")
    # the fused kernel alone, on the arguments of one update
    captured = {}
    real = ops.seg_label_map_rescaled

    def capture(*a, **k):
        captured["call"] = (a, k)
        return real(*a, **k)

    ops.seg_label_map_rescaled = capture
    try:
        with torch.no_grad():
            ev.update(imgs, gts)
    finally:
        ops.seg_label_map_rescaled = real
    a, k = captured["call"]
    sampler = ClockSampler().start()
    k_med, k_lo, k_hi = timed(lambda: real(*a, **k), 40)
    k_clk = sampler.stop()
    pixels = sum(o[0] * o[1] for o in outs)
    say(f"{name}: segclip_seg_label_map_rescaled + areas alone {k_med * 1e6:9.1f} us (min {k_lo * 1e6:.1f}, max {k_hi * 1e6:.1f}) for "
        f"{pixels} output pixels = {pixels / k_med / 1e9:.2f} Gpixel/s   clock {k_clk}   share of update {k_med / med:.4f}")
    s_med, s_lo, s_hi = timed(lambda: torch.stack([imgs[i][:, y:y + 224, x:x + 224] for (i, y, x) in wins]), 2)
    say(f"{name}: window extraction (torch.stack of {len(wins)} slices) alone {s_med * 1e3:8.2f} ms (min {s_lo * 1e3:.2f}, "
        f"max {s_hi * 1e3:.2f})   share of update {s_med / med:.4f}")

    def obvious():
        areas = torch.zeros(3, C, device="cuda")
        for img, gt in zip(imgs, gts):
            logits = seg.encode_decode(img[None])
            pred = F.interpolate(logits, size=tuple(gt.shape), mode="bilinear", align_corners=False).argmax(dim=1)[0]
            keep = gt != 255
            p, t = pred[keep].float(), gt[keep].float()
            areas[0] += torch.histc(p[p == t], bins=C, min=0, max=C - 1)
            areas[1] += torch.histc(p, bins=C, min=0, max=C - 1)
            areas[2] += torch.histc(t, bins=C, min=0, max=C - 1)
        return areas

    ev.reset()
    with torch.no_grad():
        ev.update(imgs, gts)
        ref = obvious()
    same = float((ev.areas.double() - ref.double()).abs().sum() / ref.double().sum())
    sampler = ClockSampler().start()
    o_med, o_lo, o_hi = timed(obvious, 1)
    o_clk = sampler.stop()
    say(f"{name}: the obvious way (encode_decode per image -> F.interpolate -> argmax -> 3 histc, batch 1) {o_med * 1e3:8.2f} ms "
        f"(min {o_lo * 1e3:.2f}, max {o_hi * 1e3:.2f})  {n_images / o_med:8.1f} images/s   ratio {o_med / med:6.2f}x   clock {o_clk}   "
        f"areas differ by {same:.2e} of their sum")
    say(f"{name}: peak allocation of one call: update {peak_of(lambda: ev.update(imgs, gts)) / 2**20:8.1f} MiB, the obvious way "
        f"{peak_of(obvious) / 2**20:8.1f} MiB")


def raw_inputs(seg, n_images=64):
    g = torch.Generator().manual_seed(1)
    outs = [EVAL_SIZES[i % len(EVAL_SIZES)] for i in range(n_images)]
    raws = [torch.randint(0, 256, (*o, 3), generator=g, dtype=torch.uint8).cuda() for o in outs]
    gts = [torch.randint(0, seg.num_classes, o, generator=g).to(torch.uint8).cuda() for o in outs]
    return raws, gts


def raw_case(model, text, n_images=64):
    from segclip_amd.segmentation import ImageTransform, SegEvaluator, preprocess
    from tools import rocprof_roofline as rr
    name = f"(v)  raw    {n_images} mixed sizes"
    seg = SegInference(model, text, True, bg_thresh=0.80, mode="slide", crop_size=(224, 224), stride=(224, 224))
    tf = ImageTransform()
    raws, gts = raw_inputs(seg, n_images)
    ev = SegEvaluator(seg)
    mean = torch.tensor(tf.mean, device="cuda")[:, None, None]
    std = torch.tensor(tf.std, device="cuda")[:, None, None]

    def eager_front():
        return [(F.interpolate(r.permute(2, 0, 1)[None].float(), size=tf.net_size(r.shape[0], r.shape[1]), mode="bilinear",
                               align_corners=False)[0] - mean) / std for r in raws]

    ways = [("update_raw", lambda: ev.update_raw(raws, gts, tf)),
            ("preprocess + update", lambda: ev.update(preprocess(raws, tf), gts)),
            ("eager front end + update", lambda: ev.update(eager_front(), gts))]
    with torch.no_grad():
        areas = []
        for _, fn in ways:   # warm-up, and the three ways' areas
            ev.reset()
            fn()
            areas.append(ev.areas.clone())
            fn()
        torch.cuda.synchronize()
        ts = [[] for _ in ways]
        sampler = ClockSampler().start()
        for _ in range(REPS):   # alternating: every repeat times the three ways one after the other
            for k, (_, fn) in enumerate(ways):
                t0 = time.perf_counter()
                fn()
                fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) / 2)
        clk = sampler.stop()
    meds = [statistics.median(t) for t in ts]
    for (what, _), t, med in zip(ways, ts, meds):
        say(f"{name}: {what:26s} {med * 1e3:8.2f} ms (min {min(t) * 1e3:.2f}, max {max(t) * 1e3:.2f}; {REPS} x 2 calls)  "
            f"{n_images / med:8.1f} images/s")
    spread = max((max(t) - min(t)) / statistics.median(t) for t in ts[:2])
    say(f"{name}: update_raw / (preprocess + update) {meds[0] / meds[1]:.4f}, update_raw / (eager front end + update) "
        f"{meds[0] / meds[2]:.4f}; run-to-run spread of the first two {spread:.4f} of the median; clock {clk}")
    same = float((areas[0] - areas[2]).abs().sum()) / float(areas[2].sum())
    say(f"{name}: areas of update_raw and preprocess + update equal: {bool(torch.equal(areas[0], areas[1]))}; against the eager "
        f"front end (ATen's fp32 coordinates) they differ by {same:.2e} of their sum")
    # the kernel's bytes, from the arguments of one update_raw
    captured = {}
    real = ops.seg_windows_from_u8

    def capture(*a, **k):
        out = real(*a, **k)
        captured["written"] = captured.get("written", 0) + out.numel() * 4
        return out

    ops.seg_windows_from_u8 = capture
    try:
        with torch.no_grad():
            ev.update_raw(raws, gts, tf)
    finally:
        ops.seg_windows_from_u8 = real
    written, source = captured["written"], sum(r.numel() for r in raws)
    # its own time: a child of this tool that only calls update_raw, under rocprofv3 --kernel-trace --stats
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        try:
            rc, _, err = rr.run_child([os.path.abspath(__file__), "--raw-child"], tmp)
            db = rr.find_db(tmp)
            rows = [r for r in rr.kernel_table(db) if "seg_front_kernel" in r[0]] if rc == 0 and db else []
        except Exception as e:   # no rocprofv3 on the box
            rc, err, rows = -1, repr(e), []
    if rows:
        _, calls, total_us, avg_us = rows[0]
        say(f"{name}: segclip_seg_windows_from_u8 alone (rocprofv3 --kernel-trace --stats, {calls} launches) {avg_us:8.1f} us per launch: "
            f"{written} bytes written, {source} source bytes = {written / avg_us / 1e6:.3f} TB/s written "
            f"({written / avg_us * 1e6 / HBM_PEAK:.3f} of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak), {(written + source) / avg_us / 1e6:.3f} TB/s "
            f"with the source read once; share of update_raw {avg_us * 1e-6 / meds[0]:.5f}")
    else:
        say(f"{name}: segclip_seg_windows_from_u8 alone: unmeasured (rocprofv3 child rc={rc}: {err[-200:]})")


def raw_child(model, text):
    """Five update_raw calls and nothing else: what the rocprofv3 child of raw_case traces."""
    from segclip_amd.segmentation import ImageTransform, SegEvaluator
    seg = SegInference(model, text, True, bg_thresh=0.80, mode="slide", crop_size=(224, 224), stride=(224, 224))
    raws, gts = raw_inputs(seg)
    ev = SegEvaluator(seg)
    with torch.no_grad():
        for _ in range(5):
            ev.update_raw(raws, gts, ImageTransform())
    torch.cuda.synchronize()


AUG_RATIOS = (1.0, 1.5)   # 375 x 500 -> views of 224 x 299 (2 windows) and 336 x 448 (4 windows), each unflipped and flipped


def aug_case(model, text, n_images=64):
    from segclip_amd.segmentation import ImageTransform, SegEvaluator, TestAug, preprocess, slide_windows
    from tools import rocprof_roofline as rr
    name = f"(vi) aug    {n_images} mixed sizes"
    seg = SegInference(model, text, True, bg_thresh=0.80, mode="slide", crop_size=(224, 224), stride=(224, 224))
    C = seg.num_classes
    tf, aug = ImageTransform(), TestAug(img_ratios=AUG_RATIOS, flip=True)
    raws, gts = raw_inputs(seg, n_images)
    ev = SegEvaluator(seg)
    views = [aug.views(int(r.shape[0]), int(r.shape[1]), tf) for r in raws]
    V = len(views[0])
    n_win = sum(len(slide_windows(H, W, (224, 224), (224, 224))) for per in views for (H, W, _) in per)
    pixels = sum(int(g.numel()) for g in gts)

    def eager():
        """What a user writes today: mmseg's aug_test from preprocess, encode_decode and eager torch."""
        areas = torch.zeros(3, C, device="cuda")
        nets = [preprocess(raws, tf, net_sizes=[per[v][:2] for per in views]) for v in range(V)]
        for i, gt in enumerate(gts):
            total = None
            for v in range(V):
                flags = views[i][v][2]
                dims = [d for d, bit in ((2, ops.SEG_FLIP_H), (1, ops.SEG_FLIP_V)) if flags & bit]   # of a (3, H, W) image
                x = nets[v][i].flip(dims) if dims else nets[v][i]
                logits = seg.encode_decode(x[None])
                p = F.softmax(F.interpolate(logits, size=tuple(gt.shape), mode="bilinear", align_corners=False), dim=1)
                if dims:
                    p = p.flip([d + 1 for d in dims])
                total = p if total is None else total + p
            pred = (total / V).argmax(dim=1)[0]
            keep = gt != 255
            q, t = pred[keep].float(), gt[keep].float()
            areas[0] += torch.histc(q[q == t], bins=C, min=0, max=C - 1)
            areas[1] += torch.histc(q, bins=C, min=0, max=C - 1)
            areas[2] += torch.histc(t, bins=C, min=0, max=C - 1)
        return areas

    def fused():
        ev.update_raw(raws, gts, tf, aug=aug)

    ways = [("update_raw(aug=)", fused, 2), ("eager composition", eager, 1)]   # (what, call, calls per timed repeat)
    with torch.no_grad():
        ev.reset()
        fused()
        a_fused = ev.areas.clone()
        a_eager = eager()
        fused()
        torch.cuda.synchronize()
        ts = [[] for _ in ways]
        sampler = ClockSampler().start()
        for _ in range(REPS):   # alternating: every repeat times the two ways one after the other
            for k, (_, fn, inner) in enumerate(ways):
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) / inner)
        clk = sampler.stop()
    say(f"{name}: {V} views per image (ratios {AUG_RATIOS} x flip), {n_win} windows, {pixels} output pixels, {C} classes")
    meds = [statistics.median(t) for t in ts]
    for (what, _, inner), t, med in zip(ways, ts, meds):
        say(f"{name}: {what:18s} {med * 1e3:9.2f} ms (min {min(t) * 1e3:.2f}, max {max(t) * 1e3:.2f}; {REPS} x {inner} calls)  "
            f"{n_images / med:8.1f} images/s")
    spread = max((max(t) - min(t)) / statistics.median(t) for t in ts)
    say(f"{name}: update_raw(aug=) / eager composition {meds[0] / meds[1]:.4f}; largest run-to-run spread {spread:.4f} of the median; "
        f"clock {clk}")
    same = float((a_fused.double() - a_eager.double()).abs().sum() / a_eager.double().sum())
    say(f"{name}: areas of the two differ by {same:.2e} of their sum (fp32 accumulation order and ATen's fp32 coordinates)")
    say(f"{name}: peak allocation of one call: update_raw(aug=) {peak_of(fused) / 2**20:8.1f} MiB, the eager composition "
        f"{peak_of(eager) / 2**20:8.1f} MiB")
    # the kernels' own time: a child of this tool that only calls update_raw(aug=), under rocprofv3 --kernel-trace --stats
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        try:
            rc, _, err = rr.run_child([os.path.abspath(__file__), "--aug-child"], tmp)
            db = rr.find_db(tmp)
            table = rr.kernel_table(db) if rc == 0 and db else []
        except Exception as e:   # no rocprofv3 on the box
            rc, err, table = -1, repr(e), []
    total_us = sum(r[2] for r in table)
    for what, pat in (("segclip_seg_label_map_views", "seg_views_kernel"), ("segclip_seg_view_windows_from_u8", "seg_front_kernel")):
        rows = [r for r in table if pat in r[0]]
        if not rows:
            say(f"{name}: {what} alone: unmeasured (rocprofv3 child rc={rc}: {err[-200:]})")
            continue
        calls, us = sum(r[1] for r in rows), sum(r[2] for r in rows)
        line = (f"{name}: {what} alone (rocprofv3 --kernel-trace --stats, {calls} launches) {us / calls:9.1f} us per launch, "
                f"{us / total_us:.4f} of the child's kernel time")
        if pat == "seg_views_kernel":
            avg = us / calls
            line += (f"; {avg * 1e-6 / meds[0]:.4f} of update_raw(aug=); {pixels / avg / 1e3:.3f} Gpixel/s = {avg * 1e3 / (pixels * V * C):.3f} ns "
                     f"per (pixel, view, class)")
        say(line)


def aug_child(model, text):
    """Five update_raw(aug=) calls and nothing else: what the rocprofv3 child of aug_case traces."""
    from segclip_amd.segmentation import ImageTransform, SegEvaluator, TestAug
    seg = SegInference(model, text, True, bg_thresh=0.80, mode="slide", crop_size=(224, 224), stride=(224, 224))
    raws, gts = raw_inputs(seg)
    ev = SegEvaluator(seg)
    with torch.no_grad():
        for _ in range(5):
            ev.update_raw(raws, gts, ImageTransform(), aug=TestAug(img_ratios=AUG_RATIOS, flip=True))
    torch.cuda.synchronize()


def sweep_thresholds(seg, raws, gts, tf, T=8):
    """T thresholds that decide something on synthetic weights, whose group scores lie far below the reference's 0.25-0.80 (every
    threshold of that range is clamped by table_max, and all T slices are one): the k / (T + 1) quantiles of the best_score of
    one pass over the inputs, rounded to fp32, duplicates dropped."""
    from segclip_amd.segmentation import SegEvaluator, check_thresholds
    captured = {}
    real = ops.seg_label_map_rescaled

    def capture(soft, tables, *a, **k):
        captured["score"] = tables[3].reshape(-1).clone()
        return real(soft, tables, *a, **k)

    ops.seg_label_map_rescaled = capture
    try:
        with torch.no_grad():
            SegEvaluator(seg).update_raw(raws, gts, tf)
    finally:
        ops.seg_label_map_rescaled = real
    q = torch.quantile(captured["score"].double().cpu(), torch.arange(1, T + 1, dtype=torch.float64) / (T + 1))
    return check_thresholds(sorted(set(q.float().tolist())))


def sweep_case(model, text, n_images=64):
    from segclip_amd.segmentation import ImageTransform, SegEvaluator, SegSweepEvaluator
    from tools import rocprof_roofline as rr
    name = f"(vii) sweep {n_images} mixed sizes"
    kw = dict(mode="slide", crop_size=(224, 224), stride=(224, 224))
    seg = SegInference(model, text, True, bg_thresh=0.80, **kw)
    tf = ImageTransform()
    raws, gts = raw_inputs(seg, n_images)
    SWEEP_THR = sweep_thresholds(seg, raws, gts, tf)
    T = len(SWEEP_THR)
    pixels = sum(int(g.numel()) for g in gts)
    single = SegEvaluator(seg)
    sweep = SegSweepEvaluator(seg, SWEEP_THR)
    singles = [SegEvaluator(SegInference(model, text, True, bg_thresh=t, **kw)) for t in SWEEP_THR]

    def all_singles():
        for ev in singles:
            ev.update_raw(raws, gts, tf)

    ways = [("single update_raw", lambda: single.update_raw(raws, gts, tf), 2),
            (f"sweep update_raw, {T} thresholds", lambda: sweep.update_raw(raws, gts, tf), 2),
            (f"{T} single update_raw calls", all_singles, 1)]
    with torch.no_grad():
        for _, fn, _ in ways:   # warm-up, and the areas of the sweep and of the singles after the same number of calls
            fn()
        equal = all(bool(torch.equal(sweep.areas[t], ev.areas)) for t, ev in enumerate(singles))
        distinct = 1 + sum(int(not torch.equal(sweep.areas[t], sweep.areas[t - 1])) for t in range(1, T))
        for _, fn, _ in ways:
            fn()
        torch.cuda.synchronize()
        ts = [[] for _ in ways]
        sampler = ClockSampler().start()
        for _ in range(REPS):   # alternating: every repeat times the three ways one after the other
            for k, (_, fn, inner) in enumerate(ways):
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) / inner)
        clk = sampler.stop()
    say(f"{name}: thresholds {[float(f'{t:.4g}') for t in SWEEP_THR]} (quantiles of the inputs' best_score), {pixels} output pixels, "
        f"{seg.num_classes} classes")
    meds = [statistics.median(t) for t in ts]
    for (what, _, inner), t, med in zip(ways, ts, meds):
        say(f"{name}: {what:32s} {med * 1e3:9.2f} ms (min {min(t) * 1e3:.2f}, max {max(t) * 1e3:.2f}; {REPS} x {inner} calls)  "
            f"{n_images / med:8.1f} images/s")
    spread = max((max(t) - min(t)) / statistics.median(t) for t in ts)
    say(f"{name}: sweep / single {meds[1] / meds[0]:.4f}; ({T} singles) / sweep {meds[2] / meds[1]:.4f}; largest run-to-run spread "
        f"{spread:.4f} of the median; clock {clk}")
    say(f"{name}: the {T} area slices equal the {T} single runs: {equal}; {distinct} distinct slices")
    say(f"{name}: peak allocation of one call: single {peak_of(ways[0][1]) / 2**20:8.1f} MiB, sweep {peak_of(ways[1][1]) / 2**20:8.1f} MiB, "
        f"sweep with the {T} label planes {peak_of(lambda: sweep.update_raw(raws, gts, tf, return_labels=True)) / 2**20:8.1f} MiB")
    # the kernel's own time: a child of this tool that only calls the sweep's update_raw, under rocprofv3 --kernel-trace --stats
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        try:
            rc, _, err = rr.run_child([os.path.abspath(__file__), "--sweep-child"], tmp)
            db = rr.find_db(tmp)
            table = rr.kernel_table(db) if rc == 0 and db else []
        except Exception as e:   # no rocprofv3 on the box
            rc, err, table = -1, repr(e), []
    for what, pat, med in (("segclip_seg_label_map_rescaled_sweep", "seg_sweep_kernel", meds[1]),
                           ("segclip_seg_label_map_rescaled (the single entry, middle threshold)", "seg_rescaled_kernel", meds[0])):
        rows = [r for r in table if pat in r[0]]
        if not rows:
            say(f"{name}: {what} alone: unmeasured (rocprofv3 child rc={rc}: {err[-200:]})")
            continue
        calls, us = sum(r[1] for r in rows), sum(r[2] for r in rows)
        avg = us / calls
        say(f"{name}: {what} alone (rocprofv3 --kernel-trace --stats, {calls} launches) {avg:9.1f} us per launch = {avg * 1e-6 / med:.4f} "
            f"of its update_raw; {pixels / avg / 1e3:.3f} Gpixel/s")


def sweep_child(model, text):
    """Five sweep update_raw calls and five single ones, nothing else: what the rocprofv3 child of sweep_case traces."""
    from segclip_amd.segmentation import ImageTransform, SegEvaluator, SegSweepEvaluator
    kw = dict(mode="slide", crop_size=(224, 224), stride=(224, 224))
    seg = SegInference(model, text, True, bg_thresh=0.80, **kw)
    raws, gts = raw_inputs(seg)
    tf = ImageTransform()
    thr = sweep_thresholds(seg, raws, gts, tf)
    ev, one = SegSweepEvaluator(seg, thr), SegEvaluator(SegInference(model, text, True, bg_thresh=thr[len(thr) // 2], **kw))
    with torch.no_grad():
        for _ in range(5):
            ev.update_raw(raws, gts, tf)
            one.update_raw(raws, gts, tf)
    torch.cuda.synchronize()


def eager_pamr(raw, lab, C, mean, std, dilations, iters):
    """The definition of segclip_seg_refine transcribed to eager torch in fp32 for one image: (h, w, 3) uint8 picture and (h, w)
    uint8 labels -> refined (h, w) uint8 labels.  The (C, h, w) one-hot and its (C, 8 D, h, w) unfolding exist here."""
    h, w = lab.shape
    D = len(dilations)

    def taps(t):   # (1, K, h, w) -> (1, K, 8 D, h, w)
        out = []
        for d in dilations:
            u = F.unfold(F.pad(t, (d, d, d, d), mode="replicate"), 3, dilation=d).view(1, t.shape[1], 9, h, w)
            out.append(torch.cat([u[:, :, :4], u[:, :, 5:]], dim=2))
        return torch.cat(out, dim=2)

    x = ((raw.float() - mean) / std).permute(2, 0, 1)[None]
    nx = taps(x)
    sigma = torch.cat([nx, x[:, :, None].expand(-1, -1, D, -1, -1)], dim=2).std(dim=2, keepdim=True)
    wts = torch.softmax(-((x[:, :, None] - nx).abs() / (1e-8 + 0.1 * sigma)).mean(dim=1, keepdim=True), dim=2)
    m = (lab.long()[None] == torch.arange(C, device=lab.device)[:, None, None]).float()[None]
    for _ in range(iters):
        m = (taps(m) * wts).sum(dim=2)
    top, arg = m[0].max(dim=0)
    return torch.where(top > 0, arg.to(torch.uint8), lab)


def refine_case(model, text, n_images=64):
    from segclip_amd.segmentation import PAMR, ImageTransform, SegEvaluator
    from tools import rocprof_roofline as rr
    name = f"(viii) refine {n_images} mixed sizes"
    seg = SegInference(model, text, True, bg_thresh=0.80, mode="slide", crop_size=(224, 224), stride=(224, 224))
    tf, pamr = ImageTransform(), PAMR()
    raws, gts = raw_inputs(seg, n_images)
    C, D, T = seg.num_classes, len(pamr.dilations), pamr.iters
    pixels = sum(int(g.numel()) for g in gts)
    mean, std = torch.tensor(tf.mean, device="cuda"), torch.tensor(tf.std, device="cuda")
    plain, fused, eager = SegEvaluator(seg), SegEvaluator(seg), SegEvaluator(seg)

    def eager_way(keep=None):
        maps = eager.update_raw(raws, gts, tf, return_labels=True)
        eager.areas.zero_()   # the areas of the refined maps only
        for r, l, g in zip(raws, maps, gts):
            out = eager_pamr(r, l, C, mean, std, pamr.dilations, T)
            ops.seg_areas(out, g, C, areas=eager.areas)
            if keep is not None:
                keep.append(out)

    ways = [("update_raw", lambda: plain.update_raw(raws, gts, tf), 2),
            (f"update_raw(refine=PAMR({T}, {pamr.dilations}))", lambda: fused.update_raw(raws, gts, tf, refine=pamr), 2),
            ("update_raw + eager unfold PAMR + seg_areas", eager_way, 1)]
    with torch.no_grad():
        maps = plain.update_raw(raws, gts, tf, return_labels=True)
        chunks = [max(1, (int(m.unique().numel()) + 7) // 8) for m in maps]   # chunks of 8 planes an image keeps busy
        got, want = fused.update_raw(raws, gts, tf, return_labels=True, refine=pamr), []
        eager_way(want)
        agree = sum(int((a == b).sum()) for a, b in zip(got, want)) / pixels
        moved = sum(int((a != b).sum()) for a, b in zip(got, maps)) / pixels
        for _, fn, _ in ways:
            fn()
        torch.cuda.synchronize()
        ts = [[] for _ in ways]
        sampler = ClockSampler().start()
        for _ in range(REPS):   # alternating: every repeat times the three ways one after the other
            for k, (_, fn, inner) in enumerate(ways):
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) / inner)
        clk = sampler.stop()
    say(f"{name}: {pixels} pixels, {C} classes, {T} iterations at dilations {pamr.dilations}; the refinement changes {moved:.4%} of the "
        f"labels; kernel and eager transcription agree on {agree:.4%} of the pixels")
    meds = [statistics.median(t) for t in ts]
    for (what, _, inner), t, med in zip(ways, ts, meds):
        say(f"{name}: {what:44s} {med * 1e3:9.2f} ms (min {min(t) * 1e3:.2f}, max {max(t) * 1e3:.2f}; {REPS} x {inner} calls)  "
            f"{n_images / med:8.1f} images/s")
    spread = max((max(t) - min(t)) / statistics.median(t) for t in ts)
    say(f"{name}: the refinement costs {(meds[1] - meds[0]) * 1e3:.2f} ms fused and {(meds[2] - meds[0]) * 1e3:.2f} ms eager over the "
        f"yardstick: eager / fused {(meds[2] - meds[0]) / max(meds[1] - meds[0], 1e-9):.2f}; refined / plain update_raw "
        f"{meds[1] / meds[0]:.4f}; largest run-to-run spread {spread:.4f} of the median; clock {clk}")
    say(f"{name}: peak allocation of one call: plain {peak_of(ways[0][1]) / 2**20:8.1f} MiB, refined {peak_of(ways[1][1]) / 2**20:8.1f} MiB, "
        f"eager {peak_of(eager_way) / 2**20:8.1f} MiB")
    # the kernels' own time: a child of this tool that only calls update_raw(refine=), under rocprofv3 --kernel-trace --stats
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        try:
            rc, _, err = rr.run_child([os.path.abspath(__file__), "--refine-child"], tmp)
            db = rr.find_db(tmp)
            table = rr.kernel_table(db) if rc == 0 and db else []
        except Exception as e:   # no rocprofv3 on the box
            rc, err, table = -1, repr(e), []
    design = sum(int(g.numel()) * c for g, c in zip(gts, chunks)) * T * (32 * D + 64)   # bytes of the step kernels of one call
    for what, pat in (("seg_refine_weights_kernel", "seg_refine_weights_kernel"), ("seg_refine_step_kernel", "seg_refine_step_kernel")):
        rows = [r for r in table if pat in r[0]]
        if not rows:
            say(f"{name}: {what} alone: unmeasured (rocprofv3 child rc={rc}: {err[-200:]})")
            continue
        calls, us = sum(r[1] for r in rows), sum(r[2] for r in rows)
        line = f"{name}: {what} alone (rocprofv3 --kernel-trace --stats, {calls} launches in 5 calls) {us / 5:9.1f} us per update_raw"
        if pat == "seg_refine_step_kernel":
            line += (f"; design traffic {design / 1e6:.1f} MB per call ({32 * D + 64} B per pixel, iteration and busy chunk of 8 planes) "
                     f"= {design / (us / 5 * 1e-6) / 1e12:.3f} TB/s, {design / (us / 5 * 1e-6) / HBM_PEAK:.3f} of the HBM peak")
        say(line)


def refine_child(model, text):
    """Five update_raw(refine=PAMR()) calls and nothing else: what the rocprofv3 child of refine_case traces."""
    from segclip_amd.segmentation import PAMR, ImageTransform, SegEvaluator
    seg = SegInference(model, text, True, bg_thresh=0.80, mode="slide", crop_size=(224, 224), stride=(224, 224))
    raws, gts = raw_inputs(seg)
    ev, tf, pamr = SegEvaluator(seg), ImageTransform(), PAMR()
    with torch.no_grad():
        for _ in range(5):
            ev.update_raw(raws, gts, tf, refine=pamr)
    torch.cuda.synchronize()


class _AllOutputs:
    """segclip_seg_components with every output on a list of label maps: buffers and table made once, call() enqueues only."""

    def __init__(self, maps, connectivity=8, min_area=16):
        from segclip_amd.segmentation import _Maps
        batch = _Maps.of(maps)
        self.flat, n = batch.flat, batch.flat.numel()
        self.table, self.n_blocks, self.side = ops.seg_components_table(batch.sizes, batch.offs, "cuda")
        self.ids, self.area = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        self.records = torch.empty(n, ops.SEG_CC_RECORD, dtype=torch.int64, device="cuda")   # room for one component per pixel
        self.count = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.cleaned = torch.zeros(n, dtype=torch.uint8, device="cuda")
        self.kw = dict(connectivity=connectivity, min_area=min_area, max_side=self.side)

    def call(self):
        ops.seg_components(self.table, self.n_blocks, self.flat, ids=self.ids, area_px=self.area, records=self.records,
                           count=self.count, cleaned=self.cleaned, **self.kw)


def objects_maps(model, text, n_images=64):
    from segclip_amd.segmentation import ImageTransform, SegEvaluator
    seg = SegInference(model, text, True, bg_thresh=0.80, mode="slide", crop_size=(224, 224), stride=(224, 224))
    raws, gts = raw_inputs(seg, n_images)
    tf = ImageTransform()
    with torch.no_grad():
        maps = SegEvaluator(seg).update_raw(raws, gts, tf, return_labels=True)
    return seg, tf, raws, gts, maps


def objects_case(model, text, n_images=64):
    from segclip_amd.segmentation import Despeckle, SegEvaluator, components, despeckle
    from tools import rocprof_roofline as rr
    name = f"(ix) objects {n_images} mixed sizes"
    seg, tf, raws, gts, maps = objects_maps(model, text, n_images)
    pixels = sum(int(m.numel()) for m in maps)
    d = Despeckle(16)
    full = _AllOutputs(maps)
    plain, cleaned_ev = SegEvaluator(seg), SegEvaluator(seg)
    try:
        from scipy import ndimage
        host_maps, scale, host_what = maps, 1.0, ".cpu() + scipy.ndimage.label per present class (8-structure)"
        ones = [[1, 1, 1]] * 3

        def host_one(a):
            return sum(ndimage.label(a == v, structure=ones)[1] for v in set(a.reshape(-1).tolist()))
    except ImportError:
        from tests import cc_reference
        host_maps, scale = maps[:4], n_images / 4
        host_what = f".cpu() + the numpy restatement of the tests on 4 maps, scaled by {scale:g} (no scipy here)"

        def host_one(a):
            return len(cc_reference.components([a], 8)[2])

    def host_way():
        return sum(host_one(m.cpu().numpy()) for m in host_maps)

    ways = [("seg_components, every output, no host copy", full.call, 4),
            ("components() (ids + records, one host sync)", lambda: components(maps, max_objects=pixels), 4),
            (f"despeckle(min_area={d.min_area})", lambda: despeckle(maps, d.min_area), 4),
            ("update_raw", lambda: plain.update_raw(raws, gts, tf), 2),
            (f"update_raw(clean=Despeckle({d.min_area}))", lambda: cleaned_ev.update_raw(raws, gts, tf, clean=d), 2),
            (host_what, host_way, 1)]
    with torch.no_grad():
        n_obj = components(maps, max_objects=pixels).count
        assert scale != 1.0 or n_obj == host_way(), "the host route counts other components"
        changed = sum(int((a != b).sum()) for a, b in zip(despeckle(maps, d.min_area), maps)) / pixels
        for _, fn, _ in ways[:-1]:
            fn()
        torch.cuda.synchronize()
        ts = [[] for _ in ways]
        sampler = ClockSampler().start()
        for rep in range(REPS):
            for k, (_, fn, inner) in enumerate(ways):
                if k == len(ways) - 1 and rep >= 3:
                    continue   # the host route: three repeats
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) / inner)
        clk = sampler.stop()
    say(f"{name}: {pixels} pixels in the label maps of update_raw, {n_obj} components under 8-connectivity; despeckling below "
        f"{d.min_area} pixels changes {changed:.4%} of the labels")
    meds = [statistics.median(t) * (scale if k == len(ways) - 1 else 1.0) for k, t in enumerate(ts)]
    for (what, _, inner), t, med in zip(ways, ts, meds):
        say(f"{name}: {what:60s} {med * 1e3:9.3f} ms (min {min(t) * 1e3:.3f}, max {max(t) * 1e3:.3f}; {len(t)} x {inner} calls)")
    spread = max((max(t) - min(t)) / statistics.median(t) for t in ts[:-1])
    say(f"{name}: clean= adds {(meds[4] - meds[3]) * 1e3:.3f} ms to update_raw ({meds[4] / meds[3]:.4f} x); host route / components() "
        f"{meds[5] / meds[1]:.1f}; host route / every output {meds[5] / meds[0]:.1f}; every output: {pixels / meds[0] / 1e9:.2f} Gpixel/s; "
        f"largest run-to-run spread {spread:.4f} of the median; clock {clk}")
    # atomic contention: one root for every tile, one root per pixel, and noise
    side = 500
    g = torch.Generator().manual_seed(2)
    yy, xx = torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij")
    for what, m, conn in (("one component", torch.ones(side, side, dtype=torch.uint8), 8),
                          ("checkerboard, 4-connectivity", ((yy + xx) % 2).to(torch.uint8), 4),
                          ("3-label noise", torch.randint(0, 3, (side, side), generator=g).to(torch.uint8), 8)):
        one = _AllOutputs([m.cuda()], connectivity=conn)
        med, lo, hi = timed(one.call, 20)
        say(f"{name}: {side} x {side} {what:30s} {int(one.count.item()):7d} components, every output {med * 1e6:9.1f} us "
            f"(min {lo * 1e6:.1f}, max {hi * 1e6:.1f}; {REPS} x 20 calls)")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        try:
            rc, _, err = rr.run_child([os.path.abspath(__file__), "--objects-child"], tmp)
            db = rr.find_db(tmp)
            table = rr.kernel_table(db) if rc == 0 and db else []
        except Exception as e:   # no rocprofv3 on the box
            rc, err, table = -1, repr(e), []
    rows = [r for r in table if "seg_cc_" in r[0]]
    if not rows:
        say(f"{name}: the kernels alone: unmeasured (rocprofv3 child rc={rc}: {err[-200:]})")
    for r in rows:
        say(f"{name}: {r[0][r[0].find('seg_cc_'):][:36]:36s} alone (rocprofv3 --kernel-trace --stats, {r[1]} launches in 5 calls) {r[2] / 5:9.1f} us per call")
    if rows:
        say(f"{name}: all seg_cc kernels {sum(r[2] for r in rows) / 5:9.1f} us per call with every output")


def objects_child(model, text):
    """Five calls of segclip_seg_components with every output on the 64 label maps: what the rocprofv3 child of objects_case traces."""
    full = _AllOutputs(objects_maps(model, text)[4])
    for _ in range(5):
        full.call()
    torch.cuda.synchronize()


def host_merge(a, min_area, ndimage):
    """One round of the merge on the host: scipy.ndimage.label per class, a cross dilation per small component."""
    cross, ones = ndimage.generate_binary_structure(2, 1), [[1, 1, 1]] * 3
    comp, areas, labels = a.astype("int64") * 0, [0], [-1]
    for v in set(a.reshape(-1).tolist()):
        lab, n = ndimage.label(a == v, structure=ones)
        comp[lab > 0] = lab[lab > 0] + len(areas) - 1
        areas += [int(x) for x in ndimage.sum_labels(lab > 0, lab, range(1, n + 1))]
        labels += [v] * n
    out = a.copy()
    for k, sl in enumerate(ndimage.find_objects(comp), start=1):
        if areas[k] >= min_area:
            continue
        box = tuple(slice(max(s.start - 1, 0), s.stop + 1) for s in sl)   # the component's box, one pixel wider
        mask = comp[box] == k
        ring = ndimage.binary_dilation(mask, structure=cross) & ~mask
        cand = [c for c in set(comp[box][ring].tolist()) if areas[c] >= min_area]
        if cand:
            out[box][mask] = labels[min(cand, key=lambda c: (-areas[c], labels[c]))]
    return out


def merge_case(model, text, n_images=64):
    """(xii) despeckling by merging (csrc/segment_sieve.inc) on the label maps of --objects, alternating within every repeat"""
    from segclip_amd.segmentation import Despeckle, SegEvaluator, despeckle
    from tools import rocprof_roofline as rr
    name = f"(xii) merge {n_images} mixed sizes"
    seg, tf, raws, gts, maps = objects_maps(model, text, n_images)
    pixels = sum(int(m.numel()) for m in maps)
    m = 16
    d = Despeckle(m, merge=True)
    plain, cleaned_ev = SegEvaluator(seg), SegEvaluator(seg)
    # the host route comes last and update_raw first: the short calls do not follow the quarter second in which the device idles
    ways = [("update_raw", lambda: plain.update_raw(raws, gts, tf), 2),
            (f"update_raw(clean=Despeckle({m}, merge=True))", lambda: cleaned_ev.update_raw(raws, gts, tf, clean=d), 2),
            (f"despeckle(min_area={m}) as shipped: the yardstick", lambda: despeckle(maps, m), 4),
            (f"despeckle(min_area={m}, merge=True)", lambda: despeckle(maps, m, merge=True), 4),
            (f"despeckle(min_area={m}, merge=True, rounds=2)", lambda: despeckle(maps, m, merge=True, rounds=2), 4)]
    try:
        from scipy import ndimage
        ways.append((".cpu() + scipy.ndimage.label per class + a dilation per small component, one round",
                     lambda: [host_merge(a.cpu().numpy(), m, ndimage) for a in maps], 1))
    except ImportError:
        ndimage = None
    with torch.no_grad():
        one, two = despeckle(maps, m, merge=True), despeckle(maps, m, merge=True, rounds=2)
        changed = [sum(int((a != b).sum()) for a, b in zip(x, maps)) / pixels for x in (despeckle(maps, m), one, two)]
        if ndimage is not None:
            assert all(bool((torch.from_numpy(host_merge(a.cpu().numpy(), m, ndimage)).cuda() == b).all())
                       for a, b in zip(maps[:8], one)), "the host route merges otherwise"
        for _, fn, _ in ways[:5]:
            fn()
        torch.cuda.synchronize()
        ts = [[] for _ in ways]
        sampler = ClockSampler().start()
        for rep in range(REPS):
            for k, (_, fn, inner) in enumerate(ways):
                if k == 5 and rep >= 3:
                    continue   # the host route: three repeats
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) / inner)
        clk = sampler.stop()
    say(f"{name}: {pixels} pixels in the label maps of update_raw; below {m} pixels the fill changes {changed[0]:.4%} of the labels, "
        f"one round of merging {changed[1]:.4%}, two rounds {changed[2]:.4%}")
    meds = [statistics.median(t) for t in ts]
    for (what, _, inner), t, med in zip(ways, ts, meds):
        say(f"{name}: {what:84s} {med * 1e3:9.3f} ms (min {min(t) * 1e3:.3f}, max {max(t) * 1e3:.3f}; {len(t)} x {inner} calls)")
    spread = max((max(t) - min(t)) / statistics.median(t) for t in ts[:5])
    say(f"{name}: merging / the fill mode {meds[3] / meds[2]:.3f} (one round), {meds[4] / meds[2]:.3f} (two); clean= adds "
        f"{(meds[1] - meds[0]) * 1e3:.3f} ms to update_raw ({meds[1] / meds[0]:.4f} x)"
        + (f"; host route / one round {meds[5] / meds[3]:.1f}" if len(meds) > 5 else "; host route: unmeasured (no scipy here)")
        + f"; largest run-to-run spread {spread:.4f} of the median; clock {clk}")
    # how much the vote costs where most pixels vote: one kept component, orphans only, and noise whose components are mostly small
    side = 500
    g = torch.Generator().manual_seed(2)
    yy, xx = torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij")
    for what, a, conn in (("one component", torch.ones(side, side, dtype=torch.uint8), 8),
                          ("checkerboard, 4-connectivity", ((yy + xx) % 2).to(torch.uint8), 4),
                          ("3-label noise, 4-connectivity", torch.randint(0, 3, (side, side), generator=g).to(torch.uint8), 4),
                          ("3-label noise", torch.randint(0, 3, (side, side), generator=g).to(torch.uint8), 8)):
        flat = a.cuda().reshape(-1)
        table, n_blocks, max_side = ops.seg_components_table([(side, side)], [0], "cuda")
        out, filled = torch.zeros_like(flat), torch.zeros_like(flat)
        kw = dict(connectivity=conn, min_area=m, max_side=max_side)
        t_fill = timed(lambda: ops.seg_components(table, n_blocks, flat, cleaned=filled, **kw), 20)
        t_one = timed(lambda: ops.seg_sieve(table, n_blocks, flat, cleaned=out, **kw), 20)
        share = float((out != flat).float().mean())
        t_two = timed(lambda: ops.seg_sieve(table, n_blocks, flat, cleaned=out, rounds=2, **kw), 20)
        say(f"{name}: {side} x {side} {what:30s} one round changes {share:8.4%} of the labels: fill mode {t_fill[0] * 1e6:7.1f} us, "
            f"one round {t_one[0] * 1e6:7.1f} us (min {t_one[1] * 1e6:.1f}, max {t_one[2] * 1e6:.1f}), two rounds {t_two[0] * 1e6:7.1f} us "
            f"({REPS} x 20 calls)")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        try:
            rc, _, err = rr.run_child([os.path.abspath(__file__), "--merge-child"], tmp)
            db = rr.find_db(tmp)
            table = rr.kernel_table(db) if rc == 0 and db else []
        except Exception as e:   # no rocprofv3 on the box
            rc, err, table = -1, repr(e), []
    rows = [r for r in table if "seg_cc_" in r[0] or "seg_sieve_" in r[0]]
    if not rows:
        say(f"{name}: the kernels alone: unmeasured (rocprofv3 child rc={rc}: {err[-200:]})")
    for r in rows:
        tag = "seg_sieve_" if "seg_sieve_" in r[0] else "seg_cc_"
        per = r[2] / 5
        note = ""
        if "seg_sieve_vote" in r[0]:   # design traffic: 4 B of root + 4 B of gathered area per pixel; the small pixels' extra reads are few
            note = f"   {8 * pixels / (per * 1e-6) / 1e12:.2f} TB/s of its 8 B per pixel ({8 * pixels / (per * 1e-6) / HBM_PEAK:.1%} of the HBM peak)"
        if "seg_sieve_final" in r[0]:  # 4 B of root + 4 B of area + 1 B read, 1 B written
            note = f"   {10 * pixels / (per * 1e-6) / 1e12:.2f} TB/s of its 10 B per pixel ({10 * pixels / (per * 1e-6) / HBM_PEAK:.1%} of the HBM peak)"
        say(f"{name}: {r[0][r[0].find(tag):][:36]:36s} alone (rocprofv3 --kernel-trace --stats, {r[1]} launches in 5 calls) {per:9.1f} us per call{note}")
    if rows:
        say(f"{name}: all kernels of one round {sum(r[2] for r in rows) / 5:9.1f} us per call (the clearing of the slots is a fill, not in this list)")


def merge_child(model, text):
    """Five one-round calls of despeckle(merge=True) on the 64 label maps: what the rocprofv3 child of merge_case traces."""
    from segclip_amd.segmentation import despeckle
    maps = objects_maps(model, text)[4]
    for _ in range(5):
        despeckle(maps, 16, merge=True)
    torch.cuda.synchronize()


class _BoundaryCall:
    """segclip_seg_boundary on a list of label maps and ground truths, the outputs allocated once."""

    def __init__(self, maps, gts, C, boundary, bands):
        from segclip_amd.segmentation import _Maps
        batch = _Maps.of(maps)
        self.flat = batch.flat
        self.gt, gt_offs = _Maps.gapless_of(list(gts))
        self.radii = [boundary.radius_of(h, w, i) for i, (h, w) in enumerate(batch.sizes)]
        self.table, self.n_blocks, self.side = ops.seg_boundary_table(batch.sizes, batch.offs, gt_offs, self.radii, "cuda")
        self.areas = torch.zeros(2, 3, C, dtype=torch.int64, device="cuda")
        self.pred_band = torch.zeros_like(self.flat) if bands else None
        self.gt_band = torch.zeros_like(self.gt) if bands else None
        self.C = C

    def call(self):
        ops.seg_boundary(self.table, self.n_blocks, self.flat, gt=self.gt, num_classes=self.C, pred_band=self.pred_band,
                         gt_band=self.gt_band, areas=self.areas, max_side=self.side)


def boundary_case(model, text, n_images=64):
    from segclip_amd.segmentation import Boundary, SegEvaluator
    from tools import rocprof_roofline as rr
    name = f"(x) boundary {n_images} mixed sizes"
    seg, tf, raws, gts, maps = objects_maps(model, text, n_images)
    pixels = sum(int(m.numel()) for m in maps)
    C, b = seg.num_classes, Boundary()
    plain, with_b = SegEvaluator(seg), SegEvaluator(seg, boundary=b)
    alone, banded = _BoundaryCall(maps, gts, C, b, False), _BoundaryCall(maps, gts, C, b, True)
    HOST = min(8, n_images)   # the host route takes seconds per map: the first 8 maps, scaled to all
    try:
        from scipy import ndimage
        ones = [[True] * 3] * 3

        def host_one(p, g, d):
            out = torch.zeros(2, 3, C, dtype=torch.int64)
            bp, bg = torch.zeros(p.shape, dtype=torch.bool), torch.zeros(p.shape, dtype=torch.bool)
            for m, band in ((p, bp), (g, bg)):
                for v in set(m.reshape(-1).tolist()):
                    mask = m == v
                    band |= torch.from_numpy(mask & ~ndimage.binary_erosion(mask, ones, iterations=d, border_value=0))
            keep = torch.from_numpy(g != 255)
            p, g = torch.from_numpy(p).long(), torch.from_numpy(g).long()
            # slot 0 alone: the trimap would need the frame taken off the eroded band
            out[0, 0] = torch.bincount(p[keep & bp & bg & (p == g)], minlength=256)[:C]
            out[0, 1] = torch.bincount(p[keep & bp], minlength=256)[:C]
            out[0, 2] = torch.bincount(g[keep & bg & (g < C)], minlength=256)[:C]
            return out

        def host_way():
            return sum(host_one(m.cpu().numpy(), g.cpu().numpy(), d) for m, g, d in zip(maps[:HOST], gts[:HOST], alone.radii))
    except ImportError:
        host_way = None

    ways = [("update_raw", lambda: plain.update_raw(raws, gts, tf), 2),
            ("update_raw of SegEvaluator(boundary=Boundary())", lambda: with_b.update_raw(raws, gts, tf), 2),
            ("seg_boundary alone, areas only", alone.call, 4),
            ("seg_boundary alone, areas and both bands", banded.call, 4)]
    if host_way is not None:
        ways.append((f".cpu() + scipy binary_erosion per present class + counting (slot 0), {HOST} maps scaled to {n_images}", host_way, 1))
    with torch.no_grad():
        if host_way is not None:
            first = _BoundaryCall(maps[:HOST], gts[:HOST], C, b, False)
            first.call()
            assert torch.equal(first.areas[0].cpu(), host_way()[0]), "the host route counts other areas"
        for _, fn, _ in ways[:4]:
            fn()
        torch.cuda.synchronize()
        peaks = [peak_of(fn) for _, fn, _ in ways[:2]]
        ts = [[] for _ in ways]
        sampler = ClockSampler().start()
        for rep in range(REPS):
            for k, (_, fn, inner) in enumerate(ways):
                if k == 4 and rep >= 2:
                    continue   # the host route: two repeats
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) / inner)
        clk = sampler.stop()
    say(f"{name}: {pixels} pixels in the label maps of update_raw, radii {min(alone.radii)} .. {max(alone.radii)} at ratio {b.ratio}; "
        f"ground truths of per-pixel noise: every pixel lies in the band")
    meds = [statistics.median(t) * (n_images / HOST if k == 4 else 1.0) for k, t in enumerate(ts)]
    for k, ((what, _, inner), t, med) in enumerate(zip(ways, ts, meds)):
        f = n_images / HOST if k == 4 else 1.0
        say(f"{name}: {what:96s} {med * 1e3:9.3f} ms (min {min(t) * f * 1e3:.3f}, max {max(t) * f * 1e3:.3f}; {len(t)} x {inner} calls)")
    spread = max((max(t) - min(t)) / statistics.median(t) for t in ts[:4])
    host = f"host route / seg_boundary alone {meds[4] / meds[2]:.1f}" if host_way is not None else "host route: **Unmeasured** (no scipy here)"
    say(f"{name}: boundary= adds {(meds[1] - meds[0]) * 1e3:.3f} ms to update_raw ({meds[1] / meds[0]:.4f} x); {host}; areas only: "
        f"{pixels / meds[2] / 1e9:.2f} Gpixel/s; peak allocation {peaks[0] / 2**20:.1f} MiB without, {peaks[1] / 2**20:.1f} MiB with boundary=; "
        f"largest run-to-run spread {spread:.4f} of the median; clock {clk}")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        try:
            rc, _, err = rr.run_child([os.path.abspath(__file__), "--boundary-child"], tmp)
            db = rr.find_db(tmp)
            table = rr.kernel_table(db) if rc == 0 and db else []
        except Exception as e:   # no rocprofv3 on the box
            rc, err, table = -1, repr(e), []
    rows = [r for r in table if "seg_bd_" in r[0]]
    if not rows:
        say(f"{name}: the kernels alone: **Unmeasured** (rocprofv3 child rc={rc}: {err[-200:]})")
    for r in rows:
        say(f"{name}: {r[0][r[0].find('seg_bd_'):][:36]:36s} alone (rocprofv3 --kernel-trace --stats, {r[1]} launches in 5 calls) {r[2] / 5:9.1f} us per call")
    if rows:
        say(f"{name}: all seg_bd kernels {sum(r[2] for r in rows) / 5:9.1f} us per call with every output")


def boundary_child(model, text):
    """Five calls of segclip_seg_boundary with every output on the 64 label maps: what the rocprofv3 child of boundary_case traces."""
    from segclip_amd.segmentation import Boundary
    seg, _, _, gts, maps = objects_maps(model, text)
    full = _BoundaryCall(maps, gts, seg.num_classes, Boundary(), True)
    for _ in range(5):
        full.call()
    torch.cuda.synchronize()


class _WideVariantLib:
    """The library with ONE entry replaced: segclip_seg_label_map_rescaled_wide from a second build of csrc/segment.hip with one
    build-time switch of csrc/segment_wide.inc set: -DSEG_WIDE_LANE_SCAN=1 (every lane scans the classes of its own undecided
    pixels at every class count, the uint8 kernel's scheme) or -DSEG_WIDE_LANE_SCAN_CLASSES=0 (the wave-cooperative scan at every
    class count).  The second build links against the first for everything else; it is made here when it is missing (hipcc,
    gfx950), as csrc/build/variants/libsegclip_seg_<tag>.so."""

    ENTRY = "segclip_seg_label_map_rescaled_wide"

    def __init__(self, define, tag):
        import ctypes
        import subprocess
        from segclip_amd import _lib as L
        self.main = L.load()
        csrc = os.path.join(os.path.dirname(L.lib_path()), "csrc")
        path = os.path.join(csrc, "build", "variants", f"libsegclip_seg_{tag}.so")   # not beside the objects build.sh links
        if not os.path.exists(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            hipcc, obj = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), path[:-3] + ".o"
            subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", define, "-c",
                            os.path.join(csrc, "segment.hip"), "-o", obj], check=True)
            subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", obj, "-L" + os.path.dirname(L.lib_path()),
                            "-l:" + os.path.basename(L.lib_path()), "-Wl,-rpath,$ORIGIN/../../..", "-o", path], check=True)
        self.entry = getattr(ctypes.CDLL(path), self.ENTRY)
        self.entry.restype, self.entry.argtypes = L.SIGNATURES[self.ENTRY]

    def __getattr__(self, name):
        return self.entry if name == self.ENTRY else getattr(self.main, name)


def wide_case(model, n_images=64):
    """(xi) the 16-bit label-map kernel at 21, 151, 460 and 848 classes on the inputs of --eval."""
    from segclip_amd import _lib as L
    from segclip_amd.segmentation import SegEvaluator, test_size
    outs = [EVAL_SIZES[i % len(EVAL_SIZES)] for i in range(n_images)]
    g = torch.Generator().manual_seed(1)
    imgs = [torch.randn(3, *test_size(*o), generator=g).cuda() for o in outs]
    pixels = sum(o[0] * o[1] for o in outs)
    try:
        lane_lib = _WideVariantLib("-DSEG_WIDE_LANE_SCAN=1", "lane_scan")
        coop_lib = _WideVariantLib("-DSEG_WIDE_LANE_SCAN_CLASSES=0", "coop_always")
    except Exception as e:   # no hipcc on the box
        lane_lib = coop_lib = None
        say(f"(xi) wide: the builds with the scan fixed are missing and cannot be made here ({e!r}): unmeasured")
    for C in (21, 151, 460, 848):
        name = f"(xi) wide   C={C:4d}"
        text = torch.randn(C - 1, 512, generator=g)
        text = (text / text.norm(dim=-1, keepdim=True)).cuda()
        seg = SegInference(model, text, True, bg_thresh=0.80, mode="slide", crop_size=(224, 224), stride=(224, 224),
                           label_dtype=torch.int16)
        gts = [torch.randint(0, C, o, generator=g).to(torch.int16).cuda() for o in outs]
        ev = SegEvaluator(seg, ignore_index=65535)
        captured = {}
        real = ops.seg_label_map_rescaled_wide

        def capture(*a, **k):
            captured["call"] = (a, k)
            return real(*a, **k)

        ops.seg_label_map_rescaled_wide = capture
        try:
            with torch.no_grad():
                ev.update(imgs, gts, return_labels=True)
        finally:
            ops.seg_label_map_rescaled_wide = real
        a, k = captured["call"]
        soft, tables, dwin, images = a[:4]
        n_elems = k["labels"].numel()

        def fresh(dtype):
            return dict(k, labels=torch.zeros(n_elems, dtype=dtype, device="cuda"), gt=k["gt"].to(dtype),
                        areas=torch.zeros(3, C, dtype=torch.int64, device="cuda"))

        kw = fresh(torch.int16)
        ways = [(f"wide kernel ({'per-lane' if C <= 32 else 'wave-cooperative'} class scan at this class count)", lambda: real(*a, **kw), 5)]
        checks = []

        def variant(lib, what):
            kv = fresh(torch.int16)

            def call():
                main, L._lib = L._lib, lib
                try:
                    real(*a, **kv)
                finally:
                    L._lib = main

            ways.append((f"wide kernel built with {what}", call, 5))
            checks.append((f"build with {what}", kv))

        if C <= 256:
            k8 = fresh(torch.uint8)
            k8["ignore_index"] = 255   # C <= 255: no ground truth reaches it, as none reaches 65535
            ways.append(("uint8 kernel, segclip_seg_label_map_rescaled", lambda: ops.seg_label_map_rescaled(*a, **k8), 5))
            checks.append(("uint8 kernel", k8))
        else:
            gt_long = [t.long() for t in gts]
            first = images[:, 0].tolist()
            count = images[:, 1].tolist()
            dfirst = [torch.tensor([0, c], dtype=torch.int32, device="cuda") for c in count]
            soft3 = soft.view(dwin.shape[0], -1, 14 * 14)
            comp_areas = torch.zeros(3, C, dtype=torch.int64, device="cuda")

            def composition():
                for i, (img, gt) in enumerate(zip(imgs, gt_long)):
                    sl = slice(first[i], first[i] + count[i])
                    logits = ops.seg_logits(soft3[sl], tuple(t[sl] for t in tables), dwin[sl], dfirst[i], (1, img.shape[1], img.shape[2]),
                                            (224, 224), (14, 14), True, 0.80)
                    pred = F.interpolate(logits, size=tuple(gt.shape), mode="bilinear", align_corners=False).argmax(dim=1)[0]
                    keep = gt != 65535
                    p, t = pred[keep], gt[keep]
                    comp_areas[0] += torch.bincount(p[p == t], minlength=C)
                    comp_areas[1] += torch.bincount(p, minlength=C)
                    comp_areas[2] += torch.bincount(t, minlength=C)

            ways.append(("ops.seg_logits per image -> F.interpolate -> argmax -> 3 bincount", composition, 1))
        if lane_lib is not None:   # both scans at every class count: where the kernel's switch between them belongs
            variant(lane_lib, "-DSEG_WIDE_LANE_SCAN=1 (per-lane class scan)")
            variant(coop_lib, "-DSEG_WIDE_LANE_SCAN_CLASSES=0 (wave-cooperative class scan)")
        with torch.no_grad():
            for _, fn, _ in ways:
                fn()
            torch.cuda.synchronize()
            for what, other in checks:
                say(f"{name}: labels equal those of the {what}: {bool(torch.equal(kw['labels'].long(), other['labels'].long()))}; areas "
                    f"equal: {bool(torch.equal(kw['areas'], other['areas']))}")
            if C > 256:
                say(f"{name}: the composition's areas differ from the kernel's by "
                    f"{float((comp_areas - kw['areas']).abs().sum()) / float(kw['areas'].sum()):.2e} of their sum")
            for _, fn, _ in ways:
                fn()
            torch.cuda.synchronize()
            ts = [[] for _ in ways]
            sampler = ClockSampler().start()
            for _ in range(REPS):   # alternating: every repeat times the ways one after the other
                for i, (_, fn, inner) in enumerate(ways):
                    t0 = time.perf_counter()
                    for _ in range(inner):
                        fn()
                    torch.cuda.synchronize()
                    ts[i].append((time.perf_counter() - t0) / inner)
            clk = sampler.stop()
        meds = [statistics.median(t) for t in ts]
        say(f"{name}: {n_images} images, {dwin.shape[0]} windows, {pixels} output pixels; clock {clk}")
        for (what, _, inner), t, med in zip(ways, ts, meds):
            say(f"{name}: {what:78s} {med * 1e6:11.1f} us (min {min(t) * 1e6:.1f}, max {max(t) * 1e6:.1f}; {REPS} x {inner} calls)  "
                f"{pixels / med / 1e9:7.2f} Gpixel/s   {med / meds[0]:7.2f}x the wide kernel")
        if C > 256:
            say(f"{name}: peak allocation of one call: wide kernel {peak_of(ways[0][1]) / 2**20:8.1f} MiB, the composition "
                f"{peak_of(ways[1][1]) / 2**20:8.1f} MiB")


def confusion_case(model, n_images=64):
    """(xiii) ops.seg_confusion at 21, 151, 460 and 848 classes against torch.bincount and against ops.seg_areas."""
    from segclip_amd.segmentation import SegEvaluator, test_size
    outs = [EVAL_SIZES[i % len(EVAL_SIZES)] for i in range(n_images)]
    g = torch.Generator().manual_seed(1)
    imgs = [torch.randn(3, *test_size(*o), generator=g).cuda() for o in outs]
    pixels = sum(o[0] * o[1] for o in outs)
    for C in (21, 151, 460, 848):
        wide = C > 256
        dtype, ignore = (torch.int16, 65535) if wide else (torch.uint8, 255)
        text = torch.randn(C - 1, 512, generator=g)
        text = (text / text.norm(dim=-1, keepdim=True)).cuda()
        seg = SegInference(model, text, True, bg_thresh=0.80, mode="slide", crop_size=(224, 224), stride=(224, 224), label_dtype=dtype)
        dummy = [torch.zeros(o, dtype=dtype, device="cuda") for o in outs]
        with torch.no_grad():
            labels = SegEvaluator(seg, ignore_index=ignore).update(imgs, dummy, return_labels=True)
        shifted = []
        for m in labels:   # the annotation of a prediction: the map moved by (3, 2), 40 rectangles relabelled, a band ignored
            t = torch.roll(m, (3, 2), (0, 1)).clone()
            h, w = t.shape
            for _ in range(40):
                y, x = int(torch.randint(0, h - 40, (1,), generator=g)), int(torch.randint(0, w - 40, (1,), generator=g))
                t[y:y + int(torch.randint(8, 40, (1,), generator=g)), x:x + int(torch.randint(8, 40, (1,), generator=g))] = \
                    int(torch.randint(0, C, (1,), generator=g))
            t[:4] = -1 if wide else 255
            shifted.append(t.reshape(-1))
        maps = torch.cat([m.reshape(-1) for m in labels])
        noise = [torch.randint(0, C, (pixels,), generator=g).to(dtype).cuda() for _ in range(2)]
        truths = {"shifted maps": (maps, torch.cat(shifted)), "random truth": (maps, noise[0]), "both random": (noise[1], noise[0])}
        areas_fn = ops.seg_areas_wide if wide else ops.seg_areas
        route = ops.seg_confusion_route(C, dtype)
        for gt_name, (pred, gt) in truths.items():
            name = f"(xiii) confusion C={C:4d} {gt_name:13s}"
            distinct = int(torch.unique(pred.long() & 0xFFFF).numel())
            conf = torch.zeros(C + 1, C + 1, dtype=torch.int64, device="cuda")
            areas = torch.zeros(3, C, dtype=torch.int64, device="cuda")
            kept = {}

            def by_bincount():
                p, t = pred.long(), gt.long()
                if wide:
                    p, t = p & 0xFFFF, t & 0xFFFF
                keep = t != ignore
                p, t = p[keep].clamp_(max=C), t[keep].clamp_(max=C)
                kept["m"] = torch.bincount(t * (C + 1) + p, minlength=(C + 1) * (C + 1)).view(C + 1, C + 1)

            ways = [(f"ops.seg_confusion ({route} route)", lambda: ops.seg_confusion(pred, gt, C, ignore, conf=conf), 10),
                    ("masking in torch -> g * (C + 1) + p as int64 -> torch.bincount", by_bincount, 3),
                    ("ops.seg_areas_wide" if wide else "ops.seg_areas", lambda: areas_fn(pred, gt, C, ignore, areas=areas), 10)]
            with torch.no_grad():
                conf.zero_()
                areas.zero_()
                for _, fn, _ in ways:
                    fn()
                torch.cuda.synchronize()
                cells = int((conf > 0).sum())
                say(f"{name}: matrix equal to bincount's: {bool(torch.equal(conf, kept['m']))}; its projection equal to the areas: "
                    f"{bool(torch.equal(torch.stack([conf.diagonal()[:C], conf.sum(0)[:C], conf.sum(1)[:C]]), areas))}; "
                    f"{distinct} distinct predicted labels, {cells} non-empty cells")
                for _ in range(2):
                    for _, fn, _ in ways:
                        fn()
                torch.cuda.synchronize()
                ts = [[] for _ in ways]
                sampler = ClockSampler().start()
                for _ in range(REPS):   # alternating: every repeat times the ways one after the other
                    for i, (_, fn, inner) in enumerate(ways):
                        t0 = time.perf_counter()
                        for _ in range(inner):
                            fn()
                        torch.cuda.synchronize()
                        ts[i].append((time.perf_counter() - t0) / inner)
                clk = sampler.stop()
            meds = [statistics.median(t) for t in ts]
            nbytes = 2 * pixels * pred.element_size()
            say(f"{name}: {pixels} pixels of {'int16' if wide else 'uint8'} maps, {nbytes / 2**20:.1f} MiB read per call; clock {clk}")
            for (what, _, inner), t, med in zip(ways, ts, meds):
                say(f"{name}: {what:68s} {med * 1e6:10.1f} us (min {min(t) * 1e6:.1f}, max {max(t) * 1e6:.1f}; {REPS} x {inner} calls)  "
                    f"{nbytes / med / 1e9:8.1f} GB/s = {nbytes / med / HBM_PEAK:6.4f} of the HBM peak   {med / meds[0]:7.2f}x seg_confusion")
            say(f"{name}: ratios: bincount / seg_confusion {meds[1] / meds[0]:.2f}, seg_confusion / seg_areas {meds[0] / meds[2]:.2f}; "
                f"peak allocation of one call: seg_confusion {peak_of(ways[0][1]) / 2**20:.1f} MiB, bincount {peak_of(by_bincount) / 2**20:.1f} MiB")


def wide_post_ways(model, text, n_images=64):
    """-> (the pairs (what, call on the uint8 maps, call on their int16 copies), the pixels of the maps)"""
    from segclip_amd.segmentation import Boundary, boundary_areas, components, despeckle
    seg, _, _, gts, maps = objects_maps(model, text, n_images)
    maps = [m.clone() for m in maps]
    pixels = sum(int(m.numel()) for m in maps)
    wide, wide_gts = [m.to(torch.int16) for m in maps], [g.to(torch.int16) for g in gts]
    C, b = seg.num_classes, Boundary()
    pairs = [("components()", lambda m, g: components(m, max_objects=pixels).records),
             ("despeckle(min_area=16)", lambda m, g: torch.cat([c.reshape(-1) for c in despeckle(m, 16)])),
             ("despeckle(min_area=16, merge=True)", lambda m, g: torch.cat([c.reshape(-1) for c in despeckle(m, 16, merge=True)])),
             ("boundary_areas()", lambda m, g: boundary_areas(m, g, C, b))]
    ways = [(what, (lambda fn=fn: fn(maps, gts)), (lambda fn=fn: fn(wide, wide_gts))) for what, fn in pairs]
    return ways, pixels


def wide_post_case(model, text, n_images=64):
    from tools import rocprof_roofline as rr
    name = f"(xiv) wide-post {n_images} mixed sizes"
    ways, pixels = wide_post_ways(model, text, n_images)
    with torch.no_grad():
        for what, narrow, wide in ways:
            a, b = narrow(), wide()
            assert torch.equal(a.to(torch.int64), b.to(torch.int64)), f"{what}: the int16 maps give another result"
        torch.cuda.synchronize()
        ts = [([], []) for _ in ways]
        sampler = ClockSampler().start()
        for _ in range(REPS):
            for k, (_, narrow, wide) in enumerate(ways):
                for side, fn in enumerate((narrow, wide)):
                    t0 = time.perf_counter()
                    for _ in range(4):
                        fn()
                    torch.cuda.synchronize()
                    ts[k][side].append((time.perf_counter() - t0) / 4)
        clk = sampler.stop()
    say(f"{name}: {pixels} pixels in the label maps of update_raw and in their int16 copies (values below 256: equal results, checked); "
        f"{REPS} repeats x 4 calls, the calls alternating within each repeat; clock {clk}")
    for (what, _, _), (t8, t16) in zip(ways, ts):
        m8, m16 = statistics.median(t8), statistics.median(t16)
        say(f"{name}: {what:38s} uint8 {m8 * 1e3:8.3f} ms (min {min(t8) * 1e3:.3f}, max {max(t8) * 1e3:.3f})   int16 {m16 * 1e3:8.3f} ms "
            f"(min {min(t16) * 1e3:.3f}, max {max(t16) * 1e3:.3f})   int16 / uint8 {m16 / m8:.3f}")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        try:
            rc, _, err = rr.run_child([os.path.abspath(__file__), "--wide-post-child"], tmp)
            db = rr.find_db(tmp)
            table = rr.kernel_table(db) if rc == 0 and db else []
        except Exception as e:   # no rocprofv3 on the box
            rc, err, table = -1, repr(e), []
    rows = [r for r in table if any(tag in r[0] for tag in ("seg_cc_", "seg_sieve_", "seg_bd_"))]
    if not rows:
        say(f"{name}: the kernels alone: unmeasured (rocprofv3 child rc={rc}: {err[-200:]})")
    for r in rows:
        start = min(r[0].find(tag) for tag in ("seg_cc_", "seg_sieve_", "seg_bd_") if tag in r[0])
        say(f"{name}: {r[0][start:][:52]:52s} alone (rocprofv3 --kernel-trace --stats, {r[1]} launches in the child's 5 calls of each) "
            f"{r[2] / r[1]:9.1f} us per launch")


def wide_post_child(model, text):
    """Five calls of each of wide_post_case's calls on both widths: what its rocprofv3 child traces."""
    ways, _ = wide_post_ways(model, text)
    with torch.no_grad():
        for _, narrow, wide in ways:
            for _ in range(5):
                narrow()
                wide()
    torch.cuda.synchronize()


def snap_inputs(model, text, n_images=64):
    """-> (seg, transform, raws, gts, update_raw's label maps as clones) on the inputs of --raw"""
    from segclip_amd.segmentation import ImageTransform, SegEvaluator
    seg = SegInference(model, text, True, bg_thresh=0.80, mode="slide", crop_size=(224, 224), stride=(224, 224))
    tf = ImageTransform()
    raws, gts = raw_inputs(seg, n_images)
    with torch.no_grad():
        maps = [m.clone() for m in SegEvaluator(seg).update_raw(raws, gts, tf, return_labels=True)]
    return seg, tf, raws, gts, maps


def snap_case(model, text, n_images=64):
    import numpy as np
    from segclip_amd.segmentation import SegEvaluator, Snap, snap_labels, superpixels
    from tests import superpixel_reference as sr
    from tools import rocprof_roofline as rr
    name = f"(xv) snap   {n_images} mixed sizes"
    seg, tf, raws, gts, maps = snap_inputs(model, text, n_images)
    snap, C = Snap(), seg.num_classes
    sp = snap.superpixels
    pixels = sum(int(m.numel()) for m in maps)
    ev = SegEvaluator(seg)
    with torch.no_grad():
        segments = superpixels(raws, sp)
    k_total = sum(segments.counts)
    ways = [("update_raw", lambda: ev.update_raw(raws, gts, tf)),
            ("update_raw(snap=Snap())", lambda: ev.update_raw(raws, gts, tf, snap=snap)),
            ("superpixels alone", lambda: superpixels(raws, sp)),
            ("snap_labels alone", lambda: snap_labels(maps, segments, C, min_share=snap.min_share))]
    with torch.no_grad():
        for _, fn in ways:
            fn()
            fn()
        torch.cuda.synchronize()
        ts = [[] for _ in ways]
        sampler = ClockSampler().start()
        for _ in range(REPS):   # alternating: every repeat times the four ways one after the other
            for k, (_, fn) in enumerate(ways):
                t0 = time.perf_counter()
                fn()
                fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) / 2)
        clk = sampler.stop()
        snapped = snap_labels(maps, segments, C, min_share=snap.min_share)
        moved = sum(int((a != b).sum()) for a, b in zip(snapped, maps))
    meds = [statistics.median(t) for t in ts]
    say(f"{name}: {pixels} pixels, {C} classes, Snap(Superpixels(step={sp.step}, compactness={sp.compactness}, iters={sp.iters}), "
        f"min_share={snap.min_share}): {k_total} superpixels; {REPS} repeats x 2 calls, the ways alternating within each repeat; clock {clk}")
    for (what, _), t, med in zip(ways, ts, meds):
        say(f"{name}: {what:26s} {med * 1e3:8.2f} ms (min {min(t) * 1e3:.2f}, max {max(t) * 1e3:.2f})  {n_images / med:8.1f} images/s")
    say(f"{name}: update_raw(snap=) / update_raw {meds[1] / meds[0]:.4f}; the stage moves {moved} of {pixels} labels "
        f"({moved / pixels:.4f}; random pictures under the label maps of synthetic weights)")
    say(f"{name}: peak allocation beyond the inputs: superpixels {peak_of(ways[2][1]) / 2 ** 20:.1f} MiB (4 B of ids per pixel + 44 B per "
        f"centre), snap_labels {peak_of(ways[3][1]) / 2 ** 20:.1f} MiB (the ids at the labels' offsets, the output and "
        f"{k_total * (C + 1) * 4 / 2 ** 20:.1f} MiB of counts and winners)")
    # the host route: the numpy restatement on .cpu() copies of 8 maps
    n_host = min(8, n_images)
    t0 = time.perf_counter()
    for r, m in zip(raws[:n_host], maps[:n_host]):
        ids, cen = sr.slic(r.cpu().numpy(), sp.step, sp.compactness, sp.iters)
        torch.from_numpy(sr.vote(m.cpu().numpy(), ids, cen.shape[0], C, snap.min_share)).cuda()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) * n_images / n_host
    say(f"{name}: host route (numpy restatement on .cpu() copies, {n_host} maps scaled to {n_images}) {host * 1e3:10.1f} ms = "
        f"{host / (meds[2] + meds[3]):.0f} x superpixels + snap_labels")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        try:
            rc, _, err = rr.run_child([os.path.abspath(__file__), "--snap-child"], tmp)
            db = rr.find_db(tmp)
            table = rr.kernel_table(db) if rc == 0 and db else []
        except Exception as e:   # no rocprofv3 on the box
            rc, err, table = -1, repr(e), []
    rows = [r for r in table if any(tag in r[0] for tag in ("seg_sp_", "seg_vote_"))]
    if not rows:
        say(f"{name}: the kernels alone: unmeasured (rocprofv3 child rc={rc}: {err[-200:]})")
    raw_bytes = sum(int(r.numel()) for r in raws)
    design = {"seg_sp_assign_kernel<false>": raw_bytes, "seg_sp_assign_kernel<true>": raw_bytes + 4 * pixels,
              "seg_vote_count_kernel": 5 * pixels, "seg_vote_apply_kernel": 6 * pixels, "seg_vote_winner_kernel": k_total * (C + 1) * 4}
    for r in rows:
        start = min(r[0].find(tag) for tag in ("seg_sp_", "seg_vote_") if tag in r[0])
        kernel = r[0][start:]
        avg_us = r[2] / r[1]
        note = ""
        for key, nbytes in design.items():
            if kernel.startswith(key):   # an instantiation of the assignment by its template argument, the others by name
                note = f"  design traffic {nbytes} B = {nbytes / avg_us / 1e6:.3f} TB/s ({nbytes / avg_us * 1e6 / HBM_PEAK:.3f} of the HBM peak)"
        say(f"{name}: {kernel[:48]:48s} alone (rocprofv3 --kernel-trace --stats, {r[1]} launches in the child's 5 calls of each) "
            f"{avg_us:9.1f} us per launch{note}")


def snap_child(model, text):
    """Five calls of superpixels and of snap_labels and nothing else: what the rocprofv3 child of snap_case traces."""
    from segclip_amd.segmentation import Snap, snap_labels, superpixels
    seg, _, raws, _, maps = snap_inputs(model, text)
    snap = Snap()
    with torch.no_grad():
        for _ in range(5):
            segments = superpixels(raws, snap.superpixels)
            snap_labels(maps, segments, seg.num_classes, min_share=snap.min_share)
    torch.cuda.synchronize()


def per_image_case(model, text, n_images=64):
    """(xvi) image_areas against one seg_areas call per picture, and update_raw with and without per_image=True."""
    from segclip_amd.segmentation import SegEvaluator, _Maps, image_areas
    seg, tf, raws, gts, maps = objects_maps(model, text, n_images)
    batch = _Maps.of(maps)   # update_raw's label buffer: views, every map at a multiple of 4
    assert batch.flat.data_ptr() == min(m.data_ptr() for m in maps), "the maps are not read where they lie"
    pixels = sum(h * w for h, w in batch.sizes)
    shifted = []
    for m in maps:   # the annotation of a prediction: the map moved by (3, 2), a band ignored
        t = torch.roll(m, (3, 2), (0, 1)).clone()
        t[:4] = 255
        shifted.append(t)
    wide_flat = batch.flat.to(torch.int16)
    wide_maps = _Maps(wide_flat, batch.offs, batch.sizes).views()
    verdicts = []
    for dtype, classes in ((torch.uint8, (21, 151)), (torch.int16, (21, 151, 460, 848))):
        wide = dtype == torch.int16
        preds, flat = (wide_maps, wide_flat) if wide else (maps, batch.flat)
        ignore = 65535 if wide else 255
        areas_fn = ops.seg_areas_wide if wide else ops.seg_areas
        for truth_name, truth in (("noise truth", gts), ("shifted maps", shifted)):
            # 255 -> 65535: the ignored band stays ignored in the int16 copies
            truth = [torch.where(t == 255, -1, t.to(torch.int16)).to(torch.int16) for t in truth] if wide else truth
            gt_flat, gt_offs = _Maps.gapless_of(truth)
            table, n_blocks = ops.seg_image_areas_table(batch.offs, gt_offs, [h * w for h, w in batch.sizes], "cuda")
            for C in classes:
                name = f"(xvi) per-image {'int16' if wide else 'uint8'} C={C:4d} {truth_name:12s}"
                rows = torch.zeros(n_images, 3, C, dtype=torch.int64, device="cuda")
                alone = torch.zeros_like(rows)
                kept = {}

                def one_call():
                    kept["rows"] = image_areas(preds, truth, C, ignore)

                def per_picture():
                    for i, (p, t) in enumerate(zip(preds, truth)):
                        areas_fn(p.reshape(-1), t.reshape(-1), C, ignore, areas=rows[i])

                ways = [("segmentation.image_areas: one call, one launch", one_call, 10),
                        ("ops.seg_image_areas alone, table and flat truths made beforehand",
                         lambda: ops.seg_image_areas(flat, gt_flat, table, n_blocks, C, ignore, out=alone), 10),
                        (f"one {'ops.seg_areas_wide' if wide else 'ops.seg_areas'} call per picture ({n_images} launches)", per_picture, 3)]
                with torch.no_grad():
                    for _, fn, _ in ways:
                        fn()
                    torch.cuda.synchronize()
                    say(f"{name}: the rows of the one call equal those of the per-picture loop: {bool(torch.equal(kept['rows'], rows))}; "
                        f"of the launch alone: {bool(torch.equal(alone, rows))}; {int((rows[:, 2] > 0).sum())} (picture, class) pairs labelled")
                    for _ in range(2):
                        for _, fn, _ in ways:
                            fn()
                    torch.cuda.synchronize()
                    ts = [[] for _ in ways]
                    sampler = ClockSampler().start()
                    for _ in range(REPS):   # alternating: every repeat times the ways one after the other
                        for i, (_, fn, inner) in enumerate(ways):
                            t0 = time.perf_counter()
                            for _ in range(inner):
                                fn()
                            torch.cuda.synchronize()
                            ts[i].append((time.perf_counter() - t0) / inner)
                    clk = sampler.stop()
                meds = [statistics.median(t) for t in ts]
                nbytes = 2 * pixels * flat.element_size()
                say(f"{name}: {n_images} pictures, {pixels} pixels, {n_blocks} workgroups, {nbytes / 2**20:.1f} MiB read per call; clock {clk}")
                for (what, _, inner), t, med in zip(ways, ts, meds):
                    say(f"{name}: {what:70s} {med * 1e6:10.1f} us (min {min(t) * 1e6:.1f}, max {max(t) * 1e6:.1f}; {REPS} x {inner} calls)  "
                        f"{nbytes / med / 1e9:8.1f} GB/s = {nbytes / med / HBM_PEAK:6.4f} of the HBM peak   {med / meds[2]:6.3f}x the loop")
                slower = min(ts[0]) > max(ts[2])
                verdicts.append(slower)
                say(f"{name}: loop / one call {meds[2] / meds[0]:.2f}, loop / launch alone {meds[2] / meds[1]:.2f}; the one call is "
                    f"{'SLOWER than the loop outside both min-max ranges' if slower else 'not slower than the loop outside the runs min-max'}")
    say(f"(xvi) per-image: the one call slower than the per-picture loop outside the min-max ranges in {sum(verdicts)} of {len(verdicts)} cases")
    # the evaluator: update_raw without the feature (the yardstick) and with it
    name = f"(xvi) per-image update_raw {n_images} mixed sizes"
    ev0, ev1 = SegEvaluator(seg), SegEvaluator(seg, per_image=True)

    def with_rows():
        ev1.reset()   # the rows of earlier calls are not kept: the same work every call
        ev1.update_raw(raws, gts, tf)

    ways = [("SegEvaluator.update_raw", lambda: ev0.update_raw(raws, gts, tf), 2),
            ("SegEvaluator(per_image=True).update_raw", with_rows, 2)]
    with torch.no_grad():
        for _ in range(3):
            for _, fn, _ in ways:
                fn()
        torch.cuda.synchronize()
        ev0.reset()
        ev0.update_raw(raws, gts, tf)
        say(f"{name}: the rows sum to the areas of the evaluator without them: {bool(torch.equal(ev1.image_areas.sum(0), ev0.areas))}; "
            f"rows {tuple(ev1.image_areas.shape)}")
        ts = [[] for _ in ways]
        sampler = ClockSampler().start()
        for _ in range(REPS):
            for i, (_, fn, inner) in enumerate(ways):
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                ts[i].append((time.perf_counter() - t0) / inner)
        clk = sampler.stop()
    meds = [statistics.median(t) for t in ts]
    for (what, _, inner), t, med in zip(ways, ts, meds):
        say(f"{name}: {what:42s} {med * 1e3:8.3f} ms (min {min(t) * 1e3:.3f}, max {max(t) * 1e3:.3f}; {REPS} x {inner} calls)   clock {clk}")
    say(f"{name}: per_image=True adds {(meds[1] - meds[0]) * 1e3:+.3f} ms = {(meds[1] / meds[0] - 1) * 100:+.2f} %; update_raw's own "
        f"max - min is {(max(ts[0]) - min(ts[0])) * 1e3:.3f} ms; peak allocation of one call: without {peak_of(ways[0][1]) / 2**20:.1f} MiB, "
        f"with {peak_of(ways[1][1]) / 2**20:.1f} MiB")


def write_out():
    """the lines of this run into OUT; --wide-post and --per-image keep what stands above their mark (the kernels' resource
    tables, the tile measurements)"""
    head = []
    mark = WIDE_POST_MARK if WIDE_POST else PER_IMAGE_MARK if PER_IMAGE else None
    if mark is not None:
        if os.path.exists(OUT):
            old = open(OUT).read().split("\n")
            head = old[:old.index(mark)] if mark in old else old
        head.append(mark)
    with open(OUT, "w") as f:
        f.write("\n".join(head + lines) + "\n")


if __name__ == "__main__":
    segclip_amd.set_compute_dtype(torch.bfloat16)
    model, _ = synth.build_model(synth.SPECS["vitb16"], {}, device="cuda")
    model.eval()
    g = torch.Generator().manual_seed(0)
    text = torch.randn(20, 512, generator=g)
    text = (text / text.norm(dim=-1, keepdim=True)).cuda()
    say(f"# tools/bench_seg.py  ViT-B/16 synthetic weights, bf16 towers, 20 classes + background, {torch.cuda.get_device_name(0)}")
    if RAW_CHILD:
        raw_child(model, text)
        sys.exit(0)
    if AUG_CHILD:
        aug_child(model, text)
        sys.exit(0)
    if SWEEP_CHILD:
        sweep_child(model, text)
        sys.exit(0)
    if REFINE_CHILD:
        refine_child(model, text)
        sys.exit(0)
    if OBJECTS_CHILD:
        objects_child(model, text)
        sys.exit(0)
    if BOUNDARY_CHILD:
        boundary_child(model, text)
        sys.exit(0)
    if MERGE_CHILD:
        merge_child(model, text)
        sys.exit(0)
    if WIDE_POST_CHILD:
        wide_post_child(model, text)
        sys.exit(0)
    if SNAP_CHILD:
        snap_child(model, text)
        sys.exit(0)
    if PER_IMAGE:
        per_image_case(model, text)
    elif SNAP:
        snap_case(model, text)
    elif WIDE_POST:
        wide_post_case(model, text)
    elif CONFUSION:
        confusion_case(model)
    elif MERGE:
        merge_case(model, text)
    elif WIDE:
        wide_case(model)
    elif BOUNDARY:
        boundary_case(model, text)
    elif OBJECTS:
        objects_case(model, text)
    elif REFINE:
        refine_case(model, text)
    elif SWEEP:
        sweep_case(model, text)
    elif AUG:
        aug_case(model, text)
    elif RAW:
        raw_case(model, text)
    elif EVAL:
        eval_case(model, text)
    else:
        case("(i)  whole  B=64 224x224", model, text, 64, 224, 224, 3)
        case("(ii) slide  B=16 448x672", model, text, 16, 448, 672, 2, mode="slide", crop_size=(224, 224), stride=(224, 224))
    if OUT:
        write_out()
