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
an entry of the list plan, so the windows of all views share the tower calls, and one kernel (csrc/segment_aug.inc) rescales
every view's logits, takes their soft-max, mirrors, averages and takes the first maximum per output pixel.

Deviations from the reference.  mmseg takes a softmax between the resize and the arg-max; without augmentation the arg-max
is taken of the logits here, which can differ only where fp32 exp rounds two different logits to one value (the augmented
path takes the soft-max mmseg takes: the mean over views needs it).  A ground-truth value of 255 stays
ignored whatever reduce_zero_label says.  The resized pixel is kept in fp32 and not rounded back to uint8 as cv2's 8-bit
fixed-point resize does: about one grey level, 0.015 in normalised units (unmeasured: cv2 is not a dependency).  The overlay
is drawn on the decoded image itself, where the reference draws on a de-normalised copy of the network input resized back
to the picture's size.  Text is not drawn: input_pred_label returns the anchor positions beside the overlay.
"""
import colorsys
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


def _raw_sizes(raws, transform, net_sizes):
    """Checks of a list of decoded images -> their network sizes [(H, W)]."""
    if len(raws) == 0:
        raise ValueError("empty image list")
    if not isinstance(transform, ImageTransform):
        raise TypeError("transform is an ImageTransform")
    for t in raws:
        if not t.is_cuda:
            raise RuntimeError(f"segclip_amd: HIP kernels need device tensors (there is no CPU fallback); got a {t.device} tensor")
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8:
            raise ValueError(f"a decoded image is an (h, w, 3) uint8 tensor, got {t.dtype} {tuple(t.shape)}")
    if net_sizes is None:
        return [transform.net_size(int(t.shape[0]), int(t.shape[1])) for t in raws]
    if len(net_sizes) != len(raws):
        raise ValueError(f"{len(raws)} images but {len(net_sizes)} network sizes")
    return [(int(a), int(b)) for (a, b) in net_sizes]


def _raw_windows(raws, transform, sizes, table, dwin, wh, ww):
    return ops.seg_windows_from_u8(raws, sizes, dwin, (wh, ww), transform.mean, transform.inv_std,
                                   reverse_channels=transform.channel_order == "bgr", table=table)


@torch.no_grad()
def preprocess(raws, transform, net_sizes=None):
    """[(h_i, w_i, 3) uint8] -> [(3, H_i, W_i) fp32]: every image resized to its network size (transform.net_size, or
    net_sizes) and normalised, by the kernel of predict_raw with one whole-image window per image, one launch per distinct
    size.  predict_list on the result equals predict_raw on the raw images bit for bit; predict_raw does not form it."""
    sizes = _raw_sizes(raws, transform, net_sizes)
    table = ops.seg_source_table(raws, sizes)
    by_size = {}
    for i, hw in enumerate(sizes):
        by_size.setdefault(hw, []).append(i)
    out = [None] * len(raws)
    for (H, W), members in by_size.items():
        x = _raw_windows(raws, transform, sizes, table, [(i, 0, 0) for i in members], H, W)
        for k, i in enumerate(members):
            out[i] = x[k]
    return out


class _SlicedImages:
    """The tower input of _list_forward from images already resized and normalised: one slice per window."""

    def __init__(self, model, imgs):
        if len(imgs) == 0:
            raise ValueError("empty image list")
        for t in imgs:
            _require_eval_gpu(model, t)
            if t.dim() != 3 or t.shape[0] != 3:
                raise ValueError(f"predict_list takes (3, H, W) images, got {tuple(t.shape)}")
        self.imgs, self.device = imgs, imgs[0].device
        self.sizes = [(int(t.shape[1]), int(t.shape[2])) for t in imgs]
        self.default_out = self.sizes

    def windows(self, chunk, dwin, wh, ww):
        return torch.stack([self.imgs[i][:, y:y + wh, x0:x0 + ww] for (i, y, x0) in chunk])


class _RawImages:
    """The tower input of _list_forward from decoded uint8 images: the front-end kernel writes a chunk's windows."""

    def __init__(self, model, raws, transform, net_sizes):
        self.sizes = _raw_sizes(raws, transform, net_sizes)
        _require_eval_gpu(model, raws[0])
        self.raws, self.transform, self.device = raws, transform, raws[0].device
        self.default_out = [(int(t.shape[0]), int(t.shape[1])) for t in raws]   # mmseg's ori_shape
        self.table = ops.seg_source_table(raws, self.sizes)

    def windows(self, chunk, dwin, wh, ww):
        return _raw_windows(self.raws, self.transform, self.sizes, self.table, dwin, wh, ww)


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


class _Views:
    """Bookkeeping of the (image, view) entries of a list plan: entry e = view e - first[i] of image i."""

    def _set_views(self, counts):
        self.view_counts = counts
        self.owner = [(i, v) for i, n in enumerate(counts) for v in range(n)]

    def name(self, e):
        return "image %d view %d" % self.owner[e]


class _SlicedViews(_Views):
    """The tower input from views already resized, normalised and flipped (what mmseg hands to aug_test)."""

    def __init__(self, model, views):
        if len(views) == 0:
            raise ValueError("empty image list")
        self.imgs, self.flags = [], []
        for i, per in enumerate(views):
            if len(per) == 0:
                raise ValueError(f"image {i}: no views")
            for v, (t, flags) in enumerate(per):
                _require_eval_gpu(model, t)
                if t.dim() != 3 or t.shape[0] != 3:
                    raise ValueError(f"image {i} view {v}: a view is a (3, H, W) tensor, got {tuple(t.shape)}")
                if int(flags) not in (0, 1, 2, 3):
                    raise ValueError(f"image {i} view {v}: flags {flags}, bit 0 = horizontal flip and bit 1 = vertical flip")
                self.imgs.append(t)
                self.flags.append(int(flags))
        self._set_views([len(per) for per in views])
        self.device = self.imgs[0].device
        self.sizes = [(int(t.shape[1]), int(t.shape[2])) for t in self.imgs]
        self.default_out = None

    def windows(self, chunk, dwin, wh, ww):
        return torch.stack([self.imgs[e][:, y:y + wh, x0:x0 + ww] for (e, y, x0) in chunk])


class _RawViews(_Views):
    """The tower input from decoded uint8 images and an augmentation: the view kernel of the front end resizes, normalises
    and mirrors a chunk's windows; neither a resized nor a flipped image exists."""

    def __init__(self, model, raws, transform, aug, net_sizes):
        if not isinstance(aug, TestAug):
            raise TypeError("aug is a TestAug")
        _raw_sizes(raws, transform, None)
        _require_eval_gpu(model, raws[0])
        lists = [aug.views(int(t.shape[0]), int(t.shape[1]), transform) for t in raws]
        if net_sizes is not None:   # per image one (H, W) per view, in the order of aug.views
            if len(net_sizes) != len(raws) or any(len(a) != len(b) for a, b in zip(net_sizes, lists)):
                raise ValueError("with aug, net_sizes holds one (H, W) per view of every image")
            lists = [[(int(H), int(W), f) for (H, W), (_, _, f) in zip(a, b)] for a, b in zip(net_sizes, lists)]
        self._set_views([len(per) for per in lists])
        self.sizes = [(H, W) for per in lists for (H, W, _) in per]
        self.flags = [f for per in lists for (_, _, f) in per]
        self.raws = [raws[i] for i, _ in self.owner]
        self.transform, self.device = transform, raws[0].device
        self.default_out = [(int(t.shape[0]), int(t.shape[1])) for t in raws]   # mmseg's ori_shape
        self.table = ops.seg_view_source_table(self.raws, self.sizes, self.flags)

    def windows(self, chunk, dwin, wh, ww):
        t = self.transform
        return ops.seg_view_windows_from_u8(self.raws, self.sizes, self.flags, dwin, (wh, ww), t.mean, t.inv_std,
                                            reverse_channels=t.channel_order == "bgr", table=self.table)


def _require_eval_gpu(model, t):
    if not t.is_cuda:
        raise RuntimeError(f"segclip_amd: HIP kernels need device tensors (there is no CPU fallback); got a {t.device} tensor")
    if model.training:
        raise RuntimeError("segclip_amd.segmentation: call model.eval() first (training mode draws Gumbel noise)")


def build_text_embedding(model, text_tokens, chunk=1024):
    """(N, T, L) int64 prompt ids (N classes x T templates) -> (N, C): encode_text, mean over the templates, L2 norm
    (evaluation/builder.py:59-66).  The N * T captions go through the text tower `chunk` rows at a time."""
    _require_eval_gpu(model, text_tokens)
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
    encode_image call (at most `max_windows` at a time)."""

    def __init__(self, model, text_embedding, with_bg, bg_thresh=0.95, mode="whole", crop_size=(224, 224), stride=(224, 224),
                 max_windows=256):
        if mode not in ("whole", "slide"):
            raise ValueError(f"mode must be 'whole' or 'slide', got {mode!r}")
        if not text_embedding.is_cuda:
            raise RuntimeError("segclip_amd: HIP kernels need device tensors (there is no CPU fallback); got a "
                               f"{text_embedding.device} text embedding")
        self.model = model
        self.text_embedding = text_embedding.detach().float().contiguous()
        self.with_bg, self.bg_thresh, self.mode = bool(with_bg), float(bg_thresh), mode
        self.crop_size, self.stride, self.max_windows = tuple(crop_size), tuple(stride), int(max_windows)
        self.num_classes = self.text_embedding.shape[0] + int(self.with_bg)
        self._lists = {}

    def window_list(self, B, H, W):
        """(windows [(image, y0, x0)], (win_h, win_w)) of a (B, 3, H, W) batch."""
        if self.mode == "whole":
            return [(b, 0, 0) for b in range(B)], (H, W)
        per = slide_windows(H, W, self.crop_size, self.stride)
        return [(b, y, x) for b in range(B) for (y, x) in per], self.crop_size

    def _device_lists(self, B, H, W, device):
        """The window list on the device; the last (B, H, W) is kept (a dataset of varying sizes does not accumulate lists)."""
        key = (B, H, W, str(device))
        if self._lists.get("key") != key:
            wins, size = self.window_list(B, H, W)
            per = len(wins) // B
            if per > 64:
                raise ValueError(f"slide mode: {per} windows per image, at most 64 supported")
            self._lists = dict(key=key, value=(wins, size, torch.tensor(wins, dtype=torch.int32, device=device).view(-1, 3),
                                               torch.arange(0, len(wins) + 1, per, dtype=torch.int32, device=device)))
        return self._lists["value"]

    def _windows_forward(self, img, with_tables=True):
        """Vision tower + group tables of every window -> the pixel kernels' arguments.  with_tables=False (group_map: the
        groups do not depend on the classes): zero tables of one class instead of segclip_seg_group_table."""
        _require_eval_gpu(self.model, img)
        B, _, H, W = img.shape
        if B == 0:
            raise ValueError("empty image batch")
        p = self.model.clip.visual.patch_size
        wins, (wh, ww), dwin, dfirst = self._device_lists(B, H, W, img.device)
        if wh % p or ww % p:
            raise ValueError(f"window {wh}x{ww} is not a multiple of the patch size {p}")
        grid = (wh // p, ww // p)
        N = self.text_embedding.shape[0]
        topk = min(5, N)
        nW = len(wins)
        parts = []
        for s in range(0, nW, self.max_windows):
            e = min(s + self.max_windows, nW)
            if self.mode == "whole":
                x = img[s:e]
            else:
                x = torch.stack([img[b, :, y:y + wh, x0:x0 + ww] for (b, y, x0) in wins[s:e]])
            # the reference segments one image per call, where the two key layouts of the cross-attention block coincide;
            # in a batch only "intended" keeps every window attending to its own tokens (config.py, SURVEY finding 0.4)
            with config.scope(cross_mode="intended"):
                feat, hidden, mid = self.model.clip.encode_image(x, return_hidden=True)
            if not mid["attns"]:
                raise ValueError(f"window {wh}x{ww}: the vision tower takes its segmentation branch only at 1x or 4x the "
                                 "training token count (modules/module_seg_vit.py:423)")
            soft = mid["attns"][-1]["soft_attn"]
            del mid, x
            if with_tables:
                tables = ops.seg_group_table(hidden[:, 1:, :], feat, self.text_embedding, self.model.clip.logit_scale, topk)
            else:
                n, G = soft.shape[0], soft.shape[1]
                tables = (soft.new_zeros(n, G, 1), soft.new_zeros(n), soft.new_zeros(n, G, dtype=torch.int32), soft.new_zeros(n, G))
            parts.append((soft,) + tables)
        if len(parts) == 1:
            soft, tables = parts[0][0], parts[0][1:]
        else:
            cat = [torch.cat([q[i] for q in parts]) for i in range(5)]
            soft, tables = cat[0], tuple(cat[1:])
        return soft, tables, dwin, dfirst, (B, H, W), (wh, ww), grid

    @torch.no_grad()
    def predict(self, img):
        """(B, 3, H, W) -> (B, H, W) uint8 labels (class 0 = background when with_bg)."""
        if self.num_classes > 256:
            raise ops.L.Unsupported(f"predict: {self.num_classes} classes do not fit a uint8 label map; use encode_decode")
        soft, tables, dwin, dfirst, size, win, grid = self._windows_forward(img)
        return ops.seg_label_map(soft, tables, dwin, dfirst, size, win, grid, self.with_bg, self.bg_thresh)[0]

    @torch.no_grad()
    def group_map(self, img):
        """(B, 3, H, W) -> (B, H, W) uint8: the group of every pixel (in its first covering window)."""
        soft, tables, dwin, dfirst, size, win, grid = self._windows_forward(img, with_tables=False)
        return ops.seg_label_map(soft, tables, dwin, dfirst, size, win, grid, self.with_bg, self.bg_thresh, labels=False,
                                 groups=True)[1]

    @torch.no_grad()
    def encode_decode(self, img):
        """(B, 3, H, W) -> (B, N + with_bg, H, W) fp32 logits (vit_seg.py:202-256; any batch size)."""
        soft, tables, dwin, dfirst, size, win, grid = self._windows_forward(img)
        return ops.seg_logits(soft, tables, dwin, dfirst, size, win, grid, self.with_bg, self.bg_thresh)

    # ------------------------------------------------------------------------------------------ images of mixed sizes
    def _list_plan(self, sizes):
        """Windows of a list of image sizes -> (batches [(win size, [(image, y0, x0)])] in tower order, per-image
        (first window, window count, win size)).  Slide mode: one batch of all windows; whole mode: one batch per size."""
        per_image = [None] * len(sizes)
        if self.mode == "slide":
            wins = []
            for i, (H, W) in enumerate(sizes):
                per = slide_windows(H, W, self.crop_size, self.stride)
                if len(per) > 64:
                    raise ValueError(f"slide mode: {len(per)} windows per image, at most 64 supported")
                per_image[i] = (len(wins), len(per), self.crop_size)
                wins += [(i, y, x) for (y, x) in per]
            return [(self.crop_size, wins)], per_image
        by_size = {}
        for i, hw in enumerate(sizes):
            by_size.setdefault(hw, []).append(i)
        batches, n = [], 0
        for hw, members in by_size.items():
            for k, i in enumerate(members):
                per_image[i] = (n + k, 1, hw)
            batches.append((hw, [(i, 0, 0) for i in members]))
            n += len(members)
        return batches, per_image

    def _list_towers(self, src, classes=True, plan=None):
        """The tower part of a list call: every window of the plan (_list_plan(src.sizes) unless the caller has it) through
        encode_image (max_windows at a time) and, with `classes`, segclip_seg_group_table.  -> (flat soft_attn, tables, device
        window list, per-entry (first window, window count, win size), a window's offset in soft_attn, group count)."""
        name = getattr(src, "name", None)
        p = self.model.clip.visual.patch_size
        batches, per_image = self._list_plan(src.sizes) if plan is None else plan
        N = self.text_embedding.shape[0]
        dev = src.device
        for (wh, ww), wins in batches:
            if wh % p or ww % p:
                raise ValueError((f"{name(wins[0][0])}: " if name else "") + f"window {wh}x{ww} is not a multiple of the patch size {p}")
        wins_all = [w for _, wins in batches for w in wins]
        dwin = torch.tensor(wins_all, dtype=torch.int32, device=dev).view(-1, 3)
        parts, done, win_off, floats = [], 0, [], 0   # win_off: a window's offset in the flat soft_attn
        for (wh, ww), wins in batches:
            for s in range(0, len(wins), self.max_windows):
                chunk = wins[s:s + self.max_windows]
                x = src.windows(chunk, dwin[done + s:done + s + len(chunk)], wh, ww)
                with config.scope(cross_mode="intended"):   # see _windows_forward
                    feat, hidden, mid = self.model.clip.encode_image(x, return_hidden=True)
                if not mid["attns"]:
                    raise ValueError((f"{name(chunk[0][0])}: " if name else "") +
                                     f"window {wh}x{ww}: the vision tower takes its segmentation branch only at 1x or 4x the "
                                     "training token count (modules/module_seg_vit.py:423)")
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
        return soft, tables, dwin, per_image, win_off, n_groups

    def _list_forward(self, src, out_shapes, gts=None, areas=None, ignore_index=255, reduce_zero_label=False, want_labels=True,
                      groups=None):
        """src: _SlicedImages or _RawImages - the network sizes of the images and the tower input of a chunk of windows.
        groups: None, "also" (-> (labels, group maps, G), both at out_shapes, from the same pass of the tower) or "only"
        (-> (None, group maps, G): no class tables, no label map)."""
        sizes, n_img = src.sizes, len(src.sizes)
        if out_shapes is None:
            out_shapes = src.default_out
        if len(out_shapes) != n_img:
            raise ValueError(f"{n_img} images but {len(out_shapes)} output shapes")
        out_shapes = [(int(a), int(b)) for (a, b) in out_shapes]
        classes = groups != "only"
        if classes and self.num_classes > 256:
            raise ops.L.Unsupported(f"{self.num_classes} classes do not fit a uint8 label map; use encode_decode")
        p = self.model.clip.visual.patch_size
        plan = self._list_plan(sizes)
        if groups is not None:
            for i, (_, count, _) in enumerate(plan[1]):
                if count != 1:
                    raise ValueError(f"group maps are defined for one window per image: image {i} ({sizes[i][0]}x{sizes[i][1]}) "
                                     f"has {count} windows in slide mode")
        dev = src.device
        soft, tables, dwin, per_image, win_off, n_groups = self._list_towers(src, classes, plan)
        rows, gt_off = [], 0
        for i, (first, count, (wh, ww)) in enumerate(per_image):
            rows.append(dict(first=first, count=count, net=sizes[i], out=out_shapes[i], win=(wh, ww), grid=(wh // p, ww // p),
                             soft_off=win_off[first], gt_off=gt_off if gts is not None else -1))
            gt_off += out_shapes[i][0] * out_shapes[i][1]
        images, offs, nbytes, n_blocks, most = ops.seg_image_table(rows, dev)

        def views(flat):
            return [flat[o:o + oh * ow].view(oh, ow) for o, (oh, ow) in zip(offs, out_shapes)]

        labels = None
        if classes:
            labels = torch.empty(nbytes, dtype=torch.uint8, device=dev) if want_labels else None
            gt = None
            if gts is not None:
                gt = gts[0].reshape(-1) if len(gts) == 1 else torch.cat([g.reshape(-1) for g in gts])
            ops.seg_label_map_rescaled(soft, tables, dwin, images, n_blocks, most, self.with_bg, self.bg_thresh, labels=labels,
                                       gt=gt, areas=areas, ignore_index=ignore_index, reduce_zero_label=reduce_zero_label)
            labels = views(labels) if want_labels else None
        if groups is None:
            return labels
        # the table's label offsets and workgroup numbers serve the group maps as they are: same sizes, same tile
        gmaps = ops.seg_groups_rescaled(soft, images, n_blocks, n_groups, torch.empty(nbytes, dtype=torch.uint8, device=dev))
        return labels, views(gmaps), n_groups

    def _views_forward(self, src, out_shapes, gts=None, areas=None, ignore_index=255, reduce_zero_label=False, want_labels=True,
                       dense=False):
        """The augmented list call.  src: _SlicedViews or _RawViews - one plan entry per (image, view) pair, so the windows of
        all views share the tower calls of _list_towers; segclip_seg_label_map_views takes the place of the rescaled kernel.
        dense: -> the (C, oh, ow) fp32 mean probabilities of the single image instead of labels."""
        counts, n_img = src.view_counts, len(src.view_counts)
        if out_shapes is None:
            out_shapes = src.default_out
        if out_shapes is None or len(out_shapes) != n_img:
            raise ValueError(f"{n_img} images but {0 if out_shapes is None else len(out_shapes)} output shapes")
        out_shapes = [(int(a), int(b)) for (a, b) in out_shapes]
        if self.num_classes > 256:
            raise ops.L.Unsupported(f"{self.num_classes} classes: the multi-view kernel holds at most 256")
        if dense and n_img != 1:
            raise ValueError(f"the dense probabilities are formed for one image per call, got {n_img}")
        p = self.model.clip.visual.patch_size
        base = self.model.clip.visual.transformer.patch_len ** 2   # tokens of the training resolution
        # what a single view already requires, and the limits of the kernel's device-side lists (what exceeds them would be
        # silently ignored), before anything runs
        e0 = 0
        for i, V in enumerate(counts):
            if V > ops.SEG_MAX_VIEWS:
                raise ValueError(f"image {i}: {V} views, at most {ops.SEG_MAX_VIEWS} supported")
            n_win = 0
            for e in range(e0, e0 + V):
                try:
                    _, count, (wh, ww) = self._list_plan([src.sizes[e]])[1][0]
                except ValueError as err:
                    raise ValueError(f"{src.name(e)}: {err}") from None
                if wh % p or ww % p:
                    raise ValueError(f"{src.name(e)}: window {wh}x{ww} is not a multiple of the patch size {p}")
                if (wh // p) * (ww // p) not in (base, 4 * base):
                    raise ValueError(f"{src.name(e)}: window {wh}x{ww}: the vision tower takes its segmentation branch only at 1x "
                                     f"or 4x the training token count ({base}; modules/module_seg_vit.py:423)")
                n_win += count
            if n_win > ops.SEG_MAX_IMAGE_WINDOWS:
                raise ValueError(f"image {i}: {n_win} windows over its {V} views, at most {ops.SEG_MAX_IMAGE_WINDOWS} supported")
            e0 += V
        dev = src.device
        soft, tables, dwin, per_entry, win_off, _ = self._list_towers(src)
        rows, gt_off, e = [], 0, 0
        for i, V in enumerate(counts):
            for _ in range(V):
                first, count, (wh, ww) = per_entry[e]
                rows.append(dict(first=first, count=count, net=src.sizes[e], out=out_shapes[i], win=(wh, ww), grid=(wh // p, ww // p),
                                 soft_off=win_off[first], gt_off=gt_off if gts is not None else -1, flags=src.flags[e]))
                e += 1
            gt_off += out_shapes[i][0] * out_shapes[i][1]
        images, vtab, offs, nbytes, n_blocks, most_img, most_view, most_v = ops.seg_view_tables(rows, counts, dev)
        if dense:
            return ops.seg_view_probs(soft, tables, dwin, images, vtab, n_blocks, most_img, most_view, most_v, self.with_bg,
                                      self.bg_thresh, out_shapes[0])
        labels = torch.empty(nbytes, dtype=torch.uint8, device=dev) if want_labels else None
        gt = None
        if gts is not None:
            gt = gts[0].reshape(-1) if len(gts) == 1 else torch.cat([g.reshape(-1) for g in gts])
        ops.seg_label_map_views(soft, tables, dwin, images, vtab, n_blocks, most_img, most_view, most_v, self.with_bg, self.bg_thresh,
                                labels=labels, gt=gt, areas=areas, ignore_index=ignore_index, reduce_zero_label=reduce_zero_label)
        if not want_labels:
            return None
        return [labels[o:o + oh * ow].view(oh, ow) for o, (oh, ow) in zip(offs, out_shapes)]

    @torch.no_grad()
    def predict_list(self, imgs, out_shapes=None):
        """[(3, H_i, W_i)] of any mix of sizes -> [(oh_i, ow_i) uint8 labels], views of one flat buffer; out_shapes defaults
        to the images' own sizes.  The logits are rescaled bilinearly (align_corners=False) to the output size and the first
        maximum taken there, as mmseg's resize(size=ori_shape) + arg-max, inside one kernel launch for the whole list.
        Slide mode: the windows of all images go through encode_image max_windows at a time; whole mode: one call per size."""
        return self._list_forward(_SlicedImages(self.model, imgs), out_shapes)

    @torch.no_grad()
    def predict_raw(self, raws, transform, out_shapes=None, net_sizes=None, aug=None):
        """[(h_i, w_i, 3) uint8 decoded images] -> [(oh_i, ow_i) uint8 labels] as predict_list(preprocess(raws, transform,
        net_sizes), out_shapes), bit for bit, without the resized images: the windows of a tower call are written from the
        raw bytes by one launch of segclip_seg_windows_from_u8.  out_shapes defaults to the raw images' own sizes (mmseg's
        ori_shape); net_sizes overrides transform.net_size (whole mode needs multiples of the patch size).
        aug (a TestAug): mmseg's aug_test over the views of aug.views - every view segmented, its logits rescaled to the output
        size and passed through a soft-max, flipped back, the probabilities averaged over the views, first maximum.  net_sizes
        then holds one (H, W) per view of every image."""
        if aug is not None:
            return self._views_forward(_RawViews(self.model, raws, transform, aug, net_sizes), out_shapes)
        return self._list_forward(_RawImages(self.model, raws, transform, net_sizes), out_shapes)

    @torch.no_grad()
    def predict_views(self, views, out_shapes):
        """views[i] = [((3, H, W) tensor, flags)]: the views of image i, pre-processed and ALREADY FLIPPED as mmseg hands imgs
        and img_metas to aug_test (flags: ops.SEG_FLIP_H | ops.SEG_FLIP_V, what img_metas' flip / flip_direction say)
        -> [(oh_i, ow_i) uint8 labels] of the mean probabilities, as predict_raw(aug=)."""
        return self._views_forward(_SlicedViews(self.model, views), out_shapes)

    @torch.no_grad()
    def predict_proba_views(self, views, out_shape):
        """The views [((3, H, W) tensor, flags)] of ONE image -> (N + with_bg, oh, ow) fp32: the mean over the views of the
        soft-max of the rescaled logits, what aug_test takes the arg-max of (predict_views' label is its first maximum)."""
        return self._views_forward(_SlicedViews(self.model, [views]), [out_shape], dense=True)

    @torch.no_grad()
    def predict_proba_raw(self, raw, transform, aug=None, out_shape=None, net_sizes=None):
        """predict_proba_views from ONE decoded (h, w, 3) uint8 image; aug defaults to the single unflipped view, out_shape to
        the image's own size."""
        src = _RawViews(self.model, [raw], transform, TestAug() if aug is None else aug, None if net_sizes is None else [net_sizes])
        return self._views_forward(src, None if out_shape is None else [out_shape], dense=True)

    # ------------------------------------------------------------------------------------------ the demo's outputs
    @torch.no_grad()
    def groups_list(self, imgs, out_shapes=None):
        """[(3, H_i, W_i)] -> [(oh_i, ow_i) uint8 group maps], views of one flat buffer: the soft assignment resized to the
        network size and again to the output size, first maximum over the groups (get_attn_maps + show_result's group
        branch, vit_seg.py:144-200, :359-362), one launch for the list.  out_shapes defaults to the images' own sizes, where
        the result equals group_map's.  Every image is one window: a slide-mode image with more raises ValueError."""
        return self._list_forward(_SlicedImages(self.model, imgs), out_shapes, groups="only")[1]

    @torch.no_grad()
    def groups_raw(self, raws, transform, out_shapes=None, net_sizes=None):
        """groups_list from decoded (h_i, w_i, 3) uint8 images, as predict_raw; out_shapes defaults to the raw sizes."""
        return self._list_forward(_RawImages(self.model, raws, transform, net_sizes), out_shapes, groups="only")[1]

    @torch.no_grad()
    def render_raw(self, raws, transform, vis_modes, palette, group_palette=None, net_sizes=None):
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
        call whatever the modes: labels and group maps come from the same encode_image pass."""
        modes = list(vis_modes)
        for m in modes:
            if m not in VIS_MODES:
                raise ValueError(f"unknown vis mode {m!r}; known: {', '.join(VIS_MODES)}")
        want_labels = any(m in ("pred", "input_pred", "input_pred_label") for m in modes)
        want_groups = any(m in _GROUP_MODES for m in modes)
        src = _RawImages(self.model, raws, transform, net_sizes)
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


def _flat_maps(maps):
    """Index maps -> (flat uint8 buffer, offset of every map).  Views of one buffer (what predict_raw and groups_raw return)
    are used where they lie; anything else is copied into a new buffer at offsets that are multiples of 4."""
    store = maps[0].untyped_storage().data_ptr()
    if all(m.is_contiguous() and m.untyped_storage().data_ptr() == store for m in maps):
        lo = min(m.storage_offset() for m in maps)
        hi = max(m.storage_offset() + m.numel() for m in maps)
        return torch.as_strided(maps[0], (hi - lo,), (1,), lo), [m.storage_offset() - lo for m in maps]
    offs, n = [], 0
    for m in maps:
        offs.append(n)
        n += (m.numel() + 3) // 4 * 4
    flat = torch.zeros(n, dtype=torch.uint8, device=maps[0].device)
    for m, o in zip(maps, offs):
        flat[o:o + m.numel()].view(m.shape).copy_(m)
    return flat, offs


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
    if len(raws) == 0:
        raise ValueError("empty image list")
    if len(raws) != len(maps):
        raise ValueError(f"{len(raws)} images but {len(maps)} index maps")
    for t in list(raws) + list(maps):
        if not t.is_cuda:
            raise RuntimeError(f"segclip_amd: HIP kernels need device tensors (there is no CPU fallback); got a {t.device} tensor")
    for t, m in zip(raws, maps):
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8:
            raise ValueError(f"a decoded image is an (h, w, 3) uint8 tensor, got {t.dtype} {tuple(t.shape)}")
        if m.dtype != torch.uint8 or m.dim() != 2 or tuple(m.shape) != tuple(t.shape[:2]):
            raise ValueError(f"an index map is an (h, w) uint8 tensor of its image's size {tuple(t.shape[:2])}, got {m.dtype} "
                             f"{tuple(m.shape)}")
    dev = raws[0].device
    palette = _check_palette(palette, dev)
    flat, map_offs = _flat_maps(list(maps))
    table, offs, nbytes, n_blocks = ops.seg_blend_table(list(raws), map_offs)
    out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sums = torch.zeros(len(raws), palette.shape[0], 3, dtype=torch.int64, device=dev) if anchors else None
    ops.seg_blend(table, n_blocks, flat, palette, opacity, out, skip_zero=skip_zero, reverse_channels=channel_order == "bgr",
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
    `areas` (sum) before compute()."""

    def __init__(self, seg, ignore_index=255, reduce_zero_label=False):
        self.seg, self.ignore_index, self.reduce_zero_label = seg, int(ignore_index), bool(reduce_zero_label)
        self.areas = torch.zeros(3, seg.num_classes, dtype=torch.int64, device=seg.text_embedding.device)

    def reset(self):
        self.areas.zero_()

    @torch.no_grad()
    def update(self, imgs, gts, return_labels=False):
        """imgs [(3, H_i, W_i)], gts [(oh_i, ow_i) uint8]: the labels are formed at each ground truth's size."""
        self._check_gts(imgs, gts)
        return self._forward(_SlicedImages(self.seg.model, imgs), gts, return_labels)

    @torch.no_grad()
    def update_raw(self, raws, gts, transform, return_labels=False, net_sizes=None, aug=None):
        """raws [(h_i, w_i, 3) uint8 decoded images] instead of pre-processed ones, as SegInference.predict_raw (aug included)."""
        self._check_gts(raws, gts)
        if aug is not None:
            return self._forward(_RawViews(self.seg.model, raws, transform, aug, net_sizes), gts, return_labels, views=True)
        return self._forward(_RawImages(self.seg.model, raws, transform, net_sizes), gts, return_labels)

    @torch.no_grad()
    def update_views(self, views, gts, return_labels=False):
        """views[i] = [((3, H, W) tensor, flags)] as SegInference.predict_views, scored at each ground truth's size."""
        self._check_gts(views, gts)
        return self._forward(_SlicedViews(self.seg.model, views), gts, return_labels, views=True)

    @staticmethod
    def _check_gts(imgs, gts):
        if len(imgs) != len(gts):
            raise ValueError(f"{len(imgs)} images but {len(gts)} ground truths")
        for g in gts:
            if not g.is_cuda:
                raise RuntimeError(f"segclip_amd: HIP kernels need device tensors (there is no CPU fallback); got a {g.device} tensor")
            if g.dtype != torch.uint8 or g.dim() != 2:
                raise ValueError(f"a ground truth is an (oh, ow) uint8 tensor, got {g.dtype} {tuple(g.shape)}")

    def _forward(self, src, gts, return_labels, views=False):
        forward = self.seg._views_forward if views else self.seg._list_forward
        return forward(src, [tuple(g.shape) for g in gts], gts=list(gts), areas=self.areas, ignore_index=self.ignore_index,
                       reduce_zero_label=self.reduce_zero_label, want_labels=return_labels)

    @staticmethod
    def metrics_from_areas(areas):
        """(3, C) integer CPU tensor -> dict(mIoU, aAcc, mAcc, IoU, Acc) as mmseg's eval_metrics: IoU = I / (P + L - I),
        Acc = I / L, aAcc = sum(I) / sum(L); a class absent from prediction and label is NaN and left out of the means."""
        a = areas.to(torch.float64)
        inter, pred, label = a[0], a[1], a[2]
        iou, acc = inter / (pred + label - inter), inter / label
        return dict(mIoU=float(torch.nanmean(iou)), aAcc=float(inter.sum() / label.sum()), mAcc=float(torch.nanmean(acc)),
                    IoU=iou, Acc=acc)

    def compute(self):
        return self.metrics_from_areas(self.areas.cpu())
