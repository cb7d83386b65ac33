"""Zero-shot segmentation inference: an image batch and class prompts in, a label map out.

Replaces seg_segmentation/evaluation of the reference without mmseg / mmcv: build_text_embedding is the text step of
build_seg_inference (evaluation/builder.py:55-66), SegInference is ViTSegInference (evaluation/vit_seg.py:118-256) plus
mmseg's whole / slide inference.  The dataset, the tokenizer, rescaling to the original image size and mIoU stay with the
caller.  The post-processing runs in three HIP kernels (csrc/segment.hip): the label map is written as one byte per pixel
without the reference's (H, W, G) / (H, W, N) intermediates, and the vision tower sees every window once, all windows of
all images of a call in one batch.
"""
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
