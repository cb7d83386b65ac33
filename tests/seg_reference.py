"""Torch-CPU statement of the zero-shot segmentation inference math, written from its description (not from the reference's
program text) and pinned to the real reference by tests/golden/seg_tiny.npz (tests/test_seg_reference_golden.py).

  text_embedding : mean over the templates, L2 norm
  group_table    : per window the G x N table = softmax(group logits) * softmax(group logits masked to the top-k classes
                   of the pooled feature); its maximum; first maximum of every row; top-k mask (ties: lowest index)
  window_groups  : bilinear (align_corners=False) upsampling of the soft assignment, first maximum over the groups
  slide_windows  : mmseg's window grid.  mmseg is not part of the reference tree: the slide assembly below (sum of the
                   windows' logits / window count) is UNPINNED third-party behaviour restated here
  assemble       : logits (B, N + off, H, W), labels, groups and the top-two gaps the tests use to verify near-ties

Everything takes a dtype (float64 = the yardstick, float32 = the count of what fp32 alone changes).
"""
import torch


def text_embedding(feats, n_classes, n_templates):
    e = feats.view(n_classes, n_templates, -1).mean(dim=1)
    return e / e.norm(dim=-1, keepdim=True)


def group_table(group_tokens, pooled, text, logit_scale, topk, dtype=torch.float64):
    """group_tokens (W, G, C), pooled (W, C), text (N, C) normalised, logit_scale = the raw parameter (log scale)."""
    gt, pf, tx = group_tokens.to(dtype), pooled.to(dtype), text.to(dtype)
    gt = gt / gt.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    pf = pf / pf.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    scale = torch.as_tensor(logit_scale, dtype=dtype).exp().clamp(max=100.0)
    glog = gt @ tx.t() * scale                                   # (W, G, N)
    pre = torch.softmax(glog, dim=-1)
    pprob = torch.softmax(pf @ tx.t() * scale, dim=-1)           # (W, N)
    order = torch.sort(pprob, dim=-1, descending=True, stable=True).indices[:, :topk]   # equal values: lowest index first
    mask = torch.zeros_like(pprob, dtype=torch.bool)
    mask.scatter_(1, order, True)
    masked = glog.masked_fill(~mask[:, None, :], float("-inf"))
    table = torch.softmax(masked, dim=-1) * pre
    best_score, best_class = table.max(dim=-1)                   # torch.max returns the first maximum
    if table.shape[-1] > 1:
        top2 = table.topk(2, dim=-1).values
        row_gap = top2[..., 0] - top2[..., 1]
    else:
        row_gap = torch.full_like(best_score, float("inf"))
    return dict(table=table, table_max=table.amax(dim=(1, 2)), best_class=best_class, best_score=best_score, mask=mask,
                row_gap=row_gap)


def _taps(n_dst, n_src, dtype):
    d = torch.arange(n_dst, dtype=dtype)
    s = ((d + 0.5) * (torch.tensor(n_src, dtype=dtype) / torch.tensor(n_dst, dtype=dtype)) - 0.5).clamp_min(0.0)
    i0 = s.floor().long().clamp_max(n_src - 1)
    i1 = (i0 + 1).clamp_max(n_src - 1)
    return i0, i1, s - i0.to(dtype)


def upsample(soft, out_h, out_w, dtype=torch.float64):
    """(..., h, w) -> (..., out_h, out_w), bilinear, align_corners=False."""
    x = soft.to(dtype)
    y0, y1, ly = _taps(out_h, x.shape[-2], dtype)
    x0, x1, lx = _taps(out_w, x.shape[-1], dtype)
    ly = ly[:, None]

    def row(r):
        return (1 - lx) * r[..., x0] + lx * r[..., x1]
    return (1 - ly) * row(x[..., y0, :]) + ly * row(x[..., y1, :])


def window_groups(soft, out_h, out_w, dtype=torch.float64):
    """soft (W, G, h, w) -> groups (W, out_h, out_w) = first maximum over G, gap = top value - second value."""
    up = upsample(soft, out_h, out_w, dtype)
    groups = up.argmax(dim=1)
    if up.shape[1] > 1:
        top2 = up.topk(2, dim=1).values
        gap = top2[:, 0] - top2[:, 1]
    else:
        gap = torch.full(groups.shape, float("inf"), dtype=dtype)
    return groups, gap


def slide_windows(H, W, crop, stride):
    (ch, cw), (sh, sw) = crop, stride
    hg = max(H - ch + sh - 1, 0) // sh + 1
    wg = max(W - cw + sw - 1, 0) // sw + 1
    out = []
    for i in range(hg):
        for j in range(wg):
            y1, x1 = min(i * sh + ch, H), min(j * sw + cw, W)
            out.append((max(y1 - ch, 0), max(x1 - cw, 0)))
    return out


def window_list(B, H, W, mode, crop=None, stride=None):
    if mode == "whole":
        return [(b, 0, 0) for b in range(B)], (H, W)
    return [(b, y, x) for b in range(B) for (y, x) in slide_windows(H, W, crop, stride)], tuple(crop)


def assemble(soft, tab, windows, out_size, win_size, with_bg, bg_thresh, dtype=torch.float64):
    """soft (nW, G, h, w); tab = group_table(...) of the same windows; windows [(image, y0, x0)].
    -> dict(logits (B, N + off, H, W), labels, groups (first covering window), count,
            group_gap = smallest top-two gap of the interpolated groups over the covering windows,
            class_gap = top-two gap of the class logits)."""
    B, H, W = out_size
    wh, ww = win_size
    table = tab["table"].to(dtype)
    nW, G, N = table.shape
    off = 1 if with_bg else 0
    grp, gap = window_groups(soft, wh, ww, dtype)
    logits = torch.zeros(B, N + off, H, W, dtype=dtype)
    count = torch.zeros(B, H, W, dtype=dtype)
    groups = torch.zeros(B, H, W, dtype=torch.long)
    group_gap = torch.full((B, H, W), float("inf"), dtype=dtype)
    for k, (b, y0, x0) in enumerate(windows):
        rows = table[k][grp[k]]                                  # (wh, ww, N): every pixel's row of the table
        lg = torch.zeros(N + off, wh, ww, dtype=dtype)
        lg[off:] = rows.permute(2, 0, 1)
        if with_bg:
            thr = torch.minimum(torch.tensor(bg_thresh, dtype=dtype), tab["table_max"][k].to(dtype))
            lg[0] = (rows.amax(dim=-1) < thr).to(dtype)
        sl = (b, slice(y0, y0 + wh), slice(x0, x0 + ww))
        first = count[sl] == 0
        groups[sl] = torch.where(first, grp[k], groups[sl])
        group_gap[sl] = torch.minimum(group_gap[sl], gap[k])
        logits[b, :, y0:y0 + wh, x0:x0 + ww] += lg
        count[sl] += 1
    logits = logits / count.clamp_min(1)[:, None]
    labels = logits.argmax(dim=1)
    if N + off > 1:
        top2 = logits.topk(2, dim=1).values
        class_gap = top2[:, 0] - top2[:, 1]
    else:
        class_gap = torch.full((B, H, W), float("inf"), dtype=dtype)
    return dict(logits=logits, labels=labels, groups=groups, count=count, group_gap=group_gap, class_gap=class_gap)
