"""The definition of the pixel-adaptive refinement (include/segclip_hip.h, segclip_seg_refine) restated in torch on the CPU:
shift-and-clamp neighbours, stack and std, soft-max, T steps.  fp64 by default; `dtype` runs the same text in fp32, which is how
the GPU tests measure the rounding floor of a case.  Nothing here shares code with the library."""
import torch

OFFSETS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))   # (row, column)


def neighbours(t, dilations):
    """t (..., h, w) -> (..., 8 D, h, w): t at clamp(p + d o), dilation-major (replicate padding)"""
    h, w = t.shape[-2:]
    ys, xs = torch.arange(h), torch.arange(w)
    out = []
    for d in dilations:
        for oy, ox in OFFSETS:
            yy, xx = (ys + d * oy).clamp(0, h - 1), (xs + d * ox).clamp(0, w - 1)
            out.append(t[..., yy[:, None], xx[None, :]])
    return torch.stack(out, dim=-3)


def normalise(raw, mean, std, reverse_channels=False, dtype=torch.float64):
    """(h, w, 3) uint8 -> x (3, h, w): the picture's channel s meets entry 2 - s of mean / std when it is BGR"""
    mean, std = torch.tensor(mean, dtype=dtype), torch.tensor(std, dtype=dtype)
    if reverse_channels:
        mean, std = mean.flip(0), std.flip(0)
    return ((raw.to(dtype) - mean) / std).permute(2, 0, 1)


def weights(raw, mean, std, dilations, reverse_channels=False, dtype=torch.float64):
    """-> w (8 D, h, w): softmax_n of a(p, n) = -(1/3) sum_c |x_c(p) - x_c(q_n)| / (1e-8 + 0.1 sigma_c(p))"""
    x = normalise(raw, mean, std, reverse_channels, dtype)                     # (3, h, w)
    nb = neighbours(x, dilations)                                              # (3, 8 D, h, w)
    centre = x[:, None].expand(-1, len(dilations), -1, -1)
    sigma = torch.cat([nb, centre], dim=1).std(dim=1, unbiased=True)           # divisor 9 D - 1
    a = -((x[:, None] - nb).abs() / (1e-8 + 0.1 * sigma[:, None])).sum(dim=0) / 3.0
    return torch.softmax(a, dim=0)


def one_hot(labels, num_classes, dtype=torch.float64):
    """(h, w) uint8 -> m0 (C, h, w); a byte >= C belongs to no plane"""
    k = torch.arange(num_classes)[:, None, None]
    return (labels.long()[None] == k).to(dtype)


def planes(raw, labels, num_classes, mean, std, dilations, iters, reverse_channels=False, dtype=torch.float64):
    """-> m^T (C, h, w)"""
    w = weights(raw, mean, std, dilations, reverse_channels, dtype)
    m = one_hot(labels, num_classes, dtype)
    for _ in range(iters):
        m = (w[None] * neighbours(m, dilations)).sum(dim=1)
    return m


def labels_from_planes(m, labels):
    """the smallest k that attains the maximum; a pixel whose planes are all zero keeps its input byte"""
    top, arg = m.max(dim=0)
    first = (m == top[None]).to(torch.uint8).argmax(dim=0)   # argmax of a 0/1 map: its first 1
    assert torch.equal(m.gather(0, first[None])[0], top) and bool((first <= arg).all())
    return torch.where(top > 0, first.to(torch.uint8), labels)


def refine(raw, labels, num_classes, mean, std, dilations, iters, reverse_channels=False, dtype=torch.float64):
    """-> (L' (h, w) uint8, m^T (C, h, w))"""
    m = planes(raw, labels, num_classes, mean, std, dilations, iters, reverse_channels, dtype)
    return labels_from_planes(m, labels), m


def margin(m):
    """(C, h, w) -> the gap between the largest and the second largest plane per pixel (inf for one class)"""
    if m.shape[0] == 1:
        return torch.full(m.shape[1:], float("inf"), dtype=m.dtype)
    top = m.topk(2, dim=0).values
    return top[0] - top[1]


def miou(pred, gt, num_classes):
    """mean over the classes present in pred or gt of intersection / union"""
    ious = []
    for k in range(num_classes):
        p, g = pred == k, gt == k
        union = int((p | g).sum())
        if union:
            ious.append(int((p & g).sum()) / union)
    return sum(ious) / len(ious)


def snapping_scene(h=96, w=128, noise=12, shift=(5, -5), seed=0):
    """Three flat colour regions plus uniform byte noise; the ground truth is the regions, the input labels are the ground truth
    displaced by `shift` pixels (rows, columns; replicated at the border).  -> (raw (h, w, 3) uint8, labels, gt)"""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.arange(h)[:, None], torch.arange(w)[None, :]
    gt = torch.zeros(h, w, dtype=torch.uint8)
    gt[(ys >= h // 3) & (xs < (5 * w) // 8)] = 1
    gt[(xs >= (5 * w) // 8) & (ys + xs // 4 >= h // 2)] = 2
    colours = torch.tensor([[60, 90, 200], [200, 70, 60], [70, 190, 80]], dtype=torch.int64)
    raw = colours[gt.long()] + torch.randint(-noise, noise + 1, (h, w, 3), generator=g)
    raw = raw.clamp(0, 255).to(torch.uint8)
    yy = (torch.arange(h) - shift[0]).clamp(0, h - 1)
    xx = (torch.arange(w) - shift[1]).clamp(0, w - 1)
    return raw, gt[yy[:, None], xx[None, :]].contiguous(), gt
