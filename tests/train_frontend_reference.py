"""Integer restatement of the training front end (csrc/train_frontend.inc, segclip_amd/transforms.py), numpy and Python only:
Pillow's 8-bit BICUBIC resize of a crop (ImagingResample: coefficients in fp64, rounded to 22 bits, int32 accumulators, a uint8
image between the horizontal and the vertical pass), the ToTensor + Normalize value table, ATen's `nearest` index and the patch
mean of get_felzenszwalb_from_cache, the draws of RandomResizedCropCoord.get_params and torchvision's Resize + CenterCrop
geometry (reference dataloaders/rawimage_util.py:33-53, :100-144, :303-361).  Everything here is exact: the tests compare with
array_equal."""
import math

import numpy as np
import torch

PRECISION_BITS = 22
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coefficients(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the whole axis of n_in pixels -> n_out:
    [(xmin, [int coefficient per tap])] per destination.  Python floats are the C doubles."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
        out.append((xmin, k))
    return out


def _pass(a, n_out):
    """one pass along axis 1 of a (rows, n_in, C) uint8 array -> (rows, n_out, C) uint8"""
    n_in = a.shape[1]
    res = np.empty((a.shape[0], n_out, a.shape[2]), dtype=np.uint8)
    src = a.astype(np.int64)
    for xx, (xmin, k) in enumerate(coefficients(n_in, n_out)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, xmin:xmin + len(k)], np.asarray(k, dtype=np.int64), axes=([1], [0]))
        assert acc.size == 0 or (abs(acc).max() < (1 << 31)), "Pillow's int accumulator would overflow"
        res[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return res


def resize_crop(a, box, RW, RH):
    """Image.fromarray(a).crop(box).resize((RW, RH), Image.BICUBIC) for an (h, w, 3) uint8 array and box = (left, upper,
    right, lower) inside it: the filter sees the crop alone."""
    x0, y0, x1, y1 = box
    c = np.ascontiguousarray(a[y0:y1, x0:x1])
    hp = _pass(c, RW)                                   # horizontal first, rounded to bytes
    return _pass(hp.transpose(1, 0, 2), RH).transpose(1, 0, 2)


def value_table(mean=CLIP_MEAN, std=CLIP_STD):
    """ToTensor then Normalize of every byte: (256, 3) fp32, the operations of torchvision in their order"""
    m = torch.tensor(mean, dtype=torch.float32).view(1, 3)
    s = torch.tensor(std, dtype=torch.float32).view(1, 3)
    return ((torch.arange(256, dtype=torch.float32) / 255).view(-1, 1) - m) / s


def train_image(a, box, RW, RH, window, out_hw, flags=0, lut=None):
    """one output of segclip_train_images_from_u8: (3, out_h, out_w) fp32.  box = (x0, y0, bw, bh), window = (ox, oy)"""
    x0, y0, bw, bh = box
    r = resize_crop(a, (x0, y0, x0 + bw, y0 + bh), RW, RH)
    ox, oy = window
    r = r[oy:oy + out_hw[0], ox:ox + out_hw[1]]
    assert r.shape[:2] == tuple(out_hw)
    if flags & 1:
        r = r[:, ::-1]
    if flags & 2:
        r = r[::-1]
    lut = value_table() if lut is None else lut
    idx = torch.from_numpy(np.ascontiguousarray(r)).long()          # (H, W, 3)
    return torch.stack([lut[idx[..., c], c] for c in range(3)])


def nearest_index(n_in, n_out):
    """ATen's nearest source index of every destination: min((int64) floorf(d * ((float) in / out)), in - 1), in fp32"""
    scale = np.float32(n_in) / np.float32(n_out)
    d = np.arange(n_out, dtype=np.float32)
    return np.minimum(np.floor(d * scale).astype(np.int64), n_in - 1)


def nearest_index_integer(n_in, n_out):
    """the tempting integer form, which is NOT ATen's (480 -> 224 differs at one index)"""
    return np.minimum(np.arange(n_out, dtype=np.int64) * n_in // n_out, n_in - 1)


def label_box(coord, h, w):
    """the crop of get_felzenszwalb_from_cache (rawimage_util.py:106-125) from one coord row (the reference's is a float32
    tensor) -> (x0, y0, x1, y1, flags); a box thinner than 2 stands for the whole map"""
    xu, yu, xl, yl = (float(np.float32(v)) for v in coord)
    flags = 0
    if xu > xl:
        xu, xl, flags = xl, xu, flags | 1
    if yu > yl:
        yu, yl, flags = yl, yu, flags | 2
    return int(xu * w), int(yu * h), math.ceil(xl * w), math.ceil(yl * h), flags


def patch_labels(seg, box, flags, size, patch):
    """get_felzenszwalb_from_cache for one (h, w) integer map and an integer box -> (size / patch, size / patch) int64"""
    x0, y0, x1, y1 = box
    m = np.asarray(seg)
    if not (y1 - y0 < 2 or x1 - x0 < 2):
        m = m[y0:y1, x0:x1]
    if flags & 1:
        m = m[:, ::-1]
    if flags & 2:
        m = m[::-1]
    r = m[nearest_index(m.shape[0], size)][:, nearest_index(m.shape[1], size)].astype(np.int64)
    P = size // patch
    s = r.reshape(P, patch, P, patch).transpose(0, 2, 1, 3).reshape(P, P, patch * patch).sum(-1)
    return s // (patch * patch)


def sample(h, w, rng, scale=(0.5, 1.0), ratio=(3. / 4., 4. / 3.)):
    """RandomResizedCropCoord.get_params + the coord of __call__ (rawimage_util.py:303-361), with rng a random.Random in
    place of the module: -> ((i, j, ch, cw), [4 floats])"""
    area = h * w
    got = None
    for _ in range(10):
        target_area = rng.uniform(*scale) * area
        log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
        aspect_ratio = math.exp(rng.uniform(*log_ratio))
        cw = int(round(math.sqrt(target_area * aspect_ratio)))
        ch = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < cw <= w and 0 < ch <= h:
            i = rng.randint(0, h - ch)
            j = rng.randint(0, w - cw)
            got = (i, j, ch, cw)
            break
    if got is None:
        in_ratio = float(w) / float(h)
        if in_ratio < min(ratio):
            cw = w
            ch = int(round(cw / min(ratio)))
        elif in_ratio > max(ratio):
            ch = h
            cw = int(round(ch * max(ratio)))
        else:
            cw, ch = w, h
        got = ((h - ch) // 2, (w - cw) // 2, ch, cw)
    i, j, ch, cw = got
    if w - 1 == 0 or h - 1 == 0:
        coord = [0., 0., 0., 0.]
    else:
        coord = [float(j) / (w - 1), float(i) / (h - 1), float(j + cw - 1) / (w - 1), float(i + ch - 1) / (h - 1)]
    return got, coord


def eval_geometry(h, w, size):
    """torchvision's Resize(size) (short side to size, the other int(size * long / short)) then CenterCrop(size) on an image at
    least `size` on both resized sides -> (RW, RH, ox, oy)"""
    if (w <= h and w == size) or (h <= w and h == size):
        RW, RH = w, h
    elif w < h:
        RW, RH = size, int(size * h / w)
    else:
        RW, RH = int(size * w / h), size
    return RW, RH, int(round((RW - size) / 2.0)), int(round((RH - size) / 2.0))


# ------------------------------------------------------------------------------------------------ the case table
def source(kind, h, w, seed):
    """(h, w, 3) uint8, closed-form from the seed: "rand" bytes, "bits" random 0 / 255, "checker" a 0 / 255 checkerboard that
    is shifted per channel, "smooth" a gradient with a little noise"""
    rng = np.random.default_rng(seed)
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    if kind == "rand":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "bits":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    if kind == "checker":
        return (((y + x + c) % 2) * 255).astype(np.uint8)
    if kind == "smooth":
        return np.clip(2 * y + 3 * x + 40 * c + rng.integers(0, 8, (h, w, 3)), 0, 255).astype(np.uint8)
    raise ValueError(kind)


A, BZ, CW = (32, 48), (40, 36), (40, 38)   # outputs (out_h, out_w): 40 rows are no multiple of the 16-row band, 38 columns none of 4
# name: ((h, w), (x0, y0, bw, bh), (RW, RH), (ox, oy), (out_h, out_w), flags, kind)
CASES = {
    "inside_down": ((100, 90), (7, 9, 75, 83), (48, 32), (0, 0), A, 0, "smooth"),    # non-integer scales, box strictly inside
    "inside_rand": ((100, 90), (7, 9, 75, 83), (48, 32), (0, 0), A, 0, "rand"),
    "corner_tl": ((60, 70), (0, 0, 50, 41), (36, 40), (0, 0), BZ, 0, "rand"),
    "corner_tr": ((60, 70), (20, 0, 50, 41), (36, 40), (0, 0), BZ, 0, "rand"),
    "corner_bl": ((60, 70), (0, 19, 50, 41), (36, 40), (0, 0), BZ, 0, "rand"),
    "corner_br": ((60, 70), (20, 19, 50, 41), (36, 40), (0, 0), BZ, 0, "rand"),
    "scale8_x": ((40, 320), (4, 2, 288, 36), (36, 40), (0, 0), BZ, 0, "rand"),
    "scale8_both": ((330, 300), (6, 5, 288, 320), (36, 40), (0, 0), BZ, 0, "rand"),
    "scale8_bits": ((330, 300), (6, 5, 288, 320), (36, 40), (0, 0), BZ, 0, "bits"),
    "up_5x7": ((5, 7), (0, 0, 7, 5), (48, 32), (0, 0), A, 0, "rand"),
    "up_3x3_224": ((3, 3), (0, 0, 3, 3), (224, 224), (0, 0), (224, 224), 0, "rand"),
    "identity_x": ((50, 48), (0, 3, 48, 40), (48, 32), (0, 0), A, 0, "rand"),
    "identity_both": ((32, 48), (0, 0, 48, 32), (48, 32), (0, 0), A, 0, "rand"),
    "one_row": ((1, 60), (0, 0, 60, 1), (48, 32), (0, 0), A, 0, "rand"),
    "one_column": ((50, 1), (0, 0, 1, 50), (36, 40), (0, 0), BZ, 0, "rand"),
    "checker_down": ((64, 96), (0, 0, 96, 64), (48, 32), (0, 0), A, 0, "checker"),
    "checker_up": ((20, 18), (0, 0, 18, 20), (36, 40), (0, 0), BZ, 0, "checker"),
    "checker_odd": ((77, 91), (2, 1, 85, 73), (38, 40), (0, 0), CW, 0, "checker"),
    "bits_w38": ((90, 100), (3, 4, 90, 80), (38, 40), (0, 0), CW, 0, "bits"),
    "bits_up": ((11, 13), (0, 0, 13, 11), (48, 32), (0, 0), A, 0, "bits"),
    "flip_h": ((100, 90), (7, 9, 75, 83), (48, 32), (0, 0), A, 1, "rand"),
    "flip_v": ((100, 90), (7, 9, 75, 83), (48, 32), (0, 0), A, 2, "rand"),
    "flip_hv": ((100, 90), (7, 9, 75, 83), (48, 32), (0, 0), A, 3, "rand"),
    "flip_hv_w38": ((90, 100), (3, 4, 90, 80), (38, 40), (0, 0), CW, 3, "rand"),
    "window_ox": ((40, 100), (0, 0, 100, 40), (80, 32), (16, 0), A, 0, "rand"),      # eval: Resize then CenterCrop
    "window_oy": ((150, 72), (0, 0, 72, 150), (48, 100), (0, 34), A, 0, "rand"),
    "window_both_flip": ((70, 80), (5, 6, 70, 60), (50, 47), (7, 5), BZ, 1, "rand"),
}
GOLDEN_CASES = ["inside_down", "corner_br", "scale8_both", "up_5x7", "checker_down", "bits_w38", "window_ox"]
# eval geometry through Pillow: (h, w), size
GOLDEN_EVAL = {"eval_landscape": ((40, 100), 32), "eval_portrait": ((90, 37), 32), "eval_square": ((50, 50), 32),
               "eval_short_is_size": ((32, 45), 32)}


def case_source(name):
    (h, w), _, _, _, _, _, kind = CASES[name]
    return source(kind, h, w, 1 + list(CASES).index(name))


def case_resized(name):
    """the whole resized crop of a case, (RH, RW, 3) uint8"""
    _, (x0, y0, bw, bh), (RW, RH), _, _, _, _ = CASES[name]
    return resize_crop(case_source(name), (x0, y0, x0 + bw, y0 + bh), RW, RH)


def eval_source(name):
    (h, w), _ = GOLDEN_EVAL[name]
    return source("rand", h, w, 100 + list(GOLDEN_EVAL).index(name))


def eval_bytes(name):
    """RawImageExtractor's test transform up to the bytes: (size, size, 3) uint8"""
    (h, w), size = GOLDEN_EVAL[name]
    RW, RH, ox, oy = eval_geometry(h, w, size)
    return resize_crop(eval_source(name), (0, 0, w, h), RW, RH)[oy:oy + size, ox:ox + size]
