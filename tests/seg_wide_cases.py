"""The synthetic cases of the 16-bit label-map tests (tests/test_seg_wide_gpu.py, tests/test_seg_wide_cpu.py) and their fp64
reference, on the CPU alone: windows of 64 x 64 on a 4 x 4 grid, 8 groups, tables in which every (window, group) pair has a
dominant class of its own, spread over the whole vocabulary (the high label byte, the last class, labels 255 / 256 / 257).
The yardsticks are tests/seg_reference.py and tests/seg_eval_reference.py; the near-tie rule is that of
tests/test_seg_eval_gpu.py (TIE = 1e-6, at most 0.05 % of a case's output pixels).  `python -m tests.seg_wide_cases` prints the
NEAR_TIE_COUNTS table."""
import functools

import torch

from tests import seg_eval_reference as ser
from tests import seg_reference as sr

TIE, CAP = 1e-6, 5e-4
G, GRID, WIN = 8, (4, 4), (64, 64)

# name: (mode, stride, B, net (H, W), out (oh, ow), N, with_bg, bg_thresh, seed, step)
CASES = {
    "w848_slide": ("slide", 32, 1, (64, 96), (90, 131), 847, True, 0.8, 41, 53),
    "w460_whole": ("whole", 0, 2, (64, 64), (75, 100), 459, True, 0.8, 32, 29),
    "w1024_nobg": ("slide", 48, 1, (64, 112), (64, 112), 1024, False, 0.0, 33, 61),
    "w300_down": ("slide", 32, 1, (96, 96), (50, 71), 300, True, 0.5, 34, 131),
    "w21_small": ("slide", 32, 2, (64, 96), (90, 131), 20, True, 0.8, 35, 7),
    # above the 32 classes up to which every lane scans its own pixel, and small enough for the LDS copy of the tables: the
    # wave-cooperative scan on staged tables (w21_small takes the per-lane scan)
    "w61_staged": ("slide", 32, 2, (64, 96), (90, 131), 60, True, 0.8, 36, 11),
}
# name: (output pixels, near-ties of the fp64 reference, distinct labels, labels above 255, largest label), from the CPU
# reference alone; in every case the fp32 restatement's labels equal the fp64 ones
NEAR_TIE_COUNTS = {
    "w848_slide": (11790, 0, 12, 11, 847),
    "w460_whole": (15000, 0, 12, 9, 459),
    "w1024_nobg": (7168, 0, 13, 12, 1023),
    "w300_down": (3550, 0, 22, 5, 300),
    "w21_small": (23580, 0, 15, 0, 20),
    "w61_staged": (23580, 0, 18, 0, 60),
}


def f32_tables(table):
    """A table rounded to fp32 and everything derived from it exactly (both sides then read the same numbers)."""
    t = table.float()
    score, cls = t.max(dim=-1)
    return dict(table=t, table_max=t.amax(dim=(1, 2)), best_class=cls, best_score=score)


def dominant(i, N, step):
    """The dominant class of (window, group) pair i = window * G + group."""
    return [N - 1, 255, 256][i - 1] % N if 1 <= i <= 3 else (i * step + N - 3) % N


def make_case(name, N=None):
    """-> dict(soft, t32, wins, win, ...) of a case, all on the CPU.  N: the case cut to fewer classes."""
    mode, stride, B, (H, W), out, N0, with_bg, thr, seed, step = CASES[name]
    N = N0 if N is None else N
    wins, win = sr.window_list(B, H, W, mode, WIN, (stride, stride))
    nW = len(wins)
    g = torch.Generator().manual_seed(1000 + seed)
    soft = torch.softmax(torch.randn(nW, G, *GRID, generator=g) * (1.0 + seed % 4), dim=1)
    g = torch.Generator().manual_seed(2000 + seed)
    table = torch.rand(nW, G, N, generator=g, dtype=torch.float64) * 0.1
    for k in range(nW):
        for j in range(G):
            table[k, j, dominant(k * G + j, N, step)] = 0.82 + 0.15 * float(torch.rand((), generator=g))
    table[:, ::4] *= 0.5      # every fourth group falls under the background threshold
    return dict(name=name, B=B, net=(H, W), out=out, N=N, with_bg=with_bg, thr=thr, wins=wins, win=win, soft=soft,
                t32=f32_tables(table), per=nW // B)


def reference_of(case, dtype=torch.float64):
    """fp64 labels at the output size, the near-tie mask, the network-size assembly."""
    B, (H, W), (oh, ow) = case["B"], case["net"], case["out"]
    ref = sr.assemble(case["soft"], case["t32"], case["wins"], (B, H, W), case["win"], case["with_bg"], case["thr"], dtype)
    labels, gap = ser.rescale_labels(ref["logits"], oh, ow, dtype)
    src_tie = (ref["group_gap"] < TIE) | ((ref["count"] > 1) & (ref["class_gap"] < TIE))
    return labels, ser.spread(src_tie, oh, ow) | (gap < TIE), ref


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, fp64 labels (B, oh, ow), near-tie mask) of a named case, computed once and shared: nobody writes to them."""
    case = make_case(name)
    labels, tie, _ = reference_of(case)
    return case, labels, tie


def counts(labels, tie):
    return (tie.numel(), int(tie.sum()), labels.unique().numel(), int((labels.unique() > 255).sum()), int(labels.max()))


def image_rows(case, gt_offsets=None):
    gh, gw = GRID
    return [dict(first=b * case["per"], count=case["per"], net=case["net"], out=case["out"], win=case["win"], grid=GRID,
                 soft_off=b * case["per"] * G * gh * gw, gt_off=-1 if gt_offsets is None else gt_offsets[b])
            for b in range(case["B"])]


def to_i16(t):
    """An integer tensor of values 0 .. 65535 -> torch.int16 with the same 16 bits."""
    t = t.long()
    return torch.where(t >= 32768, t - 65536, t).to(torch.int16)


def from_i16(t):
    """torch.int16 -> long, the 16 bits read as an unsigned value."""
    return t.long() & 0xFFFF


def synthetic_gt(want, C, seed):
    """The reference's labels with random rectangles relabelled, a band of 65535 and the values C and C + 3."""
    g = torch.Generator().manual_seed(seed)
    gt = want.clone()
    B, oh, ow = gt.shape
    for _ in range(12):
        b, y, x = int(torch.randint(0, B, (1,), generator=g)), int(torch.randint(0, oh - 20, (1,), generator=g)), \
            int(torch.randint(0, ow - 20, (1,), generator=g))
        h, w = int(torch.randint(5, oh // 3, (1,), generator=g)), int(torch.randint(5, ow // 3, (1,), generator=g))
        gt[b, y:y + h, x:x + w] = int(torch.randint(0, C, (1,), generator=g))
    gt[:, oh // 2:oh // 2 + 9, :] = 65535
    gt[:, 3:7, 5:40] = C + 3
    gt[:, -1, -5:] = C
    return gt


if __name__ == "__main__":
    for name in CASES:
        case, want, tie = reference(name)
        l32, _, _ = reference_of(case, torch.float32)
        print(f'"{name}": {counts(want, tie)},   # the fp32 reference differs at {int((l32 != want).sum())}', flush=True)
