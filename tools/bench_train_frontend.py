"""The training front end on the device against the copy it replaces (tool only; writes profiles/train_frontend.txt).

Workload: 256 decoded images of mixed CC3M-like sizes (long side 300 .. 640, closed-form from a seed), already on the device as
uint8, and an int32 segment map per image; RawImageTransform(224, is_train=True) with crops drawn from a fixed seed.

  (a) the whole RawImageTransform.__call__ (crop sampling, table upload, ONE segclip_train_images_from_u8 launch) and
      patch_labels, and the host-to-device copy of the (256, 3, 224, 224) fp32 batch (154.1 MB, pinned) + the (256, 1, 14, 14)
      int64 label grid that a CPU pipeline would hand over, alternating within each repeat on the same box
  (b) the two kernels alone in a `rocprofv3 --kernel-trace --stats` child of their own (--child: ten calls and nothing else),
      and the image kernel's bytes per second against its design bound: the crop bytes read once + 12 B per output pixel

  python tools/bench_train_frontend.py [repeats] [output file]
"""
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from segclip_amd.transforms import RawImageTransform

CHILD = "--child" in sys.argv[1:]
ARGV = [a for a in sys.argv[1:] if a != "--child"]
REPS = int(ARGV[0]) if len(ARGV) > 0 else 7
OUT = ARGV[1] if len(ARGV) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                 "train_frontend.txt")
HBM_PEAK = 8.0e12   # bytes / s, MI355X specification
B, SIZE, SEED = 256, 224, 11
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def inputs():
    rng = random.Random(SEED)
    g = torch.Generator(device="cuda").manual_seed(SEED)
    raws, maps = [], []
    for _ in range(B):
        long_side, ratio = rng.randint(300, 640), rng.choice((1.0, 4 / 3, 3 / 2, 16 / 9, 5 / 4))
        h, w = long_side, max(int(long_side / ratio), 1)
        if rng.random() < 0.7:
            h, w = w, h
        raws.append(torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8, device="cuda"))
        maps.append(torch.randint(0, 200, (h, w), generator=g, dtype=torch.int32, device="cuda"))
    return raws, maps


def child():
    """ten calls of the two launches and nothing else: what the rocprofv3 child traces"""
    tf = RawImageTransform(SIZE, is_train=True)
    raws, maps = inputs()
    rng = random.Random(SEED)
    boxes = [tf.sample(int(t.shape[0]), int(t.shape[1]), rng)[0] for t in raws]
    for _ in range(10):
        _, coord = tf(raws, boxes=boxes)
        tf.patch_labels(maps, coord)
    torch.cuda.synchronize()


def main():
    from tools import rocprof_roofline as rr
    from tools.clock_sampler import ClockSampler
    say(f"# tools/bench_train_frontend.py  {B} images, long side 300 .. 640, -> {SIZE} x {SIZE}, {torch.cuda.get_device_name(0)}")
    tf = RawImageTransform(SIZE, is_train=True)
    raws, maps = inputs()
    rng = random.Random(SEED)
    boxes = [tf.sample(int(t.shape[0]), int(t.shape[1]), rng)[0] for t in raws]
    crop_bytes = sum(3 * ch * cw for (_, _, ch, cw) in boxes)
    written = B * 3 * SIZE * SIZE * 4
    scales = sorted(max(ch, cw) / SIZE for (_, _, ch, cw) in boxes)
    say(f"crops: {crop_bytes} bytes, scale (long crop side / {SIZE}) median {scales[B // 2]:.2f}, max {scales[-1]:.2f}; "
        f"{written} bytes written; design bound {(crop_bytes + written) / HBM_PEAK * 1e6:.1f} us at {HBM_PEAK / 1e12:.0f} TB/s")
    host_img = torch.randn(B, 3, SIZE, SIZE).pin_memory()
    host_seg = torch.zeros(B, 1, SIZE // 16, SIZE // 16, dtype=torch.int64).pin_memory()
    dev_img, dev_seg = torch.empty_like(host_img, device="cuda"), torch.empty_like(host_seg, device="cuda")
    state = {}

    def front():
        state["img"], coord = tf(raws, rng=random.Random(SEED))
        state["seg"] = tf.patch_labels(maps, coord)

    def front_given():
        state["img"], coord = tf(raws, boxes=boxes)
        state["seg"] = tf.patch_labels(maps, coord)

    def copy():
        dev_img.copy_(host_img, non_blocking=True)
        dev_seg.copy_(host_seg, non_blocking=True)

    ways = [("__call__ + patch_labels", front), ("the same, boxes given", front_given), ("pinned H2D copy it replaces", copy)]
    for _, fn in ways:
        fn()
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in ways]
    sampler = ClockSampler().start()
    for _ in range(REPS):   # alternating: every repeat times the ways one after the other
        for k, (_, fn) in enumerate(ways):
            t0 = time.perf_counter()
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) / 5)
    clk = sampler.stop()
    meds = [statistics.median(t) for t in ts]
    for (what, _), t, med in zip(ways, ts, meds):
        say(f"{what:30s} {med * 1e3:8.3f} ms (min {min(t) * 1e3:.3f}, max {max(t) * 1e3:.3f}; {REPS} x 5 calls)")
    say(f"__call__ + patch_labels / copy {meds[0] / meds[2]:.3f}; clock {clk}")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        try:
            rc, _, err = rr.run_child([os.path.abspath(__file__), "--child"], tmp)
            db = rr.find_db(tmp)
            table = rr.kernel_table(db) if rc == 0 and db else []
        except Exception as e:   # no rocprofv3 on the box
            rc, err, table = -1, repr(e), []
    for kern, what in (("train_front_kernel", "segclip_train_images_from_u8"), ("train_labels_kernel", "segclip_train_patch_labels")):
        rows = [r for r in table if kern in r[0]]
        if not rows:
            say(f"{what} alone: unmeasured (rocprofv3 child rc={rc}: {str(err)[-200:]})")
            continue
        _, calls, _, avg_us = rows[0]
        if kern == "train_front_kernel":
            say(f"{what} alone (rocprofv3 --kernel-trace --stats, {calls} launches) {avg_us:8.1f} us per launch: "
                f"{(crop_bytes + written) / avg_us / 1e6:.3f} TB/s of crop bytes once + writes = "
                f"{(crop_bytes + written) / avg_us * 1e6 / HBM_PEAK:.3f} of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
        else:
            say(f"{what} alone (rocprofv3 --kernel-trace --stats, {calls} launches) {avg_us:8.1f} us per launch")
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    child() if CHILD else main()
