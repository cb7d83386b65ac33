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
usage: python tools/bench_seg.py [reps=7] [out=profiles/seg_infer.txt]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import segclip_amd
from segclip_amd import config, ops, synth
from segclip_amd.segmentation import SegInference
from tools.clock_sampler import ClockSampler

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "seg_infer.txt")
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
    _, _, dwin, dfirst = seg._device_lists(B, H, W, img.device)
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


if __name__ == "__main__":
    segclip_amd.set_compute_dtype(torch.bfloat16)
    model, _ = synth.build_model(synth.SPECS["vitb16"], {}, device="cuda")
    model.eval()
    g = torch.Generator().manual_seed(0)
    text = torch.randn(20, 512, generator=g)
    text = (text / text.norm(dim=-1, keepdim=True)).cuda()
    say(f"# tools/bench_seg.py  ViT-B/16 synthetic weights, bf16 towers, 20 classes + background, {torch.cuda.get_device_name(0)}")
    case("(i)  whole  B=64 224x224", model, text, 64, 224, 224, 3)
    case("(ii) slide  B=16 448x672", model, text, 16, 448, 672, 2, mode="slide", crop_size=(224, 224), stride=(224, 224))
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")
