"""CPU: tests/seg_reference.py (the yardstick of the segmentation kernels' GPU tests) reproduces what the REAL reference's
ViTSegInference.encode_decode computed (tests/golden/seg_tiny.npz, made by tests/golden/make_golden_seg.py)."""
import numpy as np
import pytest
import torch

from tests import seg_reference as sr
from tests.helpers import load_golden

G = load_golden("seg_tiny.npz")
CASES = [(si, ci) for si in range(len(G["sizes"])) for ci in range(len(G["cases"]))]


@pytest.mark.parametrize("si,ci", CASES)
def test_seg_reference_reproduces_encode_decode(si, ci):
    """Logits to 1e-5 absolute (0/1 indicators and products of two softmaxes, all in [0, 1]); arg-max label maps equal.
    The per-window inputs are the real reference's encode_image outputs, so only the post-processing is compared."""
    H, W = (int(v) for v in G["sizes"][si])
    with_bg, N, thr = bool(G["cases"][ci][0]), int(G["cases"][ci][1]), float(G["cases"][ci][2])
    hidden, feat = torch.from_numpy(G[f"hidden_{si}"]), torch.from_numpy(G[f"feat_{si}"])
    soft = torch.from_numpy(G[f"soft_{si}"])
    text = torch.from_numpy(G["text_embedding"])[:N]
    B = hidden.shape[0]
    tab = sr.group_table(hidden[:, 1:], feat, text, float(G["logit_scale"]), min(5, N))
    assert int(tab["mask"].sum()) == B * min(5, N)
    wins, size = sr.window_list(B, H, W, "whole")
    out = sr.assemble(soft.view(B, -1, H // 16, W // 16), tab, wins, (B, H, W), size, with_bg, thr)
    ref = torch.from_numpy(G[f"logits_{si}_{ci}"]).double()
    assert out["logits"].shape == ref.shape
    assert float((out["logits"] - ref).abs().max()) <= 1e-5
    assert torch.equal(out["labels"], ref.argmax(dim=1))


def test_seg_reference_text_embedding():
    feats = torch.from_numpy(G["text_feats"])
    n, t = G["prompt_ids"].shape[:2]
    got = sr.text_embedding(feats, n, t)
    assert float((got - torch.from_numpy(G["text_embedding"])).abs().max()) <= 1e-6


def test_seg_reference_fp32_against_fp64_near_ties():
    """What fp32 alone changes on the golden's own soft_attn: the count behind the caps of tests/test_seg_gpu.py."""
    for si in range(len(G["sizes"])):
        H, W = (int(v) for v in G["sizes"][si])
        soft = torch.from_numpy(G[f"soft_{si}"])
        soft = soft.view(soft.shape[0], -1, H // 16, W // 16)
        g64, gap = sr.window_groups(soft, H, W, torch.float64)
        g32, _ = sr.window_groups(soft, H, W, torch.float32)
        diff = g64 != g32
        assert bool((gap[diff] < 1e-6).all())
        assert int((gap < 1e-6).sum()) <= 1e-4 * gap.numel()
        assert int((gap < 1e-4).sum()) <= 2.5e-3 * gap.numel()


def test_slide_windows_grid():
    assert sr.slide_windows(224, 224, (224, 224), (224, 224)) == [(0, 0)]
    assert sr.slide_windows(448, 448, (224, 224), (224, 224)) == [(0, 0), (0, 224), (224, 0), (224, 224)]
    assert sr.slide_windows(300, 500, (224, 224), (224, 224)) == [(0, 0), (0, 224), (0, 276), (76, 0), (76, 224), (76, 276)]
    assert sr.slide_windows(225, 224, (224, 224), (224, 224)) == [(0, 0), (1, 0)]
    from segclip_amd import segmentation
    for H, W, c, s in [(300, 500, (224, 224), (224, 224)), (225, 224, (224, 224), (224, 224)), (448, 672, (224, 224), (112, 150))]:
        assert segmentation.slide_windows(H, W, c, s) == sr.slide_windows(H, W, c, s)
