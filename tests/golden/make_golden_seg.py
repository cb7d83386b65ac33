"""Golden vectors for zero-shot segmentation inference, produced by the REAL reference's ViTSegInference on CPU.

Run in the build container only:   python tests/golden/make_golden_seg.py
Output (committed): tests/golden/seg_tiny.npz

mmcv and mmseg are not installed; vit_seg.py needs of them only a Config that behaves like a dict and a base class whose
constructor chain reaches nn.Module, so both are in-script stand-ins (mmcv.imread / imwrite etc. are never reached).  The
package __init__ files of seg_segmentation import the dataset builders (mmseg.datasets, omegaconf), so the two packages are
registered as bare namespaces and only evaluation/vit_seg.py is executed.

Stored: the image batches, the prompt ids and the text embedding (the real encode_text followed by the three lines of
evaluation/builder.py:63-66), the real encode_image outputs of every image (the per-window inputs of the post-processing;
one image per call as encode_decode does it - with the torch-1.8 key layout of the cross-attention block a batch mixes its
samples, and only at batch 1 do both layouts coincide), and per case the real encode_decode output.  Cases: with / without background; N = 3 (top-k = N) and N = 12 (top-5 mask
active); a bg_thresh above and one below the table maximum; 128 x 128 (2x the training resolution) and 256 x 64 (4x by 1x:
resize_attn_map's h > w branch; the vision tower takes its segmentation branch only at 1x or 4x the training token count,
modules/module_seg_vit.py:423, so 2x by 3x is not available).  Weights are the closed-form generators of segclip_amd/synth.py.
"""
import importlib
import logging
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_harness as rh  # noqa: E402
from segclip_amd import synth  # noqa: E402
from tests import seg_reference as sr  # noqa: E402

SIZES = [(128, 128), (256, 64)]
N_IMAGES = 2
N_CLASSES, N_TEMPLATES = 12, 2
# (with_bg, N, bg_thresh): 0.95 lies above every table maximum of these inputs, 0.1 (N = 3) / 0.03 (N = 12) below (asserted)
CASES = [(True, 3, 0.95), (True, 3, 0.1), (False, 3, 0.95), (True, 12, 0.95), (True, 12, 0.03), (False, 12, 0.95)]


def import_vit_seg():
    rh.import_reference()
    root = os.path.join(rh.REF_ROOT, "seg_segmentation")

    def namespace(name, path):
        m = types.ModuleType(name)
        m.__path__ = [path]
        sys.modules[name] = m
        return m

    namespace("seg_segmentation", root)
    namespace("seg_segmentation.evaluation", os.path.join(root, "evaluation"))
    lg = types.ModuleType("seg_segmentation.logger")
    lg.get_logger = lambda *a, **k: logging.getLogger("seg_golden")
    sys.modules["seg_segmentation.logger"] = lg

    class Config(dict):
        pass

    mmcv = types.ModuleType("mmcv")
    mmcv.Config = Config
    sys.modules["mmcv"] = mmcv

    class EncoderDecoder(torch.nn.Module):
        pass

    mmseg = types.ModuleType("mmseg")
    mmseg_models = types.ModuleType("mmseg.models")
    mmseg_models.EncoderDecoder = EncoderDecoder
    mmseg.models = mmseg_models
    sys.modules["mmseg"], sys.modules["mmseg.models"] = mmseg, mmseg_models
    return importlib.import_module("seg_segmentation.evaluation.vit_seg")


if __name__ == "__main__":
    torch.manual_seed(0)
    vit_seg = import_vit_seg()
    spec = synth.SPECS["tiny"]
    model, _ = rh.build_reference_model(spec, {}, rank=0, world_size=1, cross_mode="t18")
    synth.apply_closed_form_weights(model)
    model.eval()
    out = {"sizes": np.array(SIZES), "cases": np.array([(int(b), n, t) for b, n, t in CASES], dtype=np.float64)}
    with torch.no_grad():
        ids = synth.synthetic_batch(spec, N_CLASSES * N_TEMPLATES, seed=77)["input_ids"][:, 0]
        ids = ids.view(N_CLASSES, N_TEMPLATES, -1)
        feats = model.clip.encode_text(ids.view(N_CLASSES * N_TEMPLATES, -1))
        emb = feats.view(N_CLASSES, N_TEMPLATES, -1).mean(dim=1)
        emb = emb / emb.norm(dim=-1, keepdim=True)
        out["prompt_ids"], out["text_feats"], out["text_embedding"] = ids.numpy(), feats.numpy(), emb.numpy()
        out["logit_scale"] = model.clip.logit_scale.detach().numpy()
        g = torch.Generator().manual_seed(654)
        for si, (H, W) in enumerate(SIZES):
            image = torch.randn(N_IMAGES, 3, H, W, generator=g)
            per = [model.clip.encode_image(image[b:b + 1], return_hidden=True) for b in range(N_IMAGES)]
            feat, hidden = torch.cat([q[0] for q in per]), torch.cat([q[1] for q in per])
            soft = torch.cat([q[2]["attns"][-1]["soft_attn"] for q in per])
            out[f"image_{si}"], out[f"feat_{si}"], out[f"hidden_{si}"] = image.numpy(), feat.numpy(), hidden.numpy()
            out[f"soft_{si}"] = soft.numpy()
            h, w = H // spec["patch"], W // spec["patch"]
            _, gap = sr.window_groups(soft.view(N_IMAGES, -1, h, w), H, W)
            print(f"size {H}x{W}: pixels with a top-two group gap below 1e-4: {int((gap < 1e-4).sum())} of {gap.numel()}, "
                  f"below 1e-6: {int((gap < 1e-6).sum())}")
            for ci, (with_bg, N, thr) in enumerate(CASES):
                seg = vit_seg.ViTSegInference(model, emb[:N].clone(), with_bg, test_cfg=dict(mode="whole", bg_thresh=thr))
                logits = torch.cat([seg.encode_decode(image[b:b + 1], None) for b in range(N_IMAGES)])
                out[f"logits_{si}_{ci}"] = logits.numpy()
                tmax = sr.group_table(hidden[:, 1:], feat, emb[:N], model.clip.logit_scale, min(5, N))["table_max"]
                assert bool((tmax < 0.95).all()) and (thr == 0.95 or bool((tmax > thr).all())), tmax
                print(f"  case {ci} with_bg={with_bg} N={N} bg_thresh={thr}: table max {tmax.tolist()}, "
                      f"background share {float((logits.argmax(1) == 0).double().mean()) if with_bg else 0:.3f}")
    path = os.path.join(HERE, "seg_tiny.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")
