"""Shared test utilities (oracle-side parameter dicts, golden loading)."""
import os
import re

import numpy as np
import torch

import segclip_amd
from segclip_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FULL_FLAGS = dict(use_seglabel=True, use_vision_mae_recon=True)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segclip_hip.h")


def header_declaration(name):
    """The parameters of the entry `name` as include/segclip_hip.h words them: ["const uint8_t* pred", "int64_t n", ...].  For
    tests that pin the header's text; that the binding agrees with the header is the business of tests/test_abi.py alone."""
    m = re.search(r"^\w[\w* ]*\b" + name + r"\s*\(([^;]*)\)\s*;", open(HEADER).read(), re.M)
    assert m, f"{name} is not declared in include/segclip_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _beyond(got, ref, rtol):
    got, ref = got.double(), ref.double()
    scale = float(ref.pow(2).mean().sqrt())
    err = (got - ref).abs()
    return ~(err <= rtol * (ref.abs() + scale)), err, scale   # (a NaN is beyond any bound)


def within(got, ref, rtol):
    """check()'s bound as a predicate"""
    return not bool(_beyond(got, ref, rtol)[0].any())


def check(got, ref, rtol, what):
    """|got - ref| <= rtol * (|ref| + the rms of ref): bf16 outputs round to 2^-9 relative, fp32 ones hold the fp32 sum"""
    bad, err, scale = _beyond(got, ref, rtol)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} beyond tolerance, max err {float(err.max()):.3e} (rms {scale:.3e})"


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def oracle_params(spec, names_shapes, requires_grad=True):
    """Closed-form parameter dict keyed by reference state-dict names (same values build_model loads)."""
    from oracle import segclip_oracle as so
    P = {}
    for name, shape in names_shapes:
        if name.endswith("decoder_pos_embed"):
            if name.startswith("seq_mae_decoder."):
                t = so.position_encoding_init(shape[-2], shape[-1]).reshape(shape)
            else:
                n = (spec["image_res"] // spec["patch"])
                t = so.sincos_pos_embed_2d(shape[-1], n).reshape(shape)
            P[name] = t
            continue
        t = synth.closed_form_tensor(name, shape).float()
        P[name] = t.requires_grad_(requires_grad)
    return P


def model_param_shapes(spec, flags):
    """(name, shape) of every state-dict entry, taken from the module mirror built on CPU."""
    model, _ = synth.build_model(spec, flags, device="cpu", closed_form=False)
    return [(k, tuple(v.shape)) for k, v in model.state_dict().items()]


def noise_items(noise, flags):
    items = [("gumbel", noise["gumbel_main"])]
    if flags.get("use_vision_mae_recon"):
        items += [("rand", noise["mask_noise"]), ("gumbel", noise["gumbel_mae"])]
    return items


def tiny_seg_model(dtype=torch.float32):
    """The tiny synthetic model in eval mode on the GPU, at the compute dtype `dtype` (the caller restores the dtype)."""
    segclip_amd.set_compute_dtype(dtype)
    model, _ = synth.build_model(synth.SPECS["tiny"], {}, device="cuda:0")
    return model.eval()


class CountedEncodeImage:
    """The sizes (windows) of the encode_image calls of a model inside the block."""

    def __init__(self, model):
        self.model, self.calls = model, []

    def __enter__(self):
        real = self.model.clip.encode_image

        def counted(*a, **k):
            self.calls.append(a[0].shape[0])
            return real(*a, **k)

        self.model.clip.encode_image = counted
        return self.calls

    def __exit__(self, *exc):
        del self.model.clip.encode_image
