"""CPU: the C-ABI library loads and exports every symbol include/segclip_hip.h declares; what _lib reads from that header
(every entry's types, every struct's layout, every constant) is what a C++ compiler reads from it; the module
mirror exposes the reference's state-dict keys; the product path refuses to run without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from segclip_amd import _lib, synth
from tests.helpers import FULL_FLAGS, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ensure_built():
    if not os.path.exists(_lib.lib_path()):
        import __graft_entry__ as ge
        ge.build()


def test_header_symbols_exported():
    _ensure_built()
    hdr = open(os.path.join(ROOT, "include", "segclip_hip.h")).read()
    names = set(re.findall(r"\b(segclip_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 30
    lib = ctypes.CDLL(_lib.lib_path())
    missing = [n for n in sorted(names) if not hasattr(lib, n)]
    assert not missing, missing
    assert set(_lib.SIGNATURES) == names, sorted(set(_lib.SIGNATURES) ^ names)


def test_library_loads_and_reports_version():
    _ensure_built()
    lib = _lib.load()
    assert lib.segclip_version() == 1
    assert lib.segclip_last_error_string() is not None


_PROBE_HEAD = """
#include "segclip_hip.h"
#include <cstddef>
#include <cstdio>
#include <type_traits>
// one letter per type as it crosses the ABI: pointer, 32-bit int, 64-bit int, size_t, float, double
template <class T> constexpr char kind() {
  using U = std::remove_all_extents_t<T>;
  return std::is_pointer_v<U> ? 'p' : std::is_same_v<U, float> ? 'f' : std::is_same_v<U, double> ? 'd' : std::is_same_v<U, size_t> ? 'z'
       : std::is_integral_v<U> && std::is_signed_v<U> && sizeof(U) == 4 ? 'i'
       : std::is_integral_v<U> && std::is_signed_v<U> && sizeof(U) == 8 ? 'l' : '?';
}
template <class R, class... A> void entry(const char* name, R (*)(A...)) {
  std::printf("%s %c(", name, kind<R>());
  (std::putchar(kind<A>()), ...);
  std::printf(")\\n");
}
#define ENTRY(f) entry(#f, (decltype(&f))nullptr);   /* the symbol is never referenced: nothing links against the library */
#define STRUCT(s) std::printf("%s %zu\\n", #s, sizeof(s));
#define FIELD(s, f) std::printf("%s.%s %zu %zu %c\\n", #s, #f, offsetof(s, f), sizeof(s::f), kind<decltype(s::f)>());
#define CONSTANT(c) std::printf("%s %lld\\n", #c, (long long)(c));
int main() {
"""


def _kind(t):
    t = getattr(t, "_type_", t) if issubclass(t, ctypes.Array) else t
    if issubclass(t, (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)):
        return "p"
    return {ctypes.c_int: "i", ctypes.c_int64: "l", ctypes.c_size_t: "z", ctypes.c_float: "f", ctypes.c_double: "d"}[t]


def test_struct_layout_matches_header(tmp_path):
    """Everything _lib derives from the header against what a C++ compiler makes of the same header: the result and parameter
    types of EVERY entry, size, and offset / size / type of every field of every struct, and the value of every constant.  The
    probe includes the header alone and references no symbol; it needs a host compiler, no hipcc and no GPU."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "the ABI test needs a host C++ compiler (c++, g++ or clang++, or $CXX)"
    body, want = [], []
    for name, (res, args) in _lib.SIGNATURES.items():
        body.append(f"ENTRY({name})")
        want.append(f"{name} {_kind(res)}({''.join(map(_kind, args))})")
    for typedef, pyname in _lib.STRUCT_NAMES.items():
        cls = getattr(_lib, pyname)
        body.append(f"STRUCT({typedef})")
        want.append(f"{typedef} {ctypes.sizeof(cls)}")
        for field, t in cls._fields_:
            body.append(f"FIELD({typedef}, {field})")
            want.append(f"{typedef}.{field} {getattr(cls, field).offset} {getattr(cls, field).size} {_kind(t)}")
    for name, value in _lib.CONSTANTS.items():
        body.append(f"CONSTANT({name})")
        want.append(f"{name} {value}")
    assert len(_lib.SIGNATURES) >= 100 and len(_lib.STRUCT_NAMES) == 10
    src = tmp_path / "abi_probe.cpp"
    src.write_text(_PROBE_HEAD + "\n".join(body) + "\nreturn 0;\n}\n")
    exe = tmp_path / "abi_probe"
    subprocess.run([cxx, "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(want)
    wrong = [f"ctypes: {w!r}  compiler: {g!r}" for w, g in zip(want, got) if w != g]
    assert not wrong, "\n".join(wrong)


def test_gemm_rejects_a_bf16_operand_without_unit_stride():
    _ensure_built()
    lib = _lib.load()
    # a descriptor with a bf16 operand that has no unit stride must be rejected host-side (no launch)
    d = _lib.GemmDesc()
    d.M = d.N = d.K = 64
    d.A = d.B = d.C = ctypes.c_void_p(16)
    d.sam, d.sak, d.sbn, d.sbk = 3, 5, 64, 1
    d.a_dtype = d.b_dtype = d.c_dtype = _lib.BF16
    rc = lib.segclip_gemm(ctypes.byref(d), None)
    assert rc == -1
    assert b"unit stride" in lib.segclip_last_error_string()


def test_state_dict_keys_match_reference():
    g = load_golden("tiny_t18.npz")
    model, _ = synth.build_model(synth.SPECS["tiny"], FULL_FLAGS, device="cpu")
    ref = set(g["grad_names"].tolist()) | set(g["none_grad"].tolist())
    assert set(model.state_dict().keys()) == ref
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert frozen == ["vis_mae_decoder.decoder_pos_embed"]


def test_no_cpu_fallback():
    """The product path must fail loudly on CPU tensors instead of silently computing elsewhere."""
    _ensure_built()
    model, _ = synth.build_model(synth.SPECS["tiny"], {}, device="cpu")
    batch = synth.synthetic_batch(synth.SPECS["tiny"], 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(batch["input_ids"], batch["segment_ids"], batch["input_mask"], batch["image"])


def test_product_does_not_import_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "segclip_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("oracle/", "").lower() or f == "synth.py" and "oracle" not in src, (dirpath, f)


def test_synthetic_generators_are_deterministic():
    a = synth.closed_form_tensor("clip.visual.proj", (8, 4))
    b = synth.closed_form_tensor("clip.visual.proj", (8, 4))
    assert torch.equal(a, b)
    b1 = synth.synthetic_batch(synth.SPECS["tiny"], 3, seed=1)
    b2 = synth.synthetic_batch(synth.SPECS["tiny"], 3, seed=1)
    assert all(torch.equal(b1[k], b2[k]) for k in b1)
    ids = b1["input_ids"][:, 0]
    assert (ids[:, 0] == synth.SPECS["tiny"]["vocab_size"] - 2).all()
    assert ((ids == synth.SPECS["tiny"]["vocab_size"] - 1).sum(-1) == 1).all()
