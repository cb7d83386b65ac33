"""ctypes binding of libsegclip_hip.so (include/segclip_hip.h).

The product path has NO CPU fallback: if the shared library is missing, or a kernel returns an
error, a RuntimeError is raised.  Device pointers come from torch tensors (torch is used for memory
and streams only); nothing of torch crosses the C ABI.
"""
import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libsegclip_hip.so")
_BUILT_HEADER_PATH = os.path.join(_HERE, "libsegclip_hip.h")   # the header as csrc/build.sh compiled it
_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "segclip_hip.h")
_lib = None

i64, i32, f32, vp = C.c_int64, C.c_int32, C.c_float, C.c_void_p

# ---------------------------------------------------------------- the ABI, read from the header
# The types that cross the ABI by value; the names of _POINTEES may stand only behind a `*`.  Any other name is an error.
_SCALARS = {"int": C.c_int, "int32_t": i32, "int64_t": i64, "float": f32, "double": C.c_double, "size_t": C.c_size_t}
_POINTEES = {"void", "char", "uint8_t", "uint16_t"}
STRUCT_NAMES = {"segclip_gemm_desc": "GemmDesc", "segclip_gemm_route": "GemmRoute", "segclip_attn_route": "AttnRoute",
                "segclip_reduce_entry": "ReduceEntry", "segclip_wgrad_item": "WgradItem", "segclip_train_ctrl": "TrainCtrl",
                "segclip_adamw_group": "AdamWGroup", "segclip_adamw_tensor": "AdamWTensor", "segclip_attn_desc": "AttnDesc",
                "segclip_resblock_fwd_desc": "ResBlockFwdDesc"}
_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_DEFINE = re.compile(r"\s*#\s*define\s+(SEGCLIP_\w+)\s+\(?(-?\d+)\)?\s*$")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_ENUM = re.compile(r"enum\s*\w*\s*\{([^{}]*)\}\s*;")
_PROTOTYPE = re.compile(r"([\w\s*]+?)\b(segclip_\w+)\s*\(([^(){};]*)\)\s*;")
_DECLARATOR = re.compile(r"\s*((?:\*\s*(?:const\s*)?)*)(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*$")


def _blank(m):
    return " " + "\n" * m.group(0).count("\n")   # keeps every line number


def _parse_header(path):
    """include/segclip_hip.h -> (name -> (restype, argtypes), typedef name -> Structure class, constant name -> int).
    Strict: beside comments and preprocessor lines, everything at file scope is a `typedef struct`, an `enum`, a prototype or the
    extern "C" wrapper, and every type name stands in the tables above.  Anything else raises and names the line; no type is
    ever guessed."""
    if not os.path.exists(path):
        raise RuntimeError(f"segclip_amd: {path} not found - the binding is read from the C header of the source tree "
                           "(include/segclip_hip.h beside the segclip_amd package). There is no built-in copy of the ABI.")
    text = re.sub(_COMMENT, _blank, open(path).read())
    signatures, structs, constants = {}, {}, {}

    def fail(pos, msg):
        raise RuntimeError(f"segclip_amd: {path}:{text.count(chr(10), 0, pos) + 1}: {msg}")

    def directive(m):   # `#define SEGCLIP_X <integer>` is a constant; a guard, #include, #if... say nothing about the ABI
        d = _DEFINE.match(m.group(0))
        if d:
            constants[d.group(1)] = int(d.group(2))
        elif re.match(r"\s*#\s*define\s+\w+\s+\S", m.group(0)):
            fail(m.start(), f"a macro that is no `SEGCLIP_X <integer>`: {m.group(0).strip()!r}")
        return _blank(m)
    text = re.sub(r"^[ \t]*#[^\n]*", directive, text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{|\}\s*\Z', _blank, text)

    def declare(decl, pos, result=False):
        """'const float* const* gamma' or 'int64_t M, N, K' or 'int32_t reserved[2]' -> [(name, ctype), ...]"""
        m = re.match(r"\s*(?:const\s+)?(\w+)\b(.*)$", decl, flags=re.S)
        base, out = (m.group(1), []) if m else fail(pos, f"cannot read the declaration {decl.strip()!r}")
        for part in m.group(2).split(","):
            d = _DECLARATOR.match(part) or fail(pos, f"cannot read the declaration {decl.strip()!r}")
            stars, name, length = d.group(1).count("*"), d.group(2), d.group(3)
            if not (base in _SCALARS or stars and (base in _POINTEES or base in structs)):
                fail(pos, f"unknown type {base + '*' * stars!r} of {name!r}")
            t = (_SCALARS[base] if not stars else C.POINTER(structs[base]) if stars == 1 and base in structs else
                 C.c_char_p if result and stars == 1 and base == "char" else vp)
            out.append((name, t * int(length) if length else t))
        return out

    def declare_each(body, start, sep):   # the declarations of a struct body or a parameter list, each with its own line
        for m in re.finditer(r"[^%s]+" % sep, body):
            if m.group(0).strip():
                yield from declare(m.group(0), start + m.start() + len(m.group(0)) - len(m.group(0).lstrip()))

    pos = re.compile(r"\s*").match(text).end()
    while pos < len(text):
        if (m := _STRUCT.match(text, pos)):
            if m.group(1) != m.group(3) or m.group(1) not in STRUCT_NAMES:
                fail(pos, f"struct {m.group(1)} has no class name in STRUCT_NAMES")
            if not re.search(r";\s*$", m.group(2)):
                fail(m.end(2), "the last member of the struct has no ';'")
            structs[m.group(1)] = type(STRUCT_NAMES[m.group(1)], (C.Structure,),
                                       {"_fields_": list(declare_each(m.group(2), m.start(2), ";")), "__doc__": m.group(1)})
        elif (m := _ENUM.match(text, pos)):
            value = -1
            for item in filter(None, (e.strip() for e in m.group(1).split(","))):
                e = re.match(r"(SEGCLIP_\w+)(?:\s*=\s*(-?\d+))?$", item) or fail(pos, f"cannot read the enumerator {item!r}")
                value = int(e.group(2)) if e.group(2) else value + 1
                constants[e.group(1)] = value
        elif (m := _PROTOTYPE.match(text, pos)):
            if m.group(2) in signatures:
                fail(pos, f"{m.group(2)} is declared twice")
            (_, restype), = declare(m.group(1) + " " + m.group(2), pos, result=True)
            params = [] if m.group(3).strip() == "void" else list(declare_each(m.group(3), m.start(3), ","))
            if any(issubclass(t, C.Array) for _, t in params):
                fail(pos, f"{m.group(2)} has an array parameter")
            signatures[m.group(2)] = (restype, [t for _, t in params])
        else:
            fail(pos, f"neither a struct, an enum nor a prototype: {text[pos:].split(chr(10), 1)[0][:80]!r}")
        pos = re.compile(r"\s*").match(text, m.end()).end()
    missing = sorted(set(STRUCT_NAMES) - set(structs))
    if missing:
        raise RuntimeError(f"segclip_amd: {path} does not define {missing}")
    return signatures, structs, constants


# name -> (restype, argtypes) of every entry; the Structure classes; every `#define SEGCLIP_X <integer>` and enumerator
SIGNATURES, _structs, CONSTANTS = _parse_header(_HEADER_PATH)
globals().update({cls.__name__: cls for cls in _structs.values()})   # GemmDesc, GemmRoute, ...: the values of STRUCT_NAMES


def const(name):
    """The header's SEGCLIP_<name>."""
    return CONSTANTS["SEGCLIP_" + name]


def _routes(prefix):
    return {v: None if k == prefix + "NONE" else k[len(prefix):].lower() for k, v in CONSTANTS.items() if k.startswith(prefix)}


F32, BF16 = const("F32"), const("BF16")
ACT_NONE, ACT_QUICK_GELU, ACT_GELU_ERF = const("ACT_NONE"), const("ACT_QUICK_GELU"), const("ACT_GELU_ERF")
GEMM_DEFER_SPLITK, GEMM_DEFER_COLSUM = const("GEMM_DEFER_SPLITK"), const("GEMM_DEFER_COLSUM")
REDUCE_SLABS, REDUCE_ROWS, REDUCE_MAX = const("REDUCE_SLABS"), const("REDUCE_ROWS"), const("REDUCE_MAX")
ATTN_FP8 = const("ATTN_FP8")
GEMM_ROUTE_FAMILIES = _routes("SEGCLIP_GEMM_ROUTE_")   # segclip_gemm_route.family
ATTN_ROUTE_KERNELS = _routes("SEGCLIP_ATTN_ROUTE_")    # segclip_attn_route.fwd_kernel / bwd_kernel


def _code_lines(path):
    """(line number, text) of every line of a header that holds code, comments dropped and white space normalised"""
    text = re.sub(_COMMENT, _blank, open(path).read())
    return [(n, " ".join(line.split())) for n, line in enumerate(text.split("\n"), 1) if line.strip()]


def _check_built_header():
    """The library must have been compiled from the header that this binding was read from (csrc/build.sh keeps a copy of what
    it compiled beside the library): a prototype, struct or table width that differs would hand the kernels wrong arguments."""
    if not os.path.exists(_BUILT_HEADER_PATH):
        raise RuntimeError(f"segclip_amd: {_BUILT_HEADER_PATH} not found - rebuild the library with segclip_amd/csrc/build.sh")
    if open(_HEADER_PATH).read() == open(_BUILT_HEADER_PATH).read():
        return
    now, built = _code_lines(_HEADER_PATH), _code_lines(_BUILT_HEADER_PATH)
    if [t for _, t in now] != [t for _, t in built]:
        (n, line), (_, was) = next((a, b) for a, b in zip(now + [(0, "")], built + [(0, "")]) if a[1] != b[1])
        raise RuntimeError(f"segclip_amd: {_LIB_PATH} was built from another {_HEADER_PATH} - rebuild it (segclip_amd/csrc/build.sh). "
                           f"First difference, line {n}: {line!r}; the library was built with {was!r}")


def lib_path():
    return _LIB_PATH


def load():
    """Load the shared library (once).  Raises RuntimeError when it is absent: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"segclip_amd: {_LIB_PATH} not found - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or segclip_amd/csrc/build.sh (hipcc, gfx950). There is no CPU / PyTorch fallback.")
    _check_built_header()
    lib = C.CDLL(_LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here means the .so is stale w.r.t. the header
        fn.restype = res
        fn.argtypes = args
    if lib.segclip_version() != const("ABI_VERSION"):
        raise RuntimeError(f"segclip_amd: ABI version mismatch: {_LIB_PATH} is version {lib.segclip_version()}, "
                           f"{_HEADER_PATH} is version {const('ABI_VERSION')}")
    _lib = lib
    return lib


class Unsupported(RuntimeError):
    """SEGCLIP_ERR_UNSUPPORTED (-2): the library has no kernel for this combination; nothing was launched."""


def check(rc, what):
    if rc != 0:
        msg = load().segclip_last_error_string().decode(errors="replace")
        raise (Unsupported if rc == const("ERR_UNSUPPORTED") else RuntimeError)(f"segclip_hip {what} failed (rc={rc}): {msg}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """hipStream_t of torch's current stream on the current device.  Called once per kernel launch (~800 per step): the raw
    accessor avoids torch.cuda.current_stream()'s Python wrappers (9 us per call = 2 ms of host time per forward)."""
    if _raw_stream is not None and _cur_device is not None:
        return C.c_void_p(_raw_stream(_cur_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"segclip_amd: unsupported dtype {t.dtype}")


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("segclip_amd: HIP kernels need device tensors (there is no CPU fallback); got a "
                           f"{t.device} tensor")
    return C.c_void_p(t.data_ptr())


def struct_ptr(t, cls):
    """ptr(t) for an argument that the header declares as a pointer to the struct `cls`."""
    return None if t is None else C.cast(ptr(t), C.POINTER(cls))


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("segclip_amd: HIP kernels need device tensors (there is no CPU fallback); got a "
                               f"{t.device} tensor")
