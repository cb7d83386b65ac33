"""Host-side operator layer: raw launches of the C-ABI kernels (p_* functions, no autograd) and the
torch.autograd.Function wrappers the module mirror (segclip_amd/modules) is built from.

torch is used for device memory (caching allocator), streams, autograd bookkeeping and
torch.distributed - every FLOP-carrying op of the hot path is a call into libsegclip_hip.so.
There is no CPU fallback: tensors must live on the GPU.

Activation dtype == compute mode: torch.float32 -> exact-f32 MFMA path, torch.bfloat16 -> bf16 MFMA
path (fp32 residual stream, fp32 parameters / parameter gradients in both modes).
"""
import collections
import ctypes as C
import math
import os
import weakref

import torch
import torch.distributed as dist
from torch.autograd import Function

from . import _lib as L
from . import config as _cfg

ACT_NONE, ACT_QUICK_GELU, ACT_GELU_ERF = L.ACT_NONE, L.ACT_QUICK_GELU, L.ACT_GELU_ERF


class _GemmProfile:
    """Optional per-launch timing of the dominant (GEMM) kernel with HIP events on the launch stream (tools/gemm_breakdown.py,
    bench.py's fallback when rocprofv3 is not usable).  Off by default; adds two event records per launch when enabled."""
    enabled = False
    records = []  # (start_event, end_event, flops, is_bf16, algorithmic bytes)

    @classmethod
    def start(cls):
        cls.enabled, cls.records = True, []

    @classmethod
    def stop(cls):
        cls.enabled = False
        torch.cuda.synchronize()
        out = [(s.elapsed_time(e) * 1e-3, f, b, nb) for s, e, f, b, nb in cls.records]
        cls.records = []
        return out


class _OpCount:
    """Algorithmic work of one model pass, per kernel class (bench.py's roofline block divides it by the kernel time
    rocprofv3 measured for the same class): records (class, flops, bytes) per launch, no device work.  Off by default."""
    enabled = False
    records = []

    @classmethod
    def start(cls):
        cls.enabled, cls.records = True, []

    @classmethod
    def stop(cls):
        cls.enabled = False
        out, cls.records = cls.records, []
        return out

    @classmethod
    def add(cls, kind, flops, nbytes):
        cls.records.append((kind, float(flops), float(nbytes)))


class ReduceQueue:
    """Deferred trailing reductions of a group of launches (one residual block's backward): the split-K combines of the
    weight gradients and the row reductions behind the LayerNorm backwards / fused bias-gradient column sums are left in
    their workspaces and combined by ONE launch per kind (segclip_reduce_multi) when the group is flushed - 2 launches
    instead of ~8 per block.  The workspaces are kept alive until the flush has been enqueued."""

    def __init__(self):
        self.slabs, self.rows, self.keep = [], [], []

    def add_slabs(self, ws, out, n_slabs, width, scale):
        e = L.ReduceEntry()
        e.src, e.out0, e.rows, e.width, e.scale, e.out_dtype = L.ptr(ws), L.ptr(out), n_slabs, width, float(scale), L.dt(out)
        self.slabs.append(e)
        self.keep.extend((ws, out))

    def add_rows(self, part, rows, width, ld, outs, seg):
        e = L.ReduceEntry()
        e.src, e.rows, e.width, e.ld, e.seg = L.ptr(part), rows, width, ld, seg
        e.out0, e.out1, e.out2 = (L.ptr(o) for o in (tuple(outs) + (None, None))[:3])
        self.rows.append(e)
        self.keep.append(part)
        self.keep.extend(o for o in outs if o is not None)

    def flush(self):
        lib = L.load()
        if not self.slabs and not self.rows:
            return
        for kind, ents in ((L.REDUCE_SLABS, self.slabs), (L.REDUCE_ROWS, self.rows)):
            for i in range(0, len(ents), L.REDUCE_MAX):
                chunk = ents[i:i + L.REDUCE_MAX]
                arr = (L.ReduceEntry * len(chunk))(*chunk)
                L.check(lib.segclip_reduce_multi(arr, len(chunk), kind, L.stream()), "reduce_multi")
        self.slabs, self.rows, self.keep = [], [], []


class WgradGroup:
    """Weight gradients dw = dy^T x of several consecutive residual blocks, collected and run as ONE launch of the
    weight-gradient kernel (segclip_wgrad_group).  A block's four gradients have 9-36 output tiles each; one by one, each is
    cut into 7-28 K ranges to fill the 256 CUs and leaves 64 MB of fp32 partial tiles to combine; grouped, the chip is full
    with 1-4 K ranges (7 vision blocks: none).  The operands stay referenced until flush(); add() hands out the result
    tensor, which is valid once flush() has been enqueued."""

    def __init__(self):
        self.items = []

    @staticmethod
    def covers(dy, x, out):
        return (dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dy.dim() == 2 and x.dim() == 2
                and dy.shape[0] == x.shape[0] and dy.shape[0] % 64 == 0 and dy.shape[1] % 256 == 0 and x.shape[1] % 256 == 0
                and dy.stride(1) == 1 and x.stride(1) == 1 and dy.stride(0) % 8 == 0 and x.stride(0) % 8 == 0
                and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
                and (out is None or (out.is_contiguous() and out.data_ptr() % 16 == 0)))

    def add(self, dy, x, out=None):
        if not self.covers(dy, x, out) or (self.items and self.items[0][0].shape[0] != dy.shape[0]) or len(self.items) >= 48:
            return p_wgrad(dy, x, out=out)
        dw = out if out is not None else _empty((dy.shape[1], x.shape[1]), torch.float32, dy)
        self.items.append((dy, x, dw))
        return dw

    def flush(self):
        if not self.items:
            return
        lib = L.load()
        items, self.items = self.items, []
        R = items[0][0].shape[0]
        arr = (L.WgradItem * len(items))()
        tiles = 0
        for a, (dy, x, dw) in zip(arr, items):
            a.dy, a.x, a.dw = L.ptr(dy), L.ptr(x), L.ptr(dw)
            a.M, a.N, a.ld_dy, a.ld_x, a.ld_dw = dy.shape[1], x.shape[1], dy.stride(0), x.stride(0), dw.stride(0)
            tiles += (dy.shape[1] // 256) * (x.shape[1] // 256)
        splits = lib.segclip_wgrad_group_splits(tiles, R // 64)
        nbytes = lib.segclip_wgrad_group_ws_bytes(arr, len(items), splits)
        ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=items[0][0].device)
        if _OpCount.enabled:   # ONE launch: its flops / algorithmic bytes are the sums over the problems
            _OpCount.add("gemm_bf16", sum(2.0 * R * dy.shape[1] * x.shape[1] for dy, x, dw in items),
                         sum(2 * R * (dy.shape[1] + x.shape[1]) + 4 * dw.numel() for dy, x, dw in items))
        try:
            L.check(lib.segclip_wgrad_group(arr, len(items), R, splits, L.ptr(ws), nbytes, L.stream()), "wgrad_group")
        except L.Unsupported:
            for dy, x, dw in items:
                p_wgrad(dy, x, out=dw)
            return
        if splits > 1:
            rq, off = ReduceQueue(), 0
            for dy, x, dw in items:
                n = dw.numel()
                rq.add_slabs(ws[off:off + splits * n], dw, splits, n, 1.0)
                off += splits * n
            rq.flush()


_PLAN_CACHE = {}


def wgrad_group_plan(nblk, tiles_blk, ksteps, gmax):
    """Sizes (in blocks, in backward order) of the weight-gradient groups of a stack of nblk equal blocks: the partition with
    the smallest modelled time (segclip_wgrad_group_model_us at the K-range count the library would choose)."""
    key = (int(nblk), int(tiles_blk), int(ksteps), int(gmax))
    if key not in _PLAN_CACHE:
        _PLAN_CACHE[key] = _wgrad_group_plan(*key)
    return list(_PLAN_CACHE[key])


def _wgrad_group_plan(nblk, tiles_blk, ksteps, gmax):
    lib = L.load()
    gmax = max(1, min(int(gmax), nblk, 48 // 4))
    cost = [0.0] * (gmax + 1)
    for n in range(1, gmax + 1):
        s = lib.segclip_wgrad_group_splits(tiles_blk * n, ksteps)
        cost[n] = lib.segclip_wgrad_group_model_us(tiles_blk * n, ksteps, s)
    best = [(0.0, [])] + [None] * nblk
    for k in range(1, nblk + 1):
        best[k] = min(((best[k - n][0] + cost[n], best[k - n][1] + [n]) for n in range(1, min(gmax, k) + 1)), key=lambda t: t[0])
    return best[nblk][1]


def _empty(shape, dtype, like):
    return torch.empty(shape, dtype=dtype, device=like.device)


# Row pitch of the MLP hidden tensors (h, act'(u), du: M x 4D bf16).  A pitch that is a multiple of 2 KiB (4D = 3072 bf16 =
# 6144 B) makes the 256-row store burst of every GEMM tile camp on a few HBM channels: with 1 KiB more per row the c_fc
# forward with its two outputs runs 385 -> 312 us, the c_proj data gradient 324 -> 290 us, and the GEMMs that read these
# tensors as their A operand 2-5 % faster (M = 50176; tools/debug/gemm_ldc_probe2.py).  _HIDDEN_PAD = extra
# elements per row.
_HIDDEN_PAD = 512


def _empty_pitched(shape, dtype, like):
    """(M, N) view of a buffer whose row pitch avoids multiples of 2 KiB (dense when the pitch is harmless or M is small)."""
    M, N = shape
    esz = torch.empty((), dtype=dtype).element_size()
    if M < 4096 or (N * esz) % 2048 != 0:
        return _empty(shape, dtype, like)
    return torch.empty((M, N + _HIDDEN_PAD), dtype=dtype, device=like.device)[:, :N]


def _off(t, off):
    if t is None:
        return None
    L.require_cuda(t)
    return C.c_void_p(t.data_ptr() + off * t.element_size())


# ------------------------------------------------------------------------------------------------
# raw launches
# ------------------------------------------------------------------------------------------------
def p_gemm(A, B, Cc, M, N, K, sa, sb, ldc, **kw):
    """C(m,n) = epi(alpha * sum_k A(m,k) B(n,k)); sa = (sam, sak), sb = (sbn, sbk) element strides.  The keywords, with their
    defaults, are those of _gemm_desc: it fills the descriptor (an unknown one is its TypeError).
    r_mod > 0: the residual of output row m is residual row m % r_mod (L.Unsupported where the library has no such kernel)."""
    lib = L.load()
    L.require_cuda(A, B, Cc)
    if (A.dtype == torch.float32 and B.dtype == torch.float32 and Cc.dtype == torch.float32
            and kw.get("nb1", 1) * kw.get("nb2", 1) == 1 and kw.get("colsum") is None and kw.get("r_mod", 0) == 0
            and M >= 256 and N >= 64 and K >= 64 and K % 8 == 0 and _cfg.f32_split
            and _gemm_f32_split(A, B, Cc, M, N, K, sa, sb, ldc, **kw)):
        return Cc
    d, _keep = _gemm_desc(lib, True, A, B, Cc, M, N, K, sa, sb, ldc, **kw)
    if _OpCount.enabled or _GemmProfile.enabled:
        nz = kw.get("nb1", 1) * kw.get("nb2", 1)
        nbytes = _gemm_algo_bytes(A, B, Cc, M, N, K, nz, kw.get("residual"), kw.get("aux"))
        if _OpCount.enabled:
            _OpCount.add("gemm_bf16" if B.dtype == torch.bfloat16 else "gemm_f32", 2.0 * M * N * K * nz, nbytes)
        if _GemmProfile.enabled:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L.check(lib.segclip_gemm(C.byref(d), L.stream()), "gemm")
            e1.record()
            _GemmProfile.records.append((e0, e1, 2.0 * M * N * K * nz, B.dtype == torch.bfloat16, nbytes))
            return Cc
    L.check(lib.segclip_gemm(C.byref(d), L.stream()), "gemm")
    return Cc


def _addr(t, off=0):
    """_off for a tensor on any device: the planner reads addresses only"""
    return None if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


class _NoQueue:
    """gemm_plan's stand-in for a ReduceQueue: the deferral flags are set, nothing is queued"""

    def add_slabs(self, *args):
        pass

    add_rows = add_slabs


def _gemm_algo_bytes(A, B, Cc, M, N, K, nz, residual, aux):
    """algorithmic bytes of a GEMM: operands read once + outputs written once"""
    return nz * (M * K * A.element_size() + N * K * B.element_size() + M * N * Cc.element_size()
                 + (M * N * residual.element_size() if residual is not None else 0)
                 + (M * N * aux.element_size() if aux is not None else 0))


def _gemm_desc(lib, cuda, A, B, Cc, M, N, K, sa, sb, ldc, *, a_off=0, b_off=0, c_off=0, bias=None, residual=None, ldr=0,
               r_off=0, aux=None, ldaux=0, act=ACT_NONE, mul_dact=False, alpha=1.0, nb1=1, nb2=1, bsA=(0, 0),
               bsB=(0, 0), bsC=(0, 0), bsR=None, colsum=None, aux_kind=0, defer=None, r_mod=0):
    """The descriptor of p_gemm's launch and the buffers it points into (column-sum partials, split-K workspace), which the
    caller keeps alive; queues the deferred reductions on `defer`.  cuda = False (gemm_plan): tensors on any device.
    This keyword list is THE keyword list of p_gemm and gemm_plan, which pass theirs on."""
    off, ptr = (_off, L.ptr) if cuda else (_addr, _addr)
    d = L.GemmDesc()
    d.A, d.B, d.C = off(A, a_off), off(B, b_off), off(Cc, c_off)
    d.bias = ptr(bias)
    d.residual = off(residual, r_off)
    d.aux = off(aux, c_off) if aux is not None else None
    d.M, d.N, d.K = M, N, K
    d.sam, d.sak = sa
    d.sbn, d.sbk = sb
    d.ldc, d.ldr, d.ldaux = ldc, ldr, ldaux
    d.nb1, d.nb2 = nb1, nb2
    d.bsA1, d.bsA2 = bsA
    d.bsB1, d.bsB2 = bsB
    d.bsC1, d.bsC2 = bsC
    d.bsR1, d.bsR2 = bsC if bsR is None else bsR
    d.a_dtype, d.b_dtype, d.c_dtype = L.dt(A), L.dt(B), L.dt(Cc)
    d.r_dtype = L.dt(residual) if residual is not None else L.F32
    if aux is not None and aux.dtype != (torch.uint8 if aux_kind == 2 else Cc.dtype):
        raise TypeError("gemm: aux dtype must equal output dtype (uint8 for aux_kind 2)")
    d.act, d.mul_dact, d.alpha, d.aux_kind = act, int(mul_dact), float(alpha), int(aux_kind)
    flags = 0
    csws = ws = None
    if colsum is not None:
        csws = torch.empty((max(M // 64, 1), N), dtype=torch.float32, device=A.device)
        d.colsum, d.colsum_ws = ptr(colsum), ptr(csws)
        if defer is not None:
            flags |= L.GEMM_DEFER_COLSUM
            defer.add_rows(csws, M // 64, N, N, (colsum,), N)
    # a workspace exists only for split-K (no epilogue operands): skip the query call on the ~60 % of launches that can never
    # have one (host time: the step is ~800 launches)
    nbytes = (lib.segclip_gemm_ws_bytes(C.byref(d))
              if (bias is None and residual is None and aux is None and act == ACT_NONE and not mul_dact) else 0)
    if nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=A.device)
        d.ws, d.ws_bytes = ptr(ws), nbytes
        # split-K: the combine can be deferred when C is one contiguous (M, N) array
        if (defer is not None and nb1 * nb2 == 1 and ldc == N and c_off == 0 and Cc.is_contiguous()
                and (M * N) % 4 == 0 and Cc.data_ptr() % 16 == 0):
            ns = lib.segclip_gemm_splits(C.byref(d))
            if ns > 1:
                flags |= L.GEMM_DEFER_SPLITK
                defer.add_slabs(ws, Cc, ns, M * N, alpha)
    d.flags = flags
    d.res_row_mod = int(r_mod)
    return d, (csws, ws)


def gemm_plan(A, B, Cc, M, N, K, sa, sb, ldc, **kw):
    """The route p_gemm would take with the same arguments (include/segclip_hip.h: segclip_gemm_plan), as gemm_last_route reports it
    afterwards; raises what p_gemm would raise before launching.  Nothing is launched and nothing queued on `defer`; the tensors
    may live on any device (only their addresses are read).  The config.f32_split rewrite is not applied: plan its bf16 problem."""
    lib = L.load()
    if kw.get("defer") is not None:
        kw["defer"] = _NoQueue()
    d, _keep = _gemm_desc(lib, False, A, B, Cc, M, N, K, sa, sb, ldc, **kw)
    r = L.GemmRoute()
    L.check(lib.segclip_gemm_plan(C.byref(d), C.byref(r), None), "gemm")
    return GemmRoute(L.GEMM_ROUTE_FAMILIES[r.family], bool(r.a_ks), bool(r.b_ks), r.tile_m, r.tile_n, r.splits, r.variant)


GemmRoute = collections.namedtuple("GemmRoute", "family a_ks b_ks tile_m tile_n splits variant")


def gemm_last_route():
    """The kernel instance the last segclip_gemm call of this thread launched (include/segclip_hip.h: segclip_gemm_last_route):
    family 'generic' / 'dma' / 'p8' / 'pq' / 'f32', or None when that call launched nothing."""
    r = L.GemmRoute()
    L.load().segclip_gemm_last_route(C.byref(r))
    return GemmRoute(L.GEMM_ROUTE_FAMILIES[r.family], bool(r.a_ks), bool(r.b_ks), r.tile_m, r.tile_n, r.splits, r.variant)


def _split3(t, off, rows, cols, ld, stack, role):
    """fp32 operand (rows x cols view at element offset `off`, row pitch ld) -> its (hi, lo) bf16 parts, three blocks along the
    contraction dimension (include/segclip_hip.h: segclip_split3_bf16)."""
    out = torch.empty((3 * rows, cols) if stack else (rows, 3 * cols), dtype=torch.bfloat16, device=t.device)
    L.check(L.load().segclip_split3_bf16(_off(t, off), L.ptr(out), rows, cols, ld, int(stack), int(role), L.stream()), "split3")
    return out


def _gemm_f32_split(A, B, Cc, M, N, K, sa, sb, ldc, a_off=0, b_off=0, **kw):
    """config.f32_split: C = epi(A B^T) for fp32 operands as ONE bf16 GEMM of contraction length 3 K over the operands' bf16 parts
    (A: hi | lo | hi, B: hi | hi | lo along k: A_hi B_hi + A_lo B_hi + A_hi B_lo, fp32 accumulators and epilogue).  Returns False
    when a layout or an epilogue has no bf16 kernel: the caller then takes the exact fp32 GEMM.  kw: p_gemm's; the operands
    are new tensors, so the (single) problem's batch keywords do not pass on."""
    (sam, sak), (sbn, sbk) = sa, sb
    epi = {k: v for k, v in kw.items() if k not in ("nb1", "nb2", "bsA", "bsB", "bsC", "bsR", "colsum", "r_mod")}
    if not ((sak == 1 or sam == 1) and (sbk == 1 or sbn == 1)):
        return False
    if (sak == 1 and (sam % 4 or K % 4)) or (sak != 1 and (sak % 4 or M % 4)) or (sbk == 1 and (sbn % 4 or K % 4)) or (sbk != 1 and (sbk % 4 or N % 4)):
        return False
    if a_off % 4 or b_off % 4:
        return False
    if sak == 1:      # A stored (M, K): blocks side by side
        A3, sa3 = _split3(A, a_off, M, K, sam, False, 0), (3 * K, 1)
    else:             # A stored (K, M), k-strided: blocks stacked along k
        A3, sa3 = _split3(A, a_off, K, M, sak, True, 0), (1, M)
    if sbk == 1:
        B3, sb3 = _split3(B, b_off, N, K, sbn, False, 1), (3 * K, 1)
    else:
        B3, sb3 = _split3(B, b_off, K, N, sbk, True, 1), (1, N)
    try:
        p_gemm(A3, B3, Cc, M, N, 3 * K, sa3, sb3, ldc, **epi)
    except L.Unsupported:
        return False
    return True


def _ld(x):
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError(f"expected a 2-D row-major view, got shape {tuple(x.shape)} strides {x.stride()}")
    return x.stride(0)


def p_cast(t, dtype):
    if t.dtype == dtype:
        return t
    t = t.contiguous()
    out = torch.empty_like(t, dtype=dtype)
    L.check(L.load().segclip_cast(L.ptr(t), L.ptr(out), t.numel(), L.dt(t), L.dt(out), L.stream()), "cast")
    return out


def p_linear(x, w, bias=None, act=ACT_NONE, residual=None, want_aux=False, out_dtype=None, w_kn=False, aux_kind=0,
             pitched=False, out=None, aux_out=None):
    """y = act(x w^T + bias) + residual.  x (M,K) view; w (N,K) [or (K,N) when w_kn]; same dtype family.
    want_aux: also return what the backward needs of the pre-activation u: u itself (aux_kind 0) or act'(u) (aux_kind 1).
    out / aux_out: preallocated y (its dtype is the output dtype) / preallocated aux in the form aux_kind names."""
    M, K = x.shape
    N = w.shape[1] if w_kn else w.shape[0]
    out_dtype = out.dtype if out is not None else (out_dtype or x.dtype)
    alloc = _empty_pitched if pitched else _empty
    y = out if out is not None else alloc((M, N), out_dtype, x)
    aux = None
    if want_aux and act != ACT_NONE:
        aux = aux_out if aux_out is not None else alloc((M, N), torch.uint8 if aux_kind == 2 else out_dtype, x)
    sb = (1, w.stride(0)) if w_kn else (w.stride(0), 1)
    try:
        p_gemm(x, w, y, M, N, K, (_ld(x), 1), sb, _ld(y), bias=bias, residual=residual,
               ldr=_ld(residual) if residual is not None else 0, aux=aux, ldaux=_ld(aux) if aux is not None else N, act=act,
               aux_kind=aux_kind)
    except L.Unsupported:
        if aux_kind != 2 or aux is None:
            raise
        # the one-byte derivative needs full 256 x 256 tiles and 16-byte aligned operands (include/segclip_hip.h): keep it
        # as bf16 instead (QuickGELU: aux_kind 1; erf-GELU: the pre-activation itself, aux_kind 0); the backward reads the
        # form off the tensor's dtype
        aux = alloc((M, N), out_dtype, x)
        p_gemm(x, w, y, M, N, K, (_ld(x), 1), sb, _ld(y), bias=bias, residual=residual,
               ldr=_ld(residual) if residual is not None else 0, aux=aux, ldaux=_ld(aux), act=act,
               aux_kind=1 if act == ACT_QUICK_GELU else 0)
    return y, aux


def fused_colsum_ok(M, N, K, dtype):
    """Shapes for which the bf16 LDS-DMA GEMM can emit the column sums of its output in the epilogue."""
    return dtype == torch.bfloat16 and M % 128 == 0 and N % 256 == 0 and K % 64 == 0     # (128: a last row of half-tiles)


def p_dgrad(dy, w, out_dtype, aux=None, act=ACT_NONE, w_kn=False, want_colsum=False, colsum_out=None, aux_kind=0, defer=None,
            pitched=False):
    """dx = dy w   [* act'(aux)]  ;  dy (M,N), w (N,K) [or (K,N) when w_kn] -> (M,K)
    want_colsum: also return the column sums of dx (= bias gradient of the Linear that produced the
    pre-activation), fused into the GEMM epilogue when the shape allows, else by the colsum kernel."""
    M, N = dy.shape
    K = w.shape[0] if w_kn else w.shape[1]
    dx = (_empty_pitched if pitched else _empty)((M, K), out_dtype, dy)
    sb = (w.stride(0), 1) if w_kn else (1, w.stride(0))
    if aux is not None and aux.dtype != (torch.uint8 if aux_kind == 2 else out_dtype):
        raise TypeError("dgrad: aux dtype must equal output dtype (uint8 for aux_kind 2)")
    cs = None
    if want_colsum and fused_colsum_ok(M, K, N, out_dtype) and dy.dtype == torch.bfloat16:
        cs = colsum_out if colsum_out is not None else _empty((K,), torch.float32, dy)
    p_gemm(dy, w, dx, M, K, N, (_ld(dy), 1), sb, _ld(dx), aux=aux, ldaux=_ld(aux) if aux is not None else K, act=act,
           mul_dact=aux is not None, colsum=cs, aux_kind=aux_kind, defer=defer)
    if want_colsum:
        return dx, (cs if cs is not None else p_colsum(dx, out=colsum_out))
    return dx


def _slot_of(w):
    """GradSync slot of a Parameter (segclip_amd/dist.py), looked up at forward time."""
    return getattr(w, "_segclip_gslot", None)


def _slot_out(slot, shape):
    """Gradient output buffer inside the parameter's all-reduce bucket (zero-copy), or None."""
    if slot is None:
        return None
    out = slot.out_buffer()
    if out is not None and tuple(out.shape) != tuple(shape):
        out = out.view(shape) if out.numel() == math.prod(shape) else None
    return out


def p_wgrad(dy, x, w_kn=False, out=None, defer=None):
    """dw = dy^T x (N,K) fp32  [or x^T dy (K,N) when w_kn];  dy (M,N), x (M,K).  `out`: preallocated fp32 result."""
    M, N = dy.shape
    K = x.shape[1]
    if w_kn:
        if x.dtype == torch.float32 and dy.dtype != torch.float32:
            x = p_cast(x, dy.dtype)
        dw = out if out is not None else _empty((K, N), torch.float32, dy)
        if dy.dtype == torch.float32 and x.dtype != torch.float32:
            dy = p_cast(dy, x.dtype)
        p_gemm(x, dy, dw, K, N, M, (1, _ld(x)), (1, _ld(dy)), N, defer=defer)
        return dw
    if x.dtype == torch.float32 and dy.dtype != torch.float32:
        x = p_cast(x, dy.dtype)  # only the A operand may be fp32 on the bf16 path
    dw = out if out is not None else _empty((N, K), torch.float32, dy)
    if (dy.dtype == torch.float32 and x.dtype == torch.float32 and N * K <= 1024 and M >= 4096 and M % 64 == 0
            and dw.is_contiguous() and defer is None):   # (the batched form has nothing to defer: a caller that wants to takes the plain path)
        # a tiny weight (the 8 x 8 Linear over the center axis of the MAE branch's ReconstructLayer, reference
        # modules/module_seg_vit.py:338-341) over many rows: ONE output tile, i.e. one workgroup walking all M rows (1.6 ms at
        # M = 12544) - instead M / 64 batched problems of 64 rows each and a column sum of their partial results
        S = M // 64
        part = _empty((S, N * K), torch.float32, dy)
        p_gemm(dy, x, part, N, K, 64, (1, _ld(dy)), (1, _ld(x)), K, nb1=S, bsA=(64 * _ld(dy), 0), bsB=(64 * _ld(x), 0),
               bsC=(N * K, 0))
        p_colsum(part, out=dw.view(N * K))
        return dw
    p_gemm(dy, x, dw, N, K, M, (1, _ld(dy)), (1, _ld(x)), K, defer=defer)
    return dw


def p_colsum(x, out=None):
    M, N = x.shape
    lib = L.load()
    if out is None:
        out = _empty((N,), torch.float32, x)
    ws = torch.empty(max(lib.segclip_colsum_ws_bytes(M, N), 4), dtype=torch.uint8, device=x.device)
    L.check(lib.segclip_colsum(L.ptr(x), L.ptr(out), L.ptr(ws), M, N, _ld(x), L.dt(x), L.stream()), "colsum")
    return out


def p_ln_fwd(x, w, b, eps, out_dtype, out=None, seg=None, stats=None):
    """seg = (seg_in, seg_out, off) with out = a (n * seg_out, cols) buffer: row r of x is written to row
    (r // seg_in) * seg_out + off + r % seg_in of out (LayerNorm into a token slice of every sample).
    stats: preallocated fp32 (mean, rstd) of `rows` entries each."""
    x = x.contiguous()
    rows, cols = x.shape
    y = out if out is not None else _empty((rows, cols), out_dtype, x)
    mean, rstd = stats if stats is not None else (_empty((rows,), torch.float32, x), _empty((rows,), torch.float32, x))
    if _OpCount.enabled:
        _OpCount.add("ln_fwd", 0, rows * cols * (x.element_size() + y.element_size()))
    if seg is None:
        L.check(L.load().segclip_layernorm_fwd(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(mean), L.ptr(rstd), rows,
                                               cols, eps, L.dt(x), L.dt(y), L.stream()), "layernorm_fwd")
    else:
        if out is None or not out.is_contiguous() or rows % seg[0] or out.numel() != rows // seg[0] * seg[1] * cols:
            raise ValueError("layernorm_fwd_seg: out must be the contiguous (rows / seg_in * seg_out, cols) buffer")
        L.check(L.load().segclip_layernorm_fwd_seg(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(mean), L.ptr(rstd), rows,
                                                   cols, eps, L.dt(x), L.dt(y), seg[0], seg[1], seg[2], L.stream()),
                "layernorm_fwd_seg")
    return y, mean, rstd


def p_ln_bwd(dy, x, w, mean, rstd, dres=None, dx_dtype=None, want_bf16=False, want_dres_colsum=False, outs=(None, None, None),
             defer=None, seg=None):
    """-> dx, dgamma, dbeta [, dx_bf16] [, colsum(dres)];  outs = preallocated (dgamma, dbeta, colsum) buffers or None.
    seg = (seg_in, seg_out, off): the rows of dy are mapped like the output of p_ln_fwd(seg=...)."""
    lib = L.load()
    dy = dy.contiguous()
    if seg is not None and (x.shape[0] % seg[0] or dy.numel() != x.shape[0] // seg[0] * seg[1] * x.shape[1]):
        raise ValueError("layernorm_bwd_seg: dy must be the contiguous (rows / seg_in * seg_out, cols) buffer")
    rows, cols = x.shape
    dx_dtype = dx_dtype or x.dtype
    dx = _empty((rows, cols), dx_dtype, x)
    dw = outs[0] if outs[0] is not None else _empty((cols,), torch.float32, x)
    db = outs[1] if outs[1] is not None else _empty((cols,), torch.float32, x)
    dx16 = _empty((rows, cols), torch.bfloat16, x) if want_bf16 else None
    dsum = None
    if want_dres_colsum and dres is not None:
        dsum = outs[2] if outs[2] is not None else _empty((cols,), torch.float32, x)
    if dres is not None:
        dres = dres.contiguous()
        if dres.dtype != dx_dtype:
            raise TypeError("layernorm_bwd: dres dtype must equal dx dtype")
    if _OpCount.enabled:
        _OpCount.add("ln_bwd", 0, rows * cols * (dy.element_size() + x.element_size() + dx.element_size() * (2 if dres is not None else 1)
                                                 + (2 if want_bf16 else 0)))
    wsb = lib.segclip_layernorm_bwd_ws_bytes(rows, cols)
    ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=x.device)
    deferred = defer is not None and rows > 0 and all(t.data_ptr() % 16 == 0 for t in (dw, db) + ((dsum,) if dsum is not None else ()))
    if seg is None:
        L.check(lib.segclip_layernorm_bwd(L.ptr(dy), L.ptr(x), L.ptr(w), L.ptr(mean), L.ptr(rstd), L.ptr(dres), L.ptr(dx),
                                          L.ptr(dx16), None if deferred else L.ptr(dw), L.ptr(db), L.ptr(dsum), L.ptr(ws), rows,
                                          cols, L.dt(dy), L.dt(x), L.dt(dx), L.stream()), "layernorm_bwd")
    else:
        L.check(lib.segclip_layernorm_bwd_seg(L.ptr(dy), L.ptr(x), L.ptr(w), L.ptr(mean), L.ptr(rstd), L.ptr(dres), L.ptr(dx),
                                              L.ptr(dx16), None if deferred else L.ptr(dw), L.ptr(db), L.ptr(dsum), L.ptr(ws),
                                              rows, cols, L.dt(dy), L.dt(x), L.dt(dx), seg[0], seg[1], seg[2], L.stream()),
                "layernorm_bwd_seg")
    if deferred:   # ws = [blocks][dgamma | dbeta | colsum(dres)] partial rows
        defer.add_rows(ws, wsb // (3 * cols * 4), (3 if dsum is not None else 2) * cols, 3 * cols, (dw, db, dsum), cols)
    out = [dx, dw, db]
    if want_bf16:
        out.append(dx16)
    if want_dres_colsum:
        out.append(dsum)
    return tuple(out)


def _attn_desc(q, k, v, o, B, H, Tq, Tk, hd, qs, ks, vs, os_, scale, causal, q_off=0, k_off=0, v_off=0, fp8=False,
               klen=None):
    d = L.AttnDesc()
    d.flags = L.ATTN_FP8 if (fp8 and klen is None) else 0
    if klen is not None:
        if klen.dtype != torch.int32 or klen.numel() != B or not klen.is_contiguous():
            raise TypeError("attention: klen must be a contiguous int32 tensor of B entries")
        L.require_cuda(klen)
        d.klen = L.ptr(klen)
    d.Q, d.K, d.V, d.O = _off(q, q_off), _off(k, k_off), _off(v, v_off), L.ptr(o)
    d.B, d.H, d.Tq, d.Tk, d.hd = B, H, Tq, Tk, hd
    d.q_sb, d.q_st = qs
    d.k_sb, d.k_st = ks
    d.v_sb, d.v_st = vs
    d.o_sb, d.o_st = os_
    d.scale, d.causal, d.dtype = float(scale), int(causal), L.dt(q)
    return d


def attn_desc_packed(qkv, o, B, H, T, causal, klen=None, fp8=False):
    """Self-attention over a packed projection: qkv holds rows of 3 * D columns (Q | K | V of one token, tokens of a sample
    in consecutive rows), o rows of D columns; the head dimension is D / H."""
    D = qkv.shape[-1] // 3
    hd = D // H
    s3 = (T * 3 * D, 3 * D)
    return _attn_desc(qkv, qkv, qkv, o, B, H, T, T, hd, s3, s3, s3, (T * D, D), 1.0 / math.sqrt(hd), causal, 0, D, 2 * D,
                      fp8=fp8, klen=klen)


AttnRoute = collections.namedtuple("AttnRoute", "fwd_kernel bwd_kernel tiles variant")


def attn_last_route():
    """The kernel instance the last segclip_attn_fwd / segclip_attn_bwd call of this thread launched
    (include/segclip_hip.h: segclip_attn_last_route): kernels by name, None in the direction that did not run."""
    r = L.AttnRoute()
    L.load().segclip_attn_last_route(C.byref(r))
    return AttnRoute(L.ATTN_ROUTE_KERNELS[r.fwd_kernel], L.ATTN_ROUTE_KERNELS[r.bwd_kernel], r.tiles, r.variant)


def p_attn_fwd(d, like, stats=None):
    """stats: optional fp32 buffer of segclip_attn_stats_bytes (the tests hand in one inside a sentinel frame)"""
    lib = L.load()
    if stats is None:
        stats = torch.empty(max(lib.segclip_attn_stats_bytes(C.byref(d)) // 4, 1), dtype=torch.float32, device=like.device)
    d.stats = L.ptr(stats)
    if _OpCount.enabled:   # QK^T + PV (causal: half), Q K V read + O written
        fl = 4.0 * d.B * d.H * d.Tq * d.Tk * d.hd * (0.5 if d.causal else 1.0)
        _OpCount.add("attn_fwd", fl, 2.0 * d.B * d.H * d.hd * (2 * d.Tq + 2 * d.Tk))
    L.check(lib.segclip_attn_fwd(C.byref(d), L.stream()), "attn_fwd")
    return stats


def p_attn_bwd(d, stats, do, dq, dk, dv, dqs, dks, dvs, dos, dq_off=0, dk_off=0, dv_off=0, colsum_part=None, ws=None):
    """colsum_part (bf16 path only): fp32 (B, 3*H*hd) buffer that receives the per-sample token sums of dQ|dK|dV.
    ws: optional workspace of at least segclip_attn_bwd_ws_bytes bytes (default: allocated here, uninitialised)."""
    lib = L.load()
    d.stats = L.ptr(stats)
    d.colsum_part = L.ptr(colsum_part)
    d.dO, d.dQ, d.dK, d.dV = L.ptr(do), _off(dq, dq_off), _off(dk, dk_off), _off(dv, dv_off)
    d.dq_sb, d.dq_st = dqs
    d.dk_sb, d.dk_st = dks
    d.dv_sb, d.dv_st = dvs
    d.do_sb, d.do_st = dos
    nbytes = lib.segclip_attn_bwd_ws_bytes(C.byref(d))
    if ws is None:
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=do.device)
    elif ws.numel() * ws.element_size() < nbytes:
        raise ValueError(f"attention backward: workspace of {ws.numel() * ws.element_size()} bytes, {nbytes} needed")
    d.ws = L.ptr(ws)
    if _OpCount.enabled:   # S, dP, dV, dK, dQ = 2.5 x forward; Q K V O dO read + dQ dK dV written
        fl = 10.0 * d.B * d.H * d.Tq * d.Tk * d.hd * (0.5 if d.causal else 1.0)
        _OpCount.add("attn_bwd", fl, 2.0 * d.B * d.H * d.hd * (4 * d.Tq + 4 * d.Tk))
    L.check(lib.segclip_attn_bwd(C.byref(d), L.stream()), "attn_bwd")


def interp_pos_table(table, h, w):
    """(1 + n*n, D) positional table -> (1 + h*w, D): class row kept, patch rows bicubically resampled
    (modules/module_clip_vtransformer.py:35-53, eval only: no gradient)."""
    n = int(round(math.sqrt(table.shape[0] - 1)))
    D = table.shape[1]
    src = table.detach().float().contiguous()
    out = torch.empty(1 + h * w, D, dtype=torch.float32, device=table.device)
    out[0] = src[0]
    L.check(L.load().segclip_interp_bicubic(_off(src, D), _off(out, D), n, h, w, D, L.stream()), "interp_bicubic")
    return out


_WCAST_PARAMS = {}  # id -> weakref of every Parameter that went through wcast (the GEMM weights)


def wcast(w, act_dtype):
    """Parameter (fp32 master) in the compute dtype of the current mode.

    bf16 copies ("shadows") live on the Parameter object as `_segclip_shadow = [tensor, version]` and are valid while
    the parameter's autograd version is unchanged.  They are written either by refresh_weight_shadows() (one
    multi-tensor cast at the start of a forward) or by the fused optimizer together with the parameter itself
    (modules/optimization_adamw.py, shadow_bf16=True).  A miss casts on the spot and registers the parameter."""
    if act_dtype == torch.bfloat16:
        sh = getattr(w, "_segclip_shadow", None)
        if sh is not None and sh[1] == w._version and sh[0].shape == w.shape:
            return sh[0]
        if isinstance(w, torch.nn.Parameter) and w.is_contiguous():
            buf = sh[0] if (sh is not None and sh[0].shape == w.shape) else torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
            p_cast_into(w.detach(), buf)
            w._segclip_shadow = [buf, w._version]
            _WCAST_PARAMS[id(w)] = weakref.ref(w)
            return buf
    return p_cast(w.detach(), act_dtype)


def p_cast_into(x, out):
    lib = L.load()
    L.check(lib.segclip_cast(L.ptr(x), L.ptr(out), x.numel(), L.dt(x), L.dt(out), L.stream()), "cast")
    return out


def refresh_weight_shadows(force=True):
    """Re-cast every registered GEMM weight in ceil(T/32) launches.  force=False trusts shadows whose version
    still matches (what the fused optimizer guarantees); force=True is the conservative per-forward behaviour."""
    todo = []
    for key, ref in list(_WCAST_PARAMS.items()):
        w = ref()
        if w is None:
            del _WCAST_PARAMS[key]
            continue
        sh = getattr(w, "_segclip_shadow", None)
        if sh is None or not w.is_cuda:
            continue
        if force or sh[1] != w._version:
            todo.append((w, sh))
    if not todo:
        return 0
    n = len(todo)
    src = (C.c_void_p * n)(*[w.data_ptr() for w, _ in todo])
    dst = (C.c_void_p * n)(*[sh[0].data_ptr() for _, sh in todo])
    cnt = (C.c_int64 * n)(*[w.numel() for w, _ in todo])
    L.check(L.load().segclip_multi_cast_bf16(C.cast(src, C.c_void_p), C.cast(dst, C.c_void_p), C.cast(cnt, C.c_void_p), n,
                                             L.stream()), "multi_cast_bf16")
    for w, sh in todo:
        sh[1] = w._version
    return n


# ------------------------------------------------------------------------------------------------
# autograd Functions
# ------------------------------------------------------------------------------------------------
class LayerNormFn(Function):
    """modules/module_clip_util.py:126-132 / nn.LayerNorm.  x (rows, cols)."""

    @staticmethod
    def forward(ctx, x, w, b, eps, out_dtype):
        x = x.contiguous()
        y, mean, rstd = p_ln_fwd(x, w, b, eps, out_dtype)
        ctx.save_for_backward(x, w, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd = ctx.saved_tensors
        dx, dw, db = p_ln_bwd(dy, x, w, mean, rstd, None, x.dtype)[:3]
        return dx, dw, db, None, None


class LayerNormCatFn(Function):
    """LayerNorm(cat([a, b], dim=1)) for a (B, Ta, D), b (B, Tb, D) WITHOUT the concatenated copy: each part is
    normalised straight into its token slice of the (B, Ta+Tb, D) result, and the backward reads each part's
    gradient from the slice.  The learnable-center cross-attention normalises cat([centers, tokens]) as its K/V input
    in both of its layers (reference modules/module_seg_vit.py:294-296 `kv = torch.cat([q, inputs], dim=1)`, :211
    `self.ln_1(k)`): 2 x (B*204*768 fp32 copy forward + its slice-copy backward) per step."""

    @staticmethod
    def forward(ctx, a, b, w, bias, eps, out_dtype):
        B, Ta, D = a.shape
        Tb = b.shape[1]
        S = Ta + Tb
        a2, b2 = a.reshape(B * Ta, D), b.reshape(B * Tb, D)
        y = _empty((B * S, D), out_dtype, a)
        _, ma, ra = p_ln_fwd(a2, w, bias, eps, out_dtype, out=y, seg=(Ta, S, 0))
        _, mb, rb = p_ln_fwd(b2, w, bias, eps, out_dtype, out=y, seg=(Tb, S, Ta))
        ctx.save_for_backward(a2, b2, w, ma, ra, mb, rb)
        ctx.dims = (B, Ta, Tb, D)
        return y.view(B, S, D)

    @staticmethod
    def backward(ctx, dy):
        a2, b2, w, ma, ra, mb, rb = ctx.saved_tensors
        B, Ta, Tb, D = ctx.dims
        S = Ta + Tb
        dy = dy.contiguous().view(B * S, D)
        da, dwa, dba = p_ln_bwd(dy, a2, w, ma, ra, None, a2.dtype, seg=(Ta, S, 0))[:3]
        db_, dwb, dbb = p_ln_bwd(dy, b2, w, mb, rb, None, b2.dtype, seg=(Tb, S, Ta))[:3]
        dwa += dwb
        dba += dbb
        return da.view(B, Ta, D), db_.view(B, Tb, D), dwa, dba, None, None


def _ptr_array(tensors):
    L.require_cuda(*tensors)
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _seg_maps(segs):
    flat = []
    for sg in segs:
        flat += [0, 0, 0] if sg is None else [int(v) for v in sg]
    return (C.c_int64 * len(flat))(*flat)


class LayerNormMultiFn(Function):
    """y_k = LayerNorm(x; w_k, b_k), k < 3, from ONE read of x (rows, D) fp32 and one (mean, rstd); backward: one dx = sum
    of the three LayerNorm backwards.  segs[k] = None (y_k is (rows, D)) or (seg_in, seg_out, off): y_k is a
    (rows / seg_in, seg_out, D) buffer of which only the token slice [off, off + seg_in) of every sample is written - the
    rest is filled in place later (LayerNormIntoFn), and the matching rows of its gradient are ignored here.
    The learnable-center stage: `self.norm(inputs)` + `ln_1(cat([q, inputs]))` of both cross-attention layers
    (reference modules/module_seg_vit.py:289,294-296,211)."""

    @staticmethod
    def forward(ctx, x, eps, out_dtype, segs, *wb):
        rows, D = x.shape
        lib = L.load()
        ys = [_empty((rows, D) if sg is None else (rows // sg[0], sg[1], D), out_dtype, x) for sg in segs]
        mean = _empty((rows,), torch.float32, x)
        rstd = _empty((rows,), torch.float32, x)
        ws, bs = wb[0::2], wb[1::2]
        L.check(lib.segclip_layernorm_fwd_multi(L.ptr(x), len(segs), _ptr_array(ws), _ptr_array(bs), _ptr_array(ys),
                                                _seg_maps(segs), L.ptr(mean), L.ptr(rstd), rows, D, eps, L.dt(x), L.dt(ys[0]),
                                                L.stream()), "layernorm_fwd_multi")
        if _OpCount.enabled:
            _OpCount.add("ln_fwd", 0, rows * D * (x.element_size() + len(segs) * ys[0].element_size()))
        ctx.save_for_backward(x, mean, rstd, *ws)
        ctx.segs, ctx.out_dtype = segs, out_dtype
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        x, mean, rstd = ctx.saved_tensors[:3]
        ws = ctx.saved_tensors[3:]
        rows, D = x.shape
        n = len(ctx.segs)
        lib = L.load()
        dys = [dy.contiguous() if dy is not None else
               torch.zeros((rows, D) if sg is None else (rows // sg[0], sg[1], D), dtype=ctx.out_dtype, device=x.device)
               for dy, sg in zip(dys, ctx.segs)]
        dx = torch.empty_like(x)
        dgb = _empty((2 * n, D), torch.float32, x)
        wsb = torch.empty(max(lib.segclip_layernorm_bwd_multi_ws_bytes(rows, D, n), 4), dtype=torch.uint8, device=x.device)
        if _OpCount.enabled:
            _OpCount.add("ln_bwd", 0, rows * D * (2 * x.element_size() + n * dys[0].element_size()))
        L.check(lib.segclip_layernorm_bwd_multi(_ptr_array(dys), L.ptr(x), n, _ptr_array(ws), _seg_maps(ctx.segs), L.ptr(mean),
                                                L.ptr(rstd), L.ptr(dx), L.ptr(dgb), L.ptr(wsb), rows, D, L.dt(dys[0]), L.dt(x),
                                                L.stream()), "layernorm_bwd_multi")
        return (dx, None, None, None) + tuple(dgb[i] for i in range(2 * n))


def layer_norm_multi(x, affines, segs, eps, out_dtype):
    """-> tuple of outputs, or None when the library has no kernel for this combination (run the single LayerNorms)."""
    wb = [t for w, b in affines for t in (w, b)]
    try:
        return LayerNormMultiFn.apply(x.contiguous(), float(eps), out_dtype, tuple(segs), *wb)
    except L.Unsupported:
        return None


class LayerNormIntoFn(Function):
    """buf[:, off:off+Ta] = LayerNorm(a) IN PLACE, for a (B, Ta, D) and a (B, S, D) buffer whose other token rows are
    already final (LayerNormMultiFn).  The gradient of buf passes through unchanged: its consumer ignores these rows."""

    @staticmethod
    def forward(ctx, buf, a, w, bias, eps, off):
        B, S, D = buf.shape
        Ta = a.shape[1]
        a2 = a.reshape(B * Ta, D)
        _, m, r = p_ln_fwd(a2, w, bias, eps, buf.dtype, out=buf.view(B * S, D), seg=(Ta, S, off))
        ctx.mark_dirty(buf)
        ctx.save_for_backward(a2, w, m, r)
        ctx.dims = (B, S, Ta, D, off)
        return buf

    @staticmethod
    def backward(ctx, dbuf):
        a2, w, m, r = ctx.saved_tensors
        B, S, Ta, D, off = ctx.dims
        dbuf = dbuf.contiguous()
        da, dw, db = p_ln_bwd(dbuf.view(B * S, D), a2, w, m, r, None, a2.dtype, seg=(Ta, S, off))[:3]
        return dbuf, da.view(B, Ta, D), dw, db, None, None


def layer_norm_into(buf, a, w, bias, eps, off=0):
    return LayerNormIntoFn.apply(buf, a.contiguous(), w, bias, float(eps), int(off))


def layer_norm_cat(a, b, w, bias, eps=1e-5, out_dtype=None):
    return LayerNormCatFn.apply(a.contiguous(), b.contiguous(), w, bias, eps, out_dtype or a.dtype)


def layer_norm(x, w, b, eps=1e-5, out_dtype=None):
    shp = x.shape
    y = LayerNormFn.apply(x.reshape(-1, shp[-1]), w, b, eps, out_dtype or x.dtype)
    return y.view(shp)


class LinearFn(Function):
    """y = act(x w^T + b) + residual (nn.Linear / `@ proj`).  x (M,K); w (N,K) or (K,N) if w_kn."""

    @staticmethod
    def forward(ctx, x, w, b, residual, act, out_dtype, act_dtype, w_kn):
        if x.dtype != act_dtype:
            x = p_cast(x, act_dtype)
        wc = wcast(w, act_dtype)
        y, aux = p_linear(x, wc, b, act, residual, want_aux=True, out_dtype=out_dtype, w_kn=w_kn)
        ctx.save_for_backward(x, wc, aux)
        ctx.act, ctx.w_kn, ctx.has_b, ctx.has_r = act, w_kn, b is not None, residual is not None
        ctx.act_dtype = act_dtype
        ctx.gslot = _slot_of(w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wc, aux = ctx.saved_tensors
        dy = dy.contiguous()
        du = dy
        if ctx.act != ACT_NONE:
            du = torch.empty_like(dy)
            L.check(L.load().segclip_act_bwd(L.ptr(dy), L.ptr(aux), L.ptr(du), dy.numel(), ctx.act, L.dt(dy),
                                             L.stream()), "act_bwd")
        db = p_colsum(du) if (ctx.has_b and ctx.needs_input_grad[2]) else None
        if du.dtype == torch.float32 and x.dtype == torch.bfloat16:
            # an fp32 output gradient (fp32 residual stream) of a bf16 Linear: the GEMMs round it to bf16 while staging
            # anyway, but an fp32 operand keeps them off the LDS-DMA kernels - round once here (same values)
            du = p_cast(du, torch.bfloat16)
        dx = p_dgrad(du, wc, x.dtype, w_kn=ctx.w_kn) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            shp = (x.shape[1], du.shape[1]) if ctx.w_kn else (du.shape[1], x.shape[1])
            dw = p_wgrad(du, x, w_kn=ctx.w_kn, out=_slot_out(ctx.gslot, shp))
        dres = dy if (ctx.has_r and ctx.needs_input_grad[3]) else None
        return dx, dw, db, dres, None, None, None, None


def linear(x, w, b=None, act=ACT_NONE, residual=None, out_dtype=None, act_dtype=None, w_kn=False):
    shp = x.shape
    act_dtype = act_dtype or x.dtype
    out_dtype = out_dtype or act_dtype
    N = w.shape[1] if w_kn else w.shape[0]
    r2 = residual.reshape(-1, N) if residual is not None else None
    y = LinearFn.apply(x.reshape(-1, shp[-1]), w, b, r2, act, out_dtype, act_dtype, w_kn)
    return y.view(*shp[:-1], N)


class BmmFn(Function):
    """C[b] = A[b] @ B[b]  (transB: A[b] @ B[b]^T).  3-D operands of one dtype with arbitrary (b, row)
    strides and unit stride on one of the two inner axes; used for the small contractions of the center
    stage (modules/module_seg_vit.py:304,309,342) and the contrastive logits (modules/modeling.py:356-357)."""

    @staticmethod
    def forward(ctx, A, B, transB, out_dtype):
        if A.dtype != B.dtype:
            raise TypeError(f"bmm: operand dtypes differ ({A.dtype} vs {B.dtype})")
        nb, M, K = A.shape
        N = B.shape[1] if transB else B.shape[2]
        Cc = _empty((nb, M, N), out_dtype, A)
        sb = (B.stride(1), B.stride(2)) if transB else (B.stride(2), B.stride(1))
        p_gemm(A, B, Cc, M, N, K, (A.stride(1), A.stride(2)), sb, N, nb1=nb, bsA=(A.stride(0), 0),
               bsB=(B.stride(0), 0), bsC=(M * N, 0))
        ctx.save_for_backward(A, B)
        ctx.transB = transB
        return Cc

    @staticmethod
    def backward(ctx, dC):
        A, B = ctx.saved_tensors
        nb, M, K = A.shape
        dC = p_cast(dC.contiguous(), A.dtype)
        N = dC.shape[2]
        dA = dB = None
        sn, sk = (B.stride(1), B.stride(2)) if ctx.transB else (B.stride(2), B.stride(1))  # Bop(n,k)
        if ctx.needs_input_grad[0]:
            # dA(m,k) = sum_n dC(m,n) Bop(n,k): contraction over n
            dA = _empty((nb, M, K), A.dtype, A)
            p_gemm(dC, B, dA, M, K, N, (N, 1), (sk, sn), K, nb1=nb, bsA=(M * N, 0), bsB=(B.stride(0), 0),
                   bsC=(M * K, 0))
        if ctx.needs_input_grad[1]:
            if ctx.transB:
                # dB(n,k) = sum_m dC(m,n) A(m,k)
                dB = _empty((nb, N, K), B.dtype, B)
                p_gemm(dC, A, dB, N, K, M, (1, N), (A.stride(2), A.stride(1)), K, nb1=nb, bsA=(M * N, 0),
                       bsB=(A.stride(0), 0), bsC=(N * K, 0))
            else:
                # dB(k,n) = sum_m A(m,k) dC(m,n)
                dB = _empty((nb, K, N), B.dtype, B)
                p_gemm(A, dC, dB, K, N, M, (A.stride(2), A.stride(1)), (1, N), N, nb1=nb, bsA=(A.stride(0), 0),
                       bsB=(M * N, 0), bsC=(K * N, 0))
        return dA, dB, None, None


def bmm(A, B, transB=False, out_dtype=None):
    return BmmFn.apply(A, B, transB, out_dtype or A.dtype)


class ActFn(Function):
    @staticmethod
    def forward(ctx, x, act):
        x = x.contiguous()
        y = torch.empty_like(x)
        L.check(L.load().segclip_act_fwd(L.ptr(x), L.ptr(y), x.numel(), act, L.dt(x), L.stream()), "act_fwd")
        ctx.save_for_backward(x)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        L.check(L.load().segclip_act_bwd(L.ptr(dy), L.ptr(x), L.ptr(dx), x.numel(), ctx.act, L.dt(x), L.stream()),
                "act_bwd")
        return dx, None


# The state of one residual block, in forward order: its parameters (also: their GradSync slots, their needs_input_grad flags,
# their gradients) and what its forward saves for the backward (weights: in the compute dtype).  Plain tuples to autograd.
BlockParams = collections.namedtuple("BlockParams", "ln1w ln1b wqkv bqkv wo bo ln2w ln2b wfc bfc wpr bpr")
BlockSaved = collections.namedtuple("BlockSaved", "x ln1w mean1 rstd1 y1 wqkv qkv o stats wo x1 ln2w mean2 rstd2 y2 wfc u h wpr")


def _block_records(kind, flat, start=0, count=None):
    """The per-block records in a flat sequence (a stack's *params, saved_tensors or needs_input_grad from `start` on)."""
    n = len(kind._fields)
    count = (len(flat) - start) // n if count is None else count
    return [kind._make(flat[start + b * n:start + (b + 1) * n]) for b in range(count)]


def _resblock_fwd_exec(s, P, xo, B, T, n_head, causal, act, eps, klen, ak):
    """config.c_exec: the block's seven forward launches enqueued by ONE C-ABI call (segclip_resblock_fwd, csrc/exec.cpp) into
    the buffers of s (BlockSaved) and xo - the same kernels with the same descriptors as the launch-by-launch path of
    _resblock_fwd, so results are bit-identical (tests/test_block_exec_gpu.py); ~60 us of host time per block instead of ~300.
    Returns False when the library has no kernel for one of the block's GEMMs in this form (the one-byte derivative off the
    256 x 256 kernel): the call plans all four before its first launch, so nothing was launched, and the caller takes the
    launch-by-launch path at the price of this one failed call."""
    M, D = s.x.shape
    d = L.ResBlockFwdDesc()
    d.x = s.x.data_ptr()
    d.ln1w, d.ln1b, d.wqkv, d.bqkv = P.ln1w.data_ptr(), P.ln1b.data_ptr(), s.wqkv.data_ptr(), P.bqkv.data_ptr()
    d.wo, d.bo, d.ln2w, d.ln2b = s.wo.data_ptr(), P.bo.data_ptr(), P.ln2w.data_ptr(), P.ln2b.data_ptr()
    d.wfc, d.bfc, d.wpr, d.bpr = s.wfc.data_ptr(), P.bfc.data_ptr(), s.wpr.data_ptr(), P.bpr.data_ptr()
    d.y1, d.mean1, d.rstd1 = s.y1.data_ptr(), s.mean1.data_ptr(), s.rstd1.data_ptr()
    d.qkv, d.o, d.stats, d.x1 = s.qkv.data_ptr(), s.o.data_ptr(), s.stats.data_ptr(), s.x1.data_ptr()
    d.y2, d.mean2, d.rstd2 = s.y2.data_ptr(), s.mean2.data_ptr(), s.rstd2.data_ptr()
    d.h, d.ld_h = s.h.data_ptr(), s.h.stride(0)
    if s.u is not None:
        d.u, d.ld_u = s.u.data_ptr(), s.u.stride(0)
    d.xo = xo.data_ptr()
    if klen is not None:
        d.klen = klen.data_ptr()
    d.M, d.B, d.T, d.D, d.F, d.H = M, B, T, D, s.wfc.shape[0], n_head
    d.eps, d.attn_scale = float(eps), 1.0 / math.sqrt(D // n_head)
    d.causal, d.act, d.aux_kind, d.x_dtype = int(causal), int(act), int(ak), L.dt(s.x)
    try:
        L.check(L.load().segclip_resblock_fwd(C.byref(d), L.stream()), "resblock_fwd")
    except L.Unsupported:
        return False
    return True


def _resblock_fwd(x2, P, B, T, n_head, causal, act, eps, act_dtype, klen):
    """One pre-LN residual block on the (B*T, D) residual stream x2 - fp32, or bf16 inside a ResStackFn running with
    config.bf16_resid - : returns (x_out (B*T, D) in the stream's dtype, the BlockSaved for the backward).  The buffers and the
    BlockSaved are built once, here; one segclip_resblock_fwd call (config.c_exec) or seven p_* launches fill them."""
    P = BlockParams._make(P)
    M, D = x2.shape
    F4 = P.wfc.shape[0]
    for w in P:
        sl = _slot_of(w)
        if sl is not None:
            sl.note_forward_use()
    bf = act_dtype == torch.bfloat16
    fp8 = bf and bool(_cfg.attn_fp8)
    wqkv_c, wo_c, wfc_c, wpr_c = (wcast(w, act_dtype) for w in (P.wqkv, P.wo, P.wfc, P.wpr))
    ak = _aux_kind(act_dtype, act, M, F4)
    hidden = _empty_pitched if bf else _empty
    y1, y2, o = (_empty((M, D), act_dtype, x2) for _ in range(3))
    qkv = _empty((M, 3 * D), act_dtype, x2)
    mean1, rstd1, mean2, rstd2 = _empty((4, M), torch.float32, x2).unbind(0)
    x1, xo = _empty((M, D), x2.dtype, x2), _empty((M, D), x2.dtype, x2)
    h = hidden((M, F4), act_dtype, x2)
    # bf16 mode: the c_fc epilogue stores act'(u) (its exponential is already there), the c_proj dgrad multiplies by it
    u = hidden((M, F4), torch.uint8 if ak == 2 else act_dtype, x2) if act != ACT_NONE else None
    ad = attn_desc_packed(qkv, o, B, n_head, T, causal, klen=klen, fp8=fp8)      # (checks klen)
    stats = _empty((max(L.load().segclip_attn_stats_bytes(C.byref(ad)) // 4, 1),), torch.float32, x2)
    s = BlockSaved(x=x2, ln1w=P.ln1w, mean1=mean1, rstd1=rstd1, y1=y1, wqkv=wqkv_c, qkv=qkv, o=o, stats=stats, wo=wo_c, x1=x1,
                   ln2w=P.ln2w, mean2=mean2, rstd2=rstd2, y2=y2, wfc=wfc_c, u=u, h=h, wpr=wpr_c)
    if (bf and _cfg.c_exec and not _OpCount.enabled and not _GemmProfile.enabled and not fp8 and x2.is_contiguous() and D % 8 == 0
            and _resblock_fwd_exec(s, P, xo, B, T, n_head, causal, act, eps, klen, ak)):
        return xo, s
    p_ln_fwd(x2, P.ln1w, P.ln1b, eps, act_dtype, out=y1, stats=(mean1, rstd1))
    p_linear(y1, wqkv_c, P.bqkv, out=qkv)
    if M > B * T:                 # row-padded stack (ResStackFn): the attention kernel writes the B * T token rows only
        o[B * T:].zero_()
    p_attn_fwd(ad, x2, stats=stats)
    p_linear(o, wo_c, P.bo, residual=x2, out=x1)
    p_ln_fwd(x1, P.ln2w, P.ln2b, eps, act_dtype, out=y2, stats=(mean2, rstd2))
    _, u = p_linear(y2, wfc_c, P.bfc, act=act, want_aux=True, aux_kind=ak, pitched=bf, out=h, aux_out=u)
    p_linear(h, wpr_c, P.bpr, residual=x1, out=xo)
    return xo, s._replace(u=u)      # (p_linear keeps a refused one-byte derivative as bf16: the backward reads the form off u.dtype)


def _aux_kind(act_dtype, act, M=0, N=0):
    """What the residual blocks keep of the MLP pre-activation in bf16 mode: act'(u), as one byte per element (aux_kind 2,
    config.aux_u8: half the bytes of the block's largest side tensor; absolute error <= 0.0025 for QuickGELU, about 0.0065 for
    the erf-GELU of the MAE decoders, whose derivative spans [-0.129, 1.129]) when the GEMM runs on 256 x 256 tiles (rows a
    multiple of 128); else act'(u) as bf16 for QuickGELU and u itself for erf-GELU.  u itself in the exact-f32 mode."""
    if act_dtype == torch.bfloat16 and act in (ACT_QUICK_GELU, ACT_GELU_ERF):
        # round 6: the MAE decoders' erf-GELU keeps the one-byte derivative as well where the 256 x 256-tile GEMM takes the shape
        # (c_fc forward 172 -> 9x us, the c_proj data gradient no longer re-evaluates erf per element: 247 -> 1xx us at M = 50432)
        if _cfg.aux_u8 and M > 0 and M % 128 == 0 and N % 256 == 0:
            return 2
        return 1 if act == ACT_QUICK_GELU else 0
    return 0


def _resblock_bwd(s, cfg, klen, slots, need, g, g16, chain, wgroup=None, rqueue=None):
    """Hand-scheduled backward of one block.  s: its BlockSaved; slots: the BlockParams of the parameters' GradSync slots (or
    None each); need: the BlockParams of "gradient wanted" flags.  g: fp32 (M, D) gradient of the block output or None; g16:
    its bf16 copy or None.
    chain=False: fp32 residual gradient in and out (plus the bf16 copy the LayerNorm backward emits for free).
    chain=True (bf16 mode inside ResStackFn): the residual gradient travels between the LayerNorm backwards as ONE bf16
    tensor (read 2 + written 2 bytes per element instead of 4 + 4 + 2): g may be None, returns dx fp32 = None.
    -> (dx fp32 or None, dx bf16 or None, the parameter gradients as a BlockParams)"""
    B, T, D, n_head, causal, act, act_dtype = cfg
    M = s.x.shape[0]              # B * T, or that rounded up to 128 rows in a row-padded stack (pad rows: zero gradients)
    bf = act_dtype == torch.bfloat16
    # bf16 mode: the residual-stream gradients feed the GEMMs as bf16 copies (all GEMMs then run on the LDS-DMA
    # kernels and read half the bytes); the copy of dx comes for free out of the LayerNorm backward.
    if bf and g16 is None:
        g16 = p_cast(g, act_dtype)
    if not bf:
        g16 = g
    res_in = g16 if chain else g
    rdt = act_dtype if chain else torch.float32
    F4 = s.wfc.shape[0]

    # the block's trailing reductions (split-K combines, LayerNorm / bias column sums) are queued and flushed as two
    # launches at the end of the block
    # rqueue (ResStackFn with grouped weight gradients): the caller's queue - the trailing reductions of all blocks of a group
    # are flushed together (2 launches per 16 entries instead of 2 per block)
    rq = ReduceQueue() if rqueue is None else rqueue

    def wgrad(dy_, x_, out_):
        # wgroup (ResStackFn): the weight gradients of several blocks run later, as one grouped launch (WgradGroup)
        if wgroup is not None:
            return wgroup.add(dy_, x_, out_)
        return p_wgrad(dy_, x_, out=out_, defer=rq)

    def vec_out(slot, wanted, n):   # a vector gradient lands directly in its all-reduce bucket (segclip_amd/dist.py), as the weights' do
        return _slot_out(slot, (n,)) if wanted else None
    # ---- MLP
    du, dbfc = p_dgrad(g16, s.wpr, act_dtype, aux=s.u, act=act, want_colsum=True, colsum_out=vec_out(slots.bfc, need.bfc, F4),
                       aux_kind=2 if s.u.dtype == torch.uint8 else _aux_kind(act_dtype, act),
                       defer=rq, pitched=bf)  # (dy c_proj)*act'(u), colsum
    dwpr = wgrad(g16, s.h, _slot_out(slots.wpr, (D, F4))) if need.wpr else None
    dy2 = p_dgrad(du, s.wfc, act_dtype)
    dwfc = wgrad(du, s.y2, _slot_out(slots.wfc, (F4, D))) if need.wfc else None
    two = bf and not chain   # fp32 dx + its bf16 copy
    r = p_ln_bwd(dy2, s.x1, s.ln2w, s.mean2, s.rstd2, dres=res_in, dx_dtype=rdt, want_bf16=two, want_dres_colsum=True,
                 outs=(vec_out(slots.ln2w, need.ln2w, D), vec_out(slots.ln2b, need.ln2b, D), vec_out(slots.bpr, need.bpr, D)), defer=rq)
    dx1, dln2w, dln2b = r[0], r[1], r[2]
    dx1_16 = r[3] if two else dx1
    dbpr = r[-1] if need.bpr else None                           # colsum(g), fused into the LN2 backward
    # ---- attention
    do = p_dgrad(dx1_16, s.wo, act_dtype)
    dwo = wgrad(dx1_16, s.o, _slot_out(slots.wo, (D, D))) if need.wo else None
    dqkv = _empty((M, 3 * D), act_dtype, s.x)
    if M > B * T:
        dqkv[B * T:].zero_()      # the attention backward writes the token rows; a pad row must contribute exact zeros downstream
    s3 = (T * 3 * D, 3 * D)
    ad = attn_desc_packed(s.qkv, s.o, B, n_head, T, causal, klen=klen)
    part = _empty((B, 3 * D), torch.float32, s.x) if (bf and need.bqkv) else None  # in_proj bias gradient per sample
    p_attn_bwd(ad, s.stats, do, dqkv, dqkv, dqkv, s3, s3, s3, (T * D, D), 0, D, 2 * D, colsum_part=part)
    dy1 = p_dgrad(dqkv, s.wqkv, act_dtype)
    dwqkv = wgrad(dqkv, s.y1, _slot_out(slots.wqkv, (3 * D, D))) if need.wqkv else None
    dbqkv = None
    if need.bqkv:
        bq_out = _slot_out(slots.bqkv, (3 * D,))
        if part is not None and (bq_out is None or bq_out.data_ptr() % 16 == 0):
            # in_proj bias gradient = token sums of dQ|dK|dV, left per sample by the attention backward: its B partial rows
            # join the block's ONE row-reduction launch (was: a column-sum launch + its reduction per block)
            dbqkv = bq_out if bq_out is not None else _empty((3 * D,), torch.float32, s.x)
            rq.add_rows(part, B, 3 * D, 3 * D, (dbqkv,), 3 * D)
        else:
            dbqkv = p_colsum(part if part is not None else dqkv, out=bq_out)
    r = p_ln_bwd(dy1, s.x, s.ln1w, s.mean1, s.rstd1, dres=dx1, dx_dtype=rdt, want_bf16=two, want_dres_colsum=True,
                 outs=(vec_out(slots.ln1w, need.ln1w, D), vec_out(slots.ln1b, need.ln1b, D), vec_out(slots.bo, need.bo, D)), defer=rq)
    if rqueue is None:
        rq.flush()
    dbo = r[-1] if need.bo else None                             # colsum(dx1), fused into the LN1 backward
    dx32 = None if chain else r[0]
    dx16 = r[0] if chain else (r[3] if two else None)
    return dx32, dx16, BlockParams(ln1w=r[1], ln1b=r[2], wqkv=dwqkv, bqkv=dbqkv, wo=dwo, bo=dbo, ln2w=dln2w, ln2b=dln2b, wfc=dwfc,
                                   bfc=dbfc, wpr=dwpr, bpr=dbpr)


def _bf16_side_copy(g):
    """The bf16 copy of the gradient g that its producer's LayerNorm backward left on it (attribute _segclip_bf16 of the same
    tensor object), or None: it must be of g's size, on g's device, and g contiguous, to be viewed like g."""
    st = getattr(g, "_segclip_bf16", None)
    if st is not None and (st.numel() != g.numel() or st.device != g.device or not g.is_contiguous()):
        return None
    return st


def _pad_rows(t, Mp):
    """(M, D) -> (Mp, D): the rows of t, then zero rows"""
    M = t.shape[0]
    padded = _empty((Mp, t.shape[1]), t.dtype, t)
    padded[:M].copy_(t)
    padded[M:].zero_()
    return padded


class ResBlockFn(Function):
    """Fused pre-LN residual attention block (modules/module_clip_ttransformer.py:20-37,
    module_seg_vit.py:175-196, module_mae.py:185-201):
        x += out_proj(MHA(LN1 x));  x += c_proj(act(c_fc(LN2 x)))
    x (B,T,D) fp32 residual stream.  Backward is hand-scheduled: residual-gradient adds are fused into
    the LayerNorm backward, act' into the c_proj dgrad epilogue, and no gradient is re-read."""

    @staticmethod
    def forward(ctx, x, ln1w, ln1b, wqkv, bqkv, wo, bo, ln2w, ln2b, wfc, bfc, wpr, bpr, n_head, causal, act, eps,
                act_dtype, klen=None):
        B, T, D = x.shape
        x2 = x.contiguous().view(B * T, D)
        P = BlockParams(ln1w, ln1b, wqkv, bqkv, wo, bo, ln2w, ln2b, wfc, bfc, wpr, bpr)
        xo, saved = _resblock_fwd(x2, P, B, T, n_head, causal, act, eps, act_dtype, klen)
        ctx.save_for_backward(*saved)
        ctx.cfg = (B, T, D, n_head, causal, act, act_dtype)
        ctx.klen = klen
        ctx.slots = BlockParams._make(_slot_of(w) for w in P)
        _GradFold.other[id(ln1w)] = weakref.ref(ln1w)        # a producer that does not fold: its block's gradients go the engine's way
        return xo.view(B, T, D)

    @staticmethod
    def backward(ctx, g):
        B, T, D, n_head, causal, act, act_dtype = ctx.cfg
        M = B * T
        st = _bf16_side_copy(g)   # left by the next block's LayerNorm backward
        g = g.contiguous().view(M, D)
        g16 = st.view(M, D) if (st is not None and act_dtype == torch.bfloat16) else None
        (need,) = _block_records(BlockParams, ctx.needs_input_grad, start=1, count=1)     # (after x)
        dx, dx16, grads = _resblock_bwd(BlockSaved._make(ctx.saved_tensors), ctx.cfg, ctx.klen, ctx.slots, need, g, g16, False)
        dx = dx.view(B, T, D)
        if dx16 is not None:
            dx._segclip_bf16 = dx16.view(B, T, D)
        return (dx,) + grads + (None, None, None, None, None, None)


class _GradFold:
    """config.fold_param_grads: the first gradient a parameter receives in a backward pass is remembered (and goes to autograd
    as usual: it sits in the engine's input buffer until every producer of that parameter has run); a later gradient of the
    same pass is added INTO that tensor by one multi-tensor launch per caller and autograd gets None for it.  An entry is
    valid for one pass: the epoch advances when the pass ends (engine callback) and at every model forward (a backward that
    raised never ran its callback)."""
    epoch = 0
    armed = -1
    first = {}
    uses = {}      # id(first parameter of a block) -> ResStackFn forwards over that block since the last advance(): armed from 2
    other = {}     # id(first parameter of a block) -> weak reference to it, for blocks a NON-stack node (ResBlockFn) used since the last advance(): never folded.
    #                Folding is only sound while every producer of a parameter's gradient in the pass is a folding ResStackFn node: a
    #                gradient delivered by another producer in between makes the engine build a NEW sum tensor (the alias below raises
    #                the storage's use count), and a later in-place add would land in the stale one

    @classmethod
    def advance(cls):
        cls.epoch += 1
        cls.first.clear()
        cls.uses.clear()
        cls.other.clear()

    @classmethod
    def used_elsewhere(cls, p):
        r = cls.other.get(id(p))
        return r is not None and r() is p      # (an id alone may be a dead tensor's, reused)

    @classmethod
    def take(cls, p, gr, adds):
        """gr: this node's gradient of parameter p -> what the node returns to autograd for it"""
        if gr is None or gr.dtype != torch.float32 or not gr.is_contiguous():
            return gr
        ent = cls.first.get(id(p))
        if ent is not None and ent[0] == cls.epoch and ent[1].shape == gr.shape and ent[1].device == gr.device:
            adds.append((ent[1], gr))
            return None
        # an ALIAS of the gradient (same storage, its own TensorImpl): AccumulateGrad takes an incoming gradient over without
        # a copy only while nothing else references that tensor object - a plain reference here costs one clone per parameter
        cls.first[id(p)] = (cls.epoch, gr.detach())
        if cls.armed != cls.epoch:
            cls.armed = cls.epoch
            torch.autograd.Variable._execution_engine.queue_callback(cls.advance)
        return gr

    @staticmethod
    def flush(adds):
        if not adds:
            return
        n = len(adds)
        dst = (C.c_void_p * n)(*[d.data_ptr() for d, _ in adds])
        src = (C.c_void_p * n)(*[s_.data_ptr() for _, s_ in adds])
        cnt = (C.c_int64 * n)(*[d.numel() for d, _ in adds])
        L.check(L.load().segclip_multi_add_f32(C.cast(dst, C.c_void_p), C.cast(src, C.c_void_p), C.cast(cnt, C.c_void_p), n,
                                               L.stream()), "multi_add_f32")
        adds.clear()


class ResStackFn(Function):
    """N consecutive ResBlockFn blocks as ONE autograd node (the towers: 10 + 2 vision blocks, 12 text blocks).  Inside
    the node the gradients travel between the blocks as plain tensors, so in bf16 mode (config.bf16_resgrad) the
    residual-stream gradient is a single bf16 tensor per LayerNorm backward (10 instead of 16 bytes per element); the
    node's own input / output gradients stay fp32.  With segclip_amd.dist.GradSync active, each block's parameter
    gradients are published (p.grad = bucket slot, ready hook) as soon as the block's backward has been enqueued, not
    when the whole stack returns, so the bucket all-reduces keep overlapping with the rest of the backward.
    inputs: x, n_head, causal, act, eps, act_dtype, klen, chain, keep16, then 12 parameters per block."""

    NP = len(BlockParams._fields)

    @staticmethod
    def forward(ctx, x, n_head, causal, act, eps, act_dtype, klen, chain, keep16, *params):
        B, T, D = x.shape
        blocks = _block_records(BlockParams, params)
        cur = x.contiguous().view(B * T, D)
        # config.pad_rows (bf16 mode): a token-row count that is not a multiple of 128 (the text tower's B x 77 at any batch
        # that is not a multiple of 128 samples) keeps every GEMM of the stack off the 256 x 256-tile kernel, off the one-byte
        # derivative and - when it is not a multiple of 64 either - off the grouped weight gradients.  The stack then runs on
        # M rounded up to 128 rows: pad rows start as zeros, every operator of a block is row-wise except attention (which
        # only touches the B * T token rows; its outputs' pad rows are zeroed), so pad rows stay finite, carry exactly zero
        # gradients and contribute exact zeros to every weight / bias gradient.
        M = B * T
        Mp = 128 * -(-M // 128) if (act_dtype == torch.bfloat16 and bool(_cfg.pad_rows) and M % 128 != 0 and M >= _PAD_ROWS_MIN) else M
        ctx.Mp = Mp
        # config.bf16_resid (bf16 mode): the residual stream is bf16 between the blocks of the stack (the out_proj / c_proj
        # epilogues read and write 2 instead of 4 bytes per element and run on gemm_bf16_pq.hip; every LayerNorm pass reads
        # 2 bytes less).  Input / output of the node: fp32, or bf16 when the neighbouring node is a stack too (keep16).
        ctx.in_dtype = x.dtype
        resid16 = act_dtype == torch.bfloat16 and (bool(_cfg.bf16_resid) or x.dtype == torch.bfloat16)
        if resid16 and cur.dtype != torch.bfloat16:
            cur = p_cast(cur, torch.bfloat16)
        elif not resid16 and cur.dtype != torch.float32:
            cur = p_cast(cur, torch.float32)
        if Mp != M:
            cur = _pad_rows(cur, Mp)
        saved = []
        for P in blocks:
            cur, sv = _resblock_fwd(cur, P, B, T, n_head, causal, act, eps, act_dtype, klen)
            saved.extend(sv)
        if Mp != M:
            cur = cur[:M]
        ctx.save_for_backward(*saved)
        ctx.cfg = (B, T, D, n_head, causal, act, act_dtype)
        ctx.klen = klen
        ctx.chain = (bool(chain) or resid16) and act_dtype == torch.bfloat16
        ctx.wgrad_group, ctx.wgrad_group_dist = int(_cfg.wgrad_group_blocks), int(_cfg.wgrad_group_blocks_dist)
        ctx.fold = bool(_cfg.fold_param_grads) and len(params) > 0
        if ctx.fold:     # per block (the same blocks may be cut into different stacks by the two passes)
            for P in blocks:
                k = id(P.ln1w)       # (a block is known by its first parameter)
                _GradFold.uses[k] = _GradFold.uses.get(k, 0) + 1
        ctx.blocks = blocks
        ctx.slots = [BlockParams._make(_slot_of(w) for w in P) for P in blocks]
        if resid16 and not keep16:
            cur = p_cast(cur, torch.float32)
        return cur.view(B, T, D)

    @staticmethod
    def backward(ctx, g):
        B, T, D, n_head, causal, act, act_dtype = ctx.cfg
        M, nblk = B * T, len(ctx.blocks)
        Mp = ctx.Mp
        bf = act_dtype == torch.bfloat16
        st = _bf16_side_copy(g)
        g = g.contiguous().view(M, D)
        if Mp != M:               # row-padded stack: the gradient of a pad row is zero
            st = None
            g, M = _pad_rows(g, Mp), Mp
        cur16 = st.view(M, D) if (st is not None and bf) else None
        if bf and cur16 is None and g.dtype == torch.bfloat16:   # bf16 output of the node (keep16)
            cur16 = g
        if ctx.chain and cur16 is None:
            cur16 = p_cast(g, act_dtype)
        cur32 = None if ctx.chain else (g if g.dtype == torch.float32 else p_cast(g, torch.float32))
        saved = _block_records(BlockSaved, ctx.saved_tensors)
        needs = _block_records(BlockParams, ctx.needs_input_grad, start=len(ctx.needs_input_grad) - nblk * ResStackFn.NP)
        out = [None] * nblk       # per block: what autograd gets for its parameters
        # config.wgrad_group_blocks (captured at forward time): the weight gradients of up to that many consecutive blocks run
        # as one grouped launch (WgradGroup); with GradSync slots the groups stay short so that the bucket exchanges keep
        # overlapping with the backward pass.  A block's gradients are published when its group has been enqueued.
        wg, sizes = None, []
        if ctx.wgrad_group > 1 and ctx.cfg[-1] == torch.bfloat16 and nblk > 1:
            Dm, F4 = ctx.blocks[0].wqkv.shape[1], ctx.blocks[0].wfc.shape[0]
            if Dm % 256 == 0 and F4 % 256 == 0 and Mp % 64 == 0:
                no_slots = all(s is None for sl in ctx.slots for s in sl)
                gmax = ctx.wgrad_group if no_slots else min(ctx.wgrad_group, ctx.wgrad_group_dist)
                tiles_blk = (4 * Dm * Dm + 2 * F4 * Dm) // 65536
                sizes = wgrad_group_plan(nblk, tiles_blk, Mp // 64, gmax)
                wg = WgradGroup() if max(sizes) > 1 else None
        left = sizes.pop(0) if wg is not None else 0
        grq = ReduceQueue() if wg is not None else None
        pending = []
        adds = []
        for b in reversed(range(nblk)):
            cur32, cur16, grads = _resblock_bwd(saved[b], ctx.cfg, ctx.klen, ctx.slots[b], needs[b], cur32, cur16, ctx.chain, wg, grq)
            pending.append((b, ctx.blocks[b], ctx.slots[b], grads))
            if wg is not None:
                left -= 1
                if left > 0 and b > 0:
                    continue
                wg.flush()
                if grq is not None:
                    grq.flush()
                left = sizes.pop(0) if sizes else nblk
            for b_, P_, sl_, grads_ in pending:
                fold = ctx.fold and _GradFold.uses.get(id(P_.ln1w), 0) > 1 and not _GradFold.used_elsewhere(P_.ln1w)   # only blocks a second STACK node of this pass shares
                given = out[b_] = list(grads_)
                for i, (p, gr, slot) in enumerate(zip(P_, grads_, sl_)):
                    if gr is None:
                        continue
                    owner = slot.owner() if slot is not None else None
                    if owner is not None and gr.data_ptr() == slot.ptr and p.grad is None and slot.single_use():
                        # zero-copy gradient inside its all-reduce bucket: publish it now (autograd gets None for it)
                        p.grad = gr
                        owner._on_grad(p)
                        given[i] = None
                    elif fold and slot is None:
                        given[i] = _GradFold.take(p, gr, adds)
            pending = []
        _GradFold.flush(adds)
        if Mp != B * T:                      # row-padded stack: back to the token rows
            cur16 = cur16[:B * T] if cur16 is not None else None
            cur32 = cur32[:B * T] if cur32 is not None else None
        if ctx.chain and ctx.in_dtype == torch.bfloat16:
            dx = cur16                       # the producer is a stack with a bf16 output: no cast, no side copy
        elif ctx.chain:
            dx = p_cast(cur16, torch.float32)
        else:
            dx = cur32
        dx = dx.view(B, T, D)
        if cur16 is not None and dx.dtype != torch.bfloat16:
            dx._segclip_bf16 = cur16.view(B, T, D)
        return (dx, None, None, None, None, None, None, None, None) + tuple(gr for given in out for gr in given)


def res_stack(x, blocks_params, n_head, causal, act, eps, act_dtype, klen=None, keep16=False):
    """Run consecutive residual blocks (each a 12-tuple of parameters in ResBlockFn order) as one ResStackFn node.
    keep16 (config.bf16_resid only): hand the bf16 residual stream to the caller as it is - for the next stack."""
    flat = [p for P in blocks_params for p in P]
    keep16 = bool(keep16) and bool(_cfg.bf16_resid) and act_dtype == torch.bfloat16
    return ResStackFn.apply(x, n_head, causal, act, eps, act_dtype, klen, bool(_cfg.bf16_resgrad), keep16, *flat)


def _cross_attn_desc(qp, kv, o, B, G, S, n_head, mode):
    """Cross attention of queries qp (B*G, D) against kv (B*S, 2D) = [K | V] into o: the descriptor, and the (sample, token)
    strides of the q-side and the kv-side tensors, which p_attn_bwd takes for the gradients too.
    mode "t18": the torch-1.8 key reshape reinterprets the (B,S,D) buffer as (S,B,D): sample b attends to
    flat tokens {r*B + b} (SURVEY.md finding 0.4).  mode "intended": its own S tokens."""
    D = qp.shape[1]
    hd = D // n_head
    qs = (G * D, D)
    ks = (2 * D, B * 2 * D) if mode == "t18" else (S * 2 * D, 2 * D)
    return _attn_desc(qp, kv, kv, o, B, n_head, G, S, hd, qs, ks, ks, qs, 1.0 / math.sqrt(hd), False, 0, 0, D), qs, ks


class CrossAttnFn(Function):
    """Attention core of CrossAttentionBlock (modules/module_seg_vit.py:215): queries (B*G, D) against
    the projected [centers; patches] buffer kv (B*S, 2D) = [K | V]; mode: see _cross_attn_desc."""

    @staticmethod
    def forward(ctx, qp, kv, B, G, S, n_head, mode):
        o = torch.empty_like(qp)
        ad, _, _ = _cross_attn_desc(qp, kv, o, B, G, S, n_head, mode)
        stats = p_attn_fwd(ad, qp)
        ctx.save_for_backward(qp, kv, o, stats)
        ctx.cfg = (B, G, S, n_head, mode)
        return o

    @staticmethod
    def backward(ctx, do):
        qp, kv, o, stats = ctx.saved_tensors
        B, G, S, n_head, mode = ctx.cfg
        D = qp.shape[1]
        do = do.contiguous()
        ad, qs, ks = _cross_attn_desc(qp, kv, o, B, G, S, n_head, mode)
        dq = torch.empty_like(qp)
        dkv = torch.empty_like(kv)
        p_attn_bwd(ad, stats, do, dq, dkv, dkv, qs, ks, ks, qs, 0, 0, D)
        return dq, dkv, None, None, None, None, None


class CrossInProjAttnFn(Function):
    """nn.MultiheadAttention of CrossAttentionBlock up to (not including) out_proj, with different query and key/value
    inputs (modules/module_seg_vit.py:215): q = xq w[:D]^T + b[:D], [k | v] = xk w[D:]^T + b[D:], o = CrossAttnFn core.
    One Function instead of two LinearFn on slices of in_proj_weight + CrossAttnFn: the weight gradient is ONE (3D, D)
    buffer written by both wgrads (autograd's slice backward cost 4 zero fills + 4 copies + 2 adds per layer), the
    bf16 weight comes from the parameter's shadow, and in bf16 mode the bias gradient is the attention backward's
    per-sample token sums (no column-sum pass over the (B*S, 2D) gradient)."""

    @staticmethod
    def forward(ctx, xq, xk, w, b, B, G, S, n_head, mode, act_dtype):
        D = w.shape[1]
        xq, xk = xq.reshape(B * G, D), xk.reshape(B * S, D)
        if xq.dtype != act_dtype:
            xq = p_cast(xq, act_dtype)
        if xk.dtype != act_dtype:
            xk = p_cast(xk, act_dtype)
        wc = wcast(w, act_dtype)
        bd = b.detach()
        qp = p_linear(xq, wc[:D], bd[:D])[0]
        kv = p_linear(xk, wc[D:], bd[D:])[0]
        o = torch.empty_like(qp)
        ad, _, _ = _cross_attn_desc(qp, kv, o, B, G, S, n_head, mode)
        stats = p_attn_fwd(ad, qp)
        ctx.save_for_backward(xq, xk, wc, qp, kv, o, stats)
        ctx.cfg = (B, G, S, n_head, mode)
        ctx.gslot = _slot_of(w)
        return o

    @staticmethod
    def backward(ctx, do):
        xq, xk, wc, qp, kv, o, stats = ctx.saved_tensors
        B, G, S, n_head, mode = ctx.cfg
        D = qp.shape[1]
        do = do.contiguous()
        ad, qs, ks = _cross_attn_desc(qp, kv, o, B, G, S, n_head, mode)
        dq = torch.empty_like(qp)
        dkv = torch.empty_like(kv)
        part = _empty((B, 3 * D), torch.float32, do) if qp.dtype == torch.bfloat16 else None
        p_attn_bwd(ad, stats, do, dq, dkv, dkv, qs, ks, ks, qs, 0, 0, D, colsum_part=part)
        dxq = p_dgrad(dq, wc[:D], xq.dtype)
        dxk = p_dgrad(dkv, wc[D:], xk.dtype)
        dw = _slot_out(ctx.gslot, (3 * D, D))
        if dw is None:
            dw = _empty((3 * D, D), torch.float32, do)
        p_wgrad(dq, xq, out=dw[:D])
        p_wgrad(dkv, xk, out=dw[D:])
        if part is not None:
            db = p_colsum(part)
        else:
            db = _empty((3 * D,), torch.float32, do)
            p_colsum(dq, out=db[:D])
            p_colsum(dkv, out=db[D:])
        return dxq.view(B, G, D), dxk.view(B, S, D), dw, db, None, None, None, None, None, None


class CrossBlockFn(Function):
    """One CrossAttentionBlock of the learnable-center stage (reference modules/module_seg_vit.py:199-218) as ONE autograd node:
        q1 = q + out_proj(MHA(ln_x q, ln_k kv, ln_k kv)),  kv = cat([q, tokens]);   q2 = q1 + c_proj(QuickGELU(c_fc(ln_2 q1)))
    q (B, G, D) fp32; kn_buf (B, S, D) in the compute dtype whose rows [G, S) of every sample already hold ln_k(tokens)
    (LayerNormMultiFn) - rows [0, G) are written here, in place (ln_k q).  The block is 8 center rows per sample: every
    kernel is a few microseconds, so the node count is the cost - as separate LinearFn / LayerNormFn nodes its backward was
    ~45 launches (a split-K combine, a bias column sum and its reduction per Linear, a reduction per LayerNorm, an add per
    residual branch); here the residual adds ride in the LayerNorm backwards, the bias gradients come out of them / the
    attention backward / the c_proj data gradient, and every trailing reduction joins ONE queue (2 launches).
    Returns (q2, kn_buf); the gradient of kn_buf covers all S rows (its consumer reads the token rows only)."""

    NPARAM = 14

    @staticmethod
    def forward(ctx, q, kn_buf, lnxw, lnxb, lnkw, lnkb, w_in, b_in, wo, bo, ln2w, ln2b, wfc, bfc, wpr, bpr,
                n_head, mode, eps, act_dtype):
        B, G, D = q.shape
        S = kn_buf.shape[1]
        M, F4 = B * G, wfc.shape[0]
        act = ACT_QUICK_GELU
        for w in (lnxw, lnxb, lnkw, lnkb, w_in, b_in, wo, bo, ln2w, ln2b, wfc, bfc, wpr, bpr):
            sl = _slot_of(w)
            if sl is not None:
                sl.note_forward_use()
        q2d = q.contiguous().view(M, D)
        kn2d = kn_buf.view(B * S, D)
        qn, mx, rx = p_ln_fwd(q2d, lnxw, lnxb, eps[0], act_dtype)
        _, mk, rk = p_ln_fwd(q2d, lnkw, lnkb, eps[1], act_dtype, out=kn2d, seg=(G, S, 0))
        ctx.mark_dirty(kn_buf)
        wc, wo_c, wfc_c, wpr_c = (wcast(w, act_dtype) for w in (w_in, wo, wfc, wpr))
        bd = b_in.detach()
        qp = p_linear(qn, wc[:D], bd[:D])[0]
        kv = p_linear(kn2d, wc[D:], bd[D:])[0]
        o = torch.empty_like(qp)
        ad, _, _ = _cross_attn_desc(qp, kv, o, B, G, S, n_head, mode)
        stats = p_attn_fwd(ad, qp)
        q1 = p_linear(o, wo_c, bo, residual=q2d, out_dtype=torch.float32)[0]
        z, m2, r2 = p_ln_fwd(q1, ln2w, ln2b, eps[2], act_dtype)
        h, u = p_linear(z, wfc_c, bfc, act=act, want_aux=True, aux_kind=_aux_kind(act_dtype, act, M, F4))
        q2 = p_linear(h, wpr_c, bpr, residual=q1, out_dtype=torch.float32)[0]
        # (kn_buf itself, not its 2-D view: a view made here of a tensor this node marks dirty may not be saved)
        ctx.save_for_backward(q2d, lnxw, mx, rx, qn, lnkw, mk, rk, kn_buf, wc, qp, kv, o, stats, wo_c, q1, ln2w, m2, r2, z, wfc_c, u, h,
                              wpr_c)
        ctx.cfg = (B, G, S, D, n_head, mode, act, act_dtype)
        ctx.gslots = tuple(_slot_of(w) for w in (w_in, wo, wfc, wpr))
        return q2.view(B, G, D), kn_buf

    @staticmethod
    def backward(ctx, dq2, _dbuf):
        (q2d, lnxw, mx, rx, qn, lnkw, mk, rk, kn_buf, wc, qp, kv, o, stats, wo_c, q1, ln2w, m2, r2, z, wfc_c, u, h,
         wpr_c) = ctx.saved_tensors
        B, G, S, D, n_head, mode, act, act_dtype = ctx.cfg
        kn2d = kn_buf.detach().view(B * S, D)
        M, F4 = B * G, wfc_c.shape[0]
        bf = act_dtype == torch.bfloat16
        s_in, s_o, s_fc, s_pr = ctx.gslots
        g = dq2.contiguous().view(M, D)
        if g.dtype != torch.float32:
            g = p_cast(g, torch.float32)
        g16 = p_cast(g, act_dtype) if bf else g
        rq = ReduceQueue()
        # the four weight gradients over the block's 8 center rows per sample (B*G rows: 9-36 output tiles each, 42 us apiece as
        # separate split-K launches) run as ONE grouped launch at the end of the node (round 6; bf16 mode)
        wg = WgradGroup() if bf else None

        def small_wgrad(dy_, x_, out_):
            if wg is not None and WgradGroup.covers(dy_, x_, out_):
                return wg.add(dy_, x_, out=out_)
            return p_wgrad(dy_, x_, out=out_, defer=rq)
        # ---- MLP
        du, dbfc = p_dgrad(g16, wpr_c, act_dtype, aux=u, act=act, want_colsum=True,
                           aux_kind=2 if u.dtype == torch.uint8 else _aux_kind(act_dtype, act), defer=rq)
        dwpr = small_wgrad(g16, h, _slot_out(s_pr, (D, F4)))
        dz = p_dgrad(du, wfc_c, act_dtype)
        dwfc = small_wgrad(du, z, _slot_out(s_fc, (F4, D)))
        r = p_ln_bwd(dz, q1, ln2w, m2, r2, dres=g, dx_dtype=torch.float32, want_bf16=bf, want_dres_colsum=True, defer=rq)
        dq1, dln2w, dln2b = r[0], r[1], r[2]
        dq1_16 = r[3] if bf else dq1
        dbpr = r[-1]                                             # colsum(g): the c_proj bias gradient
        # ---- attention
        do = p_dgrad(dq1_16, wo_c, act_dtype)
        dwo = small_wgrad(dq1_16, o, _slot_out(s_o, (D, D)))
        ad, qs, ks = _cross_attn_desc(qp, kv, o, B, G, S, n_head, mode)
        dqp, dkv = torch.empty_like(qp), torch.empty_like(kv)
        part = _empty((B, 3 * D), torch.float32, do) if bf else None
        p_attn_bwd(ad, stats, do, dqp, dkv, dkv, qs, ks, ks, qs, 0, 0, D, colsum_part=part)
        dqn = p_dgrad(dqp, wc[:D], act_dtype)
        dkn = p_dgrad(dkv, wc[D:], act_dtype)
        dw_in = _slot_out(s_in, (3 * D, D))
        if dw_in is None:
            dw_in = _empty((3 * D, D), torch.float32, do)
        small_wgrad(dqp, qn, dw_in[:D])
        p_wgrad(dkv, kn2d, out=dw_in[D:], defer=rq)
        db_in = _empty((3 * D,), torch.float32, do)
        if part is not None:
            rq.add_rows(part, B, 3 * D, 3 * D, (db_in,), 3 * D)
        else:
            p_colsum(dqp, out=db_in[:D])
            p_colsum(dkv, out=db_in[D:])
        # ---- the two LayerNorms of q: ln_x (dres = dq1: the residual branch; its column sums = the out_proj bias gradient),
        # then ln_k's center rows (dres = what the first one produced)
        r = p_ln_bwd(dqn, q2d, lnxw, mx, rx, dres=dq1, dx_dtype=torch.float32, want_dres_colsum=True, defer=rq)
        dq_a, dlnxw, dlnxb, dbo = r[0], r[1], r[2], r[-1]
        r = p_ln_bwd(dkn, q2d, lnkw, mk, rk, dres=dq_a, dx_dtype=torch.float32, defer=rq, seg=(G, S, 0))
        dq, dlnkw, dlnkb = r[0], r[1], r[2]
        if wg is not None:
            wg.flush()
        rq.flush()
        return (dq.view(B, G, D), dkn.view(B, S, D), dlnxw, dlnxb, dlnkw, dlnkb, dw_in, db_in, dwo, dbo, dln2w, dln2b, dwfc, dbfc,
                dwpr, dbpr, None, None, None, None)


class PatchEmbedFn(Function):
    """conv1 (16x16/16, no bias) as im2col + GEMM with the positional table fused as the epilogue
    residual (modules/module_clip_vtransformer.py:56-64).  The CLS row the reference prepends is
    discarded by SegViT before any use (modules/module_seg_vit.py:419), so it is never materialised;
    class_embedding therefore receives an all-zero gradient, exactly as in the reference.
    bf16 mode pads the contraction dimension 3*p*p to a multiple of 64 with zero columns (ViT-L/14: 588 -> 640) so
    that the patch GEMM runs on the LDS-DMA kernels."""

    @staticmethod
    def forward(ctx, image, conv_w, cls, pos, patch, act_dtype):
        lib = L.load()
        B, Cc, H, W = image.shape
        D = conv_w.shape[0]
        T = (H // patch) * (W // patch)
        Kd = Cc * patch * patch
        Kp = Kd if (act_dtype != torch.bfloat16 or Kd % 64 == 0) else -(-Kd // 64) * 64
        image = image.contiguous()
        cols = _empty((B * T, Kp), act_dtype, image)
        L.check(lib.segclip_im2col_ld(L.ptr(image), L.ptr(cols), B, Cc, H, W, patch, 0, L.dt(cols), Kp, L.stream()), "im2col")
        if Kp == Kd:
            wc = wcast(conv_w.reshape(D, Kd), act_dtype)
        else:
            wc = torch.zeros((D, Kp), dtype=act_dtype, device=image.device)
            wc[:, :Kd] = p_cast(conv_w.detach().reshape(D, Kd).contiguous(), act_dtype)
        x = _empty((B, T, D), torch.float32, image)
        posc = pos.detach().contiguous()
        done = False
        if act_dtype == torch.bfloat16 and (B * T) % 128 == 0 and D % 256 == 0:
            # one (B*T, D) GEMM whose epilogue adds positional row (m % T) - the batched form below runs B problems of T = 196
            # rows on 256-row tiles (289 us against 105 us at B = 256)
            try:
                p_gemm(cols, wc, x, B * T, D, Kp, (Kp, 1), (Kp, 1), D, residual=posc, ldr=D, r_off=D, r_mod=T)
                done = True
            except L.Unsupported:
                pass
        if not done:
            p_gemm(cols, wc, x, T, D, Kp, (Kp, 1), (Kp, 1), D, residual=posc, ldr=D, r_off=D, nb1=B, bsA=(T * Kp, 0),
                   bsC=(T * D, 0), bsR=(0, 0))
        ctx.save_for_backward(cols)
        ctx.shape = (B, T, D, Kd, Kp, tuple(conv_w.shape), tuple(cls.shape), tuple(pos.shape))
        return x

    @staticmethod
    def backward(ctx, dx):
        (cols,) = ctx.saved_tensors
        B, T, D, Kd, Kp, wshape, cshape, pshape = ctx.shape
        dx = dx.contiguous()
        dw = dcls = dpos = None
        if ctx.needs_input_grad[1]:
            dw = p_wgrad(dx.view(B * T, D), cols)
            dw = (dw if Kp == Kd else dw[:, :Kd].contiguous()).view(wshape)
        if ctx.needs_input_grad[2]:
            dcls = torch.zeros(cshape, dtype=torch.float32, device=dx.device)
        if ctx.needs_input_grad[3]:
            dpos = torch.zeros(pshape, dtype=torch.float32, device=dx.device)
            dpos[1:] = p_colsum(dx.view(B, T * D)).view(T, D)
        return None, dw, dcls, dpos, None, None


class EmbedFn(Function):
    """token_embedding(ids) + positional_embedding[:L]  (modules/module_clip.py:109-112)."""

    @staticmethod
    def forward(ctx, ids, table, pos):
        B, Lq = ids.shape
        V, D = table.shape
        ids = ids.contiguous()
        out = _empty((B, Lq, D), torch.float32, table)
        posc = pos.detach().contiguous()
        L.check(L.load().segclip_embed_fwd(L.ptr(ids), L.ptr(table), L.ptr(posc), L.ptr(out), B, Lq, D, V, L.stream()),
                "embed_fwd")
        ctx.save_for_backward(ids)
        ctx.shape = (B, Lq, D, V, tuple(pos.shape))
        ctx.gslot = _slot_of(table)
        return out

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        B, Lq, D, V, pshape = ctx.shape
        dout = dout.contiguous()
        dtable = None
        if ctx.needs_input_grad[1]:
            dtable = _slot_out(ctx.gslot, (V, D))
            dtable = dtable.zero_() if dtable is not None else torch.zeros((V, D), dtype=torch.float32, device=dout.device)
        dpos_l = _empty((Lq, D), torch.float32, dout) if ctx.needs_input_grad[2] else None
        L.check(L.load().segclip_embed_bwd(L.ptr(ids), L.ptr(dout), L.ptr(dtable), L.ptr(dpos_l), B, Lq, D, V,
                                           L.stream()), "embed_bwd")
        dpos = None
        if dpos_l is not None:
            dpos = torch.zeros(pshape, dtype=torch.float32, device=dout.device)
            dpos[:Lq] = dpos_l
        return None, dtable, dpos


class ReconMixFn(Function):
    """out (B,M,D) = a (B,M,8) @ x (B,8,D) in fp32 (reference modules/module_seg_vit.py:342: the token rows of the MAE branch rebuilt
    from the 8 centers) as one pass over the output; backward da = dout x^T, dx = a^T dout in one kernel."""

    @staticmethod
    def forward(ctx, a, x):
        B, M, G = a.shape
        D = x.shape[2]
        a, x = a.contiguous(), x.contiguous()
        out = _empty((B, M, D), torch.float32, a)
        L.check(L.load().segclip_recon_mix_fwd(L.ptr(a), L.ptr(x), L.ptr(out), B, M, G, D, L.stream()), "recon_mix_fwd")
        ctx.save_for_backward(a, x)
        return out

    @staticmethod
    def backward(ctx, dout):
        a, x = ctx.saved_tensors
        B, M, G = a.shape
        D = x.shape[2]
        dout = dout.contiguous()
        da = _empty((B, M, G), torch.float32, a)
        dx = _empty((B, G, D), torch.float32, a)
        L.check(L.load().segclip_recon_mix_bwd(L.ptr(a), L.ptr(x), L.ptr(dout), L.ptr(da), L.ptr(dx), B, M, G, D, L.stream()),
                "recon_mix_bwd")
        return da, dx


# config.pad_rows applies from this many token rows on: below it a step is bound by the host's launch rate (per-GPU batch 64:
# 13.5 ms of enqueue per step), where the ~50 extra small launches of a padded tower cost more than the faster kernels return
_PAD_ROWS_MIN = 6144


def recon_mix(a, x):
    """a (B,M,G) @ x (B,G,D) -> (B,M,D), fp32: the dedicated kernel for G = 8, the batched GEMM otherwise."""
    if (a.dtype == torch.float32 and x.dtype == torch.float32 and a.dim() == 3 and x.dim() == 3 and a.shape[2] == 8
            and x.shape[1] == 8 and x.shape[2] % 4 == 0 and 4 <= x.shape[2] <= 4096):
        return ReconMixFn.apply(a, x)
    return bmm(a, x, transB=False, out_dtype=torch.float32)


class MeanCatFn(Function):
    """cat([mean(x, dim=1, keepdim=True), x], dim=1) for x (B,T,D) fp32 (reference modules/modeling.py:240-242 and the MAE branch
    of modules/module_seg_vit.py: the mean over the tokens stands in for the CLS row): one kernel each way."""

    @staticmethod
    def forward(ctx, x):
        B, T, D = x.shape
        x = x.contiguous()
        out = _empty((B, T + 1, D), torch.float32, x)
        L.check(L.load().segclip_mean_cat_fwd(L.ptr(x), L.ptr(out), B, T, D, L.stream()), "mean_cat_fwd")
        ctx.shape = (B, T, D)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, T, D = ctx.shape
        dout = dout.contiguous()
        dx = _empty((B, T, D), torch.float32, dout)
        L.check(L.load().segclip_mean_cat_bwd(L.ptr(dout), L.ptr(dx), B, T, D, L.stream()), "mean_cat_bwd")
        return dx


def mean_cat(x):
    """x (B,T,D) -> (B,T+1,D) with the token mean as row 0; fp32 rows of a multiple of 4 columns on the HIP kernel."""
    if x.dtype == torch.float32 and x.dim() == 3 and x.shape[-1] % 4 == 0 and x.shape[1] > 0:
        return MeanCatFn.apply(x)
    return torch.cat([torch.mean(x, dim=1, keepdim=True), x], dim=1)


class MaeUnshuffleFn(Function):
    """Decoder input of the MAE heads (reference modules/module_mae.py:310-314 / 338-342):
    gather(cat([x, mask_token.expand(B, L - K, D)], 1), ids_restore) + pos_embed, without the concatenated tensor:
    out[b][j] = (ids[b][j] < K ? x[b][ids[b][j]] : mask_token) + pos[j].  x (B,K,D) fp32, mask_token (D) or (1,1,D), ids (B,L)
    int64 (a permutation of 0..L-1 per sample), pos (L,D) or (1,L,D)."""

    @staticmethod
    def forward(ctx, x, mask_token, ids, pos):
        B, K, D = x.shape
        Lq = ids.shape[1]
        x, ids = x.contiguous(), ids.contiguous()
        mt, pe = mask_token.detach().reshape(D).float().contiguous(), pos.detach().reshape(Lq, D).float().contiguous()
        out = _empty((B, Lq, D), torch.float32, x)
        L.check(L.load().segclip_mae_unshuffle_fwd(L.ptr(x), L.ptr(mt), L.ptr(ids), L.ptr(pe), L.ptr(out), B, K, Lq, D, L.stream()),
                "mae_unshuffle_fwd")
        ctx.save_for_backward(ids)
        ctx.dims = (B, K, Lq, D, mask_token.shape, pos.shape, mask_token.dtype, pos.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        B, K, Lq, D, mshape, pshape, mdt, pdt = ctx.dims
        dout = dout.contiguous()
        dx = _empty((B, K, D), torch.float32, dout)
        dpos = _empty((Lq, D), torch.float32, dout)
        mpart = _empty((Lq, D), torch.float32, dout)
        L.check(L.load().segclip_mae_unshuffle_bwd(L.ptr(dout), L.ptr(ids), L.ptr(dx), L.ptr(dpos), L.ptr(mpart), B, K, Lq, D, L.stream()),
                "mae_unshuffle_bwd")
        dmask = p_colsum(mpart) if ctx.needs_input_grad[1] else None
        return (dx, dmask.reshape(mshape).to(mdt) if dmask is not None else None, None,
                dpos.reshape(pshape).to(pdt) if ctx.needs_input_grad[3] else None)


class GatherRowsFn(Function):
    """out[b,j,:] = src[b, idx[b,j], :] with unique idx per b (EOT pick, MAE keep / un-shuffle)."""

    @staticmethod
    def forward(ctx, src, idx):
        B, Ts, D = src.shape
        To = idx.shape[1]
        src = src.contiguous()
        idx = idx.contiguous()
        out = _empty((B, To, D), src.dtype, src)
        L.check(L.load().segclip_gather_rows(L.ptr(src), L.ptr(idx), L.ptr(out), B, Ts, To, D, L.dt(src), L.stream()),
                "gather_rows")
        ctx.save_for_backward(idx)
        ctx.shape = (B, Ts, To, D)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        B, Ts, To, D = ctx.shape
        dout = dout.contiguous()
        dsrc = torch.zeros((B, Ts, D), dtype=dout.dtype, device=dout.device)
        L.check(L.load().segclip_scatter_rows(L.ptr(dout), L.ptr(idx), L.ptr(dsrc), B, Ts, To, D, L.dt(dout),
                                              L.stream()), "scatter_rows")
        return dsrc, None


class AssignFn(Function):
    """gumbel_softmax(hard=True, dim=centers) + soft assignment (modules/module_seg_vit.py:221-242,305-306).
    logits (B,G,T) fp32, gumbel (B,G,T) fp32 or None (eval).  Returns hard (straight-through gradient),
    soft (no grad, like the reference's use), idx uint8 (B,T)."""

    @staticmethod
    def forward(ctx, logits, gumbel, tau):
        B, G, T = logits.shape
        logits = logits.contiguous()
        g = gumbel.contiguous() if gumbel is not None else None
        y = torch.empty_like(logits)
        soft = torch.empty_like(logits)
        hard = torch.empty_like(logits)
        idx = torch.empty((B, T), dtype=torch.uint8, device=logits.device)
        counts = torch.empty((B, G), dtype=torch.float32, device=logits.device)
        L.check(L.load().segclip_assign_fwd(L.ptr(logits), L.ptr(g), tau if g is not None else 1.0, L.ptr(y),
                                            L.ptr(soft), L.ptr(idx), L.ptr(hard), L.ptr(counts), B, G, T, L.stream()),
                "assign_fwd")
        ctx.save_for_backward(y)
        ctx.tau = tau if g is not None else 1.0
        ctx.mark_non_differentiable(soft, idx, counts)
        return hard, soft, idx, counts

    @staticmethod
    def backward(ctx, dhard, _dsoft, _didx, _dcounts):
        (y,) = ctx.saved_tensors
        B, G, T = y.shape
        dhard = dhard.contiguous()
        dl = torch.empty_like(y)
        L.check(L.load().segclip_assign_bwd(L.ptr(dhard), L.ptr(y), ctx.tau, L.ptr(dl), B, G, T, L.stream()),
                "assign_bwd")
        return dl, None, None


class L2NormFn(Function):
    """x / ||x||  (modules/modeling.py:341-345)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        rows, cols = x.shape
        y = torch.empty_like(x)
        n = _empty((rows,), torch.float32, x)
        L.check(L.load().segclip_l2norm_fwd(L.ptr(x), L.ptr(y), L.ptr(n), rows, cols, L.stream()), "l2norm_fwd")
        ctx.save_for_backward(y, n)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, n = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(y)
        L.check(L.load().segclip_l2norm_bwd(L.ptr(dy), L.ptr(y), L.ptr(n), L.ptr(dx), y.shape[0], y.shape[1],
                                            L.stream()), "l2norm_bwd")
        return dx


class CrossEntropyFn(Function):
    """mean_i -log softmax(logits_i)[i + label_offset]  (nn.CrossEntropyLoss, modules/modeling.py:205-208)."""

    @staticmethod
    def forward(ctx, logits, label_offset):
        logits = logits.contiguous()
        rows, cols = logits.shape
        lib = L.load()
        lse = _empty((rows,), torch.float32, logits)
        lr = _empty((rows,), torch.float32, logits)
        L.check(lib.segclip_ce_fwd(L.ptr(logits), L.ptr(lse), L.ptr(lr), rows, cols, label_offset, L.stream()), "ce_fwd")
        loss = _empty((), torch.float32, logits)
        L.check(lib.segclip_reduce_sum(L.ptr(lr), L.ptr(loss), rows, 1.0 / rows, L.stream()), "reduce_sum")
        ctx.save_for_backward(logits, lse)
        ctx.label_offset = label_offset
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, lse = ctx.saved_tensors
        rows, cols = logits.shape
        g = g.contiguous().float()
        dl = torch.empty_like(logits)
        L.check(L.load().segclip_ce_bwd(L.ptr(logits), L.ptr(lse), L.ptr(g), 1.0, L.ptr(dl), rows, cols,
                                        ctx.label_offset, L.stream()), "ce_bwd")
        return dl, None


class CrossEntropyLabelsFn(Function):
    """nn.CrossEntropyLoss(ignore_index) with explicit labels: mean over the rows whose label is not ignored
    (text-MAE vocabulary loss, modules/module_mae.py:351-353).  logits (R, V) fp32, labels (R,) int64."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        logits = logits.contiguous()
        labels = labels.to(torch.int64).contiguous()
        L.require_cuda(logits, labels)
        rows, cols = logits.shape
        lib = L.load()
        lse, lr, valid = (_empty((rows,), torch.float32, logits) for _ in range(3))
        L.check(lib.segclip_ce_labels_fwd(L.ptr(logits), L.ptr(labels), int(ignore_index), L.ptr(lse), L.ptr(lr), L.ptr(valid),
                                          rows, cols, L.stream()), "ce_labels_fwd")
        tot, cnt, loss = (_empty((), torch.float32, logits) for _ in range(3))
        L.check(lib.segclip_reduce_sum(L.ptr(lr), L.ptr(tot), rows, 1.0, L.stream()), "reduce_sum")
        L.check(lib.segclip_reduce_sum(L.ptr(valid), L.ptr(cnt), rows, 1.0, L.stream()), "reduce_sum")
        inv = torch.reciprocal(cnt)
        L.check(lib.segclip_scale(L.ptr(tot), L.ptr(inv), L.ptr(loss), 1, L.stream()), "scale")
        ctx.save_for_backward(logits, lse, labels, inv)
        ctx.ignore_index = int(ignore_index)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, lse, labels, inv = ctx.saved_tensors
        rows, cols = logits.shape
        g = g.contiguous().float()
        dl = torch.empty_like(logits)
        L.check(L.load().segclip_ce_labels_bwd(L.ptr(logits), L.ptr(lse), L.ptr(labels), ctx.ignore_index, L.ptr(g),
                                               L.ptr(inv), L.ptr(dl), rows, cols, L.stream()), "ce_labels_bwd")
        return dl, None, None


def prefix_mask_lengths(attention_mask):
    """(B, L) 0/1 attention mask of END-PADDED captions (the dataloader contract, dataloaders/dataloader_cc_retrieval.py:
    valid tokens first) -> int32 (B,) number of valid keys, the form the attention kernels take the key-padding mask in.
    The prefix form (no interior zeros, no left padding, at least one valid key per row - a row without keys has
    lse = -inf) is checked ON EVERY CALL without a host synchronisation: the verdict is computed on the device and
    handed to torch._assert_async, which fails the stream (the error surfaces at the next synchronisation) instead of
    silently attending to the wrong keys.  SEGCLIP_CHECK_MASKS=1 additionally raises at the call site (one host sync)."""
    m = attention_mask.reshape(attention_mask.shape[0], -1)
    mi = m.to(torch.int32)
    ok = (mi[:, 1:] <= mi[:, :-1]).all() & (mi[:, 0] >= 1).all() & ((mi == 0) | (mi == 1)).all()
    if _CHECK_MASKS or not mi.is_cuda:
        if not bool(ok.item()):
            raise NotImplementedError("attention_mask must be a 0/1 PREFIX mask with >= 1 valid token per row "
                                      "(end-padded captions); interior zeros / left padding are not supported")
    else:
        torch._assert_async(ok, "segclip: attention_mask is not a 0/1 prefix mask (interior zeros / left padding / empty row)")
    return mi.sum(dim=1, dtype=torch.int32).contiguous()


_CHECK_MASKS = bool(int(__import__("os").environ.get("SEGCLIP_CHECK_MASKS", "0")))


class SuperpixelKLFn(Function):
    """Symmetric KL between the hard assignment and its superpixel mean (modules/modeling.py:212-224)."""

    @staticmethod
    def forward(ctx, hard, seg):
        B, G, T = hard.shape
        hard = hard.contiguous()
        L.require_cuda(hard, seg)
        if seg.is_floating_point() or seg.dtype == torch.bool:
            raise TypeError(f"superpixel_kl: image_seg must hold integer superpixel labels, got {seg.dtype}")
        seg = seg.to(torch.int64).contiguous().view(B, T)   # the kernel reads int64; loaders may hand over int32 / uint8
        lib = L.load()
        lr = _empty((B,), torch.float32, hard)
        dh = torch.empty_like(hard)
        L.check(lib.segclip_superpixel_kl(L.ptr(hard), L.ptr(seg), L.ptr(lr), L.ptr(dh), B, G, T, L.stream()),
                "superpixel_kl")
        loss = _empty((), torch.float32, hard)
        L.check(lib.segclip_reduce_sum(L.ptr(lr), L.ptr(loss), B, 1.0, L.stream()), "reduce_sum")
        ctx.save_for_backward(dh)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dh,) = ctx.saved_tensors
        g = g.contiguous().float()
        out = torch.empty_like(dh)
        L.check(L.load().segclip_scale(L.ptr(dh), L.ptr(g), L.ptr(out), dh.numel(), L.stream()), "scale")
        return out, None


class MaskedMSEFn(Function):
    """MAE reconstruction loss (modules/module_mae.py:322-328): pred (B,1+T,Dp) [row 0 = CLS, dropped],
    target (B,T,Dp) fp32 (patchify), mask (B,1+T) fp32."""

    @staticmethod
    def forward(ctx, pred, target, mask):
        B, T1, Dp = pred.shape
        T = T1 - 1
        pred = pred.contiguous()
        lib = L.load()
        lr = _empty((B * T,), torch.float32, pred)
        L.check(lib.segclip_masked_mse_fwd(L.ptr(pred), L.ptr(target), L.ptr(mask), L.ptr(lr), B, T, Dp, L.dt(pred),
                                           L.stream()), "masked_mse_fwd")
        msum = _empty((), torch.float32, pred)
        mflat = mask[:, 1:].contiguous()
        L.check(lib.segclip_reduce_sum(L.ptr(mflat), L.ptr(msum), B * T, 1.0, L.stream()), "reduce_sum")
        tot = _empty((), torch.float32, pred)
        L.check(lib.segclip_reduce_sum(L.ptr(lr), L.ptr(tot), B * T, 1.0, L.stream()), "reduce_sum")
        loss = _empty((), torch.float32, pred)
        # loss = tot / msum  (single-element division, done by the scale kernel with 1/msum)
        inv = torch.reciprocal(msum)
        L.check(lib.segclip_scale(L.ptr(tot), L.ptr(inv), L.ptr(loss), 1, L.stream()), "scale")
        ctx.save_for_backward(pred, target, mask, msum)
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, target, mask, msum = ctx.saved_tensors
        B, T1, Dp = pred.shape
        g = g.contiguous().float()
        dp = torch.empty_like(pred)
        L.check(L.load().segclip_masked_mse_bwd(L.ptr(pred), L.ptr(target), L.ptr(mask), L.ptr(g), L.ptr(msum), 1.0,
                                                L.ptr(dp), B, T1 - 1, Dp, L.dt(pred), L.stream()), "masked_mse_bwd")
        return dp, None, None


def patchify_target(image, patch):
    """MAE target `patchify(imgs)` (modules/module_mae.py:18-29): (B,3,H,W) -> (B, T, p*p*3), fp32."""
    B, Cc, H, W = image.shape
    T = (H // patch) * (W // patch)
    image = image.contiguous()
    out = _empty((B, T, Cc * patch * patch), torch.float32, image)
    L.check(L.load().segclip_im2col(L.ptr(image), L.ptr(out), B, Cc, H, W, patch, 1, L.F32, L.stream()), "im2col")
    return out


def mask_sort(noise, len_keep):
    """MAE random masking indices (modules/module_clip_util.py:91-124, keep_cls=True).
    Returns ids_shuffle, ids_restore (int64) and mask (fp32), bit-exact functions of `noise`."""
    B, Lq = noise.shape
    noise = noise.contiguous().float()
    ids_shuffle = torch.empty((B, Lq), dtype=torch.int64, device=noise.device)
    ids_restore = torch.empty((B, Lq), dtype=torch.int64, device=noise.device)
    mask = torch.empty((B, Lq), dtype=torch.float32, device=noise.device)
    L.check(L.load().segclip_mask_sort(L.ptr(noise), L.ptr(ids_shuffle), L.ptr(ids_restore), L.ptr(mask), B, Lq,
                                       len_keep, L.stream()), "mask_sort")
    return ids_shuffle, ids_restore, mask


class _on_comm_stream:
    """The embedding exchange runs on the communication stream (the one GradSync's bucket all-reduces use), ordered
    against the compute stream by events on both sides instead of being enqueued in-line on it: RCCL's launch-side
    bookkeeping then never sits between two compute kernels, and the collective keeps its own hardware queue."""

    def __init__(self, t):
        self.t = t

    def __enter__(self):
        if not self.t.is_cuda:      # CPU tensors (gloo tests): nothing to order
            self.ctx = None
            return
        from . import streams
        self.main = torch.cuda.current_stream(self.t.device)
        self.comm = streams.side_stream("comm", self.main)
        self.comm.wait_stream(self.main)
        self.ctx = torch.cuda.stream(self.comm)
        self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is None:
            return False
        self.ctx.__exit__(*exc)
        self.main.wait_stream(self.comm)   # the consumer (logits GEMM) follows at once: no allocator hand-over needed
        return False


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 0


def _gather_raw(x, world):
    """rank-ordered all-gather of (B, ...) -> (B * world, ...), no autograd.  world 0 (no process group): identity."""
    if world == 0:
        return x
    x = x.contiguous()
    if x.is_cuda and dist.get_backend() != "nccl":
        # gloo has no device all-gather (only broadcast / all-reduce take GPU tensors): the single-GPU
        # multi-process tests gather by summing rank-disjoint slices, which is exact
        out = torch.zeros((world * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        r = dist.get_rank()
        out[r * x.shape[0]:(r + 1) * x.shape[0]] = x
        dist.all_reduce(out, op=dist.ReduceOp.SUM)
        return out
    out = torch.empty((world * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    with _on_comm_stream(x):
        dist.all_gather_into_tensor(out, x)
    return out


def _scatter_sum_raw(g, world):
    """the adjoint: reduce-scatter(SUM) of (B * world, ...) -> this rank's (B, ...), no autograd"""
    if world == 0:
        return g
    g = g.contiguous()
    n = g.shape[0] // world
    if dist.get_backend() == "nccl":
        out = torch.empty((n,) + tuple(g.shape[1:]), dtype=g.dtype, device=g.device)
        with _on_comm_stream(g):
            dist.reduce_scatter_tensor(out, g, op=dist.ReduceOp.SUM)
        return out
    g = g.clone()
    dist.all_reduce(g, op=dist.ReduceOp.SUM)
    r = dist.get_rank()
    return g[r * n:(r + 1) * n].contiguous()


class AllGatherFn(Function):
    """Differentiable rank-ordered all-gather of (B, ...) embeddings (dist_collect,
    modules/util_module.py:180-190; diffdist semantics: all_gather forward, reduce-scatter(SUM)
    backward).  On RCCL ("nccl" backend) both directions are ONE fused collective; the gloo branch
    (CPU tests) uses all_reduce + own slice, which is the same arithmetic.  World size 1 = identity."""

    @staticmethod
    def forward(ctx, x):
        ctx.world = _world()
        return _gather_raw(x, ctx.world)

    @staticmethod
    def backward(ctx, g):
        return _scatter_sum_raw(g, ctx.world)


def all_gather_embeddings(x):
    return AllGatherFn.apply(x)


class MaxTokensFn(Function):
    """cls = max over the patch tokens (modules/module_seg_vit.py:441): x (B, T, D) fp32 -> (B, D).  The backward writes the
    routed gradient as fp32 AND (bf16 mode) as the bf16 copy the residual stack's backward takes as its operand, in one pass
    (torch: zero-fill + scatter, then a cast)."""

    @staticmethod
    def forward(ctx, x, want_bf16):
        x = x.contiguous()
        B, T, D = x.shape
        L.require_cuda(x)
        out = _empty((B, D), torch.float32, x)
        idx = torch.empty((B, D), dtype=torch.int32, device=x.device)
        L.check(L.load().segclip_max_tokens_fwd(L.ptr(x), L.ptr(out), L.ptr(idx), B, T, D, L.stream()), "max_tokens_fwd")
        ctx.save_for_backward(idx)
        ctx.shape, ctx.want_bf16 = (B, T, D), bool(want_bf16)
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        B, T, D = ctx.shape
        g = g.contiguous().float()
        dx = _empty((B, T, D), torch.float32, g)
        dx16 = _empty((B, T, D), torch.bfloat16, g) if ctx.want_bf16 else None
        L.check(L.load().segclip_max_tokens_bwd(L.ptr(g), L.ptr(idx), L.ptr(dx), L.ptr(dx16), B, T, D, L.stream()), "max_tokens_bwd")
        if dx16 is not None:
            dx._segclip_bf16 = dx16
        return dx, None


class ClipLossFn(Function):
    """The contrastive head of the training step as ONE autograd node (modules/modeling.py:338-362 + :204-209):
    L2-normalise both feature matrices, all-gather them in one stacked message, the two logits matrices
    clamp(exp(logit_scale), 100) * (t v_all^T), (v t_all^T) in exact fp32, both cross entropies and their mean - forward in
    4 launches (+ the collective), backward in 5.  Returns the loss; the raw cosine matrices are kept on the context object
    handed back through `box` (for model.last_logits)."""

    @staticmethod
    def forward(ctx, v_feat, t_feat, logit_scale, rank, box):
        lib = L.load()
        v_feat, t_feat = v_feat.contiguous().float(), t_feat.contiguous().float()
        L.require_cuda(v_feat, t_feat, logit_scale)
        B, C = v_feat.shape
        world = _world()
        both = _empty((B, 2, C), torch.float32, v_feat)
        norms = _empty((2 * B,), torch.float32, v_feat)
        L.check(lib.segclip_l2norm_pair_fwd(L.ptr(v_feat), L.ptr(t_feat), L.ptr(both), L.ptr(norms), B, C, L.stream()), "l2norm_pair_fwd")
        allb = _gather_raw(both, world)                       # (N, 2, C): [:, 0] = visual, [:, 1] = text of every rank
        N = allb.shape[0]
        off = B * int(rank)
        if off + B > N:
            raise ValueError(f"contrastive loss: rank {rank} with per-rank batch {B} does not fit the gathered batch {N}")
        cosm = _empty((2, B, N), torch.float32, v_feat)
        # [0] = t . v_all^T, [1] = v . t_all^T: one batched exact-fp32 launch (batch strides -C / +C swap the roles)
        p_gemm(both, allb, cosm, B, N, C, (2 * C, 1), (2 * C, 1), N, a_off=C, nb1=2, bsA=(-C, 0), bsB=(C, 0), bsC=(B * N, 0))
        ls = logit_scale.detach()
        lse, loss_rows = _empty((2 * B,), torch.float32, v_feat), _empty((2 * B,), torch.float32, v_feat)
        loss = _empty((), torch.float32, v_feat)
        L.check(lib.segclip_clip_ce_fwd(L.ptr(cosm), L.ptr(ls), L.ptr(lse), L.ptr(loss_rows), L.ptr(loss), B, N, off, L.stream()), "clip_ce_fwd")
        ctx.save_for_backward(both, allb, norms, cosm, lse, ls)
        ctx.cfg = (B, C, N, off, world, tuple(logit_scale.shape))
        if box is not None:
            box["cos"], box["logit_scale"] = cosm, ls
        return loss

    @staticmethod
    def backward(ctx, g):
        both, allb, norms, cosm, lse, ls = ctx.saved_tensors
        B, C, N, off, world, ls_shape = ctx.cfg
        lib = L.load()
        g = g.contiguous().float()
        dcos = torch.empty_like(cosm)
        ds_rows = _empty((2 * B,), torch.float32, cosm)
        dls = _empty(ls_shape, torch.float32, cosm) if ctx.needs_input_grad[2] else None
        L.check(lib.segclip_clip_ce_bwd(L.ptr(cosm), L.ptr(lse), L.ptr(ls), L.ptr(g), L.ptr(dcos), L.ptr(ds_rows), L.ptr(dls), B, N, off,
                                        L.stream()), "clip_ce_bwd")
        # this rank's rows as the LEFT factors: d t_n = dcos[0] v_all, d v_n = dcos[1] t_all  -> dboth[:, 1], dboth[:, 0]
        dboth = _empty((B, 2, C), torch.float32, cosm)
        p_gemm(dcos, allb, dboth, B, C, N, (N, 1), (1, 2 * C), 2 * C, c_off=C, nb1=2, bsA=(B * N, 0), bsB=(C, 0), bsC=(-C, 0))
        # every rank's rows as the RIGHT factors: d v_all = dcos[0]^T t_n, d t_all = dcos[1]^T v_n -> dall[:, 0], dall[:, 1]
        dall = _empty((N, 2, C), torch.float32, cosm)
        single = world <= 1          # N == B: the two contributions meet in the GEMM epilogue (residual = dboth)
        p_gemm(dcos, both, dall, N, C, B, (1, N), (1, 2 * C), 2 * C, b_off=C, nb1=2, bsA=(B * N, 0), bsB=(-C, 0), bsC=(C, 0),
               residual=dboth if single else None, ldr=2 * C if single else 0, bsR=(C, 0))
        dv, dt = _empty((B, C), torch.float32, cosm), _empty((B, C), torch.float32, cosm)
        if single:
            L.check(lib.segclip_l2norm_pair_bwd(L.ptr(dall), None, L.ptr(both), L.ptr(norms), L.ptr(dv), L.ptr(dt), B, C, L.stream()),
                    "l2norm_pair_bwd")
        else:
            dloc = _scatter_sum_raw(dall, world)              # reduce-scatter(SUM): diffdist's adjoint of the all-gather
            L.check(lib.segclip_l2norm_pair_bwd(L.ptr(dboth), L.ptr(dloc), L.ptr(both), L.ptr(norms), L.ptr(dv), L.ptr(dt), B, C,
                                                L.stream()), "l2norm_pair_bwd")
        return dv, dt, dls, None, None


class SegMeanFn(Function):
    """outputs = (hard @ v) / clamp_min(hard.sum(-1), 1)  (modules/module_seg_vit.py:308-309) for the one-hot hard assignment
    of AssignFn: a segment mean by center index in one launch, and its backward (dv, and dhard through numerator and
    normaliser) in one launch.  hard (B,G,T) fp32 carries the straight-through gradient; idx (B,T) uint8 and counts (B,G) are
    AssignFn's; v (B,T,D) fp32 or bf16.  -> (B,G,D) fp32."""

    @staticmethod
    def forward(ctx, hard, idx, counts, v):
        B, G, T = hard.shape
        D = v.shape[2]
        v = v.contiguous()
        L.require_cuda(hard, idx, counts, v)
        out = _empty((B, G, D), torch.float32, v)
        L.check(L.load().segclip_segmean_fwd(L.ptr(idx), L.ptr(v), L.dt(v), L.ptr(counts), L.ptr(out), B, G, T, D, L.stream()), "segmean_fwd")
        ctx.save_for_backward(idx, counts, v, out)
        ctx.shape = (B, G, T, D)
        return out

    @staticmethod
    def backward(ctx, dout):
        idx, counts, v, out = ctx.saved_tensors
        B, G, T, D = ctx.shape
        dout = dout.contiguous().float()
        dv = torch.empty_like(v)
        dhard = _empty((B, G, T), torch.float32, v)
        L.check(L.load().segclip_segmean_bwd(L.ptr(dout), L.ptr(out), L.ptr(idx), L.ptr(v), L.dt(v), L.ptr(counts), L.ptr(dv), L.ptr(dhard),
                                             B, G, T, D, L.stream()), "segmean_bwd")
        return dhard, None, None, dv


class CenterLogitsFn(Function):
    """Assignment logits of the learnable-center stage, attn = q k^T un-scaled (modules/module_seg_vit.py:304): q (B,G,D), k (B,T,D),
    both fp32 -> (B,G,T) fp32, and dq = dattn k, dk = dattn^T q, as per-sample token loops (csrc/center.hip) instead of batched
    M = 8 products on 32-row MFMA tiles (3 launches of 110-140 us).  The summation order over D is not the exact-fp32 GEMM's:
    the module uses this in bf16 mode only (the exact-f32 mode keeps the GEMM, whose argmax the parity tests pin)."""

    @staticmethod
    def forward(ctx, q, k):
        q, k = q.contiguous().float(), k.contiguous().float()
        B, G, D = q.shape
        T = k.shape[1]
        L.require_cuda(q, k)
        attn = _empty((B, G, T), torch.float32, q)
        L.check(L.load().segclip_center_logits_fwd(L.ptr(q), L.ptr(k), L.ptr(attn), B, G, T, D, L.stream()), "center_logits_fwd")
        ctx.save_for_backward(q, k)
        return attn

    @staticmethod
    def backward(ctx, dattn):
        q, k = ctx.saved_tensors
        B, G, D = q.shape
        T = k.shape[1]
        dattn = dattn.contiguous().float()
        dq, dk = torch.empty_like(q), torch.empty_like(k)
        L.check(L.load().segclip_center_logits_bwd(L.ptr(dattn), L.ptr(q), L.ptr(k), L.ptr(dq), L.ptr(dk), B, G, T, D, L.stream()),
                "center_logits_bwd")
        return dq, dk


def center_logits_covers(G, T, D, backward):
    """Whether the token-loop kernels of csrc/center.hip take the shape.  Each limit restates ONE condition of that file:
      forward:  segclip_center_logits_fwd, `(size_t)T * CG * sizeof(float) > 60000` -> unsupported         (T <= 1875)
      backward: segclip_center_logits_bwd, `lds = (T * CG + CG * D) * sizeof(float)`, `lds > 64000` -> unsupported
                                                                          (T <= 1232 at D = 768, T <= 976 at D = 1024)
    A change of either line there is a change of the matching line here (tests/test_center_stage_gpu.py runs both sides of
    both limits through center_logits)."""
    if G != 8 or D not in (768, 1024):
        return False
    if T * 8 * 4 > 60000:
        return False
    return not backward or (T * 8 + 8 * D) * 4 <= 64000


def center_logits(q, k, exact):
    """(B,G,T) fp32 assignment logits; exact=True (the exact-f32 mode) or uncovered shapes: the exact-fp32 batched GEMM.
    Where a gradient will be asked for, the token-loop forward is chosen only if the token-loop backward covers the shape too
    (its LDS limit is the lower one); a forward-only call keeps the token loop up to the forward's own limit."""
    B, G, D = q.shape
    needs_grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad)
    if not exact and center_logits_covers(G, k.shape[1], D, backward=needs_grad):
        return CenterLogitsFn.apply(q, k)
    return bmm(q, k, transB=True, out_dtype=torch.float32)


# ---------------------------------------------------------------- zero-shot segmentation inference (segment.hip)
def seg_group_table(group_tokens, pooled, text, logit_scale, topk, want_mask=False):
    """Per window the G x N group-class table of ViTSegInference.encode_decode (vit_seg.py:218-254).
    group_tokens (W, G, C) and pooled (W, C) may be strided views of one (W, 1 + G, C) tensor; text (N, C) normalised;
    logit_scale a device scalar.  -> (table (W, G, N), table_max (W), best_class (W, G) int32, best_score (W, G))
    [+ topk_mask (W, N) uint8].  No autograd, fp32 only."""
    L.require_cuda(group_tokens, pooled, text, logit_scale)
    Wn, G, Cc = group_tokens.shape
    N = text.shape[0]
    for t in (group_tokens, pooled, text, logit_scale):
        if t.dtype != torch.float32:
            raise TypeError("seg_group_table: fp32 inputs only")
    text = text.contiguous()
    if group_tokens.stride(2) != 1 or group_tokens.stride(1) != Cc or (Wn > 1 and group_tokens.stride(0) < G * Cc):
        group_tokens = group_tokens.contiguous()
    if pooled.stride(1) != 1:
        pooled = pooled.contiguous()
    if pooled.shape != (Wn, Cc) or text.shape[1] != Cc:
        raise ValueError("seg_group_table: shapes do not agree")
    dev = text.device
    table = torch.empty(Wn, G, N, dtype=torch.float32, device=dev)
    tmax = torch.empty(Wn, dtype=torch.float32, device=dev)
    bcls = torch.empty(Wn, G, dtype=torch.int32, device=dev)
    bsc = torch.empty(Wn, G, dtype=torch.float32, device=dev)
    mask = torch.empty(Wn, N, dtype=torch.uint8, device=dev) if want_mask else None
    L.check(L.load().segclip_seg_group_table(L.ptr(group_tokens), group_tokens.stride(0), L.ptr(pooled), pooled.stride(0),
                                             L.ptr(text), L.ptr(logit_scale.detach()), L.ptr(table), L.ptr(tmax), L.ptr(bcls),
                                             L.ptr(bsc), L.ptr(mask), Wn, G, N, Cc, int(topk), L.stream()), "seg_group_table")
    out = (table, tmax, bcls, bsc)
    return out + (mask,) if want_mask else out


def _seg_pixel_args(soft_attn, tables, windows, image_first, out_size, win_size, grid):
    table, tmax, bcls, bsc = tables
    L.require_cuda(soft_attn, table, tmax, bcls, bsc, windows, image_first)
    nW, G, N = table.shape
    B, H, W = out_size
    if soft_attn.dtype != torch.float32 or table.dtype != torch.float32 or windows.dtype != torch.int32 \
            or image_first.dtype != torch.int32 or bcls.dtype != torch.int32:
        raise TypeError("seg pixel kernels: fp32 soft_attn / tables, int32 window list")
    if soft_attn.numel() != nW * G * grid[0] * grid[1] or tuple(windows.shape) != (nW, 3) or image_first.numel() != B + 1 \
            or tmax.numel() != nW or bcls.numel() != nW * G or bsc.numel() != nW * G:
        raise ValueError("seg pixel kernels: shapes do not agree")
    keep = tuple(t.contiguous() for t in (soft_attn, table, tmax, bcls, bsc, windows, image_first))
    return keep, (nW, B, H, W, win_size[0], win_size[1], grid[0], grid[1], G, N)


def seg_label_map(soft_attn, tables, windows, image_first, out_size, win_size, grid, with_bg, bg_thresh, labels=True,
                  groups=False):
    """The fused pixel kernel (segclip_seg_label_map): soft_attn (nW, G, gh * gw) + the outputs of seg_group_table + the
    window list -> labels (B, H, W) uint8 and / or groups (B, H, W) uint8.  `labels` / `groups`: True (allocate), False
    (skip) or a contiguous uint8 tensor of B * H * W elements to write into."""
    keep, dims = _seg_pixel_args(soft_attn, tables, windows, image_first, out_size, win_size, grid)

    def out(o):
        if o is False or o is None:
            return None
        if o is True:
            return torch.empty(out_size, dtype=torch.uint8, device=soft_attn.device)
        if o.dtype != torch.uint8 or not o.is_contiguous() or o.numel() != out_size[0] * out_size[1] * out_size[2]:
            raise ValueError("seg_label_map: outputs are contiguous uint8 tensors of B * H * W elements")
        return o

    lab, grp = out(labels), out(groups)
    L.check(L.load().segclip_seg_label_map(*(L.ptr(t) for t in keep), *dims, int(bool(with_bg)), float(bg_thresh), L.ptr(lab),
                                           L.ptr(grp), L.stream()), "seg_label_map")
    return lab, grp


def seg_logits(soft_attn, tables, windows, image_first, out_size, win_size, grid, with_bg, bg_thresh, out=None):
    """The dense output (segclip_seg_logits): (B, N + with_bg, H, W) fp32 as encode_decode / slide_inference define it."""
    keep, dims = _seg_pixel_args(soft_attn, tables, windows, image_first, out_size, win_size, grid)
    N = tables[0].shape[2]
    shape = (out_size[0], N + int(bool(with_bg)), out_size[1], out_size[2])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=soft_attn.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != shape[0] * shape[1] * shape[2] * shape[3]:
        raise ValueError("seg_logits: out is a contiguous fp32 tensor of B * (N + with_bg) * H * W elements")
    L.check(L.load().segclip_seg_logits(*(L.ptr(t) for t in keep), *dims, int(bool(with_bg)), float(bg_thresh), L.ptr(out),
                                        L.stream()), "seg_logits")
    return out


SEG_IMAGE_COLS = L.const("SEG_IMAGE_COLS")  # int64 columns of one row of the image table of segclip_seg_label_map_rescaled
SEG_EVAL_TILE = L.const("SEG_EVAL_TILE")  # output pixels of one of its workgroups


def _upload_table(rows, dtype, device):
    """A host-built descriptor table -> the device, through pinned memory: the copy is enqueued on the current stream and the
    host does not wait for the device (a copy from pageable memory waits for the stream, and with it for everything enqueued
    before).  torch's host allocator keeps the pinned block until the copy has run."""
    table = torch.tensor(rows, dtype=dtype)
    if torch.device(device).type != "cuda":   # the table builders also run without a device (their layout is tested there)
        return table.to(device)
    return table.pin_memory().to(device, non_blocking=True)


def _seg_image_row(what, r, out, label_off, gt_off, first_block, flags=0):
    """One row of the 16-column image table: of an image (seg_image_table) or of one of its views (seg_view_tables), which
    carries its image's output size, label offset, ground-truth offset and first workgroup."""
    (H, W), (oh, ow), (wh, ww), (gh, gw) = r["net"], out, r["win"], r["grid"]
    if min(H, W, oh, ow, wh, ww, gh, gw) < 1 or r["count"] < 1:
        raise ValueError(f"{what}: sizes must be positive, got {r}")
    return [r["first"], r["count"], H, W, oh, ow, label_off, gt_off, first_block, wh, ww, gh, gw, r["soft_off"], flags, 0]


def seg_image_table(rows, device):
    """The device descriptor table of seg_label_map_rescaled from per-image dicts(first, count, net=(H, W), out=(oh, ow),
    win=(win_h, win_w), grid=(gh, gw), soft_off[, gt_off]).  Label offsets are assigned here, each a multiple of 4.
    -> (table (B, 16) int64, label offsets, labels_bytes, n_blocks, max windows of an image)."""
    tab, offs, lab, blk, most = [], [], 0, 0, 0
    for r in rows:
        oh, ow = r["out"]
        tab.append(_seg_image_row("seg_image_table", r, (oh, ow), lab, r.get("gt_off", -1), blk))
        offs.append(lab)
        lab += (oh * ow + 3) // 4 * 4
        blk += (oh * ow + SEG_EVAL_TILE - 1) // SEG_EVAL_TILE
        most = max(most, r["count"])
    return _upload_table(tab, torch.int64, device).view(-1, SEG_IMAGE_COLS), offs, lab, blk, most


def _seg_fused_args(what, soft_attn, tables, windows, images, views=None):
    """The common inputs of the fused label-map kernels: flat soft_attn, the outputs of seg_group_table, the window list, the
    image table and, for the view kernels, the view table (they do not read best_class).
    -> (the tensors, contiguous, in the kernels' argument order; (nW, G, N))."""
    table, tmax, bcls, bsc = tables
    ints, tabs = ((bcls,), (images,)) if views is None else ((), (images, views))
    L.require_cuda(soft_attn, table, tmax, *ints, bsc, windows, *tabs)
    nW, G, N = table.shape
    if soft_attn.dtype != torch.float32 or table.dtype != torch.float32 or windows.dtype != torch.int32 \
            or any(t.dtype != torch.int32 for t in ints) or any(t.dtype != torch.int64 for t in tabs):
        raise TypeError(f"{what}: fp32 soft_attn / tables, int32 window list, int64 image "
                        f"{'table' if views is None else 'and view tables'}")
    if tuple(windows.shape) != (nW, 3) or images.dim() != 2 or images.shape[1] != SEG_IMAGE_COLS or tmax.numel() != nW \
            or any(t.numel() != nW * G for t in ints + (bsc,)) \
            or (views is not None and (views.dim() != 2 or views.shape[1] != L.const("SEG_VIEW_COLS"))):
        raise ValueError(f"{what}: shapes do not agree")
    return tuple(t.contiguous() for t in (soft_attn, table, tmax, *ints, bsc, windows, *tabs)), (nW, G, N)


def _seg_check_outputs(what, labels, gt, areas, n_classes, T=None, dtype=torch.uint8):
    """`labels` / `gt` / `areas` of the fused label-map kernels and of seg_refine; T: the sweep's leading dimension of
    `labels` and `areas`, one plane per threshold; dtype: of the label maps (torch.int16 for the wide entries)."""
    L.require_cuda(labels, gt, areas)
    for name, t in (("labels", labels), ("gt", gt)):
        if t is not None and (t.dtype != dtype or not t.is_contiguous()):
            raise ValueError(f"{what}: {name} is a contiguous {str(dtype).split('.')[-1]} tensor")
    if T is not None and labels is not None and (labels.dim() != 2 or labels.shape[0] != T):
        raise ValueError(f"{what}: labels is a (T, labels_bytes) uint8 tensor, one plane per threshold")
    if (gt is None) != (areas is None):
        raise ValueError(f"{what}: gt and areas go together")
    lead, shape = ((), "(3, N + with_bg)") if T is None else ((T,), "(T, 3, N + 1)")
    if areas is not None and (areas.dtype != torch.int64 or not areas.is_contiguous() or tuple(areas.shape) != lead + (3, n_classes)):
        raise ValueError(f"{what}: areas is a contiguous {shape} int64 tensor")


def seg_label_map_rescaled(soft_attn, tables, windows, images, n_blocks, max_image_windows, with_bg, bg_thresh, labels=None,
                           gt=None, areas=None, ignore_index=255, reduce_zero_label=False):
    """The fused evaluation kernel (segclip_seg_label_map_rescaled): flat soft_attn + the outputs of seg_group_table + the
    window list + the image table -> `labels` (flat uint8, or None) at every image's output size and, with `gt` (flat uint8),
    the (3, C) int64 `areas` added to in place."""
    keep, (nW, G, N) = _seg_fused_args("seg_label_map_rescaled", soft_attn, tables, windows, images)
    _seg_check_outputs("seg_label_map_rescaled", labels, gt, areas, N + int(bool(with_bg)))
    L.check(L.load().segclip_seg_label_map_rescaled(
        L.ptr(keep[0]), keep[0].numel(), *(L.ptr(t) for t in keep[1:]), nW, images.shape[0], int(n_blocks), int(max_image_windows),
        G, N, int(bool(with_bg)), float(bg_thresh), L.ptr(labels), labels.numel() if labels is not None else 0, L.ptr(gt),
        gt.numel() if gt is not None else 0, int(ignore_index), int(bool(reduce_zero_label)), L.ptr(areas), L.stream()),
        "seg_label_map_rescaled")
    return labels


SEG_WIDE_MAX_CLASSES = L.const("SEG_WIDE_MAX_CLASSES")  # classes (background included) of the 16-bit label maps: segclip_seg_label_map_rescaled_wide


def seg_label_map_rescaled_wide(soft_attn, tables, windows, images, n_blocks, max_image_windows, with_bg, bg_thresh, labels=None,
                                gt=None, areas=None, ignore_index=255, reduce_zero_label=False):
    """seg_label_map_rescaled for up to SEG_WIDE_MAX_CLASSES classes (segclip_seg_label_map_rescaled_wide): `labels` and `gt`
    are flat contiguous torch.int16 tensors whose elements the kernel reads and writes as unsigned 16-bit values (a uint16
    array goes in as .view(torch.int16)), the offsets of the image table count elements, `areas` is (3, C) int64 and
    ignore_index an integer compared with the unsigned value."""
    keep, (nW, G, N) = _seg_fused_args("seg_label_map_rescaled_wide", soft_attn, tables, windows, images)
    _seg_check_outputs("seg_label_map_rescaled_wide", labels, gt, areas, N + int(bool(with_bg)), dtype=torch.int16)
    L.check(L.load().segclip_seg_label_map_rescaled_wide(
        L.ptr(keep[0]), keep[0].numel(), *(L.ptr(t) for t in keep[1:]), nW, images.shape[0], int(n_blocks), int(max_image_windows),
        G, N, int(bool(with_bg)), float(bg_thresh), L.ptr(labels), labels.numel() if labels is not None else 0, L.ptr(gt),
        gt.numel() if gt is not None else 0, int(ignore_index), int(bool(reduce_zero_label)), L.ptr(areas), L.stream()),
        "seg_label_map_rescaled_wide")
    return labels


SEG_MAX_THRESHOLDS = L.const("SEG_MAX_THRESHOLDS")  # background thresholds of one segclip_seg_label_map_rescaled_sweep launch


def seg_label_map_sweep(soft_attn, tables, windows, images, n_blocks, max_image_windows, thresholds, labels=None, gt=None,
                        areas=None, ignore_index=255, reduce_zero_label=False):
    """The threshold sweep (segclip_seg_label_map_rescaled_sweep): seg_label_map_rescaled with the background class for every
    bg_thresh of `thresholds` (T host floats, finite and strictly increasing, T <= 16) in one launch -> `labels` ((T, labels_bytes)
    uint8: plane t is the single call's output at thresholds[t], or None) and, with `gt`, the (T, 3, N + 1) int64 `areas` added
    to in place, slice t as the single call adds it.  The library checks the thresholds: a bad list is a RuntimeError, more than
    16 an L.Unsupported."""
    keep, (nW, G, N) = _seg_fused_args("seg_label_map_sweep", soft_attn, tables, windows, images)
    thr = [float(v) for v in thresholds]
    T = len(thr)
    _seg_check_outputs("seg_label_map_sweep", labels, gt, areas, N + 1, T)
    host = (L.C.c_float * max(T, 1))(*thr)
    L.check(L.load().segclip_seg_label_map_rescaled_sweep(
        L.ptr(keep[0]), keep[0].numel(), *(L.ptr(t) for t in keep[1:]), nW, images.shape[0], int(n_blocks), int(max_image_windows),
        G, N, L.C.cast(host, L.C.c_void_p), T, L.ptr(labels), labels.shape[1] if labels is not None else 0, L.ptr(gt),
        gt.numel() if gt is not None else 0, int(ignore_index), int(bool(reduce_zero_label)), L.ptr(areas), L.stream()),
        "seg_label_map_sweep")
    return labels


SEG_MAX_VIEWS = L.const("SEG_MAX_VIEWS")  # views of one image in segclip_seg_label_map_views
SEG_MAX_IMAGE_WINDOWS = L.const("SEG_MAX_IMAGE_WINDOWS")  # windows of one image, over all its views
SEG_FLIP_H, SEG_FLIP_V = L.const("SEG_FLIP_H"), L.const("SEG_FLIP_V")


def seg_view_tables(rows, view_counts, device):
    """The device tables of seg_label_map_views / seg_view_probs.  rows: one dict per view as seg_image_table takes them, plus
    flags (SEG_FLIP_H | SEG_FLIP_V), the views of an image consecutive; view_counts: the number of views of every image.
    Every view row carries its image's output size, label offset (a multiple of 4), ground-truth offset and first workgroup.
    -> (image table (R, 16) int64, view table (B, 2) int64, label offsets per image, labels_bytes, n_blocks,
        most windows of an image over its views, most windows of a view, most views)."""
    if sum(view_counts) != len(rows):
        raise ValueError(f"seg_view_tables: {len(rows)} view rows but the view counts sum to {sum(view_counts)}")
    tab, vtab, offs, lab, blk, r0 = [], [], [], 0, 0, 0
    most_img = most_view = 0
    for i, V in enumerate(view_counts):
        if not 1 <= V <= SEG_MAX_VIEWS:
            raise ValueError(f"image {i}: {V} views, 1 .. {SEG_MAX_VIEWS} supported")
        mine = rows[r0:r0 + V]
        oh, ow = mine[0]["out"]
        for v, r in enumerate(mine):
            if tuple(r["out"]) != (oh, ow):
                raise ValueError(f"image {i} view {v}: output size {tuple(r['out'])}, its first view has {(oh, ow)}")
            flags = int(r.get("flags", 0))
            if flags not in (0, 1, 2, 3):
                raise ValueError(f"image {i} view {v}: flags {flags}, bit 0 = horizontal flip and bit 1 = vertical flip")
            tab.append(_seg_image_row("seg_view_tables", r, (oh, ow), lab, mine[0].get("gt_off", -1), blk, flags))
            most_view = max(most_view, r["count"])
        n_win = sum(r["count"] for r in mine)
        if n_win > SEG_MAX_IMAGE_WINDOWS:
            raise ValueError(f"image {i}: {n_win} windows over its {V} views, at most {SEG_MAX_IMAGE_WINDOWS} supported")
        most_img = max(most_img, n_win)
        vtab.append([r0, V])
        offs.append(lab)
        lab += (oh * ow + 3) // 4 * 4
        blk += (oh * ow + SEG_EVAL_TILE - 1) // SEG_EVAL_TILE
        r0 += V
    return (torch.tensor(tab, dtype=torch.int64, device=device).view(-1, SEG_IMAGE_COLS),
            torch.tensor(vtab, dtype=torch.int64, device=device).view(-1, 2), offs, lab, blk, most_img, most_view, max(view_counts))


def seg_label_map_views(soft_attn, tables, windows, images, views, n_blocks, max_image_windows, max_view_windows, max_views, with_bg,
                        bg_thresh, labels=None, gt=None, areas=None, ignore_index=255, reduce_zero_label=False):
    """The fused multi-view kernel (segclip_seg_label_map_views): as seg_label_map_rescaled with the tables of
    seg_view_tables - per view the rescaled class logits at the mirrored position, their soft-max, the mean over an image's
    views, its first maximum -> `labels` (flat uint8, or None) and, with `gt`, the (3, C) int64 `areas` added to in place."""
    (soft, table, tmax, bsc, win, img, vws), (nW, G, N) = _seg_fused_args("seg_label_map_views", soft_attn, tables, windows, images, views)
    _seg_check_outputs("seg_label_map_views", labels, gt, areas, N + int(bool(with_bg)))
    L.check(L.load().segclip_seg_label_map_views(
        L.ptr(soft), soft.numel(), L.ptr(table), L.ptr(tmax), L.ptr(bsc), L.ptr(win), L.ptr(img), img.shape[0], L.ptr(vws), nW,
        vws.shape[0], int(n_blocks), int(max_image_windows), int(max_view_windows), int(max_views), G, N, int(bool(with_bg)),
        float(bg_thresh), L.ptr(labels), labels.numel() if labels is not None else 0, L.ptr(gt), gt.numel() if gt is not None else 0,
        int(ignore_index), int(bool(reduce_zero_label)), L.ptr(areas), L.stream()), "seg_label_map_views")
    return labels


def seg_view_probs(soft_attn, tables, windows, images, views, n_blocks, max_image_windows, max_view_windows, max_views, with_bg,
                   bg_thresh, out_size, out=None):
    """The dense twin (segclip_seg_view_probs) for ONE image: (N + with_bg, oh, ow) fp32, the mean over its views of the
    soft-max of the rescaled class logits, by the device functions of seg_label_map_views (whose label is its first maximum)."""
    (soft, table, tmax, bsc, win, img, vws), (nW, G, N) = _seg_fused_args("seg_view_probs", soft_attn, tables, windows, images, views)
    if vws.shape[0] != 1:
        raise ValueError(f"seg_view_probs: one image per call, got a view table of {vws.shape[0]}")
    shape = (N + int(bool(with_bg)), int(out_size[0]), int(out_size[1]))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=soft.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != shape[0] * shape[1] * shape[2]:
        raise ValueError("seg_view_probs: out is a contiguous fp32 tensor of (N + with_bg) * oh * ow elements")
    L.require_cuda(out)
    L.check(L.load().segclip_seg_view_probs(
        L.ptr(soft), soft.numel(), L.ptr(table), L.ptr(tmax), L.ptr(bsc), L.ptr(win), L.ptr(img), img.shape[0], L.ptr(vws), nW,
        int(n_blocks), int(max_image_windows), int(max_view_windows), int(max_views), G, N, int(bool(with_bg)), float(bg_thresh),
        L.ptr(out), out.numel(), L.stream()), "seg_view_probs")
    return out


def seg_areas(pred, gt, num_classes, ignore_index=255, reduce_zero_label=False, areas=None):
    """mmseg's intersect_and_union of uint8 label maps (segclip_seg_areas): -> (3, C) int64 = intersection, prediction area,
    label area per class; added to `areas` when given."""
    L.require_cuda(pred, gt, areas)
    if pred.dtype != torch.uint8 or gt.dtype != torch.uint8 or pred.numel() != gt.numel():
        raise ValueError("seg_areas: pred and gt are uint8 tensors of the same size")
    if areas is None:
        areas = torch.zeros(3, num_classes, dtype=torch.int64, device=pred.device)
    elif areas.dtype != torch.int64 or not areas.is_contiguous() or tuple(areas.shape) != (3, num_classes):
        raise ValueError("seg_areas: areas is a contiguous (3, C) int64 tensor")
    pred, gt = pred.contiguous(), gt.contiguous()
    L.check(L.load().segclip_seg_areas(L.ptr(pred), L.ptr(gt), pred.numel(), int(num_classes), int(ignore_index),
                                       int(bool(reduce_zero_label)), L.ptr(areas), L.stream()), "seg_areas")
    return areas


def seg_areas_wide(pred, gt, num_classes, ignore_index=255, reduce_zero_label=False, areas=None):
    """seg_areas for 16-bit label maps (segclip_seg_areas_wide): pred and gt are torch.int16 tensors read as unsigned 16-bit
    values, at most SEG_WIDE_MAX_CLASSES classes -> (3, C) int64; added to `areas` when given."""
    L.require_cuda(pred, gt, areas)
    if pred.dtype != torch.int16 or gt.dtype != torch.int16 or pred.numel() != gt.numel():
        raise ValueError("seg_areas_wide: pred and gt are int16 tensors of the same size")
    if areas is None:
        areas = torch.zeros(3, num_classes, dtype=torch.int64, device=pred.device)
    elif areas.dtype != torch.int64 or not areas.is_contiguous() or tuple(areas.shape) != (3, num_classes):
        raise ValueError("seg_areas_wide: areas is a contiguous (3, C) int64 tensor")
    pred, gt = pred.contiguous(), gt.contiguous()
    L.check(L.load().segclip_seg_areas_wide(L.ptr(pred), L.ptr(gt), pred.numel(), int(num_classes), int(ignore_index),
                                            int(bool(reduce_zero_label)), L.ptr(areas), L.stream()), "seg_areas_wide")
    return areas


def seg_confusion(pred, gt, num_classes, ignore_index=255, reduce_zero_label=False, conf=None):
    """The confusion matrix of label maps (segclip_seg_confusion / segclip_seg_confusion_wide, picked by the dtype: uint8, or
    torch.int16 read as unsigned 16-bit values): -> (C + 1, C + 1) int64, row = ground-truth class, column = predicted class,
    index C on either axis the out-of-range bin; the ground-truth rule is seg_areas'.  Added to `conf` when given."""
    L.require_cuda(pred, gt, conf)
    if pred.dtype not in (torch.uint8, torch.int16) or gt.dtype != pred.dtype or pred.numel() != gt.numel():
        raise ValueError("seg_confusion: pred and gt are both uint8 or both int16 tensors of the same size")
    side = int(num_classes) + 1
    if conf is None:
        conf = torch.zeros(side, side, dtype=torch.int64, device=pred.device)
    elif conf.dtype != torch.int64 or not conf.is_contiguous() or tuple(conf.shape) != (side, side):
        raise ValueError("seg_confusion: conf is a contiguous (C + 1, C + 1) int64 tensor")
    pred, gt = pred.contiguous(), gt.contiguous()
    wide = pred.dtype == torch.int16
    fn = L.load().segclip_seg_confusion_wide if wide else L.load().segclip_seg_confusion
    L.check(fn(L.ptr(pred), L.ptr(gt), pred.numel(), int(num_classes), int(ignore_index), int(bool(reduce_zero_label)), L.ptr(conf),
               L.stream()), "seg_confusion_wide" if wide else "seg_confusion")
    return conf


def seg_confusion_route(num_classes, dtype=torch.uint8):
    """The route seg_confusion takes for this class count and label dtype on the current device: "dense" (the whole matrix in
    LDS) or "sparse" (a table of pairs in LDS).  Raises as seg_confusion does for a class count it refuses."""
    if dtype not in (torch.uint8, torch.int16):
        raise ValueError("seg_confusion_route: the label dtype is torch.uint8 or torch.int16")
    rc = L.load().segclip_seg_confusion_route(int(num_classes), int(dtype == torch.int16))
    if rc < 0:
        L.check(rc, "seg_confusion_route")
    return ("dense", "sparse")[rc]


SEG_IA_COLS = L.const("SEG_IA_COLS")  # int64 columns of one row of the image table of segclip_seg_image_areas
SEG_IA_TILE = L.const("SEG_IA_TILE")  # pixels of one of its workgroups


def seg_image_areas_table(pred_offs, gt_offs, counts, device):
    """The device image table of seg_image_areas: pred_offs [the element offset of each picture's prediction in the flat
    prediction buffer], gt_offs [that of its ground truth in the flat ground-truth buffer], counts [its pixels]
    -> (table (B, 4) int64, n_blocks).  The host lists go to the device in one small copy through pinned memory."""
    n = len(counts)
    if n == 0:
        raise ValueError("seg_image_areas: counts is empty")
    for name, v in (("pred_offs", pred_offs), ("gt_offs", gt_offs)):
        if len(v) != n:
            raise ValueError(f"seg_image_areas: {n} counts but {name} has {len(v)} entries")
    tab, blk = [], 0
    for i, (po, go, cnt) in enumerate(zip(pred_offs, gt_offs, counts)):
        po, go, cnt = int(po), int(go), int(cnt)
        if not 1 <= cnt < 1 << 31:
            raise ValueError(f"seg_image_areas: a picture has 1 .. 2^31 - 1 pixels, picture {i} has {cnt}")
        if po < 0 or go < 0:
            raise ValueError(f"seg_image_areas: offsets are not negative, picture {i} has {po} and {go}")
        tab.append([po, go, cnt, blk])
        blk += (cnt + SEG_IA_TILE - 1) // SEG_IA_TILE
    return _upload_table(tab, torch.int64, device).view(-1, SEG_IA_COLS), blk


def seg_image_areas(pred, gt, table, n_blocks, num_classes, ignore_index=255, reduce_zero_label=False, out=None):
    """The (3, C) areas of seg_areas for every picture of a list on its own, in one launch (segclip_seg_image_areas /
    segclip_seg_image_areas_wide, picked by the dtype: uint8, or torch.int16 read as unsigned 16-bit values): pred and gt are
    flat buffers, `table` and n_blocks those of seg_image_areas_table -> (B, 3, C) int64, row i = intersection, prediction area
    and label area of picture i; added to `out` when given.  A picture whose table row the device refuses is skipped.  No host
    synchronisation."""
    L.require_cuda(pred, gt, table, out)
    if pred.dtype not in (torch.uint8, torch.int16) or gt.dtype != pred.dtype:
        raise ValueError("seg_image_areas: pred and gt are both uint8 or both int16 tensors")
    if not pred.is_contiguous() or not gt.is_contiguous():
        raise ValueError("seg_image_areas: pred and gt are contiguous buffers (the table's offsets count their elements)")
    _check_image_table("seg_image_areas", table, SEG_IA_COLS, "seg_image_areas_table")
    B, C = table.shape[0], int(num_classes)
    if out is None:
        out = torch.zeros(B, 3, max(C, 0), dtype=torch.int64, device=pred.device)
    elif out.dtype != torch.int64 or not out.is_contiguous() or tuple(out.shape) != (B, 3, C):
        raise ValueError(f"seg_image_areas: out is a contiguous (B, 3, C) = ({B}, 3, {C}) int64 tensor")
    wide = pred.dtype == torch.int16
    fn = L.load().segclip_seg_image_areas_wide if wide else L.load().segclip_seg_image_areas
    L.check(fn(L.ptr(pred), pred.numel(), L.ptr(gt), gt.numel(), L.ptr(table), B, int(n_blocks), C, int(ignore_index),
               int(bool(reduce_zero_label)), L.ptr(out), L.stream()), "seg_image_areas_wide" if wide else "seg_image_areas")
    return out


SEG_SOURCE_COLS = L.const("SEG_SOURCE_COLS")  # int64 columns of one row of the source table of segclip_seg_windows_from_u8
SEG_SOURCE_LIMIT = L.const("SEG_SOURCE_LIMIT")  # h, w, H, W of an image stay below it (the kernel's integer coordinates)


def _seg_pictures(what, raws, noun="a source image"):
    """The decoded pictures of a table builder, checked one by one: (h, w, 3) uint8 on one device, sides of 1 ..
    SEG_SOURCE_LIMIT - 1, channels interleaved and pixels contiguous, rows possibly strided.  `what:` opens the messages, `noun`
    names a picture in them.  Yields (address, h, w, row stride in bytes) per picture."""
    L.require_cuda(*raws)
    for t in raws:
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8:
            raise ValueError(f"{what}: {noun} is an (h, w, 3) uint8 tensor, got {t.dtype} {tuple(t.shape)}")
        h, w = int(t.shape[0]), int(t.shape[1])
        if t.device != raws[0].device:
            raise ValueError(f"{what}: the {noun.split(' ', 1)[1]}s are on different devices")
        if min(h, w) < 1 or max(h, w) >= SEG_SOURCE_LIMIT:
            raise ValueError(f"{what}: sizes 1 .. {SEG_SOURCE_LIMIT - 1} supported, got {h}x{w}")
        if t.stride(2) != 1 or t.stride(1) != 3 or (h > 1 and t.stride(0) < 3 * w):
            raise ValueError(f"{what}: {noun} has interleaved channels and contiguous pixels (strides (>= 3 w, 3, 1)), got "
                             f"{tuple(t.stride())}")
        yield t.data_ptr(), h, w, max(int(t.stride(0)), 3 * w)


def _check_image_table(what, table, cols, builder, rows=None):
    """`table` of a kernel that takes one int64 row of `cols` columns per image, as `builder` makes it."""
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != cols or not table.is_contiguous() \
            or (rows is not None and table.shape[0] != rows):
        raise ValueError(f"{what}: table is the (B, {cols}) int64 tensor of {builder}")


def _workspace(what, ws_bytes, device, floor=0):
    """The workspace a *_ws_bytes query asks for, at least `floor` bytes; a negative answer is the library's error."""
    if ws_bytes < 0:
        L.check(ws_bytes, what)
    return torch.empty(max(ws_bytes, floor), dtype=torch.uint8, device=device)


def _max_side(max_side):
    """The largest h or w of a table, what its builder returned; without one the limit."""
    return SEG_SOURCE_LIMIT - 1 if max_side is None else int(max_side)


def seg_view_source_table(raws, net_sizes, flags):
    """The source table of seg_view_windows_from_u8: seg_source_table's rows and a flag word per row (SEG_FLIP_H | SEG_FLIP_V)
    -> (B, 7) int64.  One row per view: an image with several views appears once per view in `raws`.  flags None: the (B, 6)
    table of the plain kernel."""
    if len(raws) == 0 or len(raws) != len(net_sizes):
        raise ValueError(f"seg_source_table: {len(raws)} images but {len(net_sizes)} network sizes")
    if flags is not None and (len(flags) != len(raws) or any(int(f) not in (0, 1, 2, 3) for f in flags)):
        raise ValueError("seg_view_windows_from_u8: one flag word of 0 .. 3 per source row")
    L.require_cuda(*raws)
    for t in raws:
        if t.dtype != torch.uint8:   # the front end's own error type for a wrong dtype
            raise TypeError(f"seg_windows_from_u8: a source image is uint8, got {t.dtype}")
    tab = []
    for k, ((ptr, h, w, row), (H, W)) in enumerate(zip(_seg_pictures("seg_windows_from_u8", raws), net_sizes)):
        if min(int(H), int(W)) < 1 or max(int(H), int(W)) >= SEG_SOURCE_LIMIT:
            raise ValueError(f"seg_windows_from_u8: sizes 1 .. {SEG_SOURCE_LIMIT - 1} supported, got {h}x{w} -> {H}x{W}")
        tab.append([ptr, h, w, row, int(H), int(W)] + ([] if flags is None else [int(flags[k])]))
    return _upload_table(tab, torch.int64, raws[0].device).view(len(tab), -1)


def seg_source_table(raws, net_sizes):
    """The device source table of seg_windows_from_u8: raws [(h, w, 3) uint8 device tensors, pixels contiguous, rows
    possibly strided], net_sizes [(H, W)] -> (B, 6) int64.  It holds the tensors' addresses: keep `raws` alive while it is
    in use."""
    return seg_view_source_table(raws, net_sizes, None)


def seg_view_windows_from_u8(raws, net_sizes, flags, windows, win_size, mean, inv_std, reverse_channels=False, out=None, table=None):
    """seg_windows_from_u8 for flipped views (segclip_seg_view_windows_from_u8): window pixel (Y, X) of a row with the
    horizontal flag reads the resized image at (Y, W - 1 - X), with the vertical flag at (H - 1 - Y, X) - mmseg's flip after
    the resize.  Flags 0 give seg_windows_from_u8's output bit for bit.  table: seg_view_source_table(raws, net_sizes, flags)."""
    return _seg_windows_launch(raws, net_sizes, flags, table, windows, win_size, mean, inv_std, reverse_channels, out)


def seg_windows_from_u8(raws, net_sizes, windows, win_size, mean, inv_std, reverse_channels=False, out=None, table=None):
    """The fused front end (segclip_seg_windows_from_u8): decoded uint8 images -> (n_windows, 3, win_h, win_w) fp32, every
    window pixel resized bilinearly (cv2 INTER_LINEAR geometry) from its image to the image's network size and normalised as
    (r - mean[c]) * inv_std[c].  windows: (n_windows, 3) int32 device rows (image, y0, x0), or a list of them; a window outside
    its image's network size or with an image index outside the list is zero-filled.  table: seg_source_table(raws,
    net_sizes) when the caller launches several times on the same images."""
    return _seg_windows_launch(raws, net_sizes, None, table, windows, win_size, mean, inv_std, reverse_channels, out)


def _seg_windows_launch(raws, net_sizes, flags, table, windows, win_size, mean, inv_std, reverse_channels, out):
    """flags None: the plain kernel on the (B, 6) table; a flag word per row: the view kernel on the (B, 7) one."""
    entry, cols = ("segclip_seg_windows_from_u8", SEG_SOURCE_COLS) if flags is None else \
        ("segclip_seg_view_windows_from_u8", L.const("SEG_SOURCE_VIEW_COLS"))
    if table is None:
        table = seg_view_source_table(raws, net_sizes, flags)
    _check_image_table("seg_windows_from_u8", table, cols, "seg_source_table", rows=len(raws))
    if not torch.is_tensor(windows):
        windows = torch.tensor(windows, dtype=torch.int32, device=table.device).view(-1, 3)
    L.require_cuda(table, windows, out)
    if windows.dtype != torch.int32 or windows.dim() != 2 or windows.shape[1] != 3:
        raise ValueError("seg_windows_from_u8: windows is an (n_windows, 3) int32 tensor")
    windows = windows.contiguous()
    wh, ww = int(win_size[0]), int(win_size[1])
    if wh < 1 or ww < 1 or len(mean) != 3 or len(inv_std) != 3:
        raise ValueError("seg_windows_from_u8: a window has win_h, win_w >= 1; mean and inv_std have 3 entries")
    n = windows.shape[0]
    if out is None:
        out = torch.empty(n, 3, wh, ww, dtype=torch.float32, device=table.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n * 3 * wh * ww:
        raise ValueError("seg_windows_from_u8: out is a contiguous fp32 tensor of n_windows * 3 * win_h * win_w elements")
    f3 = L.f32 * 3
    L.check(getattr(L.load(), entry)(L.ptr(table), L.ptr(windows), n, table.shape[0], wh, ww, f3(*mean), f3(*inv_std),
                                     int(bool(reverse_channels)), L.ptr(out), L.stream()), "seg_windows_from_u8")
    return out


# ---------------------------------------------------------------- rendering of segmentation results (segment_render.inc)
SEG_RENDER_TILE = L.const("SEG_RENDER_TILE")  # pixels of one workgroup of segclip_seg_groups_rescaled and segclip_seg_blend
SEG_BLEND_COLS = L.const("SEG_BLEND_COLS")  # int64 columns of one row of the image table of segclip_seg_blend
SEG_MAX_GROUPS = L.const("SEG_MAX_GROUPS")


def seg_groups_rescaled(soft_attn, images, n_blocks, G, groups):
    """The group-map kernel (segclip_seg_groups_rescaled): flat soft_attn + the image table of seg_image_table (one window
    per image; its label offsets are the group offsets) -> `groups`, a flat uint8 tensor written at every image's output
    size.  An image whose row the device refuses keeps its bytes."""
    L.require_cuda(soft_attn, images, groups)
    if soft_attn.dtype != torch.float32 or images.dtype != torch.int64:
        raise TypeError("seg_groups_rescaled: fp32 soft_attn, int64 image table")
    if images.dim() != 2 or images.shape[1] != SEG_IMAGE_COLS:
        raise ValueError("seg_groups_rescaled: images is the (B, 16) table of seg_image_table")
    if groups.dtype != torch.uint8 or not groups.is_contiguous():
        raise ValueError("seg_groups_rescaled: groups is a contiguous uint8 tensor")
    soft_attn, images = soft_attn.contiguous(), images.contiguous()
    L.check(L.load().segclip_seg_groups_rescaled(L.ptr(soft_attn), soft_attn.numel(), L.ptr(images), images.shape[0], int(n_blocks),
                                                 int(G), L.ptr(groups), groups.numel(), L.stream()), "seg_groups_rescaled")
    return groups


def seg_blend_table(raws, map_offsets):
    """The device image table of seg_blend: raws [(h, w, 3) uint8 device tensors, pixels contiguous, rows possibly strided],
    map_offsets [offset of each image's (h, w) indices in the flat map buffer].  Output offsets are assigned here, each a
    multiple of 4.  It holds the tensors' addresses: keep `raws` alive while it is in use.
    -> (table (B, 8) int64, output offsets, out_bytes, n_blocks)."""
    if len(raws) == 0 or len(raws) != len(map_offsets):
        raise ValueError(f"seg_blend: {len(raws)} images but {len(map_offsets)} index maps")
    tab, offs, out, blk = [], [], 0, 0
    for (ptr, h, w, row), mo in zip(_seg_pictures("seg_blend", raws), map_offsets):
        tab.append([ptr, h, w, row, int(mo), out, blk, 0])
        offs.append(out)
        out += (3 * h * w + 3) // 4 * 4
        blk += (h * w + SEG_RENDER_TILE - 1) // SEG_RENDER_TILE
    return torch.tensor(tab, dtype=torch.int64, device=raws[0].device).view(-1, SEG_BLEND_COLS), offs, out, blk


def seg_blend(table, n_blocks, maps, palette, opacity, out, skip_zero=False, reverse_channels=False, sums=None):
    """The overlay kernel (segclip_seg_blend): the table of seg_blend_table + the flat uint8 index maps + a (P, 3) uint8 RGB
    palette -> `out`, flat uint8, (h, w, 3) per image at the table's output offsets; `sums` (B, P, 3) int64 is added to."""
    L.require_cuda(table, maps, palette, out, sums)
    _check_image_table("seg_blend", table, SEG_BLEND_COLS, "seg_blend_table")
    if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= 256:
        raise ValueError(f"seg_blend: a palette is a (P <= 256, 3) uint8 tensor, got {palette.dtype} {tuple(palette.shape)}")
    opacity = float(opacity)
    if not 0.0 < opacity <= 1.0:
        raise ValueError(f"seg_blend: opacity lies in (0, 1], got {opacity}")
    for name, t in (("maps", maps), ("out", out)):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError(f"seg_blend: {name} is a contiguous uint8 tensor")
    P = palette.shape[0]
    if sums is not None and (sums.dtype != torch.int64 or not sums.is_contiguous() or tuple(sums.shape) != (table.shape[0], P, 3)):
        raise ValueError("seg_blend: sums is a contiguous (B, P, 3) int64 tensor")
    palette = palette.contiguous()
    L.check(L.load().segclip_seg_blend(L.ptr(table), table.shape[0], int(n_blocks), L.ptr(maps), maps.numel(), L.ptr(palette), P,
                                       int(bool(reverse_channels)), 1.0 - opacity, opacity, int(bool(skip_zero)), L.ptr(out),
                                       out.numel(), L.ptr(sums), L.stream()), "seg_blend")
    return out


# ---------------------------------------------------------------- pixel-adaptive refinement of label maps (segment_refine.inc)
SEG_REFINE_TILE = L.const("SEG_REFINE_TILE")  # pixels of one workgroup of segclip_seg_refine
SEG_REFINE_COLS = L.const("SEG_REFINE_COLS")  # int64 columns of one row of its image table
SEG_REFINE_MAX_DILATIONS = L.const("SEG_REFINE_MAX_DILATIONS")
SEG_REFINE_MAX_DILATION = L.const("SEG_REFINE_MAX_DILATION")
SEG_REFINE_MAX_ITERS = L.const("SEG_REFINE_MAX_ITERS")


def seg_refine_table(raws, label_offsets):
    """The device image table of seg_refine: raws [(h, w, 3) uint8 device tensors, pixels contiguous, rows possibly strided],
    label_offsets [offset of each image's (h, w) labels in the flat label buffer; the refined labels take the same offsets].
    The ground truths of a call lie flat one after the other, so their offsets are the running sum of h * w.  It holds the
    tensors' addresses: keep `raws` alive while it is in use.  -> (table (B, 8) int64, n_blocks, largest side)."""
    if len(raws) == 0 or len(raws) != len(label_offsets):
        raise ValueError(f"seg_refine: {len(raws)} images but {len(label_offsets)} label maps")
    tab, gt, blk, side = [], 0, 0, 0
    for (ptr, h, w, row), lo in zip(_seg_pictures("seg_refine", raws, "a picture"), label_offsets):
        tab.append([ptr, h, w, row, int(lo), gt, blk, 0])
        gt += h * w
        blk += (h * w + SEG_REFINE_TILE - 1) // SEG_REFINE_TILE
        side = max(side, h, w)
    return torch.tensor(tab, dtype=torch.int64, device=raws[0].device).view(-1, SEG_REFINE_COLS), blk, side


def seg_refine(table, n_blocks, labels, num_classes, dilations, iters, mean, inv_std, reverse_channels=False, out=None, gt=None,
               areas=None, ignore_index=255, reduce_zero_label=False, probs=None, max_side=None):
    """Pixel-adaptive refinement (segclip_seg_refine; the definition stands in include/segclip_hip.h): the table of
    seg_refine_table + the flat uint8 `labels` -> `out`, flat uint8 with the same offsets (a new tensor unless given; it may not
    overlap `labels`).  dilations: 1 .. 6 increasing values in 1 .. 32; iters: 0 .. 32.  With `gt` (flat uint8) the (3, C) int64
    `areas` of seg_areas are added to for the refined labels, by the last kernel.  probs: a flat fp32 buffer for ONE image's
    (C, h, w) final planes, for tests and inspection.  max_side: the largest h or w of the table (seg_refine_table's third
    result; defaults to the limit).  No host synchronisation; the workspace does not depend on num_classes."""
    L.require_cuda(table, labels, out, gt, areas, probs)
    _check_image_table("seg_refine", table, SEG_REFINE_COLS, "seg_refine_table")
    if out is None:
        out = torch.empty_like(labels)
    _seg_check_outputs("seg_refine", labels, gt, areas, int(num_classes))
    if out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("seg_refine: out is a contiguous uint8 tensor")
    if probs is not None and (probs.dtype != torch.float32 or not probs.is_contiguous()):
        raise ValueError("seg_refine: probs is a contiguous fp32 tensor")
    if len(mean) != 3 or len(inv_std) != 3:
        raise ValueError("seg_refine: mean and inv_std have 3 entries")
    dil = [int(d) for d in dilations]
    B, D = table.shape[0], len(dil)
    lib = L.load()
    ws_bytes, ws = 0, None
    if int(iters) != 0:   # no iteration: the labels pass through, nothing to hold
        ws_bytes = lib.segclip_seg_refine_ws_bytes(labels.numel(), B, D)
        ws = _workspace("seg_refine", ws_bytes, labels.device)
    f3 = L.f32 * 3
    L.check(lib.segclip_seg_refine(
        L.ptr(table), B, int(n_blocks), _max_side(max_side), L.ptr(labels), labels.numel(),
        int(num_classes), (C.c_int32 * max(D, 1))(*dil), D, int(iters), f3(*mean), f3(*inv_std), int(bool(reverse_channels)),
        L.ptr(out), out.numel(), L.ptr(gt), gt.numel() if gt is not None else 0, int(ignore_index), int(bool(reduce_zero_label)),
        L.ptr(areas), L.ptr(probs), probs.numel() if probs is not None else 0, L.ptr(ws), ws_bytes, L.stream()), "seg_refine")
    return out


# ---------------------------------------------------------------- connected components of label maps (segment_objects.inc)
def _seg_label_width(what, labels, name="labels"):
    """Components, sieve and boundary take label maps of either width: -> True for int16 (the wide entries), False for uint8."""
    if labels.dtype not in (torch.uint8, torch.int16) or not labels.is_contiguous():
        raise ValueError(f"{what}: {name} is a contiguous uint8 or int16 tensor")
    return labels.dtype == torch.int16


SEG_CC_TILE = (L.const("SEG_CC_TILE_H"), L.const("SEG_CC_TILE_W"))  # (TH, TW): rows x columns of one workgroup's tile of segclip_seg_components
SEG_CC_COLS = L.const("SEG_CC_COLS")  # int64 columns of one row of its image table
SEG_CC_RECORD = L.const("SEG_CC_RECORD")  # int64 columns of a record: image, id, label, area, y0, x0, y1, x1, sum of y, sum of x


def seg_components_table(sizes, offsets, device):
    """The device image table of seg_components: sizes [(h, w)], offsets [offset of each image's h * w entries in the flat
    label buffer; ids, area_px and cleaned take the same offsets] -> (table (B, 8) int64, n_blocks, largest side)."""
    if len(sizes) == 0 or len(sizes) != len(offsets):
        raise ValueError(f"seg_components: {len(sizes)} sizes but {len(offsets)} offsets")
    th, tw = SEG_CC_TILE
    tab, blk, side = [], 0, 0
    for (h, w), off in zip(sizes, offsets):
        h, w = int(h), int(w)
        if min(h, w) < 1 or max(h, w) >= SEG_SOURCE_LIMIT:
            raise ValueError(f"seg_components: sizes 1 .. {SEG_SOURCE_LIMIT - 1} supported, got {h}x{w}")
        tab.append([h, w, int(off), blk, 0, 0, 0, 0])
        blk += ((h + th - 1) // th) * ((w + tw - 1) // tw)
        side = max(side, h, w)
    return torch.tensor(tab, dtype=torch.int64, device=device).view(-1, SEG_CC_COLS), blk, side


def seg_components(table, n_blocks, labels, connectivity=8, skip_label=None, ids=None, area_px=None, records=None, count=None,
                   min_area=0, fill=0, cleaned=None, max_side=None):
    """Connected components of the flat uint8 or int16 `labels` under the table of seg_components_table (segclip_seg_components
    / segclip_seg_components_wide by the dtype; the definition stands in include/segclip_hip.h).  An int16 tensor holds the
    16-bit label maps of SegInference(label_dtype=torch.int16) and is read as unsigned 16-bit values.  Every output is optional
    and written where given: ids / area_px flat int32 with one entry per label, records (K, 10) int64 with count (1,) int64
    (count alone is allowed), cleaned flat, of the labels' dtype and size (it may not overlap them): fill where a component has
    fewer than min_area pixels.  skip_label: a value whose pixels belong to no component.  skip_label and fill are in 0 .. 255
    for uint8 labels and 0 .. 65535 for int16 labels.  max_side: the largest h or w of the table (defaults to the limit).  No
    host synchronisation.  -> None."""
    L.require_cuda(table, labels, ids, area_px, records, count, cleaned)
    _check_image_table("seg_components", table, SEG_CC_COLS, "seg_components_table")
    wide = _seg_label_width("seg_components", labels)
    for name, t, dt in (("ids", ids, torch.int32), ("area_px", area_px, torch.int32), ("records", records, torch.int64),
                        ("count", count, torch.int64), ("cleaned", cleaned, labels.dtype)):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise ValueError(f"seg_components: {name} is a contiguous {dt} tensor")
    if records is not None and (records.dim() != 2 or records.shape[1] != SEG_CC_RECORD):
        raise ValueError(f"seg_components: records is a (K, {SEG_CC_RECORD}) int64 tensor, got {tuple(records.shape)}")
    if count is not None and count.numel() != 1:
        raise ValueError("seg_components: count holds one int64")
    px = [t.numel() for t in (ids, area_px) if t is not None]
    if len(set(px)) > 1:
        raise ValueError("seg_components: ids and area_px have the same number of entries")
    B = table.shape[0]
    lib = L.load()
    ws_bytes = lib.segclip_seg_components_ws_bytes(labels.numel(), B, int(n_blocks))
    ws = _workspace("seg_components", ws_bytes, labels.device, 16)
    L.check((lib.segclip_seg_components_wide if wide else lib.segclip_seg_components)(
        L.ptr(table), B, int(n_blocks), _max_side(max_side), L.ptr(labels), labels.numel(),
        int(connectivity), -1 if skip_label is None else int(skip_label), L.ptr(ids), L.ptr(area_px), px[0] if px else 0,
        L.ptr(records), records.shape[0] if records is not None else 0, L.ptr(count), int(min_area), int(fill), L.ptr(cleaned),
        cleaned.numel() if cleaned is not None else 0, L.ptr(ws), ws_bytes, L.stream()), "seg_components")


SEG_SIEVE_MAX_ROUNDS = L.const("SEG_SIEVE_MAX_ROUNDS")


def seg_sieve(table, n_blocks, labels, connectivity=8, skip_label=None, min_area=0, orphan_fill=None, rounds=1, cleaned=None,
              max_side=None):
    """Despeckling by merging (segclip_seg_sieve; the definition stands in include/segclip_hip.h): under the table of
    seg_components_table, every component of the flat uint8 or int16 `labels` (int16: 16-bit label maps read as unsigned,
    segclip_seg_sieve_wide) with fewer than min_area pixels takes the label of its largest kept 4-neighbour (among equal areas
    the smallest label), `rounds` (1 .. 8) times with the components formed anew.  A small component without a kept neighbour
    keeps its label, or becomes orphan_fill after the last round.  skip_label and orphan_fill are in 0 .. 255 for uint8 labels
    and 0 .. 65535 for int16 labels.  cleaned: flat, of the labels' dtype and size (a new tensor unless given; it may not overlap
    `labels`); only the pixels of the table's images are written.  max_side: the largest h or w of the table (defaults to the
    limit).  No host synchronisation.  -> cleaned."""
    L.require_cuda(table, labels, cleaned)
    _check_image_table("seg_sieve", table, SEG_CC_COLS, "seg_components_table")
    wide = _seg_label_width("seg_sieve", labels)
    if cleaned is None:
        cleaned = torch.zeros_like(labels)
    if cleaned.dtype != labels.dtype or not cleaned.is_contiguous():
        raise ValueError(f"seg_sieve: cleaned is a contiguous {labels.dtype} tensor, as labels")
    B = table.shape[0]
    lib = L.load()
    ws_bytes = (lib.segclip_seg_sieve_wide_ws_bytes if wide else lib.segclip_seg_sieve_ws_bytes)(labels.numel(), B, int(n_blocks))
    ws = _workspace("seg_sieve", ws_bytes, labels.device, 16)
    L.check((lib.segclip_seg_sieve_wide if wide else lib.segclip_seg_sieve)(
        L.ptr(table), B, int(n_blocks), _max_side(max_side), L.ptr(labels), labels.numel(),
        int(connectivity), -1 if skip_label is None else int(skip_label), int(min_area),
        -1 if orphan_fill is None else int(orphan_fill), int(rounds), L.ptr(cleaned), cleaned.numel(), L.ptr(ws), ws_bytes,
        L.stream()), "seg_sieve")
    return cleaned


# ---------------------------------------------------------------- superpixels (segment_superpixel.inc)
SEG_SP_TILE = (L.const("SEG_SP_TILE_H"), L.const("SEG_SP_TILE_W"))  # (rows, columns) of one workgroup's tile of segclip_seg_superpixels
SEG_SP_COLS = L.const("SEG_SP_COLS")  # int64 columns of one row of its image table
SEG_SP_MIN_STEP = L.const("SEG_SP_MIN_STEP")
SEG_SP_MAX_STEP = L.const("SEG_SP_MAX_STEP")
SEG_SP_MAX_COMPACTNESS = L.const("SEG_SP_MAX_COMPACTNESS")
SEG_SP_MAX_ITERS = L.const("SEG_SP_MAX_ITERS")


def _seg_sp_step(what, step):
    if not SEG_SP_MIN_STEP <= int(step) <= SEG_SP_MAX_STEP:
        raise ValueError(f"{what}: step is in {SEG_SP_MIN_STEP} .. {SEG_SP_MAX_STEP}, got {step}")
    return int(step)


def seg_superpixels_table(raws, step, id_offsets=None):
    """The device image table of seg_superpixels: raws [(h, w, 3) uint8 device tensors, pixels contiguous, rows possibly
    strided], step S of the grid, id_offsets [offset of each image's (h, w) ids in the flat id buffer; by default the maps lie
    flat one after the other].  An image has ceil(h / S) * ceil(w / S) centres, numbered through the images.  It holds the
    tensors' addresses: keep `raws` alive while it is in use.
    -> (table (B, 8) int64, n_blocks, largest side, counts [K per image])."""
    S = _seg_sp_step("seg_superpixels", step)
    if len(raws) == 0 or (id_offsets is not None and len(raws) != len(id_offsets)):
        raise ValueError(f"seg_superpixels: {len(raws)} images but {0 if id_offsets is None else len(id_offsets)} id offsets")
    th, tw = SEG_SP_TILE
    tab, counts, off, cen, blk, side = [], [], 0, 0, 0, 0
    for i, (ptr, h, w, row) in enumerate(_seg_pictures("seg_superpixels", raws, "a picture")):
        k = ((h + S - 1) // S) * ((w + S - 1) // S)
        tab.append([ptr, h, w, row, off if id_offsets is None else int(id_offsets[i]), cen, blk, 0])
        counts.append(k)
        off += h * w
        cen += k
        blk += ((h + th - 1) // th) * ((w + tw - 1) // tw)
        side = max(side, h, w)
    return torch.tensor(tab, dtype=torch.int64, device=raws[0].device).view(-1, SEG_SP_COLS), blk, side, counts


def seg_superpixels(table, n_blocks, ids, num_centres, step=16, compactness=10, iters=5, centres=None, max_side=None):
    """Integer SLIC superpixels (segclip_seg_superpixels; the definition stands in include/segclip_hip.h): the table of
    seg_superpixels_table -> the flat int32 `ids`, a pixel's id the index of its centre inside its image.  num_centres: the sum
    of the table's counts.  step 4 .. 64, compactness 1 .. 64, iters 0 .. 16.  centres: optional (num_centres, 5) int32, the
    final (y, x, r, g, b) of every centre.  No connectivity pass (seg_components gives the connected parts of an id map).
    max_side: the largest h or w of the table (defaults to the limit).  No host synchronisation.  -> ids."""
    L.require_cuda(table, ids, centres)
    _check_image_table("seg_superpixels", table, SEG_SP_COLS, "seg_superpixels_table")
    S = _seg_sp_step("seg_superpixels", step)
    if not 1 <= int(compactness) <= SEG_SP_MAX_COMPACTNESS:
        raise ValueError(f"seg_superpixels: compactness is in 1 .. {SEG_SP_MAX_COMPACTNESS}, got {compactness}")
    if not 0 <= int(iters) <= SEG_SP_MAX_ITERS:
        raise ValueError(f"seg_superpixels: iters is in 0 .. {SEG_SP_MAX_ITERS}, got {iters}")
    if ids.dtype != torch.int32 or not ids.is_contiguous():
        raise ValueError("seg_superpixels: ids is a contiguous int32 tensor")
    K = int(num_centres)
    if centres is not None and (centres.dtype != torch.int32 or not centres.is_contiguous() or tuple(centres.shape) != (K, 5)):
        raise ValueError(f"seg_superpixels: centres is a contiguous ({K}, 5) int32 tensor")
    lib = L.load()
    ws_bytes = lib.segclip_seg_superpixels_ws_bytes(K)
    ws = _workspace("seg_superpixels", ws_bytes, ids.device, 16)
    L.check(lib.segclip_seg_superpixels(L.ptr(table), table.shape[0], int(n_blocks), _max_side(max_side), S, int(compactness),
                                        int(iters), L.ptr(ids), ids.numel(), K, L.ptr(centres), L.ptr(ws), ws_bytes, L.stream()),
            "seg_superpixels")
    return ids


# ---------------------------------------------------------------- majority voting inside segments (segment_vote.inc)
SEG_VOTE_TILE = L.const("SEG_VOTE_TILE")  # pixels of one workgroup of segclip_seg_vote
SEG_VOTE_COLS = L.const("SEG_VOTE_COLS")  # int64 columns of one row of its image table
SEG_VOTE_MAX_SEGMENTS = L.const("SEG_VOTE_MAX_SEGMENTS")  # segments of one image


def seg_vote_table(sizes, offsets, counts, device):
    """The device image table of seg_vote: sizes [(h, w)], offsets [offset of each image's h * w entries in the flat label
    buffer; the segment ids and the output take the same offsets], counts [K per image: its segment ids are 0 .. K - 1]
    -> (table (B, 8) int64, n_blocks, num_segments = the sum of the counts, the largest count)."""
    if len(sizes) == 0 or len(sizes) != len(offsets) or len(sizes) != len(counts):
        raise ValueError(f"seg_vote: {len(sizes)} sizes but {len(offsets)} offsets and {len(counts)} segment counts")
    tab, seg, blk = [], 0, 0
    for (h, w), off, k in zip(sizes, offsets, counts):
        h, w, k = int(h), int(w), int(k)
        if min(h, w) < 1 or max(h, w) >= SEG_SOURCE_LIMIT:
            raise ValueError(f"seg_vote: sizes 1 .. {SEG_SOURCE_LIMIT - 1} supported, got {h}x{w}")
        if not 1 <= k <= SEG_VOTE_MAX_SEGMENTS:
            raise ValueError(f"seg_vote: 1 .. {SEG_VOTE_MAX_SEGMENTS} segments per image supported, got {k}")
        tab.append([int(off), h * w, seg, k, blk, 0, 0, 0])
        seg += k
        blk += (h * w + SEG_VOTE_TILE - 1) // SEG_VOTE_TILE
    return torch.tensor(tab, dtype=torch.int64, device=device).view(-1, SEG_VOTE_COLS), blk, seg, max(int(k) for k in counts)


def seg_vote(table, n_blocks, labels, segments, num_segments, num_classes, min_share=0, out=None, max_count=None):
    """Majority voting inside segments (segclip_seg_vote / segclip_seg_vote_wide by the labels' dtype; the definition stands in
    include/segclip_hip.h): under the table of seg_vote_table, every pixel whose label is below num_classes and whose int32
    segment id lies in its image's 0 .. K - 1 takes the most frequent label of its segment (among equal counts the smallest),
    provided that label holds at least min_share percent of the segment's voters; every other pixel keeps its value.  labels:
    flat uint8, or int16 read as unsigned 16-bit values (up to SEG_WIDE_MAX_CLASSES classes); segments: flat int32 of the same
    size.  out: flat, of the labels' dtype and size (a new tensor unless given; it may not overlap `labels`); only the pixels of
    the table's images are written.  max_count: the largest K of the table (defaults to the limit).  No host synchronisation.
    -> out."""
    L.require_cuda(table, labels, segments, out)
    _check_image_table("seg_vote", table, SEG_VOTE_COLS, "seg_vote_table")
    wide = _seg_label_width("seg_vote", labels)
    if segments.dtype != torch.int32 or not segments.is_contiguous() or segments.numel() != labels.numel():
        raise ValueError("seg_vote: segments is a contiguous int32 tensor with one entry per label")
    if not 0 <= int(min_share) <= 100:
        raise ValueError(f"seg_vote: min_share is a percentage in 0 .. 100, got {min_share}")
    if out is None:
        out = torch.zeros_like(labels)
    if out.dtype != labels.dtype or not out.is_contiguous():
        raise ValueError(f"seg_vote: out is a contiguous {labels.dtype} tensor, as labels")
    lib = L.load()
    K, C = int(num_segments), int(num_classes)
    ws_bytes = lib.segclip_seg_vote_ws_bytes(K, C)
    ws = _workspace("seg_vote", ws_bytes, labels.device, 16)
    L.check((lib.segclip_seg_vote_wide if wide else lib.segclip_seg_vote)(
        L.ptr(table), table.shape[0], int(n_blocks), SEG_VOTE_MAX_SEGMENTS if max_count is None else int(max_count), L.ptr(labels),
        labels.numel(), L.ptr(segments), segments.numel(), K, C, int(min_share), L.ptr(out), out.numel(), L.ptr(ws), ws_bytes,
        L.stream()), "seg_vote")
    return out


# ---------------------------------------------------------------- boundary bands and areas (segment_boundary.inc)
# (rows, columns) of one wave's strip of segclip_seg_boundary; the columns are also its rows pass's chunk
SEG_BOUNDARY_TILE = (L.const("SEG_BOUNDARY_TILE_H"), L.const("SEG_BOUNDARY_TILE_W"))
SEG_BOUNDARY_WAVES = L.const("SEG_BOUNDARY_WAVES")  # consecutive strips of a map that share a workgroup
SEG_BOUNDARY_COLS = L.const("SEG_BOUNDARY_COLS")  # int64 columns of one row of its image table
SEG_BOUNDARY_MAX_RADIUS = L.const("SEG_BOUNDARY_MAX_RADIUS")


def seg_boundary_table(sizes, pred_offsets, gt_offsets, radii, device):
    """The device image table of seg_boundary: sizes [(h, w)], pred_offsets [offset of each map's h * w bytes in the flat
    prediction buffer and in pred_band], gt_offsets [the same for the ground truths and gt_band; None: no map has one, a single
    None or -1: that map has none], radii [d of each map] -> (table (B, 8) int64, n_blocks, largest side)."""
    n = len(sizes)
    if n == 0:
        raise ValueError("seg_boundary: sizes is empty")
    if gt_offsets is None:
        gt_offsets = [-1] * n
    for name, v in (("pred_offsets", pred_offsets), ("gt_offsets", gt_offsets), ("radii", radii)):
        if len(v) != n:
            raise ValueError(f"seg_boundary: {n} sizes but {name} has {len(v)} entries")
    sh, tw = SEG_BOUNDARY_TILE
    tab, blk, side = [], 0, 0
    for i, ((h, w), po, go, d) in enumerate(zip(sizes, pred_offsets, gt_offsets, radii)):
        h, w, d = int(h), int(w), int(d)
        go = -1 if go is None else int(go)
        if min(h, w) < 1 or max(h, w) >= SEG_SOURCE_LIMIT:
            raise ValueError(f"seg_boundary: sizes 1 .. {SEG_SOURCE_LIMIT - 1} supported, map {i} is {h}x{w}")
        if not 1 <= d <= SEG_BOUNDARY_MAX_RADIUS:
            raise ValueError(f"seg_boundary: radii 1 .. {SEG_BOUNDARY_MAX_RADIUS} supported, map {i} ({h}x{w}) has radius {d}")
        if int(po) < 0:
            raise ValueError(f"seg_boundary: pred_offsets are not negative, map {i} has {po}")
        if go < -1:
            raise ValueError(f"seg_boundary: gt_offsets are not negative (-1 or None: no ground truth), map {i} has {go}")
        tab.append([h, w, int(po), go, d, blk, 0, 0])
        strips = ((h + sh - 1) // sh) * ((w + tw - 1) // tw)
        blk += (strips + SEG_BOUNDARY_WAVES - 1) // SEG_BOUNDARY_WAVES
        side = max(side, h, w)
    # through pinned memory: SegEvaluator.update_maps scores without waiting for the device
    return _upload_table(tab, torch.int64, device).view(-1, SEG_BOUNDARY_COLS), blk, side


def seg_boundary(table, n_blocks, pred, gt=None, num_classes=1, ignore_index=255, reduce_zero_label=False, pred_band=None,
                 gt_band=None, areas=None, max_side=None):
    """Boundary bands and boundary areas of the flat `pred` (and `gt`) under the table of seg_boundary_table (the definition
    stands in include/segclip_hip.h).  pred and gt are both uint8 (segclip_seg_boundary, at most 256 classes) or both int16
    (segclip_seg_boundary_wide: 16-bit label maps read as unsigned, at most 1024 classes, ignore_index 0 .. 65535).  Every output
    is optional and written where given: pred_band / gt_band flat uint8, whatever the labels' dtype, with one byte per element of
    pred / gt (bit 0: a label change within the radius, bit 1: the window leaves the map), areas (2, 3, C) int64 that is ADDED to
    (slot 0 Boundary IoU, slot 1 trimap; needs gt).  max_side: the largest h or w of the table (defaults to the limit).  No host
    synchronisation.  -> None."""
    L.require_cuda(table, pred, gt, pred_band, gt_band, areas)
    _check_image_table("seg_boundary", table, SEG_BOUNDARY_COLS, "seg_boundary_table")
    wide = _seg_label_width("seg_boundary", pred, "pred")
    if gt is not None and (gt.dtype not in (torch.uint8, torch.int16) or not gt.is_contiguous()):
        raise ValueError("seg_boundary: gt is a contiguous uint8 or int16 tensor")
    if gt is not None and gt.dtype != pred.dtype:
        raise ValueError("seg_boundary: pred and gt are both uint8 or both int16 tensors")
    for name, t in (("pred_band", pred_band), ("gt_band", gt_band)):
        if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous()):
            raise ValueError(f"seg_boundary: {name} is a contiguous uint8 tensor")
    if pred_band is not None and pred_band.numel() != pred.numel():
        raise ValueError(f"seg_boundary: pred_band has the layout of pred: {pred.numel()} bytes, got {pred_band.numel()}")
    if gt is None and (gt_band is not None or areas is not None):
        raise ValueError("seg_boundary: gt_band and areas need gt")
    if gt_band is not None and gt_band.numel() != gt.numel():
        raise ValueError(f"seg_boundary: gt_band has the layout of gt: {gt.numel()} bytes, got {gt_band.numel()}")
    num_classes = int(num_classes)
    if num_classes < 1:
        raise ValueError(f"seg_boundary: num_classes is positive, got {num_classes}")
    if areas is not None and (areas.dtype != torch.int64 or not areas.is_contiguous() or tuple(areas.shape) != (2, 3, num_classes)):
        raise ValueError(f"seg_boundary: areas is a contiguous (2, 3, {num_classes}) int64 tensor")
    lib = L.load()
    gt_bytes = gt.numel() if gt is not None else 0
    ws_bytes = lib.segclip_seg_boundary_ws_bytes(pred.numel(), gt_bytes)
    ws = _workspace("seg_boundary", ws_bytes, pred.device, 16)
    L.check((lib.segclip_seg_boundary_wide if wide else lib.segclip_seg_boundary)(
        L.ptr(table), table.shape[0], int(n_blocks), _max_side(max_side), L.ptr(pred),
        pred.numel(), L.ptr(gt), gt_bytes, num_classes, int(ignore_index), int(bool(reduce_zero_label)), L.ptr(pred_band),
        L.ptr(gt_band), L.ptr(areas), L.ptr(ws), ws_bytes, L.stream()), "seg_boundary")


# ---------------------------------------------------------------- image-text retrieval evaluation (retrieval.hip)
RETRIEVAL_BAD_INDEX = L.const("RETRIEVAL_BAD_INDEX")  # status bit of segclip_retrieval_thresholds: an image index outside [0, Ni)


def _retrieval_inputs(what, visual, sequence, image_index):
    L.require_cuda(visual, sequence, image_index)
    if visual.dtype != torch.float32 or sequence.dtype != torch.float32 or image_index.dtype != torch.int32:
        raise TypeError(f"{what}: fp32 visual and sequence embeddings, int32 image_index")
    if visual.dim() != 2 or sequence.dim() != 2 or visual.shape[1] != sequence.shape[1] \
            or tuple(image_index.shape) != (sequence.shape[0],):
        raise ValueError(f"{what}: visual (Ni, E), sequence (Nt, E), image_index (Nt,); got {tuple(visual.shape)}, "
                         f"{tuple(sequence.shape)}, {tuple(image_index.shape)}")
    return visual.contiguous(), sequence.contiguous(), image_index.contiguous()


def retrieval_thresholds(visual, sequence, image_index, status):
    """segclip_retrieval_thresholds: -> (thr_t (Nt,) fp32 = <sequence[t], visual[image_index[t]]>, best (Ni,) fp32 = the
    maximum of thr_t over an image's captions, n_cap (Ni,) int32 = its captions).  status: (1,) int32, OR-ed into on the
    device (RETRIEVAL_BAD_INDEX)."""
    V, T, g = _retrieval_inputs("retrieval_thresholds", visual, sequence, image_index)
    L.require_cuda(status)
    if status.dtype != torch.int32 or status.numel() != 1:
        raise ValueError("retrieval_thresholds: status is a (1,) int32 tensor")
    (Ni, E), Nt = V.shape, T.shape[0]
    thr, best, n_cap = _empty((Nt,), torch.float32, V), _empty((Ni,), torch.float32, V), _empty((Ni,), torch.int32, V)
    L.check(L.load().segclip_retrieval_thresholds(L.ptr(V), L.ptr(T), L.ptr(g), Ni, Nt, E, L.ptr(thr), L.ptr(best), L.ptr(n_cap),
                                                  L.ptr(status), L.stream()), "retrieval_thresholds")
    return thr, best, n_cap


def retrieval_count(visual, sequence, image_index, thr_t, best):
    """segclip_retrieval_count: the tiled compare-and-count pass -> (rank_t2i (Nt,), rank_i2t (Ni,)) int32.  No (Nt, Ni)
    array exists; an image without captions has rank 0 here and -1 after retrieval_hist."""
    V, T, g = _retrieval_inputs("retrieval_count", visual, sequence, image_index)
    L.require_cuda(thr_t, best)
    (Ni, E), Nt = V.shape, T.shape[0]
    if thr_t.dtype != torch.float32 or best.dtype != torch.float32 or not thr_t.is_contiguous() or not best.is_contiguous() \
            or tuple(thr_t.shape) != (Nt,) or tuple(best.shape) != (Ni,):
        raise ValueError("retrieval_count: thr_t (Nt,) and best (Ni,) are the contiguous fp32 outputs of retrieval_thresholds")
    rank_t2i = torch.zeros(Nt, dtype=torch.int32, device=V.device)
    rank_i2t = torch.zeros(Ni, dtype=torch.int32, device=V.device)
    L.check(L.load().segclip_retrieval_count(L.ptr(V), L.ptr(T), L.ptr(g), L.ptr(thr_t), L.ptr(best), Ni, Nt, E, L.ptr(rank_t2i),
                                             L.ptr(rank_i2t), L.stream()), "retrieval_count")
    return rank_t2i, rank_i2t


def retrieval_hist(rank_t2i, rank_i2t, n_cap):
    """segclip_retrieval_hist: -> (hist_t2i (Ni,), hist_i2t (Nt + 1,)) int64, the number of captions / of images with captions
    at every rank; rank_i2t becomes -1 in place where n_cap is 0."""
    L.require_cuda(rank_t2i, rank_i2t, n_cap)
    for name, t in (("rank_t2i", rank_t2i), ("rank_i2t", rank_i2t), ("n_cap", n_cap)):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"retrieval_hist: {name} is a contiguous one-dimensional int32 tensor")
    Nt, Ni = rank_t2i.shape[0], rank_i2t.shape[0]
    if n_cap.shape[0] != Ni:
        raise ValueError(f"retrieval_hist: n_cap has {n_cap.shape[0]} entries for {Ni} images")
    hist_t2i = torch.zeros(Ni, dtype=torch.int64, device=rank_t2i.device)
    hist_i2t = torch.zeros(Nt + 1, dtype=torch.int64, device=rank_t2i.device)
    L.check(L.load().segclip_retrieval_hist(L.ptr(rank_t2i), L.ptr(rank_i2t), L.ptr(n_cap), Ni, Nt, L.ptr(hist_t2i),
                                            L.ptr(hist_i2t), L.stream()), "retrieval_hist")
    return hist_t2i, hist_i2t


def retrieval_topk(queries, gallery, k, splits=0):
    """segclip_retrieval_topk: queries (Nq, E), gallery (Nx, E), contiguous fp32 -> (idx (Nq, k) int32, val (Nq, k) fp32): per
    query the first min(k, Nx) gallery rows under "higher <q, x> first, equal scores: lower index first" with their scores,
    then idx = -1, val = -inf.  No (Nq, Nx) array exists and nothing synchronises.  splits = 0 lets the library choose the
    number of partial lists; a test passes another value to hold every partition to one result, nothing else should."""
    L.require_cuda(queries, gallery)
    if queries.dtype != torch.float32 or gallery.dtype != torch.float32:
        raise TypeError(f"retrieval_topk: fp32 queries and gallery, got {queries.dtype} and {gallery.dtype}")
    if queries.dim() != 2 or gallery.dim() != 2 or queries.shape[1] != gallery.shape[1]:
        raise ValueError(f"retrieval_topk: queries (Nq, E) and gallery (Nx, E) of equal E; got {tuple(queries.shape)}, "
                         f"{tuple(gallery.shape)}")
    if not queries.is_contiguous() or not gallery.is_contiguous():
        raise ValueError("retrieval_topk: queries and gallery are contiguous")
    (Nq, E), Nx, k, splits = queries.shape, gallery.shape[0], int(k), int(splits)
    lib = L.load()
    ws_bytes = lib.segclip_retrieval_topk_ws_bytes(Nq, Nx, k, splits)
    if ws_bytes < 0:
        L.check(ws_bytes, "retrieval_topk")
    idx, val = _empty((Nq, k), torch.int32, queries), _empty((Nq, k), torch.float32, queries)
    ws = _empty((ws_bytes // 8,), torch.int64, queries) if ws_bytes else None
    L.check(lib.segclip_retrieval_topk(L.ptr(queries), L.ptr(gallery), Nq, Nx, E, k, splits, L.ptr(idx), L.ptr(val), L.ptr(ws),
                                       ws_bytes, L.stream()), "retrieval_topk")
    return idx, val


# ---------------------------------------------------------------- front end of training (train_frontend.inc)
TRAIN_SOURCE_COLS = L.const("TRAIN_SOURCE_COLS")  # int64 columns of one row of the source table of segclip_train_images_from_u8
TRAIN_MAP_COLS = L.const("TRAIN_MAP_COLS")  # int64 columns of one row of the map table of segclip_train_patch_labels
TRAIN_MAX_SCALE = L.const("TRAIN_MAX_SCALE")  # crop side / resized side, per axis (33 filter taps)
TRAIN_MAX_OUT_W = L.const("TRAIN_MAX_OUT_W")


def train_source_table(raws, geometry, out_size):
    """The device source table of train_images_from_u8: raws [(h, w, 3) uint8 device tensors, pixels contiguous, rows possibly
    strided], geometry [(x0, y0, bw, bh, RW, RH, ox, oy, flags)] per image - the crop box, the size it is resized to, the
    offset of the out_size = (out_h, out_w) window in the resized image, flags bit 0 / 1 = horizontal / vertical flip of the
    window -> (B, 13) int64.  Everything the device would refuse raises here.  It holds the tensors' addresses: keep `raws`
    alive while it is in use."""
    if len(raws) == 0 or len(raws) != len(geometry):
        raise ValueError(f"train_source_table: {len(raws)} images but {len(geometry)} geometry rows")
    L.require_cuda(*raws)
    oh, ow = int(out_size[0]), int(out_size[1])
    if oh < 1 or ow < 1 or oh >= SEG_SOURCE_LIMIT or ow > TRAIN_MAX_OUT_W:
        raise ValueError(f"train_images_from_u8: an output of 1 .. {SEG_SOURCE_LIMIT - 1} rows and 1 .. {TRAIN_MAX_OUT_W} columns, "
                         f"got {oh}x{ow}")
    tab = []
    for t, g in zip(raws, geometry):
        if t.dtype != torch.uint8:
            raise TypeError(f"train_images_from_u8: a source image is uint8, got {t.dtype}")
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"train_images_from_u8: a source image is (h, w, 3), got {tuple(t.shape)}")
        h, w = int(t.shape[0]), int(t.shape[1])
        if t.device != raws[0].device:
            raise ValueError("train_images_from_u8: the source images are on different devices")
        if len(g) != 9:
            raise ValueError("train_images_from_u8: a geometry row is (x0, y0, bw, bh, RW, RH, ox, oy, flags)")
        x0, y0, bw, bh, RW, RH, ox, oy, flags = (int(v) for v in g)
        if min(h, w, RW, RH) < 1 or max(h, w, RW, RH) >= SEG_SOURCE_LIMIT:
            raise ValueError(f"train_images_from_u8: sizes 1 .. {SEG_SOURCE_LIMIT - 1} supported, got {h}x{w} -> {RH}x{RW}")
        if t.stride(2) != 1 or t.stride(1) != 3 or (h > 1 and t.stride(0) < 3 * w):
            raise ValueError(f"train_images_from_u8: a source image has interleaved channels and contiguous pixels (strides "
                             f"(>= 3 w, 3, 1)), got {tuple(t.stride())}")
        if x0 < 0 or y0 < 0 or bw < 1 or bh < 1 or x0 + bw > w or y0 + bh > h:
            raise ValueError(f"train_images_from_u8: the box (x0, y0, bw, bh) = {(x0, y0, bw, bh)} is not inside the {h}x{w} image")
        if ox < 0 or oy < 0 or ox + ow > RW or oy + oh > RH:
            raise ValueError(f"train_images_from_u8: the {oh}x{ow} window at (ox, oy) = {(ox, oy)} is not inside the resized "
                             f"{RH}x{RW} image")
        if bw > TRAIN_MAX_SCALE * RW or bh > TRAIN_MAX_SCALE * RH:
            raise ValueError(f"train_images_from_u8: a crop of {bh}x{bw} to {RH}x{RW} shrinks more than {TRAIN_MAX_SCALE} times")
        if not 0 <= flags <= 3:
            raise ValueError(f"train_images_from_u8: flags are 0 .. 3, got {flags}")
        tab.append([t.data_ptr(), h, w, max(int(t.stride(0)), 3 * w), x0, y0, bw, bh, RW, RH, ox, oy, flags])
    return torch.tensor(tab, dtype=torch.int64, device=raws[0].device).view(-1, TRAIN_SOURCE_COLS)


def train_images_from_u8(raws, geometry, out_size, lut, out=None, table=None):
    """The training front end (segclip_train_images_from_u8): decoded uint8 images -> (B, 3, out_h, out_w) fp32, each the
    out_size window of Pillow's BICUBIC resize of its crop, looked up in `lut` (256, 3) fp32 - bit for bit
    Image.crop(box).resize((RW, RH), Image.BICUBIC), ToTensor and Normalize.  One launch.  table: train_source_table(raws,
    geometry, out_size) when the caller built it already; the device zero-fills an image whose row it refuses.  Crops more
    than 8 times the resized side are not supported and raise."""
    if table is None:
        table = train_source_table(raws, geometry, out_size)
    elif table.dtype != torch.int64 or tuple(table.shape) != (len(raws), TRAIN_SOURCE_COLS) or not table.is_contiguous():
        raise ValueError("train_images_from_u8: table is the (B, 13) int64 tensor of train_source_table")
    L.require_cuda(table, lut, out)
    oh, ow = int(out_size[0]), int(out_size[1])
    if lut.dtype != torch.float32 or tuple(lut.shape) != (256, 3) or not lut.is_contiguous():
        raise ValueError("train_images_from_u8: lut is a contiguous (256, 3) fp32 tensor")
    B = table.shape[0]
    if out is None:
        out = torch.empty(B, 3, oh, ow, dtype=torch.float32, device=table.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * 3 * oh * ow:
        raise ValueError("train_images_from_u8: out is a contiguous fp32 tensor of B * 3 * out_h * out_w elements")
    L.check(L.load().segclip_train_images_from_u8(L.ptr(table), B, oh, ow, L.ptr(lut), L.ptr(out), L.stream()),
            "train_images_from_u8")
    return out


def train_patch_labels(seg_maps, boxes, size, patch, out=None, table=None):
    """The patch labels of a batch (segclip_train_patch_labels): seg_maps [(h, w) int32 device tensors, rows possibly strided],
    boxes [(x0, y0, x1, y1, flags)] per map - a box thinner than 2 takes the whole map, flags bit 0 / 1 = horizontal /
    vertical flip of the crop -> (B, 1, size / patch, size / patch) int64, bit for bit get_felzenszwalb_from_cache.  One
    launch.  A map with a negative label among the pixels read gives a row of -1."""
    size, patch = int(size), int(patch)
    if size < 1 or size >= SEG_SOURCE_LIMIT or patch < 1 or size % patch != 0:
        raise ValueError(f"train_patch_labels: size 1 .. {SEG_SOURCE_LIMIT - 1}, a multiple of patch; got {size} / {patch}")
    if table is None:
        if len(seg_maps) == 0 or len(seg_maps) != len(boxes):
            raise ValueError(f"train_patch_labels: {len(seg_maps)} maps but {len(boxes)} boxes")
        L.require_cuda(*seg_maps)
        tab = []
        for t, bx in zip(seg_maps, boxes):
            if t.dtype != torch.int32:
                raise TypeError(f"train_patch_labels: a segment map is int32, got {t.dtype}")
            if t.dim() != 2:
                raise ValueError(f"train_patch_labels: a segment map is (h, w), got {tuple(t.shape)}")
            h, w = int(t.shape[0]), int(t.shape[1])
            if t.device != seg_maps[0].device:
                raise ValueError("train_patch_labels: the segment maps are on different devices")
            if min(h, w) < 1 or max(h, w) >= SEG_SOURCE_LIMIT:
                raise ValueError(f"train_patch_labels: sizes 1 .. {SEG_SOURCE_LIMIT - 1} supported, got {h}x{w}")
            if t.stride(1) != 1 or (h > 1 and t.stride(0) < w):
                raise ValueError(f"train_patch_labels: a segment map has contiguous rows (strides (>= w, 1)), got {tuple(t.stride())}")
            x0, y0, x1, y1, flags = (int(v) for v in bx)
            whole = x1 - x0 < 2 or y1 - y0 < 2
            if not whole and (x0 < 0 or y0 < 0 or x1 > w or y1 > h):
                raise ValueError(f"train_patch_labels: the box {(x0, y0, x1, y1)} is not inside the {h}x{w} map")
            if not 0 <= flags <= 3:
                raise ValueError(f"train_patch_labels: flags are 0 .. 3, got {flags}")
            tab.append([t.data_ptr(), h, w, 4 * max(int(t.stride(0)), w), x0, y0, x1, y1, flags])
        table = torch.tensor(tab, dtype=torch.int64, device=seg_maps[0].device).view(-1, TRAIN_MAP_COLS)
    elif table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != TRAIN_MAP_COLS or not table.is_contiguous():
        raise ValueError("train_patch_labels: table is a (B, 9) int64 tensor")
    L.require_cuda(table, out)
    B, P = table.shape[0], size // patch
    if out is None:
        out = torch.empty(B, 1, P, P, dtype=torch.int64, device=table.device)
    elif out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != B * P * P:
        raise ValueError("train_patch_labels: out is a contiguous int64 tensor of B * (size / patch)^2 elements")
    L.check(L.load().segclip_train_patch_labels(L.ptr(table), B, size, patch, L.ptr(out), L.stream()), "train_patch_labels")
    return out
