"""GPU: every kernel instance of the learnable-center stage - csrc/group_linear.hip, csrc/center.hip and assign_fwd / assign_bwd of
csrc/misc.hip - reached by a row of the tables below and checked against fp64 torch on exactly the values the kernel reads
(bf16 operands are rounded first and then widened).  All kernel calls go through the C ABI (segclip_amd._lib), the test owns
every buffer.

Per row: (1) every output is a view inside a larger NaN buffer (64 guard words before, two guard rows + 64 words after; for the
grouped linear the pitch columns beyond groups * 64 of every row as well; 0xAB for the uint8 center index): the guards survive
and everything inside becomes finite; (2) the inputs sit in frames of the same kind, NaN in their pitch, in the rows after M and
in the guards; (3) the same call a second time into the same frames is bit-identical, frames included; (4) the values against
fp64 with the bound of tests/helpers.check, |err| <= rtol * (|ref| + rms(ref)); (5) the same bound REJECTS the fp64 reference
after a small defect (listed per family below).  Inputs are drawn on the host from seeded generators.

Instances (a pure function of the shape: instance_of() below restates the dispatchers) and the rows that reach them:
  group_linear_kernel<1,1> | <1,2> | <2,1>: gl11_* | gl12_* | gl21_* - each with M in 1 31 32 33 127 129 1000 (partial 32-row wave
      block, partial 128-row workgroup, the row clamp), groups in 1 7 12 13 16 (7: two empty blockIdx.y shares of the six; 13: a
      last share of one group), pitched (ld_in = D + 8, ld_out = D + 24) and contiguous; GroupLinearPairFn end to end (k, v, dx and
      both weight gradients) on a pitched input: test_group_linear_pair_end_to_end
  segmean_fwd_fast / segmean_bwd_fast <fp32 | bf16, 768 | 1024>: smf_* with T in 1 2 3 (the `wave < T` prefetch guard) 5 49 196,
      and smf_limit (B = 1, D = 768, T = 1874: exactly 60000 bytes of LDS in the backward)
  segmean_fwd_kernel / segmean_bwd_kernel <fp32 | bf16> (generic): smg_* with G in 3 5 8, D in 4 64 772 1024 (772: a last 256-column
      group of one lane; G = 5 at D = 1024 must be generic), T in 1 7 50
      all segment-mean rows: one center empty in every sample, sample 0 with every token on one center, counts = bincount(idx)
  center_logits_fwd<3 | 4>: cl_* - token ranges over blockIdx.y: 9 x 64 (B 2, T 576), 12 x 61 + 52 (B 16, T 784), one (B 3, T 48),
      no split (B 130, T 5); T in 1 3; cl_fwd_lds_max (B 128, T 1875, D 768: 60000 bytes of LDS, forward only)
  center_logits_bwd<3 | 4>: the same rows, and its limits cl_bwd_limit_768 (T 1232) and cl_bwd_limit_1024 (T 976)
  recon_mix_fwd: rm_* - one token segment (M 1 63) against four (M 64, ragged: 65 197), one or several 64-lane column chunks
  recon_mix_bwd: rm_* - D 4 40 (part of one wave), 260 (65 lanes: a second, partly live wave), 768 1024 2048, 4096 (16 waves)
  assign_fwd / assign_bwd: as_* - G in 3 5 8, T in 1 7 577 with B * T = 257, 259, 1731 (a last thread block partly live), training
      (Gumbel noise, tau 0.9) and evaluation; the evaluation rows hold a token with two equal largest logits and a token with all
      G equal (the lowest index wins, as torch.max).  The inputs are made decisive on the host (top two of z less than 1e-3 apart:
      the larger is raised by 1e-2), so idx, hard and counts are compared bit-exactly at EVERY token.
  gates (test_gate_*): ops.center_logits, ops.recon_mix, _group_linear_pair and the module's _segment_mean on both sides of every
      limit, forward and backward, asserting the path taken (grad_fn) and the same bounds.

Defects the bound must reject (5):
  grouped linear: the last group multiplied by the previous group's weight block; row M - 1 replaced by row M - 2 (the clamp);
      for <2,1> the second input dropped
  segment mean: the last token left out of `out`; one token moved to the neighbouring center (out, dv); the clamp removed on the
      empty center (dhard); the normaliser term dc dropped (dhard)
  assignment logits: the last token of the last token range replaced by its neighbour; the last four columns of D zeroed
  recon mix: center 7 dropped; row m = M - 1 replaced by its neighbour
  assignment: token n replaced by token n - 1 (y_soft, soft, dlogits); the row-dot term of the softmax backward dropped (dlogits)

Bounds.
  bf16 outputs (grouped linear; dv of the segment mean with bf16 v): derived, not measured.  The operands are exact bf16, the
      products are exact in fp32 and the sum over K = 64 or 128 is held in fp32 (2^-24 per step, invisible next to the output
      rounding); the only rounding that counts is the output's to bf16, half an ulp = 2^-9 relative.  rtol = 2^-8: the factor 2
      is the margin tests/test_attn_routes_gpu.py takes over its emulated floor.  (dv is a copy of dout / max(count, 1): 2^-9.)
  fp32 outputs: floor = torch float32 of the same expression (the *_expr functions below, on the device) against fp64, in check()
      units |err| / (|ref| + rms(ref)), the maximum over the rows of a kernel; bound = 4 x floor rounded up to one digit (the 4
      covers another summation order over up to 1024 columns or 1875 tokens).  The floor never involves the kernel.
      Measured on an MI355X by floors() below (FLOORS holds the figures, RT is computed from them):
                        floor   -> bound                          floor   -> bound                          floor   -> bound
        segmean out   2.913e-6 -> 2e-5       logits attn        1.630e-6 -> 7e-6       recon out          2.931e-7 -> 2e-6
        segmean dv    4.452e-8 -> 2e-7       logits dq          1.496e-6 -> 6e-6       recon da           1.820e-6 -> 8e-6
        segmean dhard 1.802e-6 -> 8e-6       logits dk          4.503e-7 -> 2e-6       recon dx           6.746e-7 -> 3e-6
        assign y_soft 6.269e-7 -> 3e-6       assign soft        2.097e-7 -> 9e-7       assign dlogits     5.105e-6 -> 3e-5
        weight gradients of GroupLinearPairFn (fp32 results of exact bf16 products over M = 129 rows): 3.189e-7 -> 2e-6
      (segmean dv in fp32 is a copy of dout / max(count, 1): one division.  The largest floors come from smf_limit (out: a sum
      over up to 1874 tokens), cl_fwd_lds_max and cl_13x61 (attn, dq), rm_m65_d4096 (da) and as_g8_t577_train.)

Fixes that came with this file:
  - ops.center_logits chose the token-loop forward by the forward's LDS limit alone (T <= 1875) and the backward then raised
    SEGCLIP_ERR_UNSUPPORTED above T = 1232 (D 768) / 976 (D 1024): gate rows T = 977, 1233, 1875.
  - SemanticLearnerModule ran SegMeanFn whenever G <= 8 and D <= 1024; the backward refuses T > 1874 and D % 4 != 0:
    gate rows T = 1875 and D = 770.
  - GroupLinearFn addressed its input as dense rows whatever its pitch, and GroupLinearPairFn's weight gradients likewise (the
    data path of the fused kernel used the pitch): test_gate_group_linear_pair[pitch_not_8] and
    test_group_linear_pair_end_to_end.
"""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from segclip_amd import _lib as L  # noqa: E402
from segclip_amd import ops  # noqa: E402
from segclip_amd.modules import module_seg_vit as msv  # noqa: E402
from tests.kernel_frames import BF, DEV, F32, F64, Bounds, Frame, draw, lib_call, put, run_twice, seeded  # noqa: E402

TAU = 0.9
TAU32 = float(torch.tensor(TAU, dtype=F32))     # the value the kernel receives through its `float tau`

RT_BF = 2.0 ** -8
# floors measured by floors() (torch float32 against fp64 on this file's rows, maximum over the rows of the kernel) ...
FLOORS = {
    "segmean.out": 2.913e-6, "segmean.dv": 4.452e-8, "segmean.dhard": 1.802e-6,
    "logits.attn": 1.630e-6, "logits.dq": 1.496e-6, "logits.dk": 4.503e-7,
    "recon.out": 2.931e-7, "recon.da": 1.820e-6, "recon.dx": 6.746e-7,
    "assign.y_soft": 6.269e-7, "assign.soft": 2.097e-7, "assign.dlogits": 5.105e-6,
    "gl.dw": 3.189e-7,
}

# ... and the bounds: 4 x floor rounded up to one digit (tests/kernel_frames.Bounds); BOUNDS.stats is None while the rows assert,
# floors() sets a dict there and the rows record floors and errors instead
BOUNDS = Bounds(FLOORS)
RT = BOUNDS.rt
judge, rejects = BOUNDS.judge, BOUNDS.rejects


# ---- grouped 64-channel linear ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class GL:
    n_in: int
    n_out: int
    M: int
    groups: int
    pitched: bool

    @property
    def name(self):
        return f"gl{self.n_in}{self.n_out}_m{self.M}_g{self.groups}_{'pitched' if self.pitched else 'dense'}"


_GL_MG = [(1, 7, True), (31, 1, False), (32, 12, True), (33, 13, False), (127, 16, True), (129, 12, False), (1000, 7, True),
          (1000, 13, False)]
GL_CASES = ([GL(1, 1, m, g, p) for m, g, p in _GL_MG] + [GL(1, 2, m, g, not p) for m, g, p in _GL_MG]
            + [GL(2, 1, m, g, p) for m, g, p in _GL_MG])
# (1000 appears twice per instance so that M = 1 does not have to carry groups = 1: that row would have no defect to reject)


def gl_expr(xs, ws, n_out, groups, dt):
    """out_o(m, g*64 + n) = sum_i sum_k in_i(m, g*64 + k) * w[i * n_out + o][g*64 + n][k]"""
    M = xs[0].shape[0]
    outs = []
    for o in range(n_out):
        acc = 0
        for i, x in enumerate(xs):
            acc = acc + torch.einsum("mgk,gnk->mgn", x.to(dt).view(M, groups, 64), ws[i * n_out + o].to(dt).view(groups, 64, 64))
        outs.append(acc.reshape(M, groups * 64))
    return outs


@pytest.mark.parametrize("c", GL_CASES, ids=[c.name for c in GL_CASES])
def test_group_linear(c):
    gen = seeded(c.name)
    D = c.groups * 64
    ld_in, ld_out = (D + 8, D + 24) if c.pitched else (D, D)
    xs = [draw(gen, c.M, D, dtype=BF) for _ in range(c.n_in)]
    ws = [draw(gen, D, 64, dtype=BF, scale=0.125) for _ in range(c.n_in * c.n_out)]
    fx, fw = [put(x, ld_in) for x in xs], [put(w) for w in ws]
    fo = [Frame((c.M, D), BF, ld_out) for _ in range(c.n_out)]
    run_twice(c.name, lambda: msv._gl64([f.v for f in fx], [f.v for f in fo], [f.v for f in fw], c.M, c.groups), fo)
    ref = gl_expr(xs, ws, c.n_out, c.groups, F64)
    for o in range(c.n_out):
        judge("gl", f"{c.name}: out {o}", fo[o].v, ref[o], rtol=RT_BF)
    wrong = {}
    if c.groups >= 2:
        w2 = [w.clone() for w in ws]
        for w in w2:
            w[-64:] = w[-128:-64]
        wrong["the last group with the previous group's weights"] = gl_expr(xs, w2, c.n_out, c.groups, F64)
    if c.M >= 2:
        swapped = [r.clone() for r in ref]
        for r in swapped:
            r[c.M - 1] = r[c.M - 2]
        wrong["row M - 1 replaced by row M - 2"] = swapped
    if c.n_in == 2:
        wrong["the second input dropped"] = gl_expr(xs[:1], ws[:1], 1, c.groups, F64)
    assert wrong
    for what, w in wrong.items():
        for o in range(c.n_out):
            rejects("gl", f"{c.name}: out {o}, {what}", fo[o].v, w[o], rtol=RT_BF)


def pair_reference(x, wk, wv, gk, gv, groups):
    """k, v, the two parts of dx, dWk, dWv in fp64 of the bf16 operands (the weights are cast to bf16 by the op)"""
    D = x.shape[1]
    hd = D // groups
    X, GK, GV = (t.double().view(-1, groups, hd) for t in (x, gk, gv))
    WK, WV = (w.detach().to(BF).double().view(groups, hd, hd) for w in (wk, wv))       # [g][n][k]
    flat = lambda t: t.reshape(-1, D)   # noqa: E731
    return {"k": flat(torch.einsum("mgk,gnk->mgn", X, WK)), "v": flat(torch.einsum("mgk,gnk->mgn", X, WV)),
            "dx_k": flat(torch.einsum("mgn,gnk->mgk", GK, WK)), "dx_v": flat(torch.einsum("mgn,gnk->mgk", GV, WV)),
            "dwk": torch.einsum("mgn,mgk->gnk", GK, X).reshape(D, hd, 1), "dwv": torch.einsum("mgn,mgk->gnk", GV, X).reshape(D, hd, 1)}


def pair_inputs(name, M, D, groups, pitch):
    gen = seeded(name)
    fx = put(draw(gen, M, D, dtype=BF), pitch)
    x = fx.v.detach().requires_grad_()
    hd = D // groups
    wk, wv = (draw(gen, D, hd, 1, scale=hd ** -0.5).requires_grad_() for _ in range(2))
    gk, gv = draw(gen, M, D, dtype=BF), draw(gen, M, D, dtype=BF)
    return fx, x, wk, wv, gk, gv


def dw_expr32(x, gk, groups):
    hd = x.shape[1] // groups
    return torch.einsum("mgn,mgk->gnk", gk.float().view(-1, groups, hd), x.float().view(-1, groups, hd)).reshape(x.shape[1], hd, 1)


def test_group_linear_pair_end_to_end():
    """GroupLinearPairFn on an input with a row pitch of D + 8: <1,2> forward, <2,1> data gradient, the weight gradients through
    the batched GEMM (fp32 results of exact bf16 products: the fp32 bound)"""
    M, D, groups = 129, 768, 12
    fx, x, wk, wv, gk, gv = pair_inputs("pair_e2e", M, D, groups, D + 8)
    k, v = msv._group_linear_pair(x, wk, wv, groups)
    assert type(k.grad_fn).__name__ == "GroupLinearPairFnBackward", "the pitched input must stay on the fused kernel"
    torch.autograd.backward([k, v], [gk, gv])
    torch.cuda.synchronize()
    assert fx.intact()
    ref = pair_reference(x.detach(), wk, wv, gk, gv, groups)
    judge("gl", "pair: k", k.detach(), ref["k"], rtol=RT_BF)
    judge("gl", "pair: v", v.detach(), ref["v"], rtol=RT_BF)
    judge("gl", "pair: dx", x.grad, ref["dx_k"] + ref["dx_v"], rtol=RT_BF)
    judge("gl.dw", "pair: dWk", wk.grad, ref["dwk"], dw_expr32(x.detach(), gk, groups))
    judge("gl.dw", "pair: dWv", wv.grad, ref["dwv"], dw_expr32(x.detach(), gv, groups))
    rejects("gl", "pair: dx without the v part", x.grad, ref["dx_k"], rtol=RT_BF)
    shifted = ref["dwk"].clone()
    shifted[-64:] = ref["dwk"][-128:-64]
    rejects("gl.dw", "pair: dWk, the last group replaced by the previous one", wk.grad, shifted)


# ---- segment mean ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class SM:
    name: str
    B: int
    G: int
    T: int
    D: int
    dtype: torch.dtype


def _sm_cases():
    cases = []
    for D in (768, 1024):
        for dt in (F32, BF):
            for T in (1, 2, 3, 5, 49, 196):
                cases.append(SM(f"smf_d{D}_{'bf16' if dt == BF else 'f32'}_t{T}", 3, 8, T, D, dt))
    cases.append(SM("smf_limit", 1, 8, 1874, 768, F32))
    n = 0
    for G in (3, 5, 8):
        for D in (4, 64, 772, 1024):
            if G == 8 and D == 1024:
                continue
            for T in (1, 7, 50):
                dt = (F32, BF)[n % 2]
                n += 1
                cases.append(SM(f"smg_g{G}_d{D}_{'bf16' if dt == BF else 'f32'}_t{T}", 3, G, T, D, dt))
    return cases


SM_CASES = _sm_cases()


def sm_assignment(gen, B, G, T):
    """idx (B, T): center 1 stays empty in every sample, sample 0 has every token on center 2"""
    allowed = torch.tensor([g for g in range(G) if g != 1])
    idx = allowed[torch.randint(0, G - 1, (B, T), generator=gen)]
    idx[0] = 2
    return idx.to(torch.uint8)


def sm_expr(idx, v, dout, G, dt, clamp=True, drop_dc=False):
    hard = torch.nn.functional.one_hot(idx.long(), G).permute(0, 2, 1).to(dt)        # (B, G, T)
    v, dout = v.to(dt), dout.to(dt)
    cnt = hard.sum(-1, keepdim=True)
    c = cnt.clamp_min(1.0) if clamp else cnt
    out = hard @ v / c
    dn = dout / c
    dc = torch.where(cnt >= 1, -(dout * out).sum(-1, keepdim=True) / c, torch.zeros_like(c))
    dhard = dn @ v.transpose(1, 2)
    return {"out": out, "dv": hard.transpose(1, 2) @ dn, "dhard": dhard if drop_dc else dhard + dc, "hard": hard, "c": c}


def sm_run(name, idx, v, dout, G):
    """forward and backward through the C ABI in frames -> (out, dv, dhard) views"""
    B, T, D = v.shape
    counts = torch.stack([torch.bincount(r.long(), minlength=G) for r in idx.cpu()]).float().to(DEV)
    fi, fv, fc, fd = put(idx), put(v), put(counts), put(dout)
    fo, fdv, fdh = Frame((B, G, D), F32), Frame((B, T, D), v.dtype), Frame((B, G, T), F32)
    run_twice(name + " fwd", lambda: lib_call("segclip_segmean_fwd", fi.p, fv.p, L.dt(v), fc.p, fo.p, B, G, T, D), [fo])
    run_twice(name + " bwd", lambda: lib_call("segclip_segmean_bwd", fd.p, fo.p, fi.p, fv.p, L.dt(v), fc.p, fdv.p, fdh.p, B, G, T, D),
              [fdv, fdh])
    assert fo.intact() and all(f.intact() for f in (fi, fv, fc, fd))
    return fo.v, fdv.v, fdh.v


@pytest.mark.parametrize("c", SM_CASES, ids=[c.name for c in SM_CASES])
def test_segment_mean(c):
    gen = seeded(c.name)
    idx = sm_assignment(gen, c.B, c.G, c.T).to(DEV)
    v, dout = draw(gen, c.B, c.T, c.D, dtype=c.dtype), draw(gen, c.B, c.G, c.D)
    out, dv, dhard = sm_run(c.name, idx, v, dout, c.G)
    ref = sm_expr(idx, v, dout, c.G, F64)
    r32 = sm_expr(idx, v, dout, c.G, F32) if BOUNDS.stats is not None else {}
    bf = c.dtype == BF
    judge("segmean.out", f"{c.name}: out", out, ref["out"], r32.get("out"))
    if bf:
        judge("segmean.dv_bf16", f"{c.name}: dv", dv, ref["dv"], rtol=RT_BF)
    else:
        judge("segmean.dv", f"{c.name}: dv", dv, ref["dv"], r32.get("dv"))
    judge("segmean.dhard", f"{c.name}: dhard", dhard, ref["dhard"], r32.get("dhard"))
    # defects
    rejects("segmean.out", f"{c.name}: out, the last token left out", out, ref["out"] - ref["hard"][:, :, -1:] * v.double()[:, -1:, :] / ref["c"])
    moved = idx.clone()
    moved[:, c.T // 2] = (idx[:, c.T // 2] + 1) % c.G
    wrong = sm_expr(moved, v, dout, c.G, F64)
    rejects("segmean.out", f"{c.name}: out, a token moved to the neighbouring center", out, wrong["out"])
    rejects("segmean.dv", f"{c.name}: dv, a token moved to the neighbouring center", dv, wrong["dv"], rtol=RT_BF if bf else None)
    rejects("segmean.dhard", f"{c.name}: dhard, no clamp on the empty center", dhard, sm_expr(idx, v, dout, c.G, F64, clamp=False)["dhard"])
    rejects("segmean.dhard", f"{c.name}: dhard, dc dropped", dhard, sm_expr(idx, v, dout, c.G, F64, drop_dc=True)["dhard"])


# ---- assignment logits -------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class CL:
    name: str
    B: int
    T: int
    D: int
    bwd: bool = True


CL_CASES = [
    CL("cl_9x64_d768", 2, 576, 768), CL("cl_9x64_d1024", 2, 576, 1024), CL("cl_13x61_d768", 16, 784, 768),
    CL("cl_13x61_d1024", 16, 784, 1024), CL("cl_one_range_d768", 3, 48, 768), CL("cl_one_range_d1024", 3, 48, 1024),
    CL("cl_no_split_d768", 130, 5, 768), CL("cl_no_split_d1024", 130, 5, 1024), CL("cl_t1_d768", 3, 1, 768),
    CL("cl_t1_d1024", 2, 1, 1024), CL("cl_t3_d768", 2, 3, 768), CL("cl_t3_d1024", 3, 3, 1024),
    CL("cl_bwd_limit_768", 1, 1232, 768), CL("cl_bwd_limit_1024", 1, 976, 1024),
    CL("cl_fwd_lds_max", 128, 1875, 768, bwd=False),
]


def cl_expr(q, k, dl, dt):
    q, k = q.to(dt), k.to(dt)
    r = {"attn": q @ k.transpose(1, 2)}
    if dl is not None:
        dl = dl.to(dt)
        r["dq"], r["dk"] = dl @ k, dl.transpose(1, 2) @ q
    return r


def cl_defects(q, k, dl, ref):
    T = k.shape[1]
    wrong = {}
    if T >= 2:
        k2 = k.clone()
        k2[:, T - 1] = k[:, T - 2]
        w = {"attn": cl_expr(q, k2, None, F64)["attn"]}
        if dl is not None:
            w["dq"] = cl_expr(q, k2, dl, F64)["dq"]
            w["dk"] = ref["dk"].clone()
            w["dk"][:, T - 1] = ref["dk"][:, T - 2]
        wrong["the last token replaced by its neighbour"] = w
    q2 = q.clone()
    q2[..., -4:] = 0
    w = {"attn": cl_expr(q2, k, None, F64)["attn"]}
    if dl is not None:
        w["dq"], w["dk"] = ref["dq"].clone(), ref["dk"].clone()
        w["dq"][..., -4:] = 0
        w["dk"][..., -4:] = 0
    wrong["the last four columns zeroed"] = w
    return wrong


@pytest.mark.parametrize("c", [c for c in CL_CASES if c.bwd], ids=[c.name for c in CL_CASES if c.bwd])
def test_center_logits(c):
    gen = seeded(c.name)
    q, k, dl = draw(gen, c.B, 8, c.D), draw(gen, c.B, c.T, c.D), draw(gen, c.B, 8, c.T)
    fq, fk, fdl = put(q), put(k), put(dl)
    fa, fdq, fdk = Frame((c.B, 8, c.T), F32), Frame((c.B, 8, c.D), F32), Frame((c.B, c.T, c.D), F32)
    run_twice(c.name + " fwd", lambda: lib_call("segclip_center_logits_fwd", fq.p, fk.p, fa.p, c.B, 8, c.T, c.D), [fa])
    run_twice(c.name + " bwd", lambda: lib_call("segclip_center_logits_bwd", fdl.p, fq.p, fk.p, fdq.p, fdk.p, c.B, 8, c.T, c.D),
              [fdq, fdk])
    assert all(f.intact() for f in (fq, fk, fdl))
    ref = cl_expr(q, k, dl, F64)
    r32 = cl_expr(q, k, dl, F32) if BOUNDS.stats is not None else {}
    got = {"attn": fa.v, "dq": fdq.v, "dk": fdk.v}
    for n in got:
        judge(f"logits.{n}", f"{c.name}: {n}", got[n], ref[n], r32.get(n))
    for what, w in cl_defects(q, k, dl, ref).items():
        for n in got:
            rejects(f"logits.{n}", f"{c.name}: {n}, {what}", got[n], w[n])


def test_center_logits_forward_at_its_largest_lds():
    """B = 128 (no token split), T = 1875: 60000 bytes of LDS.  k is one host-drawn block of 8 samples tiled 16 times, copy j
    multiplied by 2^(j - 8) (exact), so the fp64 reference of copy j is the block's times 2^(j - 8); all 128 samples compared"""
    c = CL_CASES[-1]
    gen = seeded(c.name)
    q, kb = draw(gen, c.B, 8, c.D), draw(gen, 8, c.T, c.D)
    fq, fk, fa = put(q), Frame((c.B, c.T, c.D), F32), Frame((c.B, 8, c.T), F32)
    for j in range(16):
        torch.mul(kb, 2.0 ** (j - 8), out=fk.v[8 * j:8 * j + 8])
    run_twice(c.name, lambda: lib_call("segclip_center_logits_fwd", fq.p, fk.p, fa.p, c.B, 8, c.T, c.D), [fa])
    assert fq.intact() and fk.intact()
    kb2 = kb.clone()
    kb2[:, -1] = kb[:, -2]
    for j in range(16):
        s = slice(8 * j, 8 * j + 8)
        ref = cl_expr(q[s], kb, None, F64)["attn"] * 2.0 ** (j - 8)
        r32 = cl_expr(q[s], kb * 2.0 ** (j - 8), None, F32)["attn"] if BOUNDS.stats is not None else None
        judge("logits.attn", f"{c.name}: samples {8 * j}..{8 * j + 7}", fa.v[s], ref, r32)
        rejects("logits.attn", f"{c.name}: copy {j}, the last token replaced by its neighbour", fa.v[s],
                cl_expr(q[s], kb2, None, F64)["attn"] * 2.0 ** (j - 8))
        q2 = q[s].clone()
        q2[..., -4:] = 0
        rejects("logits.attn", f"{c.name}: copy {j}, the last four columns zeroed", fa.v[s], cl_expr(q2, kb, None, F64)["attn"] * 2.0 ** (j - 8))


# ---- recon mix ---------------------------------------------------------------------------------------------------------------
RM_CASES = [(2 if D >= 2048 else 3, M, D) for M in (1, 63, 64, 65, 197) for D in (4, 40, 260, 768, 1024, 2048, 4096)]


def rm_expr(a, x, dout, dt):
    a, x, dout = a.to(dt), x.to(dt), dout.to(dt)
    return {"out": a @ x, "da": dout @ x.transpose(1, 2), "dx": a.transpose(1, 2) @ dout}


def rm_defects(a, x, dout, ref):
    M = a.shape[1]
    a7 = a.clone()
    a7[..., 7] = 0
    w = {"out": rm_expr(a7, x, dout, F64)["out"], "da": ref["da"].clone(), "dx": ref["dx"].clone()}
    w["da"][..., 7] = 0
    w["dx"][:, 7] = 0
    wrong = {"center 7 dropped": w}
    if M >= 2:
        d2 = dout.clone()
        d2[:, M - 1] = dout[:, M - 2]
        w = {"out": ref["out"].clone(), "da": ref["da"].clone(), "dx": rm_expr(a, x, d2, F64)["dx"]}
        w["out"][:, M - 1] = ref["out"][:, M - 2]
        w["da"][:, M - 1] = ref["da"][:, M - 2]
        wrong["row M - 1 replaced by its neighbour"] = w
    return wrong


@pytest.mark.parametrize("B,M,D", RM_CASES, ids=[f"rm_m{M}_d{D}" for _, M, D in RM_CASES])
def test_recon_mix(B, M, D):
    name = f"rm_m{M}_d{D}"
    gen = seeded(name)
    a, x, dout = draw(gen, B, M, 8), draw(gen, B, 8, D), draw(gen, B, M, D)
    fa, fx, fd = put(a), put(x), put(dout)
    fo, fda, fdx = Frame((B, M, D), F32), Frame((B, M, 8), F32), Frame((B, 8, D), F32)
    run_twice(name + " fwd", lambda: lib_call("segclip_recon_mix_fwd", fa.p, fx.p, fo.p, B, M, 8, D), [fo])
    run_twice(name + " bwd", lambda: lib_call("segclip_recon_mix_bwd", fa.p, fx.p, fd.p, fda.p, fdx.p, B, M, 8, D), [fda, fdx])
    assert all(f.intact() for f in (fa, fx, fd))
    ref = rm_expr(a, x, dout, F64)
    r32 = rm_expr(a, x, dout, F32) if BOUNDS.stats is not None else {}
    got = {"out": fo.v, "da": fda.v, "dx": fdx.v}
    for n in got:
        judge(f"recon.{n}", f"{name}: {n}", got[n], ref[n], r32.get(n))
    for what, w in rm_defects(a, x, dout, ref).items():
        for n in got:
            rejects(f"recon.{n}", f"{name}: {n}, {what}", got[n], w[n])


# ---- hard assignment -----------------------------------------------------------------------------------------------------------
AS_CASES = [(B, G, T, train) for G in (3, 5, 8) for B, T in ((257, 1), (37, 7), (3, 577)) for train in (True, False)]


def as_inputs(name, B, G, T, train):
    """logits (and Gumbel noise) on the host, made decisive: no token whose two largest z are less than 1e-3 apart, except the
    two intended ties of the evaluation rows (token 0 of sample 0: two equal largest; token 0 of sample 1: all G equal)"""
    gen = seeded(name)
    l = (torch.randn(B, G, T, generator=gen, dtype=F64) * 5.0).float()
    g = torch.randn(B, G, T, generator=gen, dtype=F64).float() if train else None
    z = lambda: ((l + g) / torch.tensor(TAU32) if train else l.clone())   # noqa: E731  fp32, as the kernel forms it
    top = z().topk(2, dim=1)
    close_ = (top.values[:, 0] - top.values[:, 1]) < 1e-3                  # (B, T)
    bump = torch.zeros_like(l).scatter_(1, top.indices[:, :1], (close_.float() * 1e-2 * (TAU32 if train else 1.0)).unsqueeze(1))
    l = l + bump
    ties = torch.zeros(B, T, dtype=torch.bool)
    if not train:
        m = l[0, :, 0].max() + 1.0
        l[0, 0, 0], l[0, G - 1, 0] = m, m
        l[1, :, 0] = 0.5
        ties[0, 0] = ties[1, 0] = True
    top = z().topk(2, dim=1).values
    assert not bool((((top[:, 0] - top[:, 1]) < 1e-3) & ~ties).any()), "an undecided token remains"
    return l.to(DEV), (g.to(DEV) if train else None)


def as_expr(l, g, tau, dhard, dt):
    l = l.to(dt)
    z = (l + g.to(dt)) / tau if g is not None else l
    y = z.softmax(1)
    dh = dhard.to(dt)
    return {"z": z, "y_soft": y, "soft": l.softmax(1), "dlogits": y * (dh - (dh * y).sum(1, keepdim=True)) / tau,
            "nodot": y * dh / tau}


def first_max(z):
    """index of the first maximum along dim 1, spelled out (ties: the lowest index)"""
    G = z.shape[1]
    ar = torch.arange(G, device=z.device).view(1, G, 1).expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, ar, torch.full_like(ar, G)).min(1).values


@pytest.mark.parametrize("B,G,T,train", AS_CASES, ids=[f"as_g{G}_t{T}_{'train' if tr else 'eval'}" for _, G, T, tr in AS_CASES])
def test_assign(B, G, T, train):
    name = f"as_g{G}_t{T}_{'train' if train else 'eval'}"
    l, g = as_inputs(name, B, G, T, train)
    tau = TAU32 if train else 1.0
    dhard = draw(seeded(name + "d"), B, G, T)
    fl, fg, fdh = put(l), (put(g) if train else None), put(dhard)
    fy, fs, fh = (Frame((B, G, T), F32) for _ in range(3))
    fi, fc, fdl = Frame((B, T), torch.uint8), Frame((B, G), F32), Frame((B, G, T), F32)
    run_twice(name + " fwd", lambda: lib_call("segclip_assign_fwd", fl.p, fg.p if train else None, tau, fy.p, fs.p, fi.p, fh.p, fc.p, B, G, T),
              [fy, fs, fh, fi, fc])
    run_twice(name + " bwd", lambda: lib_call("segclip_assign_bwd", fdh.p, fy.p, tau, fdl.p, B, G, T), [fdl])
    assert fl.intact() and fdh.intact() and fy.intact() and (fg is None or fg.intact())
    ref = as_expr(l, g, tau, dhard, F64)
    r32 = as_expr(l, g, tau, dhard, F32) if BOUNDS.stats is not None else {}
    idx = first_max(ref["z"])
    if not train:
        assert int(idx[0, 0]) == 0 and int(idx[1, 0]) == 0, "the ties are meant to be won by the lowest index"
    assert torch.equal(fi.v.long(), idx), f"{name}: the arg-max over the centers must be bit exact at every token"
    hard = torch.nn.functional.one_hot(idx, G).permute(0, 2, 1).float()
    assert torch.equal(fh.v, hard), f"{name}: hard is not the one-hot of idx"
    assert torch.equal(fc.v, hard.sum(-1)), f"{name}: counts are not bincount(idx)"
    got = {"y_soft": fy.v, "soft": fs.v, "dlogits": fdl.v}
    for n in got:
        judge(f"assign.{n}", f"{name}: {n}", got[n], ref[n], r32.get(n))
    flat = lambda t: t.permute(0, 2, 1).reshape(B * T, G)   # noqa: E731  token-major
    for n in got:
        w = flat(ref[n]).clone()
        w[-1] = w[-2]
        rejects(f"assign.{n}", f"{name}: {n}, the last token replaced by its neighbour", flat(got[n]), w)
    rejects("assign.dlogits", f"{name}: dlogits without the row-dot term", got["dlogits"], ref["nodot"])


# ---- gates ---------------------------------------------------------------------------------------------------------------------
def fn_name(t):
    return type(t.grad_fn).__name__


@pytest.mark.parametrize("T,D,loop", [(976, 1024, True), (977, 1024, False), (1232, 768, True), (1233, 768, False), (1875, 768, False),
                                      (1876, 768, False)])
def test_gate_center_logits(T, D, loop):
    """ops.center_logits on both sides of the backward's limit (976 | 977, 1232 | 1233) and of the forward's (1875 | 1876): where
    a gradient is needed, the token loop only if its backward covers the shape; forward and backward meet the bounds"""
    gen = seeded(f"gate_cl_{T}_{D}")
    q, k, dl = draw(gen, 1, 8, D).requires_grad_(), draw(gen, 1, T, D).requires_grad_(), draw(gen, 1, 8, T)
    attn = ops.center_logits(q, k, exact=False)
    assert fn_name(attn) == ("CenterLogitsFnBackward" if loop else "BmmFnBackward")
    attn.backward(dl)
    ref = cl_expr(q.detach(), k.detach(), dl, F64)
    for n, got in (("attn", attn), ("dq", q.grad), ("dk", k.grad)):
        judge(f"logits.{n}", f"gate T={T} D={D}: {n}", got, ref[n])
    with torch.no_grad():          # inference keeps the token-loop forward up to the forward's own limit
        inf = ops.center_logits(q, k, exact=False)
    judge("logits.attn", f"gate T={T} D={D}: attn without grad", inf, ref["attn"])
    fa = Frame((1, 8, T), F32)
    if T <= 1875:
        lib_call("segclip_center_logits_fwd", L.ptr(q.detach()), L.ptr(k.detach()), fa.p, 1, 8, T, D)
        assert torch.equal(inf, fa.v), "a forward-only call is expected on the token-loop kernel"
    else:
        with pytest.raises(L.Unsupported):
            lib_call("segclip_center_logits_fwd", L.ptr(q.detach()), L.ptr(k.detach()), fa.p, 1, 8, T, D)
        assert bool(fa.buf.isnan().all())


@pytest.mark.parametrize("G,D,kernel", [(8, 4096, True), (8, 4100, False), (7, 768, False)])
def test_gate_recon_mix(G, D, kernel):
    B, M = 2, 65
    gen = seeded(f"gate_rm_{G}_{D}")
    a, x, dout = draw(gen, B, M, G).requires_grad_(), draw(gen, B, G, D).requires_grad_(), draw(gen, B, M, D)
    out = ops.recon_mix(a, x)
    assert fn_name(out) == ("ReconMixFnBackward" if kernel else "BmmFnBackward")
    out.backward(dout)
    ref = rm_expr(a.detach(), x.detach(), dout, F64)
    for n, got in (("out", out), ("da", a.grad), ("dx", x.grad)):
        judge(f"recon.{n}", f"gate G={G} D={D}: {n}", got, ref[n])


@pytest.mark.parametrize("T,D,dtype,kernel", [(1874, 768, F32, True), (1875, 768, F32, False), (50, 770, F32, False),
                                               (1874, 768, BF, True), (1875, 768, BF, False)])
def test_gate_segment_mean(T, D, dtype, kernel):
    """the module's segment-mean branch on both sides of the backward's LDS limit and at a width that is no multiple of 4.  On
    the batched-GEMM side in bf16 the product part of dhard, dN v^T, has dN rounded to bf16 (half an ulp, 2^-9, per term) and
    leaves the GEMM as bf16 (2^-9 of the result): |err| <= 2 * 2^-9 * (|dN| |v|^T + |dN v^T|) per element there, the factor 2
    as everywhere in this file; the fp32 bound everywhere else."""
    B, G = 1, 8
    gen = seeded(f"gate_sm_{T}_{D}")
    idx = sm_assignment(gen, B, G, T).to(DEV)
    v, dout = draw(gen, B, T, D, dtype=dtype).requires_grad_(), draw(gen, B, G, D)
    hard = torch.nn.functional.one_hot(idx.long(), G).permute(0, 2, 1).float().contiguous().requires_grad_()
    counts = hard.detach().sum(-1)
    out = msv._segment_mean(hard, idx, counts, v)
    assert (fn_name(out) == "SegMeanFnBackward") == kernel
    out.backward(dout)
    ref = sm_expr(idx, v.detach(), dout, G, F64)
    gemm16 = dtype == BF and not kernel
    judge("segmean.out", f"gate T={T} D={D}: out", out, ref["out"])
    judge("segmean.dv", f"gate T={T} D={D}: dv", v.grad, ref["dv"], rtol=RT_BF if dtype == BF else None)
    if gemm16:
        dn, vt = dout.double() / ref["c"], v.detach().double().transpose(1, 2)
        err = (hard.grad.double() - ref["dhard"]).abs()
        assert bool((err <= 2.0 ** -8 * (dn.abs() @ vt.abs() + (dn @ vt).abs())).all()), f"dhard: max err {float(err.max()):.3e}"
    else:
        judge("segmean.dhard", f"gate T={T} D={D}: dhard", hard.grad, ref["dhard"])
    with torch.no_grad():          # inference: the forward kernel has no limit on T
        inf = msv._segment_mean(hard, idx, counts, v)
    judge("segmean.out", f"gate T={T} D={D}: out without grad", inf, ref["out"])


@pytest.mark.parametrize("D,groups,pitch,fused", [(768, 12, 776, True), (768, 12, 772, False), (384, 12, 392, False)],
                         ids=["pitch_8", "pitch_not_8", "hd32"])
def test_gate_group_linear_pair(D, groups, pitch, fused):
    """_group_linear_pair: the fused kernel for 64-channel groups and a row pitch that is a multiple of 8, two batched GEMMs
    otherwise.  On the GEMM side dx is the bf16 sum of two bf16 results: three roundings of half an ulp, of the two parts and of
    their sum - bound 2 * 2^-9 * (|part k| + |part v| + |sum|) per element, the factor 2 as everywhere in this file."""
    M = 129
    fx, x, wk, wv, gk, gv = pair_inputs(f"gate_gl_{D}_{pitch}", M, D, groups, pitch)
    k, v = msv._group_linear_pair(x, wk, wv, groups)
    assert fn_name(k) == ("GroupLinearPairFnBackward" if fused else "GroupLinearFnBackward")
    torch.autograd.backward([k, v], [gk, gv])
    torch.cuda.synchronize()
    assert fx.intact()
    ref = pair_reference(x.detach(), wk, wv, gk, gv, groups)
    judge("gl", f"gate {D}/{pitch}: k", k, ref["k"], rtol=RT_BF)
    judge("gl", f"gate {D}/{pitch}: v", v, ref["v"], rtol=RT_BF)
    dx = ref["dx_k"] + ref["dx_v"]
    if fused:
        judge("gl", f"gate {D}/{pitch}: dx", x.grad, dx, rtol=RT_BF)
    else:
        err = (x.grad.double() - dx).abs()
        assert bool((err <= 2.0 ** -8 * (ref["dx_k"].abs() + ref["dx_v"].abs() + dx.abs())).all()), f"dx: max err {float(err.max()):.3e}"
    judge("gl.dw", f"gate {D}/{pitch}: dWk", wk.grad, ref["dwk"])
    judge("gl.dw", f"gate {D}/{pitch}: dWv", wv.grad, ref["dwv"])


# ---- the table reaches every instance ------------------------------------------------------------------------------------------
def instance_of(kind, **s):
    """the kernel instance a shape reaches: the dispatchers of csrc/center.hip and csrc/group_linear.hip restated"""
    if kind == "segmean":
        dt = "bf16" if s["dtype"] == BF else "f32"
        return ("fast", dt, s["D"]) if s["G"] == 8 and s["D"] in (768, 1024) else ("generic", dt)
    if kind == "logits":
        return (s["D"] // 256, "split" if s["B"] < 128 and s["T"] > 64 else "whole")
    raise KeyError(kind)


def test_rows_reach_every_instance():
    assert {(c.n_in, c.n_out) for c in GL_CASES} == {(1, 1), (1, 2), (2, 1)}
    for inst in ((1, 1), (1, 2), (2, 1)):
        rows = [c for c in GL_CASES if (c.n_in, c.n_out) == inst]
        assert {c.M for c in rows} == {1, 31, 32, 33, 127, 129, 1000} and {c.groups for c in rows} == {1, 7, 12, 13, 16}
        assert {c.pitched for c in rows} == {True, False}
    sm = {}
    for c in SM_CASES:
        sm.setdefault(instance_of("segmean", G=c.G, D=c.D, dtype=c.dtype), []).append(c)
    assert set(sm) == {("fast", d, D) for d in ("f32", "bf16") for D in (768, 1024)} | {("generic", "f32"), ("generic", "bf16")}
    for inst, rows in sm.items():
        if inst[0] == "fast":
            assert {1, 2, 3, 5} <= {c.T for c in rows}
        else:
            assert {c.G for c in rows} == {3, 5, 8} and {c.D for c in rows} == {4, 64, 772, 1024} and {c.T for c in rows} == {1, 7, 50}
    assert ("generic", "f32") == instance_of("segmean", G=5, D=1024, dtype=F32)
    cl = {instance_of("logits", B=c.B, T=c.T, D=c.D) for c in CL_CASES}
    assert cl == {(n, w) for n in (3, 4) for w in ("split", "whole")}
    assert {D for _, _, D in RM_CASES} == {4, 40, 260, 768, 1024, 2048, 4096} and {M for _, M, _ in RM_CASES} == {1, 63, 64, 65, 197}


# ---- the measurement behind FLOORS -----------------------------------------------------------------------------------------------
def floors():
    """every row once with BOUNDS.stats set: {key: floor of torch float32 against fp64, the kernel's error, the rows they come from}"""
    BOUNDS.stats = {}
    try:
        for c in SM_CASES:
            test_segment_mean(c)
        for c in CL_CASES:
            if c.bwd:
                test_center_logits(c)
        test_center_logits_forward_at_its_largest_lds()
        for r in RM_CASES:
            test_recon_mix(*r)
        for r in AS_CASES:
            test_assign(*r)
        test_group_linear_pair_end_to_end()
        return BOUNDS.stats
    finally:
        BOUNDS.stats = None
