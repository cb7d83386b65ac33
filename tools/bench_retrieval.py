"""The fused retrieval evaluation against its eager composition from torch (tool only; writes profiles/retrieval.txt).

Workload: COCO-5k scale - 5 000 images x 25 000 captions (5 per image, shuffled) x E = 512, synthetic unit vectors from a seed.

  (a) RetrievalEvaluator.add_embeddings(normalise=False) + ranks() (three kernel entries, no (Nt, Ni) array) and the eager
      composition - a chunked matmul, two comparisons and two sums per chunk, giving the same two rank vectors - alternating
      within each repeat on the same box; the shader clock held over the timed region; the peak allocation of each above the
      inputs; and that the two agree (ranks may differ where fp32 cannot order two dot products: counted)
  (b) the kernels alone in a `rocprofv3 --kernel-trace --stats` child of their own (--child: ten calls and nothing else), and the
      count pass's share of the f32-MFMA peak (256 flop / clock / CU) at the clock held

  python tools/bench_retrieval.py [repeats] [output file]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from segclip_amd.retrieval import RetrievalEvaluator

CHILD = "--child" in sys.argv[1:]
ARGV = [a for a in sys.argv[1:] if a != "--child"]
REPS = int(ARGV[0]) if len(ARGV) > 0 else 7
OUT = ARGV[1] if len(ARGV) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                 "retrieval.txt")
NI, PER, E, SEED = 5000, 5, 512, 7
NT = NI * PER
EAGER_CHUNK = 2048
CUS, MFMA_F32_FLOP_PER_CLK_CU = 256, 256   # MI355X; v_mfma_f32_32x32x2_f32: 64 flop / clock / SIMD
CALLS = 20
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def inputs():
    g = torch.Generator(device="cuda").manual_seed(SEED)
    V = torch.nn.functional.normalize(torch.randn(NI, E, generator=g, device="cuda"), dim=1)
    idx = torch.arange(NI, device="cuda", dtype=torch.int32).repeat_interleave(PER)[torch.randperm(NT, generator=g, device="cuda")]
    T = torch.nn.functional.normalize(V[idx.long()] + 1.5 * torch.randn(NT, E, generator=g, device="cuda") / E ** 0.5, dim=1)
    return V, T, idx.contiguous()


def fused(V, T, g):
    ev = RetrievalEvaluator()
    ev.add_embeddings(V, T, g, normalise=False)
    return ev.ranks()


def eager(V, T, g):
    Ni, Nt = V.shape[0], T.shape[0]
    gl = g.long()
    thr = (T * V[gl]).sum(1)
    best = torch.full((Ni,), float("-inf"), device=V.device).scatter_reduce(0, gl, thr, "amax")
    cols = torch.arange(Ni, device=V.device)
    rank_t2i = torch.empty(Nt, dtype=torch.int32, device=V.device)
    rank_i2t = torch.zeros(Ni, dtype=torch.int32, device=V.device)
    for s in range(0, Nt, EAGER_CHUNK):
        sim = T[s:s + EAGER_CHUNK] @ V.T
        other = gl[s:s + EAGER_CHUNK, None] != cols[None, :]
        rank_t2i[s:s + EAGER_CHUNK] = ((sim > thr[s:s + EAGER_CHUNK, None]) & other).sum(1)
        rank_i2t += ((sim > best[None, :]) & other).sum(0)
    rank_i2t[torch.bincount(gl, minlength=Ni) == 0] = -1
    return rank_t2i, rank_i2t


def child():
    """ten calls of the three entries and nothing else: what the rocprofv3 child traces"""
    V, T, g = inputs()
    for _ in range(10):
        fused(V, T, g)
    torch.cuda.synchronize()


def peak_of(fn, *args):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn(*args)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    from tools import rocprof_roofline as rr
    from tools.clock_sampler import ClockSampler
    say(f"# tools/bench_retrieval.py  {NI} images x {NT} captions x E = {E}, {torch.cuda.get_device_name(0)}")
    V, T, g = inputs()
    flop = 2.0 * NT * NI * E
    matrix = NT * NI * 4
    say(f"similarity matrix never formed: {matrix} bytes; count pass {flop / 1e9:.1f} GFLOP; inputs {(NI + NT) * E * 4} bytes")
    ways = [("add_embeddings + ranks()", fused), (f"eager torch, chunks of {EAGER_CHUNK}", eager)]
    for _, fn in ways:
        fn(V, T, g)
        fn(V, T, g)
    a, b = fused(V, T, g), eager(V, T, g)
    say(f"ranks that differ between the two (fp32 summation orders): t2i {int((a[0] != b[0]).sum())} of {NT}, "
        f"i2t {int((a[1] != b[1]).sum())} of {NI}; largest difference {int((a[0] - b[0]).abs().max())}, "
        f"{int((a[1] - b[1]).abs().max())}")
    peaks = [peak_of(fn, V, T, g) for _, fn in ways]
    ts = [[] for _ in ways]
    sampler = ClockSampler().start()
    for _ in range(REPS):   # alternating: every repeat times the ways one after the other
        for k, (_, fn) in enumerate(ways):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn(V, T, g)
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) / CALLS)
    clk = sampler.stop()
    meds = [statistics.median(t) for t in ts]
    for (what, _), t, med, pk in zip(ways, ts, meds, peaks):
        say(f"{what:32s} {med * 1e3:8.3f} ms (min {min(t) * 1e3:.3f}, max {max(t) * 1e3:.3f}; {REPS} x {CALLS} calls); "
            f"peak allocation above the inputs {pk} bytes = {pk / matrix:.4f} of the matrix")
    spread = max(max(t) - min(t) for t in ts)
    say(f"fused / eager {meds[0] / meds[1]:.3f}; largest max - min of a way {spread * 1e3:.3f} ms; clock {clk}")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        try:
            rc, _, err = rr.run_child([os.path.abspath(__file__), "--child"], tmp)
            db = rr.find_db(tmp)
            table = rr.kernel_table(db) if rc == 0 and db else []
        except Exception as e:   # no rocprofv3 on the box
            rc, err, table = -1, repr(e), []
    mhz = clk["sclk_mhz_mean"] if clk else None
    for kern in ("retrieval_count_kernel", "retrieval_thr_kernel", "retrieval_hist_kernel", "retrieval_init_kernel",
                 "retrieval_best_kernel"):
        rows = [r for r in table if kern in r[0]]
        if not rows:
            say(f"{kern} alone: unmeasured (rocprofv3 child rc={rc}: {str(err)[-200:]})")
            continue
        _, calls, _, avg_us = rows[0]
        line = f"{kern} alone (rocprofv3 --kernel-trace --stats, {calls} launches) {avg_us:9.1f} us per launch"
        if kern == "retrieval_count_kernel":
            line += f": {flop / avg_us / 1e6:.1f} TFLOP/s"
            if mhz:
                peak = CUS * MFMA_F32_FLOP_PER_CLK_CU * mhz * 1e6
                line += f" = {flop / (avg_us * 1e-6) / peak:.3f} of the f32-MFMA peak at the {mhz:.0f} MHz held ({peak / 1e12:.1f} TFLOP/s)"
            else:
                line += "; clock unmeasured, so no share of peak"
        say(line)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    child() if CHILD else main()
