"""The top-K search against its eager composition from torch (tool only; writes profiles/retrieval_topk.txt).  The shape and the
method are those of tools/bench_retrieval.py.

Workload: COCO-5k scale - 5 000 images x 25 000 captions (5 per image, shuffled) x E = 512, k = 10, synthetic unit vectors from
a seed, both directions; and one query against 100 000 rows, the interactive case, which runs on partial lists.

  (a) retrieval.search(normalise=False) and the eager composition (Q[i:i+c] @ X.T).topk(k) in chunks, alternating within each
      repeat on the same box; the shader clock held over the timed region; the peak allocation of each above the inputs; and
      that the two return the same index sets wherever fp32 can tell the k-th from the (k+1)-th score
  (b) the kernels alone in `rocprofv3 --kernel-trace --stats` children of their own (--child=<what>: ten calls and nothing else),
      retrieval_topk_kernel beside retrieval_count_kernel on the same shape: the same product without the selection, so the
      difference is the price of the epilogue

  python tools/bench_retrieval_topk.py [repeats] [output file]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from segclip_amd.retrieval import RetrievalEvaluator, search

CHILD = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--child=")), None)
ARGV = [a for a in sys.argv[1:] if not a.startswith("--child=")]
REPS = int(ARGV[0]) if len(ARGV) > 0 else 7
OUT = ARGV[1] if len(ARGV) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                 "retrieval_topk.txt")
NI, PER, E, K, SEED = 5000, 5, 512, 10, 7
NT = NI * PER
ROWS = 100000                # the gallery of the one-query case
EAGER_CHUNK = 2048
CUS, MFMA_F32_FLOP_PER_CLK_CU = 256, 256   # MI355X; v_mfma_f32_32x32x2_f32: 64 flop / clock / SIMD
CALLS = 20
GAP = 2.0 * E * 2.0 ** -24   # two fp32 dot products of unit vectors closer than this need not be ordered alike
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def inputs():
    g = torch.Generator(device="cuda").manual_seed(SEED)
    V = torch.nn.functional.normalize(torch.randn(NI, E, generator=g, device="cuda"), dim=1)
    idx = torch.arange(NI, device="cuda", dtype=torch.int32).repeat_interleave(PER)[torch.randperm(NT, generator=g, device="cuda")]
    T = torch.nn.functional.normalize(V[idx.long()] + 1.5 * torch.randn(NT, E, generator=g, device="cuda") / E ** 0.5, dim=1)
    big = torch.nn.functional.normalize(torch.randn(ROWS, E, generator=g, device="cuda"), dim=1)
    return V, T, idx.contiguous(), big


def fused(Q, X):
    return search(Q, X, K, normalise=False)


def eager(Q, X, k=K):
    idx = torch.empty(Q.shape[0], k, dtype=torch.int64, device=Q.device)
    val = torch.empty(Q.shape[0], k, dtype=torch.float32, device=Q.device)
    for s in range(0, Q.shape[0], EAGER_CHUNK):
        val[s:s + EAGER_CHUNK], idx[s:s + EAGER_CHUNK] = (Q[s:s + EAGER_CHUNK] @ X.T).topk(k)
    return idx, val


def child(what):
    """ten calls of one entry and nothing else: what a rocprofv3 child traces"""
    V, T, g, big = inputs()
    for _ in range(10):
        if what == "count":
            ev = RetrievalEvaluator()
            ev.add_embeddings(V, T, g, normalise=False)
            ev.ranks()
        else:
            fused(*{"t2i": (T, V), "i2t": (V, T), "one": (T[:1], big)}[what])
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


def agreement(Q, X):
    """rows whose index sets differ between the two, and those of them that fp32 could have told apart"""
    a, _ = fused(Q, X)
    b, bv = eager(Q, X, K + 1)
    differ = (a.long().sort(1).values != b[:, :K].sort(1).values).any(1)
    clear = bv[:, K - 1] - bv[:, K] > GAP
    return int(differ.sum()), int((differ & clear).sum())


def traced(what, done={}):
    """the kernel table of the child `what` (one rocprofv3 run per child)"""
    if what not in done:
        done[what] = _traced(what)
    return done[what]


def _traced(what):
    from tools import rocprof_roofline as rr
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        try:
            rc, _, err = rr.run_child([os.path.abspath(__file__), f"--child={what}"], tmp)
            db = rr.find_db(tmp)
            return (rr.kernel_table(db) if rc == 0 and db else []), rc, err
        except Exception as e:   # no rocprofv3 on the box
            return [], -1, repr(e)


def main():
    from tools.clock_sampler import ClockSampler
    say(f"# tools/bench_retrieval_topk.py  {NI} images x {NT} captions x E = {E}, k = {K}; 1 query x {ROWS} rows; "
        f"{torch.cuda.get_device_name(0)}")
    V, T, _, big = inputs()
    matrix = NT * NI * 4
    cases = [("captions -> images", T, V), ("images -> captions", V, T), (f"1 query -> {ROWS} rows", T[:1].contiguous(), big)]
    ways = [("search()", fused), (f"eager (Q[i:i+{EAGER_CHUNK}] @ X.T).topk({K})", eager)]
    say(f"similarity matrix never formed: {matrix} bytes; inputs {(NI + NT) * E * 4} bytes")
    for what, Q, X in cases:
        for _, fn in ways:
            fn(Q, X)
            fn(Q, X)
        n, m = agreement(Q, X)
        say(f"{what}: rows whose index sets differ between the two {n} of {Q.shape[0]}; of these, rows whose k-th and (k+1)-th "
            f"scores lie farther apart than 2 E 2^-24: {m}")
    peaks = [[peak_of(fn, Q, X) for _, fn in ways] for _, Q, X in cases]
    ts = [[[] for _ in ways] for _ in cases]
    sampler = ClockSampler().start()
    for _ in range(REPS):   # alternating: every repeat times the ways one after the other
        for c, (_, Q, X) in enumerate(cases):
            for w, (_, fn) in enumerate(ways):
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    fn(Q, X)
                torch.cuda.synchronize()
                ts[c][w].append((time.perf_counter() - t0) / CALLS)
    clk = sampler.stop()
    for c, (what, Q, X) in enumerate(cases):
        meds = [statistics.median(t) for t in ts[c]]
        for w, (way, _) in enumerate(ways):
            t = ts[c][w]
            say(f"{what:24s} {way:36s} {meds[w] * 1e3:8.3f} ms (min {min(t) * 1e3:.3f}, max {max(t) * 1e3:.3f}; {REPS} x {CALLS} "
                f"calls); peak allocation above the inputs {peaks[c][w]} bytes = {peaks[c][w] / (Q.shape[0] * X.shape[0] * 4):.4f} "
                f"of its matrix")
        say(f"{what:24s} search / eager {meds[0] / meds[1]:.3f}")
    say(f"clock {clk}")
    mhz = clk["sclk_mhz_mean"] if clk else None
    flop = 2.0 * NT * NI * E
    peak = CUS * MFMA_F32_FLOP_PER_CLK_CU * mhz * 1e6 if mhz else None
    for what, kern in (("count", "retrieval_count_kernel"), ("t2i", "retrieval_topk_kernel"), ("i2t", "retrieval_topk_kernel"),
                       ("i2t", "retrieval_topk_merge_kernel"), ("one", "retrieval_topk_kernel"),
                       ("one", "retrieval_topk_merge_kernel")):
        table, rc, err = traced(what)
        rows = [r for r in table if kern in r[0] and ("merge" in r[0]) == ("merge" in kern)]
        if not rows:
            say(f"{kern} ({what}) alone: unmeasured (rocprofv3 child rc={rc}: {str(err)[-200:]})")
            continue
        _, calls, _, avg_us = rows[0]
        line = f"{kern} ({what}) alone (rocprofv3 --kernel-trace --stats, {calls} launches) {avg_us:9.1f} us per launch"
        if what != "one" and "merge" not in kern:
            line += f": {flop / avg_us / 1e6:.1f} TFLOP/s"
            if peak:
                line += f" = {flop / (avg_us * 1e-6) / peak:.3f} of the f32-MFMA peak at the {mhz:.0f} MHz held ({peak / 1e12:.1f} TFLOP/s)"
        say(line)
    say("# the clock is sampled over the whole alternating timed region (all cases, both ways), the kernel times come from the "
        "separate traced children; retrieval_count_kernel is the same product on the same shape without the selection")
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    child(CHILD) if CHILD else main()
