"""GPU: the top-K search - segclip_retrieval_topk (csrc/retrieval_topk.inc), ops.retrieval_topk, retrieval.search,
RetrievalEvaluator.topk / search_texts / search_images, train.eval_retrieval_epoch(topk=) and retrieval.ZeroShotClassifier -
against tests/retrieval_topk_reference.py (numpy, fp64).

Exact cases: entries are multiples of 1/8, so every dot product is exact in fp32 in any order and ties are real; indices and
scores are compared with torch.equal, for every number of partial lists.  Realistic cases: unit vectors; with b = E 2^-24 (the
fp32 dot-product error bound for unit vectors) a result must pass topk_valid, whose last clause pins the index wherever the
fp64 order is determined; tests/test_retrieval_topk_cpu.py asserts on the reference alone that this holds for at least 90 % of
the entries of these seeds, and the tests here assert it again."""
import ctypes

import numpy as np
import pytest
import torch

from segclip_amd import _lib as L
from segclip_amd import ops, synth
from segclip_amd.retrieval import RetrievalEvaluator, ZeroShotClassifier, search
from segclip_amd.train import eval_retrieval_epoch
from tests import retrieval_reference as rr
from tests import retrieval_topk_reference as tr
from tests.helpers import tiny_seg_model
from tests.kernel_frames import Frame

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXACT_SHAPES = [(1, 1, 32), (5, 3, 64), (127, 129, 512), (333, 67, 768), (1300, 260, 512), (3, 5000, 64)]   # Nq, Nx, E
REALISTIC = [(21, 333, 67, 512, 10), (22, 640, 200, 768, 10), (41, 700, 5000, 64, 10), (41, 700, 5000, 64, 64)]
KS = (1, 5, 10, 64)
SPLITS = (0, 1, 2, 7)   # auto and three fixed partitions; the library clamps to the number of gallery tiles


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _assert_exact(Q, X, what):
    """every k and every number of partial lists gives the yardstick's indices and scores, bit for bit"""
    idx64, val64 = tr.topk(Q, X, max(KS))
    Qd, Xd = _dev(Q, X)
    for k in KS:
        want_idx, want_val = torch.from_numpy(idx64[:, :k].copy()), torch.from_numpy(val64[:, :k].copy())
        for splits in SPLITS:
            idx, val = ops.retrieval_topk(Qd, Xd, k, splits)
            assert idx.dtype == torch.int32 and val.dtype == torch.float32 and tuple(idx.shape) == tuple(val.shape) == (Q.shape[0], k)
            assert torch.equal(idx.cpu().long(), want_idx), f"{what} k={k} splits={splits}: indices"
            assert torch.equal(val.cpu().double(), want_val), f"{what} k={k} splits={splits}: scores"


@pytest.mark.parametrize("Nq,Nx,E", EXACT_SHAPES)
def test_exact_inputs_give_exact_equality(Nq, Nx, E):
    X, Q, _ = rr.exact_case(100 + Nq, Nq, Nx, E)    # exact_case(seed, Nt, Ni, E) -> V (Ni, E), T (Nt, E)
    _assert_exact(Q, X, "captions -> images")
    _assert_exact(X, Q, "images -> captions")


def test_rising_and_constant_galleries():
    """Rising: the scores of query 0 rise strictly with the index, so every tile admits k new entries (the worst case of a
    threshold filter); those of query 1 fall (the best case).  Constant: every score is equal, the answer is 0 .. k - 1."""
    Nq, Nx, E = 3, 5000, 64
    X, Q, _ = rr.exact_case(100 + Nq, Nq, Nx, E)
    X[:, 0] = np.arange(Nx, dtype=np.float32)
    Q[:2] = 0
    Q[0, 0], Q[1, 0] = 1, -1
    idx, _ = tr.topk(Q, X, 10)
    assert idx[0].tolist() == list(range(Nx - 1, Nx - 11, -1)) and idx[1].tolist() == list(range(10))
    _assert_exact(Q, X, "rising")
    X[:] = X[7]
    idx, val = tr.topk(Q, X, 64)
    assert (idx == np.arange(64)[None, :]).all() and (val == val[:, :1]).all()
    _assert_exact(Q, X, "constant")


def test_empty_queries_and_an_empty_gallery():
    Q, X = torch.ones(5, 32, device=DEV), torch.ones(0, 32, device=DEV)
    idx, val = ops.retrieval_topk(Q, X, 3)
    assert bool((idx == -1).all()) and bool(torch.isneginf(val).all()) and tuple(idx.shape) == (5, 3)
    idx, val = ops.retrieval_topk(X, Q, 3)
    assert tuple(idx.shape) == tuple(val.shape) == (0, 3)


@pytest.mark.parametrize("seed,Nt,Ni,E,k", REALISTIC)
def test_realistic_inputs_lie_inside_the_fp32_interval(seed, Nt, Ni, E, k):
    V, T, _ = rr.realistic_case(seed, Nt, Ni, E)
    b = rr.dot_gap(E) / 2
    for what, Q, X in (("captions -> images", T, V), ("images -> captions", V, T)):
        s64 = tr.scores(Q, X)
        idx, val = search(*_dev(Q, X), k, normalise=False)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        bad, share = tr.topk_valid(s64, idx, val, k, b)
        print(f"{what}: determined share {share:.3f}; entries off the fp64 yardstick "
              f"{int((idx != tr.topk_of_scores(s64, k)[0]).sum())}/{idx.size}")
        assert share >= 0.9        # the interval cannot hide a failure
        assert bad == [], f"{what}: {bad}"


@pytest.mark.parametrize("Nq", [127, 128, 129])
@pytest.mark.parametrize("Nx,splits", [(5, 0), (127, 0), (128, 0), (129, 0), (129, 2), (257, 0), (257, 3)])
def test_c_abi_writes_inside_its_frames(Nq, Nx, splits):
    E, k = 32, 10
    rng = np.random.default_rng(7 * Nq + Nx)                   # as exact_case: multiples of 1/8, a quarter of the gallery copies
    Q = rng.integers(-8, 9, size=(Nq, E)).astype(np.float32) / 8
    X = rng.integers(-8, 9, size=(Nx, E)).astype(np.float32) / 8
    X[rng.permutation(Nx)[:Nx // 4]] = X[rng.integers(0, Nx, size=Nx // 4)]
    want_idx, want_val = tr.topk(Q, X, k)
    Qd, Xd = _dev(Q, X)
    lib = L.load()
    need = lib.segclip_retrieval_topk_ws_bytes(Nq, Nx, k, splits)
    assert need >= 0 and need % 8 == 0 and (need > 0) == (splits > 1 or (splits == 0 and Nx > 128))
    idx, val, ws = Frame((Nq, k), torch.int32), Frame((Nq, k), torch.float32), Frame((max(need // 8, 1),), torch.int64)

    def call():
        L.check(lib.segclip_retrieval_topk(L.ptr(Qd), L.ptr(Xd), Nq, Nx, E, k, splits, idx.p, val.p, ws.p, need, L.stream()),
                "retrieval_topk")
        torch.cuda.synchronize()

    call()
    snap = [f.bits() for f in (idx, val, ws)]
    assert idx.intact() and val.intact() and ws.intact()
    if need == 0:
        assert ws.untouched()
    assert torch.equal(idx.v.cpu().long(), torch.from_numpy(want_idx))
    assert torch.equal(val.v.cpu().double(), torch.from_numpy(want_val))
    if Nx < k:
        assert bool((idx.v[:, Nx:] == -1).all()) and bool(torch.isneginf(val.v[:, Nx:]).all())
    call()
    assert all(torch.equal(a, f.bits()) for a, f in zip(snap, (idx, val, ws))), "the second call differs"


def test_agrees_with_the_ranks_of_the_evaluation():
    """The search and the ranks read the same numbers: exact equalities of integers, whether or not fp32 ties occur."""
    k = 10
    V, T, g = _dev(*rr.realistic_case(31, 1300, 260, 512))
    ev = RetrievalEvaluator()
    ev.add_embeddings(V, T, g, normalise=False)
    rank_t2i, rank_i2t = ev.ranks()
    top = ev.topk(k)
    assert ev.topk(k) is top                                   # cached beside the ranks
    thr, best, n_cap = ops.retrieval_thresholds(V, T, g, torch.zeros(1, dtype=torch.int32, device=DEV))
    idx_t, val_t = top["t2i"]
    idx_i, val_i = top["i2t"]
    assert torch.equal((val_t > thr[:, None]).sum(1), rank_t2i.clamp(max=k).long())
    has = n_cap > 0
    assert int(has.sum()) > 200 and int((~has).sum()) >= 1
    assert torch.equal((val_i > best[:, None]).sum(1)[has], rank_i2t.clamp(max=k).long()[has])
    own = idx_t == g[:, None]
    assert int(own.sum()) > 1000                               # most captions retrieve their image among the first 10
    assert torch.equal(val_t[own].view(torch.int32), thr[own.any(1)].view(torch.int32))
    ev.add_embeddings(visual=V[:3], normalise=False)
    assert ev._topk is None                                    # reset with the ranks


def _tiny_inputs(Ni=13, Nt=29):
    spec = synth.SPECS["tiny"]
    images = synth.synthetic_batch(spec, Ni, seed=3, device=DEV)["image"]
    texts = synth.synthetic_batch(spec, Nt, seed=4, device=DEV)
    g = rr.caption_index(np.random.default_rng(5), Nt, Ni)
    return images, texts["input_ids"], texts["segment_ids"], texts["input_mask"], g


def test_nothing_synchronises():
    V, T, g = _dev(*rr.realistic_case(33, 333, 67, 512))
    model = tiny_seg_model()
    images, ids, seg, mask, g_tiny = _tiny_inputs()
    labels = torch.arange(67, device=DEV) % 29
    tiny = RetrievalEvaluator(model, chunk=5)
    tiny.add_images(images)
    tiny.add_texts(ids, seg, mask, torch.from_numpy(g_tiny).to(DEV))

    def run(clf):
        ev = RetrievalEvaluator()
        ev.add_embeddings(V[:30], T[:100], g[:100])
        ev.add_embeddings(V[30:], T[100:], g[100:])
        clf.update_embeddings(V, labels)
        return (search(T, V, 10), search(V[:3], T, 64), ev.topk(10), tiny.search_texts(ids[:7], seg[:7], mask[:7], 5),
                tiny.search_images(images[:7], 5), clf)

    warm = run(ZeroShotClassifier(None, T[:29]))
    fresh = ZeroShotClassifier(None, T[:29])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = run(fresh)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(warm[:2] + warm[3:5], got[:2] + got[3:5]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for key in ("t2i", "i2t") for x, y in zip(warm[2][key], got[2][key]))
    assert warm[5].compute() == got[5].compute() and got[5].compute()["n"] == 67


def test_allocates_less_than_an_eighth_of_the_similarity_matrix():
    Nq, Nx, E, k = 4096, 2048, 512, 10
    gen = torch.Generator().manual_seed(9)
    X = torch.nn.functional.normalize(torch.randn(Nx, E, generator=gen), dim=1).to(DEV)
    Q = torch.nn.functional.normalize(torch.randn(Nq, E, generator=gen), dim=1).to(DEV)
    search(Q, X, k, normalise=False)
    torch.cuda.synchronize()   # warmed up: the library is loaded
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    idx, val = search(Q, X, k, normalise=False)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak above the inputs {peak} bytes; the similarity matrix {Nq * Nx * 4} bytes")
    assert peak < Nq * Nx * 4 // 8
    s64 = (Q[:64].double() @ X.double().T).cpu().numpy()   # spot check at this size: the first rows against fp64 on the device
    bad, share = tr.topk_valid(s64, idx[:64].cpu().numpy(), val[:64].cpu().numpy(), k, rr.dot_gap(E) / 2)
    print(f"determined share of the 64 rows {share:.3f}")
    assert bad == [], bad


def test_search_end_to_end_on_the_tiny_model():
    """search_texts / search_images in uneven chunks (chunk = 5 over 13 images and 29 captions) against search() on the
    embeddings of get_sequence_output / get_visual_output over the same chunks; the epoch driver with topk."""
    spec = synth.SPECS["tiny"]
    Ni, Nt, chunk, k = 13, 29, 5, 5
    model = tiny_seg_model()
    images, ids, seg, mask, g = _tiny_inputs(Ni, Nt)
    g_dev = torch.from_numpy(g).to(DEV)
    ev = RetrievalEvaluator(model, chunk=chunk)
    ev.add_images(images)
    ev.add_texts(ids, seg, mask, g_dev)
    with torch.no_grad():
        vis = torch.cat([model.get_visual_output(images[i:i + chunk]).squeeze(1) for i in range(0, Ni, chunk)])
        flat = lambda t, a, b: t[a:b].reshape(b - a, -1)
        seq = torch.cat([model.get_sequence_output(flat(ids, a, min(a + chunk, Nt)), flat(seg, a, min(a + chunk, Nt)),
                                                   flat(mask, a, min(a + chunk, Nt)), shaped=True).squeeze(1)
                         for a in range(0, Nt, chunk)])
    assert tuple(vis.shape) == (Ni, spec["embed_dim"]) and tuple(seq.shape) == (Nt, spec["embed_dim"])
    added = lambda: (sum(t.shape[0] for t in ev._visual), sum(t.shape[0] for t in ev._sequence))
    assert added() == (Ni, Nt)
    for got, want in ((ev.search_texts(ids, seg, mask, k), search(seq, vis, k)),
                      (ev.search_images(images, k), search(vis, seq, k)),
                      (ev.topk(k)["t2i"], search(seq, vis, k)), (ev.topk(k)["i2t"], search(vis, seq, k))):
        assert tuple(got[0].shape) == tuple(want[0].shape) and got[0].shape[1] == k
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))   # bit for bit
    assert added() == (Ni, Nt)                                 # the queries were not added
    idx, val = ev.topk(k)["t2i"]
    bad, _ = tr.topk_valid(tr.scores(ev._sequence[0].cpu().numpy(), ev._visual[0].cpu().numpy()), idx.cpu().numpy(),
                           val.cpu().numpy(), k, rr.dot_gap(spec["embed_dim"]) / 2)
    assert bad == [], bad

    batches = ([images[:10].cpu(), images[10:].cpu()],
               [(ids[:15].cpu(), seg[:15].cpu(), mask[:15].cpu(), torch.from_numpy(g[:15])),
                (ids[15:].cpu(), seg[15:].cpu(), mask[15:].cpu(), torch.from_numpy(g[15:]))])
    plain = eval_retrieval_epoch(None, model, DEV, *batches, chunk=chunk)
    epoch = eval_retrieval_epoch(None, model, DEV, *batches, chunk=chunk, topk=k)
    assert set(plain) == {"t2i", "i2t"} and plain == ev.compute()
    assert {key: epoch[key] for key in plain} == plain
    for key in ("t2i", "i2t"):
        for got, want in zip(epoch["topk"][key], ev.topk(k)[key]):
            assert not got.is_cuda and torch.equal(got, want.cpu())


def _hits(Q, X, labels, ks):
    idx, _ = tr.topk(Q, X, max(ks))
    return [int((idx[:, :K] == labels[:, None]).any(axis=1).sum()) for K in ks]


@pytest.mark.parametrize("classes,n", [(37, 101), (3, 13)])
def test_zero_shot_classifier_counts_exactly(classes, n):
    """exact_case embeddings (ties are real), seeded labels, two calls of uneven size; 3 classes: k = 5 > the class count"""
    C, S, _ = rr.exact_case(500 + classes, n, classes, 64)     # C (classes, E), S (n, E)
    labels = np.random.default_rng(classes).integers(0, classes, size=n)
    if classes >= 8:    # sample i is labelled with the class at place i % 8 of its row: hits at every place, and misses
        labels = tr.topk(S, C, 8)[0][np.arange(n), np.arange(n) % 8]
    top1, top5 = _hits(S, C, labels, (1, 5))
    assert 0 < top1 < top5 <= n
    Cd, Sd, lab = _dev(C, S, labels)
    clf = ZeroShotClassifier(None, Cd)
    clf.update_embeddings(Sd[:n // 3], lab[:n // 3], normalise=False)
    clf.update_embeddings(Sd[n // 3:], lab[n // 3:].to(torch.int32), normalise=False)
    assert clf.compute() == {"top1": 100.0 * top1 / n, "top5": 100.0 * top5 / n, "n": n}
    assert clf._hits.dtype == torch.int64 and clf._hits.is_cuda
    clf.reset()
    assert clf.compute()["n"] == 0


def test_zero_shot_classifier_on_the_tiny_model_and_a_bad_label():
    model = tiny_seg_model()
    images, ids, seg, mask, _ = _tiny_inputs()
    with torch.no_grad():
        text = ops.L2NormFn.apply(model.get_sequence_output(ids[:7].reshape(7, -1), seg[:7].reshape(7, -1),
                                                            mask[:7].reshape(7, -1), shaped=True).squeeze(1).float())
        vis = torch.cat([model.get_visual_output(images[i:i + 5]).squeeze(1) for i in range(0, 13, 5)])
    labels = torch.arange(13, device=DEV) % 7
    a, b = ZeroShotClassifier(model, text, chunk=5), ZeroShotClassifier(None, text)
    a.update(images, labels)
    b.update_embeddings(vis.float(), labels)
    assert torch.equal(a._hits, b._hits) and a.compute() == b.compute() and a.compute()["n"] == 13
    with pytest.raises(RuntimeError, match="needs the model"):
        b.update(images, labels)
    for bad in (7, -1):
        b.reset()
        labels[4] = bad
        b.update_embeddings(vis.float(), labels)         # found on the device: nothing raises before the host copy
        with pytest.raises(ValueError, match=r"labels.*7 classes"):
            b.compute()


def test_refusals():
    gen = torch.Generator().manual_seed(2)
    Q, X = torch.randn(8, 64, generator=gen).to(DEV), torch.randn(6, 64, generator=gen).to(DEV)
    for k in (0, 65):
        with pytest.raises(L.Unsupported, match=rf"\bk={k}\b"):
            search(Q, X, k)
    with pytest.raises(L.Unsupported, match=r"\bE=48\b"):
        search(Q[:, :48].contiguous(), X[:, :48].contiguous(), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        search(Q.cpu(), X.cpu(), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.retrieval_topk(Q, X.cpu(), 3)
    with pytest.raises(ValueError, match="equal E"):
        search(Q, X[:, :32].contiguous(), 3)
    with pytest.raises(ValueError, match="contiguous"):
        search(Q[:, ::2], X[:, :32].contiguous(), 3, normalise=False)
    with pytest.raises(TypeError, match="fp32"):
        ops.retrieval_topk(Q.double(), X.double(), 3)

    model = tiny_seg_model()
    batch = synth.synthetic_batch(synth.SPECS["tiny"], 2, seed=1, device=DEV)
    ev = RetrievalEvaluator(model)
    ev.add_images(batch["image"])
    ev.add_texts(batch["input_ids"], batch["segment_ids"], batch["input_mask"], torch.zeros(2, dtype=torch.int32, device=DEV))
    try:
        model.train()
        with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
            ev.search_images(batch["image"], 1)
        with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
            ev.search_texts(batch["input_ids"], batch["segment_ids"], batch["input_mask"], 1)
    finally:
        model.eval()
    with pytest.raises(RuntimeError, match="needs the model"):
        RetrievalEvaluator().search_images(batch["image"], 1)


def test_refuses_a_small_workspace_without_a_launch():
    Nq, Nx, E, k = 3, 5000, 64, 10
    X, Q, _ = rr.exact_case(100 + Nq, Nq, Nx, E)
    Qd, Xd = _dev(Q, X)
    lib = L.load()
    need = lib.segclip_retrieval_topk_ws_bytes(Nq, Nx, k, 0)
    assert need >= 128 * 2 * k * 8                              # few queries, many tiles: several partial lists
    assert lib.segclip_retrieval_topk_ws_bytes(Nq, Nx, 65, 0) == -2
    idx, val, ws = Frame((Nq, k), torch.int32), Frame((Nq, k), torch.float32), Frame((need // 8,), torch.int64)
    for ws_ptr, ws_bytes in ((ws.p, need - 8), (ctypes.c_void_p(None), need)):
        rc = lib.segclip_retrieval_topk(L.ptr(Qd), L.ptr(Xd), Nq, Nx, E, k, 0, idx.p, val.p, ws_ptr, ws_bytes, L.stream())
        torch.cuda.synchronize()
        assert rc == -1 and f"workspace_bytes={ws_bytes}".encode() in lib.segclip_last_error_string()
        assert idx.untouched() and val.untouched() and ws.untouched()
