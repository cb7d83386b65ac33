"""The yardstick of the retrieval evaluation: numpy, fp64.  The reference ships no retrieval evaluator, so the definition is
this project's (segclip_amd/retrieval.py, include/segclip_hip.h) and is restated here.

    V (Ni, E) image embeddings, T (Nt, E) caption embeddings, g (Nt,) the image of every caption (any number per image)
    sim[t, j]   = <T[t], V[j]>
    rank_t2i[t] = #{ j != g[t] : sim[t, j] > sim[t, g[t]] }                     0-based, strict: a tie favours the ground truth
    rank_i2t[j] = #{ t : g[t] != j and sim[t, j] > best[j] },  best[j] = max{ sim[t, j] : g[t] == j };  -1 without captions
    R1, R5, R10 = 100 * share of ranks < K;  MedianR = np.median(rank + 1);  MeanR = mean(rank + 1);  ranks of -1 left out
"""
import numpy as np

KS = (1, 5, 10)


def similarity(V, T):
    return np.asarray(T, dtype=np.float64) @ np.asarray(V, dtype=np.float64).T


def ranks(V, T, g, gap=0.0):
    """-> (rank_t2i (Nt,), rank_i2t (Ni,)) int64.  gap shifts both thresholds: #{sim > threshold + gap}."""
    sim = similarity(V, T)
    Nt, Ni = sim.shape
    g = np.asarray(g, dtype=np.int64)
    thr = sim[np.arange(Nt), g]
    other = g[:, None] != np.arange(Ni)[None, :]
    rank_t2i = (other & (sim > thr[:, None] + gap)).sum(axis=1)
    best = np.full(Ni, -np.inf)
    np.maximum.at(best, g, thr)
    rank_i2t = (other & (sim > best[None, :] + gap)).sum(axis=0)
    rank_i2t[np.bincount(g, minlength=Ni) == 0] = -1
    return rank_t2i.astype(np.int64), rank_i2t.astype(np.int64)


def rank_intervals(V, T, g, gap):
    """The ranks a computation with an absolute error below gap / 2 per dot product may give: (lo_t2i, hi_t2i, lo_i2t, hi_i2t),
    lo = #{sim > thr + gap}, hi = #{sim > thr - gap}."""
    lo_t, lo_i = ranks(V, T, g, gap)
    hi_t, hi_i = ranks(V, T, g, -gap)
    return lo_t, hi_t, lo_i, hi_i


def ranks_by_argsort(V, T, g):
    """The second definition: the position of the ground truth in the stable descending order of the candidates, the ground
    truth moved in front of its ties.  For an image the ground truth is its best caption."""
    sim = similarity(V, T)
    Nt, Ni = sim.shape
    g = np.asarray(g, dtype=np.int64)
    rank_t2i = np.zeros(Nt, dtype=np.int64)
    for t in range(Nt):
        cand = np.concatenate([[g[t]], np.delete(np.arange(Ni), g[t])])
        order = cand[np.argsort(-sim[t, cand], kind="stable")]
        rank_t2i[t] = int(np.nonzero(order == g[t])[0][0])
    rank_i2t = np.full(Ni, -1, dtype=np.int64)
    for j in range(Ni):
        own = np.nonzero(g == j)[0]
        if own.size == 0:
            continue
        cand = np.concatenate([own, np.nonzero(g != j)[0]])
        order = cand[np.argsort(-sim[cand, j], kind="stable")]
        rank_i2t[j] = int(np.nonzero(g[order] == j)[0][0])
    return rank_t2i, rank_i2t


def metrics(rank):
    r = np.asarray(rank, dtype=np.int64)
    r = r[r >= 0]
    out = {f"R{k}": 100.0 * float(np.mean(r < k)) for k in KS}
    out["MedianR"] = float(np.median(r + 1))
    out["MeanR"] = float(np.mean(r + 1))
    return out


def hists(rank_t2i, rank_i2t):
    """-> (hist_t2i (Ni,), hist_i2t (Nt + 1,)) int64: the number of queries at every rank."""
    rank_t2i, rank_i2t = np.asarray(rank_t2i), np.asarray(rank_i2t)
    Nt, Ni = rank_t2i.shape[0], rank_i2t.shape[0]
    return (np.bincount(rank_t2i, minlength=Ni).astype(np.int64),
            np.bincount(rank_i2t[rank_i2t >= 0], minlength=Nt + 1).astype(np.int64))


# ---------------------------------------------------------------- seeded inputs shared by the CPU and the GPU tests
def caption_index(rng, Nt, Ni, tile=128):
    """g with 0..7 captions per image, Nt in all, in shuffled order.  Image 1 has none (Ni >= 3); the first and the last image
    of every tile of `tile` images have at least one, where Nt allows."""
    counts = rng.integers(0, 8, size=Ni)
    must = sorted({j for j in list(range(0, Ni, tile)) + list(range(tile - 1, Ni, tile)) + [Ni - 1] if Ni < 3 or j != 1})[:Nt]
    counts[must] = np.maximum(counts[must], 1)
    frozen = 1 if Ni >= 3 else -1
    if frozen >= 0:
        counts[frozen] = 0
    free = np.array([j for j in range(Ni) if j != frozen])
    assert len(must) <= Nt <= 7 * free.size
    while counts.sum() > Nt:
        j = rng.choice(free)
        if counts[j] > (1 if j in must else 0):
            counts[j] -= 1
    while counts.sum() < Nt:
        j = rng.choice(free)
        if counts[j] < 7:
            counts[j] += 1
    return rng.permutation(np.repeat(np.arange(Ni), counts)).astype(np.int32)


def exact_case(seed, Nt, Ni, E):
    """Entries that are multiples of 1/8 in [-1, 1]: every dot product is exact in fp32 in any order, and ties are real.  A
    quarter of the images and of the captions are copies of others, and one image is a copy of caption 0's own image: rows
    and columns have ties above, below and at the threshold."""
    rng = np.random.default_rng(seed)
    V = rng.integers(-8, 9, size=(Ni, E)).astype(np.float32) / 8
    T = rng.integers(-8, 9, size=(Nt, E)).astype(np.float32) / 8
    g = caption_index(rng, Nt, Ni)
    if Ni >= 8:
        for _ in range(Ni // 4):
            a, b = rng.choice(Ni, size=2, replace=False)
            V[a] = V[b]
        V[(g[0] + 2) % Ni] = V[g[0]]
    if Nt >= 8:
        for _ in range(Nt // 4):
            a, b = rng.choice(Nt, size=2, replace=False)
            T[a] = T[b]
    return V, T, g


def realistic_case(seed, Nt, Ni, E, hard=0.15):
    """Random unit image vectors; a caption is its image's vector plus noise, small for most captions and of 5 to 30 times
    the vector's length for a share `hard` of them, whose ranks then spread from 0 to far beyond 10."""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((Ni, E))
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    g = caption_index(rng, Nt, Ni)
    sigma = np.where(rng.random(Nt) < hard, rng.uniform(5.0, 30.0, size=Nt), 1.0)
    noise = rng.standard_normal((Nt, E)) / np.sqrt(E)
    T = V[g] + sigma[:, None] * noise
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    return V.astype(np.float32), T.astype(np.float32), g


def dot_gap(E):
    """2 E 2^-24: the fp32 dot-product error bound for unit vectors, twice because two dot products are compared."""
    return 2.0 * E * 2.0 ** -24
