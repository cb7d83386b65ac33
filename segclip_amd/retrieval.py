"""Image-text retrieval evaluation on the device: Recall@1/5/10, median rank and mean rank, text->image and image->text.

The reference trains "SegCLIP on Retrieval Task": its model carries get_similarity_logits / _loose_similarity for that
(modules/modeling.py:338-372) and its COCO loader builds the multi-caption layout an evaluation needs (sentences_dict,
cut_off_points, sentence_num, image_num, multi_sentence_per_image; dataloaders/dataloader_coco_retrieval.py:85-104), but it
ships no evaluator.  The definition is this project's (include/segclip_hip.h, tests/retrieval_reference.py):

    sim[t, j]   = <T[t], V[j]>                      L2-normalised caption and image embeddings; the logit scale is left out
    rank_t2i[t] = #{ j != g[t] : sim[t, j] > sim[t, g[t]] }                     0-based; a tie favours the ground truth
    rank_i2t[j] = #{ t : g[t] != j and sim[t, j] > best[j] },  best[j] = max{ sim[t, j] : g[t] == j };  -1 without captions
    R1, R5, R10 = 100 * share of ranks < K;  MedianR = median(rank + 1);  MeanR = mean(rank + 1)

The (Nt, Ni) similarity matrix never exists (csrc/retrieval.hip compares in the epilogue of the tile product), and nothing
synchronises with the host before compute().

What was retrieved, not only where the ground truth ranks: search() and RetrievalEvaluator.topk / search_texts / search_images
give, per query, the first k gallery rows under "higher score first, equal scores: lower index first" with their scores
(csrc/retrieval_topk.inc: the same tile product, the same bits, a selecting epilogue; positions from min(k, gallery size) on
hold idx = -1, val = -inf), again without the matrix.  ZeroShotClassifier is its small consumer: the gallery is the class
embeddings, and top-1 / top-5 accuracy is counted on the device.
"""
import torch

from . import ops

L = ops.L
KS = (1, 5, 10)


def image_index_from_cut_off_points(cut_off_points):
    """The loader's cut_off_points (dataloaders/dataloader_coco_retrieval.py:86-92: the number of sentences up to and including
    image i) -> the (Nt,) int32 CPU tensor g with g[t] = the image of sentence t.  An image may have no sentence."""
    cuts = torch.as_tensor(cut_off_points, dtype=torch.int64).reshape(-1).cpu()
    counts = torch.diff(cuts, prepend=torch.zeros(1, dtype=torch.int64))
    if cuts.numel() and (int(cuts[0]) < 0 or bool((counts < 0).any())):
        raise ValueError("cut_off_points: the running sentence counts do not decrease and start at 0 or above")
    return torch.repeat_interleave(torch.arange(cuts.numel(), dtype=torch.int32), counts)


def metrics_from_hist(hist):
    """(bins,) integer CPU tensor, hist[r] = the number of queries of 0-based rank r -> dict(R1, R5, R10, MedianR, MeanR),
    exactly what the rank vector gives: R@K = 100 * share of ranks < K, MedianR = median(rank + 1), MeanR = mean(rank + 1)."""
    if hist.is_cuda:
        raise ValueError("metrics_from_hist takes a CPU copy of the histogram (hist.cpu())")
    h = hist.reshape(-1).to(torch.int64)
    n = int(h.sum())
    if n == 0:
        return dict({f"R{k}": float("nan") for k in KS}, MedianR=float("nan"), MeanR=float("nan"))
    cum = torch.cumsum(h, 0)

    def at(p):   # the p-th smallest rank
        return int(torch.searchsorted(cum, torch.tensor(p, dtype=torch.int64), right=True))

    out = {f"R{k}": 100.0 * (int(h[:k].sum()) / n) for k in KS}
    out["MedianR"] = (at((n - 1) // 2) + 1 + at(n // 2) + 1) / 2.0
    out["MeanR"] = int((h * torch.arange(1, h.numel() + 1, dtype=torch.int64)).sum()) / n
    return out


@torch.no_grad()
def search(queries, gallery, k, normalise=True):
    """queries (Nq, E), gallery (Nx, E), fp32 on the device -> (idx (Nq, k) int32, val (Nq, k) fp32): the k best gallery rows of
    every query, best first, a tie going to the lower index; val[q, p] = <queries[q], gallery[idx[q, p]]> of the L2-normalised
    rows (normalise=False: of the rows as they are).  1 <= k <= 64.  Nothing synchronises."""
    L.require_cuda(queries, gallery)
    if normalise:
        for name, t in (("queries", queries), ("gallery", gallery)):
            if t.dim() != 2 or t.dtype != torch.float32:
                raise ValueError(f"{name} is an (N, E) fp32 tensor, got {t.dtype} {tuple(t.shape)}")
        queries, gallery = ops.L2NormFn.apply(queries), ops.L2NormFn.apply(gallery)
    return ops.retrieval_topk(queries, gallery, k)


class RetrievalEvaluator:
    """Collects L2-normalised image and caption embeddings on the device and ranks them with the three retrieval kernels.

    add_images / add_texts run the model's towers `chunk` rows at a time; add_embeddings takes ready embeddings (several
    ranks: gather them first).  image_index numbers the images in the order they were added, over all calls.  ranks() and
    compute() work on everything added since the last reset()."""

    def __init__(self, model=None, chunk=256):
        if int(chunk) < 1:
            raise ValueError(f"chunk is at least 1, got {chunk}")
        self.model, self.chunk = model, int(chunk)
        self.reset()

    def reset(self):
        self._visual, self._sequence, self._index = [], [], []
        self._status = None
        self._result = self._topk = None

    def _towers(self, what):
        if self.model is None:
            raise RuntimeError(f"RetrievalEvaluator.{what} needs the model; this evaluator takes add_embeddings only")
        if self.model.training:
            raise RuntimeError("segclip_amd.retrieval: call model.eval() first (training mode masks and draws Gumbel noise)")
        return self.model

    @torch.no_grad()
    def add_images(self, image):
        """image: (B, 1, 3, H, W) as the loader gives it, or (B, 3, H, W)."""
        L.require_cuda(image)
        model = self._towers("add_images")
        shaped = image.dim() == 4
        for i in range(0, image.shape[0], self.chunk):
            v = model.get_visual_output(image[i:i + self.chunk].contiguous(), shaped=shaped)
            self.add_embeddings(visual=v.squeeze(1).float())

    @torch.no_grad()
    def add_texts(self, input_ids, token_type_ids, attention_mask, image_index):
        """input_ids, token_type_ids, attention_mask: (B, L) or (B, 1, L); image_index: (B,) the image of every caption."""
        L.require_cuda(input_ids, image_index)
        model = self._towers("add_texts")
        image_index = image_index.reshape(-1)
        if image_index.shape[0] != input_ids.shape[0]:
            raise ValueError(f"image_index: {image_index.shape[0]} entries for {input_ids.shape[0]} captions")
        flat = lambda t: None if t is None else t.reshape(-1, t.shape[-1])
        ids, tt, am = flat(input_ids), flat(token_type_ids), flat(attention_mask)
        for i in range(0, ids.shape[0], self.chunk):
            cut = lambda t: None if t is None else t[i:i + self.chunk].contiguous()
            s = model.get_sequence_output(cut(ids), cut(tt), cut(am), shaped=True)
            self.add_embeddings(sequence=s.squeeze(1).float(), image_index=image_index[i:i + self.chunk])

    @torch.no_grad()
    def add_embeddings(self, visual=None, sequence=None, image_index=None, normalise=True):
        """visual (Ni, E) and / or sequence (Nt, E) with image_index (Nt,), fp32 on the device.  normalise=False takes the rows
        as they are (they are already unit vectors, or the caller wants the plain dot products ranked) and keeps the tensors
        themselves instead of copies."""
        if (sequence is None) != (image_index is None):
            raise ValueError("sequence and image_index go together")
        L.require_cuda(visual, sequence, image_index)
        for name, t in (("visual", visual), ("sequence", sequence)):
            if t is not None and (t.dim() != 2 or t.dtype != torch.float32):
                raise ValueError(f"{name} is an (N, E) fp32 tensor, got {t.dtype} {tuple(t.shape)}")
        if image_index is not None:
            if image_index.dtype not in (torch.int32, torch.int64) or tuple(image_index.shape) != (sequence.shape[0],):
                raise ValueError(f"image_index is an (Nt,) int32 or int64 tensor, got {image_index.dtype} {tuple(image_index.shape)}")
            lo, hi = -(1 << 31), (1 << 31) - 1   # an int64 index beyond int32 stays out of range after the cast
            image_index = image_index.clamp(lo, hi).to(torch.int32) if image_index.dtype == torch.int64 else image_index
        norm = (lambda t: ops.L2NormFn.apply(t)) if normalise else (lambda t: t.detach())
        if visual is not None and visual.shape[0]:
            self._visual.append(norm(visual))
        if sequence is not None and sequence.shape[0]:
            self._sequence.append(norm(sequence))
            self._index.append(image_index)
        self._result = self._topk = None

    @staticmethod
    def _joined(parts):
        if len(parts) > 1:
            parts[:] = [torch.cat(parts)]
        return parts[0]

    def _run(self):
        if self._result is None:
            if not self._visual or not self._sequence:
                raise ValueError("RetrievalEvaluator: add images and captions first")
            V, T, g = self._joined(self._visual), self._joined(self._sequence), self._joined(self._index)
            if self._status is None:
                self._status = torch.zeros(1, dtype=torch.int32, device=V.device)
            thr, best, n_cap = ops.retrieval_thresholds(V, T, g, self._status)
            rank_t2i, rank_i2t = ops.retrieval_count(V, T, g, thr, best)
            hist_t2i, hist_i2t = ops.retrieval_hist(rank_t2i, rank_i2t, n_cap)
            self._result = (rank_t2i, rank_i2t, hist_t2i, hist_i2t)
        return self._result

    def ranks(self):
        """-> (rank_t2i (Nt,), rank_i2t (Ni,)) int32 on the device; rank_i2t is -1 for an image without captions."""
        return self._run()[:2]

    def hists(self):
        """-> (hist_t2i (Ni,), hist_i2t (Nt + 1,)) int64 on the device: the number of queries at every rank."""
        return self._run()[2:]

    def topk(self, k):
        """-> {"t2i": (idx (Nt, k), val (Nt, k)), "i2t": (idx (Ni, k), val (Ni, k))}: the k best images of every caption and
        the k best captions of every image added, on the device, from the very tensors ranks() reads (search())."""
        k = int(k)
        if self._topk is None or self._topk[0] != k:
            if not self._visual or not self._sequence:
                raise ValueError("RetrievalEvaluator: add images and captions first")
            V, T = self._joined(self._visual), self._joined(self._sequence)
            self._topk = (k, {"t2i": ops.retrieval_topk(T, V, k), "i2t": ops.retrieval_topk(V, T, k)})
        return self._topk[1]

    def _searched(self, embed, n, parts, what, k):
        """the rows of `embed(i, j)` for [i, j) in chunks, normalised, against everything in `parts`"""
        if not parts:
            raise ValueError(f"RetrievalEvaluator: add {what} first")
        q = [ops.L2NormFn.apply(embed(i, min(i + self.chunk, n)).squeeze(1).float()) for i in range(0, n, self.chunk)]
        q = q or [parts[0].new_empty((0, parts[0].shape[1]))]
        return ops.retrieval_topk(torch.cat(q) if len(q) > 1 else q[0], self._joined(parts), k)

    @torch.no_grad()
    def search_texts(self, input_ids, token_type_ids, attention_mask, k):
        """Captions as add_texts takes them -> (idx (B, k), val (B, k)) over the images added; the captions are not added."""
        L.require_cuda(input_ids)
        model = self._towers("search_texts")
        flat = lambda t: None if t is None else t.reshape(-1, t.shape[-1])
        ids, tt, am = flat(input_ids), flat(token_type_ids), flat(attention_mask)
        cut = lambda t, i, j: None if t is None else t[i:j].contiguous()
        embed = lambda i, j: model.get_sequence_output(cut(ids, i, j), cut(tt, i, j), cut(am, i, j), shaped=True)
        return self._searched(embed, ids.shape[0], self._visual, "images", k)

    @torch.no_grad()
    def search_images(self, image, k):
        """Images as add_images takes them -> (idx (B, k), val (B, k)) over the captions added; the images are not added."""
        L.require_cuda(image)
        model = self._towers("search_images")
        shaped = image.dim() == 4
        embed = lambda i, j: model.get_visual_output(image[i:j].contiguous(), shaped=shaped)
        return self._searched(embed, image.shape[0], self._sequence, "captions", k)

    def compute(self):
        """-> {"t2i": {R1, R5, R10, MedianR, MeanR}, "i2t": {...}}.  The one host copy: both histograms and the status word."""
        hist_t2i, hist_i2t = self.hists()
        host = torch.cat([hist_t2i, hist_i2t, self._status.to(torch.int64)]).cpu()
        if int(host[-1]) & ops.RETRIEVAL_BAD_INDEX:
            raise ValueError(f"image_index: an entry lies outside [0, Ni) with Ni = {hist_t2i.shape[0]} images added")
        n = hist_t2i.shape[0]
        return {"t2i": metrics_from_hist(host[:n]), "i2t": metrics_from_hist(host[n:-1])}


ZEROSHOT_BAD_LABEL = 1   # status bit of ZeroShotClassifier: a label outside [0, classes)


class ZeroShotClassifier:
    """Zero-shot classification accuracy: the gallery of the search is the class embeddings.

    text_embedding: (classes, E), what segmentation.build_text_embedding returns (one row per class, the mean over the
    prompt templates, L2-normalised there and taken as it is).  update(image, labels) runs the vision tower `chunk` images
    at a time; update_embeddings(visual, labels) takes ready embeddings.  A sample is a top-K hit when its label is among the
    first K classes search() returns (a tie goes to the lower class).  The counters stay on the device; compute() makes the
    one host copy."""

    def __init__(self, model, text_embedding, ks=(1, 5), chunk=256):
        if int(chunk) < 1:
            raise ValueError(f"chunk is at least 1, got {chunk}")
        ks = tuple(int(k) for k in ks)
        if not ks or min(ks) < 1 or max(ks) > 64:
            raise ValueError(f"ks: top-K sizes in [1, 64], got {ks}")
        L.require_cuda(text_embedding)
        if text_embedding.dim() != 2 or text_embedding.shape[0] < 1:
            raise ValueError(f"text_embedding is a (classes, E) tensor, got {tuple(text_embedding.shape)}")
        self.model, self.ks, self.chunk = model, ks, int(chunk)
        self.classes = text_embedding.detach().float().contiguous()
        self._places = torch.tensor(ks, dtype=torch.int64, device=text_embedding.device)
        self.reset()

    def reset(self):
        dev = self.classes.device
        self._hits = torch.zeros(len(self.ks), dtype=torch.int64, device=dev)
        self._status = torch.zeros(1, dtype=torch.int64, device=dev)
        self._n = 0

    @torch.no_grad()
    def update_embeddings(self, visual, labels, normalise=True):
        """visual (B, E) fp32 and labels (B,) int32 or int64 on the device.  normalise=False takes the rows as they are."""
        L.require_cuda(visual, labels)
        if labels.dtype not in (torch.int32, torch.int64) or labels.dim() != 1 or visual.dim() != 2 \
                or labels.shape[0] != visual.shape[0]:
            raise ValueError(f"visual (B, E) and labels (B,) int32 or int64; got {tuple(visual.shape)}, {labels.dtype} "
                             f"{tuple(labels.shape)}")
        if visual.dtype != torch.float32:
            raise ValueError(f"visual is a (B, E) fp32 tensor, got {visual.dtype}")
        idx, _ = ops.retrieval_topk(ops.L2NormFn.apply(visual) if normalise else visual, self.classes, max(self.ks))
        labels = labels.to(torch.int64)
        place = (idx.to(torch.int64) == labels[:, None]).to(torch.int64).cumsum(1)   # 1 from the label's place on (idx >= -1)
        inside = (labels >= 0) & (labels < self.classes.shape[0])
        hit = place[:, self._places - 1] * inside[:, None]
        self._hits += hit.sum(0)
        self._status |= (~inside).any().to(torch.int64) * ZEROSHOT_BAD_LABEL
        self._n += visual.shape[0]

    @torch.no_grad()
    def update(self, image, labels):
        """image: (B, 1, 3, H, W) or (B, 3, H, W); labels: (B,)."""
        L.require_cuda(image, labels)
        if self.model is None:
            raise RuntimeError("ZeroShotClassifier.update needs the model; this classifier takes update_embeddings only")
        if self.model.training:
            raise RuntimeError("segclip_amd.retrieval: call model.eval() first (training mode masks and draws Gumbel noise)")
        if labels.dim() != 1 or labels.shape[0] != image.shape[0]:
            raise ValueError(f"labels: {tuple(labels.shape)} for {image.shape[0]} images")
        shaped = image.dim() == 4
        for i in range(0, image.shape[0], self.chunk):
            v = self.model.get_visual_output(image[i:i + self.chunk].contiguous(), shaped=shaped)
            self.update_embeddings(v.squeeze(1).float(), labels[i:i + self.chunk])

    def compute(self):
        """-> {"top1": ..., "top5": ..., "n": samples} in percent (one entry per K of ks).  The one host copy."""
        host = torch.cat([self._hits, self._status]).cpu()
        if int(host[-1]) & ZEROSHOT_BAD_LABEL:
            raise ValueError(f"labels: an entry lies outside [0, classes) with {self.classes.shape[0]} classes")
        out = {f"top{k}": (100.0 * int(h) / self._n if self._n else float("nan")) for k, h in zip(self.ks, host[:-1])}
        out["n"] = self._n
        return out
