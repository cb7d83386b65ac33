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
        self._result = None

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
        self._result = None

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

    def compute(self):
        """-> {"t2i": {R1, R5, R10, MedianR, MeanR}, "i2t": {...}}.  The one host copy: both histograms and the status word."""
        hist_t2i, hist_i2t = self.hists()
        host = torch.cat([hist_t2i, hist_i2t, self._status.to(torch.int64)]).cpu()
        if int(host[-1]) & ops.RETRIEVAL_BAD_INDEX:
            raise ValueError(f"image_index: an entry lies outside [0, Ni) with Ni = {hist_t2i.shape[0]} images added")
        n = hist_t2i.shape[0]
        return {"t2i": metrics_from_hist(host[:n]), "i2t": metrics_from_hist(host[n:-1])}
