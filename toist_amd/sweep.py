"""Task sweep: many captions over one image pass (host side).

TOIST asks "which object would I use to <task>" for 14 tasks per image (COCO-Tasks), and the reference's loader makes one sample per (image, task):
the ResNet runs once per pair, RoBERTa too (datasets/tdod.py + engine.py:253-342).  Neither depends on the other input.  A sweep of T captions over
B images runs B image passes (MDETR.sweep_images), T text passes (MDETR.sweep_text) and one pair stage over P (image, caption) pairs
(MDETR.sweep_pairs: toist_sweep_assemble + the cross-modal encoder); the decoder and PostProcess see an ordinary batch of P rows.

This module holds what the host does around it: the pair tables, the per-pair view of the tokenized captions, and the keying of the results.
Shared: backbone, input_proj, position encoding (per image); RoBERTa, resizer (per caption).  Not shared: encoder, decoder, heads, PostProcess."""
import torch

from .transformer import TokenizedText


class SweepImages:
    """What MDETR.sweep_images keeps of a batch of images: tok / pos bf16 [B, HW, d], mask bool [B, h, w], feats (the backbone's NHWC maps)."""

    __slots__ = ("tok", "pos", "mask", "feats")

    def __init__(self, tok, pos, mask, feats):
        self.tok, self.pos, self.mask, self.feats = tok, pos, mask, feats


def _index_list(v, what):
    if torch.is_tensor(v):
        if v.dim() != 1 or v.dtype.is_floating_point or v.dtype == torch.bool:
            raise ValueError(f"{what} must be a vector of integers")
        v = v.tolist()
    out = []
    for x in v:
        if isinstance(x, bool) or int(x) != x:
            raise ValueError(f"{what} must hold integers (got {x!r})")
        out.append(int(x))
    return out


def check_tables(pair_image, pair_caption, n_images, n_captions):
    """Host check of two pair tables (lists or host tensors) -> (pair_image, pair_caption) as int32 host tensors; ValueError when they are empty, differ
    in length or name an image outside [0, n_images) / a caption outside [0, n_captions)."""
    pi, pc = _index_list(pair_image, "pair_image"), _index_list(pair_caption, "pair_caption")
    if not pi or len(pi) != len(pc):
        raise ValueError(f"pair tables must be non-empty and of one length (got {len(pi)} images, {len(pc)} captions)")
    for p, (i, t) in enumerate(zip(pi, pc)):
        if not 0 <= i < n_images or not 0 <= t < n_captions:
            raise ValueError(f"pair {p} = (image {i}, caption {t}) is outside the sweep's {n_images} images x {n_captions} captions")
    return torch.tensor(pi, dtype=torch.int32), torch.tensor(pc, dtype=torch.int32)


def device_tables(pair_image, pair_caption, n_images, n_captions, device):
    """The two pair tables as the launches take them -> (pair_image, pair_caption int32 on the device, pair_caption on the host or None).  Lists and
    host tensors: check_tables (ValueError), then two uploads that nothing waits for.  int32 DEVICE vectors pass as they are -- the launch that
    reads them checks them -- and the host knows nothing of them: None."""
    if torch.is_tensor(pair_image) and pair_image.is_cuda:
        return pair_image, pair_caption, None
    pi, pc = check_tables(pair_image, pair_caption, n_images, n_captions)
    return pi.to(device, non_blocking=True), pc.to(device, non_blocking=True), pc


def pair_tables(n_images, n_captions, pairs=None, capacity=None):
    """-> (pair_image int32 [P], pair_caption int32 [P], live): the tables toist_sweep_assemble reads, on the host.
    pairs=None: the full product, image-major (p = i * n_captions + t); else the explicit list of (image, caption), in its order, repeats allowed.
    capacity: P = capacity, the rows behind the `live` real pairs are the pair (0, 0) (a captured step has one table size; keyed_results drops them).
    ValueError: no image / caption / pair, an index out of range, more pairs than capacity."""
    n_images, n_captions = int(n_images), int(n_captions)
    if n_images <= 0 or n_captions <= 0:
        raise ValueError(f"a sweep needs at least one image and one caption (got {n_images} x {n_captions})")
    if pairs is None:
        pi = [i for i in range(n_images) for _ in range(n_captions)]
        pc = [t for _ in range(n_images) for t in range(n_captions)]
    else:
        pairs = list(pairs)
        if any(len(tuple(pr)) != 2 for pr in pairs):
            raise ValueError("pairs is a list of (image, caption)")
        pi, pc = [pr[0] for pr in pairs], [pr[1] for pr in pairs]
    pi, pc = check_tables(pi, pc, n_images, n_captions)
    live = int(pi.numel())
    if capacity is not None:
        capacity = int(capacity)
        if live > capacity:
            raise ValueError(f"{live} pairs do not fit a capacity of {capacity}")
        pad = torch.zeros(capacity - live, dtype=torch.int32)
        pi, pc = torch.cat([pi, pad]), torch.cat([pc, pad])
    return pi, pc, live


def pair_passes(n_pairs, pairs_per_pass):
    """The (lo, hi) slices of P pairs that the mask program of a sweep runs one after the other: at most `pairs_per_pass` pairs each, in table order,
    the last one holding the remainder.  The per-map intermediates of a pass are what the step holds at a time (DETRsegm.decode_mask_sweep).
    ValueError: no pair, or a pass size that is not a positive integer."""
    if isinstance(n_pairs, bool) or isinstance(pairs_per_pass, bool) or int(n_pairs) != n_pairs or int(pairs_per_pass) != pairs_per_pass:
        raise ValueError(f"pair_passes: whole numbers of pairs (got {n_pairs!r} pairs, {pairs_per_pass!r} per pass)")
    n_pairs, pairs_per_pass = int(n_pairs), int(pairs_per_pass)
    if n_pairs <= 0 or pairs_per_pass <= 0:
        raise ValueError(f"pair_passes: {n_pairs} pairs in passes of {pairs_per_pass}: both must be positive")
    return [(lo, min(lo + pairs_per_pass, n_pairs)) for lo in range(0, n_pairs, pairs_per_pass)]


class SweepTokenized(TokenizedText):
    """The tokenized captions of a sweep as the pairs see them: input_ids / attention_mask hold caption pair_caption[p] in row p, and
    char_to_token(p, c) answers for that caption -- ClusterCriterion.infer_choice finds the word 'something' of every pair through it."""

    def __init__(self, captions, pair_caption=None):
        if pair_caption is None:                       # TokenizedText.to(): type(self)({...}) on the rows of an existing instance
            super().__init__(captions)
            return
        rows = pair_caption.tolist() if torch.is_tensor(pair_caption) else [int(t) for t in pair_caption]
        n = captions["input_ids"].shape[0]
        if any(not 0 <= t < n for t in rows):
            raise ValueError(f"pair_caption names a caption outside the {n} tokenized ones")
        index = torch.tensor(rows, dtype=torch.int64, device=captions["input_ids"].device)
        super().__init__({"input_ids": captions["input_ids"].index_select(0, index), "attention_mask": captions["attention_mask"].index_select(0, index)})
        object.__setattr__(self, "_captions", captions)
        object.__setattr__(self, "_rows", rows)

    def char_to_token(self, batch_or_char, char=None):
        base = self.__dict__.get("_captions")
        if base is None or not hasattr(base, "char_to_token"):
            raise AttributeError("the sweep's tokenized captions do not answer char_to_token (pass a tokenizer's BatchEncoding, or captions as strings)")
        if char is None:                               # (a BatchEncoding reads one argument as a character of row 0)
            return base.char_to_token(self._rows[0], batch_or_char)
        return base.char_to_token(self._rows[batch_or_char], char)

    def to(self, device):
        out = SweepTokenized({k_: (v.to(device) if torch.is_tensor(v) else v) for k_, v in self.items()})
        for name in ("_captions", "_rows"):
            if name in self.__dict__:
                object.__setattr__(out, name, self.__dict__[name])
        return out


def keyed_results(results, image_ids, task_names, pair_image, pair_caption, live=None):
    """PostProcess results of the P pairs -> {(image_id, task_name): result}.  Rows from `live` on are padding and are dropped; a pair listed twice
    keeps its last row."""
    pi, pc = _index_list(pair_image, "pair_image"), _index_list(pair_caption, "pair_caption")
    live = len(pi) if live is None else int(live)
    if len(pc) != len(pi) or live > len(pi) or len(results) < live:
        raise ValueError(f"{len(results)} results, tables of {len(pi)} and {len(pc)} pairs, {live} of them live")
    out = {}
    for p in range(live):
        image_id = image_ids[pi[p]]
        out[(int(image_id) if torch.is_tensor(image_id) else image_id, task_names[pc[p]])] = results[p]
    return out
