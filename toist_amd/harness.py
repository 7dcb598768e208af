"""Synthetic-input harness shared by bench.py, __graft_entry__.smoke() and the tests: default args
(the flag defaults of /root/reference/main.py:32-274), the synthetic batches of SURVEY.md 8(d), the finite-loss guard and the evaluation loop.
The steps replayed from hipGraphs live in captured.py; their names are re-exported here (harness.CapturedTrainStep, ...)."""
from types import SimpleNamespace

import torch

from .captured import (CapturedDistillStep, CapturedEvalStep, CapturedMaskPairTrainStep, CapturedMaskSweepStep, CapturedPairTrainStep,  # noqa: F401
                       CapturedSweepStep, CapturedTrainStep, size_pairs)
from .transformer import TokenizedText


def default_args(**over):
    a = dict(
        device="cuda", masks=False, mask_model="none", frozen_weights=None, num_queries=100, aux_loss=True,
        contrastive_loss_hdim=64, contrastive_align_loss=False, contrastive_loss=False, cluster_num=3, dec_layers=6, enc_layers=6,
        eos_coef=0.1, temperature_NCE=0.07, hidden_dim=256, nheads=8, dim_feedforward=2048, dropout=0.1, pre_norm=False,
        pass_pos_and_query=True, text_encoder_type="roberta-base", freeze_text_encoder=False, without_pretrain=True,
        ce_loss_coef=1.0, bbox_loss_coef=5.0, giou_loss_coef=2.0, mask_loss_coef=1.0, dice_loss_coef=1.0,
        contrastive_align_loss_coef=1.0, set_loss="hungarian", set_cost_class=1.0, set_cost_bbox=5.0, set_cost_giou=2.0,
        lr_backbone=1e-5, backbone="resnet101", dilation=False, position_embedding="sine", nsthl2_loss=False, softkd_loss=False,
        cluster=False, distillation=False, lr=1e-4, text_encoder_lr=5e-5, weight_decay=1e-4, clip_max_norm=0.1,
        nsthl2_coef=1e4, softkd_coef=1.0, cluster_choice_loss=0.0, cluster_feature_loss=1e4, cluster_memory_size=1024, fifo_memory=False,
        train_batch_size=4,
    )
    a.update(over)
    return SimpleNamespace(**a)


def finite_or_exit(loss_value, loss_dict=None, criterion=None):
    """The NaN / inf guard of the reference loop (engine.py:82-85, 212-215): print the losses and sys.exit(1).  When the criterion is
    given, an invalid matcher cost block is reported as the ValueError SciPy raises in the reference (matcher.py:85)."""
    import math
    import sys
    v = float(loss_value)
    from . import kernels
    kernels.xdec_check()        # (the float() above synchronised) a group of an XCD-resident launch that was not co-resident gave up waiting: results invalid
    if math.isfinite(v):
        return v
    if criterion is not None:
        criterion.check_status()
    print("Loss is {}, stopping training".format(v))
    if loss_dict is not None:
        print({k: float(x) for k, x in loss_dict.items()})
    sys.exit(1)


def _box_masks(boxes, height, width):
    """One rectangle per normalised cxcywh box, at least one pixel -> bool [t, height, width]."""
    m = torch.zeros(len(boxes), height, width, dtype=torch.bool)
    for j in range(len(boxes)):
        x0, y0 = int((boxes[j, 0] - boxes[j, 2] / 2) * width), int((boxes[j, 1] - boxes[j, 3] / 2) * height)
        x1, y1 = int((boxes[j, 0] + boxes[j, 2] / 2) * width), int((boxes[j, 1] + boxes[j, 3] / 2) * height)
        m[j, max(y0, 0):max(y1, 1), max(x0, 0):max(x1, 1)] = True
    return m


def synthetic_batch(batch, height=640, width=640, tokens=16, seed=1000, device="cpu", max_targets=10, with_masks=False):
    """Images ~ N(0,1) (already normalised), all-False padding mask; captions = <s> + ids + </s>;
    T_i ~ U{0..max_targets} boxes with cx,cy~U(.2,.8), w,h~U(.05,.4); positive_map rows = 1/(tokens-2)
    on the caption tokens."""
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(batch, 3, height, width, generator=g)
    mask = torch.zeros(batch, height, width, dtype=torch.bool)
    ids = torch.randint(3, 50265, (batch, tokens), generator=g)
    ids[:, 0], ids[:, -1] = 0, 2
    tokenized = TokenizedText({"input_ids": ids, "attention_mask": torch.ones(batch, tokens, dtype=torch.int64)})
    targets, rows = [], []
    for i in range(batch):
        t = int(torch.randint(0, max_targets + 1, (1,), generator=g))
        c = torch.rand(t, 2, generator=g) * 0.6 + 0.2
        s = torch.rand(t, 2, generator=g) * 0.35 + 0.05
        boxes = torch.cat([c, s], -1)
        pm = torch.zeros(t, 256)
        pm[:, 1:tokens - 1] = 1.0 / (tokens - 2)
        tgt = {"boxes": boxes, "labels": torch.ones(t, dtype=torch.int64), "positive_map": pm,
               "token_spans": [[(1, tokens - 2)] for _ in range(t)]}
        if with_masks:
            tgt["masks"] = _box_masks(boxes, height, width)
        targets.append(tgt)
        rows.append(pm)
    positive_map = torch.cat(rows) if rows else torch.zeros(0, 256)

    def to(x):
        return x.to(device) if torch.is_tensor(x) else x

    from .misc import NestedTensor
    samples = NestedTensor(images.to(device), mask.to(device))
    targets = [{k: (to(v) if k != "token_spans" else v) for k, v in t.items()} for t in targets]
    return samples, tokenized.to(device), targets, positive_map.to(device)


# ---- shared-image training: B images and T captions as P (image, caption) pairs (MDETR.encode_pairs) ----------------------------
def synthetic_pair_batch(images, captions, pairs, height=640, width=640, tokens=16, seed=1000, max_targets=10, device="cpu", with_masks=False):
    """What a loader that serves several captions of one augmented image delivers: `images` images, `captions` tokenized captions and P pairs.
    pairs: a list of (image, caption) in batch order, or the number P -- then pair p is (image p * images // P, caption p % captions): every image
    and caption is used when P >= max(images, captions), each image by a run of consecutive pairs.
    -> (samples [B], tokenized [T], pair_image int32 [P], pair_caption int32 [P] (host), targets [P], positive_map [sum of the targets, 256]): the
    targets and the positive map are in PAIR order -- target dict p belongs to pair p, as batch row p of the expanded batch would carry it.
    with_masks: every target dict also carries "masks" bool [t, height, width], one rectangle per box (synthetic_batch's); the boxes are the same
    with and without."""
    from . import sweep
    images, captions = int(images), int(captions)
    if not isinstance(pairs, (list, tuple)):
        P = int(pairs)
        pairs = [(p * images // P, p % captions) for p in range(P)]
    pair_image, pair_caption, P = sweep.pair_tables(images, captions, pairs)
    samples = synthetic_batch(images, height, width, tokens=tokens, seed=seed, device=device, max_targets=0)[0]
    tokenized = synthetic_batch(captions, 1, 1, tokens=tokens, seed=seed + 1, device=device, max_targets=0)[1]
    _, _, targets, positive_map = synthetic_batch(P, 1, 1, tokens=tokens, seed=seed + 2, device=device, max_targets=max_targets)
    if with_masks:
        for t in targets:
            t["masks"] = _box_masks(t["boxes"].cpu(), int(height), int(width)).to(device)
    return samples, tokenized, pair_image, pair_caption, targets, positive_map


def expand_pairs(samples, tokenized, pair_image, pair_caption, targets, positive_map):
    """The per-sample batch of a pair batch: samples[pair_image], tokenized[pair_caption] and the same targets -> (samples [P], tokenized [P],
    targets, positive_map), what MDETR.encode / CapturedTrainStep take.  This is what the per-sample path has to run for the same P problems."""
    from . import sweep
    from .misc import NestedTensor
    dev = samples.tensors.device
    rows = torch.as_tensor(sweep._index_list(pair_image, "pair_image"), dtype=torch.int64, device=dev)
    expanded = NestedTensor(samples.tensors.index_select(0, rows), samples.mask.index_select(0, rows))
    return expanded, sweep.SweepTokenized(tokenized, sweep._index_list(pair_caption, "pair_caption")), targets, positive_map


def pair_train_losses(model, criterion, batch):
    """The eager forward half of the shared-image training step on batch = (samples, tokenized, pair_image, pair_caption, targets, positive_map):
    encode_pairs -> decode -> criterion.  -> (loss dict, outputs)."""
    samples, tokenized, pair_image, pair_caption, targets, positive_map = batch
    mc = model.encode_pairs(samples, tokenized, pair_image, pair_caption)
    outputs = model.decode(mc)
    return criterion(mc, outputs, targets, positive_map, None), outputs


def mask_pair_train_losses(model, criterion, batch):
    """pair_train_losses for a model with a mask head (DETRsegm): encode_mask_pairs -> decode_mask_pairs -> criterion (with or without "masks"; the
    targets, in pair order, carry "masks" when it has them).  -> (loss dict, outputs with "pred_masks" [P, Q, Hm, Wm])."""
    samples, tokenized, pair_image, pair_caption, targets, positive_map = batch
    mc = model.encode_mask_pairs(samples, tokenized, pair_image, pair_caption)
    outputs = model.decode_mask_pairs(mc)
    return criterion(mc, outputs, targets, positive_map, None), outputs


# ---- distillation (BASELINE config 5): (noun, pronoun) pairs -------------------------------------------------------
class SyntheticCaptions(TokenizedText):
    """Pre-tokenised synthetic captions that also answer char_to_token the way a HF BatchEncoding does, for the
    span lookups of the distillation losses (no tokenizer files exist offline): 4 characters per token, token 0 = <s>."""

    def char_to_token(self, batch_or_char, char=None):
        c = batch_or_char if char is None else char
        t = c // 4 + 1
        return t if 0 <= c and t < self["input_ids"].shape[1] - 1 else None


def synthetic_distill_batch(batch, height=640, width=640, tokens=16, seed=1000, device="cpu", max_targets=10, tokens_pronoun=None):
    """What collate_fn (util/misc.py:40-91) delivers for `batch` (noun, pronoun) pairs: the two sides share image and
    boxes; the noun caption names the object (characters 8..15 -> tokens 3..4), the pronoun caption says 'something'
    at the same place.  Returns dict(samples, targets, positive_map, captions, tokenized) with two-element lists.
    tokens_pronoun: the pronoun caption's own token count (the reference tokenises the two captions separately, so they differ): that side
    then has its own ids, positive map and token spans, of the same form as the noun side's."""
    samples, tok, targets, pmap = synthetic_batch(batch, height, width, tokens=tokens, seed=seed, device=device, max_targets=max_targets)
    out = {"samples": [samples, samples], "positive_map": [pmap, pmap], "example_rel": list(range(batch)), "targets": [], "captions": [], "tokenized": []}
    for side, word in enumerate(("scissors", "something")):
        n_tok = tokens if side == 0 or tokens_pronoun is None else int(tokens_pronoun)
        caption = ("use the " + word + " to cut the paper up")[:4 * (n_tok - 2)]
        out["captions"].append([caption] * batch)
        if n_tok != tokens:
            ids = torch.randint(3, 50265, (batch, n_tok), generator=torch.Generator().manual_seed(seed + 7919))
            ids[:, 0], ids[:, -1] = 0, 2
            tok = TokenizedText({"input_ids": ids, "attention_mask": torch.ones(batch, n_tok, dtype=torch.int64)}).to(device)
            pmap = torch.zeros_like(pmap)
            pmap[:, 1:n_tok - 1] = 1.0 / (n_tok - 2)
            out["positive_map"][side] = pmap
        tg = []
        for i, t in enumerate(targets):
            t = dict(t)
            if n_tok != tokens:
                n = len(t["boxes"])
                t["positive_map"], t["token_spans"] = pmap[:n].clone(), [[(1, n_tok - 2)] for _ in range(n)]
            t["noun_tokens_positive"] = [[(8, 8 + len(word))] for _ in range(len(t["boxes"]))]
            t["dataset_name"] = f"task_{1 + (i + side * 0) % 14}_train.json"
            tg.append(t)
        out["targets"].append(tg)
        out["tokenized"].append(SyntheticCaptions(dict(tok)))
    return out


def distillation_losses(model, model_noun, criterion, cluster_criterion, batch):
    """Forward half of engine.py:152-190 (train_one_epoch_distillation) up to the loss dict: teacher and student encode, memory-bank update and prototype
    substitution, both decodes, the paired criterion (+ the cluster losses)."""
    s_noun, s_sth = batch["samples"]
    t_noun, t_sth = batch["targets"]
    c_noun, c_sth = batch["captions"]
    k_noun, k_sth = batch["tokenized"]
    mc_noun = model_noun(s_noun, k_noun, encode_and_save=True)
    if cluster_criterion is not None:
        mc_noun = cluster_criterion.update_memory(mc_noun, t_noun, c_noun)
    out_noun = model_noun(s_noun, k_noun, encode_and_save=False, memory_cache=mc_noun)
    mc_sth = model(s_sth, k_sth, encode_and_save=True)
    loss_cluster = {}
    if cluster_criterion is not None:
        mc_sth, loss_cluster = cluster_criterion(mc_sth, t_sth, c_sth)
    out_sth = model(s_sth, k_sth, encode_and_save=False, memory_cache=mc_sth)
    losses = criterion([mc_noun, mc_sth], [out_noun, out_sth], [t_noun, t_sth], batch["positive_map"], batch.get("example_rel"))
    losses.update(loss_cluster)
    return losses


def distillation_step(model, model_noun, criterion, cluster_criterion, weight_dict, batch):
    """distillation_losses + the weighted total (engine.py:227).  Returns (total loss, loss dict)."""
    losses = distillation_losses(model, model_noun, criterion, cluster_criterion, batch)
    from .mdetr import weighted_total
    join = getattr(losses, "join", None)
    if join is not None:                       # (only inside a capture: part of the dict was produced on a side stream)
        torch.cuda.current_stream().wait_stream(join)
    total = weighted_total(losses, weight_dict)
    return total, losses


# ---- evaluation (engine.py:253-342) ---------------------------------------------------------------------------------
def synthetic_ground_truth(batches):
    """COCO-format ground truth of synthetic batches (lists of target dicts carrying "image_id", "orig_size", "boxes" in
    normalised cxcywh and optionally "masks" at the original size): what COCO(annFile) holds for the evaluator."""
    images, anns = [], []
    for targets in batches:
        for t in targets:
            h, w = (int(v) for v in t["orig_size"].tolist())
            img = int(t["image_id"])
            images.append({"id": img, "height": h, "width": w})
            boxes = t["boxes"].detach().float().cpu()
            for j in range(boxes.shape[0]):
                cx, cy, bw, bh = (float(v) for v in boxes[j])
                ann = {"id": len(anns) + 1, "image_id": img, "category_id": 1, "iscrowd": 0,
                       "bbox": [(cx - bw / 2) * w, (cy - bh / 2) * h, bw * w, bh * h], "area": bw * w * bh * h}
                if "masks" in t:
                    m = t["masks"][j].cpu().numpy()
                    ann["segmentation"], ann["area"] = m, float(m.sum())
                anns.append(ann)
    return {"images": images, "annotations": anns, "categories": [{"id": 1, "name": "preferred"}]}


def _captured_eval_batch(captured, batch, rows=False):
    """One batch of evaluate(captured=...): forward + post-processing from the CapturedEvalStep (rows: step_rows' (out, masks) instead of step's dicts).  The sizes are taken from batch["orig_sizes"] /
    batch["sizes"] (host lists of (h, w), what a loader has) when present, else read back from the targets' tensors."""
    targets = batch["targets"]
    text = batch["tokenized"] if "tokenized" in batch else [t["caption"] for t in targets]
    orig = batch["orig_sizes"] if "orig_sizes" in batch else torch.stack([t["orig_size"] for t in targets], dim=0).tolist()
    sizes = batch["sizes"] if "sizes" in batch else torch.stack([t["size"] for t in targets], dim=0).tolist()
    names = captions = None
    if captured.cluster_criterion is not None:
        names, captions = [t["dataset_name"] for t in targets], [t["caption"] for t in targets]
    step = captured.step_rows if rows else captured.step
    return step(batch["samples"], text, orig, sizes, dataset_names=names, captions=captions)


@torch.no_grad()
def evaluate_sweep(model, postprocessor, batches, tasks, device, cluster_criterion=None, captured=None, max_pairs=None, tokenized=None, observe=None,
                   evaluator=None, pairs_per_pass=8):
    """Task-sweep inference: every task's caption on every image of every batch, at the cost of ONE image pass per image and ONE text pass per
    caption for the whole loop (the reference's loader makes one sample per (image, task): engine.py:253-342 runs the ResNet and RoBERTa once per pair).
    tasks: [(name, caption[, dataset_name])]; batches yield dicts with "samples", "image_ids", "orig_sizes" ((h, w) per image, host values) and
    optionally "pairs" (a list of (image, task) indices: only those; default every task on every image).
    -> {(image_id, task_name): {"scores" [Q], "labels" [Q], "boxes" [Q, 4]}}: PostProcess's result of that pair, tensors on the device.
    The text stage runs once, before the first batch.  max_pairs: the most pairs one pair stage (encoder, decoder, heads) may hold; a batch with more
    runs it per group of max_pairs // B captions, every group on the same image state.
    cluster_criterion: the prototype choice (ClusterCriterion.infer_choice) runs per pair stage, with each pair's dataset name and caption; it needs the
    tasks' dataset names, and captions that answer char_to_token (strings through the model's tokenizer, or tokenized= a BatchEncoding of them).
    captured: a CapturedSweepStep built around `model` -- image stage, text stage, assembly, decode and post-processing of a batch are one graph
    replay.  With cluster_criterion it must be the step's own (captured.cluster_criterion, recorded into its graphs as one toist_sweep_prototypes
    launch); the tasks' dataset names and captions are passed through.  tokenized: the T captions already tokenized (offline use; else the strings go through the tokenizer).
    observe: callable(memory_cache, outputs, pair_image, pair_caption) called after every eager pair stage (tests, logging).
    evaluator: a coco_eval.SweepEvaluator holding every task's ground truth -- each pair stage's rows are scored on the device inside the loop
    (update_rows: two launches per stage, read in place, so the captured step's reused output buffers are consumed before the next replay), no keyed
    results are kept, and the function returns evaluator.summarize() after synchronize_between_processes() and accumulate(): {"tasks": {name: the
    12 COCO stats}, "mAP50", "mAP"}.
    A model with a mask head (DETRsegm): the pair stages go through mask_sweep_pairs / decode_mask_sweep -- an image's FPN terms computed once, the
    per-map program in passes of `pairs_per_pass` pairs -- and PostProcessSegm(packed=True): every result gains "mask_bits" int64 [Q, w, ceil(h / 64)]
    and "mask_size" (h, w).  The batches then also carry "sizes": each image's (h, w) inside the padded batch, host values.  postprocessor may be
    the dict of build_postprocessors (its "segm" entry gives the threshold).  captured: a CapturedMaskSweepStep.  evaluator: a SweepEvaluator built
    with iou_types holding "segm" scores the planes in place too, and summarize() carries the mask numbers under "segm"."""
    from . import kernels, sweep
    from .postprocessors import PostProcessSegm
    segm = hasattr(model, "decode_mask_sweep")
    det = model.detr if segm else model
    seg_post = None
    if isinstance(postprocessor, dict):
        seg_post, postprocessor = postprocessor.get("segm"), postprocessor["bbox"]
    if segm:
        seg_post = PostProcessSegm(threshold=seg_post.threshold if seg_post is not None else 0.5, packed=True)
        if captured is not None and not isinstance(captured, CapturedMaskSweepStep):
            raise ValueError("a model with a mask head sweeps through a CapturedMaskSweepStep (captured=)")
    tasks = [tuple(t) for t in tasks]
    if not tasks or any(len(t) not in (2, 3) for t in tasks):
        raise ValueError("tasks is a non-empty list of (name, caption) or (name, caption, dataset_name)")
    names, captions = [t[0] for t in tasks], [t[1] for t in tasks]
    dataset_names = [t[2] if len(t) == 3 else None for t in tasks]
    if len(set(names)) != len(names):
        raise ValueError("task names must be unique: they key the results")
    T = len(tasks)
    if cluster_criterion is not None:
        if captured is not None and cluster_criterion is not getattr(captured, "cluster_criterion", None):
            raise ValueError("a captured sweep runs the cluster criterion it was built with (captured.cluster_criterion): pass that one, or run the "
                             "eager loop (captured=None) for the prototype choice")
        if any(n is None for n in dataset_names):
            raise ValueError("the prototype choice needs every task's dataset name: tasks = [(name, caption, dataset_name)]")
        cluster_criterion.eval()
    model.eval()
    text = tokenized if tokenized is not None else captions
    choice = {"dataset_names": dataset_names, "captions": captions} if captured is not None and cluster_criterion is not None else {}
    out = {}
    for batch in batches:
        samples, image_ids, orig = batch["samples"], list(batch["image_ids"]), size_pairs(batch["orig_sizes"])
        B = len(image_ids)
        if len(orig) != B or samples.tensors.shape[0] != B:
            raise ValueError(f"a batch of {samples.tensors.shape[0]} images with {B} image ids and {len(orig)} original sizes")
        pi, pc, live = sweep.pair_tables(B, T, batch.get("pairs"))
        crop = None
        if segm:
            if "sizes" not in batch:
                raise ValueError("a sweep with a mask head needs batch['sizes']: each image's (h, w) inside the padded batch")
            crop = size_pairs(batch["sizes"])
            if len(crop) != B:
                raise ValueError(f"a batch of {B} images with {len(crop)} sizes")
        if captured is not None and evaluator is not None:
            if segm:
                rows, masks, pi, pc, live = captured.step_rows(samples, text, orig, crop, pairs=batch.get("pairs"), **choice)
                evaluator.update_rows(rows, image_ids, names, pi, pc, live, masks=masks)
                continue
            rows, pi, pc, live = captured.step_rows(samples, text, orig, pairs=batch.get("pairs"), **choice)
            evaluator.update_rows(rows, image_ids, names, pi, pc, live)
            continue
        if captured is not None:
            if segm:
                results, pi, pc, live = captured.step(samples, text, orig, crop, pairs=batch.get("pairs"), **choice)
            else:
                results, pi, pc, live = captured.step(samples, text, orig, pairs=batch.get("pairs"), **choice)
            out.update(sweep.keyed_results(results, image_ids, names, pi, pc, live))
            continue
        samples = samples.to(device)
        if not hasattr(text, "flat"):
            text = det.sweep_text(text, device=device)            # once: the captions do not change
            if text.key_pad.shape[0] != T:
                raise ValueError(f"{T} tasks but {text.key_pad.shape[0]} tokenized captions")
        state = det.sweep_images(samples, levels=(1, 2, 3, 4) if segm else (4,))
        for lo, hi in _sweep_groups(pi, pc, B, T, max_pairs, product=batch.get("pairs") is None):
            gi, gc = pi[lo:hi], pc[lo:hi]
            mc = model.mask_sweep_pairs(state, text, gi, gc) if segm else model.sweep_pairs(state, text, gi, gc)
            if cluster_criterion is not None:
                mc = cluster_criterion.infer_choice(mc, [dataset_names[t] for t in gc.tolist()], [captions[t] for t in gc.tolist()])
            outputs = model.decode_mask_sweep(mc, pairs_per_pass) if segm else model.decode(mc)
            rows_hw = [orig[i] for i in gi.tolist()]
            sizes = torch.tensor(rows_hw, dtype=torch.int64).to(device, non_blocking=True)
            results = postprocessor(outputs, sizes)
            masks = None
            if segm:                                            # one launch for the group's rows; the first resize target is the padded batch
                Q = outputs["pred_masks"].shape[1]
                cap_hw = (max(h for h, _ in rows_hw), max(w for _, w in rows_hw))
                cap_words = Q * cap_hw[1] * kernels.mask_words(cap_hw[0])
                table = torch.tensor([crop[i] + orig[i] for i in gi.tolist()], dtype=torch.int64).to(device, non_blocking=True)
                bits = torch.empty(len(rows_hw) * cap_words, dtype=torch.int64, device=device)
                results = seg_post.forward_static(results, outputs, table, rows_hw, tuple(samples.tensors.shape[-2:]), cap_hw, out=bits,
                                                  capacity_words=cap_words)
                if evaluator is not None and "segm" in getattr(evaluator, "iou_types", ()):
                    from .coco_eval import RowMasks
                    masks = RowMasks(bits, cap_words, sizes, rows_hw)
            if observe is not None:
                observe(mc, outputs, gi, gc)
            if evaluator is not None:                           # the postprocessor's rows, stacked: what kernels.postprocess's dict holds
                rows = {"scores": torch.stack([r["scores"] for r in results]), "boxes": torch.stack([r["boxes"] for r in results])}
                if masks is not None:
                    evaluator.update_rows(rows, image_ids, names, gi, gc, masks=masks)
                else:
                    evaluator.update_rows(rows, image_ids, names, gi, gc)
            else:
                out.update(sweep.keyed_results(results, image_ids, names, gi, gc))
        kernels.sweep_check()     # (one 4-byte read: it synchronises) a pair table entry the launch refused
        kernels.xdec_check()      # an XCD-resident decoder launch whose groups were not co-resident
    if evaluator is not None:
        evaluator.synchronize_between_processes()
        evaluator.accumulate()
        return evaluator.summarize()
    return out


def _sweep_groups(pair_image, pair_caption, B, T, max_pairs, product):
    """The (lo, hi) slices of a batch's pair tables that each run as one pair stage.  The full product is image-major (p = i * T + t), so a group of
    captions is not a slice of it: the tables are re-ordered IN PLACE group by group (image-major inside a group) -- the keys do not depend on the
    order.  An explicit pair list is cut in its own order."""
    P = pair_image.numel()
    if max_pairs is None or P <= int(max_pairs):
        return [(0, P)]
    max_pairs = int(max_pairs)
    if not product:
        if max_pairs < 1:
            raise ValueError("max_pairs must be at least 1")
        return [(lo, min(lo + max_pairs, P)) for lo in range(0, P, max_pairs)]
    per = max_pairs // B
    if per < 1:
        raise ValueError(f"max_pairs = {max_pairs} does not hold one caption on each of the batch's {B} images")
    order = [i * T + t for g in range(0, T, per) for i in range(B) for t in range(g, min(g + per, T))]
    index = torch.tensor(order, dtype=torch.int64)
    pair_image.copy_(pair_image[index])
    pair_caption.copy_(pair_caption[index])
    return [(g * B, min(g + per, T) * B) for g in range(0, T, per)]


@torch.no_grad()
def evaluate(model, criterion, cluster_criterion, postprocessors, weight_dict, batches, evaluator_list, device, args, captured=None, score_rows=False):
    """The reference's evaluation loop: per batch encode -> (prototype choice) -> decode -> losses for logging -> PostProcess
    (-> PostProcessSegm) -> evaluator.update; then gather across ranks, accumulate, summarize.  `batches` yields dicts with
    "samples", "tokenized" (or captions), "targets", "positive_map"; returns {"loss": ..., "coco_eval_bbox": [12 numbers],
    "coco_eval_masks": [...]}.
    captured: a CapturedEvalStep built around `model` -- forward and post-processing of every batch then come from its hipGraphs (one upload + one
    graph launch per batch).  The losses for logging still need an eager forward and are computed only when `criterion` is given; with
    criterion=None the loop is graph replays + evaluator updates.  (With a cluster criterion AND a criterion the prototype choice runs twice per batch;
    k-means restarted from converged centres leaves them where they are.)
    score_rows=True (needs `captured` and coco_eval.TDODCocoEvaluator evaluators; ValueError otherwise): every batch is captured.step_rows + each
    evaluator's update_rows(out, image_ids, masks=masks) -- boxes and masks of the whole batch scored on the device, read in place on the stream of
    the replay, no per-image dicts and no keyed results; the returned stats are the same."""
    from . import dist as tdist
    from .mdetr import weighted_total
    if score_rows:
        from .coco_eval import TDODCocoEvaluator
        if captured is None or not hasattr(captured, "step_rows"):
            raise ValueError("evaluate(score_rows=True) scores the rows a captured step leaves on the device: pass captured=CapturedEvalStep")
        if any(not isinstance(e, TDODCocoEvaluator) for e in evaluator_list):
            raise ValueError("evaluate(score_rows=True) needs coco_eval.TDODCocoEvaluator evaluators (update_rows)")
    model.eval()
    if criterion is not None:
        criterion.eval()
    if cluster_criterion is not None:
        cluster_criterion.eval()
    sums, n = {}, 0
    for batch in batches:
        samples, targets = batch["samples"], batch["targets"]
        text = batch["tokenized"] if "tokenized" in batch else [t["caption"] for t in targets]
        if captured is None or criterion is not None:               # (beside a captured step the eager forward only feeds the losses for logging)
            memory_cache = model(samples, text, encode_and_save=True)
            if getattr(args, "cluster", False):
                memory_cache = cluster_criterion.infer_choice(memory_cache, [t["dataset_name"] for t in targets], [t["caption"] for t in targets])
            outputs = model(samples, text, encode_and_save=False, memory_cache=memory_cache)
        if criterion is not None:
            loss_dict = tdist.reduce_dict(criterion(memory_cache, outputs, targets, batch.get("positive_map"), batch.get("example_rel")))
            for name, v in loss_dict.items():
                sums[name] = sums.get(name, 0.0) + float(v)
            sums["loss"] = sums.get("loss", 0.0) + float(weighted_total(loss_dict, weight_dict))
        n += 1
        if score_rows:
            out, masks = _captured_eval_batch(captured, batch, rows=True)
            image_ids = [int(t["image_id"]) for t in targets]
            for evaluator in evaluator_list:
                evaluator.update_rows(out, image_ids, masks=masks)
            continue
        if captured is not None:
            results = _captured_eval_batch(captured, batch)         # (reads the XCD-resident decoder's status itself before it returns)
        else:
            orig = torch.stack([t["orig_size"] for t in targets], dim=0)
            results = postprocessors["bbox"](outputs, orig)
            if "segm" in postprocessors:
                results = postprocessors["segm"](results, outputs, orig, torch.stack([t["size"] for t in targets], dim=0))
        res = {int(t["image_id"]): r for t, r in zip(targets, results)}
        for evaluator in evaluator_list:
            evaluator.update(res)
        if captured is None:
            from . import kernels
            kernels.xdec_check()      # (the results above reached the host: no extra synchronisation) an XCD-resident launch whose groups were not co-resident
    stats = {name: v / max(n, 1) for name, v in sums.items()}
    for evaluator in evaluator_list:
        evaluator.synchronize_between_processes()
        evaluator.accumulate()
        evaluator.summarize(verbose=tdist.is_main_process() and getattr(args, "verbose_eval", False))
        if "bbox" in evaluator.coco_eval:
            stats["coco_eval_bbox"] = evaluator.coco_eval["bbox"].stats.tolist()
        if "segm" in evaluator.coco_eval:
            stats["coco_eval_masks"] = evaluator.coco_eval["segm"].stats.tolist()
    return stats
