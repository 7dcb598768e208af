"""The steps replayed from hipGraphs -- CapturedTrainStep, CapturedPairTrainStep, CapturedMaskPairTrainStep, CapturedEvalStep, CapturedSweepStep, CapturedMaskSweepStep, CapturedDistillStep (also importable from toist_amd.harness) -- and the one
core they share: bucket keys, the static image / text inputs of a bucket and the upload into them, the pair tables of a pair-shaped bucket and
their fill (pair_inputs / fill_pair_inputs), the LRU of buckets, the eager pass followed by the capture, the rule that voids captured graphs once
the XCD-resident decoder launches have been turned off, and the bodies of a step on a filled bucket: _CapturedStep._train_tail and
_replay_or_capture for the two training steps (the distillation step keeps its own two-call backward and shares _replayed), _replay_checked for
the two inference steps."""
from collections import OrderedDict

import torch

from . import devcache, kernels, staging
from .misc import NestedTensor
from .transformer import TokenizedText

# the capture state of a bucket entry: what _eager_then_capture sets and _void_graphs resets.  kept: the devcache.Keep of the capture -- every cached
# table and scratch buffer the graph's launches read or write, released together with the graph and never before
_NO_GRAPH = {"graph": None, "kept": None, "loss": None, "xdec": False}


def _is_distributed():
    return torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1


def _pad_id(model):
    return getattr(getattr(model, "detr", model).transformer.text_encoder.config, "pad_token_id", 1)


def round_up(v, m):
    return (int(v) + m - 1) // m * m


def size_pairs(v):
    """(h, w) rows as a caller has them -- lists, host tensors, a list of tensors -- -> a list of int pairs."""
    rows = v.tolist() if torch.is_tensor(v) else [(r.tolist() if torch.is_tensor(r) else r) for r in v]
    return [(int(r[0]), int(r[1])) for r in rows]


def host_targets(targets):
    return [{k_: (v.cpu() if torch.is_tensor(v) else v) for k_, v in t.items()} for t in targets]


def host_positive_map(positive_map):
    return positive_map.cpu() if torch.is_tensor(positive_map) else positive_map


def static_inputs(batch, Hp, Wp, Lp, pad_id, device, mask_fill=True):
    """The fixed-address image and text inputs of one bucket: zero images under a mask of `mask_fill` (True = everything is padding until a batch is
    uploaded), `pad_id` tokens under a zero attention mask."""
    return {"samples": NestedTensor(torch.zeros(batch, 3, Hp, Wp, device=device), torch.full((batch, Hp, Wp), mask_fill, dtype=torch.bool, device=device)),
            "tok": TokenizedText({"input_ids": torch.full((batch, Lp), pad_id, dtype=torch.int64, device=device),
                                  "attention_mask": torch.zeros(batch, Lp, dtype=torch.int64, device=device)}),
            "pad_id": pad_id, "mask_fill": mask_fill}


def upload(ent, samples, tokenized):
    """A batch's images and tokens into the static inputs of `ent` (on the current stream); a batch that does not fill the bucket finds the rest blank."""
    img, msk = ent["samples"].tensors, ent["samples"].mask
    H, W = samples.tensors.shape[-2:]
    if (H, W) != tuple(img.shape[-2:]):
        img.zero_()
        msk.fill_(ent["mask_fill"])
    img[:, :, :H, :W].copy_(samples.tensors, non_blocking=True)
    msk[:, :H, :W].copy_(samples.mask, non_blocking=True)
    ids, att = ent["tok"]["input_ids"], ent["tok"]["attention_mask"]
    L = tokenized["input_ids"].shape[1]
    if L != ids.shape[1]:
        ids.fill_(ent["pad_id"])
        att.zero_()
    ids[:, :L].copy_(tokenized["input_ids"], non_blocking=True)
    att[:, :L].copy_(tokenized["attention_mask"], non_blocking=True)


def pair_inputs(captions, pairs, Lp, pad_id, device, sizes=False, crops=False):
    """What a pair-shaped bucket holds besides its images: text inputs for the CAPTIONS (not one row per image), the two int32 pair tables at fixed
    device addresses (+ sizes: an int64 [pairs, 2] table of each pair's original (h, w); + crops, with sizes: an int64 [pairs, 4] table of each pair's
    (crop_h, crop_w, h, w) for toist_mask_resize_pack_batch) and ONE staging buffer for them -- rows 0 .. P = pair_image, P .. 2P = pair_caption,
    behind them the sizes and the crops -- so that fill_pair_inputs' copies travel under one fence."""
    if crops and not sizes:
        raise ValueError("pair_inputs: the crop table comes with the size table")
    views, nbytes = staging.typed_views([(torch.int32, (2 * pairs,))] + ([(torch.int64, (pairs, 2))] if sizes else []) +
                                        ([(torch.int64, (pairs, 4))] if crops else []))
    ent = {"tok": static_inputs(captions, 1, 1, Lp, pad_id, device)["tok"],
           "pair_image": torch.zeros(pairs, dtype=torch.int32, device=device), "pair_caption": torch.zeros(pairs, dtype=torch.int32, device=device),
           "stage": staging.Staging(torch.zeros(nbytes, dtype=torch.uint8), device), "stage_views": views}
    if sizes:
        ent["sizes"] = torch.ones(pairs, 2, dtype=torch.int64, device=device)
    if crops:
        ent["crops"] = torch.ones(pairs, 4, dtype=torch.int64, device=device)
    return ent


def fill_pair_inputs(ent, pi, pc, sizes=None, crops=None):
    """Host tables (int32 [P] each, + a list of P (h, w) when the bucket holds sizes, + a list of P (crop_h, crop_w, h, w) when it holds crops) into
    pair_inputs' device tables: two to four copies, one record."""
    P = pi.numel()
    tables, *rest = ent["stage_views"](ent["stage"].open())
    tables[:P] = pi
    tables[P:] = pc
    copies = [(ent["pair_image"], tables[:P]), (ent["pair_caption"], tables[P:])]
    if sizes is not None:
        rest[0].copy_(torch.tensor(sizes, dtype=torch.int64))
        copies.append((ent["sizes"], rest[0]))
    if crops is not None:
        rest[1].copy_(torch.tensor(crops, dtype=torch.int64))
        copies.append((ent["crops"], rest[1]))
    ent["stage"].upload(*copies)


def row_results(out, rows, live, num_queries, device):
    """PostProcess's dict for each of the first `live` of the `rows` rows of kernels.postprocess's output `out`: views into it, and into the cached
    all-ones labels tensor of that shape."""
    from .postprocessors import PostProcess
    labels = PostProcess._LABELS.get((str(device), rows, num_queries), lambda: torch.ones(rows, num_queries, dtype=torch.int64, device=device))
    results = []
    for i in range(live):
        r = {"scores": out["scores"][i], "labels": labels[i], "boxes": out["boxes"][i]}
        if "scores_refexp" in out:
            r["scores_refexp"] = out["scores_refexp"][i]
        results.append(r)
    return results


class _CapturedStep:
    """What the captured steps share.  A subclass sets device (+ pad_hw, pad_tokens, max_graphs and _static_inputs(key) when it has more than one bucket)."""

    def _init_capture_state(self, side=None, xdec_seen=False):
        self._buckets = OrderedDict()          # (Hp, Wp, Lp) -> dict(static inputs and outputs of the bucket, **_NO_GRAPH), least recently used first
        self._side = side                      # the stream of the eager-pass-then-capture; created on first use when None (no GPU is needed before)
        self._xdec_seen = xdec_seen            # this object has already acted on kernels.XDEC_FAILED
        self.captures = 0
        self.replays = 0
        self.skipped = 0                       # steps that resolve_skipped() found vetoed
        self._guard_opts, self._loss_word, self._xdec_bit = [], None, {}

    def _init_guard(self, optimizers):
        """The device-side finite-loss guard: when EVERY optimizer of the step is a FusedClipAdamWEMA(skip_nonfinite=True), the step owns a one-element
        fp32 loss word (the subclass copies the total loss into it before the optimizers' step(): the reference's math.isfinite(loss_value),
        engine.py:82-85, on the device -- the gradient norm alone is not enough, some analytic backward kernels turn a NaN loss into finite gradients,
        sign(NaN) for one) registered as a float veto, and the sticky status word of the device's XCD-resident decoder launches registered as an integer
        veto.  The status word is rank-local: under torch.distributed only the norm and the loss can veto, which are the same on every rank after the
        all-reduce -- a rank that skipped alone would leave the replicas with different weights."""
        opts = list(optimizers)
        if not opts or not all(getattr(o, "skip_nonfinite", False) for o in opts):
            return
        self._guard_opts = opts
        self._loss_word = torch.zeros(1, dtype=torch.float32, device=self.device)
        for o in opts:
            o.add_veto(self._loss_word)
        if not _is_distributed():
            index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            ctl = kernels._xdec_ctl(torch.device("cuda", index))          # allocated here, eagerly: never from a capturing graph's pool
            if ctl is not None:
                for o in opts:
                    self._xdec_bit[id(o)] = o.add_veto(ctl[-1:])                   # the sticky status word

    def resolve_skipped(self):
        """Was the last step applied?  Reads the optimizers' device state (synchronises) -> None: it was; "xdec": it was skipped because an XCD-resident
        decoder launch had reported failure -- kernels.xdec_check has been called (the status word is cleared, the launches are off for the process),
        the next step() drops the graphs and runs the SAME batch, which the caller passes again, on the per-op launches; "nonfinite": it was skipped
        because the loss or the gradient norm was not finite (or a veto word of the caller's objected) -- go on with the next batch.  A skipped step
        has changed no parameter, moment, average or step count; `self.skipped` counts them.  Always None without the guard (an optimizer built
        without skip_nonfinite=True): then a bad step has already been applied."""
        why = None
        for o in self._guard_opts:
            st = o.device_state()
            if st["skipped"]:
                why = "xdec" if st["veto_mask"] & self._xdec_bit.get(id(o), 0) or why == "xdec" else "nonfinite"
        if why is not None:
            self.skipped += 1
        if why == "xdec":
            kernels.xdec_check(raise_on_failure=False)
        return why

    def bucket_of(self, samples, tokenized):
        H, W = samples.tensors.shape[-2:]
        L = tokenized["input_ids"].shape[1]
        return round_up(H, self.pad_hw), round_up(W, self.pad_hw), round_up(L, self.pad_tokens)

    def _void_graphs(self, force=False):
        """Graphs captured before kernels.XDEC_FAILED flipped contain XCD-resident decoder launches, which are off from then on (kernels.xdec_check: an
        expired spin, reached through harness.finite_or_exit on the NaN loss of that step or through CapturedEvalStep's own read): the first time this
        object sees the flag, every graph it holds is dropped; the next step of each bucket runs eagerly on the per-op launches and is captured again."""
        if force or (kernels.XDEC_FAILED and not self._xdec_seen):
            self._xdec_seen = True
            for e in self._buckets.values():
                e.update(_NO_GRAPH)

    def _entry(self, key):
        """The bucket's entry, built on first use, as the most recently used of at most `max_graphs`."""
        ent = self._buckets.get(key)
        if ent is None:
            ent = self._buckets[key] = self._static_inputs(key)
            while len(self._buckets) > self.max_graphs:
                self._buckets.popitem(last=False)          # least recently used bucket: its graph, buffers and activation pool are released
        self._void_graphs()
        self._buckets.move_to_end(key)
        return ent

    def _eager_then_capture(self, ent, body, reset=None, upload=None, capture=True):
        """The first batch of a bucket: body() eagerly -- a real step -- on the object's own stream, the stream the graph is captured on right afterwards,
        so that every per-stream cache of the launchers (split-K scratch, reduction arena) exists before the capture begins instead of being allocated
        inside it; then the capture of the same call sequence on the static inputs (nothing executes during capture), with the pointer tables of grouped
        launches beside the graph: filled once, not on every replay.  The capture hits those caches, so the graph holds their tensors' addresses:
        ent["kept"] keeps them alive beside the graph, whatever the caches evict or regrow later.  upload() runs first on that stream, reset() before each of the two passes.
        -> what the eager body() returned; what the captured one returned stays in ent["loss"]."""
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        side = self._side
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            if upload is not None:
                upload()
            if reset is not None:
                reset()
            result = body()
            if capture:
                if reset is not None:
                    reset()
                launches = kernels.XDEC_LAUNCHES
                graph = torch.cuda.CUDAGraph()
                with devcache.keeping() as kept, kernels.tables_beside_graph():
                    with torch.cuda.graph(graph, stream=side):
                        ent["loss"] = body()
                ent["graph"], ent["kept"], ent["xdec"] = graph, kept, kernels.XDEC_LAUNCHES != launches      # xdec: the graph holds an XCD-resident launch
                self.captures += 1
        torch.cuda.current_stream().wait_stream(side)
        return result

    # -- training steps: self.criterion, self.weight_dict and one self.optimizer; the subclass's _fwd_bwd_opt(ent) ends in _train_tail ---------------
    def _train_tail(self, mc, out, targets):
        """criterion -> weighted sum -> backward -> loss word -> optimizer.step() -> the total loss.  (The seed bump comes before the forward.)"""
        from .mdetr import weighted_total
        total = weighted_total(self.criterion(mc, out, targets, None, None), self.weight_dict)
        total.backward()
        if self._loss_word is not None:
            self._loss_word.copy_(total.detach())      # (device to device, captured like any other launch: every replay hands its own loss to the guard)
        self.optimizer.step()
        return total

    def _replayed(self, ent, optimizers):
        """Behind a training graph's replay -> its loss."""
        self.replays += 1
        for o in optimizers:
            if hasattr(o, "note_replayed_step"):
                o.note_replayed_step()                 # copies of the weights that the captured tail does not rewrite are stale now
        return ent["loss"]

    def _replay_or_capture(self, ent, capture=True):
        """A training step on a filled bucket: the replay of its graph, or its first step run eagerly and captured right after."""
        if ent["graph"] is not None:
            ent["graph"].replay()
            return self._replayed(ent, [self.optimizer])
        return self._eager_then_capture(ent, lambda: self._fwd_bwd_opt(ent), reset=lambda: self.optimizer.zero_grad(set_to_none=True), capture=capture)

    # -- inference steps ---------------------------------------------------------------------------------------------------------------------------
    def _replay_checked(self, ent, forward, results, handed_out=None):
        """An inference step on a filled bucket -> results().  The replay of its graph; the status words are read where the results are handed out
        (one 4-byte read each; the first synchronises): the XCD-resident decoder's when the graph holds that launch, then the step's own
        (handed_out(), which may raise) -- also behind a failed decoder launch.  That failure drops every graph (the launch's groups were not
        co-resident: per-op launches from now on), and the same batch runs again as a first batch does: forward() eagerly -- the eval-mode decode
        checks, and if need be repeats, an XCD-resident launch of the eager pass by itself -- and captured right after."""
        if ent["graph"] is not None:
            ent["graph"].replay()
            self.replays += 1
            failed = ent["xdec"] and kernels.xdec_check(raise_on_failure=False)
            if handed_out is not None:
                handed_out()
            if not failed:
                return results()
            self._void_graphs(force=True)
        self._eager_then_capture(ent, forward)
        if handed_out is not None:
            handed_out()
        return results()


class CapturedTrainStep(_CapturedStep):
    """The reference's training step (engine.py:54-101: encode -> decode -> SetCriterion -> weighted sum -> backward -> clip + AdamW + EMA)
    replayed from hipGraphs, one per input-shape BUCKET, with real variable-size batches.

    The reference resizes images to 480..800 x <= 1333 (datasets/tdod.py:305-319) and pads a batch to its largest image
    (util/misc.py:185-209); captions are padded to the longest of the batch.  A captured graph has static shapes, so the IMAGES are padded a
    little further -- height / width up to multiples of `pad_hw` -- with the padding masked out exactly as the reference masks its own
    padding (NestedTensor.mask): extra masked pixels change no result.  Caption length is NOT rounded up by default (`pad_tokens=1`):
    padded token positions are masked in every attention, but `loss_contrastive_align` takes its log-sum-exp over EVERY token column
    without an attention mask (/root/reference/models/mdetr.py:646-663), so extra pad tokens would change that loss and its gradients.
    `pad_tokens > 1` is an explicit trade: fewer graphs for captions of mixed lengths, and the contrastive term then equals the
    reference's on a batch whose longest caption has the padded length (the detection losses are unaffected).
    One graph is captured per bucket (Hp, Wp, Lp) on first use and kept in an LRU of `max_graphs`;
    targets travel through matcher.StaticTargets (fixed-address device image, any number of targets per image up to
    `max_targets_per_image`), dropout masks change per replay through the device seed word, learning rates are re-read from the
    optimizer's device table (`optimizer.sync_hyperparams()` after changing them).

    step(samples, tokenized, targets, positive_map) -> total loss (device scalar, valid until the next step of the same bucket).
    step(..., target_masks=a preprocess.DeviceTargetMasks whose pack() has run): configs[2] with the ground-truth masks prepared on the device -- the
    targets carry "mask_size" instead of "masks" (preprocess.transform_target(masks=False)), and write_into() fills the bucket's StaticTargets.masks
    on the step's stream after the targets' upload, outside the graph.
    The FIRST step of a new bucket runs eagerly (it is a real training step) and the graph is captured right after it, without
    executing anything; later steps of that bucket are one host-to-device copy of the inputs + one graph launch.
    Single process per GPU; with torch.distributed active the step falls back to the eager path (collectives are not captured).
    Forward passes made between steps (validation) must run under torch.no_grad(): a grad-enabled forward that never sees backward()
    leaves AccumulateGrad nodes bound to the stream it ran on, and torch's autograd engine would pull that stream into the next capture.

    A bad step: backward and optimizer.step() are inside the graph, so by the time the host can read the loss the update has run.  With a plain
    optimizer a non-finite loss or gradient, or a failed XCD-resident decoder launch (whose results are NaN), has then been written into the weights,
    both moments and the EMA: that is fatal, restore from a checkpoint.  With FusedClipAdamWEMA(skip_nonfinite=True) the tail skips such a step on
    the device and leaves all training state as it was; the loop asks afterwards:
        loss = cap.step(...); why = cap.resolve_skipped()      # None | "nonfinite" (go on) | "xdec" (cap.step(the same batch) once more)"""

    def __init__(self, model, criterion, optimizer, weight_dict, *, batch, max_targets_per_image=16, pad_hw=64, pad_tokens=1, max_graphs=4,
                 contrastive=None, device=None):
        self.model, self.criterion, self.optimizer, self.weight_dict = model, criterion, optimizer, weight_dict
        self.batch, self.max_t = int(batch), int(max_targets_per_image)
        self.pad_hw, self.pad_tokens, self.max_graphs = int(pad_hw), int(pad_tokens), int(max_graphs)
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        det = getattr(model, "detr", model)
        self.num_queries = det.query_embed.weight.shape[0]
        self.contrastive = bool(getattr(det, "contrastive_align_loss", False)) if contrastive is None else bool(contrastive)
        # configs[2]: the ground-truth masks travel in the bucket's StaticTargets, zero-padded to the bucket's (Hp, Wp).  The reference pads them to the
        # batch's largest image (util/misc.py:185-209) and resizes the [ceil(H/4), ceil(W/4)] predictions to that size (mdetr.py:843):
        # StaticTargets.valid_hw carries the batch's own sizes to the mask-loss kernels, which map that corner of the prediction onto that corner of
        # the targets and normalise by H * W -- the same mask losses in any bucket (round 6).
        self.masks = "masks" in getattr(criterion, "losses", ())
        self._init_capture_state(side=torch.cuda.Stream(device=self.device), xdec_seen=kernels.XDEC_FAILED)
        if kernels.SEED_DEV is None:
            kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=self.device)
        from . import engine
        engine.REUSE_GRAD_BUFFERS = True       # the loop owns the gradients: one flat buffer per program, shared by every bucket's graph and the eager steps
        self._init_guard([optimizer])

    # -- helpers ------------------------------------------------------------------------------------------------------------------
    def _static_inputs(self, key):
        from .matcher import StaticTargets
        Hp, Wp, Lp = key
        return {**static_inputs(self.batch, Hp, Wp, Lp, _pad_id(self.model), self.device), **_NO_GRAPH,
                "targets": StaticTargets(self.batch, self.max_t, self.num_queries, 256, self.device, mask_hw=(Hp, Wp) if self.masks else None)}

    def _fill(self, ent, samples, tokenized, targets, positive_map, packed, target_masks=None):
        B = samples.tensors.shape[0]
        if B != self.batch:
            raise ValueError(f"CapturedTrainStep was built for batches of {self.batch} images (got {B})")
        upload(ent, samples, tokenized)
        st = ent["targets"]
        if packed is None:
            host_t = host_targets(targets)
            masks = self.criterion.token_masks_host(host_t, tokenized) if self.contrastive else None
            st.load(host_t, host_positive_map(positive_map), masks)
        else:
            st.load_packed(packed)
        if target_masks is not None:
            last = target_masks.last
            if last is None or list(last.counts) != list(st.sizes):          # (boxes give st.sizes, "mask_rows" the counts: slot i must be target i)
                raise ValueError(f"CapturedTrainStep: target_masks holds masks for {None if last is None else list(last.counts)} targets per image, "
                                 f"the batch has {list(st.sizes)}: pack() the masks of THIS batch, with its \"mask_rows\"")
            target_masks.write_into(st)        # outside the graph, like upload(): the ground-truth masks of the batch, gathered on the device

    def _fwd_bwd_opt(self, ent):
        kernels.SEED_DEV.add_(1000003)
        mc = self.model(ent["samples"], ent["tok"], encode_and_save=True)
        out = self.model(ent["samples"], ent["tok"], encode_and_save=False, memory_cache=mc)
        return self._train_tail(mc, out, ent["targets"])

    # -- the step -------------------------------------------------------------------------------------------------------------------
    def step(self, samples, tokenized, targets=None, positive_map=None, packed=None, target_masks=None):
        if self.masks and target_masks is None:
            by_size = packed[2] is None if packed is not None else any("masks" not in t and "mask_size" in t for t in targets or ())
            if by_size:
                raise ValueError("CapturedTrainStep: the targets carry \"mask_size\" instead of \"masks\": pass target_masks= the DeviceTargetMasks "
                                 "whose pack() holds this batch's masks")
        ent = self._entry(self.bucket_of(samples, tokenized))
        self._fill(ent, samples, tokenized, targets, positive_map, packed, target_masks)
        return self._replay_or_capture(ent, capture=not _is_distributed())       # (collectives are not captured)

    __call__ = step


class CapturedPairTrainStep(_CapturedStep):
    """CapturedTrainStep for batches whose rows are (image, caption) PAIRS: `batch` images and `captions` captions give exactly `pairs` training
    samples at the cost of ONE backbone pass per image and ONE text pass per caption (MDETR.encode_pairs; the assembly's backward sums the gradients
    of an image's pairs).  One graph per bucket (Hp, Wp, Lp) -- the padding rules, the LRU, the eager first step, the finite-loss guard and
    resolve_skipped() are CapturedTrainStep's -- serves ANY pairing of the bucket's images and captions: the two pair tables sit at fixed device
    addresses and are refilled before each replay.

    step(samples [batch], tokenized [captions], pair_image, pair_caption, targets [pairs], positive_map) -> total loss.  targets and positive_map
    are in PAIR order: target dict p belongs to pair p.
    Unlike CapturedTrainStep: the number of pairs must equal `pairs` (a padding pair would add no-object loss terms and change the criterion):
    ValueError; the tables are checked on the host before anything is uploaded or launched; torch.distributed raises RuntimeError (no eager
    fall-back: encode_pairs has no data-parallel path); a criterion with mask losses raises ValueError and a mask-head model NotImplementedError."""

    def __init__(self, model, criterion, optimizer, weight_dict, *, batch, captions, pairs, max_targets_per_image=16, pad_hw=64, pad_tokens=1,
                 max_graphs=4, contrastive=None, device=None):
        if hasattr(model, "detr"):
            model.encode_pairs()                           # a mask-head model: NotImplementedError
        if "masks" in getattr(criterion, "losses", ()):
            raise ValueError("CapturedPairTrainStep takes no mask losses: the mask losses index ground-truth masks by image row, not by pair")
        self._init_pair_step(model, criterion, optimizer, weight_dict, batch, captions, pairs, max_targets_per_image, pad_hw, pad_tokens, max_graphs,
                             contrastive, device)

    masks = False                                          # the bucket's StaticTargets carry no ground-truth masks (CapturedMaskPairTrainStep: they may)

    def _init_pair_step(self, model, criterion, optimizer, weight_dict, batch, captions, pairs, max_targets_per_image, pad_hw, pad_tokens, max_graphs,
                        contrastive, device):
        """Everything of the constructor behind the refusals (shared with CapturedMaskPairTrainStep); nothing here touches the device."""
        name = type(self).__name__
        self.batch, self.captions, self.pairs = int(batch), int(captions), int(pairs)
        if self.batch <= 0 or self.captions <= 0 or self.pairs <= 0:
            raise ValueError(f"{name}: batch = {batch}, captions = {captions}, pairs = {pairs}")
        if _is_distributed():
            raise RuntimeError(f"{name} is single-process: MDETR.encode_pairs has no data-parallel path (run CapturedTrainStep on the "
                               "expanded batch under torch.distributed)")
        self.model, self.criterion, self.optimizer, self.weight_dict = model, criterion, optimizer, weight_dict
        self.max_t = int(max_targets_per_image)
        self.pad_hw, self.pad_tokens, self.max_graphs = int(pad_hw), int(pad_tokens), int(max_graphs)
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        det = getattr(model, "detr", model)
        self.num_queries = det.query_embed.weight.shape[0]
        self.contrastive = bool(getattr(det, "contrastive_align_loss", False)) if contrastive is None else bool(contrastive)
        self._init_capture_state(xdec_seen=kernels.XDEC_FAILED)
        self._ready = False                                # device state (seed word, guard words) is set up by the first step that passed the checks

    def _device_state(self):
        if self._ready:
            return
        if kernels.SEED_DEV is None:
            kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=self.device)
        from . import engine
        engine.REUSE_GRAD_BUFFERS = True       # as in CapturedTrainStep: the loop owns the gradients
        self._init_guard([self.optimizer])
        self._ready = True

    def _static_inputs(self, key):
        from .matcher import StaticTargets
        Hp, Wp, Lp = key
        pad_id = _pad_id(self.model)
        return {**static_inputs(self.batch, Hp, Wp, Lp, pad_id, self.device), **pair_inputs(self.captions, self.pairs, Lp, pad_id, self.device),
                **_NO_GRAPH, "targets": StaticTargets(self.pairs, self.max_t, self.num_queries, 256, self.device, mask_hw=(Hp, Wp) if self.masks else None)}

    def check_batch(self, samples, tokenized, pair_image, pair_caption, targets):
        """Host check of a step's arguments (ValueError; nothing has been uploaded or launched) -> the two tables as int32 host tensors."""
        from . import sweep
        name = type(self).__name__
        B, T = samples.tensors.shape[0], tokenized["input_ids"].shape[0]
        if B != self.batch or T != self.captions:
            raise ValueError(f"{name} was built for {self.batch} images and {self.captions} captions (got {B} and {T})")
        pi, pc = sweep.check_tables(pair_image, pair_caption, self.batch, self.captions)
        if pi.numel() != self.pairs:
            raise ValueError(f"{name} was built for exactly {self.pairs} pairs (got {pi.numel()}): a padding pair would add no-object "
                             "loss terms")
        if targets is not None and len(targets) != self.pairs:
            raise ValueError(f"{name}: {len(targets)} target dicts for {self.pairs} pairs (targets are in pair order)")
        return pi, pc

    def _fill(self, ent, samples, tokenized, pi, pc, targets, positive_map):
        from . import sweep
        upload(ent, samples, tokenized)
        fill_pair_inputs(ent, pi, pc)
        host_t = host_targets(targets)
        masks = None
        if self.contrastive:                   # (character spans are looked up in the caption of the target's PAIR; token spans need no lookup)
            by_pair = sweep.SweepTokenized(tokenized, pc) if any("token_spans" not in t for t in host_t) else None
            masks = self.criterion.token_masks_host(host_t, by_pair)
        ent["targets"].load(host_t, host_positive_map(positive_map), masks)

    def _fwd_bwd_opt(self, ent):
        kernels.SEED_DEV.add_(1000003)
        mc = self.model.encode_pairs(ent["samples"], ent["tok"], ent["pair_image"], ent["pair_caption"], check=False)      # (host-checked tables)
        return self._train_tail(mc, self.model.decode(mc), ent["targets"])

    def step(self, samples, tokenized, pair_image, pair_caption, targets, positive_map):
        if _is_distributed():
            raise RuntimeError(f"{type(self).__name__} is single-process: MDETR.encode_pairs has no data-parallel path")
        pi, pc = self.check_batch(samples, tokenized, pair_image, pair_caption, targets)
        self._device_state()
        ent = self._entry(self.bucket_of(samples, tokenized))
        self._fill(ent, samples, tokenized, pi, pc, targets, positive_map)
        return self._replay_or_capture(ent)

    __call__ = step


class CapturedMaskPairTrainStep(CapturedPairTrainStep):
    """CapturedPairTrainStep for a model with a mask head (DETRsegm) -- configs[2] on shared images: DETRsegm.encode_mask_pairs / decode_mask_pairs
    replayed from one hipGraph per bucket, the mask program and its backward reading the bucket's pair table, so the ResNet's forward and backward
    run once per IMAGE while the mask head runs on all `pairs` * Q maps.  The criterion may carry "masks" or not; with them the bucket's
    StaticTargets hold the ground-truth masks (mask_hw = the bucket's (Hp, Wp)) and the targets -- in PAIR order, target dict p belongs to pair p --
    carry "masks" [T_p, h, w] at the padded batch's size, as CapturedTrainStep's do on the expanded batch.  A model built with freeze_detr=True
    trains the mask head and bbox_attention alone.
    Everything else is CapturedPairTrainStep's: the exact pair count, the host-checked tables, single process, buckets and their LRU, the eager first
    step, the finite-loss guard and resolve_skipped().
    Out of scope (ValueError before anything is uploaded or launched): ground truth prepared on the device -- step(target_masks=...) and targets
    that carry "mask_size" instead of "masks"; and a model without a mask head (CapturedPairTrainStep is the step for it)."""

    def __init__(self, model, criterion, optimizer, weight_dict, *, batch, captions, pairs, max_targets_per_image=16, pad_hw=64, pad_tokens=1,
                 max_graphs=4, contrastive=None, device=None):
        if not hasattr(model, "decode_mask_pairs"):
            raise ValueError("CapturedMaskPairTrainStep takes a model with a mask head (DETRsegm); a detection model trains through CapturedPairTrainStep")
        self.masks = "masks" in getattr(criterion, "losses", ())
        self._init_pair_step(model, criterion, optimizer, weight_dict, batch, captions, pairs, max_targets_per_image, pad_hw, pad_tokens, max_graphs,
                             contrastive, device)

    def check_batch(self, samples, tokenized, pair_image, pair_caption, targets):
        pi, pc = super().check_batch(samples, tokenized, pair_image, pair_caption, targets)
        if any("mask_size" in t and "masks" not in t for t in targets or ()):
            raise ValueError("CapturedMaskPairTrainStep: the targets carry \"mask_size\" instead of \"masks\" -- ground truth prepared on the device is "
                             "out of scope for the shared-image step (CapturedTrainStep(target_masks=) on the expanded batch serves it)")
        if self.masks and any("masks" not in t for t in targets or ()):
            raise ValueError("CapturedMaskPairTrainStep: the criterion has mask losses, so every target dict (in pair order) carries \"masks\"")
        return pi, pc

    def _fwd_bwd_opt(self, ent):
        kernels.SEED_DEV.add_(1000003)
        mc = self.model.encode_mask_pairs(ent["samples"], ent["tok"], ent["pair_image"], ent["pair_caption"], check=False)      # (host-checked tables)
        return self._train_tail(mc, self.model.decode_mask_pairs(mc), ent["targets"])

    def step(self, samples, tokenized, pair_image, pair_caption, targets, positive_map, target_masks=None):
        if target_masks is not None:
            raise ValueError("CapturedMaskPairTrainStep: target_masks= (ground truth prepared on the device) is out of scope for the shared-image step")
        return super().step(samples, tokenized, pair_image, pair_caption, targets, positive_map)

    __call__ = step


class CapturedEvalStep(_CapturedStep):
    """The reference's evaluation body (engine.py:253-342: encode -> optional prototype choice -> decode -> PostProcess -> optional PostProcessSegm) replayed
    from hipGraphs, one per input-shape BUCKET (Hp, Wp, Lp) -- the padding rules and the LRU of `max_graphs` are CapturedTrainStep's; the batch size is
    fixed; everything runs under torch.no_grad() with the model in eval().

    step(samples, tokenized, orig_sizes, sizes, dataset_names=None, captions=None) -> results: a list of dicts with the keys, dtypes and shapes of
    PostProcess and PostProcessSegm(packed=True): "scores" f32 [Q], "labels" int64 [Q], "boxes" f32 [Q, 4] (+ "scores_refexp" when the model emits
    pred_isfinal), with a mask head "mask_bits" int64 [Q, w_i, ceil(h_i/64)] + "mask_size" (h_i, w_i) -- TDODCocoEvaluator.update takes them unchanged.
    Every tensor is a view into the bucket's output buffers, valid until the next step of that bucket.  dense_masks=True replaces the packed planes by
    the reference's "masks" bool [Q, 1, h_i, w_i] on the host.
    step_rows(...) -> (out, masks): the same step without the per-image dicts, out = kernels.postprocess's dict of the bucket, masks = a
    coco_eval.RowMasks over its bit planes (None without a mask head): what TDODCocoEvaluator.update_rows(masks=) scores in place.
    orig_sizes / sizes: (h, w) per image as HOST values (lists, or host tensors): they travel to the device in one fixed-address int64 table per bucket
    that the two post-processing kernels read (csrc/postproc.hip, csrc/evalmask.hip), so nothing is read back before the launch.

    The FIRST batch of a bucket runs eagerly on the object's side stream and the graph is captured right after (inside kernels.tables_beside_graph());
    later batches of that bucket are one upload of the inputs + one graph launch.
    Masks: the planes of image i start at word i * capacity of one buffer per bucket, capacity = Q * max_orig_hw[1] * ceil(max_orig_hw[0] / 64); an
    image larger than `max_orig_hw` raises ValueError before anything is launched.  In a padded bucket pred_masks cover (Hp, Wp), so the FIRST resize
    target is the bucket's (Hp, Wp), not the batch's largest image, and the crop is each image's `size` -- what the reference computes on a batch
    whose largest image is Hp x Wp (models/postprocessors.py:86-107).
    Prototype choice: with a `cluster_criterion` it runs inside the graph (ClusterCriterion.infer_choice_static on a DistillTables image filled by
    pack_eval from the tokenized captions -- which must answer char_to_token --, the caption strings and the dataset names); the preconditions are
    ClusterCriterion._static_ok's.  k-means moves cluster_centers in place, as the reference's memory_cluster does.
    XCD-resident decoder: when the captured graph holds that launch, its status word is read after every replay (kernels.xdec_check: the one
    synchronisation of a step, at the point where the results are handed out); a failed launch drops every graph, and the same batch runs again on the
    per-op launches and is captured again -- inference has no state a failed step could have poisoned.
    Data parallelism: the forward holds no collective, every rank evaluates its own shard, so the step stays captured under torch.distributed."""

    def __init__(self, model, cluster_criterion=None, *, batch, masks=None, max_orig_hw=None, pad_hw=64, pad_tokens=1, max_graphs=4, dense_masks=False,
                 threshold=0.5, device=None):
        self.model, self.cluster_criterion = model, cluster_criterion
        self.batch, self.pad_hw, self.pad_tokens, self.max_graphs = int(batch), int(pad_hw), int(pad_tokens), int(max_graphs)
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        det = getattr(model, "detr", model)
        self.num_queries = det.query_embed.weight.shape[0]
        self.masks = hasattr(model, "detr") if masks is None else bool(masks)
        self.dense_masks, self.threshold = bool(dense_masks), float(threshold)
        if self.masks and max_orig_hw is None:
            raise ValueError("CapturedEvalStep with a mask head needs max_orig_hw = the largest original (h, w) it has to hold")
        self.max_orig_hw = (int(max_orig_hw[0]), int(max_orig_hw[1])) if max_orig_hw is not None else None
        self.capacity_words = self.num_queries * self.max_orig_hw[1] * ((self.max_orig_hw[0] + 63) // 64) if self.masks else 0
        self._init_capture_state()

    # -- helpers ------------------------------------------------------------------------------------------------------------------
    def check_sizes(self, key, orig_sizes, sizes):
        """Host check of a batch's sizes against the bucket and the mask capacity (ValueError; nothing has been launched).  -> (orig, sizes) as int pairs."""
        orig, crop = size_pairs(orig_sizes), size_pairs(sizes)
        if len(orig) != self.batch or len(crop) != self.batch:
            raise ValueError(f"CapturedEvalStep was built for batches of {self.batch} images (got {len(orig)} original sizes, {len(crop)} sizes)")
        for (h, w), (ch, cw) in zip(orig, crop):
            if h <= 0 or w <= 0 or ch <= 0 or cw <= 0 or ch > key[0] or cw > key[1]:
                raise ValueError(f"CapturedEvalStep: an image of size {ch} x {cw} (original {h} x {w}) does not fit the padded batch {key[0]} x {key[1]}")
            if self.masks and (h > self.max_orig_hw[0] or w > self.max_orig_hw[1]):
                raise ValueError(f"CapturedEvalStep: an original size of {h} x {w} exceeds max_orig_hw = {self.max_orig_hw[0]} x {self.max_orig_hw[1]} "
                                 "(the capacity of the mask planes)")
        return orig, crop

    def _static_inputs(self, key):
        Hp, Wp, Lp = key
        dev, B = self.device, self.batch
        ent = {**static_inputs(B, Hp, Wp, Lp, _pad_id(self.model), dev), **_NO_GRAPH,
               # rows 0 .. 2B: (h, w) originals for toist_postprocess; rows 2B .. 6B: (crop_h, crop_w, h, w) for toist_mask_resize_pack_batch
               "sizes_stage": staging.Staging(torch.ones(6 * B, dtype=torch.int64), dev), "sizes": torch.ones(6 * B, dtype=torch.int64, device=dev),
               "out": None, "tables": None,
               "bits": torch.zeros(B * self.capacity_words, dtype=torch.int64, device=dev) if self.masks else None}
        if self.cluster_criterion is not None:
            from .distill import DistillTables
            ent["tables"] = DistillTables(B, Lp, dev, pronoun_side=True)
        return ent

    def _fill(self, ent, samples, tokenized, orig, crop, dataset_names, captions):
        B = self.batch
        upload(ent, samples, tokenized)
        host = ent["sizes_stage"].open()
        host[:2 * B] = torch.tensor(orig, dtype=torch.int64).view(-1)
        host[2 * B:] = torch.tensor([c + o for c, o in zip(crop, orig)], dtype=torch.int64).view(-1)
        ent["sizes_stage"].upload((ent["sizes"], host))
        if ent["tables"] is not None:
            ent["tables"].load_eval(tokenized, captions, dataset_names)

    def _forward(self, ent, key):
        """The launches of one batch on the bucket's static inputs (eagerly, and once more under capture)."""
        B = self.batch
        mc = self.model(ent["samples"], ent["tok"], encode_and_save=True)
        if self.cluster_criterion is not None:
            mc = self.cluster_criterion.infer_choice_static(mc, ent["tables"])
            if ent.get("img_memory_mod") is None:                # the memory with the chosen prototypes, copied to a fixed buffer: readable after any step
                ent["img_memory_mod"] = torch.empty_like(mc["img_memory_mod"])
            ent["img_memory_mod"].copy_(mc["img_memory_mod"])
        outputs = self.model(ent["samples"], ent["tok"], encode_and_save=False, memory_cache=mc)
        ent["out"] = kernels.postprocess(outputs["pred_logits"], outputs["pred_boxes"], ent["sizes"][:2 * B].view(B, 2), outputs.get("pred_isfinal"),
                                         out=ent["out"])
        if self.masks:
            logits = outputs["pred_masks"].squeeze(2).float().contiguous()                # [B, Q, h0, w0]; they cover the padded (Hp, Wp)
            kernels.mask_resize_pack_batch(logits, (key[0], key[1]), ent["sizes"][2 * B:].view(B, 4), self.max_orig_hw, self.capacity_words, ent["bits"],
                                           self.threshold)

    def _results(self, ent, orig):
        Q = self.num_queries
        results = row_results(ent["out"], self.batch, self.batch, Q, self.device)
        if self.masks:
            for i, (r, (h, w)) in enumerate(zip(results, orig)):
                words = kernels.mask_words(h)
                bits = ent["bits"][i * self.capacity_words:i * self.capacity_words + Q * w * words].view(Q, w, words)
                if self.dense_masks:
                    r["masks"] = kernels.mask_unpack(bits, h, w).unsqueeze(1).cpu()
                else:
                    r["mask_bits"], r["mask_size"] = bits, (h, w)
        return results

    # -- the step -------------------------------------------------------------------------------------------------------------------
    def step(self, samples, tokenized, orig_sizes, sizes, dataset_names=None, captions=None):
        return self._step(samples, tokenized, orig_sizes, sizes, dataset_names, captions, self._results)

    def step_rows(self, samples, tokenized, orig_sizes, sizes, dataset_names=None, captions=None):
        """step() without the per-image dicts -> (out, masks): out = the bucket's kernels.postprocess dict (scores [B, Q], boxes [B, Q, 4]), masks = a
        coco_eval.RowMasks over the bucket's bit planes and the (h, w) rows of its size table (None without a mask head) -- views, valid until the
        next step of that bucket: what a consumer that takes a whole batch of rows reads in place (TDODCocoEvaluator.update_rows(masks=), issued on
        the stream of the step, so the next replay on that stream overwrites the rows only when they have been scored).  Not with dense_masks=True."""
        if self.dense_masks:
            raise ValueError("CapturedEvalStep.step_rows hands out the packed planes: build the step with dense_masks=False")
        return self._step(samples, tokenized, orig_sizes, sizes, dataset_names, captions, self._rows)

    def _rows(self, ent, orig):
        if not self.masks:
            return ent["out"], None
        from .coco_eval import RowMasks
        return ent["out"], RowMasks(ent["bits"], self.capacity_words, ent["sizes"][:2 * self.batch].view(self.batch, 2), orig)

    @torch.no_grad()
    def _step(self, samples, tokenized, orig_sizes, sizes, dataset_names, captions, results):
        if isinstance(tokenized, (list, tuple)) and len(tokenized) and isinstance(tokenized[0], str):
            if captions is None:
                captions = list(tokenized)
            tokenized = getattr(self.model, "detr", self.model).transformer._tokenize(list(tokenized), self.device)
        if samples.tensors.shape[0] != self.batch:
            raise ValueError(f"CapturedEvalStep was built for batches of {self.batch} images (got {samples.tensors.shape[0]})")
        key = self.bucket_of(samples, tokenized)
        orig, crop = self.check_sizes(key, orig_sizes, sizes)
        if self.cluster_criterion is not None:
            if dataset_names is None or captions is None:
                raise ValueError("CapturedEvalStep with a cluster criterion needs the batch's dataset_names and captions")
            self.cluster_criterion._static_ok()
            self.cluster_criterion.eval()
        if self.model.training:
            self.model.eval()
        ent = self._entry(key)
        self._fill(ent, samples, tokenized, orig, crop, dataset_names, captions)
        return self._replay_checked(ent, lambda: self._forward(ent, key), lambda: results(ent, orig))

    __call__ = step


class CapturedSweepStep(_CapturedStep):
    """Task-sweep inference replayed from hipGraphs: `captions` captions over the `batch` images of a batch as up to `pairs` (image, caption) pairs, at
    the cost of ONE image pass per image and ONE text pass per caption (toist_amd/sweep.py).  One graph per input-shape bucket (Hp, Wp, Lp) -- the
    padding rules and the LRU of `max_graphs` are the shared core's -- holds the image stage, the text stage (a parallel branch), the
    toist_sweep_assemble launch, the encoder, decode and kernels.postprocess.  Everything runs under torch.no_grad() with the model in eval().

    step(samples, tokenized, orig_sizes, pairs=None) -> (results, pair_image, pair_caption, live): results[p], p < live, is PostProcess's dict of pair
    (pair_image[p], pair_caption[p]) -- views into the bucket's output buffers, valid until the next step of that bucket; sweep.keyed_results keys
    them.  pairs: a list of (image, caption), at most the capacity; default every caption on every image, image-major.  The tables are padded to the
    capacity with the pair (0, 0); the padded rows are computed and never handed out.
    step_rows(...) -> (out, pair_image, pair_caption, live): the same step without the per-row dicts, out = kernels.postprocess's dict of the bucket.
    The pair tables and the per-pair size table (each pair's original (h, w), gathered by pair_image on the host) sit at fixed addresses per bucket;
    they are uploaded when they CHANGE -- the full product of a whole evaluation is uploaded once.  The graph's assemble launch checks every entry it
    reads: its status word and the XCD-resident decoder's are read after every replay, where the results are handed out (one synchronisation).  A
    refused entry raises ValueError (and the tables are uploaded afresh by the next step); a failed decoder launch drops every graph, and the same
    batch runs again on the per-op launches and is captured again, as in CapturedEvalStep.
    Prototype choice: with a `cluster_criterion` (a distill.ClusterCriterion) it runs inside the graph, between the pair stage and decode:
    ClusterCriterion.infer_choice_pairs, ONE toist_sweep_prototypes launch on the encoder's bf16 rows, reading a distill.SweepChoiceTables image of
    the bucket.  step / step_rows then take dataset_names= and captions=: T strings each (the tokenized captions must answer char_to_token); the image
    is uploaded, with the pair tables, when it changes.  Padding pairs are encoded and decoded as before and never enter the k-means walk.  After a
    step ent["img_memory_mod"] is the bucket's memory with the chosen prototypes, a bf16 [S, pairs, d] view.  The preconditions are
    ClusterCriterion._static_ok's; k-means moves cluster_centers in place.  Anything but a ClusterCriterion raises ValueError."""

    def __init__(self, model, cluster_criterion=None, *, batch, captions, pairs=None, pad_hw=64, pad_tokens=1, max_graphs=4, device=None):
        self._take_criterion(cluster_criterion)
        if hasattr(model, "detr"):
            model.encode_sweep()                           # a mask-head model: NotImplementedError naming the follow-up
        self.model = model
        self.batch, self.captions = int(batch), int(captions)
        self.pairs = self.batch * self.captions if pairs is None else int(pairs)
        if self.batch <= 0 or self.captions <= 0 or self.pairs <= 0:
            raise ValueError(f"CapturedSweepStep: batch = {batch}, captions = {captions}, pairs = {pairs}")
        self.pad_hw, self.pad_tokens, self.max_graphs = int(pad_hw), int(pad_tokens), int(max_graphs)
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        self.num_queries = model.query_embed.weight.shape[0]
        self._init_capture_state()

    # -- the prototype choice (shared with CapturedMaskSweepStep) ----------------------------------------------------------------------------------
    def _take_criterion(self, cluster_criterion):
        from .distill import ClusterCriterion
        if cluster_criterion is not None and not isinstance(cluster_criterion, ClusterCriterion):
            raise ValueError(f"{type(self).__name__}: the cluster criterion of a captured sweep is a distill.ClusterCriterion "
                             f"(got {type(cluster_criterion).__name__})")
        self.cluster_criterion = cluster_criterion

    def _choice_inputs(self, Lp):
        """What a bucket holds for the prototype choice: the caption-side tables (memory_mod hangs off them)."""
        from .distill import SweepChoiceTables
        return {"choice": SweepChoiceTables(self.captions, Lp, self.device) if self.cluster_criterion is not None else None, "img_memory_mod": None}

    def _choice_args(self, tokenized, dataset_names, captions):
        """Host check of a step's dataset names and captions (ValueError; nothing has been launched) -> (dataset_names, captions) as lists, or
        (None, None) without a criterion."""
        cc = self.cluster_criterion
        if cc is None:
            return None, None
        if dataset_names is None or captions is None:
            raise ValueError(f"{type(self).__name__} with a cluster criterion needs the captions' dataset_names and captions")
        dataset_names, captions = list(dataset_names), list(captions)
        if len(dataset_names) != self.captions or len(captions) != self.captions:
            raise ValueError(f"{type(self).__name__} with a cluster criterion: {len(dataset_names)} dataset names and {len(captions)} caption strings "
                             f"for {self.captions} captions")
        from .distill import task_index
        if any(not 0 <= task_index(n) < cc.task_count for n in dataset_names):
            raise ValueError(f"{type(self).__name__}: the dataset names {dataset_names!r} name a task outside the cluster criterion's {cc.task_count}")
        if not hasattr(tokenized, "char_to_token"):
            raise ValueError(f"{type(self).__name__} with a cluster criterion: the tokenized captions must answer char_to_token")
        cc._static_ok()
        cc.eval()
        return dataset_names, captions

    def _choose(self, ent, mc):
        """The prototype stage of _forward, between the pair stage and decode."""
        if self.cluster_criterion is None:
            return mc
        mc = self.cluster_criterion.infer_choice_pairs(mc, ent["choice"], ent["pair_caption"])
        nat = mc["_native"]
        ent["img_memory_mod"] = nat["memory_mod"].view(nat["B"], nat["S"], -1).permute(1, 0, 2)     # bf16 [S, pairs, d]: a view, readable after any step
        return mc

    def _static_inputs(self, key):
        Hp, Wp, Lp = key
        pad_id = _pad_id(self.model)
        return {**static_inputs(self.batch, Hp, Wp, Lp, pad_id, self.device), **pair_inputs(self.captions, self.pairs, Lp, pad_id, self.device, sizes=True),
                **_NO_GRAPH, "uploaded": None, "out": None, **self._choice_inputs(Lp)}

    def _fill(self, ent, samples, tokenized, pi, pc, sizes, choice=None):
        upload(ent, samples, tokenized)
        tables = (pi.tolist(), pc.tolist(), sizes)
        if ent["uploaded"] != tables:                      # (the full product of a whole evaluation is uploaded once)
            fill_pair_inputs(ent, pi, pc, sizes)
            ent["uploaded"] = tables
        if choice is not None:                             # (tokenized, captions, dataset_names, live): uploaded when the image changes
            ent["choice"].load(*choice)

    def _forward(self, ent):
        """The launches of one batch on the bucket's static inputs (eagerly, and once more under capture)."""
        state, text = self.model.sweep_stages(ent["samples"], ent["tok"])
        mc = self.model.sweep_pairs(state, text, ent["pair_image"], ent["pair_caption"], check=False)       # (step reads the status word)
        outputs = self.model.decode(self._choose(ent, mc))
        ent["out"] = kernels.postprocess(outputs["pred_logits"], outputs["pred_boxes"], ent["sizes"], outputs.get("pred_isfinal"), out=ent["out"])

    def _handed_out(self, ent):
        """Read the assemble launch's status word where the results are handed out (it synchronises): a refused table entry raises ValueError."""
        try:
            kernels.sweep_check()
        except ValueError:
            ent["uploaded"] = None                         # whatever the device tables hold now, the next step uploads them afresh
            if ent["choice"] is not None:
                ent["choice"].invalidate()
            raise

    def step(self, samples, tokenized, orig_sizes, pairs=None, dataset_names=None, captions=None):
        out, pi, pc, live = self.step_rows(samples, tokenized, orig_sizes, pairs=pairs, dataset_names=dataset_names, captions=captions)
        return row_results(out, self.pairs, live, self.num_queries, self.device), pi, pc, live

    @torch.no_grad()
    def step_rows(self, samples, tokenized, orig_sizes, pairs=None, dataset_names=None, captions=None):
        """step() without the per-row dicts -> (out, pair_image, pair_caption, live): out = the bucket's kernels.postprocess dict (scores [pairs, Q],
        boxes [pairs, Q, 4]; rows from `live` on are padding), valid until the next step of that bucket -- what a consumer that takes a whole batch
        of rows reads in place (coco_eval.SweepEvaluator.update_rows)."""
        from . import sweep
        if isinstance(tokenized, (list, tuple)) and len(tokenized) and isinstance(tokenized[0], str):
            if captions is None:
                captions = list(tokenized)
            tokenized = self.model.transformer._tokenize(list(tokenized), self.device)
        if samples.tensors.shape[0] != self.batch or tokenized["input_ids"].shape[0] != self.captions:
            raise ValueError(f"CapturedSweepStep was built for {self.batch} images and {self.captions} captions "
                             f"(got {samples.tensors.shape[0]} and {tokenized['input_ids'].shape[0]})")
        orig = size_pairs(orig_sizes)
        if len(orig) != self.batch or any(h <= 0 or w <= 0 for h, w in orig):
            raise ValueError(f"CapturedSweepStep: {len(orig)} original sizes for {self.batch} images, or a size that is not positive")
        pi, pc, live = sweep.pair_tables(self.batch, self.captions, pairs, capacity=self.pairs)           # ValueError before anything is launched
        sizes = [orig[i] for i in pi.tolist()]
        dataset_names, captions = self._choice_args(tokenized, dataset_names, captions)              # the same
        if self.model.training:
            self.model.eval()
        key = self.bucket_of(samples, tokenized)
        ent = self._entry(key)
        self._fill(ent, samples, tokenized, pi, pc, sizes, (tokenized, captions, dataset_names, live) if captions is not None else None)
        out = self._replay_checked(ent, lambda: self._forward(ent), lambda: ent["out"], lambda: self._handed_out(ent))
        return out, pi, pc, live

    __call__ = step


class CapturedMaskSweepStep(CapturedSweepStep):
    """Task-sweep inference WITH THE MASK HEAD replayed from hipGraphs: CapturedSweepStep's pairs, tables and buckets around a DETRsegm.  One graph per
    bucket (Hp, Wp, Lp) holds the image stage with all four backbone levels, the text stage (a parallel branch), the toist_sweep_assemble launch, the
    encoder, decode, the mask program -- an image's terms once, the per-map program in passes of `pairs_per_pass` pairs (DETRsegm.decode_mask_sweep)
    --, kernels.postprocess and, pass by pass, kernels.mask_resize_pack_batch over the pass's rows, so the graph's pool holds the logits of one pass.

    step(samples, tokenized, orig_sizes, sizes, pairs=None) -> (results, pair_image, pair_caption, live): results[p], p < live, carries PostProcess's
    "scores" / "labels" / "boxes" of pair p plus "mask_bits" int64 [Q, w, ceil(h / 64)] and "mask_size" (h, w) of its image's original size -- what
    PostProcessSegm(packed=True) hands out; views into the bucket's buffers, valid until the next step of that bucket.
    step_rows(...) -> (out, masks, pair_image, pair_caption, live): out = kernels.postprocess's dict of the bucket, masks = a coco_eval.RowMasks over
    its planes (row p's planes start at word p * capacity_words): what coco_eval.SweepEvaluator.update_rows(masks=) scores in place.
    orig_sizes / sizes: (h, w) per IMAGE as host values; the per-pair tables -- originals for toist_postprocess, (crop_h, crop_w, h, w) for
    toist_mask_resize_pack_batch -- are gathered by pair_image on the host and uploaded with the pair tables when any of them changes.  The first
    resize target is the bucket's (Hp, Wp), as in CapturedEvalStep; capacity and size checks are CapturedEvalStep.check_sizes's, raised before
    anything is launched.  The status words (the sweep launches' and the XCD-resident decoder's) are read where results are handed out.
    Prototype choice: a `cluster_criterion` runs inside the graph between mask_sweep_pairs and decode, as in CapturedSweepStep (dataset_names= and
    captions= in step / step_rows)."""

    def __init__(self, model, cluster_criterion=None, *, batch, captions, pairs=None, max_orig_hw=None, pairs_per_pass=8, threshold=0.5, pad_hw=64,
                 pad_tokens=1, max_graphs=4, device=None):
        from .sweep import pair_passes
        self._take_criterion(cluster_criterion)
        if not hasattr(model, "detr") or not hasattr(model, "decode_mask_sweep"):
            raise ValueError("CapturedMaskSweepStep needs a model with a mask head (DETRsegm); CapturedSweepStep serves a detection model")
        if max_orig_hw is None:
            raise ValueError("CapturedMaskSweepStep needs max_orig_hw = the largest original (h, w) its mask planes have to hold")
        self.model = model
        self.batch, self.captions = int(batch), int(captions)
        self.pairs = self.batch * self.captions if pairs is None else int(pairs)
        if self.batch <= 0 or self.captions <= 0 or self.pairs <= 0:
            raise ValueError(f"CapturedMaskSweepStep: batch = {batch}, captions = {captions}, pairs = {pairs}")
        self.pairs_per_pass = int(pairs_per_pass)
        pair_passes(self.pairs, pairs_per_pass)                     # ValueError for a pass size that is not a positive integer
        self.pad_hw, self.pad_tokens, self.max_graphs = int(pad_hw), int(pad_tokens), int(max_graphs)
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        self.num_queries = model.detr.query_embed.weight.shape[0]
        self.masks, self.threshold = True, float(threshold)           # (masks: what CapturedEvalStep.check_sizes reads)
        self.max_orig_hw = (int(max_orig_hw[0]), int(max_orig_hw[1]))
        if self.max_orig_hw[0] <= 0 or self.max_orig_hw[1] <= 0:
            raise ValueError(f"CapturedMaskSweepStep: max_orig_hw = {max_orig_hw}")
        self.capacity_words = self.num_queries * self.max_orig_hw[1] * ((self.max_orig_hw[0] + 63) // 64)
        self._init_capture_state()

    check_sizes = CapturedEvalStep.check_sizes

    def _static_inputs(self, key):
        Hp, Wp, Lp = key
        pad_id = _pad_id(self.model)
        return {**static_inputs(self.batch, Hp, Wp, Lp, pad_id, self.device),
                **pair_inputs(self.captions, self.pairs, Lp, pad_id, self.device, sizes=True, crops=True), **_NO_GRAPH, "uploaded": None, "out": None,
                "bits": torch.zeros(self.pairs * self.capacity_words, dtype=torch.int64, device=self.device), **self._choice_inputs(Lp)}

    def _fill(self, ent, samples, tokenized, pi, pc, sizes, crops, choice=None):
        upload(ent, samples, tokenized)
        tables = (pi.tolist(), pc.tolist(), sizes, crops)
        if ent["uploaded"] != tables:
            fill_pair_inputs(ent, pi, pc, sizes, crops)
            ent["uploaded"] = tables
        if choice is not None:
            ent["choice"].load(*choice)

    def _forward(self, ent, key):
        """The launches of one batch on the bucket's static inputs (eagerly, and once more under capture)."""
        cap = self.capacity_words

        def pack(lo, hi, logits):                    # the planes of one pass's rows, while its logits exist
            kernels.mask_resize_pack_batch(logits, (key[0], key[1]), ent["crops"][lo:hi], self.max_orig_hw, cap, ent["bits"][lo * cap:hi * cap], self.threshold)

        state, text = self.model.mask_sweep_stages(ent["samples"], ent["tok"])
        mc = self.model.mask_sweep_pairs(state, text, ent["pair_image"], ent["pair_caption"], check=False)          # (step reads the status word)
        outputs = self.model.decode_mask_sweep(self._choose(ent, mc), self.pairs_per_pass, mask_sink=pack)
        ent["out"] = kernels.postprocess(outputs["pred_logits"], outputs["pred_boxes"], ent["sizes"], outputs.get("pred_isfinal"), out=ent["out"])

    def _planes(self, ent, p, hw):
        h, w = hw
        words = kernels.mask_words(h)
        Q, cap = self.num_queries, self.capacity_words
        return ent["bits"][p * cap:p * cap + Q * w * words].view(Q, w, words)

    def step(self, samples, tokenized, orig_sizes, sizes, pairs=None, dataset_names=None, captions=None):
        ent, sizes_p, pi, pc, live = self._step(samples, tokenized, orig_sizes, sizes, pairs, dataset_names, captions)
        results = row_results(ent["out"], self.pairs, live, self.num_queries, self.device)
        for p, r in enumerate(results):
            r["mask_bits"], r["mask_size"] = self._planes(ent, p, sizes_p[p]), sizes_p[p]
        return results, pi, pc, live

    def step_rows(self, samples, tokenized, orig_sizes, sizes, pairs=None, dataset_names=None, captions=None):
        """step() without the per-row dicts -> (out, masks, pair_image, pair_caption, live); rows from `live` on are padding."""
        from .coco_eval import RowMasks
        ent, sizes_p, pi, pc, live = self._step(samples, tokenized, orig_sizes, sizes, pairs, dataset_names, captions)
        return ent["out"], RowMasks(ent["bits"], self.capacity_words, ent["sizes"], sizes_p), pi, pc, live

    @torch.no_grad()
    def _step(self, samples, tokenized, orig_sizes, sizes, pairs, dataset_names=None, captions=None):
        from . import sweep
        if isinstance(tokenized, (list, tuple)) and len(tokenized) and isinstance(tokenized[0], str):
            if captions is None:
                captions = list(tokenized)
            tokenized = self.model.detr.transformer._tokenize(list(tokenized), self.device)
        if samples.tensors.shape[0] != self.batch or tokenized["input_ids"].shape[0] != self.captions:
            raise ValueError(f"CapturedMaskSweepStep was built for {self.batch} images and {self.captions} captions "
                             f"(got {samples.tensors.shape[0]} and {tokenized['input_ids'].shape[0]})")
        key = self.bucket_of(samples, tokenized)
        orig, crop = self.check_sizes(key, orig_sizes, sizes)                                            # ValueError before anything is launched
        pi, pc, live = sweep.pair_tables(self.batch, self.captions, pairs, capacity=self.pairs)           # the same
        rows = pi.tolist()
        sizes_p, crops_p = [orig[i] for i in rows], [crop[i] + orig[i] for i in rows]
        dataset_names, captions = self._choice_args(tokenized, dataset_names, captions)                  # the same
        if self.model.training:
            self.model.eval()
        ent = self._entry(key)
        self._fill(ent, samples, tokenized, pi, pc, sizes_p, crops_p, (tokenized, captions, dataset_names, live) if captions is not None else None)
        self._replay_checked(ent, lambda: self._forward(ent, key), lambda: None, lambda: self._handed_out(ent))
        return ent, sizes_p, pi, pc, live

    __call__ = step


class CapturedDistillStep(_CapturedStep):
    """The reference's distillation step (engine.py:152-204: teacher encode -> memory-bank update + prototypes -> teacher decode -> student encode ->
    prototype of 'something' -> student decode -> paired SetCriterion with softkd / nsthl2 + cluster losses -> backward -> clip + AdamW + EMA of both
    models) replayed from ONE hipGraph for ANY batch of a fixed shape (round 6) -- or, built without image_hw / tokens, from one
    hipGraph per input-shape BUCKET for the batches of a real loader.

    What used to tie a captured graph to its batch -- per-image target counts (LSAP problem sizes (Q - c)^2, pair tables), the grouping of the images by
    task (k-means groups, one memory-bank LSAP per task), the token tables of the captions (noun spans, the word 'something') -- now lives in
    fixed-address device images that `step()` refills before every replay: matcher.StaticTargets (one per side) and distill.DistillTables (one per
    side, attached as StaticTargets.distill); the criterion and the cluster criterion dispatch on them (SetCriterion._forward_pair_static,
    ClusterCriterion.update_memory_static / forward_static).

    step(batch) with batch = what util/misc.collate_fn delivers for (noun, pronoun) pairs (harness.synthetic_distill_batch): dict(samples=[..] * 2,
    tokenized=[..] * 2 (BatchEncodings with char_to_token), targets=[..] * 2, captions=[..] * 2, positive_map=[..] * 2) -> total loss (device scalar).
    The first step runs eagerly (a real training step) and is captured right after; later steps = the H2D copies of the inputs + one graph launch.
    Requirements (checked): one process, a batch no larger than a memory bank, both sides with the same number of targets per image (the reference's
    pairs share their boxes), images / captions of the constructor's shape when it was given one.

    Shape buckets: the reference resizes and crops every image at random, pads a batch to its largest image and tokenises the noun and the pronoun
    caption separately (datasets/tdod.py:301-325), so no two batches of a real loader share a shape and the two sides of a batch differ in caption
    length.  The bucket of a batch is (Hp, Wp, Lp): the pair's padded image size rounded up to `pad_hw` (the extra pixels are masked, as in
    CapturedTrainStep) and the LONGER caption length of the two sides rounded up to `pad_tokens`.  Padded token positions are masked in every
    attention and carry zero weights in the caption tables; loss_contrastive_align, which has no attention mask (mdetr.py:646-663), reads each
    side's OWN token count from the live-token word of that side's matcher.LiveStaticTargets (toist_contrastive_fwd_live), so a bucket gives the losses of the
    unpadded batch.  Each bucket holds both sides' static inputs, StaticTargets and DistillTables and its graph, built on first use and kept in an
    LRU of `max_graphs`; what is NOT per bucket: the memory banks, cluster centres and plan_fill's host mirror (one ClusterCriterion), the FillTables
    image (attached to every bucket's tables), the optimizers, the guard words and the programs' reused gradient buffers.  plan_fill runs once per
    step in step order, whichever bucket serves the step.

    The memory state is the device's business: the same graph serves a fresh run (every bank filling, FIFO pushes, k-means from randomly drawn bank
    rows), the step on which a task's full_label flips, the steady state (nearest replacement, k-means from the stored centres) and --fifo_memory.
    toist_bank_fifo reads update_count / full_label and decides per task; toist_kmeans_init reads full_label and decides per sample.  The host's only
    part is ClusterCriterion.plan_fill in step(): it advances the host mirror of the two counters and spends the np.random.choice draws the reference
    would spend, in its order, into a distill.FillTables image (so np.random.seed pins a run as it pins the reference's).  pack() stays stateless.
    After writing update_count / full_label directly, or loading a checkpoint, ClusterCriterion.sync_host_state() (load_state_dict calls it) re-reads
    the mirror; a disagreement between mirror and device raises at a later step (ClusterCriterion.check_start_status).

    A bad step is handled as in CapturedTrainStep: fatal for both models' training state unless BOTH optimizers were built with skip_nonfinite=True;
    then the step is skipped on the device and resolve_skipped() reports it (the loss word and the decoder status word are shared by the two tails, so
    they skip together; a gradient norm that is not finite in one model only skips that model's update)."""

    def __init__(self, model, model_noun, criterion, cluster_criterion, optimizers, weight_dict, *, batch, image_hw=None, tokens=None,
                 max_targets_per_image=16, pad_hw=64, pad_tokens=8, max_graphs=4, device=None, stream=None):
        """image_hw + tokens: the one shape the step serves (one graph).  Neither: the step is BUCKETED (class docstring) -- pad_hw, pad_tokens and
        max_graphs are CapturedTrainStep's.
        stream: the HIP stream the steps run (and the graph is captured) on; pass the stream earlier eager steps of the same models ran on, if any -- the programs'
        reused gradient buffers and the launchers' per-stream scratch must not change streams between eager steps and the capture."""
        if (image_hw is None) != (tokens is None):
            raise ValueError("CapturedDistillStep: pass image_hw AND tokens (one fixed shape, one graph) or neither (shape buckets)")
        from . import engine
        from .distill import FillTables
        from .matcher import LiveStaticTargets
        self.model, self.model_noun, self.criterion, self.cluster_criterion = model, model_noun, criterion, cluster_criterion
        self.optimizers, self.weight_dict = list(optimizers), weight_dict
        self.B, self.max_t, self.bucketed = int(batch), int(max_targets_per_image), image_hw is None
        self.pad_hw, self.pad_tokens, self.max_graphs = (int(pad_hw), int(pad_tokens), int(max_graphs)) if self.bucketed else (1, 1, 1)
        dev = self.device = torch.device(device) if device is not None else next(model.parameters()).device
        det = getattr(model, "detr", model)
        self.num_queries = det.query_embed.weight.shape[0]
        self.contrastive = bool(getattr(det, "contrastive_align_loss", False))
        self.fill = None                                   # (without a cluster criterion there is no memory to fill)
        if cluster_criterion is not None:                  # ONE image of the k-means starts (a function of B and K alone), attached to every bucket's pair of tables
            self.fill = FillTables(self.B, cluster_criterion.cluster_num, cluster_criterion.memory_size, dev)
        self._init_capture_state(side=stream if stream is not None else torch.cuda.Stream(device=dev))
        self._pack_tb = {}                                 # Lp -> the (noun, pronoun) DistillTables whose pack() builds the host images of that caption length
        if self.bucketed:
            self.hw = self.L = self.sides = None
            # pack() must not depend on which buckets exist (it may run ahead of step(), in a loader): the targets' host image has one layout for every
            # bucket, so one StaticTargets packs both sides of all of them; the caption tables depend on Lp and get host-only packers on first use
            self._pack_st = [LiveStaticTargets(self.B, self.max_t, self.num_queries, 256, dev)] * 2
        else:
            self.hw, self.L = (int(image_hw[0]), int(image_hw[1])), int(tokens)
            self._ent = self._entry((*self.hw, self.L))    # the one bucket
            self.sides = self._ent["sides"]
            self._pack_st = [side["targets"] for side in self.sides]
            self._pack_tb[self.L] = [side["targets"].distill for side in self.sides]
        if kernels.SEED_DEV is None:
            kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
        engine.REUSE_GRAD_BUFFERS = True
        self._init_guard(self.optimizers)

    def _static_inputs(self, key):
        """Both sides' static inputs of one bucket.  Fixed shape: every batch overwrites the whole mask (mask_fill=False) and no caption is padded.
        Bucketed: the usual blank-is-padding inputs, and each side's targets are a LiveStaticTargets, whose live-token word keeps the padded token columns
        out of loss_contrastive_align."""
        from .distill import DistillTables
        from .matcher import LiveStaticTargets, StaticTargets
        Hp, Wp, Lp = key
        sides = []
        for pronoun in (False, True):
            st = (LiveStaticTargets if self.bucketed else StaticTargets)(self.B, self.max_t, self.num_queries, 256, self.device)
            st.distill = DistillTables(self.B, Lp, self.device, pronoun_side=pronoun)
            sides.append({**static_inputs(self.B, Hp, Wp, Lp, _pad_id(self.model), self.device, mask_fill=self.bucketed), "targets": st})
        if self.fill is not None:
            self.fill.attach(sides[0]["targets"].distill, sides[1]["targets"].distill)
        return {"sides": sides, **_NO_GRAPH}

    def bucket_of_pair(self, batch):
        """(Hp, Wp, Lp) of a pair batch (host logic only): the pair's padded image size rounded up to pad_hw -- the two sides are the same images --,
        the LONGER of the two sides' captions rounded up to pad_tokens."""
        shapes = [tuple(s.tensors.shape) for s in batch["samples"]]
        if shapes[0] != shapes[1]:
            raise ValueError(f"CapturedDistillStep: the two sides of a pair are the same images, got {shapes[0]} (noun) and {shapes[1]} (pronoun)")
        if shapes[0][0] != self.B or any(int(t["input_ids"].shape[0]) != self.B for t in batch["tokenized"]):
            raise ValueError(f"CapturedDistillStep was built for batches of {self.B} pairs (got {shapes[0][0]} images, "
                             f"{[int(t['input_ids'].shape[0]) for t in batch['tokenized']]} captions)")
        longer = max(int(t["input_ids"].shape[1]) for t in batch["tokenized"])
        return round_up(shapes[0][2], self.pad_hw), round_up(shapes[0][3], self.pad_hw), round_up(longer, self.pad_tokens)

    def _table_packers(self, Lp):
        tb = self._pack_tb.get(Lp)
        if tb is None:
            from .distill import DistillTables
            tb = self._pack_tb[Lp] = [DistillTables(self.B, Lp, "cpu", pronoun_side=pronoun) for pronoun in (False, True)]
            for t in tb:
                t._pin = self.device.type == "cuda"        # (host-only instances: their pack() results are what step() copies to the bucket's tables)
        return tb

    def pack(self, batch):
        """Host half of a step (no device work, no synchronisation when the batch's targets are host tensors: run it in the loader): the pinned images of both
        sides' StaticTargets and DistillTables, next to the batch's image / token tensors and the batch's bucket ("key").  step(packed=...) consumes it."""
        if [len(t["boxes"]) for t in batch["targets"][0]] != [len(t["boxes"]) for t in batch["targets"][1]]:
            raise ValueError("softkd needs the same number of targets on the noun and the pronoun side of every pair")
        key = self.bucket_of_pair(batch) if self.bucketed else (*self.hw, self.L)
        tables = self._table_packers(key[2])
        out = []
        for i in range(2):
            samples, tok, targets = batch["samples"][i], batch["tokenized"][i], batch["targets"][i]
            if not self.bucketed and (tuple(samples.tensors.shape) != (self.B, 3, *self.hw) or tuple(tok["input_ids"].shape) != (self.B, self.L)):
                raise ValueError(f"CapturedDistillStep was built for {self.B} x 3 x {self.hw[0]} x {self.hw[1]} images and {self.L}-token captions")
            host_t = host_targets(targets)
            masks = self.criterion.token_masks_host(host_t, tok) if self.contrastive else None
            live = {"live_tokens": int(tok["input_ids"].shape[1])} if self.bucketed else {}       # each side's OWN caption length
            out.append({"samples": samples, "tok": tok, "key": key,
                        "targets": self._pack_st[i].pack(host_t, host_positive_map(batch["positive_map"][i]), masks, **live),
                        "tables": tables[i].pack(tok, host_t, batch["captions"][i])})
        return out

    def _plan(self, packed):
        """The stateful host half of a step, once per step and in step order, whichever bucket serves the step: the k-means starts of the samples whose
        bank is filling (ClusterCriterion.plan_fill on the task columns of the packed tables)."""
        if self.fill is None:
            return None
        tasks = [tb._views(pk["tables"])[4].tolist() for tb, pk in zip(self._table_packers(packed[0]["key"][2]), packed)]
        return self.cluster_criterion.plan_fill(*tasks)

    def _fill(self, ent, packed, starts):
        for side, pk in zip(ent["sides"], packed):
            upload(side, pk["samples"], pk["tok"])
            side["targets"].load_packed(pk["targets"])
            side["targets"].distill.load_packed(pk["tables"])
        if starts is not None:
            self.fill.load(*starts)

    def _fwd_bwd_opt(self, ent):
        """One step on the static inputs of `ent`.  The backward pass is issued in TWO calls -- the teacher's total (the noun_ keys) first, then everything else (sth_, softkd, nsthl2, cluster:
        the student's) -- which changes no gradient (the two models' graphs are disjoint: the teacher enters the cross losses detached, mdetr.py:520-599, 668-781)
        but lets a captured step run the teacher's backward beside the softkd assignment problems, which occupy 24 CUs for ~3.6 ms on a side stream
        (SetCriterion._forward_pair_static)."""
        from .harness import distillation_losses
        from .mdetr import weighted_total
        kernels.SEED_DEV.add_(1000003)
        noun, sth = ent["sides"]
        static = {"samples": [noun["samples"], sth["samples"]], "targets": [noun["targets"], sth["targets"]], "captions": [None, None],
                  "tokenized": [noun["tok"], sth["tok"]], "positive_map": [None, None]}
        self.criterion.defer_pair_join = True          # the softkd block may go to a side stream: this method joins it (below) before the student's total
        try:
            losses = distillation_losses(self.model, self.model_noun, self.criterion, self.cluster_criterion, static)
        finally:
            self.criterion.defer_pair_join = False
        w_noun = {k_: v for k_, v in self.weight_dict.items() if k_.startswith("noun_")}
        w_rest = {k_: v for k_, v in self.weight_dict.items() if not k_.startswith("noun_")}
        total_noun = weighted_total(losses, w_noun)
        total_noun.backward()
        join = getattr(losses, "join", None)
        if join is not None:
            torch.cuda.current_stream().wait_stream(join)
        total_rest = weighted_total(losses, w_rest)
        total_rest.backward()
        total = (total_noun + total_rest).detach()
        if self._loss_word is not None:
            self._loss_word.copy_(total)               # the guard's finite-loss check, as in CapturedTrainStep
        for o in self.optimizers:
            o.step()
        return total

    def _zero_grad(self):
        for o in self.optimizers:
            o.zero_grad(set_to_none=True)

    def step(self, batch=None, packed=None):
        batch = packed if packed is not None else self.pack(batch)
        if _is_distributed():
            raise RuntimeError("CapturedDistillStep is single-process (the memory-bank queue all_gathers rows across ranks: collectives are not captured)")
        ent = self._entry(batch[0]["key"])
        starts = self._plan(batch)
        if ent["graph"] is None:
            out = self._eager_then_capture(ent, lambda: self._fwd_bwd_opt(ent), reset=self._zero_grad, upload=lambda: self._fill(ent, batch, starts))
            if self.fill is not None:
                self.cluster_criterion.check_start_status(defer=True)
            return out
        side = self._side                                  # (unlike CapturedTrainStep / CapturedEvalStep, upload and replay stay on the stream of the capture)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._fill(ent, batch, starts)
            ent["graph"].replay()
            if self.fill is not None:
                self.cluster_criterion.check_start_status(defer=True)
        torch.cuda.current_stream().wait_stream(side)
        return self._replayed(ent, self.optimizers)

    __call__ = step
