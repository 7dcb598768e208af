"""Noun -> pronoun distillation pieces of TOIST (BASELINE config 5).

Mirrors the reference's ClusterCriterion (/root/reference/models/mdetr.py:29-312), its k-means
(/root/reference/models/kmeans.py) and the char-span -> token-span lookup shared by the contrastive, nsthl2 and
cluster code (mdetr.py:112-141, 614-643, 684-711).  Everything stays on the device: the memory-bank
replacement assignment (mdetr.py:98-103) runs on the HIP LSAP kernel instead of SciPy on the host, k-means
is a handful of device tensor ops per iteration ([1024, 256] bank, 3 centres), and nothing calls `.cpu()`.
Buffer names and shapes equal the reference's, so a reference checkpoint of the criterion loads unchanged.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import staging
from .devcache import DeviceCache
from .matcher import linear_sum_assignment_batch


# ---- char spans -> token positions --------------------------------------------------------------------------
def char_span_to_tokens(tokenized, batch_index, beg, end):
    """(first, last) token of the character span [beg, end) of caption `batch_index`, or None.  Same lookup
    and the same fallbacks as the reference (note that its retries drop the batch index, mdetr.py:126-139)."""
    first = tokenized.char_to_token(batch_index, beg)
    last = tokenized.char_to_token(batch_index, end - 1)
    if first is None:
        try:
            first = tokenized.char_to_token(beg + 1)
            if first is None:
                first = tokenized.char_to_token(beg + 2)
        except Exception:
            first = None
    if last is None:
        try:
            last = tokenized.char_to_token(end - 2)
            if last is None:
                last = tokenized.char_to_token(end - 3)
        except Exception:
            last = None
    if first is None or last is None:
        return None
    return first, last


def span_positions(tokenized, batch_index, spans, length):
    """int64 token positions (ascending, unique) covered by a list of character spans."""
    hit = torch.zeros(length, dtype=torch.bool)
    for beg, end in spans:
        ft = char_span_to_tokens(tokenized, batch_index, beg, end)
        if ft is not None:
            hit[ft[0]:ft[1] + 1] = True
    return hit.nonzero().reshape(-1)


# Caption-driven index tables of a batch (token weights, substitution masks, task columns) are built once on the host and kept on the device while the
# batch's objects are alive: the steps that use them issue no host -> device copy and read nothing back, so the launch queue never drains inside a
# training step (every small pageable upload is a stream synchronisation).  Keyed by object identity; the entry holds the objects, so an id cannot be reused.
_TABLES = DeviceCache(limit=64, lru=True)


def _tok_ref(tokenized):
    """the object whose identity stands for a tokenized batch: its input_ids tensor when there is one (Transformer._tokenize wraps the caller's dict in a
    new TokenizedText on every call, the tensors inside stay the same objects), else the tokenized object itself"""
    try:
        ids = tokenized["input_ids"]
        if torch.is_tensor(ids):
            return ids
    except Exception:
        pass
    return tokenized


def _cached_table(kind, refs, extra, make):
    # identity + in-place version of tensor refs: a caller that refills a static input_ids buffer in place (a captured step's feed) bumps
    # Tensor._version, so a table built for the previous contents is not served again
    key = (kind, tuple((id(r), r._version) if torch.is_tensor(r) else id(r) for r in refs), extra)
    return _TABLES.get(key, make, pin=refs)


def span_tables(tokenized, targets, L):
    """Host tables of the noun spans of a batch -> (W f32 [B, L], sub u8 [L, B]).  W[i, l] = sum over the boxes of image i of [token l belongs to the box's
    noun spans] / (tokens of the box x boxes of the image), so that W @ text_feature[i] is the reference's mean over boxes of the mean over each box's noun
    tokens (mdetr.py:112-145, 684-711); a box without any token makes the reference average an empty set: the row is NaN, as there.  sub[l, i]: token l of
    image i receives the prototype on the teacher side (images without boxes: none)."""
    W = np.zeros((len(targets), L), dtype=np.float32)
    sub = np.zeros((L, len(targets)), dtype=np.uint8)
    for i, tgt in enumerate(targets):
        boxes = tgt["noun_tokens_positive"]
        for spans in boxes:
            pos = span_positions(tokenized, i, spans, L).numpy()
            if len(pos) == 0:
                W[i, :] = np.nan
            else:
                W[i, pos] += np.float32(1.0 / (len(pos) * len(boxes)))
        if len(tgt["boxes"]) != 0:
            sub[span_positions(tokenized, i, [s_ for box in boxes for s_ in box], L).numpy(), i] = 1
    return W, sub


def something_tables(tokenized, captions, L):
    """Host tables of the word 'something' of every caption (mdetr.py:240-260) -> (W f32 [B, L] mean weights of its tokens, sub u8 [L, B], the token
    positions per caption)."""
    W = np.zeros((len(captions), L), dtype=np.float32)
    sub = np.zeros((L, len(captions)), dtype=np.uint8)
    positions = []
    for i, caption in enumerate(captions):
        beg = caption.find("something")
        first, last = (tokenized.char_to_token(i, beg), tokenized.char_to_token(i, beg + len("something") - 1)) if beg >= 0 else (None, None)
        if first is None or last is None:      # (the reference fails here too: mdetr.py:240-246 indexes with the None it gets back)
            raise ValueError(f"pronoun caption {i} ({caption!r}) has no token for the word 'something'")
        pos = np.arange(first, last + 1)
        positions.append(pos)
        if len(pos) == 0:
            W[i, :] = np.nan                   # the reference averages an empty set there
        else:
            W[i, pos] = np.float32(1.0 / len(pos))
            sub[pos, i] = 1
    return W, sub, positions


def task_groups(tasks):
    """The images grouped by task, in batch order inside a group; tasks: one index per image, -1 = the image takes no part.
    -> (group_task, group_off, members) as lists (csrc/kmeans.hip, the per-task LSAP of the memory-bank update)."""
    live = [(i, t) for i, t in enumerate(tasks) if t >= 0]
    order = sorted(set(t for _, t in live))
    members, off = [], [0]
    for t in order:
        members += [i for i, tt in live if tt == t]
        off.append(len(members))
    return order, off, members


def _noun_tables(tokenized, targets, L, device):
    """span_tables on the device (W f32, sub bool), cached while the batch's objects are alive."""
    def make():
        W, sub = span_tables(tokenized, targets, L)
        return torch.from_numpy(W).to(device), torch.from_numpy(sub).bool().to(device)
    return _cached_table("noun_w", (_tok_ref(tokenized), *targets), (L, str(device)), make)


def noun_token_weights(tokenized, targets, L, device):
    """fp32 [B, L] device copy of span_tables' W."""
    return _noun_tables(tokenized, targets, L, device)[0]


def noun_token_features(text_feature, tokenized, targets):
    """[B, d]: per image, the mean over its boxes of the mean text feature of each box's noun tokens
    (mdetr.py:112-145, 684-711); zero rows for images without boxes.  One weighted sum over the tokens with host-built, device-cached weights."""
    W = noun_token_weights(tokenized, targets, text_feature.shape[1], text_feature.device).to(text_feature.dtype)
    return (W.unsqueeze(-1) * text_feature).sum(1)


def task_index(dataset_name):
    """'task_3_train.json' -> 2 (mdetr.py:162)."""
    return int(dataset_name.split("_")[1]) - 1


# ---- the same tables at FIXED device addresses: one hipGraph of the distillation step serves any batch ------------------------------------
class DistillTables:
    """Fixed-address device image of ONE side's (noun or pronoun) caption-driven tables, the counterpart of matcher.StaticTargets for the distillation
    losses (round 6): the captured step reads every per-batch index from these buffers, `load()` refills them between replays
    (one pinned staging arena, one asynchronous H2D copy, no host sync).  `matcher.StaticTargets.distill` carries the side's tables into
    ClusterCriterion.update_memory / forward and SetCriterion.

    Arena (B = batch, L = tokens of the bucket):
      W_span  f32 [B, L]   noun_token_weights(): W @ text_memory[i] = mean over the image's boxes of the mean over each box's noun tokens (mdetr.py:112-145)
      W_sth   f32 [B, L]   mean weights of the tokens of the word 'something' in the caption (mdetr.py:240-260); zeros on the noun side
      sub_span u8 [L, B]   tokens that receive the prototype on the teacher side (images without boxes: none)
      sub_sth  u8 [L, B]   tokens of 'something'
      task    i32 [B]      task index of the image (dataset_name), -1 = the image takes no part (teacher side: no boxes)
      group_task i32 [B] | group_off i32 [B + 1] | members i32 [B]    the images grouped by task, in batch order inside a group (csrc/kmeans.hip, the
                           per-task LSAP of the memory-bank update); unused groups are empty (group_off stays at the member count).
    What depends on the fill state of the banks rather than on the batch -- the k-means start rows -- is not packed here (pack() stays stateless): a
    FillTables image attached to the two sides adds `init_rows` i32 [B, K]."""

    def __init__(self, batch, tokens, device, pronoun_side):
        self.B, self.L, self.pronoun_side = int(batch), int(tokens), bool(pronoun_side)
        self.device = torch.device(device)
        B, L = self.B, self.L                                    # nbytes: the size of the arena = of a pack()ed host image
        self._views, self.nbytes = staging.typed_views([(torch.float32, (B, L)), (torch.float32, (B, L)), (torch.uint8, (L, B)), (torch.uint8, (L, B)),
                                                        (torch.int32, (B,)), (torch.int32, (B,)), (torch.int32, (B + 1,)), (torch.int32, (B,))])
        self._pin = self.device.type == "cuda"                   # (a host-only instance packs tables in the CPU tests)
        self._stage = staging.Staging(torch.zeros(self.nbytes, dtype=torch.uint8), self.device)
        self._dev = torch.zeros(self.nbytes, dtype=torch.uint8, device=self.device)
        self.W_span, self.W_sth, self.sub_span, self.sub_sth, self.task, self.group_task, self.group_off, self.members = self._views(self._dev)

    def _staging(self, out):
        host = out if out is not None else torch.zeros(self.nbytes, dtype=torch.uint8)
        if out is None and self._pin:
            host = host.pin_memory()
        host.zero_()
        return host, [v.numpy() for v in self._views(host)]

    def pack(self, tokenized, targets, captions=None, out=None):
        """Host image of one batch.  tokenized: the side's BatchEncoding (needs char_to_token); targets: the side's list of dicts with `noun_tokens_positive`,
        `dataset_name`, `boxes`; captions: list[str] (pronoun side: where the word 'something' sits)."""
        if len(targets) != self.B:
            raise ValueError(f"DistillTables holds {self.B} images; got {len(targets)}")
        host, (W_span, W_sth, sub_span, sub_sth, task, group_task, group_off, members) = self._staging(out)
        W_span[:], sub_span[:] = span_tables(tokenized, targets, self.L)
        if self.pronoun_side:
            W_sth[:], sub_sth[:], _ = something_tables(tokenized, captions[:self.B], self.L)
            tasks = [task_index(t["dataset_name"]) for t in targets]               # the student clusters EVERY sample (mdetr.py:230-277)
        else:
            tasks = [-1 if len(t["boxes"]) == 0 else task_index(t["dataset_name"]) for t in targets]
        self._pack_groups(tasks, task, group_task, group_off, members)
        return host

    def pack_eval(self, tokenized, captions, dataset_names, out=None):
        """Host image of one EVALUATION batch (pronoun side): what the prototype choice of inference reads (mdetr.py:282-312) -- W_sth, sub_sth, task and
        the grouping by task -- from the tokenized captions (char_to_token), the caption strings and the dataset names alone.  No targets: W_span /
        sub_span stay zero (only the teacher's bank update reads them)."""
        if not self.pronoun_side:
            raise ValueError("pack_eval fills the pronoun side's tables")
        if len(captions) != self.B or len(dataset_names) != self.B:
            raise ValueError(f"DistillTables holds {self.B} images; got {len(captions)} captions and {len(dataset_names)} dataset names")
        host, (_, W_sth, _, sub_sth, task, group_task, group_off, members) = self._staging(out)
        W_sth[:], sub_sth[:], _ = something_tables(tokenized, captions, self.L)
        self._pack_groups([task_index(n) for n in dataset_names], task, group_task, group_off, members)
        return host

    @staticmethod
    def _pack_groups(tasks, task, group_task, group_off, members):
        """task_groups into the arena's views; unused groups are empty (group_off stays at the member count)."""
        order, off, mem = task_groups(tasks)
        task[:] = np.asarray(tasks, dtype=np.int32)
        group_task[:len(order)] = order
        group_off[:len(off)] = off
        group_off[len(off):] = len(mem)
        members[:len(mem)] = mem

    def load_packed(self, host):
        self._dev.copy_(host, non_blocking=True)
        return self

    def load(self, tokenized, targets, captions=None):
        self._stage.upload((self._dev, self.pack(tokenized, targets, captions, out=self._stage.open())))
        return self

    def load_eval(self, tokenized, captions, dataset_names):
        """pack_eval() into the internal staging buffer + the copy."""
        self._stage.upload((self._dev, self.pack_eval(tokenized, captions, dataset_names, out=self._stage.open())))
        return self


class FillTables:
    """Fixed-address device image of one step's k-means starts, the sibling of DistillTables for what is NOT a function of the batch alone: the bank rows
    ClusterCriterion.plan_fill drew for the samples whose task is still filling (the draws depend on the fill state and on the np.random stream, so
    they are made in step(), never in a loader's pack()).  One pinned staging arena, one asynchronous copy per step, no host sync.

    Arena: init i32 [2, B, K] -- side (0 = noun / teacher, 1 = pronoun / student), sample, centre; -1 rows = start from the stored centres.
    `attach(noun_tables, sth_tables)` hands each side's DistillTables its [B, K] view as `.init_rows`; _cluster_static reads it from there."""

    def __init__(self, batch, cluster_num, memory_size, device):
        self.B, self.K = int(batch), int(cluster_num)
        if self.B > int(memory_size):
            raise ValueError(f"a batch of {self.B} images does not fit a memory bank of {int(memory_size)} rows")
        self.device = torch.device(device)
        self._stage = staging.Staging(torch.full((2, self.B, self.K), -1, dtype=torch.int32), self.device)
        self.init = torch.full((2, self.B, self.K), -1, dtype=torch.int32, device=self.device)

    def attach(self, noun_tables, sth_tables):
        noun_tables.init_rows, sth_tables.init_rows = self.init[0], self.init[1]
        return self

    def pack(self, init_noun, init_sth, out=None):
        host = out if out is not None else torch.empty((2, self.B, self.K), dtype=torch.int32)
        for side, rows in enumerate((init_noun, init_sth)):
            rows = np.asarray(rows, dtype=np.int32)
            if rows.shape != (self.B, self.K):
                raise ValueError(f"FillTables holds {self.B} x {self.K} start rows per side; got {rows.shape}")
            host[side].copy_(torch.from_numpy(rows))
        return host

    def load(self, init_noun, init_sth):
        self._stage.upload((self.init, self.pack(init_noun, init_sth, out=self._stage.open())))
        return self


class SweepChoiceTables:
    """Fixed-address device image of what the prototype choice of a task sweep reads per CAPTION (toist_sweep_prototypes): the sibling of
    DistillTables for a batch whose rows are (image, caption) PAIRS.  Nothing here is indexed by pair -- the launch finds a pair's caption in the
    sweep's own pair_caption table -- so the image changes only when the captions, their tasks or the number of live pairs do.

    Arena (T = captions, L = tokens of the bucket):
      W_sth    f32 [T, L]   mean weights of the tokens of the word 'something' in caption t (something_tables)
      sub_sth   u8 [T, L]   tokens of 'something'
      cap_task i32 [T]      task index of the caption (its dataset name)
      group_task i32 [T]    the distinct tasks in first-appearance order, one group slot (= workgroup) each; -1 in unused slots.  Two captions of one
                            task share a slot: the walk over the pairs keeps the reference's order inside a task whatever the captions are.
      live     i32 [1]      the pairs p >= live are padding: they never enter the k-means walk
    `memory_mod` (bf16 [P * S, d], allocated by ClusterCriterion.infer_choice_pairs on first use) hangs off the same object: both belong to a bucket."""

    def __init__(self, captions, tokens, device):
        self.T, self.L = int(captions), int(tokens)
        self.device = torch.device(device)
        T, L = self.T, self.L
        self._views, self.nbytes = staging.typed_views([(torch.float32, (T, L)), (torch.uint8, (T, L)), (torch.int32, (T,)), (torch.int32, (T,)),
                                                        (torch.int32, (1,))])
        self._stage = staging.Staging(torch.zeros(self.nbytes, dtype=torch.uint8), self.device)
        self._dev = torch.zeros(self.nbytes, dtype=torch.uint8, device=self.device)
        self.W_sth, self.sub_sth, self.cap_task, self.group_task, self.live = self._views(self._dev)
        self.group_task.fill_(-1)                                # (until the first load every slot is unused)
        self._loaded = None                                      # the host image the device holds
        self.memory_mod = None

    def pack(self, tokenized, captions, dataset_names, live, out=None):
        """Host image (uint8 [nbytes]) of one sweep.  tokenized: the T captions' BatchEncoding (needs char_to_token); captions / dataset_names: T
        strings each; live: the number of live pairs.  Needs no device."""
        if len(captions) != self.T or len(dataset_names) != self.T:
            raise ValueError(f"SweepChoiceTables holds {self.T} captions; got {len(captions)} captions and {len(dataset_names)} dataset names")
        if isinstance(live, bool) or int(live) != live or int(live) < 0:
            raise ValueError(f"SweepChoiceTables: live = {live!r} is not a count of pairs")
        host = out if out is not None else torch.zeros(self.nbytes, dtype=torch.uint8)
        host.zero_()
        W_sth, sub_sth, cap_task, group_task, live_w = (v.numpy() for v in self._views(host))
        W, sub, _ = something_tables(tokenized, list(captions), self.L)
        W_sth[:], sub_sth[:] = W, sub.T
        tasks = [task_index(n) for n in dataset_names]
        if any(t < 0 for t in tasks):
            raise ValueError(f"SweepChoiceTables: dataset names {list(dataset_names)!r} name a task below 1")
        order = list(dict.fromkeys(tasks))                       # distinct, first appearance first
        cap_task[:] = tasks
        group_task[:] = -1
        group_task[:len(order)] = order
        live_w[0] = int(live)
        return host

    def load(self, tokenized, captions, dataset_names, live):
        """pack() and, when the image differs from what the device holds, one copy through the staging buffer -> whether it was uploaded."""
        host = self.pack(tokenized, captions, dataset_names, live)
        if self._loaded is not None and torch.equal(host, self._loaded):
            return False
        stage = self._stage.open()
        stage.copy_(host)
        self._stage.upload((self._dev, stage))
        self._loaded = host
        return True

    def invalidate(self):
        """The next load() uploads whatever it packs (the owner's pair tables were refused: nothing on the device is trusted)."""
        self._loaded = None


# ---- k-means (kmeans.py) ---------------------------------------------------------------------------------------
def _sq_dist(x, centers):
    return ((x.unsqueeze(1) - centers.unsqueeze(0)) ** 2.0).sum(-1)


def kmeans(X, init_cluster_centers, num_clusters, tol=1e-4, full_label=0):
    """Lloyd iterations until (sum_k |shift_k|)^2 < tol (kmeans.py:21-94).  With full_label == 0 the start is
    `np.random.choice` rows of X (kmeans.py:8-18), drawn from the global np.random stream exactly as the reference draws them: under the same
    np.random.seed the fill phase equals the reference's step by step (tests/golden/distill_fill.npz)."""
    X = X.float()
    if full_label == 0:
        centers = X[torch.as_tensor(np.random.choice(len(X), num_clusters, replace=False), device=X.device)].clone()
    else:
        centers = init_cluster_centers
    while True:
        choice = torch.argmin(_sq_dist(X, centers), dim=1)
        before = centers.clone()
        for c in range(num_clusters):          # K = 3: the reference's own per-cluster mean (same reduction order)
            members = X[choice == c]
            if len(members) != 0:              # an empty cluster keeps its centre (kmeans.py:72)
                centers[c] = members.mean(dim=0)
        shift = torch.sqrt(((centers - before) ** 2).sum(1)).sum()
        if float(shift) ** 2 < tol:
            return choice, centers


def kmeans_predict(X, centers):
    return torch.argmin(_sq_dist(X.float(), centers), dim=1)


# ---- ClusterCriterion ------------------------------------------------------------------------------------------
class ClusterCriterion(nn.Module):
    """Per-task memory bank of noun text features + k-means prototypes (mdetr.py:29-312)."""

    def __init__(self, feature_dim, memory_size, cluster_num, task_count, args):
        super().__init__()
        self.args = args
        self.feature_dim, self.memory_size, self.cluster_num, self.task_count = feature_dim, memory_size, cluster_num, task_count
        self.register_buffer("feature_bank", torch.randn(task_count, memory_size, feature_dim))
        self.register_buffer("cluster_centers", torch.randn(task_count, cluster_num, feature_dim))
        self.register_buffer("update_count", torch.zeros(task_count))
        self.register_buffer("full_label", torch.zeros(task_count))
        self._start_mail = staging.Mailbox()          # toist_kmeans_init's status word and its copies on their way to the host (check_start_status)

    @staticmethod
    def _world():
        return torch.distributed.get_world_size() if torch.distributed.is_available() and torch.distributed.is_initialized() else 1

    def syn_memory(self):
        """Average the banks and centres over the ranks (mdetr.py:54-61)."""
        world = self._world()
        if world > 1:
            torch.distributed.all_reduce(self.feature_bank)
            torch.distributed.all_reduce(self.cluster_centers)
        self.feature_bank /= world
        self.cluster_centers /= world

    _MEMBERS = DeviceCache(limit=512)

    @staticmethod
    def _members(tasks, t, device):
        """int64 device indices of the rows whose task is t, cached per task signature (no upload in steady state)"""
        return ClusterCriterion._MEMBERS.get((tuple(tasks), t, str(device)),
                                             lambda: torch.tensor([i for i, x in enumerate(tasks) if x == t], dtype=torch.int64, device=device))

    def update_memory_queue(self, feature_idx, tasks_host=None):
        """feature_idx [B, d+1]: feature | task index (-1 = none).  All ranks' rows enter every rank's bank in rank
        order (mdetr.py:63-103): FIFO until a task's bank has been filled, then FIFO or nearest-replacement.
        tasks_host: the task column as a host list when the caller knows it (one rank: the targets' dataset names) -- nothing is read back then."""
        world = self._world()
        if world > 1:
            parts = [torch.zeros_like(feature_idx) for _ in range(world)]
            torch.distributed.all_gather(parts, feature_idx)
            feature_idx = torch.cat(parts, 0)
            tasks_host = None
        if tasks_host is not None:
            tasks = [int(t) for t in tasks_host]
        else:
            tasks = feature_idx[:, -1].round().to(torch.int64).tolist()   # one host read per step; the values are small integers
        full = self._full_host()
        count = self.__dict__["_count_mirror"]
        for t in sorted(set(tasks) - {-1}):
            new = feature_idx.index_select(0, self._members(tasks, t, feature_idx.device))[:, :-1]
            n = new.shape[0]
            bank = self.feature_bank[t]
            filling = not full[t]
            if filling or self.args.fifo_memory:
                bank.copy_(torch.cat([bank[n:], new], 0))
                if filling:
                    if count[t] > self.memory_size:
                        self.full_label[t] = 1
                        full[t] = True
                    self.update_count[t] += n
                    count[t] += n
            else:   # replace the entries closest (L1) to the new features: one LSAP on the device
                # SciPy raises on an invalid matrix (mdetr.py:100) BEFORE the bank is touched.  The status check here is deferred (no host
                # sync per step), so the write itself is gated on the device: an invalid / infeasible problem leaves the bank as it was
                # and the ValueError surfaces at the next deferred check (or state_dict() / check_lsap_pending()).
                ((rows, cols),), status = linear_sum_assignment_batch([torch.cdist(new, bank, p=1)], defer_status=True, with_status=True)
                bank[cols] = torch.where(status[0] == 0, new[rows], bank[cols])

    # ---- device path: every sample of the batch in ONE launch, no host read (csrc/kmeans.hip) -------------------------------
    _INDEX_TABLES = DeviceCache(limit=256)

    def cluster_batch(self, features, tasks):
        """memory_cluster for all samples of a batch at once.  features [B, d] (device), tasks: host list, one task index per
        sample or None (sample skipped).  Samples of the same task are processed in batch order by one workgroup (a later sample starts
        from the centres an earlier one left, as in the sequential reference); the centres are updated in place.  Returns
        (pick int32 [B], chosen centre [B, d]) on the device, or None when a bank involved is still filling (random initialisation on
        the host, kmeans.py:8-18: the per-sample host path handles that phase)."""
        live = [(i, t) for i, t in enumerate(tasks) if t is not None]
        if not live or not features.is_cuda:
            return None
        full = self._full_host()
        if any(not full[t] for _, t in live):
            return None
        group_task, group_off, members = ClusterCriterion._INDEX_TABLES.get(
            (tuple(tasks), str(features.device)),
            lambda: tuple(torch.tensor(v, dtype=torch.int32, device=features.device) for v in task_groups([-1 if t is None else t for t in tasks])))
        B, d = features.shape
        pick = torch.zeros(B, dtype=torch.int32, device=features.device)
        chosen = torch.zeros(B, d, dtype=torch.float32, device=features.device)
        from . import kernels as k
        k.kmeans(self.feature_bank, self.cluster_centers, group_task, group_off, members, features.detach().float().contiguous(), 1e-4, 10000, pick, chosen)
        return pick, chosen

    def _full_host(self):
        """Host mirror of full_label (one read, then kept in step by update_memory_queue; call sync_host_state() after writing the
        buffers directly or loading a checkpoint)."""
        m = self.__dict__.get("_full_mirror")
        if m is None:
            m = self.__dict__["_full_mirror"] = [bool(v) for v in self.full_label.detach().cpu().tolist()]
            self.__dict__["_count_mirror"] = [float(v) for v in self.update_count.detach().cpu().tolist()]
        return m

    def state_dict(self, *a, **kw):
        from .matcher import check_lsap_pending
        check_lsap_pending()        # a deferred LSAP error of the bank update (invalid cost matrix) must not be saved silently
        return super().state_dict(*a, **kw)

    def sync_host_state(self):
        self.__dict__.pop("_full_mirror", None)
        self.__dict__.pop("_count_mirror", None)

    def _load_from_state_dict(self, *a, **kw):
        self.sync_host_state()
        return super()._load_from_state_dict(*a, **kw)

    def memory_cluster(self, feature, t):
        choice, centers = kmeans(self.feature_bank[t], self.cluster_centers[t].clone(), self.cluster_num, full_label=float(self.full_label[t]))
        self.cluster_centers[t] = centers
        pick = kmeans_predict(feature.reshape(1, -1), centers)[0]
        return pick, centers[pick]

    def _substitute(self, memory_cache, i, pos, t, feature):
        """Overwrite the text-memory rows `pos` of sample i in img_memory_mod with the chosen prototype."""
        pick, center = self.memory_cluster(feature.clone().detach(), t)
        L = len(memory_cache["text_memory"])
        memory_cache["img_memory_mod"][-L:, i, :][pos.to(center.device)] = self.cluster_centers[t, pick]
        return center

    # ---- hipGraph replay for ANY batch: every per-batch index comes from a DistillTables image (fixed addresses) ----------------------------
    _CONST = DeviceCache()

    def _static_ok(self, training=False):
        """training: the captured distillation step, which serves a run from step 0 under either memory policy (toist_bank_fifo, toist_kmeans_init) and
        only needs a single process.  Otherwise (captured evaluation): the steady state, as before."""
        if self._world() > 1:
            raise RuntimeError("ClusterCriterion on StaticTargets (a captured step) is single-process: the memory-bank queue all_gathers rows across ranks, "
                               "and collectives are not captured; run the list-of-dicts path")
        if not training and (self.args.fifo_memory or not all(self._full_host())):
            raise RuntimeError("ClusterCriterion on StaticTargets (a captured evaluation step) needs the steady state of a single process: every task's "
                               "memory bank full, nearest-replacement updates (fifo_memory off); run the list-of-dicts path until then")

    # ---- the fill phase and FIFO banks under capture: the host only plans the random draws ------------------------------------------------------
    def plan_fill(self, tasks_noun, tasks_sth):
        """Host half of one captured step while banks fill.  tasks_noun: task per image of the teacher side, -1 = no boxes; tasks_sth: task per image of
        the student side.  Advances the host mirror of update_count / full_label exactly as toist_bank_fifo will advance the device buffers
        (mdetr.py:85-92: the label looks at the count before the add), then draws np.random.choice(N, K, replace=False) from the global stream in
        the reference's call order (kmeans.py:8-18 as mdetr.py:171-176 and :249-263 reach it): teacher images in batch order, skipping those without
        boxes, whose task is still filling AFTER this step's queue update; then every student image in batch order whose task is filling.
        -> (init_noun, init_sth): int32 [B, K] numpy, the drawn bank rows per sample, -1 rows where the stored centres are the start."""
        tasks_noun, tasks_sth = [int(t) for t in tasks_noun], [int(t) for t in tasks_sth]
        if max(len(tasks_noun), len(tasks_sth)) > self.memory_size:
            raise ValueError(f"a batch of {max(len(tasks_noun), len(tasks_sth))} images does not fit a memory bank of {self.memory_size} rows")
        full = self._full_host()
        count = self.__dict__["_count_mirror"]
        for t in sorted(set(tasks_noun) - {-1}):
            if not full[t]:
                if count[t] > self.memory_size:
                    full[t] = True
                count[t] += tasks_noun.count(t)
        out = []
        for tasks in (tasks_noun, tasks_sth):
            init = np.full((len(tasks), self.cluster_num), -1, dtype=np.int32)
            for i, t in enumerate(tasks):
                if t >= 0 and not full[t]:
                    init[i] = np.random.choice(self.memory_size, self.cluster_num, replace=False)
            out.append(init)
        return out[0], out[1]

    def _start_status(self, device):
        """the sticky i32 status word of toist_kmeans_init on `device` (allocated on first use: before any capture, in the eager pass).  It lives in
        the mailbox its copies travel through: a deep copy of the criterion starts without either."""
        mail = self._start_mail
        if mail.word is None or mail.word.device != device:
            mail.clear()
            mail.word = torch.zeros(1, dtype=torch.int32, device=device)
        return mail.word

    def check_start_status(self, defer=True):
        """Raise when a toist_kmeans_init launch found the device's full_label and the host's plan (plan_fill) in disagreement -- the buffers were written
        without sync_host_state().  defer=True: the design of matcher.check_lsap_status(defer=True) -- the word is copied to pinned memory behind an
        event and the copies of EARLIER calls that have arrived are looked at, so no step waits for the device; defer=False waits."""
        mail = self._start_mail
        st = mail.word
        if st is None or torch.cuda.is_current_stream_capturing():
            return
        mail.post(st)
        for host in mail.drain(wait=not defer):
            if int(host[0]) != 0:
                st.zero_()
                mail.clear()
                raise RuntimeError("ClusterCriterion: the device's full_label and the host's plan of the k-means start disagreed in a captured step (the "
                                   "launch fell back to the stored centres); call sync_host_state() after writing update_count / full_label directly")

    def _replace_nearest_static(self, rows, tb):
        """update_memory_queue (mdetr.py:79-103) with the grouping of the batch by task AND the choice of the branch read from the device.  toist_bank_fifo
        goes first: the groups whose task is still filling (or every group under fifo_memory) are pushed into their banks there, with the update_count /
        full_label bookkeeping, and it leaves in `lsap_rows` the row count of each group for the nearest-replacement branch (mdetr.py:98-103) -- the
        group's size, or 0 for a group it has served and for an unused slot.  Then one LSAP problem per group slot (dead when its row count is 0), pair
        table of fixed capacity B per problem, and a bank write that skips the dead slots and the problems whose status is not OK
        (toist_scatter_rows_f32).  rows [B, d] f32 (detached features)."""
        from . import kernels as k
        from .matcher import check_lsap_status
        B, d = rows.shape
        N, dev = self.memory_size, rows.device
        def make():
            slot = torch.arange(B * B, dtype=torch.int64, device=dev)
            return torch.full((B,), N, dtype=torch.int32, device=dev), torch.arange(B, dtype=torch.int64, device=dev) * B, slot // B, slot % B
        cols, out_off, g_of, s_of = ClusterCriterion._CONST.get(("bank", B, N, str(dev)), make)
        mem = tb.members.to(torch.int64)
        off = tb.group_off.to(torch.int64)
        rs = rows.index_select(0, mem).contiguous()                                  # rows in group order
        trow = tb.task.to(torch.int64).clamp(min=0).index_select(0, mem)
        cost = torch.cdist(rs[:, None, :], self.feature_bank.index_select(0, trow), p=1).reshape(B, N).contiguous()
        n_g = torch.zeros(B, dtype=torch.int32, device=dev)
        k.bank_fifo(self.feature_bank, self.update_count, self.full_label, tb.group_task, tb.group_off, tb.members, rows.contiguous(), self.args.fifo_memory, n_g)
        ri = torch.zeros(B * B, dtype=torch.int64, device=dev)
        ci = torch.zeros(B * B, dtype=torch.int64, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        k.lsap(cost, (off[:-1] * N).contiguous(), n_g, cols, B, B, N, B * N, out_off, ri, ci, status, ld=N)
        valid = (s_of < n_g.to(torch.int64)[g_of]) & (status[g_of] == 0)
        src_row = torch.where(valid, off[g_of] + ri, torch.full_like(ri, -1))
        dst_row = torch.where(valid, tb.group_task.to(torch.int64)[g_of] * N + ci, torch.full_like(ci, -1))
        k.scatter_rows(rs, src_row, self.feature_bank.view(-1, d), dst_row)
        check_lsap_status(status, defer=True)

    def _cluster_static(self, features, tb):
        """memory_cluster for the whole batch.  A DistillTables image that carries `init_rows` (FillTables.attach: the captured distillation step) goes
        through toist_kmeans_init, where the device's full_label decides per sample between the drawn bank rows and the stored centres; one without
        (captured evaluation, which requires full banks) through toist_kmeans."""
        from . import kernels as k
        B, d = features.shape
        pick = torch.zeros(B, dtype=torch.int32, device=features.device)
        chosen = torch.zeros(B, d, dtype=torch.float32, device=features.device)
        feats = features.detach().float().contiguous()
        init_rows = getattr(tb, "init_rows", None)
        if init_rows is None:
            k.kmeans(self.feature_bank, self.cluster_centers, tb.group_task, tb.group_off, tb.members, feats, 1e-4, 10000, pick, chosen)
        else:
            k.kmeans_init(self.feature_bank, self.cluster_centers, tb.group_task, tb.group_off, tb.members, feats, 1e-4, 10000, pick, chosen,
                          self.full_label, init_rows, self._start_status(features.device))
        return pick, chosen

    def _substitute_batch(self, memory_cache, W, sub, cluster, with_loss=False, push=None):
        """The steady-state arithmetic shared by the teacher and the student side, on list targets and on a DistillTables image: features = W @ text
        memory [B, d]; push(features) (the teacher's bank update goes BEFORE the clustering, mdetr.py:105-205); img_memory_mod = a copy of img_memory;
        cluster(features) -> (pick, chosen [B, d]) for the whole batch; the text rows marked in `sub` [L, B] are overwritten by the sample's prototype.
        -> (features, loss_cluster_feature -- 0.0 without with_loss).  cluster() may return None (the list path while a bank fills): nothing is substituted then and the
        second result is None -- the caller goes sample by sample."""
        text = memory_cache["text_memory"].permute(1, 0, 2)
        B, L, _ = text.shape
        features = (W.to(text.dtype).unsqueeze(-1) * text).sum(1)
        if push is not None:
            push(features.detach().float())
        memory_cache["img_memory_mod"] = memory_cache["img_memory"].clone()
        batch = cluster(features)
        if batch is None:
            return features, None
        chosen = batch[1]
        mod = memory_cache["img_memory_mod"]
        mod[-L:] = torch.where(sub.bool()[:, :, None], chosen[None].to(mod.dtype), mod[-L:])
        if not with_loss:
            return features, 0.0
        return features, ((features - chosen.to(features.dtype)) ** 2).mean(1).sum() / max(B, 1)

    def update_memory_static(self, memory_cache_noun, tb):
        """update_memory on a DistillTables image (teacher side)."""
        self._static_ok(training=True)
        if getattr(tb, "init_rows", None) is None and not all(self._full_host()):
            raise RuntimeError("ClusterCriterion.update_memory on StaticTargets while a memory bank fills needs the step's k-means "
                               "starts: FillTables.attach() the DistillTables and load() what plan_fill returns (harness.CapturedDistillStep does)")
        self._substitute_batch(memory_cache_noun, tb.W_span, tb.sub_span, lambda f: self._cluster_static(f, tb), push=lambda rows: self._replace_nearest_static(rows, tb))
        memory_cache_noun["full_label"], memory_cache_noun["update_count"] = self.full_label, self.update_count
        return memory_cache_noun

    def forward_static(self, memory_cache_sth, tb):
        """forward (student side) on a DistillTables image: ('something' -> prototype, loss_cluster_feature)."""
        self._static_ok(training=True)
        _, loss = self._substitute_batch(memory_cache_sth, tb.W_sth, tb.sub_sth, lambda f: self._cluster_static(f, tb), with_loss=True)
        return memory_cache_sth, {"loss_cluster_choice": torch.zeros((), device=loss.device), "loss_cluster_feature": loss}

    @torch.no_grad()
    def infer_choice_static(self, memory_cache_sth, tb):
        """infer_choice (mdetr.py:279-312) on a DistillTables image filled by pack_eval: the word 'something' of every caption is replaced by the
        prototype closest to its own feature, with no host value in any launch (harness.CapturedEvalStep records it into its graphs).  k-means moves
        `cluster_centers` in place, as memory_cluster does."""
        self._static_ok()
        self._substitute_batch(memory_cache_sth, tb.W_sth, tb.sub_sth, lambda f: self._cluster_static(f, tb))
        return memory_cache_sth

    @torch.no_grad()
    def infer_choice_pairs(self, memory_cache, tables, pair_caption=None):
        """infer_choice (mdetr.py:279-312) for the P (image, caption) pairs of a task sweep, in ONE launch on the encoder's own bf16 rows
        (toist_sweep_prototypes): memory_cache is MDETR.sweep_pairs' cache, tables a loaded SweepChoiceTables, pair_caption the sweep's int32 device
        table (default: the one the cache carries).  tables.memory_mod -- allocated here on first use, reused afterwards -- receives a copy of the
        memory and, in the rows of the word 'something' of every live pair, the chosen prototype; the cache gains it as `_native["memory_mod"]`, which
        MDETR.decode reads as it stands, and a lazy fp32 "img_memory_mod" [S, P, d] for whoever reads that key.  The memory itself is not touched:
        the contrastive head and "img_memory" / "text_memory" keep the unmodified rows, as the reference's clone guarantees.  k-means moves
        `cluster_centers` in place.  Preconditions: _static_ok()'s.  No host value enters the launch: a captured sweep records it."""
        from . import kernels as k
        self._static_ok()
        nat = memory_cache.get("_native")
        if nat is None or not hasattr(memory_cache, "set_lazy"):
            raise ValueError("infer_choice_pairs takes the memory cache of MDETR.sweep_pairs (the encoder's bf16 rows under '_native')")
        if pair_caption is None:
            pair_caption = nat.get("pair_caption")
        if pair_caption is None:
            raise ValueError("infer_choice_pairs: the memory cache carries no pair_caption table; pass the sweep's")
        mem = nat["memory"]
        P, S, L, d = nat["B"], nat["S"], nat["L"], mem.shape[-1]
        if tables.L != L or pair_caption.numel() != P:
            raise ValueError(f"infer_choice_pairs: tables of {tables.L} tokens and {pair_caption.numel()} pairs for a memory of {L} tokens and {P} pairs")
        mod = tables.memory_mod
        if mod is None or mod.shape != mem.shape or mod.device != mem.device:
            mod = tables.memory_mod = torch.empty_like(mem)
        mod.copy_(mem)
        k.sweep_prototypes(mem, mod, pair_caption, tables, self.feature_bank, self.cluster_centers, S - L)
        nat["memory_mod"] = mod
        memory_cache.set_lazy("img_memory_mod", lambda: mod.view(P, S, d).permute(1, 0, 2).float())
        return memory_cache

    def update_memory(self, memory_cache_noun, targets_noun, captions_noun):
        """Teacher side (mdetr.py:105-205): push this batch's noun features into the banks, then replace the noun
        tokens of the teacher's text memory by their prototype."""
        tb = getattr(targets_noun, "distill", None)
        if tb is not None:                      # matcher.StaticTargets of a captured step
            return self.update_memory_static(memory_cache_noun, tb)
        L = len(memory_cache_noun["text_memory"])
        dev = memory_cache_noun["text_memory"].device
        tokenized = memory_cache_noun["tokenized"]
        W, sub = _noun_tables(tokenized, targets_noun, L, dev)
        tasks = [None if len(t["boxes"]) == 0 else task_index(t["dataset_name"]) for t in targets_noun]
        tasks_host = [-1 if t is None else t for t in tasks]
        task_col = _cached_table("noun_meta", (_tok_ref(tokenized), *targets_noun), (L, str(dev)), lambda: torch.tensor(tasks_host, dtype=torch.float32).to(dev))
        # queue rows: feature | task; rows of images without boxes: zero feature, task -1
        feats, done = self._substitute_batch(memory_cache_noun, W, sub, lambda f: self.cluster_batch(f, tasks),
                                             push=lambda rows: self.update_memory_queue(torch.cat([rows, task_col[:, None]], dim=1), tasks_host=tasks_host))
        if done is None:        # a bank is filling: sample by sample on the host
            for i, tgt in enumerate(targets_noun):
                if tasks[i] is not None:
                    spans = [s for box in tgt["noun_tokens_positive"] for s in box]
                    self._substitute(memory_cache_noun, i, span_positions(tokenized, i, spans, L), tasks[i], feats[i])
        memory_cache_noun["full_label"], memory_cache_noun["update_count"] = self.full_label, self.update_count
        return memory_cache_noun

    def _something(self, memory_cache, names, captions, with_loss):
        L, B = memory_cache["text_memory"].shape[:2]
        dev = memory_cache["text_memory"].device
        tokenized = memory_cache["tokenized"]

        def make():
            W, sub, positions = something_tables(tokenized, captions, L)
            return torch.from_numpy(W).to(dev), torch.from_numpy(sub).bool().to(dev), [torch.from_numpy(p_) for p_ in positions]
        W, sub, positions = _cached_table("sth_meta", (_tok_ref(tokenized),), (tuple(captions), L, str(dev)), make)
        tasks = [task_index(n) for n in names]
        features, loss_feature = self._substitute_batch(memory_cache, W, sub, lambda f: self.cluster_batch(f, tasks), with_loss)
        if loss_feature is None:        # a bank is filling: sample by sample on the host
            loss_feature = torch.zeros((), device=dev)
            for i in range(B):
                center = self._substitute(memory_cache, i, positions[i], tasks[i], features[i])
                if with_loss:
                    loss_feature = loss_feature + F.mse_loss(features[i], center)
            loss_feature = loss_feature / max(B, 1)
        return memory_cache, loss_feature

    def forward(self, memory_cache_sth, targets_sth, captions_sth):
        """Student side (mdetr.py:230-277): the pronoun 'something' is replaced by the prototype closest to its own
        feature; loss_cluster_feature pulls that feature towards the prototype (loss_cluster_choice stays 0)."""
        tb = getattr(targets_sth, "distill", None)
        if tb is not None:
            return self.forward_static(memory_cache_sth, tb)
        mc, loss = self._something(memory_cache_sth, [t["dataset_name"] for t in targets_sth], captions_sth, True)
        return mc, {"loss_cluster_choice": torch.zeros((), device=loss.device), "loss_cluster_feature": loss}

    @torch.no_grad()
    def infer_choice(self, memory_cache_sth, dataset_name_list, captions):
        """mdetr.py:282-312"""
        return self._something(memory_cache_sth, dataset_name_list, captions, False)[0]
