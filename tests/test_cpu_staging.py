"""toist_amd/staging.py on the host: the arena layouts against the offsets the tables had when each wrote its own, the host-only Staging, the hazard
rule and the mailbox's bookkeeping on a recording stand-in for the event type, and the packed images against tests/golden/staging.npz."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (batch, cap, K) -> offsets of the seven segments, total: StaticTargets.arena_views before it moved onto staging.typed_views
STATIC_LAYOUT = {(2, 6, 8): ([0, 96, 288, 480, 496, 512, 528], 544),
                 (1, 1, 256): ([0, 16, 1040, 1072, 1088, 1104, 1120], 1136),
                 (8, 128, 256): ([0, 2048, 133120, 137216, 137264, 137312, 137328], 137344)}
# (B, L) -> offsets of the eight segments, total: DistillTables before the move
DISTILL_LAYOUT = {(1, 1): ([0, 16, 32, 48, 64, 80, 96, 112], 128),
                  (3, 7): ([0, 96, 192, 224, 256, 272, 288, 304], 320),
                  (8, 24): ([0, 768, 1536, 1728, 1920, 1952, 1984, 2032], 2064)}


def _offsets(views, total):
    buf = torch.zeros(total, dtype=torch.uint8)
    return [v.data_ptr() - buf.data_ptr() for v in views(buf)]


@pytest.mark.parametrize("shape", list(STATIC_LAYOUT))
def test_static_targets_layout(shape):
    from toist_amd import staging
    from toist_amd.matcher import StaticTargets
    batch, cap, K = shape
    offs, total = STATIC_LAYOUT[shape]
    assert staging.layout([cap * 16, cap * K * 4, cap * 32, (batch + 1) * 4, (batch + 1) * 4, 4, 16]) == (offs, total)
    views, got = StaticTargets.arena_views(batch, cap, K)
    assert got == total and _offsets(views, total) == offs
    v = views(torch.zeros(total, dtype=torch.uint8))
    assert [(x.dtype, tuple(x.shape)) for x in v] == [(torch.float32, (cap, 4)), (torch.float32, (cap, K)), (torch.int64, (cap, 4)), (torch.int32, (batch + 1,)),
                                                      (torch.int32, (batch + 1,)), (torch.float32, (1,)), (torch.int32, (4,))]


@pytest.mark.parametrize("shape", list(DISTILL_LAYOUT))
def test_distill_tables_layout(shape):
    from toist_amd import staging
    from toist_amd.distill import DistillTables
    B, L = shape
    offs, total = DISTILL_LAYOUT[shape]
    assert staging.layout([B * L * 4, B * L * 4, L * B, L * B, B * 4, B * 4, (B + 1) * 4, B * 4]) == (offs, total)
    tb = DistillTables(B, L, "cpu", pronoun_side=False)
    assert tb.nbytes == total and _offsets(tb._views, total) == offs


class _Events:
    """A recording stand-in for the event type: every call of every instance lands in one log.  `arrived`: what query() answers, per instance number."""

    def __init__(self, log, arrived=lambda n: True):
        self.log, self.made, self.arrived = log, 0, arrived

    def __call__(self):
        outer, n = self, self.made
        self.made += 1

        class Event:
            def record(self):
                outer.log.append(("record", n))

            def synchronize(self):
                outer.log.append(("synchronize", n))

            def query(self):
                return outer.arrived(n)
        return Event()


class _Dst:
    """A device destination that logs the copies into it."""

    def __init__(self, log, name):
        self.log, self.name = log, name

    def copy_(self, src, non_blocking=False):
        assert non_blocking
        self.log.append(("copy", self.name, src.clone()))


def test_host_only_staging_constructs_no_event(monkeypatch):
    from toist_amd import staging

    def no_event():
        raise AssertionError("a host-only Staging constructed an event")
    monkeypatch.setattr(staging, "Event", no_event)
    st = staging.Staging(torch.zeros(32, dtype=torch.uint8), "cpu")
    dst = torch.full((32,), 9, dtype=torch.uint8)
    assert not st.pinned and not st.host.is_pinned()
    st.open()[:] = 1
    st.upload((dst, st.host))
    assert dst.tolist() == [1] * 32
    st.open_np()[:16] = 2
    st.upload_head(dst, 16)
    assert dst.tolist() == [2] * 16 + [1] * 16
    st.fence()


def test_the_hazard_rule(monkeypatch):
    """wait before the first host write, one record per upload, behind its last copy"""
    from toist_amd import staging
    log = []
    monkeypatch.setattr(staging, "Event", _Events(log))
    st = staging.Staging(torch.zeros(8, dtype=torch.int32), "cpu", pin=False)
    st.pinned = True                                                # (the fence of a pinned buffer, on an ordinary one: no GPU runtime here)
    for step in range(3):
        host = st.open()
        log.append(("handed out", step))
        host[:] = step
        st.upload((_Dst(log, "a"), host))
    kinds = [e[:2] for e in log]
    assert kinds == [("handed out", 0), ("copy", "a"), ("record", 0),
                     ("synchronize", 0), ("handed out", 1), ("copy", "a"), ("record", 0),
                     ("synchronize", 0), ("handed out", 2), ("copy", "a"), ("record", 0)]
    assert [int(e[2][0]) for e in log if e[0] == "copy"] == [0, 1, 2]            # each upload carried its own content
    # three slices behind one record
    del log[:]
    host = st.open()
    host[:] = torch.arange(8, dtype=torch.int32)
    st.upload((_Dst(log, "x"), host[:2]), (_Dst(log, "y"), host[2:4]), (_Dst(log, "z"), host[4:]))
    assert [e[:2] for e in log] == [("synchronize", 0), ("copy", "x"), ("copy", "y"), ("copy", "z"), ("record", 0)]
    assert [e[2].tolist() for e in log if e[0] == "copy"] == [[0, 1], [2, 3], [4, 5, 6, 7]]


class _Words:
    """What Mailbox.post reads of a device tensor."""
    is_cuda, shape, dtype = True, (2,), torch.int32


def _mailbox(monkeypatch, log, arrived=lambda n: True, capturing=False):
    from toist_amd import staging
    monkeypatch.setattr(staging, "Event", _Events(log, arrived))
    monkeypatch.setattr(staging, "_capturing", lambda: capturing)
    hosts = []

    def empty(shape, dtype=None, pin_memory=False):                 # pinned memory needs the GPU runtime: an ordinary tensor whose copy_ is logged
        assert pin_memory
        host = types.SimpleNamespace(n=len(hosts), copy_=lambda src, non_blocking=False: log.append(("copy", len(hosts) - 1)))
        hosts.append(host)
        return host
    monkeypatch.setattr(staging, "torch", types.SimpleNamespace(empty=empty))
    return staging.Mailbox(), hosts


def test_mailbox_posts_nothing_under_capture_or_for_host_words(monkeypatch):
    log = []
    mail, hosts = _mailbox(monkeypatch, log, capturing=True)
    mail.post(_Words())
    assert len(mail) == 0 and not log and not hosts
    mail, hosts = _mailbox(monkeypatch, log, capturing=False)
    mail.post(torch.zeros(2, dtype=torch.int32))                    # a host tensor
    assert len(mail) == 0 and not log and not hosts
    mail.post(_Words())
    assert len(mail) == 1 and log == [("copy", 0), ("record", 0)]   # the event is recorded behind the copy


def test_mailbox_drain_leaves_what_has_not_arrived_in_order(monkeypatch):
    log = []
    arrived = {1, 3}
    mail, hosts = _mailbox(monkeypatch, log, arrived=lambda n: n in arrived)
    for _ in range(5):
        mail.post(_Words())
    assert [h.n for h in mail.drain(wait=False)] == [1, 3] and len(mail) == 3
    assert [h.n for h, _ in mail._queue] == [0, 2, 4]
    arrived.add(2)
    assert [h.n for h in mail.drain(wait=False)] == [2] and [h.n for h, _ in mail._queue] == [0, 4]
    # a caller that stops midway (it raised) leaves the rest queued; waiting takes everything, oldest first
    mail.post(_Words())
    for host in mail.drain(wait=True):
        assert host.n == 0
        break
    assert [h.n for h, _ in mail._queue] == [4, 5]
    del log[:]
    assert [h.n for h in mail.drain(wait=True)] == [4, 5] and len(mail) == 0
    assert log == [("synchronize", 4), ("synchronize", 5)]
    mail.post(_Words())
    mail.clear()
    assert len(mail) == 0


def test_deepcopy_of_an_owner_gives_an_empty_mailbox(monkeypatch):
    from toist_amd import staging
    mail, _ = _mailbox(monkeypatch, [])
    mail.post(_Words())
    mail.word = torch.ones(1, dtype=torch.int32)
    owner = types.SimpleNamespace(mail=mail, other=[1, 2])
    twin = copy.deepcopy(owner)
    assert isinstance(twin.mail, staging.Mailbox) and twin.mail is not mail and len(twin.mail) == 0 and twin.mail.word is None
    assert len(mail) == 1 and mail.word is not None and twin.other == [1, 2]


def test_cluster_criterion_deepcopies_without_a_method_of_its_own():
    from toist_amd.distill import ClusterCriterion
    assert "__deepcopy__" not in vars(ClusterCriterion)
    cc = ClusterCriterion(feature_dim=4, memory_size=6, cluster_num=2, task_count=3, args=types.SimpleNamespace(train_batch_size=2, fifo_memory=False))
    cc._start_status(torch.device("cpu")).fill_(1)
    twin = copy.deepcopy(cc)
    assert torch.equal(twin.feature_bank, cc.feature_bank) and twin.feature_bank.data_ptr() != cc.feature_bank.data_ptr()
    assert set(twin.state_dict()) == set(cc.state_dict()) and twin.args.fifo_memory is False
    assert twin._start_mail is not cc._start_mail and twin._start_mail.word is None and len(twin._start_mail) == 0      # the copy starts without the word
    assert int(cc._start_mail.word[0]) == 1
    twin.check_start_status()                                       # no word: nothing to look at


# ---- the packed images ------------------------------------------------------------------------------------------------------------------------------
def _golden():
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden_staging as gen
    finally:
        sys.path.remove(GOLDEN)
    return gen, np.load(os.path.join(GOLDEN, "staging.npz"))


def test_packed_images_equal_the_recorded_ones():
    from toist_amd.distill import DistillTables
    from toist_amd.matcher import LiveStaticTargets, StaticTargets
    gen, Z = _golden()
    inp = {k: torch.from_numpy(Z[k]) for k in ("boxes", "positive_map", "token_masks", "table_boxes")}
    targets, tables = gen.batches(inp)
    B, L = gen.B, gen.L
    st = StaticTargets(B, gen.PER, gen.Q, gen.K, device="cpu")
    host, sizes = st.pack(targets, inp["positive_map"], inp["token_masks"], out=st._stage.open())
    assert sizes == list(gen.SIZES_TARGETS) and np.array_equal(host.numpy(), Z["static"])
    live = LiveStaticTargets(B, gen.PER, gen.Q, gen.K, device="cpu")
    host, _ = live.pack(targets, inp["positive_map"], inp["token_masks"], out=live._stage.open(), live_tokens=gen.LIVE_TOKENS)
    assert host.numel() == Z["static"].size + 16 and np.array_equal(host.numpy(), Z["live"])
    # load() on a host-only instance is pack + the copy: the "device" image holds the same bytes (LiveStaticTargets.load is StaticTargets.load)
    assert "load" not in vars(LiveStaticTargets)
    live.load(targets, inp["positive_map"], inp["token_masks"], live_tokens=gen.LIVE_TOKENS + 1)
    want = Z["live"].copy()
    want[Z["static"].size:Z["static"].size + 4] = np.frombuffer(np.int32(gen.LIVE_TOKENS + 1).tobytes(), dtype=np.uint8)
    assert np.array_equal(live._dev.numpy(), want) and live.live_tokens.tolist() == [gen.LIVE_TOKENS + 1] and live.sizes == list(gen.SIZES_TARGETS)
    tok = gen.tokenized()
    noun, sth = DistillTables(B, L, "cpu", pronoun_side=False), DistillTables(B, L, "cpu", pronoun_side=True)
    assert np.array_equal(noun.pack(tok, tables, [gen.NOUN_CAPTION] * B).numpy(), Z["distill_noun"])
    assert np.array_equal(sth.pack(tok, tables, [gen.STH_CAPTION] * B).numpy(), Z["distill_sth"])
    assert np.array_equal(sth.pack_eval(tok, [gen.STH_CAPTION] * B, list(gen.DATASETS)).numpy(), Z["distill_eval"])
    assert np.array_equal(sth.load_eval(tok, [gen.STH_CAPTION] * B, list(gen.DATASETS))._dev.numpy(), Z["distill_eval"])
    assert np.array_equal(sth.load(tok, tables, [gen.STH_CAPTION] * B)._dev.numpy(), Z["distill_sth"])
    assert Z["distill_noun"].any() and Z["distill_eval"].any() and not np.array_equal(Z["distill_sth"], Z["distill_eval"])
