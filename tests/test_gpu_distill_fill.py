"""The captured distillation step from step 0 (csrc/kmeans.hip: toist_bank_fifo, toist_kmeans_init; distill.FillTables, ClusterCriterion.plan_fill):
the FIFO kernel bit-exact against torch.cat([bank[n:], new]) with its update_count / full_label bookkeeping, k-means from drawn bank rows against
the host loop (toist_amd.distill.kmeans) from the same rows, the real reference's fill sequence (tests/golden/distill_fill.npz) through the kernels,
and harness.CapturedDistillStep -- ONE hipGraph from a fresh memory through the flip of full_label into nearest replacement, and under
fifo_memory -- against the list-of-dicts step (harness.distillation_step), including a resume from a checkpoint taken mid-fill."""
import copy
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "distill_fill.npz"))


def _groups(tasks, slots, dev):
    """(group_task, group_off, members) int32 device tables of DistillTables' layout for a task per sample (-1 = none)"""
    from toist_amd.distill import DistillTables
    task, gt, go, mem = np.zeros(slots, np.int32), np.zeros(slots, np.int32), np.zeros(slots + 1, np.int32), np.zeros(slots, np.int32)
    DistillTables._pack_groups(list(tasks), task, gt, go, mem)
    return tuple(torch.from_numpy(a).to(dev) for a in (gt, go, mem))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _fifo_case(dev, N, D, tasks, T, count0, label0, fifo, seed=0):
    """One toist_bank_fifo launch against the host rule.  Banks of the tasks the batch does not touch hold 0xFF bytes."""
    from toist_amd import kernels as k
    g = torch.Generator().manual_seed(seed)
    B = len(tasks)
    touched = sorted(set(t for t in tasks if t >= 0))
    banks = torch.randn(T, N, D, generator=g)
    poison = torch.full((N, D), -1, dtype=torch.int32).view(torch.float32)
    for t in range(T):
        if t not in touched:
            banks[t] = poison
    rows = torch.randn(B, D, generator=g)
    count, label = torch.tensor(count0, dtype=torch.float32), torch.tensor(label0, dtype=torch.float32)
    want_b, want_c, want_l, want_rows = banks.clone(), count.clone(), label.clone(), [0] * B
    for gi, t in enumerate(touched):
        new = rows[[i for i, tt in enumerate(tasks) if tt == t]]
        n = len(new)
        if label[t] == 0 or fifo:
            want_b[t] = torch.cat([banks[t][n:], new])
            if label[t] == 0:
                if count[t] > N:
                    want_l[t] = 1
                want_c[t] += n
        else:
            want_rows[gi] = n
    d_banks, d_count, d_label, d_rows = banks.to(dev), count.to(dev), label.to(dev), rows.to(dev)
    lsap_rows = torch.full((B,), 77, dtype=torch.int32, device=dev)
    k.bank_fifo(d_banks, d_count, d_label, *_groups(tasks, B, dev), d_rows, fifo, lsap_rows)
    torch.cuda.synchronize()
    assert torch.equal(_bits(d_banks.cpu()), _bits(want_b)), (N, D, tasks)            # bit-exact, the poisoned neighbours included
    assert torch.equal(d_count.cpu(), want_c) and torch.equal(d_label.cpu(), want_l), (d_count.tolist(), want_c.tolist(), d_label.tolist(), want_l.tolist())
    assert lsap_rows.tolist() == want_rows, (lsap_rows.tolist(), want_rows)


@pytest.mark.parametrize("N,D,n", [(4, 16, 4), (8, 16, 1), (8, 16, 3), (24, 16, 2), (32, 256, 2), (1024, 256, 1), (1024, 256, 4), (9, 6, 2)])
def test_fifo_kernel_shift(dev, N, D, n):
    """(n == N: nothing is kept; (24, 16, 2): the golden's shape; 1024 x 256: the 1 MB bank, many chunks; (9, 6, 2): D no multiple of 4, the scalar move)"""
    _fifo_case(dev, N, D, [1] * n, 3, [0.0, 5.0, 0.0], [0.0, 0.0, 0.0], fifo=False, seed=N + n)


def test_fifo_kernel_branches(dev):
    # two groups in one launch (tasks 0 and 2; the second has two members out of batch order with a -1 sample between), two empty slots
    _fifo_case(dev, 8, 16, [2, -1, 0, 2], 4, [3.0, 0.0, 1.0, 0.0], [0.0] * 4, fifo=False)
    # a full task with FIFO off: the bank is untouched, the group is the LSAP's; beside it a filling one
    _fifo_case(dev, 8, 16, [1, 1, 3], 4, [0.0, 100.0, 0.0, 2.0], [0.0, 1.0, 0.0, 0.0], fifo=False)
    # a full task with FIFO on: pushed, counters untouched
    _fifo_case(dev, 8, 16, [1, 1, 3], 4, [0.0, 100.0, 0.0, 2.0], [0.0, 1.0, 0.0, 0.0], fifo=True)
    # the flip: update_count > N seen before the add (9 > 8 flips, 8 > 8 does not), still a FIFO push on that step
    _fifo_case(dev, 8, 16, [1, 2, 1], 4, [0.0, 9.0, 8.0, 0.0], [0.0] * 4, fifo=False)
    _fifo_case(dev, 1024, 256, [5, 0, 5, 5], 6, [0.0, 0.0, 0.0, 0.0, 0.0, 1025.0], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0], fifo=False)
    # every slot empty
    _fifo_case(dev, 8, 16, [-1, -1], 2, [0.0, 0.0], [0.0, 0.0], fifo=False)


# ---- k-means from drawn rows ------------------------------------------------------------------------------------------------------------------
def _lloyd_checked(X, centers, K):
    """distill.kmeans' loop from given centres, and the smallest relative gap between a point's best and second-best distance over all iterations"""
    from toist_amd import distill
    X, centers, gap = X.float(), centers.clone(), float("inf")
    while True:
        d = distill._sq_dist(X, centers)
        two = d.topk(2, dim=1, largest=False).values
        gap = min(gap, float(((two[:, 1] - two[:, 0]) / two[:, 1]).min()))
        choice = torch.argmin(d, dim=1)
        before = centers.clone()
        for c in range(K):
            members = X[choice == c]
            if len(members) != 0:
                centers[c] = members.mean(dim=0)
        if float(torch.sqrt(((centers - before) ** 2).sum(1)).sum()) ** 2 < 1e-4:
            return centers, gap


def _blob_criterion(N, D, seed, dev):
    from toist_amd import distill
    g = torch.Generator().manual_seed(seed)
    cc = distill.ClusterCriterion(feature_dim=D, memory_size=N, cluster_num=3, task_count=14, args=types.SimpleNamespace(fifo_memory=False))
    blobs = torch.randn(14, 3, D, generator=g) * 2
    cc.feature_bank.copy_(blobs[:, torch.randint(0, 3, (N,), generator=g)] + 0.3 * torch.randn(14, N, D, generator=g))
    cc.cluster_centers.copy_(blobs + 0.5 * torch.randn(14, 3, D, generator=g))
    return cc.to(dev), g


def _kmeans_init(cc, feats, tasks, init, dev):
    from toist_amd import kernels as k
    B, D = feats.shape
    pick = torch.zeros(B, dtype=torch.int32, device=dev)
    chosen = torch.zeros(B, D, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    k.kmeans_init(cc.feature_bank, cc.cluster_centers, *_groups(tasks, B, dev), feats, 1e-4, 10000, pick, chosen, cc.full_label,
                  torch.tensor(init, dtype=torch.int32, device=dev), status)
    torch.cuda.synchronize()
    return pick, chosen, int(status)


def _host_reference(cc, feats, tasks, init):
    """the sequential host loop: sample by sample, from its drawn rows (distill.kmeans draws them itself under full_label == 0; here they are given, so
    the start is passed as centres -- the same loop) or from the task's stored centres.  -> (centres [T, K, D], picks); asserts the precondition."""
    from toist_amd import distill
    centers, picks = cc.cluster_centers.clone(), []
    for i, t in enumerate(tasks):
        X = cc.feature_bank[t]
        start = X[torch.tensor(init[i], device=X.device)].clone() if init[i][0] >= 0 else centers[t].clone()
        got, gap = _lloyd_checked(X, start, 3)
        assert gap > 1e-3, (i, t, gap)         # no near-tie in any iteration: the comparison below is well defined
        _, ref = distill.kmeans(X, start.clone(), 3, full_label=1)
        assert torch.equal(got, ref)           # (_lloyd_checked IS the yardstick's loop)
        centers[t] = ref
        picks.append(int(distill.kmeans_predict(feats[i].reshape(1, -1), ref)[0]))
    return centers, picks


@pytest.mark.parametrize("N,D,seed", [(24, 16, 4), (1024, 256, 3)])       # (seeds for which the precondition of _host_reference holds)
def test_kmeans_start_from_drawn_rows(dev, N, D, seed):
    cc, g = _blob_criterion(N, D, seed, dev)
    cc.full_label[9] = 1                       # task 9 full, tasks 4 and 0 filling
    feats = torch.randn(4, D, generator=g).to(dev)
    tasks = [4, 9, 4, 0]                       # two same-task samples chained (each restarts from its own rows); a full and two filling tasks in one launch
    rs = np.random.RandomState(seed)
    init = [rs.choice(N, 3, replace=False).tolist() if t != 9 else [-1, -1, -1] for t in tasks]
    want_c, want_p = _host_reference(cc, feats, tasks, init)
    before = cc.cluster_centers.clone()
    pick, chosen, status = _kmeans_init(cc, feats, tasks, init, dev)
    assert status == 0
    assert pick.tolist() == want_p
    assert torch.allclose(cc.cluster_centers, want_c, rtol=1e-4, atol=1e-5), float((cc.cluster_centers - want_c).abs().max())
    assert torch.equal(cc.cluster_centers[1], before[1]) and not torch.equal(cc.cluster_centers[4], before[4])
    for i, t in enumerate(tasks[1:], 1):       # (sample 0's centres were overwritten by sample 2 of the same task)
        assert torch.allclose(chosen[i], want_c[t][want_p[i]], rtol=1e-4, atol=1e-5)


def test_kmeans_start_mismatch_sets_the_status_bit(dev):
    """full_label says filling but no row was drawn, and full_label says full but rows were drawn: both fall back to the stored centres -- the result of
    toist_kmeans -- and raise bit 0 of the status word; a row outside the bank does the same."""
    cc, g = _blob_criterion(24, 16, 5, dev)
    cc.full_label[9] = 1
    feats = torch.randn(3, 16, generator=g).to(dev)
    tasks = [4, 9, 2]
    want_c, want_p = _host_reference(cc, feats, tasks, [[-1] * 3] * 3)
    pick, chosen, status = _kmeans_init(cc, feats, tasks, [[-1, -1, -1], [3, 1, 2], [0, 24, 1]], dev)
    assert status == 1
    assert pick.tolist() == want_p and torch.allclose(cc.cluster_centers, want_c, rtol=1e-4, atol=1e-5)
    # the host raises at the deferred check, then the word is clear again
    cc._start_status(torch.device(dev)).fill_(1)
    with pytest.raises(RuntimeError, match="sync_host_state"):
        cc.check_start_status(defer=False)
    cc.check_start_status(defer=False)


# ---- the reference's own fill sequence through the kernels ------------------------------------------------------------------------------------------
def _load_groups(tb, tasks):
    host = torch.zeros(tb.nbytes, dtype=torch.uint8)
    v = [x.numpy() for x in tb._views(host)]
    tb._pack_groups([int(t) for t in tasks], v[4], v[5], v[6], v[7])
    tb.load_packed(host)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_reference_fill_sequence_through_the_kernels(dev, tag):
    """update_memory_queue + memory_cluster of the REAL reference, step by step: toist_bank_fifo -> LSAP -> scatter (_replace_nearest_static), then
    toist_kmeans_init for the teacher's and the student's samples (_cluster_static) with plan_fill's draws under the recorded seed."""
    from toist_amd.distill import ClusterCriterion, DistillTables, FillTables
    from toist_amd.matcher import check_lsap_pending
    D, N, K, B, T = 16, 24, 3, 2, 4
    fifo = bool(Z[f"{tag}.fifo_memory"])
    cc = ClusterCriterion(feature_dim=D, memory_size=N, cluster_num=K, task_count=T, args=types.SimpleNamespace(train_batch_size=B, fifo_memory=fifo))
    cc.feature_bank.copy_(torch.from_numpy(Z[f"{tag}.bank0"]))
    cc.cluster_centers.copy_(torch.from_numpy(Z[f"{tag}.centers0"]))
    if fifo:
        cc.full_label.fill_(1)
        cc.update_count.fill_(100)
    cc.to(dev)
    noun, sth = DistillTables(B, 4, dev, pronoun_side=False), DistillTables(B, 4, dev, pronoun_side=True)
    ft = FillTables(B, K, N, dev).attach(noun, sth)
    np.random.seed(int(Z[f"{tag}.seed"]))
    for s in range(len(Z[f"{tag}.rows"])):
        tn, ts = Z[f"{tag}.tasks_noun"][s].tolist(), Z[f"{tag}.tasks_sth"][s].tolist()
        rows, feats = torch.from_numpy(Z[f"{tag}.rows"][s]).to(dev), torch.from_numpy(Z[f"{tag}.feats_sth"][s]).to(dev)
        ft.load(*cc.plan_fill(tn, ts))
        _load_groups(noun, tn)
        _load_groups(sth, ts)
        cc._replace_nearest_static(rows, noun)
        pn, _ = cc._cluster_static(rows, noun)
        torch.cuda.synchronize()
        assert np.array_equal(cc.feature_bank.cpu().numpy(), Z[f"{tag}.bank"][s]), s
        assert np.array_equal(cc.update_count.cpu().numpy(), Z[f"{tag}.update_count"][s]) and np.array_equal(cc.full_label.cpu().numpy(), Z[f"{tag}.full_label"][s]), s
        np.testing.assert_allclose(cc.cluster_centers.cpu().numpy(), Z[f"{tag}.centers_teacher"][s], rtol=1e-4, atol=1e-5, err_msg=str(s))
        ps, _ = cc._cluster_static(feats, sth)
        np.testing.assert_allclose(cc.cluster_centers.cpu().numpy(), Z[f"{tag}.centers"][s], rtol=1e-4, atol=1e-5, err_msg=str(s))
        assert [p for p, t in zip(pn.tolist(), tn) if t >= 0] == [p for p in Z[f"{tag}.pick_noun"][s].tolist() if p >= 0], s
        assert ps.tolist() == Z[f"{tag}.pick_sth"][s].tolist(), s
        assert cc._count_mirror == cc.update_count.tolist() and cc._full_mirror == [bool(v) for v in cc.full_label.tolist()], s
    check_lsap_pending()
    cc.check_start_status(defer=False)


# ---- one graph from step 0 ------------------------------------------------------------------------------------------------------------------------
_SETUP = {}


def _setup(dev, fifo):
    """models, criterion and a cluster criterion with blob-structured banks, as test_captured_distill_step_serves_any_batch builds them (one per policy)"""
    import toist_amd
    from toist_amd import harness
    if fifo not in _SETUP:
        args = harness.default_args(device="cuda", distillation=True, cluster=True, nsthl2_loss=True, softkd_loss=True, cluster_memory_size=32,
                                    num_queries=20, enc_layers=1, dec_layers=2, dropout=0.0, fifo_memory=fifo)
        torch.manual_seed(0)
        model, criterion, cc, weight_dict = toist_amd.build_model(args)
        noun, _, _, _ = toist_amd.build_model(args)
        for m_ in (model, noun):
            m_.to(dev).train()
            m_.transformer.text_encoder.config.hidden_dropout_prob = 0.0
            m_.transformer.text_encoder.config.attention_probs_dropout_prob = 0.0
        g = torch.Generator().manual_seed(11)
        blobs = torch.randn(14, 3, 256, generator=g) * 2
        cc.feature_bank.copy_(blobs[:, torch.randint(0, 3, (32,), generator=g)] + 0.3 * torch.randn(14, 32, 256, generator=g))
        cc.cluster_centers.copy_(blobs + 0.5 * torch.randn(14, 3, 256, generator=g))
        cc.to(dev)
        _SETUP[fifo] = (model, noun, criterion, cc, weight_dict)
    return _SETUP[fifo]


def _memory(cc0, fifo):
    cc = copy.deepcopy(cc0)
    if fifo:
        cc.full_label.fill_(1)
        cc.update_count.fill_(100)
    else:       # task 0 keeps filling; task 2 is past the bank size (flips on its first update, nearest replacement from its second); task 5 sits AT the
        cc.update_count[2] = 40                # bank size (32 > 32 is false: one more FIFO step, flips on its second update, nearest from its third)
        cc.update_count[5] = 32
    cc.sync_host_state()
    return cc


# (max targets per image, 1-based task of each image).  Fill: two images of one task (the flip of task 2); two tasks; no boxes at all on the teacher side
# while the student's tasks are filling; the flip of task 5; a step whose touched tasks are all full; two images of the filling task; full + filling.
PLANS = [(4, (3, 3)), (5, (1, 6)), (0, (1, 6)), (3, (6, 6)), (5, (3, 6)), (2, (1, 1)), (4, (3, 1)), (3, (6, 3))]


def _batch(dev, step_i, mt, tasks):
    from toist_amd import harness
    batch = harness.synthetic_distill_batch(2, 128, 160, tokens=16, seed=140 + step_i, device=dev, max_targets=mt)
    for side_t in batch["targets"]:
        for i, t in enumerate(side_t):
            t["dataset_name"] = f"task_{tasks[i]}_train.json"
    return batch


def _mirror_ok(cc):
    return cc._count_mirror == cc.update_count.tolist() and cc._full_mirror == [bool(v) for v in cc.full_label.tolist()]


@pytest.mark.parametrize("fifo", [False, True])
def test_one_graph_from_step_zero(dev, fifo):
    """harness.CapturedDistillStep against harness.distillation_step on a deep copy of the memory, np.random seeded alike before each path's step: total
    loss, two gradients, banks, centres (the tolerances of test_captured_distill_step_serves_any_batch), update_count / full_label exactly, the host
    mirror against the device, one capture for all steps."""
    from toist_amd import engine, harness, kernels
    from toist_amd.matcher import check_lsap_pending
    from toist_amd.optim import FusedClipAdamWEMA
    model, noun, criterion, cc0, weight_dict = _setup(dev, fifo)
    cc = _memory(cc0, fifo)
    cc_ref = copy.deepcopy(cc)
    cc_ref.sync_host_state()
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
    saved = engine.REUSE_GRAD_BUFFERS
    plans = PLANS[:3] if fifo else PLANS
    try:
        opts = [FusedClipAdamWEMA([{"params": [p for p in x.parameters() if p.requires_grad]}], lr=0.0, weight_decay=0.0, max_norm=0.1) for x in (model, noun)]
        cap = harness.CapturedDistillStep(model, noun, criterion, cc, opts, weight_dict, batch=2, image_hw=(128, 160), tokens=16, max_targets_per_image=6)
        for step_i, (mt, tasks) in enumerate(plans):
            batch = _batch(dev, step_i, mt, tasks)
            np.random.seed(70 + step_i)
            got = float(cap.step(batch))
            if step_i == 0:
                gviews = [model.class_embed.weight.grad, noun.transformer.decoder.layers[0].linear1.weight.grad]
            g_cap = [v.detach().clone() for v in gviews]
            for o in opts:
                o.zero_grad(set_to_none=True)
            np.random.seed(70 + step_i)
            total, _ = harness.distillation_step(model, noun, criterion, cc_ref, weight_dict, batch)
            total.backward()
            torch.cuda.synchronize()
            check_lsap_pending()
            ref = float(total.detach())
            assert abs(got - ref) <= 2e-3 * abs(ref) + 1e-4, (step_i, got, ref)
            for a, b in zip(g_cap, [model.class_embed.weight.grad, noun.transformer.decoder.layers[0].linear1.weight.grad]):
                assert float((a - b).norm()) <= 2e-2 * float(b.norm()) + 1e-6, (step_i, float((a - b).norm()), float(b.norm()))
            assert torch.equal(cc.update_count, cc_ref.update_count) and torch.equal(cc.full_label, cc_ref.full_label), (step_i, cc.update_count.tolist(), cc_ref.update_count.tolist())
            assert _mirror_ok(cc) and _mirror_ok(cc_ref), step_i
            assert torch.allclose(cc.feature_bank, cc_ref.feature_bank, rtol=1e-3, atol=1e-4), (step_i, float((cc.feature_bank - cc_ref.feature_bank).abs().max()))
            assert torch.allclose(cc.cluster_centers, cc_ref.cluster_centers, rtol=1e-3, atol=1e-4), (step_i, float((cc.cluster_centers - cc_ref.cluster_centers).abs().max()))
            cc_ref.feature_bank.copy_(cc.feature_bank)                 # (keep the two memories bit-identical, as that test does)
            cc_ref.cluster_centers.copy_(cc.cluster_centers)
        assert cap.captures == 1 and cap.replays == len(plans) - 1
        cc.check_start_status(defer=False)
        if not fifo:                           # what the sequence was built to cross
            assert cc.full_label.tolist() == [0.0, 0.0, 1.0, 0.0, 0.0, 1.0] + [0.0] * 8 and float(cc.update_count[0]) > 0
    finally:
        engine.REUSE_GRAD_BUFFERS = saved


def test_resume_mid_fill(dev):
    """A checkpoint taken after three steps of the fill phase, loaded into a fresh criterion under a fresh captured step (load_state_dict resynchronises
    the host mirror), continues like the uninterrupted run: same counters exactly, same banks, centres and losses."""
    from toist_amd import engine, harness, kernels
    from toist_amd.distill import ClusterCriterion
    from toist_amd.optim import FusedClipAdamWEMA
    model, noun, criterion, cc0, weight_dict = _setup(dev, False)
    kernels.SEED_DEV = torch.zeros(1, dtype=torch.int64, device=dev)
    saved = engine.REUSE_GRAD_BUFFERS
    plans = PLANS[:5]
    try:
        opts = [FusedClipAdamWEMA([{"params": [p for p in x.parameters() if p.requires_grad]}], lr=0.0, weight_decay=0.0, max_norm=0.1) for x in (model, noun)]

        def captured(cc):
            return harness.CapturedDistillStep(model, noun, criterion, cc, opts, weight_dict, batch=2, image_hw=(128, 160), tokens=16, max_targets_per_image=6)

        def run(cap, steps):
            out = []
            for step_i in steps:
                np.random.seed(70 + step_i)
                out.append(float(cap.step(_batch(dev, step_i, *plans[step_i]))))
            return out
        cc_a = _memory(cc0, False)
        loss_a = run(captured(cc_a), range(5))
        cc_b = _memory(cc0, False)
        loss_b = run(captured(cc_b), range(3))
        state = {k_: v.clone() for k_, v in cc_b.state_dict().items()}
        cc_c = ClusterCriterion(feature_dim=256, memory_size=32, cluster_num=3, task_count=14, args=cc0.args).to(dev)
        cc_c._full_host()                      # (a mirror read before the load must not survive it)
        cc_c.load_state_dict(state)
        loss_b += run(captured(cc_c), range(3, 5))
        torch.cuda.synchronize()
        cc_c.check_start_status(defer=False)
        assert all(abs(a - b) <= 2e-3 * abs(a) + 1e-4 for a, b in zip(loss_a, loss_b)), (loss_a, loss_b)
        assert torch.equal(cc_c.update_count, cc_a.update_count) and torch.equal(cc_c.full_label, cc_a.full_label)
        assert _mirror_ok(cc_c) and _mirror_ok(cc_a)
        assert float(cc_a.full_label.sum()) == 2 and float(cc_a.update_count[0]) > 0          # (both flips lie inside these five steps)
        assert torch.allclose(cc_c.feature_bank, cc_a.feature_bank, rtol=1e-3, atol=1e-4), float((cc_c.feature_bank - cc_a.feature_bank).abs().max())
        assert torch.allclose(cc_c.cluster_centers, cc_a.cluster_centers, rtol=1e-3, atol=1e-4), float((cc_c.cluster_centers - cc_a.cluster_centers).abs().max())
    finally:
        engine.REUSE_GRAD_BUFFERS = saved
