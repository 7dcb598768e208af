"""The fill phase of the memory banks and the FIFO policy, host side, against vectors produced by the REAL reference
(tests/golden/make_golden_distill_fill.py -> distill_fill.npz: ClusterCriterion.update_memory_queue + memory_cluster from a fresh criterion under a
fixed np.random.seed, every np.random.choice result recorded in call order):
  * the yardstick of the GPU tests -- the list path (update_memory_queue, distill.kmeans) -- reproduces the golden step by step;
  * ClusterCriterion.plan_fill spends exactly the reference's draws, in its slots, and its mirror follows update_count / full_label through the flip;
  * distill.FillTables: layout, -1 everywhere in the steady state, the batch-larger-than-a-bank error."""
import os
import types

import numpy as np
import pytest
import torch

Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "distill_fill.npz"))
D, N, K, B, T = 16, 24, 3, 2, 4


def criterion(tag, device="cpu"):
    from toist_amd.distill import ClusterCriterion
    fifo = bool(Z[f"{tag}.fifo_memory"])
    cc = ClusterCriterion(feature_dim=D, memory_size=N, cluster_num=K, task_count=T, args=types.SimpleNamespace(train_batch_size=B, fifo_memory=fifo))
    cc.feature_bank.copy_(torch.from_numpy(Z[f"{tag}.bank0"]))
    cc.cluster_centers.copy_(torch.from_numpy(Z[f"{tag}.centers0"]))
    if fifo:                                   # (sequence B: full banks under fifo_memory)
        cc.full_label.fill_(1)
        cc.update_count.fill_(100)
    return cc.to(device)


def _host_lsap(costs, defer_status=False, with_status=False):
    """linear_sum_assignment for the one- and two-row problems of the golden, by enumeration (the device LSAP kernel needs a GPU)"""
    res = []
    for c in costs:
        c = c.double()
        if c.shape[0] == 1:
            rows, cols = [0], [int(c[0].argmin())]
        else:
            assert c.shape[0] == 2
            tot = c[0][:, None] + c[1][None, :]
            tot.fill_diagonal_(float("inf"))
            a, b = divmod(int(tot.argmin()), c.shape[1])
            (rows, cols) = ([0, 1], [a, b])
        res.append((torch.tensor(rows), torch.tensor(cols)))
    status = torch.zeros(len(costs), dtype=torch.int32)
    return (res, status) if with_status else res


@pytest.mark.parametrize("tag", ["A", "B"])
def test_list_path_reproduces_the_reference_fill(tag, monkeypatch):
    from toist_amd import distill
    monkeypatch.setattr(distill, "linear_sum_assignment_batch", _host_lsap)
    cc = criterion(tag)
    np.random.seed(int(Z[f"{tag}.seed"]))
    flipped = False
    for s in range(len(Z[f"{tag}.rows"])):
        rows, tn = torch.from_numpy(Z[f"{tag}.rows"][s]), Z[f"{tag}.tasks_noun"][s].tolist()
        feats, ts = torch.from_numpy(Z[f"{tag}.feats_sth"][s]), Z[f"{tag}.tasks_sth"][s].tolist()
        before = cc.full_label.clone()
        cc.update_memory_queue(torch.cat([rows, torch.tensor(tn, dtype=torch.float32)[:, None]], dim=1), tasks_host=tn)
        flipped = flipped or not torch.equal(before, cc.full_label)
        assert np.array_equal(cc.feature_bank.numpy(), Z[f"{tag}.bank"][s]), s
        assert np.array_equal(cc.update_count.numpy(), Z[f"{tag}.update_count"][s]) and np.array_equal(cc.full_label.numpy(), Z[f"{tag}.full_label"][s]), s
        pn = [int(cc.memory_cluster(rows[i].clone(), t)[0]) if t >= 0 else -1 for i, t in enumerate(tn)]
        np.testing.assert_allclose(cc.cluster_centers.numpy(), Z[f"{tag}.centers_teacher"][s], rtol=1e-4, atol=1e-5, err_msg=str(s))
        ps = [int(cc.memory_cluster(feats[i].clone(), t)[0]) for i, t in enumerate(ts)]
        np.testing.assert_allclose(cc.cluster_centers.numpy(), Z[f"{tag}.centers"][s], rtol=1e-4, atol=1e-5, err_msg=str(s))
        assert pn == Z[f"{tag}.pick_noun"][s].tolist() and ps == Z[f"{tag}.pick_sth"][s].tolist(), s
    assert flipped == (tag == "A")             # sequence A carries one task through update_count > N


def _expected_slots(tag, s):
    """(teacher, student) [B] bool: the samples for which the reference drew at step s -- full_label AFTER the step's queue update is 0"""
    full = Z[f"{tag}.full_label"][s]
    return [[t >= 0 and full[t] == 0 for t in Z[f"{tag}.{side}"][s].tolist()] for side in ("tasks_noun", "tasks_sth")]


@pytest.mark.parametrize("tag", ["A", "B"])
def test_plan_fill_spends_the_reference_draws(tag):
    cc = criterion(tag)
    draws, at = Z[f"{tag}.draws"], 0
    np.random.seed(int(Z[f"{tag}.seed"]))
    for s in range(len(Z[f"{tag}.rows"])):
        init = cc.plan_fill(Z[f"{tag}.tasks_noun"][s].tolist(), Z[f"{tag}.tasks_sth"][s].tolist())
        for side, slots in zip(init, _expected_slots(tag, s)):
            assert side.dtype == np.int32 and side.shape == (B, K)
            for i, drawn in enumerate(slots):
                if drawn:
                    assert Z[f"{tag}.draw_step"][at] == s and np.array_equal(side[i], draws[at]), (s, i, side[i], draws[at])
                    at += 1
                else:
                    assert np.array_equal(side[i], [-1] * K), (s, i, side[i])
        assert cc._count_mirror == Z[f"{tag}.update_count"][s].tolist() and cc._full_mirror == [bool(v) for v in Z[f"{tag}.full_label"][s]], s
    assert at == len(draws)
    assert (len(draws) > 0) == (tag == "A")
    # the buffers themselves are the device's to advance (toist_bank_fifo): the planner has touched only the mirror
    assert float(cc.update_count.sum()) == (0.0 if tag == "A" else 100.0 * T)


def test_plan_fill_in_the_steady_state_draws_nothing():
    cc = criterion("A")
    cc.full_label.fill_(1)
    cc.sync_host_state()
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    a, b = cc.plan_fill([0, -1], [3, 3])
    assert (a == -1).all() and (b == -1).all()
    assert np.array_equal(np.random.get_state()[1], state)
    with pytest.raises(ValueError, match="does not fit"):
        cc.plan_fill(list(range(4)) * 7, [0] * 28)


def test_fill_tables_layout():
    from toist_amd.distill import DistillTables, FillTables
    ft = FillTables(B, K, N, "cpu")
    assert ft.init.dtype == torch.int32 and tuple(ft.init.shape) == (2, B, K) and bool((ft.init == -1).all())
    noun, sth = DistillTables(B, 8, "cpu", pronoun_side=False), DistillTables(B, 8, "cpu", pronoun_side=True)
    ft.attach(noun, sth)
    a = np.array([[3, 1, 2], [-1, -1, -1]], dtype=np.int32)
    b = np.array([[-1, -1, -1], [7, 23, 0]], dtype=np.int32)
    host = ft.pack(a, b)
    assert host.dtype == torch.int32 and np.array_equal(host.numpy(), np.stack([a, b]))
    addr = ft.init.data_ptr()
    ft.load(a, b)
    assert ft.init.data_ptr() == addr and noun.init_rows.data_ptr() == addr and sth.init_rows.data_ptr() == addr + B * K * 4      # fixed addresses
    assert np.array_equal(noun.init_rows.numpy(), a) and np.array_equal(sth.init_rows.numpy(), b)
    with pytest.raises(ValueError, match="start rows"):
        ft.pack(a[:1], b)
    with pytest.raises(ValueError, match="does not fit"):
        FillTables(N + 1, K, N, "cpu")
