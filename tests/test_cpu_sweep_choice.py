"""Host side of the prototype choice inside the captured task sweeps: the caption-side tables (distill.SweepChoiceTables.pack), what the captured
sweep steps and the loop refuse before anything touches a device, the new entry point in the C header, and the condition on the seeded inputs of
tests/test_gpu_zz_zzzzz_sweep_choice_kernel.py that makes the fp32 kernel decide as the fp64 reference does (tests/sweep_choice_ref.py)."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import sweep_choice_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _views(tables, host):
    return [v.numpy() for v in tables._views(host)]


# ------------------------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("L", [5, 8, 12])
def test_pack_equals_something_tables_row_by_row(L):
    from toist_amd.distill import SweepChoiceTables, something_tables, task_index
    tok = ref.Tokens(L)
    tables = SweepChoiceTables(3, L, "cpu")
    host = tables.pack(tok, ref.CAPTIONS, ref.DATASET_NAMES, ref.LIVE)
    assert host.dtype == torch.uint8 and host.numel() == tables.nbytes
    W_sth, sub_sth, cap_task, group_task, live = _views(tables, host)
    W, sub, positions = something_tables(tok, ref.CAPTIONS, L)
    assert [len(p) for p in positions] == [1, 2, 3]                                    # the spans the kernel test needs
    for t in range(3):
        assert np.array_equal(W_sth[t], W[t]) and np.array_equal(sub_sth[t], sub[:, t]), t
        assert sub_sth[t].nonzero()[0].tolist() == positions[t].tolist() == ref.spans(L)[t]
    assert cap_task.tolist() == [task_index(n) for n in ref.DATASET_NAMES] == [2, 4, 2]
    assert live.tolist() == [ref.LIVE]
    assert group_task.tolist() == [2, 4, -1]                                           # two captions on task 2 share one slot


def test_group_task_first_appearance_and_unused_slots():
    """The slots do not depend on the pairs: a caption whose task no pair uses still owns its slot (the workgroup finds nothing to serve)."""
    from toist_amd.distill import SweepChoiceTables
    tok = ref.Tokens(8)
    tables = SweepChoiceTables(3, 8, "cpu")
    names = ["task_9_val.json", "task_2_val.json", "task_9_val.json"]
    for live in (0, 1, 7):
        *_, cap_task, group_task, live_w = _views(tables, tables.pack(tok, ref.CAPTIONS, names, live))
        assert cap_task.tolist() == [8, 1, 8] and group_task.tolist() == [8, 1, -1] and live_w.tolist() == [live]
    *_, group_task, _ = _views(tables, tables.pack(tok, ref.CAPTIONS, ["task_1_x", "task_2_x", "task_3_x"], 3))
    assert group_task.tolist() == [0, 1, 2]
    *_, group_task, _ = _views(tables, tables.pack(tok, ref.CAPTIONS, ["task_4_x"] * 3, 3))
    assert group_task.tolist() == [3, -1, -1]


def test_pack_refuses_and_load_uploads_only_what_changed():
    from toist_amd.distill import SweepChoiceTables
    tok = ref.Tokens(8)
    tables = SweepChoiceTables(3, 8, "cpu")
    assert tables.group_task.tolist() == [-1, -1, -1]                                  # before the first load every slot is unused
    with pytest.raises(ValueError, match="3 captions"):
        tables.pack(tok, ref.CAPTIONS[:2], ref.DATASET_NAMES[:2], 1)
    with pytest.raises(ValueError, match="live"):
        tables.pack(tok, ref.CAPTIONS, ref.DATASET_NAMES, -1)
    with pytest.raises(ValueError, match="something"):
        tables.pack(tok, ["no pronoun here"] + ref.CAPTIONS[1:], ref.DATASET_NAMES, 1)
    assert tables.load(tok, ref.CAPTIONS, ref.DATASET_NAMES, 5) is True
    assert tables.load(tok, ref.CAPTIONS, ref.DATASET_NAMES, 5) is False                # the same image: nothing travels
    assert tables.live.tolist() == [5] and tables.group_task.tolist() == [2, 4, -1]
    assert tables.load(tok, ref.CAPTIONS, ref.DATASET_NAMES, 6) is True and tables.live.tolist() == [6]
    tables.invalidate()
    assert tables.load(tok, ref.CAPTIONS, ref.DATASET_NAMES, 6) is True


# ------------------------------------------------------------------------------------------------------------------ the refusals
@pytest.fixture(scope="module")
def models():
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    tiny = dict(device="cpu", enc_layers=1, dec_layers=1, num_queries=4)
    det, _, cc, _ = toist_amd.build_model(harness.default_args(distillation=True, cluster=True, cluster_memory_size=8, **tiny))
    seg = toist_amd.build_model(harness.default_args(masks=True, mask_model="smallconv", **tiny))[0].eval()
    return det.eval(), seg, cc


def test_the_steps_take_a_cluster_criterion_and_nothing_else(models):
    from toist_amd import harness
    det, seg, cc = models
    for bad in (object(), torch.nn.Module(), "criterion"):
        with pytest.raises(ValueError, match="cluster criterion"):
            harness.CapturedSweepStep(det, bad, batch=1, captions=2, device="cpu")
        with pytest.raises(ValueError, match="cluster criterion"):
            harness.CapturedMaskSweepStep(seg, bad, batch=1, captions=2, max_orig_hw=(64, 64), device="cpu")
    assert harness.CapturedSweepStep(det, cc, batch=1, captions=2, device="cpu").cluster_criterion is cc
    assert harness.CapturedMaskSweepStep(seg, cc, batch=1, captions=2, max_orig_hw=(64, 64), device="cpu").cluster_criterion is cc
    assert harness.CapturedSweepStep(det, batch=1, captions=2, device="cpu").cluster_criterion is None


def test_a_step_with_a_criterion_needs_names_and_captions_before_anything_is_launched(models):
    from toist_amd import harness
    det, seg, cc = models
    samples, tok, _, _ = harness.synthetic_batch(1, 64, 64, tokens=8, seed=1, max_targets=0)
    _, tok2, _, _ = harness.synthetic_batch(2, 32, 32, tokens=8, seed=2, max_targets=0)
    tok2 = harness.SyntheticCaptions(dict(tok2))
    names, captions = ["task_1_train.json", "task_2_train.json"], ["use something now", "sit on something"]
    step = harness.CapturedSweepStep(det, cc, batch=1, captions=2, device="cpu")
    mstep = harness.CapturedMaskSweepStep(seg, cc, batch=1, captions=2, max_orig_hw=(64, 64), device="cpu")
    calls = [lambda **kw: step.step(samples, tok2, [(64, 64)], **kw), lambda **kw: step.step_rows(samples, tok2, [(64, 64)], **kw),
             lambda **kw: mstep.step(samples, tok2, [(64, 64)], [(64, 64)], **kw), lambda **kw: mstep.step_rows(samples, tok2, [(64, 64)], [(64, 64)], **kw)]
    for call in calls:
        for kw in ({}, {"dataset_names": names}, {"captions": captions}):
            with pytest.raises(ValueError, match="dataset_names and captions"):
                call(**kw)
        with pytest.raises(ValueError, match="for 2 captions"):
            call(dataset_names=names[:1], captions=captions)
        with pytest.raises(ValueError, match="outside the cluster criterion"):
            call(dataset_names=["task_1_train.json", "task_99_train.json"], captions=captions)
        with pytest.raises(RuntimeError, match="memory bank full"):                      # _static_ok's precondition: the banks are still filling
            call(dataset_names=names, captions=captions)
    from toist_amd.transformer import TokenizedText
    with pytest.raises(ValueError, match="char_to_token"):
        step.step(samples, TokenizedText(dict(tok2)), [(64, 64)], dataset_names=names, captions=captions)
    assert step.captures == step.replays == mstep.captures == 0 and not step._buckets and not mstep._buckets


def test_the_loop_takes_the_steps_own_criterion_only(models):
    from toist_amd import harness
    from toist_amd.postprocessors import PostProcess
    det, _, cc = models
    step = harness.CapturedSweepStep(det, cc, batch=1, captions=2, device="cpu")
    plain = harness.CapturedSweepStep(det, batch=1, captions=2, device="cpu")
    tasks = [("a", "use something now", "task_1_train.json"), ("b", "sit on something", "task_2_train.json")]
    for captured, crit in ((step, copy.deepcopy(cc)), (plain, cc), (step, torch.nn.Module())):
        with pytest.raises(ValueError, match="cluster criterion"):
            harness.evaluate_sweep(det, PostProcess(), [], tasks, "cpu", cluster_criterion=crit, captured=captured)
    with pytest.raises(ValueError, match="dataset name"):                                # three-element tasks, as in the eager loop
        harness.evaluate_sweep(det, PostProcess(), [], [t[:2] for t in tasks], "cpu", cluster_criterion=cc, captured=step)
    assert harness.evaluate_sweep(det, PostProcess(), [], tasks, "cpu", cluster_criterion=cc, captured=step) == {}


def test_the_entry_point_is_declared_and_bound():
    from toist_amd import _lib
    with open(os.path.join(ROOT, "include", "toist_hip.h")) as f:
        header = f.read()
    assert header.count("TOIST_API int toist_sweep_prototypes(") == 1 and "mdetr.py:282-312" in header
    args = _lib.parse_signatures(header, {})["toist_sweep_prototypes"]
    assert len(args) == 27 and args[12:20] == [ctypes.c_int] * 8 and args[20:22] == [ctypes.c_float, ctypes.c_int]      # P .. K, tol, max_iter
    assert "toist_sweep_prototypes" in _lib.exported_symbols()


# ------------------------------------------------------------------------------------------------------------------ the condition on the GPU test's inputs
@pytest.mark.parametrize("L", [5, 8])
def test_the_seeded_inputs_keep_every_margin_above_the_fp32_bound(L):
    """On the reference alone: every live pair's margin (second-best minus best squared distance to its task's centres) clears the bound derived for
    the fp32 feature and distance sums, and so does every bank row in every Lloyd iteration -- the kernel's picks and assignments are then the fp64
    reference's whatever order its sums run in."""
    from toist_amd.distill import SweepChoiceTables
    t = ref.inputs(L)
    tables = SweepChoiceTables(3, L, "cpu")
    W_sth, sub_sth, *_ = tables._views(tables.pack(ref.Tokens(L), ref.CAPTIONS, ref.DATASET_NAMES, ref.LIVE))
    r = ref.reference(t, W_sth, sub_sth)
    assert len(r["margins"]) == ref.LIVE and r["picks"][ref.LIVE:] == [None] * (ref.P - ref.LIVE)
    for p, (margin, bound) in enumerate(r["margins"]):
        print(f"L={L} pair {p}: margin {margin:.4g} bound {bound:.4g} pick {r['picks'][p]}")
        assert margin > bound > 0, (p, margin, bound)
    print(f"L={L}: bank slack {r['bank_slack']:.4g}")
    assert r["bank_slack"] > 0
    assert len({r["picks"][p] for p in range(ref.LIVE)}) > 1                             # the picks differ from pair to pair
    assert r["rows"][:ref.LIVE].sum(1).tolist() == [len(ref.spans(L)[c]) for c in ref.PAIR_CAPTION[:ref.LIVE]] and not r["rows"][ref.LIVE:].any()
    moved = (r["centers"] - t["centers"].double()).abs().amax((1, 2))
    assert (moved > 0).nonzero().flatten().tolist() == [2, 4]                            # only the two tasks of the captions moved
    fb = r["feature_bound"][:ref.LIVE]
    assert bool((fb > 0).all()) and float(fb.max()) < 1e-5
