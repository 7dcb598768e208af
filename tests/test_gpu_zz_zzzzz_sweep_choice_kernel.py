"""toist_sweep_prototypes on the device at the smallest shapes at which it can go wrong (D = 256, K = 3, N = 32, HW = 4, L = 5 and 8, three captions
two of which share a task, 'something' spanning 1, 2 and 3 tokens, capacity 7 with 5 live pairs, a task's members not contiguous): the features
against the eager expression, the k-means against kernels.kmeans on host-built groups (bit for bit) and against the fp64 reference of
tests/sweep_choice_ref.py, memory_mod element by element, and a table corrupted on the device.
(The file sorts behind every other GPU test file on purpose: DESIGN 8 item 6.  No training step is built here.)"""
import functools

import pytest
import torch

import sweep_choice_ref as ref
from rounding_bounds import F64

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = len(ref.CAPTIONS)
POISON = -7


def _tables(dev, L, live=ref.LIVE):
    from toist_amd.distill import SweepChoiceTables
    tables = SweepChoiceTables(T, L, dev)
    assert tables.load(ref.Tokens(L), ref.CAPTIONS, ref.DATASET_NAMES, live)
    return tables


def _launch(dev, t, tables, pair_caption):
    """One launch on fresh copies of the inputs -> dict of everything it wrote (and of what it must not have written)."""
    from toist_amd import kernels
    memory = t["memory"].to(dev)
    out = {"memory": memory, "memory_mod": memory.clone(), "banks": t["banks"].to(dev), "centers": t["centers"].to(dev).clone(),
           "pick": torch.full((ref.P,), POISON, dtype=torch.int32, device=dev), "iters": torch.full((ref.P,), POISON, dtype=torch.int32, device=dev),
           "features": torch.full((ref.P, ref.D), float("nan"), device=dev)}
    kernels.sweep_prototypes(memory, out["memory_mod"], pair_caption, tables, out["banks"], out["centers"], ref.HW, pick=out["pick"],
                             features=out["features"], iters=out["iters"])
    torch.cuda.synchronize()
    return out


def _by_kmeans(dev, t, features, pairs):
    """kernels.kmeans on host-built groups over `pairs` (ascending) with the given features, from the same stored centres
    -> (pick, chosen centre, iters, centres)."""
    from toist_amd import kernels
    from toist_amd.distill import task_groups
    tasks = [-1] * ref.P
    for p in pairs:
        tasks[p] = t["tasks"][ref.PAIR_CAPTION[p]]
    group_task, group_off, members = (torch.tensor(v, dtype=torch.int32, device=dev) for v in task_groups(tasks))
    centers = t["centers"].to(dev).clone()
    pick = torch.full((ref.P,), POISON, dtype=torch.int32, device=dev)
    iters = torch.full((ref.P,), POISON, dtype=torch.int32, device=dev)
    chosen = torch.zeros(ref.P, ref.D, device=dev)
    kernels.kmeans(t["banks"].to(dev), centers, group_task, group_off, members, features.contiguous(), 1e-4, 10000, pick, chosen, iters=iters)
    torch.cuda.synchronize()
    return pick, chosen, iters, centers


def _expected_mod(t, tables, chosen, pairs, dev):
    """memory with bf16(chosen centre) in the marked caption rows of `pairs`, nothing else touched"""
    want = t["memory"].to(dev).clone()
    sub = tables.sub_sth.bool()
    for p in pairs:
        rows = sub[ref.PAIR_CAPTION[p]].nonzero().flatten() + ref.HW
        want[p, rows] = chosen[p].to(BF16)
    return want


def _bits(a):
    return a.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(dev, L):
    """inputs, the fp64 reference (computed once per L) and one launch of the kernel"""
    t = ref.inputs(L)
    tables = _tables(dev, L)
    r = ref.reference(t, tables.W_sth.cpu(), tables.sub_sth.cpu())
    got = _launch(dev, t, tables, t["pair_caption"].to(dev))
    from toist_amd import kernels
    assert kernels.sweep_check(raise_on_failure=False) == 0
    return t, tables, r, got


@pytest.mark.parametrize("L", [5, 8])
def test_features(dev, L):
    """Spans of one and two tokens: bit-equal to the eager expression (a two-term sum has no order; the zero products add nothing).  The three-token
    span: within the bound derived for an fp32 sum of three rounded products in any order."""
    t, tables, r, got = _case(dev, L)
    text = got["memory"][:, ref.HW:].float()
    W = tables.W_sth[t["pair_caption"].to(dev).long()]
    eager = (W.unsqueeze(-1) * text).sum(1)
    for p in range(ref.LIVE):
        n = len(t["spans"][ref.PAIR_CAPTION[p]])
        err = (got["features"][p].cpu().to(F64) - r["features"][p]).abs()
        ratio = float((err / r["feature_bound"][p]).max())
        print(f"L={L} pair {p}: span {n}, max |err| {float(err.max()):.3g}, err/bound {ratio:.3g}, equal to eager {torch.equal(got['features'][p], eager[p])}")
        if n <= 2:
            assert torch.equal(got["features"][p], eager[p]), p
        assert ratio <= 1.0, (p, ratio)
    assert bool(torch.isnan(got["features"][ref.LIVE:]).all())                                    # padding pairs: never looked at


@pytest.mark.parametrize("L", [5, 8])
def test_kmeans_equals_the_grouped_launch_bit_for_bit_and_the_fp64_picks(dev, L):
    t, tables, r, got = _case(dev, L)
    live = list(range(ref.LIVE))
    pick, chosen, iters, centers = _by_kmeans(dev, t, got["features"].nan_to_num(0.0), live)
    print(f"L={L}: picks {got['pick'].tolist()} iterations {got['iters'].tolist()} (grouped launch: {pick.tolist()} {iters.tolist()})")
    assert torch.equal(got["pick"], pick) and torch.equal(got["iters"], iters)                     # padding pairs: both untouched
    assert got["pick"][ref.LIVE:].tolist() == [POISON] * (ref.P - ref.LIVE)
    assert torch.equal(got["centers"], centers)
    assert got["pick"][:ref.LIVE].tolist() == r["picks"][:ref.LIVE]                                # ... and the fp64 reference's picks
    # a task's later pair starts from the centres its earlier pair left: it needs fewer iterations than the first one
    first = {}
    for p in live:
        first.setdefault(t["tasks"][ref.PAIR_CAPTION[p]], p)
    assert all(int(got["iters"][p]) >= 2 for p in first.values()) and all(int(got["iters"][p]) == 1 for p in live if p not in first.values())
    moved = (got["centers"] != t["centers"].to(dev)).flatten(1).any(1)
    assert moved.nonzero().flatten().tolist() == sorted(set(t["tasks"]))                           # no other task's centres were written
    assert float((got["centers"].cpu().to(F64) - r["centers"]).abs().max()) < 1e-4
    # the chosen centres, as the substituted rows hold them
    want = _expected_mod(t, tables, chosen, live, dev)
    assert torch.equal(_bits(got["memory_mod"]), _bits(want))


@pytest.mark.parametrize("L", [5, 8])
def test_memory_mod_holds_the_prototypes_in_the_marked_rows_and_memory_elsewhere(dev, L):
    t, tables, r, got = _case(dev, L)
    assert torch.equal(_bits(got["memory"]), _bits(t["memory"].to(dev)))                           # memory is never written
    assert torch.equal(got["banks"], t["banks"].to(dev))
    changed = (_bits(got["memory_mod"]) != _bits(got["memory"])).any(-1).cpu()                     # [P, S]
    assert not changed[:, :ref.HW].any() and not changed[ref.LIVE:].any()                          # image rows; the padding pairs' rows
    assert torch.equal(changed[:, ref.HW:], r["rows"])                                             # exactly the marked rows of live pairs
    centres = got["centers"][torch.tensor([t["tasks"][c] for c in ref.PAIR_CAPTION], device=dev)]  # each pair's task's final centres [P, K, D]
    for p in range(ref.LIVE):
        rows = r["rows"][p].nonzero().flatten() + ref.HW
        c = centres[p, r["picks"][p]]
        # a task's LAST pair sees the final centres; an earlier one the centres of its own moment -- equal here once the first pair has converged
        assert torch.equal(_bits(got["memory_mod"][p, rows]), _bits(c.to(BF16).expand(len(rows), -1))), p
        assert float((got["memory_mod"][p, rows[0]].float().cpu().to(F64) - r["chosen"][p]).abs().max()) <= float(r["chosen"][p].abs().max()) * 2.0 ** -8


def test_a_corrupted_table_entry_is_never_an_index(dev):
    """pair_caption[1] rewritten to T on the device: the pair is skipped (no substitution, no pick), the status word holds 2, kernels.sweep_check reads
    and clears it, and every other pair is what the grouped launch gives without pair 1."""
    from toist_amd import kernels
    L = 5
    t, tables, _, _ = _case(dev, L)
    assert kernels.sweep_check(raise_on_failure=False) == 0
    bad = t["pair_caption"].to(dev).clone()
    bad[1] = T
    got = _launch(dev, t, tables, bad)
    assert int(kernels.sweep_status(dev).item()) == 2
    with pytest.raises(ValueError, match="pair 1"):
        kernels.sweep_check()
    assert kernels.sweep_check(raise_on_failure=False) == 0
    others = [0, 2, 3, 4]
    pick, chosen, iters, centers = _by_kmeans(dev, t, got["features"].nan_to_num(0.0), others)
    assert torch.equal(got["pick"], pick) and torch.equal(got["iters"], iters) and int(got["pick"][1]) == POISON
    assert torch.equal(got["centers"], centers)
    assert torch.equal(_bits(got["memory_mod"]), _bits(_expected_mod(t, tables, chosen, others, dev)))
    assert torch.equal(_bits(got["memory_mod"][1]), _bits(got["memory"][1]))
    neg = t["pair_caption"].to(dev).clone()
    neg[4] = -1
    _launch(dev, t, tables, neg)
    assert kernels.sweep_check(raise_on_failure=False) == 5


def test_live_is_read_from_the_device_and_clamped(dev):
    """live = 0: nothing is served; live beyond the capacity: the capacity (the table is never read past its end)."""
    L = 5
    t, _, _, full = _case(dev, L)
    got = _launch(dev, t, _tables(dev, L, live=0), t["pair_caption"].to(dev))
    assert torch.equal(_bits(got["memory_mod"]), _bits(got["memory"])) and torch.equal(got["centers"], t["centers"].to(dev))
    assert got["pick"].tolist() == [POISON] * ref.P
    got = _launch(dev, t, _tables(dev, L, live=ref.P + 9), t["pair_caption"].to(dev))
    assert POISON not in got["pick"].tolist() and torch.equal(got["pick"][:ref.LIVE], full["pick"][:ref.LIVE])


def test_the_launcher_refuses_before_any_launch(dev):
    from toist_amd import kernels
    L = 5
    t, tables, _, _ = _case(dev, L)
    memory, pc = t["memory"].to(dev), t["pair_caption"].to(dev)
    banks, centers = t["banks"].to(dev), t["centers"].to(dev).clone()
    ok = lambda **kw: kernels.sweep_prototypes(**{**dict(memory=memory, memory_mod=memory.clone(), pair_caption=pc, tables=tables, banks=banks,
                                                         centers=centers, HW=ref.HW), **kw})
    with pytest.raises(ValueError, match="copy of memory"):
        ok(memory_mod=memory)
    with pytest.raises(ValueError, match="K <= 8"):
        ok(centers=torch.zeros(ref.N_TASKS, 9, ref.D, device=dev))
    with pytest.raises(ValueError, match="D <= 256"):
        wide = torch.zeros(ref.P, ref.HW + L, 264, dtype=BF16, device=dev)
        ok(memory=wide, memory_mod=wide.clone(), banks=torch.zeros(ref.N_TASKS, ref.N, 264, device=dev), centers=torch.zeros(ref.N_TASKS, 3, 264, device=dev))
    with pytest.raises(ValueError, match="N <= 32768"):
        ok(banks=torch.zeros(1, 32769, ref.D, device=dev).expand(ref.N_TASKS, -1, -1))
    with pytest.raises(ValueError, match="memory and memory_mod"):
        ok(HW=ref.HW + 1)
    with pytest.raises(ValueError, match="must agree"):
        ok(centers=centers[:3])
    assert torch.equal(centers, t["centers"].to(dev)) and kernels.sweep_check(raise_on_failure=False) == 0
