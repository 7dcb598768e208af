"""Host side of the task sweep (toist_amd/sweep.py): the pair tables, the per-pair view of the tokenized captions, the keying of the results, the
refusal to run without the device, and the binding of toist_sweep_assemble.  CPU only."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_tables_full_product_is_image_major():
    from toist_amd.sweep import pair_tables
    pi, pc, live = pair_tables(3, 4)
    assert live == 12 and pi.dtype == torch.int32 and pc.dtype == torch.int32
    assert pi.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2] and pc.tolist() == [0, 1, 2, 3] * 3
    for i in range(3):
        for t in range(4):
            assert (int(pi[i * 4 + t]), int(pc[i * 4 + t])) == (i, t)


def test_pair_tables_explicit_pairs_keep_order_repeats_and_gaps():
    from toist_amd.sweep import pair_tables
    pairs = [(2, 1), (0, 0), (2, 1), (0, 4), (2, 3)]              # a repeated pair; image 1 is not used
    pi, pc, live = pair_tables(3, 5, pairs)
    assert live == 5 and pi.tolist() == [2, 0, 2, 0, 2] and pc.tolist() == [1, 0, 1, 4, 3]


def test_pair_tables_pad_to_capacity_with_pair_zero():
    from toist_amd.sweep import pair_tables
    pi, pc, live = pair_tables(2, 3, [(1, 2), (0, 1), (1, 0)], capacity=8)
    assert live == 3 and pi.numel() == 8 and pc.numel() == 8
    assert pi.tolist() == [1, 0, 1, 0, 0, 0, 0, 0] and pc.tolist() == [2, 1, 0, 0, 0, 0, 0, 0]
    pi, pc, live = pair_tables(2, 3, capacity=6)                    # exactly full
    assert live == 6 and pi.numel() == 6


@pytest.mark.parametrize("call", [
    lambda f: f(0, 3), lambda f: f(3, 0), lambda f: f(2, 2, []), lambda f: f(2, 2, [(2, 0)]), lambda f: f(2, 2, [(0, 2)]), lambda f: f(2, 2, [(-1, 0)]),
    lambda f: f(2, 2, [(0, -1)]), lambda f: f(2, 3, capacity=5), lambda f: f(2, 3, [(0, 0), (1, 1)], capacity=1), lambda f: f(2, 2, [(0, 1, 1)]),
    lambda f: f(2, 2, [(0.5, 1)])])
def test_pair_tables_value_errors(call):
    from toist_amd.sweep import pair_tables
    with pytest.raises(ValueError):
        call(pair_tables)


def test_sweep_tokenized_rows_and_char_to_token_follow_the_pair_table():
    """A REAL fast tokenizer (tests/golden/tiny_roberta_tokenizer.json): row p of the per-pair view is caption pair_caption[p], and char_to_token(p, c)
    is that caption's answer -- None on a space included."""
    import tiny_tokenizer
    from toist_amd.sweep import SweepTokenized
    captions = ["use something to cut the paper up", "sit comfortably on something", "dig a hole with something"]
    enc = tiny_tokenizer.build()(captions, padding="longest", return_tensors="pt")
    rows = [2, 0, 2, 1]
    view = SweepTokenized(enc, torch.tensor(rows, dtype=torch.int32))
    assert view["input_ids"].shape == (4, enc["input_ids"].shape[1]) and view.input_ids is view["input_ids"]
    for p, t in enumerate(rows):
        assert torch.equal(view["input_ids"][p], enc["input_ids"][t]) and torch.equal(view["attention_mask"][p], enc["attention_mask"][t])
        for c in range(len(captions[t])):
            assert view.char_to_token(p, c) == enc.char_to_token(t, c), (p, c)
    beg = [c.find("something") for c in captions]
    assert len({view.char_to_token(p, beg[t]) for p, t in enumerate(rows)}) > 1            # the captions place the word differently: forwarding matters
    assert view.char_to_token(1, 3) is None and enc.char_to_token(0, 3) is None             # the space behind "use"
    assert view.char_to_token(5) == enc.char_to_token(2, 5)                                 # one argument: row 0, as a BatchEncoding reads it
    moved = view.to("cpu")
    assert isinstance(moved, SweepTokenized) and moved.char_to_token(3, beg[1]) == enc.char_to_token(1, beg[1])
    with pytest.raises(ValueError):
        SweepTokenized(enc, [0, 3])


def test_sweep_tokenized_feeds_the_something_lookup_of_the_prototype_choice():
    """distill.something_tables -- what ClusterCriterion.infer_choice locates 'something' with -- on the per-pair view equals the same lookup on a
    batch that repeats the captions pair by pair."""
    import numpy as np
    import tiny_tokenizer
    from toist_amd.distill import something_tables
    from toist_amd.sweep import SweepTokenized
    captions = ["use something to cut the paper up", "sit comfortably on something", "dig a hole with something"]
    tok = tiny_tokenizer.build()
    rows = [1, 1, 0, 2, 0]
    view = SweepTokenized(tok(captions, padding="longest", return_tensors="pt"), rows)
    repeated = [captions[t] for t in rows]
    ref = tok(repeated, padding="longest", return_tensors="pt")
    L = ref["input_ids"].shape[1]
    assert view["input_ids"].shape[1] == L
    W, sub, pos = something_tables(view, repeated, L)
    W_ref, sub_ref, pos_ref = something_tables(ref, repeated, L)
    assert np.array_equal(W, W_ref) and np.array_equal(sub, sub_ref) and all(np.array_equal(a, b) for a, b in zip(pos, pos_ref))


def test_keyed_results_drop_padding_and_key_by_image_and_task():
    from toist_amd.sweep import keyed_results, pair_tables
    pi, pc, live = pair_tables(3, 2, [(2, 1), (0, 0), (2, 0)], capacity=5)
    results = [{"row": p} for p in range(5)]
    out = keyed_results(results, [101, torch.tensor(102), 103], ["cut", "sit"], pi, pc, live)
    assert out == {(103, "sit"): {"row": 0}, (101, "cut"): {"row": 1}, (103, "cut"): {"row": 2}}
    assert all(isinstance(key[0], int) for key in out)
    full = keyed_results(results[:4], [7, 8], ["a", "b"], *pair_tables(2, 2))
    assert sorted(full) == [(7, "a"), (7, "b"), (8, "a"), (8, "b")] and full[(8, "a")] == {"row": 2}
    with pytest.raises(ValueError):
        keyed_results(results[:2], [101, 102, 103], ["cut", "sit"], pi, pc, live)


def test_sweep_groups_cover_every_pair_once():
    from toist_amd import harness
    from toist_amd.sweep import pair_tables
    B, T = 2, 5
    pi, pc, _ = pair_tables(B, T)
    groups = harness._sweep_groups(pi, pc, B, T, 4, product=True)          # 2 captions per group
    assert groups == [(0, 4), (4, 8), (8, 10)]
    assert sorted(zip(pi.tolist(), pc.tolist())) == [(i, t) for i in range(B) for t in range(T)]
    for (lo, hi), caps in zip(groups, ([0, 1], [2, 3], [4])):
        assert sorted(set(pc[lo:hi].tolist())) == caps and sorted(set(pi[lo:hi].tolist())) == [0, 1]
    pi, pc, _ = pair_tables(B, T)
    assert harness._sweep_groups(pi, pc, B, T, None, product=True) == [(0, 10)] and harness._sweep_groups(pi, pc, B, T, 10, product=True) == [(0, 10)]
    assert harness._sweep_groups(pi, pc, B, T, 3, product=False) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    with pytest.raises(ValueError):
        harness._sweep_groups(pi, pc, B, T, 1, product=True)


def test_encode_sweep_refuses_cpu_tensors_and_gradients():
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    model = toist_amd.build_model(harness.default_args(device="cpu", enc_layers=1, dec_layers=1, num_queries=4))[0].eval()
    samples, tok, _, _ = harness.synthetic_batch(1, 64, 64, tokens=6, seed=1, max_targets=0)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.encode_sweep(samples, tok)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.sweep_images(samples)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.sweep_text(tok)
    with pytest.raises(RuntimeError, match="inference only"):
        model.encode_sweep(samples, tok)
    model.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="inference only"):
        model.sweep_images(samples)


def test_sweep_assemble_is_declared_exported_and_bound():
    from toist_amd import _lib
    with open(os.path.join(ROOT, "include", "toist_hip.h")) as f:
        header = f.read()
    assert len(re.findall(r"TOIST_API\s+int\s+toist_sweep_assemble\s*\(", header)) == 1
    with open(os.path.join(ROOT, "toist_amd", "csrc", "exports.map")) as f:
        assert re.search(r"global:\s*toist_\*;", f.read())
    p, i32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib.SIGNATURES["toist_sweep_assemble"] == [p, p, p, i32, i32, p, p, i32, i32, p, p, i32, i32, p, p, p, p, p]
    fn = _lib.lib().toist_sweep_assemble
    assert list(fn.argtypes) == _lib.SIGNATURES["toist_sweep_assemble"] and fn.restype is ctypes.c_int
    # the host side of the entry point refuses bad extents and null pointers before any launch
    assert fn(None, None, None, 1, 1, None, None, 1, 1, None, None, 1, 12, None, None, None, None, None) != _lib.TOIST_OK and "multiple of 8" in _lib.last_error()
    assert fn(None, None, None, 0, 1, None, None, 1, 1, None, None, 1, 8, None, None, None, None, None) != _lib.TOIST_OK and "bad extents" in _lib.last_error()
    assert fn(None, None, None, 1, 1, None, None, 1, 1, None, None, 1, 8, None, None, None, None, None) != _lib.TOIST_OK and "null pointer" in _lib.last_error()
    assert fn(None, None, None, 1, 1 << 30, None, None, 1, 1 << 30, None, None, 4, 8, None, None, None, None, None) != _lib.TOIST_OK and "2^31" in _lib.last_error()
    # no new descriptor struct: the entry point takes plain arguments only
    assert not any(issubclass(t, ctypes._Pointer) for t in _lib.SIGNATURES["toist_sweep_assemble"])
