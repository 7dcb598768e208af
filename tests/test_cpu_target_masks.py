"""Host side of the device-side target masks (toist_amd/preprocess.py: nearest_table, mask_index_tables, pack_mask_bits, transform_target(masks=False),
DeviceTargetMasks' layout and capacity checks; the argument checks of toist_target_masks) -- everything that needs no GPU.  The tables are checked
against torch's own F.interpolate(mode="nearest") and against transform_target's host masks, exactly."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairs():
    rng = random.Random(20240)
    return [(480, 800), (640, 1066), (427, 711), (1333, 400), (333, 1333), (7, 5), (5, 7), (3, 3), (1, 9), (9, 1)] + \
           [(rng.randint(1, 1400), rng.randint(1, 1400)) for _ in range(200)]


def test_nearest_table_is_torch_nearest_interpolation():
    from toist_amd.preprocess import nearest_table
    for n_in, n_out in _pairs():
        ref = torch.nn.functional.interpolate(torch.arange(n_in, dtype=torch.float32)[None, None, None, :], size=(1, n_out), mode="nearest")[0, 0, 0]
        got = nearest_table(n_in, n_out)
        assert got.dtype == np.int32 and got.shape == (n_out,)
        assert np.array_equal(got, ref.numpy().astype(np.int32)), (n_in, n_out)
    for bad in [(0, 5), (5, 0), (-1, 3)]:
        with pytest.raises(ValueError, match="positive"):
            nearest_table(*bad)


def _gathered_equals_host(plan, seed):
    from toist_amd.preprocess import mask_index_tables, transform_target
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(2, plan.height, plan.width, generator=g) > 0.5
    ty, tx = mask_index_tables(plan)
    assert ty.dtype == np.int32 and tx.dtype == np.int32 and ty.shape == (plan.final[0],) and tx.shape == (plan.final[1],)
    assert ty.min() >= 0 and ty.max() < plan.height and tx.min() >= 0 and tx.max() < plan.width
    want = transform_target({"masks": m}, plan)["masks"]          # (no boxes: the keep rule is "the cropped mask is not empty" -- dense random masks stay)
    got = m[:, torch.from_numpy(ty.copy()).long()][:, :, torch.from_numpy(tx.copy()).long()]          # (the cached tables are read-only)
    assert want.shape == got.shape and torch.equal(want, got), plan


def test_index_tables_reproduce_the_host_masks_on_sampled_training_plans():
    """200 plans of the training recipe's own sampler on small sources (the recipe's sizes -- 400..600 first, 384.. crops, 480..800 final -- apply to
    any source size: a 40 x 70 mask is first resized UP)."""
    from toist_amd.preprocess import sample_train_plan
    rng = random.Random(7)
    kinds = set()
    for i in range(200):
        w, h = rng.randint(20, 90), rng.randint(20, 60)
        plan = sample_train_plan(rng, w, h)
        kinds.add((plan.flip, plan.first is not None, plan.crop is not None))
        _gathered_equals_host(plan, 1000 + i)
    assert kinds == {(False, False, False), (True, False, False), (False, True, True), (True, True, True)}


def test_index_tables_reproduce_the_host_masks_on_small_plans():
    """Plans built directly at small sizes: flip only, identity size, first + crop + final, a crop touching each border, and 100 random ones."""
    from toist_amd.preprocess import PrepPlan
    named = [PrepPlan(53, 37, flip=True, final=(37, 53)),                                          # flip only
             PrepPlan(53, 37, final=(37, 53)),                                                     # identity size
             PrepPlan(90, 60, final=(23, 35)), PrepPlan(53, 37, final=(64, 91)),
             PrepPlan(53, 37, flip=True, first=(50, 71), crop=(5, 7, 30, 40), final=(64, 85)),     # first + crop + final
             PrepPlan(53, 37, first=(50, 71), crop=(0, 3, 20, 30), final=(33, 50)),                # the crop touches the top
             PrepPlan(53, 37, first=(50, 71), crop=(30, 3, 20, 30), final=(33, 50)),               # ... the bottom
             PrepPlan(53, 37, flip=True, first=(50, 71), crop=(4, 0, 20, 30), final=(33, 50)),     # ... the left
             PrepPlan(53, 37, flip=True, first=(50, 71), crop=(4, 41, 20, 30), final=(33, 50)),    # ... the right
             PrepPlan(53, 37, first=(50, 71), crop=(0, 0, 50, 71), final=(60, 85)),                # ... all four
             PrepPlan(53, 37, crop=(3, 4, 30, 40), final=(45, 60)),                                # a crop without a first resize
             PrepPlan(1, 1, final=(5, 7)), PrepPlan(9, 7, final=(1, 1))]
    for i, plan in enumerate(named):
        _gathered_equals_host(plan, 50 + i)
    rng = random.Random(11)
    for i in range(100):
        w, h = rng.randint(1, 90), rng.randint(1, 60)
        first = (rng.randint(1, 80), rng.randint(1, 100)) if rng.random() < 0.6 else None
        H, W = first if first is not None else (h, w)
        crop = None
        if rng.random() < 0.7:
            ch, cw = rng.randint(1, H), rng.randint(1, W)
            crop = (rng.randint(0, H - ch), rng.randint(0, W - cw), ch, cw)
        _gathered_equals_host(PrepPlan(w, h, rng.random() < 0.5, first, crop, (rng.randint(1, 100), rng.randint(1, 120))), 200 + i)


def test_mask_bits_round_trip_and_bit_order():
    from toist_amd.preprocess import pack_mask_bits, unpack_mask_bits
    g = torch.Generator().manual_seed(3)
    for w in (1, 31, 32, 33, 64, 95):
        m = torch.rand(3, 5, w, generator=g) > 0.5
        bits = pack_mask_bits(m)
        assert torch.is_tensor(bits) and bits.dtype == torch.uint8 and tuple(bits.shape) == (3, 5, 4 * ((w + 31) // 32))
        assert torch.equal(unpack_mask_bits(bits, w), m)
        as_np = pack_mask_bits(m.numpy().astype(np.uint8) * 255)          # uint8 input, an ndarray: non-zero = set
        assert isinstance(as_np, np.ndarray) and np.array_equal(as_np, bits.numpy())
        assert np.array_equal(unpack_mask_bits(as_np, w), m.numpy())
    # pixel x of a row is bit (x & 31) of 32-bit little-endian word (x >> 5): a hand-written 2 x 33 mask
    m = np.zeros((1, 2, 33), dtype=bool)
    m[0, 0, [0, 9, 31, 32]] = True
    m[0, 1, [1, 8, 30]] = True
    bits = pack_mask_bits(m)
    assert bits.shape == (1, 2, 8)
    assert bits[0, 0].tolist() == [0x01, 0x02, 0x00, 0x80, 0x01, 0, 0, 0] and bits[0, 1].tolist() == [0x02, 0x01, 0x00, 0x40, 0, 0, 0, 0]
    assert bits[0].copy().view("<u4").tolist() == [[0x80000201, 1], [0x40000102, 0]]
    with pytest.raises(ValueError):
        pack_mask_bits(np.zeros((2, 3), dtype=bool))
    with pytest.raises(ValueError):
        unpack_mask_bits(bits, 65)


def _target(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([w * 0.8, h * 0.8])
    wh = torch.rand(n, 2, generator=g) * torch.tensor([w * 0.2, h * 0.2]) + 1.0
    return {"boxes": torch.cat([xy, xy + wh], 1), "labels": torch.arange(n), "area": wh.prod(1), "iscrowd": torch.zeros(n, dtype=torch.int64),
            "positive_map": torch.rand(n, 16, generator=g), "isfinal": torch.ones(n), "caption": "the left cup right of it",
            "masks": torch.rand(n, h, w, generator=g) > 0.5, "orig_size": torch.tensor([h, w])}


def test_transform_target_without_masks_carries_rows_and_size():
    from toist_amd.preprocess import PrepPlan, transform_target
    plans = [PrepPlan(90, 60, final=(80, 120)), PrepPlan(90, 60, flip=True, final=(60, 90)),
             PrepPlan(90, 60, flip=True, first=(80, 120), crop=(10, 20, 40, 50), final=(64, 80)),
             PrepPlan(90, 60, first=(80, 120), crop=(0, 0, 30, 35), final=(60, 70)), PrepPlan(90, 60, crop=(30, 50, 30, 40), final=(45, 60))]
    dropped = 0
    for i, plan in enumerate(plans):
        tgt = _target(6, 60, 90, 300 + i)
        full, lean = transform_target(tgt, plan), transform_target(tgt, plan, masks=False)
        assert "masks" in tgt and "mask_rows" not in tgt                       # the input is not changed
        assert set(lean) == (set(full) - {"masks"}) | {"mask_rows", "mask_size"}
        assert lean["mask_rows"].dtype == torch.int64 and torch.equal(lean["mask_rows"], full["labels"])      # labels = arange: the rows that were kept
        assert lean["mask_size"] == tuple(plan.final) == tuple(full["masks"].shape[1:])
        assert len(lean["mask_rows"]) == full["masks"].shape[0]
        dropped += 6 - len(lean["mask_rows"])
        for k in set(full) - {"masks"}:
            assert torch.equal(full[k], lean[k]) if torch.is_tensor(full[k]) else full[k] == lean[k], k
        again = transform_target(tgt, plan, masks=True)
        assert set(again) == set(full) and torch.equal(again["masks"], full["masks"])
    assert dropped > 0, "no crop dropped a target: the test does not cover the keep filter"
    # a target without masks: nothing is added
    bare = {k: v for k, v in _target(3, 60, 90, 1).items() if k != "masks"}
    assert "mask_rows" not in transform_target(bare, plans[2], masks=False)
    # masks but no boxes: the keep rule of a crop reads the pixels
    only_masks = {"masks": torch.ones(2, 60, 90, dtype=torch.bool)}
    with pytest.raises(ValueError, match="no boxes"):
        transform_target(only_masks, plans[2], masks=False)
    lean = transform_target(only_masks, plans[0], masks=False)                # without a crop nothing is filtered
    assert lean["mask_rows"].tolist() == [0, 1] and lean["mask_size"] == (80, 120) and "masks" not in lean


def test_descriptor_layout_agrees_with_the_header():
    from toist_amd import _lib
    from toist_amd.preprocess import TMASK_DESC_FIELDS
    header = open(os.path.join(ROOT, "include", "toist_hip.h")).read()
    words = int(re.search(r"#define\s+TOIST_TMASK_DESC_WORDS\s+(\d+)", header).group(1))
    assert words == _lib.TMASK_DESC_WORDS == len(TMASK_DESC_FIELDS) and words in (8, 12)
    assert TMASK_DESC_FIELDS == ("src_off", "src_h", "src_w", "src_stride_words", "out_h", "out_w", "tab_y", "tab_x")
    section = header[header.index("target masks on the device"):header.index("#define TOIST_TMASK_DESC_WORDS")]
    for i, name in enumerate(TMASK_DESC_FIELDS):
        assert re.search(rf"\b{i} {name}\b", section), f"the header does not document word {i} as {name}"


def _host_only_target_masks(**kw):
    """A DeviceTargetMasks without its device buffers: _layout (every capacity check) is host code."""
    from toist_amd.preprocess import DeviceTargetMasks
    p = DeviceTargetMasks.__new__(DeviceTargetMasks)
    p._set_capacities(**kw)
    return p


def test_target_masks_on_a_cpu_device_raise():
    from toist_amd.preprocess import DeviceTargetMasks
    with pytest.raises(RuntimeError, match="no CPU path"):
        DeviceTargetMasks("cpu", max_batch=2, max_targets_per_image=2, max_src_pixels=1000, max_out_hw=(64, 64))


def test_capacity_overruns_raise_and_layout_is_consistent():
    from toist_amd.preprocess import PrepPlan, mask_index_tables
    p = _host_only_target_masks(max_batch=3, max_targets_per_image=3, max_src_pixels=3 * 40 * 64 + 2 * 30 * 32, max_out_hw=(100, 100))
    a, b = np.ones((3, 40, 50), dtype=bool), np.ones((2, 30, 20), dtype=np.uint8)
    pa, pb = PrepPlan(50, 40, flip=True, final=(64, 80)), PrepPlan(20, 30, first=(60, 40), crop=(1, 2, 50, 30), final=(90, 100))
    none = np.zeros((0, 40, 50), dtype=bool)
    packed, rows, tables, bits, used = p._layout([a, none, b], [pa, pa, pb])
    assert packed.slots == 5 and packed.counts == (3, 0, 2) and packed.sizes == ((64, 80), (64, 80), (90, 100)) and packed.link_bytes == used <= p._blob_bytes
    assert [r["out_h"] for r in rows] == [64, 64, 64, 90, 90] and [r["src_stride_words"] for r in rows] == [2, 2, 2, 1, 1]
    assert len(tables) == 4                                              # one pair per image WITH targets, shared by its slots
    assert rows[0]["tab_y"] == rows[2]["tab_y"] == p._desc_bytes // 4 and rows[0]["tab_x"] == rows[0]["tab_y"] + 64 and rows[3]["tab_y"] == rows[0]["tab_x"] + 80
    assert np.array_equal(tables[1][1], mask_index_tables(pa)[1]) and np.array_equal(tables[2][1], mask_index_tables(pb)[0])
    assert [r["src_off"] for r in rows] == [rows[0]["src_off"] + i * 40 * 8 for i in range(3)] + [rows[0]["src_off"] + 3 * 40 * 8 + i * 30 * 4 for i in range(2)]
    # nothing overlaps: descriptors, tables, bits; every mask starts 4-byte aligned
    spans = [(0, p._desc_bytes)] + [(4 * at, 4 * (at + t.size)) for at, t in tables] + [(r["src_off"], r["src_off"] + 4 * r["src_h"] * r["src_stride_words"]) for r in rows]
    spans.sort()
    assert all(s[1] <= t[0] for s, t in zip(spans, spans[1:])) and spans[-1][1] == used and all(r["src_off"] % 4 == 0 for r in rows)
    # only the surviving rows travel, in their order
    packed, rows, _, bits, _ = p._layout([a, none, b], [pa, pa, pb], [torch.tensor([2, 0]), torch.zeros(0, dtype=torch.int64), [1]])
    assert packed.slots == 3 and packed.counts == (2, 0, 1) and bits[0][1].shape == (2, 40, 50) and bits[1][1].shape == (1, 30, 20)
    with pytest.raises(ValueError, match="max_batch"):
        p._layout([a] * 4, [pa] * 4)
    with pytest.raises(ValueError, match="max_targets_per_image"):
        p._layout([np.ones((4, 40, 50), dtype=bool)], [pa])
    with pytest.raises(ValueError, match="max_src_pixels"):
        p._layout([a, a], [pa, pa])
    with pytest.raises(ValueError, match="exceeds the capacity"):
        p._layout([a], [PrepPlan(50, 40, final=(101, 80))])
    with pytest.raises(ValueError, match="plan for"):
        p._layout([a], [PrepPlan(40, 50, final=(64, 80))])
    with pytest.raises(ValueError, match="mask rows"):
        p._layout([a], [pa], [[3]])
    with pytest.raises(ValueError, match="bool or uint8"):
        p._layout([a.astype(np.float32)], [pa])
    with pytest.raises(ValueError, match="plans"):
        p._layout([a], [pa, pa])
    p.max_table_words = 100
    with pytest.raises(ValueError, match="max_table_words"):
        p._layout([a], [pa])
    with pytest.raises(ValueError, match="positive"):
        _host_only_target_masks(max_batch=0, max_targets_per_image=3, max_src_pixels=10, max_out_hw=(8, 8))


def test_static_targets_take_mask_sizes_instead_of_masks():
    """StaticTargets.pack on host buffers only: "mask_size" targets feed valid_hw as the masks' shapes do and stage no mask bytes."""
    from toist_amd.matcher import StaticTargets
    st = StaticTargets(2, 3, 10, 8, device="cpu", mask_hw=(64, 96))       # (a host-only instance: ordinary buffers, no GPU runtime)
    views, total = StaticTargets.arena_views(2, 6, 8)
    own = st._stage.open()
    assert own.numel() == total and tuple(st._mask_host.shape) == (6, 64, 96)
    boxes = lambda n: torch.rand(n, 4)
    by_masks = [{"boxes": boxes(2), "masks": torch.ones(2, 40, 90, dtype=torch.bool)}, {"boxes": boxes(0), "masks": torch.ones(0, 60, 50, dtype=torch.bool)}]
    by_size = [{"boxes": by_masks[0]["boxes"], "mask_size": (40, 90)}, {"boxes": boxes(0), "mask_size": (60, 50)}]
    pm = torch.rand(2, 8)
    host_a, sizes_a, mh = st.pack(by_masks, pm, out=own)
    valid_a = views(host_a)[6].clone()
    host_b, sizes_b, none = st.pack(by_size, pm, out=torch.zeros(total, dtype=torch.uint8))
    assert none is None and mh is not None and sizes_a == sizes_b == [2, 0]
    assert valid_a.tolist() == views(host_b)[6].tolist() == [60, 90, 15, 23]
    assert torch.equal(host_a, host_b)
    with pytest.raises(ValueError, match="mask_size"):
        st.pack([by_masks[0], by_size[1]], pm, out=own)
    with pytest.raises(ValueError, match="mask_size of 65 x 90"):
        st.pack([{"boxes": by_masks[0]["boxes"], "mask_size": (65, 90)}, by_size[1]], pm, out=own)


def test_entry_point_checks_its_arguments_without_a_gpu():
    from toist_amd import _lib
    handle = _lib.lib()
    assert "toist_target_masks" in _lib.exported_symbols() and hasattr(handle, "toist_target_masks")
    assert handle.toist_target_masks(None, 0, None, None, 0, 0, 0, 0, None, None) == 0                    # no slots: nothing to do
    rc = handle.toist_target_masks(None, 64, None, None, 64, 1, 8, 8, None, None)
    assert rc != 0 and "null" in _lib.last_error()
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    src, desc, arena, dst = base, base + 64, base + 128, base + 192                                        # host memory: every call below fails its checks before a launch
    rc = handle.toist_target_masks(src, 64, desc + 1, arena, 16, 1, 8, 8, dst, None)
    assert rc != 0 and "aligned" in _lib.last_error()
    assert handle.toist_target_masks(src + 2, 62, desc, arena, 16, 1, 8, 8, dst, None) != 0 and "aligned" in _lib.last_error()
    assert handle.toist_target_masks(src, 64, desc, arena, 16, 1, 0, 8, dst, None) != 0 and "capacity" in _lib.last_error()
    assert handle.toist_target_masks(src, 64, desc, arena, 16, 1, 8, -1, dst, None) != 0 and "capacity" in _lib.last_error()
    assert handle.toist_target_masks(src, 64, desc, arena, 16, -1, 8, 8, dst, None) != 0 and "slot count" in _lib.last_error()


def test_public_names():
    import toist_amd
    for name in ("DeviceTargetMasks", "PackedTargetMasks", "nearest_table", "mask_index_tables", "pack_mask_bits", "unpack_mask_bits"):
        assert getattr(toist_amd, name) is getattr(toist_amd.preprocess, name)
