"""Host side of the device image preparation (toist_amd/preprocess.py): the resampling tables against Pillow's own output
(tests/golden/preprocess.npz, written by tests/golden/make_golden_preprocess.py), the size rule, the targets, the descriptor layout
and the capacity checks.  No GPU: the two integer passes the kernel runs are emulated in numpy on the same tables."""
import os
import random

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMPLE = ("upscale", "reduce", "h_only", "v_only", "reduce6", "one_pixel")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "preprocess.npz")))


def _pass(img, tables, axis):
    bounds, coef = tables
    a = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + a.shape[1:], dtype=np.uint8)
    for i, (lo, n) in enumerate(bounds):
        acc = (1 << 21) + np.tensordot(coef[i, :n].astype(np.int64), a[lo:lo + n], axes=(0, 0))
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def emulate(img, out_hw, flip=False, crop=None):
    """flip -> crop -> horizontal pass -> vertical pass (each skipped when its extents are equal), integers only."""
    from toist_amd.preprocess import resample_tables
    if flip:
        img = img[:, ::-1]
    if crop is not None:
        t, l, h, w = crop
        img = img[t:t + h, l:l + w]
    if img.shape[1] != out_hw[1]:
        img = _pass(img, resample_tables(img.shape[1], out_hw[1]), 1)
    if img.shape[0] != out_hw[0]:
        img = _pass(img, resample_tables(img.shape[0], out_hw[0]), 0)
    return img


def test_symbol_is_declared_and_exported():
    from toist_amd import _lib
    header = open(os.path.join(ROOT, "include", "toist_hip.h")).read()
    assert "toist_image_prep(" in header and "#define TOIST_PREP_DESC_WORDS %d" % _lib.PREP_DESC_WORDS in header
    assert "toist_image_prep" in _lib.exported_symbols() and hasattr(_lib.lib(), "toist_image_prep")


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    from toist_amd import _lib
    h = _lib.lib()
    assert h.toist_image_prep(None, 0, None, None, 0, None, 0, 64, 64, None, None, None, 0, None) == 0            # empty batch capacity: nothing to do
    assert h.toist_image_prep(None, 0, None, None, 0, None, 1, 64, 64, None, None, None, 0, None) != 0            # null buffers
    assert "null" in _lib.last_error()
    assert h.toist_image_prep(16, 16, 16, 16, 4, 16, 1, 64, 64, 16, 16, 16, 16, None) != 0                        # both output modes
    assert "exactly one" in _lib.last_error()
    assert h.toist_image_prep(16, 16, 16, 16, 4, 16, 1, 64, 66, 16, 16, None, 0, None) != 0                       # 16-byte stores need cap_w % 4 == 0
    assert "cap_w" in _lib.last_error()


@pytest.mark.parametrize("name", SIMPLE + ("flip", "ragged0", "ragged1", "ragged2"))
def test_tables_reproduce_pillow_fixture(golden, name):
    src, want = golden[name + "_src"], golden[name + "_u8"]
    got = emulate(src, want.shape[:2], flip=(name == "flip"))
    assert got.shape == want.shape and np.array_equal(got, want), name


def test_tables_reproduce_the_chain(golden):
    flip, fh, fw, t, l, h, w, oh, ow = (int(v) for v in golden["chain_plan"])
    mid = emulate(golden["chain_src"], (fh, fw), flip=bool(flip))
    assert np.array_equal(mid, golden["chain_mid"])
    assert np.array_equal(emulate(mid, (oh, ow), crop=(t, l, h, w)), golden["chain_u8"])


def test_normalisation_table_reproduces_the_fixture(golden):
    from toist_amd.preprocess import normalisation_table
    lut = normalisation_table().numpy()
    assert lut.shape == (3, 256) and lut.dtype == np.float32
    for name in SIMPLE + ("flip", "chain"):
        u8 = golden[name + "_u8"]
        got = np.stack([lut[c][u8[:, :, c]] for c in range(3)])
        assert np.array_equal(got, golden[name + "_f32"]), name


def test_ragged_fixture_is_from_tensor_list(golden):
    from toist_amd.misc import NestedTensor
    nt = NestedTensor.from_tensor_list([torch.from_numpy(golden[f"ragged{i}_f32"]) for i in range(3)])
    assert torch.equal(nt.tensors, torch.from_numpy(golden["ragged_batch"])) and torch.equal(nt.mask, torch.from_numpy(golden["ragged_mask"]))


def test_table_shapes_and_identity():
    from toist_amd.preprocess import resample_tables
    bounds, coef = resample_tables(500, 80)
    assert coef.shape == (80, 15) and coef.dtype == np.int32 and bounds.shape == (80, 2) and bounds.dtype == np.int32
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 500).all() and (bounds[:, 1] <= 15).all()
    assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()           # the kernel's tile range relies on monotone bounds
    for i, (lo, n) in enumerate(bounds):
        assert (coef[i, n:] == 0).all() and abs(int(coef[i].sum()) - (1 << 22)) <= 15
    bounds, coef = resample_tables(7, 7)                     # equal extents: the rule itself is the identity
    img = np.arange(7 * 3, dtype=np.uint8).reshape(7, 1, 3) * 11
    assert np.array_equal(_pass(img, (bounds, coef), 0), img)
    with pytest.raises(ValueError):
        resample_tables(0, 5)


def test_tables_equal_live_pillow_on_fresh_seeds():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for (h, w), (oh, ow) in [((23, 31), (40, 37)), ((90, 64), (31, 64)), ((17, 200), (17, 33)), ((120, 160), (200, 266)), ((2, 3), (9, 1))]:
        src = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(src).resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(emulate(src, (oh, ow)), want), ((h, w), (oh, ow))


def test_size_rule_known_answers():
    from toist_amd.preprocess import resized_size, val_plan
    assert resized_size(640, 480, 800, 1333) == (800, 1066)
    assert resized_size(1000, 300, 800, 1333) == (400, 1333)
    assert resized_size(800, 900, 800, 1333) == (900, 800)            # a side already equal to `size`: the image stays as it is
    assert resized_size(700, 800, 800, 1333) == (914, 800)
    assert resized_size(480, 640, 600) == (800, 600)                  # no cap
    assert val_plan(640, 480).final == (800, 1066) and val_plan(640, 480).first is None and not val_plan(640, 480).flip


def _target():
    return {"boxes": torch.tensor([[10., 20., 50., 60.], [80., 10., 100., 30.]]), "labels": torch.tensor([1, 2]), "area": torch.tensor([1600., 400.]),
            "iscrowd": torch.tensor([0, 1]), "isfinal": torch.tensor([1., 0.]), "positive_map": torch.eye(2, 5),
            "masks": torch.zeros(2, 40, 100, dtype=torch.bool), "caption": "the cup left of the right plate", "size": torch.tensor([40, 100]),
            "orig_size": torch.tensor([40, 100])}


def test_transform_target_flip():
    from toist_amd.preprocess import PrepPlan, transform_target
    t = _target()
    t["masks"][0, 5, 10] = True
    out = transform_target(t, PrepPlan(100, 40, flip=True, final=(40, 100)))
    # xyxy (10,20,50,60) -> flipped (50,20,90,60) -> cxcywh / (100, 40)
    assert torch.allclose(out["boxes"][0], torch.tensor([0.7, 1.0, 0.4, 1.0]))
    assert out["caption"] == "the cup right of the left plate"
    assert bool(out["masks"][0, 5, 89]) and int(out["masks"].sum()) == 1
    assert torch.equal(t["boxes"], _target()["boxes"]) and t["caption"] == _target()["caption"]          # the input is untouched


def test_transform_target_resize():
    from toist_amd.preprocess import PrepPlan, transform_target
    out = transform_target(_target(), PrepPlan(100, 40, final=(80, 150)))
    # x * 1.5, y * 2: (15,40,75,120) -> cx 45 / 150, cy 80 / 80, w 60 / 150, h 80 / 80
    assert torch.allclose(out["boxes"][0], torch.tensor([0.3, 1.0, 0.4, 1.0]))
    assert torch.allclose(out["area"], torch.tensor([4800., 1200.]))
    assert out["size"].tolist() == [80, 150] and out["masks"].shape == (2, 80, 150) and out["orig_size"].tolist() == [40, 100]


def test_transform_target_crop_drops_a_box():
    from toist_amd.preprocess import PrepPlan, transform_target
    out = transform_target(_target(), PrepPlan(100, 40, crop=(10, 5, 30, 60), final=(30, 60)))
    # box 0 -> (5,10,45,50) clamped to (5,10,45,30); box 1 starts at x = 75 > 60: zero area, dropped with its rows
    assert out["boxes"].shape == (1, 4) and out["labels"].tolist() == [1] and out["iscrowd"].tolist() == [0] and out["isfinal"].tolist() == [1.]
    assert out["positive_map"].shape == (1, 5) and out["masks"].shape == (1, 30, 60) and out["area"].tolist() == [800.]
    assert torch.allclose(out["boxes"][0], torch.tensor([25 / 60, 20 / 30, 40 / 60, 20 / 30]))
    assert out["size"].tolist() == [30, 60]


def test_transform_target_chain():
    from toist_amd.preprocess import PrepPlan, transform_target
    out = transform_target(_target(), PrepPlan(100, 40, flip=True, first=(80, 200), crop=(0, 0, 80, 100), final=(160, 200)))
    # box 0: flip (50,20,90,60) -> x2 (100,40,180,120) -> crop to w = 100: zero width, dropped.  box 1: flip (0,10,20,30) -> (0,20,40,60) -> x2 (0,40,80,120)
    assert out["labels"].tolist() == [2]
    assert torch.allclose(out["boxes"][0], torch.tensor([40 / 200, 80 / 160, 80 / 200, 80 / 160]))
    assert torch.allclose(out["area"], torch.tensor([40. * 40 * 4]))


def test_sample_train_plan_structure():
    from toist_amd.preprocess import SCALES, PrepPlan, resized_size, sample_train_plan
    rng = random.Random(3)
    boxes = torch.tensor([[100., 100., 300., 300.], [400., 50., 600., 400.]])
    kinds = set()
    for _ in range(60):
        p = sample_train_plan(rng, 640, 480, boxes=boxes, cautious=False)
        assert isinstance(p, PrepPlan) and max(p.final) <= 1333
        kinds.add((p.flip, p.first is not None))
        if p.first is None:
            assert p.crop is None and p.final in {resized_size(640, 480, s, 1333) for s in SCALES}
        else:
            assert min(p.first) in (400, 500, 600) and 384 <= p.crop[2] <= p.first[0] and 384 <= p.crop[3] <= p.first[1]
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
    for _ in range(40):           # cautious: no flip, and the crop keeps every box
        p = sample_train_plan(rng, 640, 480, boxes=boxes, cautious=True)
        assert not p.flip
        if p.crop is not None:
            t, l, h, w = p.crop
            b = boxes * torch.tensor([p.first[1] / 640, p.first[0] / 480] * 2)
            x0, y0, x1, y1 = (b - torch.tensor([l, t, l, t])).unbind(1)
            assert ((x1.clamp(0, w) > x0.clamp(0, w)) & (y1.clamp(0, h) > y0.clamp(0, h))).all()


def test_descriptor_layout_round_trips():
    from toist_amd import _lib
    from toist_amd.preprocess import DESC_FIELDS, pack_descriptor, unpack_descriptor
    assert len(DESC_FIELDS) == _lib.PREP_DESC_WORDS == 20 and DESC_FIELDS[0] == "src_off" and DESC_FIELDS[9:11] == ("out_h", "out_w") and DESC_FIELDS[17] == "dst_off"
    fields = {name: 3 * i + 1 for i, name in enumerate(DESC_FIELDS)}
    row = pack_descriptor(**fields)
    assert row.dtype == np.int32 and row.shape == (20,) and row.tolist() == [3 * i + 1 for i in range(20)]
    assert unpack_descriptor(row) == fields
    assert unpack_descriptor(pack_descriptor(out_h=5))["out_h"] == 5 and int(pack_descriptor(out_h=5).sum()) == 5
    with pytest.raises(KeyError):
        pack_descriptor(height=3)
    with pytest.raises(OverflowError):
        pack_descriptor(src_off=2 ** 31)


def test_cpu_device_raises():
    from toist_amd.preprocess import DevicePreprocessor
    with pytest.raises(RuntimeError, match="no CPU path"):
        DevicePreprocessor("cpu", max_batch=2, max_src_pixels=1000, max_out_hw=(64, 64))


def _host_only_preprocessor(**kw):
    """A DevicePreprocessor without its device buffers: _layout (every capacity check) is host code."""
    from toist_amd import _lib
    from toist_amd.preprocess import DevicePreprocessor
    p = DevicePreprocessor.__new__(DevicePreprocessor)
    p.max_batch, p.max_src_pixels, p.max_out_hw, p.max_mid_hw, p.pad_hw = kw["max_batch"], kw["max_src_pixels"], kw["max_out_hw"], kw["max_mid_hw"], kw.get("pad_hw", 1)
    p.max_table_words = kw.get("max_table_words", 100000)
    p._desc_bytes = 2 * p.max_batch * _lib.PREP_DESC_WORDS * 4
    p._head_bytes = p._desc_bytes + 4 * p.max_table_words + 3 * p.max_src_pixels + 16 * p.max_batch
    p._head_bytes = (p._head_bytes + 15) // 16 * 16
    p._mid_bytes = 3 * p.max_batch * p.max_mid_hw[0] * p.max_mid_hw[1] + 16 * p.max_batch
    return p


def test_capacity_overruns_raise_and_layout_is_consistent():
    from toist_amd.preprocess import PrepPlan, unpack_descriptor, pack_descriptor
    p = _host_only_preprocessor(max_batch=2, max_src_pixels=5000, max_out_hw=(100, 100), max_mid_hw=(80, 80), pad_hw=64)
    img = np.zeros((40, 50, 3), dtype=np.uint8)
    plan = PrepPlan(50, 40, final=(64, 80))
    packed, rows, tables, pixels, used = p._layout([img, img], [plan, PrepPlan(50, 40, flip=True, first=(60, 75), crop=(1, 2, 50, 60), final=(90, 100))], False)
    assert (packed.batch, packed.height, packed.width, packed.two_stage) == (2, 128, 128, True) and used <= p._head_bytes
    assert not rows[0][0] and rows[0][1]["out_h"] == 60 and rows[0][1]["flip"] == 1 and rows[1][1]["flip"] == 0
    assert rows[1][1]["src_off"] == p._head_bytes + rows[0][1]["dst_off"] and rows[1][1]["src_stride"] == 75 * 3
    assert (rows[1][1]["crop_y"], rows[1][1]["crop_x"], rows[1][1]["crop_h"], rows[1][1]["crop_w"]) == (1, 2, 50, 60)
    # nothing overlaps: descriptors, tables, pixels
    spans = [(0, p._desc_bytes)] + [(4 * at, 4 * (at + b.size + c.size)) for at, b, c in tables] + [(at, at + a.size) for at, a in pixels]
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= used
    for r in (rows[0][1], rows[1][0], rows[1][1]):
        assert unpack_descriptor(pack_descriptor(**r))["coef_v"] == r["coef_v"] and r["ksize_h"] >= 1
    with pytest.raises(ValueError, match="max_batch"):
        p._layout([img] * 3, [plan] * 3, False)
    with pytest.raises(ValueError, match="max_src_pixels"):
        p._layout([np.zeros((60, 50, 3), dtype=np.uint8)] * 2, [PrepPlan(50, 60, final=(64, 80))] * 2, False)
    with pytest.raises(ValueError, match="exceeds the capacity"):
        p._layout([img], [PrepPlan(50, 40, final=(101, 80))], False)
    with pytest.raises(ValueError, match="max_mid_hw"):
        p._layout([img], [PrepPlan(50, 40, first=(81, 80), final=(64, 80))], False)
    with pytest.raises(ValueError, match="plan for"):
        p._layout([img], [PrepPlan(40, 50, final=(64, 80))], False)
    with pytest.raises(ValueError, match="uint8"):
        p._layout([img.astype(np.float32)], [plan], False)
    p.max_table_words = 100
    with pytest.raises(ValueError, match="max_table_words"):
        p._layout([img], [plan], False)
    with pytest.raises(ValueError, match="leaves"):
        PrepPlan(50, 40, crop=(0, 0, 41, 50), final=(64, 80))


def test_public_names():
    import toist_amd
    from toist_amd import preprocess
    for name in ("DevicePreprocessor", "PrepPlan", "val_plan", "sample_train_plan", "transform_target", "resized_size", "resample_tables"):
        assert getattr(toist_amd, name) is getattr(preprocess, name)
