"""CPU-side checks of the boundary: the C-ABI library loads and exports every symbol of
include/toist_hip.h, struct layouts agree with the header, the module tree is state_dict compatible
with the reference, and the product path refuses to run without the HIP device (no CPU fallback)."""
import ctypes
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "toist_hip.h")) as f:
        return f.read()


def test_library_exports_every_declared_symbol():
    """The names come from a regex of this test's own, not from the binding's parser: a prototype the parser skipped would be missing
    from exported_symbols() and show here."""
    from toist_amd import _lib
    header = _header()
    declared = set(re.findall(r"\b(toist_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    handle = _lib.lib()
    missing = [n for n in sorted(declared) if not hasattr(handle, n)]
    assert not missing, f"symbols declared in toist_hip.h but not exported: {missing}"
    assert set(_lib.exported_symbols()) == declared, (sorted(set(_lib.exported_symbols()) ^ declared))
    assert set(_lib.parse_signatures(header, _lib._BYREF)) == declared and len(_lib.SIGNATURES) == len(declared)
    for name, argtypes in _lib.SIGNATURES.items():
        fn = getattr(handle, name)
        assert list(fn.argtypes) == argtypes and fn.restype is ctypes.c_int, name
    assert handle.toist_version() == 1


# C name of every ctypes.Structure class of toist_amd/_lib.py: a new descriptor class goes here
C_STRUCTS = {"toist_operand": "Operand", "toist_epilogue": "Epilogue", "toist_gemm": "Gemm", "toist_reduce_desc": "ReduceDesc",
             "toist_rowgemm_desc": "RowGemm", "toist_xdec_layer": "XdecLayer", "toist_xdec_desc": "Xdec",
             "toist_xdec_bwd_layer": "XdecBwdLayer", "toist_xdec_bwd_desc": "XdecBwd"}


def test_struct_layouts_match_header(tmp_path):
    """One generated C program: sizeof of every struct the Python side builds, offsetof and sizeof of every field BY NAME, and every
    integer constant the binding parsed out of the header, each compared with what ctypes / numpy / the parser hold."""
    from abi_probe import c_values
    from toist_amd import _lib, optim
    classes = {n for n, v in vars(_lib).items() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure}
    assert classes == set(C_STRUCTS.values()), "every Structure class of _lib.py is probed"
    layouts = {}                                                    # C struct name -> (sizeof, [(field, offset, size)])
    for c_name, py_name in C_STRUCTS.items():
        cls = getattr(_lib, py_name)
        layouts[c_name] = (ctypes.sizeof(cls), [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_])
    # the optimizer tail's device tables and state word are numpy records (toist_amd/optim.py)
    for c_name, dt in (("toist_opt_tensor", optim._TENSOR_DT), ("toist_opt_group", optim._GROUP_DT), ("toist_opt_state", optim._STATE_DT)):
        layouts[c_name] = (dt.itemsize, [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names])
    want = {}
    for c_name, (size, fields) in layouts.items():
        want[f"sizeof({c_name})"] = size
        for name, offset, fsize in fields:
            want[f"offsetof({c_name}, {name})"] = offset
            want[f"sizeof((({c_name}*)0)->{name})"] = fsize
    assert _lib.CONSTANTS and all(re.fullmatch(r"TOIST_\w+", n) for n in _lib.CONSTANTS)
    want.update(_lib.CONSTANTS)                                     # the parser against the real preprocessor
    # the grouped-launch table rows are six int64 per problem (toist_amd/kernels.py: group_table), not a class: pinned below
    pins = ["sizeof(toist_group)", "offsetof(toist_group, c_off)", "offsetof(toist_group, colsum_off)"]
    exprs = list(want) + pins
    got = dict(zip(exprs, c_values(tmp_path, exprs)))
    wrong = {e: {"C": got[e], "python": v} for e, v in want.items() if got[e] != v}
    assert not wrong, wrong
    assert [got[e] for e in pins] == [48, 16, 32]
    assert got["sizeof(toist_opt_tensor)"] == 64 and got["sizeof(toist_opt_state)"] == 32 and got["offsetof(toist_opt_state, step)"] == 16
    assert got["offsetof(toist_gemm, epi)"] == _lib.Gemm.epi.offset and got["offsetof(toist_gemm, a_colsum)"] == _lib.Gemm.a_colsum.offset
    assert got["offsetof(toist_gemm, group)"] == _lib.Gemm.group.offset
    assert got["offsetof(toist_opt_tensor, numel)"] == optim._TENSOR_DT.fields["numel"][1]
    assert got["offsetof(toist_opt_tensor, group)"] == optim._TENSOR_DT.fields["group"][1]


SYNTHETIC_HEADER = """
/* TOIST_API int toist_commented_out(double x); */
// TOIST_API int toist_commented_out_too(unsigned k);
#define TOIST_API __attribute__((visibility("default")))
#define TOIST_SEVEN 7
#define TOIST_MINUS (-2)   /* in parentheses */
#define TOIST_NOT_A_NUMBER seven
enum { TOIST_E0 = 0, TOIST_E5 = 5 };
TOIST_API int toist_none(void);
TOIST_API int toist_every(int a, int32_t b, int64_t c, long long d, uint64_t e, float f, size_t g,
                          char* buf, const float* x, /* tables are cast by the caller */ const int32_t* const* table,
                          const toist_gemm* desc, toist_group* rows,
                          void* stream);
"""


def test_parser_binds_every_accepted_type():
    from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_longlong, c_size_t, c_uint64, c_void_p
    from toist_amd import _lib
    sigs = _lib.parse_signatures(SYNTHETIC_HEADER, _lib._BYREF)
    assert sigs == {"toist_none": [],
                    "toist_every": [c_int32, c_int32, c_int64, c_longlong, c_uint64, c_float, c_size_t, c_char_p, c_void_p, c_void_p,
                                    POINTER(_lib.Gemm), c_void_p, c_void_p]}
    assert _lib.parse_constants(SYNTHETIC_HEADER) == {"TOIST_SEVEN": 7, "TOIST_MINUS": -2, "TOIST_E0": 0, "TOIST_E5": 5}


@pytest.mark.parametrize("param", ["unsigned k", "double x", "toist_gemm d", "float*", "int"])
def test_parser_refuses_what_it_does_not_know(param):
    from toist_amd import _lib
    with pytest.raises(ValueError) as e:
        _lib.parse_signatures(f"TOIST_API int toist_ok(int n);\nTOIST_API int toist_odd(const void* x,\n    {param}, void* stream);\n", _lib._BYREF)
    assert "toist_odd" in str(e.value) and param in str(e.value)
    for text in ("TOIST_API float toist_odd(int n);", "TOIST_API int toist_odd(int n)\nTOIST_API int toist_next(void);", "TOIST_API int toist_odd(int (*f)(int));"):
        with pytest.raises(ValueError, match="toist_odd"):
            _lib.parse_signatures(text, {})
    with pytest.raises(ValueError, match="TOIST_BARE"):
        _lib.parse_constants("enum { TOIST_BARE, TOIST_NEXT = 1 };")


def test_signatures_of_the_irregular_entry_points():
    """Hand-written expectations on the real header, by ctypes kind and size (whether c_int64 and c_longlong are one class or two depends on the
    platform), plus the pointee class of the typed descriptor pointers."""
    from toist_amd import _lib

    def kinds(argtypes):
        return [("P", t._type_) if issubclass(t, ctypes._Pointer) else (t._type_, ctypes.sizeof(t)) for t in argtypes]

    void_p, i32, i64, ll = ("P", 8), ("i", 4), (ctypes.c_int64._type_, 8), (ctypes.c_longlong._type_, 8)
    sig = _lib.SIGNATURES
    assert kinds(sig["toist_last_error"]) == [("z", 8), (ctypes.c_size_t._type_, 8)] and sig["toist_last_error"][0] is ctypes.c_char_p
    assert kinds(sig["toist_gemm_bf16"]) == [("P", _lib.Gemm), void_p]
    assert kinds(sig["toist_rowgemm"]) == [("P", _lib.RowGemm), void_p] and kinds(sig["toist_xdec_fwd"]) == [("P", _lib.Xdec), void_p]
    assert kinds(sig["toist_xdec_bwd"]) == [("P", _lib.XdecBwd), void_p] and kinds(sig["toist_gemm_pick_tile"]) == [("P", _lib.Gemm)]
    assert kinds(sig["toist_image_prep"]) == [void_p, ll, void_p, void_p, ll, void_p, i32, i32, i32, void_p, void_p, void_p, ll, void_p]
    assert kinds(sig["toist_splitk_reduce_batch"]) == [void_p, i32, void_p]
    assert kinds(sig["toist_group_fill"]) == [void_p, i32, void_p, void_p]
    assert kinds(sig["toist_add_bf16"]) == [void_p, void_p, i64, i64, void_p, void_p]
    assert sig["toist_version"] == [] and sig["toist_wgrad3x3_small_blocks"] == []
    # every launch ends with the stream, a pointer
    last = dict(re.findall(r"\b(toist_\w+)\s*\([^()]*?(\w+)\s*\)\s*;", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    with_stream = [n for n, p in last.items() if p == "stream"]
    assert len(with_stream) > 70 and all(sig[n][-1] is ctypes.c_void_p for n in with_stream)


def test_bad_arguments_return_error_codes_without_a_gpu():
    from toist_amd import _lib
    handle = _lib.lib()
    d = _lib.Gemm()  # all zero: bad shape
    rc = handle.toist_gemm_bf16(ctypes.byref(d), None)
    assert rc == -1 and "bad shape" in _lib.last_error()


def test_no_cpu_fallback():
    from toist_amd import kernels, ops
    x = torch.zeros(8, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.layernorm_fwd(x, torch.ones(8), torch.zeros(8), 1e-5, x)


@pytest.fixture(scope="module")
def model():
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    return toist_amd.build_model(harness.default_args(device="cpu"))


def test_state_dict_is_reference_compatible(model):
    m, criterion, cluster, weight_dict = model
    assert cluster is None
    with open(os.path.join(ROOT, "tests", "golden", "reference_state_dict_shapes.json")) as f:
        ref = json.load(f)
    sd = m.state_dict()
    for k, shape in ref.items():
        if k.endswith("position_ids") or k.startswith("contrastive_align"):
            continue  # buffer of newer HF versions / built only with --contrastive_align_loss
        assert k in sd, f"missing reference key {k}"
        assert list(sd[k].shape) == shape, (k, list(sd[k].shape), shape)
    # torchvision resnet101 naming under backbone.0.body (public architecture; reference backbone.py:87-89)
    for k, shape in {"backbone.0.body.conv1.weight": [64, 3, 7, 7], "backbone.0.body.bn1.running_var": [64],
                     "backbone.0.body.layer1.0.downsample.0.weight": [256, 64, 1, 1], "backbone.0.body.layer3.22.conv2.weight": [256, 256, 3, 3],
                     "backbone.0.body.layer4.2.bn3.bias": [2048]}.items():
        assert list(sd[k].shape) == shape
    conv_params = sum(v.numel() for k, v in sd.items() if k.startswith("backbone.0.body") and ("conv" in k or "downsample.0" in k))
    assert conv_params == 42_394_816  # torchvision resnet101: 44,549,160 total - 2,049,000 (fc) - 105,344 (BN affine)
    assert not m.backbone[0].body.layer1[0].conv1.weight.requires_grad and m.backbone[0].body.layer2[0].conv1.weight.requires_grad
    assert sorted(weight_dict)[:3] == ["loss_bbox", "loss_bbox_0", "loss_bbox_1"] and len(weight_dict) == 18
    # main.py:351-366 builds LR groups from these substrings
    names = [n for n, _ in m.named_parameters()]
    assert any("backbone" in n for n in names) and any("text_encoder" in n for n in names)
    # checkpoints with BatchNorm bookkeeping load (backbone.py:40-42 drops num_batches_tracked)
    extra = dict(sd)
    extra["backbone.0.body.bn1.num_batches_tracked"] = torch.tensor(5)
    missing, unexpected = m.load_state_dict(extra, strict=False)
    assert not missing and not unexpected
    import copy
    copy.deepcopy(m)  # EMA copy in main.py:333


def test_nested_tensor_and_targets():
    from toist_amd.misc import NestedTensor, targets_to
    a, b = torch.ones(3, 5, 7), torch.ones(3, 6, 4)
    nt = NestedTensor.from_tensor_list([a, b])
    assert nt.tensors.shape == (2, 3, 6, 7) and nt.mask.dtype == torch.bool
    assert not nt.mask[0, :5, :7].any() and nt.mask[0, 5].all() and nt.mask[1, :, 4:].all()
    nt = NestedTensor.from_tensor_list([a, b], do_round=True)
    assert nt.tensors.shape == (2, 3, 128, 128)
    t = targets_to([{"boxes": torch.zeros(1, 4), "caption": "x", "tokens_positive": [[(0, 1)]]}], "cpu")
    assert "caption" not in t[0] and t[0]["tokens_positive"] == [[(0, 1)]]


def test_nearest_mask_matches_interpolate():
    from toist_amd.backbone import nearest_mask
    g = torch.Generator().manual_seed(0)
    m = torch.rand(3, 97, 131, generator=g) > 0.5
    for hw in [(4, 5), (13, 17), (25, 33), (97, 131)]:
        ref = torch.nn.functional.interpolate(m[None].float(), size=hw).bool()[0]
        assert torch.equal(nearest_mask(m, hw), ref)


def test_matcher_module_contract_on_cpu_raises():
    from toist_amd.matcher import HungarianMatcher
    m = HungarianMatcher(1.0, 5.0, 2.0)
    out = {"pred_logits": torch.zeros(1, 4, 8), "pred_boxes": torch.rand(1, 4, 4)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(out, [{"boxes": torch.rand(2, 4)}], torch.rand(2, 8))
    with pytest.raises(AssertionError):
        HungarianMatcher(0, 0, 0)


def test_segmentation_wrapper_state_dict():
    """DETRsegm keeps the reference names (segmentation.py:17-38; main.py:481,499 rely on `.detr` and
    'mask_head.adapter3.bias') and freezes DETR before creating the mask branch when asked to."""
    import toist_amd
    from toist_amd import harness
    torch.manual_seed(0)
    args = harness.default_args(device="cpu", masks=True, mask_model="smallconv", frozen_weights="some.pth")
    model, criterion, _, wd = toist_amd.build_model(args)
    with open(os.path.join(ROOT, "tests", "golden", "reference_segm_state_dict_shapes.json")) as f:
        ref = json.load(f)
    sd = model.state_dict()
    for k, shape in ref.items():
        assert k in sd and list(sd[k].shape) == shape, k
    assert "detr.class_embed.weight" in sd and hasattr(model, "detr")
    trainable = sum(p.numel() for p in model.parameters() if p.requires_grad)
    assert trainable == sum(p.numel() for n, p in model.named_parameters() if not n.startswith("detr."))  # only the mask branch
    assert 1_300_000 < trainable < 1_400_000  # SURVEY: 1.33 M parameters
    assert "masks" in criterion.losses and wd["loss_mask"] == 1.0 and wd["loss_dice"] == 1.0


def test_compute_copy_registry_is_keyed_by_tensor_identity():
    """The caching allocator reuses a freed parameter's address for the next model: a registry hit must be the same tensor
    object, not merely the same address (a stale row in the optimizer's pointer table writes past the smaller copy)."""
    import gc
    import torch
    from toist_amd import engine
    cache = {}
    t = torch.nn.Parameter(torch.randn(8, 4))
    w = engine.compute_copy(t, engine._cast_bf16, cache, "w")
    assert engine.copy_of(t) is not None and engine.copy_of(t).w is w
    alias = t.detach()[:2]                                    # same address, another tensor (and another size)
    assert alias.data_ptr() == t.data_ptr() and engine.copy_of(alias) is None
    ptr = t.data_ptr()
    del t, alias
    gc.collect()
    engine.prune_copies()
    assert ptr not in engine.COPIES


def test_store_once_row_ranges_are_tracked_on_the_root_view():
    """ADVICE r2 (engine.py ParamView): the store-once state of a packed parameter is a set of row ranges on the ROOT view -- a second slice
    of the same rows sees the first launch (it must accumulate, not store), marking one slice does not mark its siblings, and the rows
    nothing wrote are reported for zeroing."""
    import torch
    from toist_amd.engine import ParamView
    g = torch.zeros(12, 4)
    root = ParamView(None, g, fresh=True)
    q1, v1 = root.rows(0, 8), root.rows(8, 12)
    assert not root.written and not q1.written and not v1.written
    q1.mark_written()
    assert q1.written and not v1.written and not root.written           # a sibling slice and the whole slot stay unwritten
    assert root.rows(0, 8).written and root.rows(2, 6).written          # a NEW view of the stored rows accumulates
    assert not root.rows(4, 10).written
    assert root.unwritten_rows() == [(8, 12)]
    v1.mark_written()
    assert root.written and root.unwritten_rows() == []
    root.written = False
    assert not q1.written and root.unwritten_rows() == [(0, 12)]
    root.mark_written()
    assert q1.written and root.rows(3, 4).rows(0, 1).written and root.unwritten_rows() == []
    nested = ParamView(None, torch.zeros(12, 4), fresh=True)
    nested.rows(4, 12).rows(2, 4).mark_written()                         # rows 6..8 of the root
    assert nested.unwritten_rows() == [(0, 6), (8, 12)]


def test_memory_cache_materialises_lazy_entries_on_read():
    """transformer.MemoryCache: the fp32 API copies of memory_cache are thunks until somebody reads them; reads, membership, iteration and
    assignment behave like the plain dict of the reference (transformer.py:146-157)."""
    from toist_amd.transformer import MemoryCache
    calls = []

    def thunk(name, value):
        def f():
            calls.append(name)
            return value
        return f

    mc = MemoryCache({"mask": 1}, lazy={"img_memory": thunk("img", torch.ones(2)), "pos_embed": thunk("pos", torch.zeros(2))})
    mc._lazy["text_memory"] = lambda: mc["img_memory"][-1:]
    assert "img_memory" in mc and mc.is_lazy("img_memory") and len(mc) == 4 and calls == []
    assert mc["mask"] == 1 and calls == []
    assert torch.equal(mc["text_memory"], torch.ones(1)) and calls == ["img"] and not mc.is_lazy("img_memory")
    assert mc["img_memory"] is mc["img_memory"] and calls == ["img"]              # materialised once
    mc["pos_embed"] = "replaced"                                                  # assignment drops the thunk
    assert mc.get("pos_embed") == "replaced" and "pos" not in calls
    mc2 = MemoryCache({}, lazy={"a": thunk("a", 5)})
    assert dict(mc2.items()) == {"a": 5} and calls[-1] == "a" and list(mc2) == ["a"]
    assert mc2.get("missing", 7) == 7 and mc2.pop("a") == 5 and "a" not in mc2


def test_distill_tables_follow_in_place_refills():
    """distill._cached_table keys a batch's caption-driven tables on the identity AND the in-place version of its token tensor: a loop that refills a
    static input_ids buffer in place (a captured step's feed) must not be served the previous batch's tables."""
    import torch
    from toist_amd import distill
    ids = torch.zeros(2, 4, dtype=torch.long)
    calls = []
    make = lambda: calls.append(1) or len(calls)
    assert distill._cached_table("t_test", (ids,), (), make) == 1
    assert distill._cached_table("t_test", (ids,), (), make) == 1          # same contents: cached
    ids.copy_(torch.ones(2, 4, dtype=torch.long))                          # refilled in place
    assert distill._cached_table("t_test", (ids,), (), make) == 2


@pytest.mark.parametrize("order", ["alone", "extra_before", "extra_after"])
def test_matched_rows_sentinel_survives_autograd_accumulation(order):
    """The hand-off of toist_amd/segmentation.py (`_MaskLossFn.backward` -> `matched_rows_of`), driven on the CPU with the same objects: the
    producer returns the zero sentinel (one element, expanded, kept alive by the sink); the consumer must see THAT tensor iff nothing else
    consumed pred_masks, and a correct dense sum otherwise -- in particular when the other consumer was created first, the order in which
    autograd's input buffer accumulates onto the first-arrived gradient (in place, if it owns it alone: VERDICT r5 weak #1)."""
    from toist_amd import segmentation as sg
    sink = sg._MatchedRows()
    seen = {}

    class Producer(torch.autograd.Function):          # stands for the mask program: receives the gradient of pred_masks
        @staticmethod
        def forward(ctx, x):
            return x * 1.0

        @staticmethod
        def backward(ctx, g):
            zero = sink.sentinel
            seen["is_sentinel"] = bool(zero is not None and g.data_ptr() == zero.data_ptr() and not any(g.stride()) and zero._version == sink.version)
            seen["g"] = g.clone()
            return g.contiguous()

    class Loss(torch.autograd.Function):              # stands for _MaskLossFn
        @staticmethod
        def forward(ctx, pred):
            ctx.shape = pred.shape
            return pred.sum() * 0.0

        @staticmethod
        def backward(ctx, g):
            zero = sg._zero_sentinel(torch.device("cpu"))
            sink.grad, sink.sentinel, sink.version = torch.ones(1), zero, zero._version
            return zero.expand(ctx.shape)

    x = torch.randn(3, 4, 5, requires_grad=True)
    masks = Producer.apply(x)
    extra = (masks * masks).mean() if order == "extra_before" else None
    loss = Loss.apply(masks.view(12, 5))
    if order == "extra_after":
        extra = (masks * masks).mean()
    (loss if extra is None else loss + extra).backward()
    assert seen["is_sentinel"] == (order == "alone")
    want = torch.zeros_like(x) if order == "alone" else 2 * x.detach() / x.numel()
    assert torch.allclose(seen["g"], want, atol=1e-7)
    assert float(sg._zero_sentinel(torch.device("cpu"))) == 0.0 and sg._zero_sentinel(torch.device("cpu"))._version == sink.version


def test_box_ops_against_the_reference_fixture():
    """toist_amd/box_ops.py (API-edge helpers, rewritten in round 6 as one broadcast over the four corners) against values the REAL reference's
    util/box_ops.py produced (tests/golden/box_ops.npz, make_golden.py)."""
    import numpy as np
    from toist_amd import box_ops
    d = np.load(os.path.join(ROOT, "tests", "golden", "box_ops.npz"))
    a, b = torch.from_numpy(d["a"]), torch.from_numpy(d["b"])
    axy, bxy = box_ops.box_cxcywh_to_xyxy(a), box_ops.box_cxcywh_to_xyxy(b)
    assert np.allclose(axy.numpy(), d["axy"], atol=1e-7)
    assert np.allclose(box_ops.box_xyxy_to_cxcywh(axy).numpy(), d["back"], atol=1e-6)
    iou, union = box_ops.box_iou(axy, bxy)
    assert np.allclose(iou.numpy(), d["iou"], atol=1e-6) and np.allclose(union.numpy(), d["union"], atol=1e-6)
    assert np.allclose(box_ops.generalized_box_iou(axy, bxy).numpy(), d["giou"], atol=1e-6)
    bad = axy.clone()
    bad[0, 2] = bad[0, 0] - 1.0
    with pytest.raises(AssertionError):
        box_ops.generalized_box_iou(bad, bxy)


def test_postprocess_forwards_pred_isfinal():
    """PostProcess keeps the reference's `pred_isfinal` -> `scores_refexp` branch (/root/reference/models/postprocessors.py:49-54), and
    its scores / boxes equal the reference fixture's (postprocess.npz) when the key is absent."""
    import numpy as np
    from toist_amd.postprocessors import PostProcess
    d = np.load(os.path.join(ROOT, "tests", "golden", "postprocess.npz"))
    out = {"pred_logits": torch.from_numpy(d["logits"]), "pred_boxes": torch.from_numpy(d["boxes"])}
    sizes = torch.from_numpy(d["sizes"])
    res = PostProcess()(out, sizes)
    for i, r in enumerate(res):
        assert set(r) == {"scores", "labels", "boxes"}
        assert np.allclose(r["scores"].numpy(), d["scores"][i], atol=1e-6) and np.allclose(r["boxes"].numpy(), d["out_boxes"][i], atol=1e-4)
    fin = torch.linspace(-3, 3, d["logits"].shape[0] * d["logits"].shape[1]).view(d["logits"].shape[0], -1, 1)
    res2 = PostProcess()(dict(out, pred_isfinal=fin), sizes)
    for i, r in enumerate(res2):
        assert torch.allclose(r["scores_refexp"], res[i]["scores"] * torch.sigmoid(fin[i, :, 0]), atol=1e-7)
