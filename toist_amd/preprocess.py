"""Image preparation on the device: the reference's host pipeline between a decoded uint8 image and the model's input (datasets/tdod.py:301-335
make_coco_transforms, datasets/transforms.py, util/misc.py:185-209 NestedTensor.from_tensor_list) with the pixels done by ONE HIP launch per batch
(csrc/prep.hip: toist_image_prep) -- the host link carries the original uint8 pixels, not fp32 planes at the resized size.

The host keeps what is cheap and per image: the size rule, the random decisions of the training recipe (a PrepPlan), the targets
(transform_target) and the resampling tables.  torchvision's F.resize on a PIL image is Image.resize((w, h), BILINEAR), and Pillow's 8-bit
resampler is integer arithmetic on coefficients computed in double precision: resample_tables restates that computation in numpy float64,
the kernel does the integer passes, so the prepared pixels EQUAL the reference's (tests/golden/preprocess.npz is Pillow's own output).

The masks of the targets (configs[2]) go the same way: flip, nearest resize and crop are index maps that compose into one row table and one column
table per image (mask_index_tables); DeviceTargetMasks sends the masks at their original size with one bit per pixel and ONE launch
(csrc/tmask.hip: toist_target_masks) gathers them into the bytes the mask losses read -- the bytes transform_target's torch ops produce.

Those source masks are rasterised polygon annotations (datasets/tdod.py:133-147).  DevicePolygonMasks does that on the device as well: the host sends
the vertices on rleFrPoly's 5x grid (polygon_tables) and ONE launch (csrc/poly.hip: toist_polygon_masks) writes the bits coco_eval.polygon_to_mask
computes, an object's polygons merged by union -- DeviceTargetMasks.pack_polygons puts them where toist_target_masks reads its source.

There is no CPU path: DevicePreprocessor, DeviceTargetMasks and DevicePolygonMasks on a CPU device raise, like misc.DeviceStager."""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, staging
from .box_ops import box_xyxy_to_cxcywh
from .misc import NestedTensor, interpolate

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)                      # tdod.py:303
SCALES = (480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800)            # tdod.py:305
MAX_SIZE = 1333
PRECISION_BITS = 22


# ---- sizes and tables ----------------------------------------------------------------------------------------------------------------------
def resized_size(w, h, size, max_size=None):
    """The reference's get_size_with_aspect_ratio (transforms.py:86-104): short side to `size`, long side capped at `max_size`.  -> (h, w)."""
    w, h = int(w), int(h)
    if max_size is not None:
        lo, hi = float(min(w, h)), float(max(w, h))
        if hi / lo * size > max_size:
            size = int(round(max_size * lo / hi))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def _tables(n_in, n_out):
    scale = np.float64(n_in) / np.float64(n_out)
    fs = max(scale, np.float64(1.0))
    support = fs                                                   # the bilinear filter's support is 1
    ksize = 2 * int(np.ceil(support)) + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    hi = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in)
    n = hi - lo
    j = np.arange(ksize, dtype=np.int64)[None, :]
    ss = np.float64(1.0) / fs
    w = np.maximum(0.0, 1.0 - np.abs(((j + lo[:, None]) - center[:, None] + 0.5) * ss))
    w = np.where(j < n[:, None], w, 0.0)
    total = np.zeros(n_out, dtype=np.float64)
    for c in range(ksize):                                         # left to right, as the resampler sums them
        total = total + w[:, c]
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    coef = np.trunc(w * float(1 << PRECISION_BITS) + 0.5).astype(np.int32)
    bounds = np.stack([lo, n], axis=1).astype(np.int32)
    return bounds, coef


@functools.lru_cache(maxsize=512)
def _cached_tables(n_in, n_out):
    bounds, coef = _tables(n_in, n_out)
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef


def resample_tables(n_in, n_out):
    """Pillow's bilinear resampling of one axis from extent n_in to n_out for 8-bit images.  -> (bounds int32 [n_out, 2] = (first tap, tap count),
    coef int32 [n_out, ksize], 22 fractional bits, zero behind the tap count); ksize = 2 * ceil(max(n_in / n_out, 1)) + 1.  One pass is
    out[i] = clip((2^21 + sum_j pixel[first_i + j] * coef[i, j]) >> 22, 0, 255).  Everything before the final integer rounding is float64."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"resample_tables: extents must be positive (got {n_in} -> {n_out})")
    return _cached_tables(n_in, n_out)


@functools.lru_cache(maxsize=64)
def _identity_tables(n):
    bounds = np.stack([np.arange(n), np.ones(n, dtype=np.int64)], axis=1).astype(np.int32)
    return bounds, np.full((n, 1), 1 << PRECISION_BITS, dtype=np.int32)


def _pass_tables(n_in, n_out):
    """The tables the kernel gets: a pass whose extents are equal is the identity (Pillow skips it) -- one tap of weight 1."""
    return _identity_tables(n_in) if n_in == n_out else resample_tables(n_in, n_out)


# ---- the decisions for one image -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class PrepPlan:
    """What happens to one image, in the reference's order: horizontal flip -> optional first resize -> optional crop -> final resize (-> ToTensor,
    Normalize).  width / height: the source; first: (h, w) of the first resize or None; crop: (top, left, h, w) in the coordinates of the image
    it is applied to (the first resize's output, or the flipped source without one) or None; final: (h, w) of the prepared image."""
    width: int
    height: int
    flip: bool = False
    first: Optional[Tuple[int, int]] = None
    crop: Optional[Tuple[int, int, int, int]] = None
    final: Tuple[int, int] = (0, 0)

    def __post_init__(self):
        if self.width <= 0 or self.height <= 0 or self.final[0] <= 0 or self.final[1] <= 0:
            raise ValueError(f"PrepPlan: bad sizes {self}")
        if self.first is not None and (self.first[0] <= 0 or self.first[1] <= 0):
            raise ValueError(f"PrepPlan: bad first resize {self.first}")
        if self.crop is not None:
            t, l, h, w = self.crop
            H, W = self.first if self.first is not None else (self.height, self.width)
            if t < 0 or l < 0 or h <= 0 or w <= 0 or t + h > H or l + w > W:
                raise ValueError(f"PrepPlan: the crop {self.crop} leaves the {H} x {W} image it is applied to")


def val_plan(w, h):
    """The validation recipe (tdod.py:327-333): resize 800 / 1333."""
    return PrepPlan(int(w), int(h), final=resized_size(w, h, 800, MAX_SIZE))


def _boxes_survive(boxes, plan_flip, w, h, first, region):
    t = {"boxes": torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4)}
    n = len(t["boxes"])
    if plan_flip:
        t = _t_hflip(t, w)
    t = _t_resize(t, (h, w), first)
    return len(_t_crop(t, region)["boxes"]) == n


def sample_train_plan(rng, w, h, boxes=None, cautious=False):
    """A plan with the STRUCTURE of the reference's training recipe (tdod.py:308-325): flip with probability 1/2 (never when `cautious`), then with
    probability 1/2 one resize to a random scale / 1333, else resize to one of 400 / 500 / 600, a random crop of 384 .. 1333 per side and the resize
    to a random scale / 1333.  With `cautious` the crop is drawn again (150 times at most, RandomSizeCrop's respect_boxes, transforms.py:163-181)
    until no box of `boxes` (xyxy, source coordinates) is cropped out; when none is found the image stays un-cropped, as in the reference.
    `rng` is a random.Random (random(), randint(a, b), choice(seq)).  It does NOT reproduce the reference's random stream: the reference draws from the
    global `random` module and torch.randint in an order this function does not follow, so the same seed gives other decisions."""
    w, h = int(w), int(h)
    flip = (not cautious) and rng.random() < 0.5
    if rng.random() < 0.5:
        return PrepPlan(w, h, flip, None, None, resized_size(w, h, rng.choice(SCALES), MAX_SIZE))
    first = resized_size(w, h, rng.choice((400, 500, 600)), None)
    fh, fw = first
    crop = None
    for _ in range(150):
        cw = rng.randint(min(384, fw), min(fw, MAX_SIZE))
        ch = rng.randint(min(384, fh), min(fh, MAX_SIZE))
        region = (rng.randint(0, fh - ch), rng.randint(0, fw - cw), ch, cw)
        if not cautious or boxes is None or _boxes_survive(boxes, flip, w, h, first, region):
            crop = region
            break
    ch, cw = (crop[2], crop[3]) if crop is not None else first
    return PrepPlan(w, h, flip, first, crop, resized_size(cw, ch, rng.choice(SCALES), MAX_SIZE))


# ---- targets (host) ------------------------------------------------------------------------------------------------------------------------
def _t_hflip(t, w):
    t = dict(t)
    if "boxes" in t:
        t["boxes"] = t["boxes"][:, [2, 1, 0, 3]] * torch.as_tensor([-1, 1, -1, 1]) + torch.as_tensor([w, 0, w, 0])
    if "masks" in t:
        t["masks"] = t["masks"].flip(-1)
    if "caption" in t:
        t["caption"] = t["caption"].replace("left", "[TMP]").replace("right", "left").replace("[TMP]", "right")
    return t


def _t_resize(t, old_hw, new_hw):
    t = dict(t)
    rh, rw = float(new_hw[0]) / float(old_hw[0]), float(new_hw[1]) / float(old_hw[1])
    if "boxes" in t:
        t["boxes"] = t["boxes"] * torch.as_tensor([rw, rh, rw, rh])
    if "area" in t:
        t["area"] = t["area"] * (rw * rh)
    t["size"] = torch.tensor([int(new_hw[0]), int(new_hw[1])])
    if "masks" in t:
        t["masks"] = interpolate(t["masks"][:, None].float(), tuple(int(v) for v in new_hw), mode="nearest")[:, 0] > 0.5
    return t


def _t_crop(t, region):
    t = dict(t)
    i, j, h, w = region
    t["size"] = torch.tensor([h, w])
    fields = ["labels", "area", "iscrowd", "positive_map", "isfinal", "mask_rows"]
    if "boxes" in t:
        b = t["boxes"] - torch.as_tensor([j, i, j, i])
        b = torch.min(b.reshape(-1, 2, 2), torch.as_tensor([w, h], dtype=torch.float32)).clamp(min=0)
        t["area"] = (b[:, 1, :] - b[:, 0, :]).prod(dim=1)
        t["boxes"] = b.reshape(-1, 4)
        fields.append("boxes")
    if "masks" in t:
        t["masks"] = t["masks"][:, i:i + h, j:j + w]
        fields.append("masks")
    if "boxes" in t or "masks" in t:
        if "boxes" in t:
            b = t["boxes"].reshape(-1, 2, 2)
            keep = torch.all(b[:, 1, :] > b[:, 0, :], dim=1)
        else:
            keep = t["masks"].flatten(1).any(1)
        for f in fields:
            if f in t:
                t[f] = t[f][keep]
    return t


def transform_target(target, plan, masks=True):
    """What the reference's transforms do to a target dict along `plan` (transforms.py hflip 62-80, resize 118-138, crop 18-59, Normalize 262-273), on
    the host: boxes (xyxy in, cxcywh / (w, h, w, h) out), area, size, masks (flip, nearest resize, slice: torch ops) and caption (left <-> right on a
    flip); after a crop the boxes of zero area go, with their rows of labels, area, iscrowd, positive_map, isfinal and masks.  The input is not changed.
    masks=False leaves the pixels of "masks" to the device (DeviceTargetMasks): the entry is neither read nor produced; the result carries "mask_rows"
    (int64: the source rows of "masks" that survive the crop's keep rule, all of them without a crop) and "mask_size" (plan.final as (h, w)) instead.
    The keep rule of a target with masks but no boxes reads the pixels (transforms.py crop: masks.flatten(1).any(1)): that stays a host job, and
    masks=False raises ValueError for a crop on such a target."""
    t = dict(target)
    by_size = not masks and "masks" in t
    if by_size:
        if plan.crop is not None and "boxes" not in t:
            raise ValueError("transform_target(masks=False): a crop on a target with masks but no boxes keeps the targets whose CROPPED mask is "
                             "not empty -- that rule reads the pixels, transform it with masks=True")
        n = len(t["boxes"]) if "boxes" in t else int(t["masks"].shape[0])
        del t["masks"]
        t["mask_rows"] = torch.arange(n, dtype=torch.int64)
    hw = (plan.height, plan.width)
    if plan.flip:
        t = _t_hflip(t, plan.width)
    if plan.first is not None:
        t = _t_resize(t, hw, plan.first)
        hw = plan.first
    if plan.crop is not None:
        t = _t_crop(t, plan.crop)
        hw = (plan.crop[2], plan.crop[3])
    t = _t_resize(t, hw, plan.final)
    if "boxes" in t:
        h, w = plan.final
        t["boxes"] = box_xyxy_to_cxcywh(t["boxes"]) / torch.tensor([w, h, w, h], dtype=torch.float32)
    if by_size:
        t["mask_size"] = (int(plan.final[0]), int(plan.final[1]))
    return t


# ---- target masks: index tables and packed bits (host) ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=512)
def _cached_nearest(n_in, n_out):
    scale = np.float32(n_in) / np.float32(n_out)
    t = np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale), np.float32(n_in - 1)).astype(np.int32)
    t.setflags(write=False)
    return t


def nearest_table(n_in, n_out):
    """The source index F.interpolate(mode="nearest") picks for every output index of an axis resized from n_in to n_out: int32 [n_out] =
    min(floor(float32(i) * (float32(n_in) / float32(n_out))), n_in - 1), the product formed in float32 as torch forms it.  (Read-only: cached.)"""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"nearest_table: extents must be positive (got {n_in} -> {n_out})")
    return _cached_nearest(n_in, n_out)


def mask_index_tables(plan):
    """flip -> first resize -> crop -> final resize of a mask as ONE gather: -> (ty int32 [final_h], tx int32 [final_w]), the source row of every
    prepared row and the source column of every prepared column, so that prepared = source[:, ty][:, :, tx] equals transform_target's masks bit for
    bit.  Each step is an index map; they compose by indexing one table with the next, the flip last (on source columns: width - 1 - x)."""
    h, w = (plan.crop[2], plan.crop[3]) if plan.crop is not None else plan.first if plan.first is not None else (plan.height, plan.width)
    ty, tx = nearest_table(h, plan.final[0]), nearest_table(w, plan.final[1])
    if plan.crop is not None:
        ty, tx = ty + np.int32(plan.crop[0]), tx + np.int32(plan.crop[1])
    if plan.first is not None:
        ty, tx = nearest_table(plan.height, plan.first[0])[ty], nearest_table(plan.width, plan.first[1])[tx]
    if plan.flip:
        tx = np.int32(plan.width - 1) - tx
    return np.ascontiguousarray(ty, dtype=np.int32), np.ascontiguousarray(tx, dtype=np.int32)


def _mask_array(masks):
    a = masks.detach().cpu().numpy() if torch.is_tensor(masks) else np.asarray(masks)
    if a.dtype not in (np.bool_, np.uint8) or a.ndim != 3:
        raise ValueError(f"target masks are bool or uint8 [n, h, w] (got {a.dtype} {a.shape})")
    return a


_NO_MASK = np.zeros((1, 1, 1), dtype=np.bool_)          # broadcast to [n, h, w]: a mask stack that has a shape and no pixels (pack_polygons)


def _pack_bits(a):
    n, h, w = a.shape
    b = a if a.dtype == np.bool_ else a != 0
    if w % 32:
        padded = np.zeros((n, h, 32 * ((w + 31) // 32)), dtype=np.bool_)
        padded[:, :, :w] = b
        b = padded
    return np.packbits(b, axis=-1, bitorder="little")


def pack_mask_bits(masks):
    """bool or uint8 [n, h, w] (a host tensor or an ndarray; non-zero = set) -> uint8 [n, h, 4 * ceil(w / 32)] of the same kind: one bit per pixel, pixel
    x of a row = bit (x & 31) of its 32-bit little-endian word (x >> 5), rows padded with zero bits to whole words: the source format of toist_target_masks."""
    bits = _pack_bits(_mask_array(masks))
    return torch.from_numpy(bits) if torch.is_tensor(masks) else bits


def unpack_mask_bits(bits, width):
    """The inverse of pack_mask_bits: uint8 [n, h, 4 * ceil(width / 32)] -> bool [n, h, width] of the same kind."""
    a = bits.detach().cpu().numpy() if torch.is_tensor(bits) else np.asarray(bits)
    width = int(width)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 * ((width + 31) // 32):
        raise ValueError(f"unpack_mask_bits: uint8 [n, h, {4 * ((width + 31) // 32)}] for a width of {width} (got {a.dtype} {a.shape})")
    m = np.unpackbits(a, axis=-1, bitorder="little")[:, :, :width].astype(np.bool_)
    return torch.from_numpy(m) if torch.is_tensor(bits) else m


# ---- the packed descriptor -------------------------------------------------------------------------------------------------------------------
DESC_FIELDS = ("src_off", "src_h", "src_w", "src_stride", "flip", "crop_y", "crop_x", "crop_h", "crop_w", "out_h", "out_w", "ksize_h", "ksize_v",
               "bounds_h", "coef_h", "bounds_v", "coef_v", "dst_off", "reserved0", "reserved1")
assert len(DESC_FIELDS) == _lib.PREP_DESC_WORDS


def pack_descriptor(**fields):
    """One row of toist_image_prep's descriptor table (include/toist_hip.h) as int32 [PREP_DESC_WORDS]; fields left out are 0."""
    unknown = set(fields) - set(DESC_FIELDS)
    if unknown:
        raise KeyError(f"pack_descriptor: unknown fields {sorted(unknown)}")
    row = np.zeros(len(DESC_FIELDS), dtype=np.int32)
    for name, v in fields.items():
        if not -2 ** 31 <= int(v) < 2 ** 31:
            raise OverflowError(f"pack_descriptor: {name} = {v} does not fit int32")
        row[DESC_FIELDS.index(name)] = int(v)
    return row


def unpack_descriptor(row):
    return {name: int(v) for name, v in zip(DESC_FIELDS, np.asarray(row).reshape(-1))}


def normalisation_table():
    """fp32 [3, 256]: ToTensor + Normalize of every byte value, (v / 255 - mean[c]) / std[c], computed by torch as the reference computes it."""
    v = torch.arange(256, dtype=torch.float32).div(255)
    return (v[None, :] - torch.tensor(MEAN, dtype=torch.float32)[:, None]) / torch.tensor(STD, dtype=torch.float32)[:, None]


@dataclass(frozen=True)
class PackedBatch:
    """What pack() placed in the arenas: image count, the batch extent (largest output rounded up to pad_hw) and whether any image has a first resize."""
    batch: int
    height: int
    width: int
    two_stage: bool
    sizes: tuple          # (h, w) of every prepared image


def _up(v, m):
    return (int(v) + m - 1) // m * m


def _as_hwc(img):
    a = img.detach().cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError(f"DevicePreprocessor: images are uint8 [h, w, 3] (got {a.dtype} {a.shape})")
    return a


class DevicePreprocessor:
    """Decoded uint8 images + PrepPlans -> the padded fp32 batch and its mask, on the device.

    Owns fixed-address device memory -- one blob holding the two descriptor tables, the resampling tables and the source pixels of a batch,
    followed by the intermediate uint8 images of two-resize plans; the normalisation table; the output [max_batch, 3, Hc, Wc] + mask at the capacity
    (max_out_hw rounded up to pad_hw, the width to a multiple of 4) -- and one pinned host image of the blob's head.
      pack(images, plans)   : fills the pinned buffer and issues ONE asynchronous host-to-device copy on the current stream -> PackedBatch
      launch(out=None)      : one launch (two when an image has a first resize: that stage writes the uint8 image between the resizes), sizes
                              read from the device, nothing else: the launches can be captured once and replayed after every pack()
      prepare(images, plans, out=None) = pack + launch -> NestedTensor of the batch extent (views into the capacity-sized output, which is
                              written completely: zeros and mask True outside each image, whatever it held before)
    The batch extent is the largest prepared image rounded up to pad_hw: with pad_hw = 64 it is a captured step's bucket shape, and captured.upload
    takes its existing path.  `out` = a NestedTensor [Bc <= max_batch, 3, Hp, Wp % 4 == 0] / [Bc, Hp, Wp] of the caller's to write instead.
    Every capacity (max_batch, max_src_pixels over the batch, max_out_hw, max_mid_hw for the image between two resizes, the table words) is
    checked on the host and raises ValueError before anything is copied or launched."""

    def __init__(self, device, max_batch, max_src_pixels, max_out_hw, pad_hw=1, max_mid_hw=None, max_table_words=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DevicePreprocessor prepares images in GPU memory: there is no CPU path")
        self.max_batch, self.max_src_pixels, self.pad_hw = int(max_batch), int(max_src_pixels), int(pad_hw)
        self.max_out_hw = (int(max_out_hw[0]), int(max_out_hw[1]))
        self.max_mid_hw = (int(max_mid_hw[0]), int(max_mid_hw[1])) if max_mid_hw is not None else self.max_out_hw
        if self.max_batch <= 0 or self.max_src_pixels <= 0 or self.pad_hw <= 0 or min(self.max_out_hw) <= 0 or min(self.max_mid_hw) <= 0:
            raise ValueError("DevicePreprocessor: capacities must be positive")
        self.cap_hw = (_up(self.max_out_hw[0], self.pad_hw), _up(_up(self.max_out_hw[1], self.pad_hw), 4))
        # two axes x two stages per image, ksize 3 (bounds + coefficients = 5 words per output index) with room for reductions up to ksize 16
        self.max_table_words = int(max_table_words) if max_table_words is not None else \
            self.max_batch * 2 * 18 * (sum(self.max_out_hw) + sum(self.max_mid_hw))
        B = self.max_batch
        self._desc_bytes = 2 * B * _lib.PREP_DESC_WORDS * 4
        self._head_bytes = _up(self._desc_bytes + 4 * self.max_table_words + 3 * self.max_src_pixels + 16 * (B + 1), 16)     # what pack() may fill
        self._mid_bytes = _up(3 * B * self.max_mid_hw[0] * self.max_mid_hw[1] + 16 * B, 16)
        if self._head_bytes + self._mid_bytes >= 2 ** 31:
            raise ValueError("DevicePreprocessor: the arenas address bytes with 31 bits")
        self.blob = torch.zeros(self._head_bytes + self._mid_bytes, dtype=torch.uint8, device=self.device)
        self.desc = self.blob[:self._desc_bytes].view(torch.int32).view(2, B, _lib.PREP_DESC_WORDS)      # [0]: first-resize stage, [1]: final stage
        self.arena = self.blob.view(torch.int32)          # table offsets are int32 words from the blob's start
        self.mid = self.blob[self._head_bytes:]
        self.lut = normalisation_table().to(self.device)
        self.out = NestedTensor(torch.zeros(B, 3, *self.cap_hw, device=self.device), torch.ones(B, *self.cap_hw, dtype=torch.bool, device=self.device))
        self._stage = staging.Staging(torch.zeros(self._head_bytes, dtype=torch.uint8), self.device)
        self._last = None

    # -- host side ----------------------------------------------------------------------------------------------------------------------
    def _layout(self, images, plans, u8):
        """Host check + placement of a batch: -> (PackedBatch, rows [2, B] of descriptor dicts, table list, pixel list, used bytes).  Raises ValueError on
        any capacity overrun; touches no buffer."""
        if len(images) != len(plans) or not images:
            raise ValueError(f"DevicePreprocessor: {len(images)} images for {len(plans)} plans (at least one)")
        if len(images) > self.max_batch:
            raise ValueError(f"DevicePreprocessor: a batch of {len(images)} exceeds max_batch = {self.max_batch}")
        imgs = [_as_hwc(im) for im in images]
        for a, p in zip(imgs, plans):
            if a.shape[:2] != (p.height, p.width):
                raise ValueError(f"DevicePreprocessor: a {a.shape[0]} x {a.shape[1]} image with a plan for {p.height} x {p.width}")
            limit = self.max_mid_hw if u8 else self.max_out_hw
            if p.final[0] > limit[0] or p.final[1] > limit[1]:
                raise ValueError(f"DevicePreprocessor: a prepared size of {p.final[0]} x {p.final[1]} exceeds the capacity {limit[0]} x {limit[1]}")
            if p.first is not None and u8:
                raise ValueError("DevicePreprocessor: resize_u8 takes single-resize plans")
            if p.first is not None and (p.first[0] > self.max_mid_hw[0] or p.first[1] > self.max_mid_hw[1]):
                raise ValueError(f"DevicePreprocessor: a first resize to {p.first[0]} x {p.first[1]} exceeds max_mid_hw = {self.max_mid_hw[0]} x {self.max_mid_hw[1]}")
        if sum(a.shape[0] * a.shape[1] for a in imgs) > self.max_src_pixels:
            raise ValueError(f"DevicePreprocessor: {sum(a.shape[0] * a.shape[1] for a in imgs)} source pixels exceed max_src_pixels = {self.max_src_pixels}")
        word = self._desc_bytes // 4
        tables, where = [], {}

        def place(n_in, n_out):
            nonlocal word
            key = (n_in, n_out)
            if key not in where:
                bounds, coef = _pass_tables(n_in, n_out)
                where[key] = (word, word + bounds.size, coef.shape[1])
                tables.append((word, bounds, coef))
                word += bounds.size + coef.size
            return where[key]

        def stage(src_off, src_hw, stride, flip, crop, out_hw, dst_off=0):
            t, l, ch, cw = crop if crop is not None else (0, 0, src_hw[0], src_hw[1])
            bh, ck, kh = place(cw, out_hw[1])
            bv, cv, kv = place(ch, out_hw[0])
            return dict(src_off=src_off, src_h=src_hw[0], src_w=src_hw[1], src_stride=stride, flip=int(bool(flip)), crop_y=t, crop_x=l, crop_h=ch, crop_w=cw,
                        out_h=out_hw[0], out_w=out_hw[1], ksize_h=kh, ksize_v=kv, bounds_h=bh, coef_h=ck, bounds_v=bv, coef_v=cv, dst_off=dst_off)

        rows = [[{} for _ in imgs], [{} for _ in imgs]]
        pending, mid_at = [], 0
        for i, (a, p) in enumerate(zip(imgs, plans)):
            hw = (p.height, p.width)
            if u8:
                pending.append((0, i, (hw, p.width * 3, p.flip, p.crop, p.final, mid_at)))
                mid_at += _up(3 * p.final[0] * p.final[1], 16)
            elif p.first is None:
                pending.append((1, i, (hw, p.width * 3, p.flip, p.crop, p.final)))
            else:
                pending.append((0, i, (hw, p.width * 3, p.flip, None, p.first, mid_at)))
                rows[1][i] = stage(self._head_bytes + mid_at, p.first, p.first[1] * 3, False, p.crop, p.final)
                mid_at += _up(3 * p.first[0] * p.first[1], 16)
        if mid_at > self._mid_bytes:
            raise ValueError(f"DevicePreprocessor: {mid_at} bytes of intermediate images exceed the capacity of {self._mid_bytes} (max_mid_hw)")
        # the tables are placed first, the pixels behind them: every offset is known once the table words are
        for s, i, args in pending:
            rows[s][i] = stage(0, *args)
        if word - self._desc_bytes // 4 > self.max_table_words:
            raise ValueError(f"DevicePreprocessor: {word - self._desc_bytes // 4} table words exceed max_table_words = {self.max_table_words}")
        at = _up(word * 4, 16)
        pixels = []
        for s, i, _ in pending:
            rows[s][i]["src_off"] = at
            pixels.append((at, imgs[i]))
            at += _up(imgs[i].size, 16)
        H = _up(max(p.final[0] for p in plans), self.pad_hw)
        W = _up(max(p.final[1] for p in plans), self.pad_hw)
        packed = PackedBatch(len(imgs), H, W, any(rows[0][i] for i in range(len(imgs))), tuple(tuple(p.final) for p in plans))
        return packed, rows, tables, pixels, at

    def pack(self, images, plans, _u8=False, _layout=None):
        """The batch into the arenas: pixels, descriptors and tables into the pinned buffer, then one asynchronous copy of its used head on the current
        stream (the previous copy out of the pinned buffer is waited for first).  -> PackedBatch."""
        packed, rows, tables, pixels, used = _layout if _layout is not None else self._layout(images, plans, _u8)
        assert used <= self._head_bytes
        host = self._stage.open_np()
        desc = host[:self._desc_bytes].view(np.int32).reshape(2, self.max_batch, _lib.PREP_DESC_WORDS)
        desc[:] = 0                                             # unused slots: out_h = 0 = an empty image (padding only)
        for s in (0, 1):
            for i, r in enumerate(rows[s]):
                if r:
                    desc[s, i] = pack_descriptor(**r)
        words = host.view(np.int32)
        for at, bounds, coef in tables:
            words[at:at + bounds.size] = bounds.reshape(-1)
            words[at + bounds.size:at + bounds.size + coef.size] = coef.reshape(-1)
        for at, a in pixels:
            host[at:at + a.size].reshape(a.shape)[...] = a
        self._stage.upload_head(self.blob, used)
        self._last = packed
        return packed

    # -- device side --------------------------------------------------------------------------------------------------------------------
    def launch(self, out=None, first_stage=None):
        """The launches of the batch that pack() placed: the first-resize stage (when `first_stage`; None = the last pack() needs it -- pass True in
        a captured loop whose batches may) and the final stage into `out` (default: the object's own output).  -> the capacity-sized NestedTensor."""
        from . import kernels
        out = self.out if out is None else out
        Bc = int(out.tensors.shape[0])
        if Bc > self.max_batch or (self._last is not None and Bc < self._last.batch):
            raise ValueError(f"DevicePreprocessor: an output of {Bc} images for a batch of {self._last.batch if self._last else 0} (max_batch {self.max_batch})")
        if first_stage is None:
            first_stage = self._last is not None and self._last.two_stage
        if first_stage:
            kernels.image_prep(self.blob, self.desc[0, :Bc], self.arena, dst_u8=self.mid, cap_hw=self.max_mid_hw)
        kernels.image_prep(self.blob, self.desc[1, :Bc], self.arena, lut=self.lut, out=out.tensors, mask=out.mask)
        return out

    def _check_out(self, out, packed):
        if out is None:
            return
        t, m = out.tensors, out.mask
        if t.dim() != 4 or t.shape[1] != 3 or m is None or tuple(m.shape) != (t.shape[0], t.shape[2], t.shape[3]) or t.dtype != torch.float32:
            raise ValueError("DevicePreprocessor: `out` is a NestedTensor of fp32 [B, 3, Hp, Wp] with its [B, Hp, Wp] mask")
        if t.shape[0] < packed.batch or t.shape[0] > self.max_batch or t.shape[2] < packed.height or t.shape[3] < packed.width:
            raise ValueError(f"DevicePreprocessor: `out` {tuple(t.shape)} cannot hold {packed.batch} images of extent {packed.height} x {packed.width}")

    def view(self, packed, out=None):
        """The batch extent of a capacity-sized output as a NestedTensor of views."""
        out = self.out if out is None else out
        return NestedTensor(out.tensors[:packed.batch, :, :packed.height, :packed.width], out.mask[:packed.batch, :packed.height, :packed.width])

    def prepare(self, images, plans, out=None):
        layout = self._layout(images, plans, False)            # every capacity is checked before anything is copied or launched
        self._check_out(out, layout[0])
        packed = self.pack(images, plans, _layout=layout)
        return self.view(packed, self.launch(out))

    def resize_u8(self, images, plans):
        """The intermediate mode on its own: flip / crop / resize of single-resize plans -> a list of uint8 [h, w, 3] device tensors (views into the
        intermediate arena, valid until the next call), what the reference holds as a PIL image before ToTensor."""
        packed = self.pack(images, plans, _u8=True)
        from . import kernels
        kernels.image_prep(self.blob, self.desc[0], self.arena, dst_u8=self.mid, cap_hw=self.max_mid_hw)
        res, at = [], 0
        for h, w in packed.sizes:
            res.append(self.mid[at:at + 3 * h * w].view(h, w, 3))
            at += _up(3 * h * w, 16)
        return res


# ---- target masks on the device ----------------------------------------------------------------------------------------------------------------
TMASK_DESC_FIELDS = ("src_off", "src_h", "src_w", "src_stride_words", "out_h", "out_w", "tab_y", "tab_x")
assert len(TMASK_DESC_FIELDS) == _lib.TMASK_DESC_WORDS


@dataclass(frozen=True)
class PackedTargetMasks:
    """What DeviceTargetMasks.pack() placed: the live slots (surviving targets of the batch, in target order), the surviving targets and the prepared
    (h, w) of every image, and the bytes of the one host-to-device copy."""
    slots: int
    counts: tuple
    sizes: tuple
    link_bytes: int


class DeviceTargetMasks:
    """The masks of a batch's targets at their ORIGINAL size + PrepPlans -> the prepared masks (flip, nearest resize, crop, zero padding), on the device.

    The host link carries one bit per source pixel; one launch (csrc/tmask.hip: toist_target_masks) gathers the bits through one row table and one
    column table per image (mask_index_tables) into the uint8 [slots, Hp, Wp] image that the mask losses read (matcher.StaticTargets.masks).  The
    loader side transforms its targets with transform_target(target, plan, masks=False) and keeps the source masks.
    Owns fixed-address device memory -- one blob: the descriptor table [max_batch * max_targets_per_image, TMASK_DESC_WORDS], the index tables, the
    packed bits -- and its pinned host image.
      pack(masks_per_image, plans, rows_per_image=None) : fills the pinned image and issues ONE asynchronous host-to-device copy of its used head on
                              the current stream -> PackedTargetMasks.  masks_per_image[i] = bool / uint8 [n_i, plans[i].height, plans[i].width];
                              rows_per_image[i] = the "mask_rows" of transform_target(masks=False): only those masks are uploaded, in that order.
                              Slots are the surviving targets in target order across the batch (StaticTargets' order); an image without targets
                              takes none.
      write_into(static_targets) : one launch into static_targets.masks; sizes come from the device only, so it can be captured once and replayed
                              after every pack().  Slots behind the batch's targets are not written.
      dense(packed)         : list of bool [n_i, h_i, w_i] device tensors (the list-of-dicts criterion's "masks").
    Every capacity (max_batch, max_targets_per_image, max_src_pixels = source pixels summed over the surviving masks with every row counted in whole
    32-pixel words, max_out_hw, the table words) is checked on the host and raises ValueError before anything is copied or launched."""

    def __init__(self, device, max_batch, max_targets_per_image, max_src_pixels, max_out_hw, max_table_words=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceTargetMasks prepares masks in GPU memory: there is no CPU path")
        self._set_capacities(max_batch, max_targets_per_image, max_src_pixels, max_out_hw, max_table_words)
        self.blob = torch.zeros(self._blob_bytes, dtype=torch.uint8, device=self.device)
        self.desc = self.blob[:self._desc_bytes].view(torch.int32).view(self.max_slots, _lib.TMASK_DESC_WORDS)
        self.arena = self.blob.view(torch.int32)              # table offsets are int32 words from the blob's start
        self._stage = staging.Staging(torch.zeros(self._blob_bytes, dtype=torch.uint8), self.device)
        self._dense = None                                    # uint8 [max_slots, *max_out_hw], on the first dense()
        self.last = None                                      # the PackedTargetMasks of the last pack()

    def _set_capacities(self, max_batch, max_targets_per_image, max_src_pixels, max_out_hw, max_table_words=None):
        """The capacities and the byte layout they imply (host only)."""
        self.max_batch, self.max_targets_per_image, self.max_src_pixels = int(max_batch), int(max_targets_per_image), int(max_src_pixels)
        self.max_out_hw = (int(max_out_hw[0]), int(max_out_hw[1]))
        if self.max_batch <= 0 or self.max_targets_per_image <= 0 or self.max_src_pixels <= 0 or min(self.max_out_hw) <= 0:
            raise ValueError("DeviceTargetMasks: capacities must be positive")
        self.max_slots = self.max_batch * self.max_targets_per_image
        self.max_table_words = int(max_table_words) if max_table_words is not None else self.max_batch * sum(self.max_out_hw)    # one pair per image
        self._desc_bytes = self.max_slots * _lib.TMASK_DESC_WORDS * 4
        self._blob_bytes = _up(self._desc_bytes + 4 * self.max_table_words + (self.max_src_pixels + 7) // 8, 16)
        if self.max_slots > 65535 or self._blob_bytes >= 2 ** 31:
            raise ValueError("DeviceTargetMasks: at most 65535 slots, and the blob is addressed with 31 bits")

    # -- host side ----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _selected(rows, n, what):
        """One image's "mask_rows" as int64 indices into its n masks / segmentations; ValueError when one points outside."""
        rows = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows, dtype=np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= n):
            raise ValueError(f"DeviceTargetMasks: mask rows {rows.tolist()} of an image with {n} {what}")
        return rows

    def _write_head(self, rows, tables):
        """The descriptors of the live slots and the index tables into the pinned image, once its previous upload has left it -> its numpy view."""
        host = self._stage.open_np()
        desc = host[:self._desc_bytes].view(np.int32).reshape(self.max_slots, _lib.TMASK_DESC_WORDS)
        desc[:] = 0                                             # slots behind the batch's targets: out_h = 0 = dead, not written
        for i, r in enumerate(rows):
            desc[i] = [r[name] for name in TMASK_DESC_FIELDS]
        words = host.view(np.int32)
        for at, table in tables:
            words[at:at + table.size] = table
        return host

    def _layout(self, masks_per_image, plans, rows_per_image=None):
        """Host check + placement of a batch: -> (PackedTargetMasks, descriptor dicts of the live slots, [(word, table)], [(byte, source masks)], used
        bytes).  Raises ValueError on any capacity overrun; touches no buffer."""
        if len(masks_per_image) != len(plans) or not plans:
            raise ValueError(f"DeviceTargetMasks: {len(masks_per_image)} mask stacks for {len(plans)} plans (at least one)")
        if len(plans) > self.max_batch:
            raise ValueError(f"DeviceTargetMasks: a batch of {len(plans)} exceeds max_batch = {self.max_batch}")
        if rows_per_image is not None and len(rows_per_image) != len(plans):
            raise ValueError(f"DeviceTargetMasks: {len(rows_per_image)} row lists for {len(plans)} plans")
        stacks = []
        for i, (m, p) in enumerate(zip(masks_per_image, plans)):
            a = _mask_array(m)
            if a.shape[0] and a.shape[1:] != (p.height, p.width):
                raise ValueError(f"DeviceTargetMasks: {a.shape[1]} x {a.shape[2]} masks with a plan for {p.height} x {p.width}")
            if rows_per_image is not None:
                a = a[self._selected(rows_per_image[i], a.shape[0], "masks")]
            if a.shape[0] > self.max_targets_per_image:
                raise ValueError(f"DeviceTargetMasks: {a.shape[0]} targets of one image exceed max_targets_per_image = {self.max_targets_per_image}")
            if p.final[0] > self.max_out_hw[0] or p.final[1] > self.max_out_hw[1]:
                raise ValueError(f"DeviceTargetMasks: a prepared size of {p.final[0]} x {p.final[1]} exceeds the capacity {self.max_out_hw[0]} x {self.max_out_hw[1]}")
            stacks.append(a)
        stride = lambda p: (p.width + 31) // 32
        pixels = sum(a.shape[0] * p.height * stride(p) * 32 for a, p in zip(stacks, plans))
        if pixels > self.max_src_pixels:
            raise ValueError(f"DeviceTargetMasks: {pixels} source pixels (rows in whole 32-pixel words) exceed max_src_pixels = {self.max_src_pixels}")
        word = self._desc_bytes // 4
        tables, where = [], []
        for a, p in zip(stacks, plans):
            if not a.shape[0]:
                where.append(None)
                continue
            ty, tx = mask_index_tables(p)
            where.append((word, word + ty.size))
            tables.append((word, ty))
            tables.append((word + ty.size, tx))
            word += ty.size + tx.size
        if word - self._desc_bytes // 4 > self.max_table_words:
            raise ValueError(f"DeviceTargetMasks: {word - self._desc_bytes // 4} table words exceed max_table_words = {self.max_table_words}")
        at = word * 4
        rows, bits = [], []
        for a, p, tab in zip(stacks, plans, where):
            if tab is None:
                continue
            bits.append((at, a))
            for _ in range(a.shape[0]):
                rows.append(dict(src_off=at, src_h=p.height, src_w=p.width, src_stride_words=stride(p), out_h=p.final[0], out_w=p.final[1],
                                 tab_y=tab[0], tab_x=tab[1]))
                at += p.height * stride(p) * 4
        packed = PackedTargetMasks(len(rows), tuple(a.shape[0] for a in stacks), tuple((int(p.final[0]), int(p.final[1])) for p in plans), at)
        return packed, rows, tables, bits, at

    def pack(self, masks_per_image, plans, rows_per_image=None):
        """The batch into the blob: descriptors, tables and packed bits into the pinned image, then one asynchronous copy of its used head on the
        current stream (the previous copy out of the pinned image is waited for first).  -> PackedTargetMasks."""
        packed, rows, tables, bits, used = self._layout(masks_per_image, plans, rows_per_image)
        assert used <= self._blob_bytes and packed.slots <= self.max_slots
        host = self._write_head(rows, tables)
        for at, a in bits:
            b = _pack_bits(a)
            host[at:at + b.size] = b.reshape(-1)
        self._stage.upload_head(self.blob, used)
        self.last = packed
        return packed

    def pack_polygons(self, segmentations_per_image, plans, rows_per_image=None, *, polygons):
        """pack() for targets that still are polygon annotations: segmentations_per_image[i] = one list of flat polygons per target of image i, at the
        size (plans[i].height, plans[i].width).  The descriptors and index tables are pack()'s; the source-bit area of the blob is filled by the
        rasterise launch of `polygons` (a DevicePolygonMasks) on the current stream, behind the copies, instead of by host bits, so write_into() and
        dense() work unchanged.  rows_per_image as in pack().  -> PackedTargetMasks whose link_bytes count the descriptors, the tables and the
        polygons' tables.  Every capacity of both objects is checked before anything is copied or launched."""
        if len(segmentations_per_image) != len(plans):
            raise ValueError(f"DeviceTargetMasks: {len(segmentations_per_image)} segmentation lists for {len(plans)} plans (at least one)")
        if rows_per_image is not None and len(rows_per_image) != len(plans):
            raise ValueError(f"DeviceTargetMasks: {len(rows_per_image)} row lists for {len(plans)} plans")
        objects, shapes = [], []
        for i, (segs, p) in enumerate(zip(segmentations_per_image, plans)):
            segs = list(segs)
            if rows_per_image is not None:
                segs = [segs[r] for r in self._selected(rows_per_image[i], len(segs), "segmentations").tolist()]
            objects.append(segs)
            shapes.append(np.broadcast_to(_NO_MASK, (len(segs), int(p.height), int(p.width))))          # pack()'s placement reads the shapes only
        packed, rows, tables, bits, used = self._layout(shapes, plans)
        assert used <= self._blob_bytes and packed.slots <= self.max_slots
        flat = [seg for segs in objects for seg in segs]
        layout = polygons._layout(flat, [(r["src_h"], r["src_w"]) for r in rows], [r["src_off"] for r in rows])
        self._write_head(rows, tables)
        head = min((at for at, _ in bits), default=used)       # the descriptors and the tables: the bits behind them are written on the device
        self._stage.upload_head(self.blob, head)
        placed = polygons.pack(flat, None, _layout=layout)
        polygons.rasterise(self.blob)
        self.last = PackedTargetMasks(packed.slots, packed.counts, packed.sizes, head + placed.link_bytes)
        return self.last

    # -- device side --------------------------------------------------------------------------------------------------------------------
    def write_into(self, static_targets):
        """One launch of the batch that pack() placed into static_targets.masks (matcher.StaticTargets(mask_hw=...)): its first PackedTargetMasks.slots
        slots are written completely (zeros outside each mask), the others are left alone."""
        from . import kernels
        out = static_targets.masks
        if out is None:
            raise ValueError("DeviceTargetMasks: the StaticTargets was built without mask_hw")
        slots, Hp, Wp = (int(v) for v in out.shape)
        if slots > self.max_slots:
            raise ValueError(f"DeviceTargetMasks: a StaticTargets of {slots} slots exceeds max_batch * max_targets_per_image = {self.max_slots}")
        if self.last is not None:
            if self.last.slots > slots:
                raise ValueError(f"DeviceTargetMasks: the packed batch has {self.last.slots} targets, the StaticTargets holds {slots}")
            if self.last.slots and any(h > Hp or w > Wp for (h, w), n in zip(self.last.sizes, self.last.counts) if n):
                raise ValueError(f"DeviceTargetMasks: prepared masks of {self.last.sizes} do not fit mask_hw = {Hp} x {Wp}")
        kernels.target_masks(self.blob, self.desc[:slots], self.arena, out)
        return static_targets

    def dense(self, packed):
        """The prepared masks of the batch that pack() returned `packed` for, per image: bool [n_i, h_i, w_i] device tensors, copies cut from an internal
        [max_slots, *max_out_hw] output that the next call overwrites."""
        from . import kernels
        if packed is not self.last:
            raise ValueError("DeviceTargetMasks.dense: `packed` is not the batch of the last pack()")
        if self._dense is None:
            self._dense = torch.zeros(self.max_slots, *self.max_out_hw, dtype=torch.uint8, device=self.device)
        kernels.target_masks(self.blob, self.desc, self.arena, self._dense)
        res, at = [], 0
        for n, (h, w) in zip(packed.counts, packed.sizes):
            res.append(self._dense[at:at + n, :h, :w].to(torch.bool))
            at += n
        return res


# ---- polygon annotations on the device -----------------------------------------------------------------------------------------------------------
POLY_DESC_FIELDS = ("dst_off", "h", "w", "stride_words", "poly_first", "poly_count", "reserved0", "reserved1")
assert len(POLY_DESC_FIELDS) == _lib.POLY_DESC_WORDS and _lib.POLY_REC_WORDS == 2


def polygon_tables(segmentations, sizes, offsets=None):
    """The three int32 tables toist_polygon_masks reads (include/toist_hip.h), in plain numpy: segmentations[i] = the list of flat polygons (x0, y0, x1,
    y1, ...) of object i, sizes[i] = its (h, w); offsets[i] = the byte offset of its packed rows in the destination (default: one object behind the
    other, each h rows of ceil(w / 32) words).  -> (verts int32 [V, 2] on rleFrPoly's 5x grid, int(5.0 * c + .5) in float64 as polygon_to_mask computes
    it; polys int32 [P, 2] = first vertex, vertex count; desc int32 [N, POLY_DESC_WORDS]; trace steps summed over every polygon).  An object of size
    (0, 0) is a dead slot: an all-zero row, nothing is written for it.  Every polygon passes coco_eval.polygon_vertices; raises ValueError otherwise."""
    from .coco_eval import polygon_vertices
    if sizes is None or len(segmentations) != len(sizes):
        raise ValueError(f"polygon_tables: {len(segmentations)} objects for {0 if sizes is None else len(sizes)} sizes")
    if offsets is not None and len(offsets) != len(sizes):
        raise ValueError(f"polygon_tables: {len(offsets)} offsets for {len(sizes)} objects")
    verts, polys, steps, at = [], [], 0, 0
    desc = np.zeros((len(sizes), _lib.POLY_DESC_WORDS), dtype=np.int32)
    n_verts = 0
    for i, (polygons, hw) in enumerate(zip(segmentations, sizes)):
        h, w = int(hw[0]), int(hw[1])
        if h < 0 or w < 0 or (h == 0) != (w == 0):
            raise ValueError(f"polygon_tables: object {i} has the size {h} x {w}")
        polygons = list(polygons)
        if h == 0:
            if polygons:
                raise ValueError(f"polygon_tables: object {i} has polygons and the size 0 x 0 of a dead slot")
            continue
        first = len(polys)
        for poly in polygons:
            xy, n = polygon_vertices(poly)
            verts.append(np.trunc(5.0 * xy + .5).astype(np.int32))          # polygon_vertices has checked that the grid fits int32
            polys.append((n_verts, xy.shape[0]))
            n_verts += xy.shape[0]
            steps += n
        stride = (w + 31) // 32
        off = at if offsets is None else int(offsets[i])
        if off < 0 or off % 4 or off + h * stride * 4 >= 2 ** 31:
            raise ValueError(f"polygon_tables: object {i}: a destination offset of {off} bytes (a non-negative multiple of 4, addressed with 31 bits)")
        desc[i, :6] = (off, h, w, stride, first, len(polys) - first)
        at = off + h * stride * 4
    verts = np.concatenate(verts, axis=0) if verts else np.zeros((0, 2), dtype=np.int32)
    return verts, np.asarray(polys, dtype=np.int32).reshape(-1, 2), desc, steps


@dataclass(frozen=True)
class PackedPolygons:
    """What DevicePolygonMasks.pack() placed: the object slots, their (h, w), the byte offsets of their packed rows, the polygons, vertices and trace
    steps of the batch, the end of the packed destination range and the bytes of the one host-to-device copy."""
    objects: int
    sizes: tuple
    offsets: tuple
    polygons: int
    vertices: int
    trace_steps: int
    packed_bytes: int
    link_bytes: int


class DevicePolygonMasks:
    """The polygon annotations of a batch's objects -> their masks on the device, bit for bit coco_eval.convert_coco_poly_to_mask (every polygon
    maskApi.c's rleFrPoly, an object's polygons merged by union): ONE launch (csrc/poly.hip: toist_polygon_masks).  The host link carries the grid
    vertices, 8 bytes each, instead of masks.
    Owns fixed-address device memory -- one blob: the descriptor table [max_objects, POLY_DESC_WORDS], the polygon records [max_polygons, 2], the vertex
    table [max_vertices, 2] -- and its pinned host image.
      pack(segmentations, sizes, offsets=None) : segmentations[i] = the list of flat polygons of object i, sizes[i] = its (h, w) ((0, 0) = a dead slot);
                              fills the pinned image and issues ONE asynchronous host-to-device copy on the current stream -> PackedPolygons
      rasterise(dst, offsets=None) : one launch into dst (uint8 [bytes] on the device): object i's h rows of ceil(w / 32) words in pack_mask_bits'
                              layout at its offset, every word written, nothing else.  Sizes come from the device only, so the launch can be captured
                              once and replayed after every pack().  `offsets` replaces the offsets pack() placed (one more small copy).
      dense(packed)         : list of bool [h_i, w_i] device tensors;  dense_into(out): the live regions into a uint8 [slots, cap_h, cap_w] of the caller's
    Every capacity (max_objects, max_polygons, max_vertices, max_hw with at most kernels.POLYGON_MAX_ROWS rows, and max_trace_steps = the launch's work,
    the sum over all edges of max(|dx|, |dy|) on the 5x grid: a vertex far outside the image is legal and must not buy unbounded device time) is checked
    on the host and raises ValueError before anything is copied or launched."""

    def __init__(self, device, max_objects, max_polygons, max_vertices, max_hw, max_trace_steps):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DevicePolygonMasks rasterises in GPU memory: there is no CPU path")
        self._set_capacities(max_objects, max_polygons, max_vertices, max_hw, max_trace_steps)
        self.blob = torch.zeros(self._blob_bytes, dtype=torch.uint8, device=self.device)
        words = self.blob.view(torch.int32)
        self.desc = words[:self._polys_at // 4].view(self.max_objects, _lib.POLY_DESC_WORDS)
        self.polys = words[self._polys_at // 4:self._verts_at // 4].view(self.max_polygons, 2)
        self.verts = words[self._verts_at // 4:].view(self.max_vertices, 2)
        self._stage = staging.Staging(torch.zeros(self._blob_bytes, dtype=torch.uint8), self.device)
        self._dense = None                                    # uint8 [max_objects, *max_hw], on the first dense()
        self.last = None                                      # the PackedPolygons of the last pack()
        self._end = 0                                         # where the packed rows end under the offsets the device holds

    def _set_capacities(self, max_objects, max_polygons, max_vertices, max_hw, max_trace_steps):
        """The capacities and the byte layout they imply (host only)."""
        self.max_objects, self.max_polygons, self.max_vertices = int(max_objects), int(max_polygons), int(max_vertices)
        self.max_hw, self.max_trace_steps = (int(max_hw[0]), int(max_hw[1])), int(max_trace_steps)
        if min(self.max_objects, self.max_polygons, self.max_vertices, self.max_trace_steps, *self.max_hw) <= 0:
            raise ValueError("DevicePolygonMasks: capacities must be positive")
        if self.max_hw[0] > _lib.POLY_MAX_ROWS:
            raise ValueError(f"DevicePolygonMasks: images of {self.max_hw[0]} rows: the kernel's plane holds {_lib.POLY_MAX_ROWS}")
        self._polys_at = self.max_objects * _lib.POLY_DESC_WORDS * 4
        self._verts_at = self._polys_at + self.max_polygons * 8
        self._blob_bytes = self._verts_at + self.max_vertices * 8
        if self.max_objects > 65535 or self._blob_bytes >= 2 ** 31:
            raise ValueError("DevicePolygonMasks: at most 65535 objects, and the blob is addressed with 31 bits")

    # -- host side ----------------------------------------------------------------------------------------------------------------------
    def _layout(self, segmentations, sizes, offsets=None):
        """Host check + tables of a batch: -> (PackedPolygons, verts, polys, desc).  Raises ValueError on an invalid polygon and on any capacity
        overrun; touches no buffer."""
        verts, polys, desc, steps = polygon_tables(segmentations, sizes, offsets)
        for what, n, cap in (("objects", desc.shape[0], self.max_objects), ("polygons", polys.shape[0], self.max_polygons),
                             ("vertices", verts.shape[0], self.max_vertices), ("trace steps", steps, self.max_trace_steps)):
            if n > cap:
                raise ValueError(f"DevicePolygonMasks: {n} {what} exceed max_{what.replace(' ', '_')} = {cap}")
        if desc.shape[0] and (desc[:, 1].max() > self.max_hw[0] or desc[:, 2].max() > self.max_hw[1]):
            raise ValueError(f"DevicePolygonMasks: an image of {int(desc[:, 1].max())} x {int(desc[:, 2].max())} exceeds max_hw = {self.max_hw[0]} x {self.max_hw[1]}")
        ends = desc[:, 0].astype(np.int64) + desc[:, 1].astype(np.int64) * desc[:, 3] * 4
        packed = PackedPolygons(desc.shape[0], tuple((int(r[1]), int(r[2])) for r in desc), tuple(int(r[0]) for r in desc), polys.shape[0], verts.shape[0],
                                steps, int(ends.max()) if ends.size else 0, self._verts_at + verts.shape[0] * 8)
        return packed, verts, polys, desc

    def pack(self, segmentations, sizes, offsets=None, _layout=None):
        """The batch into the blob: descriptors, polygon records and grid vertices into the pinned image, then one asynchronous copy of its used head
        on the current stream (the previous copy out of the pinned image is waited for first).  -> PackedPolygons."""
        packed, verts, polys, desc = _layout if _layout is not None else self._layout(segmentations, sizes, offsets)
        host = self._stage.open_np().view(np.int32)
        table = host[:self._polys_at // 4].reshape(self.max_objects, _lib.POLY_DESC_WORDS)
        table[:] = 0                                            # slots behind the batch's objects: h = 0 = dead, not written
        table[:desc.shape[0]] = desc
        host[self._polys_at // 4:self._polys_at // 4 + polys.size] = polys.reshape(-1)
        host[self._verts_at // 4:self._verts_at // 4 + verts.size] = verts.reshape(-1)
        self._stage.upload_head(self.blob, packed.link_bytes)
        self.last, self._end = packed, packed.packed_bytes
        return packed

    # -- device side --------------------------------------------------------------------------------------------------------------------
    def rasterise(self, dst, offsets=None):
        """One launch of the batch that pack() placed into dst, uint8 [bytes] on the device (see the class)."""
        from . import kernels
        if self.last is None:
            raise ValueError("DevicePolygonMasks.rasterise: nothing is packed")
        if not torch.is_tensor(dst) or dst.dtype != torch.uint8 or dst.dim() != 1 or not dst.is_contiguous() or dst.device != self.blob.device:
            raise ValueError("DevicePolygonMasks.rasterise: the destination is a contiguous uint8 [bytes] tensor on the rasteriser's device")
        end = self._end
        if offsets is not None:
            offsets = tuple(int(o) for o in offsets)
            if len(offsets) != self.last.objects or any(o < 0 or o % 4 for o in offsets):
                raise ValueError(f"DevicePolygonMasks.rasterise: {len(offsets)} offsets for {self.last.objects} objects (non-negative multiples of 4)")
            end = max((o + h * ((w + 31) // 32) * 4 for o, (h, w) in zip(offsets, self.last.sizes) if h), default=0)
            if end >= 2 ** 31:
                raise ValueError("DevicePolygonMasks.rasterise: the destination is addressed with 31 bits")
        if end > dst.numel():
            raise ValueError(f"DevicePolygonMasks.rasterise: the packed masks end at byte {end}, the destination holds {dst.numel()}")
        if offsets is not None:
            table = self._stage.open_np().view(np.int32)[:self._polys_at // 4].reshape(self.max_objects, _lib.POLY_DESC_WORDS)
            table[:self.last.objects, 0] = [o if h else 0 for o, (h, _) in zip(offsets, self.last.sizes)]
            self._stage.upload_head(self.blob, self._polys_at)
            self._end = end
        kernels.polygon_masks(self.desc, self.polys, self.verts, dst, cap_hw=self.max_hw)
        return dst

    def dense_into(self, out):
        """One launch of the batch that pack() placed into `out`, uint8 (or bool) [slots, cap_h, cap_w] of the caller's: the live h x w region of
        every slot is written completely (0 / 1), the rest is left alone."""
        from . import kernels
        if self.last is None:
            raise ValueError("DevicePolygonMasks.dense_into: nothing is packed")
        if out.dim() != 3 or out.shape[0] > self.max_objects or out.shape[0] < self.last.objects:
            raise ValueError(f"DevicePolygonMasks.dense_into: an output of {tuple(out.shape)} for {self.last.objects} objects (max_objects {self.max_objects})")
        if any(h > out.shape[1] or w > out.shape[2] for h, w in self.last.sizes):
            raise ValueError(f"DevicePolygonMasks.dense_into: masks of {self.last.sizes} do not fit {int(out.shape[1])} x {int(out.shape[2])}")
        kernels.polygon_masks(self.desc[:out.shape[0]], self.polys, self.verts, out)
        return out

    def dense(self, packed):
        """The masks of the batch that pack() returned `packed` for: bool [h_i, w_i] device tensors, copies cut from an internal [max_objects, *max_hw]
        output that the next call overwrites."""
        if packed is not self.last:
            raise ValueError("DevicePolygonMasks.dense: `packed` is not the batch of the last pack()")
        if self._dense is None:
            self._dense = torch.zeros(self.max_objects, *self.max_hw, dtype=torch.uint8, device=self.device)
        self.dense_into(self._dense)
        return [self._dense[i, :h, :w].to(torch.bool) for i, (h, w) in enumerate(packed.sizes)]
