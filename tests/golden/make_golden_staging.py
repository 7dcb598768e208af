"""The packed host images of the host-built device tables -- matcher.StaticTargets.pack, LiveStaticTargets.pack, distill.DistillTables.pack and pack_eval --
for one small batch each (B = 2, at most 3 targets, K = 8, L = 7), with the inputs they were packed from.  staging.npz was recorded with the tables'
own hand-written layouts, before they moved onto toist_amd/staging.py: tests/test_cpu_staging.py packs the same inputs and wants the same bytes.  The
objects are built field by field with plain host buffers, so the script needs no GPU runtime and runs at either side of that move.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_staging.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

B, PER, Q, K, L = 2, 3, 5, 8, 7
LIVE_TOKENS = 6
NOUN_CAPTION, STH_CAPTION = "use the scissors to c", "use the something to"        # 4 characters per token (harness.SyntheticCaptions), L - 2 of them
DATASETS = ("task_3_train.json", "task_1_train.json")
SIZES_TARGETS, SIZES_TABLES = (2, 1), (3, 0)                                     # targets per image: of the StaticTargets batch, of the DistillTables batch


def inputs():
    g = torch.Generator().manual_seed(20)
    tot = sum(SIZES_TARGETS)
    return {"boxes": torch.rand(tot, 4, generator=g), "positive_map": torch.rand(tot, K, generator=g),
            "token_masks": torch.tensor([[6, 0, 0, 0], [1, 0, 0, 0], [1 << 40, 0, 0, 1 << 62]], dtype=torch.int64),
            "table_boxes": torch.rand(sum(SIZES_TABLES), 4, generator=g)}


def tokenized():
    from toist_amd.harness import SyntheticCaptions
    ids = torch.arange(B * L, dtype=torch.int64).view(B, L) + 3
    return SyntheticCaptions({"input_ids": ids, "attention_mask": torch.ones(B, L, dtype=torch.int64)})


def batches(inp):
    """-> (targets of the StaticTargets batch, targets of the DistillTables batch): lists of dicts as the packers take them."""
    at, targets = 0, []
    for n in SIZES_TARGETS:
        targets.append({"boxes": inp["boxes"][at:at + n]})
        at += n
    at, tables = 0, []
    for n, name in zip(SIZES_TABLES, DATASETS):
        tables.append({"boxes": inp["table_boxes"][at:at + n], "dataset_name": name, "noun_tokens_positive": [[(8, 16)] for _ in range(n)]})
        at += n
    return targets, tables


def main():
    from toist_amd.distill import DistillTables
    from toist_amd.matcher import LiveStaticTargets, StaticTargets
    inp = inputs()
    targets, tables = batches(inp)
    views, total = StaticTargets.arena_views(B, B * PER, K)

    def host_only(cls):
        st = cls.__new__(cls)
        st.B, st.max_per_image, st.Q, st.K, st.mask_hw, st.cap = B, PER, Q, K, None, B * PER
        st._views, st._live_off = views, total
        return st
    out = {k: v.numpy() for k, v in inp.items()}
    out["static"] = host_only(StaticTargets).pack(targets, inp["positive_map"], inp["token_masks"], out=torch.zeros(total, dtype=torch.uint8))[0].numpy()
    out["live"] = host_only(LiveStaticTargets).pack(targets, inp["positive_map"], inp["token_masks"], out=torch.zeros(total + 16, dtype=torch.uint8),
                                                    live_tokens=LIVE_TOKENS)[0].numpy()
    tok = tokenized()
    out["distill_noun"] = DistillTables(B, L, "cpu", pronoun_side=False).pack(tok, tables, [NOUN_CAPTION] * B).numpy().copy()
    out["distill_sth"] = DistillTables(B, L, "cpu", pronoun_side=True).pack(tok, tables, [STH_CAPTION] * B).numpy().copy()
    out["distill_eval"] = DistillTables(B, L, "cpu", pronoun_side=True).pack_eval(tok, [STH_CAPTION] * B, list(DATASETS)).numpy().copy()
    path = os.path.join(HERE, "staging.npz")
    np.savez_compressed(path, **out)
    print("wrote staging.npz", {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
