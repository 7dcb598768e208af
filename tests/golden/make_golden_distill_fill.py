"""Golden vectors of the memory banks' FILL phase and of the FIFO policy from the REAL reference (/root/reference/models/mdetr.py:62-103,
213-234 and models/kmeans.py:8-18): ClusterCriterion.update_memory_queue and memory_cluster, called in the order update_memory / forward call them
(queue update; teacher images with boxes in batch order; every student image in batch order), from a FRESH criterion (full_label == 0) under a
fixed np.random.seed, until one task has crossed update_count > memory_size and taken nearest replacement; then a second sequence with
fifo_memory=True on full banks.  Same stubs as make_golden_distill.py (`.cuda()` and the process-group calls neutralised; the arithmetic is the
reference's).  Every np.random.choice result is recorded in call order.  Runs only in the build container (CPU).
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_distill_fill.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import formula  # noqa: E402
from transformers import RobertaModel  # noqa: E402,F401  (before the stubs)

STUBS = "/tmp/toist_ref_stubs"
for rel, text in {"IPython/__init__.py": "def embed(*a, **k):\n    pass\n", "torchvision/__init__.py": "from . import ops, models\n",
                  "torchvision/ops/__init__.py": "from . import boxes\n",
                  "torchvision/ops/boxes.py": "def box_area(b):\n    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])\n",
                  "torchvision/models/__init__.py": "from . import _utils\n", "torchvision/models/_utils.py": "class IntermediateLayerGetter:\n    pass\n",
                  "timm/__init__.py": "from . import models\n", "timm/models/__init__.py": "def create_model(*a, **k):\n    raise RuntimeError('stub')\n"}.items():
    path = os.path.join(STUBS, rel)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "w").write(text)
sys.dont_write_bytecode = True
sys.path[:0] = [STUBS, "/root/reference"]
from models.mdetr import ClusterCriterion  # noqa: E402

D, N, K, B, T = 16, 24, 3, 2, 4
SEED = {"A": 20, "B": 21}
# per step: (teacher tasks, -1 = an image without boxes), (student tasks).  Sequence A pushes task 2 past update_count > N (two images of one task, two
# tasks, a -1 row), through the flip step (count 26 > 24 seen before the add: still FIFO) and into nearest replacement; tasks 0, 1, 3 keep filling.
STEPS_A = [((2, 2), (2, 2)), ((2, 1), (1, 2)), ((2, -1), (2, 3))] + [((2, 2), s) for s in [(3, 3), (0, 2), (2, 2), (1, 2), (2, 3)] * 2] + \
          [((2, 2), (2, 1)), ((2, 2), (2, 2)), ((2, 2), (3, 2)), ((2, 1), (2, 1)), ((-1, 2), (0, 2))]
STEPS_B = [((1, 1), (1, 3)), ((0, 3), (3, 0)), ((-1, 2), (2, 2))]


def blobs(name, shape_rows, task):
    """rows around three well separated points per task (k-means on them does not hang on the last bits of a distance)"""
    centre = formula.tensor(f"fill.blob{task}", (3, D), 8.0)
    n = int(np.prod(shape_rows))
    which = (formula.unit(name + ".which", n) * 3 + 1.5).astype(np.int64).clip(0, 2)
    return (centre[torch.from_numpy(which)] + formula.tensor(name + ".noise", (n, D), 0.6)).reshape(*shape_rows, D)


def run(tag, steps, fifo, full):
    args = types.SimpleNamespace(train_batch_size=B, fifo_memory=fifo)
    cc = ClusterCriterion(feature_dim=D, memory_size=N, cluster_num=K, task_count=T, args=args)
    cc.feature_bank.copy_(torch.stack([blobs(f"fill.{tag}.bank{t}", (N,), t) for t in range(T)]))
    cc.cluster_centers.copy_(formula.tensor(f"fill.{tag}.centers", (T, K, D), 8.0))
    if full:
        cc.full_label.fill_(1)
        cc.update_count.fill_(100)
    out = {"bank0": cc.feature_bank.clone(), "centers0": cc.cluster_centers.clone(), "seed": np.int64(SEED[tag]), "fifo_memory": np.int64(fifo)}
    keys = ["rows", "tasks_noun", "feats_sth", "tasks_sth", "bank", "centers_teacher", "centers", "update_count", "full_label", "pick_noun", "pick_sth"]
    rec = {k: [] for k in keys}
    draws, draw_step = [], []
    real_choice = np.random.choice
    step_now = [0]

    def choice(*a, **k):
        got = real_choice(*a, **k)
        draws.append(np.asarray(got, dtype=np.int32))
        draw_step.append(step_now[0])
        return got
    np.random.choice = choice
    np.random.seed(SEED[tag])
    try:
        for s, (tn, ts) in enumerate(steps):
            step_now[0] = s
            rows = torch.stack([blobs(f"fill.{tag}.row{s}.{i}", (), max(t, 0)) if t >= 0 else torch.zeros(D) for i, t in enumerate(tn)])
            feats = torch.stack([blobs(f"fill.{tag}.sth{s}.{i}", (), t) for i, t in enumerate(ts)])
            cc.update_memory_queue(torch.cat([rows, torch.tensor(tn, dtype=torch.float32)[:, None]], dim=1))
            pn = [int(cc.memory_cluster(rows[i].clone(), t)[0]) if t >= 0 else -1 for i, t in enumerate(tn)]
            rec["centers_teacher"].append(cc.cluster_centers.clone())
            ps = [int(cc.memory_cluster(feats[i].clone(), t)[0]) for i, t in enumerate(ts)]
            for k, v in zip(keys, [rows, torch.tensor(tn), feats, torch.tensor(ts), cc.feature_bank.clone(), None, cc.cluster_centers.clone(),
                                   cc.update_count.clone(), cc.full_label.clone(), torch.tensor(pn), torch.tensor(ps)]):
                if v is not None:
                    rec[k].append(v)
    finally:
        np.random.choice = real_choice
    out.update({k: torch.stack(v) for k, v in rec.items()})
    out["draws"] = np.stack(draws) if draws else np.zeros((0, K), dtype=np.int32)
    out["draw_step"] = np.asarray(draw_step, dtype=np.int32)
    print(tag, "steps", len(steps), "draws", len(draws), "update_count", cc.update_count.tolist(), "full_label", cc.full_label.tolist())
    return {f"{tag}.{k}": (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.distributed.get_world_size = lambda *a, **k: 1
    torch.distributed.all_gather = lambda lst, t, *a, **k: lst[0].copy_(t)
    out = run("A", STEPS_A, fifo=False, full=False)
    out.update(run("B", STEPS_B, fifo=True, full=True))
    path = os.path.join(HERE, "distill_fill.npz")
    np.savez_compressed(path, **out)
    print("wrote distill_fill.npz", len(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
