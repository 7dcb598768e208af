"""fp64 reference of the prototype choice of a task sweep (toist_sweep_prototypes) and the seeded inputs of its tests, shared by
tests/test_cpu_sweep_choice.py (which holds the inputs to the margin condition below) and tests/test_gpu_zz_zzzzz_sweep_choice_kernel.py.  Not a
conftest and not a test.

The reference takes the tensors the kernel takes (on the CPU) and computes in fp64: every pair's feature, the sequential k-means per task through
oracle.distill_ref.kmeans in ascending pair order (a task's later pair starts from the centres its earlier pair left), the picks, the rows of
memory_mod that receive a prototype, and two margins with the bound each has to clear for the fp32 kernel to decide as the fp64 reference does:

  pair margin   second-best minus best squared distance of the pair's feature to its task's final centres.  The kernel's distances are fp32 sums of
                D squares of fp32 differences: each term carries three roundings (difference, square, add), the sum D - 1 more, so for any order
                |fl(d_k) - d_k| <= (D + 4) 2^-24 d_k to first order -- rounding_bounds.acc_term(D + 2, d_k).  Its arguments are perturbed too: the
                feature by its own fp32 error e_f (feature_bound: n products rounded, n - 1 additions -- acc_term(n, sum |w||x|), n = the span's
                tokens), a centre by e_c = acc_term(N, |c|), the fp32 mean of at most N bank rows in any order (given equal assignments: the bank
                margin).  d_k moves by at most 2 sum_d |f_d - c_kd| (e_f,d + e_c,kd) + sum_d (e_f,d + e_c,kd)^2.  The pick is the reference's when
                margin > bound(best) + bound(second best).
  bank margin   the same for every bank row against the centres of every Lloyd iteration's assignment, with e_f = 0 (a bank row is an input).
None of the terms is tuned; the inputs are built so that the margins clear them by orders of magnitude (well separated blobs)."""
import torch

from oracle import distill_ref
from rounding_bounds import F64, acc_term

BF16 = torch.bfloat16
P, LIVE, HW, D, K, N = 7, 5, 4, 256, 3, 32
N_TASKS = 6                                                       # tasks of the criterion; the captions use two of them
CAPTIONS = ["take the something over", "sits something", "something to dig with"]      # 'something' starts on a token boundary in each
DATASET_NAMES = ["task_3_train.json", "task_5_train.json", "task_3_train.json"]      # captions 0 and 2 share task 2
CHARS_PER_TOKEN = [9, 5, 4]                                       # 'something' (9 characters) spans 1, 2 and 3 tokens
PAIR_CAPTION = [0, 1, 2, 1, 0, 0, 0]                              # task 2 serves pairs 0, 2, 4 -- not contiguous; pairs 5, 6 are padding


class Tokens(dict):
    """T tokenized captions that answer char_to_token: caption t has CHARS_PER_TOKEN[t] characters per token behind the <s> token."""

    def __init__(self, L):
        super().__init__(input_ids=torch.zeros(len(CAPTIONS), L, dtype=torch.int64), attention_mask=torch.ones(len(CAPTIONS), L, dtype=torch.int64))

    def char_to_token(self, row, char):
        t = char // CHARS_PER_TOKEN[row] + 1
        return t if t < self["input_ids"].shape[1] - 1 else None


def spans(L):
    """the token positions of 'something' per caption"""
    tok = Tokens(L)
    out = []
    for t, c in enumerate(CAPTIONS):
        beg = c.find("something")
        out.append(list(range(tok.char_to_token(t, beg), tok.char_to_token(t, beg + 8) + 1)))
    return out


def inputs(L, seed=0):
    """Seeded inputs: banks of three well separated blobs per task, centres near the blob means, a memory whose 'something' rows sit near one blob of
    the pair's task (so every pair has a clear nearest prototype) and random rows elsewhere.  -> dict of CPU tensors."""
    g = torch.Generator().manual_seed(1000 + 17 * L + seed)
    S = HW + L
    means = torch.randn(N_TASKS, K, D, generator=g) * 2.0
    which = torch.arange(N) % K
    banks = means[:, which, :] + 0.25 * torch.randn(N_TASKS, N, D, generator=g)
    centers = means + 0.5 * torch.randn(N_TASKS, K, D, generator=g)
    memory = torch.randn(P, S, D, generator=g)
    tasks = [int(n.split("_")[1]) - 1 for n in DATASET_NAMES]
    sp = spans(L)
    for p, c in enumerate(PAIR_CAPTION):
        blob = (p * 2 + 1) % K
        for l in sp[c]:
            memory[p, HW + l] = means[tasks[c], blob] + 0.3 * torch.randn(D, generator=g)
    return {"memory": memory.to(BF16), "banks": banks.contiguous(), "centers": centers.contiguous(), "pair_caption": torch.tensor(PAIR_CAPTION, dtype=torch.int32),
            "tasks": tasks, "spans": sp, "L": L}


def feature_ref(W, text):
    """W f32 [L], text bf16 [L, D] -> (feature fp64 [D], bound fp64 [D]) of the fp32 weighted sum in any order of its n nonzero terms"""
    terms = W.to(F64).unsqueeze(-1) * text.to(F64)
    n = int((W != 0).sum())
    return terms.sum(0), acc_term(n, terms.abs().sum(0))


def _dist_bound(x, e_x, c, e_c):
    """bound on |fl(d_k) - d_k| for d_k = sum_d (x_d - c_kd)^2 evaluated in fp32 on arguments within e_x / e_c of x / c  (module docstring)"""
    diff = (x.unsqueeze(0) - c).abs()
    d = (diff ** 2).sum(-1)
    e = e_x.unsqueeze(0) + e_c
    return acc_term(D + 2, d) + (2 * diff * e).sum(-1) + (e ** 2).sum(-1)


def _margin(d, bound):
    """(second best - best, bound(best) + bound(second best)) of a row of squared distances"""
    order = torch.argsort(d)
    return float(d[order[1]] - d[order[0]]), float(bound[order[0]] + bound[order[1]])


def _kmeans_bank_margin(X, centers, tol=1e-4):
    """distill_ref.kmeans' loop once more, looking at every iteration's assignment: the smallest (margin - bound) over the bank rows"""
    worst = float("inf")
    centers = centers.clone()
    while True:
        e_c = acc_term(N, centers.abs())
        d = ((X.unsqueeze(1) - centers.unsqueeze(0)) ** 2.0).sum(-1)
        for n in range(X.shape[0]):
            m, b = _margin(d[n], _dist_bound(X[n], torch.zeros(D, dtype=F64), centers, e_c))
            worst = min(worst, m - b)
        choice = d.argmin(1)
        prev = centers.clone()
        for c in range(centers.shape[0]):
            sel = X[choice == c]
            if len(sel):
                centers[c] = sel.mean(0)
        if float(torch.sqrt(((centers - prev) ** 2).sum(1)).sum()) ** 2 < tol:
            return worst


def reference(t, W, sub, live=LIVE):
    """t: inputs(); W f32 [T, L], sub u8 [T, L] (SweepChoiceTables' views) -> dict: features / feature_bound fp64 [P, D] (rows of padding pairs: NaN),
    picks (list, None for padding), centers fp64 [N_TASKS, K, D] after the walk, chosen fp64 [P, D], rows bool [P, L] (the rows of memory_mod that
    receive the pair's prototype), margins [(margin, bound)] per live pair, bank_slack = min over every k-means call of (margin - bound)."""
    L = t["L"]
    text = t["memory"][:, HW:]
    banks, centers = t["banks"].to(F64), t["centers"].to(F64).clone()
    out = {"features": torch.full((P, D), float("nan"), dtype=F64), "feature_bound": torch.full((P, D), float("nan"), dtype=F64), "picks": [None] * P,
           "chosen": torch.full((P, D), float("nan"), dtype=F64), "rows": torch.zeros(P, L, dtype=torch.bool), "margins": [], "bank_slack": float("inf")}
    for p in range(live):
        c = int(t["pair_caption"][p])
        task = t["tasks"][c]
        f, fb = feature_ref(W[c], text[p])
        out["bank_slack"] = min(out["bank_slack"], _kmeans_bank_margin(banks[task], centers[task]))
        _, centers[task] = distill_ref.kmeans(banks[task], centers[task], K)
        d = ((f.unsqueeze(0) - centers[task]) ** 2).sum(-1)
        pick = int(d.argmin())
        out["margins"].append(_margin(d, _dist_bound(f, fb, centers[task], acc_term(N, centers[task].abs()))))
        out["features"][p], out["feature_bound"][p], out["picks"][p], out["chosen"][p] = f, fb, pick, centers[task][pick]
        out["rows"][p] = sub[c].bool()
    out["centers"] = centers
    return out
