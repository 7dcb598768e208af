"""Writes tests/golden/gemm_routes.npz: what the library answers for every descriptor of tests/gemm_route_cases.py.

Run once, at the commit whose dispatcher is the reference (the parent of the routing refactor), on a machine WITHOUT a GPU:

    python tests/golden/make_golden_gemm_routes.py            (TOIST_HIP_LIB may name that commit's build)

Per case it records toist_gemm_pick_tile, toist_gemm_effective_split and the outcome of toist_gemm_bf16(desc, NULL): refused (TOIST_EINVAL)
with its message, or accepted -- which, with no device, ends in TOIST_EHIP with a message that names the kernel family the call reached.
toist_gemm_bf16 gets made-up addresses here, which is only harmless where nothing can launch: the script stops before its first library
call when a device is visible.  Where the family toist_gemm_bf16 reached is not the family of the tile toist_gemm_pick_tile reported, the
case is marked: the launch is the reference there."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

TILES, CONV3, PANEL, G128, G128W, G256W = range(6)      # gemm_family of csrc/gemm_route.h
FAMILY_OF_TILE = {131: CONV3, 135: PANEL, 136: G128, 137: G128W, 138: G256W}


def family_of_message(msg):
    for words, fam in ((("256x128 weight-gradient",), G256W), (("128x128 weight-gradient",), G128W), (("128x128 kernel", "(gemm128)"), G128),
                       (("3x3 kernel", "(conv3)"), CONV3), (("panel kernel", "(panel)"), PANEL)):
        if any(w in msg for w in words):
            return fam
    return TILES


def main():
    import torch
    if torch.cuda.is_available() or torch.cuda.device_count() > 0 or os.path.exists("/dev/kfd") or os.path.exists("/dev/dri/renderD128"):
        sys.exit("a GPU is visible: this script calls toist_gemm_bf16 with made-up addresses and runs only where nothing can launch")
    import ctypes
    import gemm_route_cases
    from toist_amd import _lib
    cases = gemm_route_cases.cases()
    lib = _lib.lib()
    n = len(cases)
    pick, split, rc, family, msg_idx, marked = (np.zeros(n, np.int16) for _ in range(6))
    messages = []
    for i, (name, d) in enumerate(cases):
        pick[i] = lib.toist_gemm_pick_tile(ctypes.byref(d))
        split[i] = lib.toist_gemm_effective_split(ctypes.byref(d))
        rc[i] = lib.toist_gemm_bf16(ctypes.byref(d), None)
        msg = _lib.last_error()
        assert rc[i] in (-1, -2), (name, rc[i], msg)
        if rc[i] == -1:
            if msg not in messages:
                messages.append(msg)
            msg_idx[i], family[i] = messages.index(msg), -1
        else:
            msg_idx[i], family[i] = -1, family_of_message(msg)
            if family[i] != FAMILY_OF_TILE.get(int(pick[i]), TILES):
                marked[i] = 1
                print(f"DISAGREE {name}: pick_tile {pick[i]}, toist_gemm_bf16 reached family {family[i]} ({msg})")
    out = os.path.join(ROOT, "tests", "golden", "gemm_routes.npz")
    np.savez_compressed(out, pick=pick.astype(np.uint8), split=split.astype(np.uint8), rc=rc.astype(np.int8), family=family.astype(np.int8),
                        msg_idx=msg_idx.astype(np.int8), marked=marked.astype(np.uint8), messages=np.array(messages), digest=np.array(gemm_route_cases.digest(cases)))
    print(f"{n} cases, {int((rc == -1).sum())} refused with {len(messages)} distinct messages, {int(marked.sum())} marked; tiles {sorted(set(pick.tolist()))}, "
          f"splits {sorted(set(split.tolist()))}; {os.path.getsize(out)} bytes -> {out}")
    for m in messages:
        print("  ", m)


if __name__ == "__main__":
    main()
