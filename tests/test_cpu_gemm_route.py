"""The bf16 GEMM dispatcher (csrc/gemm_route.cpp) against tests/golden/gemm_routes.npz: what the library answered, descriptor by descriptor
of tests/gemm_route_cases.py, before the routing moved into its own host-only unit (tests/golden/make_golden_gemm_routes.py).

Nothing here calls toist_gemm_bf16: the descriptors hold made-up addresses.  The library is asked its two queries; check + route run in a
stand-alone program that links csrc/gemm_route.cpp alone, once plain and once under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gemm_route_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES, CONV3, PANEL, G128, G128W, G256W = range(6)      # gemm_family of csrc/gemm_route.h
FAMILY_OF_TILE = {131: CONV3, 135: PANEL, 136: G128, 137: G128W, 138: G256W}
POST_NONE, POST_REDUCE, POST_EPILOGUE, POST_DEFERRED = range(4)
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def cases():
    return gemm_route_cases.cases()


@pytest.fixture(scope="module")
def table(cases):
    t = dict(np.load(os.path.join(ROOT, "tests", "golden", "gemm_routes.npz")))
    assert str(t["digest"]) == gemm_route_cases.digest(cases), "tests/gemm_route_cases.py changed: the golden table no longer describes its cases"
    assert len(t["pick"]) == len(cases)
    return t


def test_table_covers_the_dispatcher(table):
    """every tile code and refusal the table was asked to hold is in it"""
    accepted = table["rc"] == -2
    assert set(table["pick"][accepted].tolist()) >= {64, 65, 128, 129, 130, 131, 132, 133, 134, 135, 136, 137, 138}
    assert {1, 2, 4, 8, 16} <= set(table["split"].tolist()) and int(table["split"].max()) > 16
    assert set(table["family"][accepted].tolist()) == {TILES, CONV3, PANEL, G128, G128W, G256W}
    for needle in ("bad shape", "null operand", "16-byte aligned", "batch strides", "source channels", "conv geometry", "leading dimension", "CONVX needs",
                   "A_KROW needs", "B_KROW needs", "needs an f32 output", "TOIST_GEMM_SPLIT_EPILOGUE needs", "a_colsum needs", "TOIST_GEMM_COLSUM_SLICES needs",
                   "a grouped launch", "split_k only supports", "split_k needs a workspace", "needs aux", "a2 needs", "bad dropout p",
                   "the 128x128 kernel does not", "the 3x3 halo kernel does not", "the short-K panel kernel does not", "the 128x128 weight-gradient kernel does not",
                   "the 256x128 weight-gradient kernel does not", "clamps to 1", "kin % 8 != 0", "bad tile code", "unsupported operand kinds"):
        assert any(needle in m for m in table["messages"].tolist()), needle
    # the cases where toist_gemm_pick_tile did not report the family toist_gemm_bf16 launched: ring word on tile 0, batch_inner = 0
    assert int(table["marked"].sum()) == 7


def test_library_queries_equal_the_table(cases, table):
    from toist_amd import _lib
    lib = _lib.lib()
    pick = np.array([lib.toist_gemm_pick_tile(ctypes.byref(d)) for _, d in cases])
    split = np.array([lib.toist_gemm_effective_split(ctypes.byref(d)) for _, d in cases])
    marked = table["marked"] != 0
    bad = np.nonzero((pick != table["pick"]) & ~marked)[0]
    assert bad.size == 0, [(cases[i][0], int(pick[i]), int(table["pick"][i])) for i in bad[:10]]
    for i in np.nonzero(marked)[0]:       # there the launch is the reference: the query now reports a tile of the family it reached
        assert FAMILY_OF_TILE.get(int(pick[i]), TILES) == table["family"][i], cases[i][0]
    bad = np.nonzero(split != table["split"])[0]
    assert bad.size == 0, [(cases[i][0], int(split[i]), int(table["split"][i])) for i in bad[:10]]


def _build(tmp_path, cxx, flags, tag):
    exe = tmp_path / f"gemm_route_{tag}"
    subprocess.check_call([cxx, "-std=c++17", *flags, os.path.join(ROOT, "tests", "gemm_route_main.cpp"),
                           os.path.join(ROOT, "toist_amd", "csrc", "gemm_route.cpp"), "-o", str(exe)])
    return exe


def _sanitizers_link(tmp_path):
    src = tmp_path / "one.cpp"
    src.write_text("int main() { return 0; }\n")
    return subprocess.call(["g++", *SANITIZE, str(src), "-o", str(tmp_path / "one")], stderr=subprocess.DEVNULL) == 0


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan_ubsan"])
def test_standalone_check_and_route_equal_the_table(cases, table, tmp_path, sanitized):
    if sanitized and not _sanitizers_link(tmp_path):
        pytest.skip("g++ cannot link a one-line program with -fsanitize=address,undefined on this machine")
    exe = _build(tmp_path, "g++", SANITIZE if sanitized else ["-O1"], "san" if sanitized else "plain")
    raw = tmp_path / "descs.bin"
    raw.write_bytes(gemm_route_cases.raw(cases))
    lines = subprocess.check_output([str(exe), str(raw)], text=True).splitlines()
    assert len(lines) == len(cases)
    messages = table["messages"].tolist()
    for i, ((name, d), line) in enumerate(zip(cases, lines)):
        plan, ws_split, queries, msg = line.split(" | ", 3)
        code, family, tile, ring, split, post = map(int, plan.split())
        q_pick, q_split = map(int, queries.split())
        want_pick, want_split = int(table["pick"][i]), int(table["split"][i])
        assert (q_pick, q_split) == (tile, int(ws_split)), name           # the entry points are the route
        assert q_split == want_split, name
        if table["rc"][i] == -1:
            assert (code, msg) == (-1, messages[table["msg_idx"][i]]), name
            assert tile == want_pick, name
            continue
        assert (code, msg) == (0, ""), (name, msg)
        if table["marked"][i]:
            assert family == table["family"][i], name
        else:
            assert tile == want_pick, name
        assert family == FAMILY_OF_TILE.get(tile, TILES) == table["family"][i], name
        assert split == want_split, name                                   # a checked call with k-slices has its workspace
        want_post = POST_NONE if split <= 1 else POST_DEFERRED if d.flags & gemm_route_cases.DEFER else \
            POST_EPILOGUE if d.flags & gemm_route_cases.SPLIT_EPI else POST_REDUCE
        assert post == want_post, name
        if family == PANEL:
            first_gen = d.tile >> 8 == 1 or d.M * d.ldc >= 1 << 30           # variant 1, or beyond panel2_kernel's byte offsets
            assert ring == (1 if first_gen else 0 if d.tile >> 8 in (0, 255) else d.tile >> 8), name
        else:
            assert ring == d.tile >> 8, name


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan_ubsan"])
def test_standalone_answers_what_the_table_cannot_hold(tmp_path, sanitized):
    """K <= 0: refused as a bad shape; both queries still answer (one k-slice, the forced or a generic tile) without a division by zero"""
    if sanitized and not _sanitizers_link(tmp_path):
        pytest.skip("g++ cannot link a one-line program with -fsanitize=address,undefined on this machine")
    extra = gemm_route_cases.unrecorded()
    exe = _build(tmp_path, "g++", SANITIZE if sanitized else ["-O1"], "san" if sanitized else "plain")
    raw = tmp_path / "descs.bin"
    raw.write_bytes(gemm_route_cases.raw(extra))
    lines = subprocess.check_output([str(exe), str(raw)], text=True).splitlines()
    assert len(lines) == len(extra)
    for (name, d), line in zip(extra, lines):
        plan, ws_split, queries, msg = line.split(" | ", 3)
        code, family, tile, ring, split, post = map(int, plan.split())
        assert (code, msg) == (-1, f"toist_gemm_bf16: bad shape M={d.M} N={d.N} K={d.K}"), name
        assert tile == (d.tile or 64) and (split, int(ws_split), post) == (1, 1, POST_NONE), name
        assert queries.split() == [str(tile), "1"], name
