"""The argument checks of toist_conv_pair_bf16 (csrc/gemm_route.cpp pair_check / pair_applies) in a stand-alone program that links that
unit alone, once plain and once under the address and undefined-behaviour sanitizers; the descriptors hold made-up addresses and nothing
launches.  The program also reports the C layout of toist_conv_pair, which the launcher's ctypes class (kernels.ConvPair) must equal."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
G128 = 3            # gemm_family of csrc/gemm_route.h
P = 0x10000         # a 16-byte aligned made-up address


def _desc(**kw):
    from toist_amd.kernels import ConvPair
    d = ConvPair()
    d.M, d.C, d.dgrad, d.lda = 12800, 256, 0, 256
    d.a, d.w_first, d.w_second, d.res, d.mid, d.out = P, 2 * P, 3 * P, 4 * P, 5 * P, 6 * P
    d.shift_mid, d.shift_out = 7 * P, 8 * P
    d.ldr, d.ldmid, d.ldout = 1024, 1024, 256
    for key, val in kw.items():
        setattr(d, key, val)
    return d


def _dgrad(**kw):
    base = dict(dgrad=1, shift_mid=None, shift_out=None, aux_mid=9 * P, aux_out=10 * P, ldaux_mid=1024, ldaux_out=256)
    base.update(kw)
    return _desc(**base)


def cases():
    """(name, descriptor, accepted, needle of the refusal, second product on gemm128_kernel)"""
    return [
        ("forward, bench shape", _desc(), True, "", True),
        ("forward, one block", _desc(M=64), True, "", False),
        ("forward, partial block", _desc(M=35), True, "", False),
        ("forward, no shifts", _desc(shift_mid=None, shift_out=None), True, "", True),
        ("forward, wide rows", _desc(lda=264, ldr=1032, ldmid=1040, ldout=512), True, "", True),
        ("dgrad, bench shape", _dgrad(), True, "", True),
        ("dgrad, 162 rows", _dgrad(M=162), True, "", False),
        ("dgrad, wide rows", _dgrad(ldaux_mid=2048, ldaux_out=264), True, "", True),
        ("no rows", _desc(M=0), False, "bad shape", None),
        ("C = 128", _desc(C=128), False, "bad shape", None),
        ("dgrad = 2", _desc(dgrad=2), False, "dgrad = 2", None),
        ("null a", _desc(a=None), False, "null operand", None),
        ("null out", _desc(out=None), False, "null operand", None),
        ("null res", _desc(res=None), False, "res is required", None),
        ("aux forward", _desc(aux_mid=9 * P), False, "belong to the data gradient", None),
        ("aux_out forward", _desc(aux_out=9 * P), False, "belong to the data gradient", None),
        ("dgrad without aux_out", _dgrad(aux_out=None), False, "needs aux_mid and aux_out", None),
        ("dgrad with a shift", _dgrad(shift_out=7 * P), False, "takes no shift", None),
        ("misaligned a", _desc(a=P + 2), False, "16-byte aligned", None),
        ("misaligned mid", _desc(mid=5 * P + 8), False, "16-byte aligned", None),
        ("misaligned shift", _desc(shift_mid=7 * P + 4), False, "16-byte aligned", None),
        ("lda below the width", _desc(lda=248), False, "leading dimensions", None),
        ("ldmid % 8", _desc(ldmid=1028), False, "leading dimensions", None),
        ("dgrad ldaux_out % 8", _dgrad(ldaux_out=260), False, "leading dimensions", None),
        ("too many rows", _desc(M=1 << 21), False, "exceed the 2 GiB", None),
    ]


def _sanitizers_link(tmp_path):
    src = tmp_path / "one.cpp"
    src.write_text("int main() { return 0; }\n")
    return subprocess.call(["g++", *SANITIZE, str(src), "-o", str(tmp_path / "one")], stderr=subprocess.DEVNULL) == 0


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan_ubsan"])
def test_standalone_pair_check(tmp_path, sanitized):
    from toist_amd.kernels import ConvPair
    if sanitized and not _sanitizers_link(tmp_path):
        pytest.skip("g++ cannot link a one-line program with -fsanitize=address,undefined on this machine")
    exe = tmp_path / "conv_pair_check"
    subprocess.check_call(["g++", "-std=c++17", *(SANITIZE if sanitized else ["-O1"]), os.path.join(ROOT, "tests", "conv_pair_main.cpp"),
                           os.path.join(ROOT, "toist_amd", "csrc", "gemm_route.cpp"), "-o", str(exe)])
    table = cases()
    raw = tmp_path / "descs.bin"
    raw.write_bytes(b"".join(bytes(d) for _, d, *_ in table))
    done = subprocess.run([str(exe), str(raw)], text=True, capture_output=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr          # a sanitizer report is on stderr and ends the program
    layout, *lines = done.stdout.splitlines()
    # every field of the ctypes class sits where the C compiler puts it
    assert [int(x) for x in layout.split()] == [ctypes.sizeof(ConvPair)] + [getattr(ConvPair, name).offset for name, _ in ConvPair._fields_]
    assert len(lines) == len(table)
    for (name, _, accepted, needle, on_g128), line in zip(table, lines):
        verdict, msg = line.split(" | ", 1)
        code, applies, family = map(int, verdict.split())
        if accepted:
            assert (code, applies, msg) == (0, 1, ""), (name, msg)
            assert (family == G128) == on_g128, name
        else:
            assert (code, applies) == (-1, 0) and msg.startswith("toist_conv_pair_bf16: ") and needle in msg, (name, msg)
