"""Every file-scope device helper under toist_amd/csrc/ is defined in exactly one file.

The kernel files share small helpers (bf16 pack/unpack, lane-group sums, the attention dropout hash the forward and both backwards draw
their mask from).  A second copy of one of them builds, and can drift from the first without anything failing until a GPU parity test runs;
the shared ones live in csrc/common.h.  The sources are read as text: no compiler, no allowlist."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "toist_amd", "csrc")
# a line that starts at column 0 (struct members are indented), says __device__, and then names a function: the identifier before the first '('
DEVICE_FN = re.compile(r"^(?=\S)[^\n]*?\b__device__\b[^(\n]*?\b([A-Za-z_]\w*)\s*\(", re.M)


def device_functions():
    """{name: sorted files that define it at file scope}"""
    where = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        with open(path) as f:
            for name in set(DEVICE_FN.findall(f.read())):
                where.setdefault(name, []).append(os.path.basename(path))
    return where


def test_the_scan_sees_the_helpers():
    """the pattern finds plain, templated and static definitions, and where the shared ones are"""
    where = device_functions()
    assert len(where) > 50
    for name in ("bf2f", "wave_sum", "hash_u32", "pair_hash", "unpack8", "unrolled", "block_sum"):
        assert where.get(name) == ["common.h"], (name, where.get(name))
    assert where["attn2_bwd_body"] == ["attn2_bwd_body.h"]


def test_no_device_helper_is_defined_in_two_files():
    twice = {name: files for name, files in device_functions().items() if len(files) > 1}
    for name in sorted(twice):
        print("%s: %s" % (name, ", ".join(twice[name])))
    assert not twice, "file-scope __device__ functions defined in more than one file: %s" % sorted(twice)
