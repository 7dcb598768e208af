"""What the C compiler says about include/toist_hip.h, for the tests that hold the Python side of the boundary against it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_values(tmp_path, exprs):
    """The values of the C integer expressions `exprs` (sizeof / offsetof / constants of toist_hip.h) as gcc evaluates them: one generated
    program prints one number per expression."""
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    lines = "".join(f'    printf("%lld\\n", (long long)({e}));\n' for e in exprs)
    src.write_text(f'#include "toist_hip.h"\n#include <stdio.h>\nint main(void) {{\n{lines}    return 0;\n}}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert len(got) == len(exprs)
    return got
