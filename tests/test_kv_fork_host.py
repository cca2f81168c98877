"""KvBlocks::fork (csrc/kv_blocks.h), the host half of mi_kv_fork_row: a row takes the first tokens of another row by mapping
its full blocks and getting one block of its own for the partly filled tail.  tests/cpu/kv_blocks_fork_test.cpp exercises it in
a stand-alone program built with the address and undefined-behaviour sanitizers: directed cases on a 12-block pool of 16-token
blocks and a seeded random walk (ensure / release / attach / publish / fork) against a naive model.  No GPU, nothing
preloaded."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CHECKS = 61          # "ok" lines of the program: 55 directed, 6 of the walk


def test_kv_blocks_fork_on_the_host_under_sanitizers(tmp_path):
    exe = tmp_path / "kv_blocks_fork_test"
    # (the sanitizer runtimes linked INTO the program: it then runs whatever else the environment loads ahead of it)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", str(ROOT / "mlx_parallm_amd" / "csrc"),
                    str(ROOT / "tests" / "cpu" / "kv_blocks_fork_test.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert not [l for l in lines if l.startswith("FAIL")]
    assert sum(l.startswith("ok ") for l in lines) == CHECKS and lines[-1] == f"checks {CHECKS}"
