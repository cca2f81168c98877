"""The paged KV cache's host state (csrc/kv_blocks.h: block pool, block tables, prefix cache) is plain C++ with no HIP in it.
tests/cpu/kv_blocks_test.cpp exercises it in a stand-alone program built with the address and undefined-behaviour
sanitizers: directed cases on a 12-block pool and a seeded random walk against a naive model.  No GPU, nothing preloaded."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CHECKS = 44          # "ok" lines of the program: 39 directed, 5 of the walk


def test_kv_blocks_on_the_host_under_sanitizers(tmp_path):
    exe = tmp_path / "kv_blocks_test"
    # (the sanitizer runtimes linked INTO the program: it then runs whatever else the environment loads ahead of it)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", str(ROOT / "mlx_parallm_amd" / "csrc"), str(ROOT / "tests" / "cpu" / "kv_blocks_test.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert not [l for l in lines if l.startswith("FAIL")]
    assert sum(l.startswith("ok ") for l in lines) == CHECKS and lines[-1] == f"checks {CHECKS}"
