"""KvBlocks::shared_sets (csrc/kv_blocks.h) in a stand-alone program under the address and undefined-behaviour sanitizers
(tests/cpu/kv_blocks_sets_test.cpp).  No GPU, nothing preloaded."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CHECKS = 6          # "ok" lines of the program


def test_kv_blocks_shared_sets_on_the_host_under_sanitizers(tmp_path):
    exe = tmp_path / "kv_blocks_sets_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", str(ROOT / "mlx_parallm_amd" / "csrc"),
                    str(ROOT / "tests" / "cpu" / "kv_blocks_sets_test.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert not [l for l in lines if l.startswith("FAIL")]
    assert sum(l.startswith("ok ") for l in lines) == CHECKS and lines[-1] == f"checks {CHECKS}"
