"""The prefix cache under per-request adapters (csrc/kv_blocks.h): K / V blocks depend on the adapter of the row that made them,
so KvBlocks::attach / publish start a row's hash chain from adapter_seed(slot, generation), and from 0 for a row without an
adapter -- the keys such rows always had.  tests/cpu/kv_blocks_adapter_test.cpp exercises it in a stand-alone program built
with the address and undefined-behaviour sanitizers: directed cases (a chain is found under its own slot and generation alone,
seed 0 leaves the keys unchanged, a replaced adapter's chain leaves through the LRU) and a seeded random walk against a naive
model keyed by (seed, token prefix).  No GPU, nothing preloaded."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CHECKS = 28          # "ok" lines of the program: 24 directed, 4 of the walk


def test_seeded_prefix_chains_on_the_host_under_sanitizers(tmp_path):
    exe = tmp_path / "kv_blocks_adapter_test"
    # (the sanitizer runtimes linked INTO the program: it then runs whatever else the environment loads ahead of it)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", str(ROOT / "mlx_parallm_amd" / "csrc"),
                    str(ROOT / "tests" / "cpu" / "kv_blocks_adapter_test.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert not [l for l in lines if l.startswith("FAIL")]
    assert sum(l.startswith("ok ") for l in lines) == CHECKS and lines[-1] == f"checks {CHECKS}"
