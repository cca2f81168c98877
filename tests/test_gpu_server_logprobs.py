"""-m gpu: a ``logprobs`` completion under ``--scheduler continuous`` on a real engine, over real HTTP: it arrives while a
streaming generation is in flight, comes back with n choices and their per-token lists, and the stream finishes."""
import json
import os
import signal
import socket
import subprocess
import sys
import threading
import time
from pathlib import Path

import numpy as np
import pytest
import requests

from oracle import ref_generate, ref_sample

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return int(s.getsockname()[1])


@pytest.fixture(scope="module")
def server(tiny_dirs, tmp_path_factory):
    model_dir = tiny_dirs["llama_q4_f32"][0]
    port = _free_port()
    log_path = tmp_path_factory.mktemp("server_lp") / "server.log"
    env = os.environ.copy()
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    args = [sys.executable, "-m", "mlx_parallm_amd.cli", "--model-path", model_dir, "--host", "127.0.0.1", "--port", str(port),
            "--max-batch-size", "4", "--scheduler", "continuous"]
    with open(log_path, "w", buffering=1) as lf:
        proc = subprocess.Popen(args, cwd=str(ROOT), stdout=lf, stderr=subprocess.STDOUT, text=True, env=env)
    base = f"http://127.0.0.1:{port}"
    import fastapi, transformers, uvicorn  # noqa: F401,E401  (pages the child's imports in: a fresh box reads them cold)
    deadline = time.time() + 600
    ok = False
    while time.time() < deadline and proc.poll() is None:
        try:
            if requests.get(f"{base}/health", timeout=2).ok:
                ok = True
                break
        except Exception:
            time.sleep(0.5)
    if not ok:
        proc.kill()
        pytest.fail("server did not come up:\n" + log_path.read_text()[-3000:])
    yield base, model_dir
    proc.send_signal(signal.SIGTERM)
    try:
        proc.wait(timeout=20)
    except subprocess.TimeoutExpired:
        proc.kill()


def test_a_logprobs_request_next_to_a_stream_in_flight(server):
    base, model_dir = server
    from mlx_parallm_amd.tokenizer_utils import load_tokenizer

    tok = load_tokenizer(model_dir)
    hf = tok._tokenizer
    first, events = threading.Event(), []

    def stream():
        with requests.post(f"{base}/v1/completions", stream=True, timeout=120, json={
                "model": model_dir, "prompt": "Tell a long story.", "max_tokens": 200, "temperature": 0.0, "stream": True}) as r:
            events.append(r.status_code)
            for line in r.iter_lines():
                if line.startswith(b"data: "):
                    events.append(line[len(b"data: "):].decode())
                    first.set()
        first.set()

    th = threading.Thread(target=stream)
    th.start()
    assert first.wait(timeout=120)
    prompt = "Say hello in one word."
    r = requests.post(f"{base}/v1/completions", timeout=120, json={
        "model": model_dir, "prompt": prompt, "max_tokens": 6, "temperature": 0.0, "logprobs": 2, "n": 2})
    th.join(timeout=120)
    assert r.status_code == 200, r.text[:500]
    j = r.json()
    assert len(j["choices"]) == 2
    ids = [int(t) for t in tok.encode(prompt)]
    ref = ref_generate.load(model_dir, max_pos=512)
    listed = 0
    for ch in j["choices"]:
        lp = ch["logprobs"]
        n = len(lp["tokens"])
        assert 1 <= n <= 7 and len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == len(lp["text_offset"]) == n
        listed += n - (1 if ch["finish_reason"] == "stop" else 0)      # (no stop strings here: "stop" is an EOS, kept in the lists)
        gen = [int(t) for t in hf.convert_tokens_to_ids(lp["tokens"])]
        seq = np.asarray(ids + gen[:-1], np.int32)[None]
        lg = np.asarray(ref(seq, cache=ref.make_cache(1, paged=False)), np.float32)[0, len(ids) - 1:]
        lsm = ref_sample.log_softmax(lg)
        want = lsm[np.arange(n), gen]
        worst = float(np.max(np.abs(np.asarray(lp["token_logprobs"]) - want)))
        print(f"max |token_logprob - oracle| = {worst:.3e}")
        assert worst <= 1e-3
        for d, t, v in zip(lp["top_logprobs"], lp["tokens"], lp["token_logprobs"]):
            assert 1 <= len(d) <= 2 and max(d, key=d.get) == t and d[t] == v     # greedy: the best entry is the token
    assert j["usage"]["completion_tokens"] == listed
    assert j["usage"]["prompt_tokens"] == len(ids) and j["usage"]["total_tokens"] == len(ids) + listed
    # the stream ran to its end
    assert not th.is_alive() and events[0] == 200 and events[-1] == "[DONE]"
    last = json.loads(events[-2])
    assert last["choices"][0]["finish_reason"] in ("stop", "length")
    text = "".join(json.loads(e)["choices"][0].get("text") or "" for e in events[1:-1])
    assert len(text) > 0
