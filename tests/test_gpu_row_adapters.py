"""Per-request LoRA adapters (-m gpu): several adapters resident on one engine, every KV row names one of them or none, and
each row of a step -- decode, prefill, mixed, score -- runs its own.  The engine against the oracle, row by row: every row is
compared with an oracle loaded with THAT row's adapter, run alone at B = 1.

Adapters (tests/row_adapter_cases.py; the recipe of test_gpu_lora_targets.py): P and Q rank 16 on all seven linears, R1 rank 1
on all seven, R5 rank 5 on q, k, v only, R64 rank 64 on gate, up, down only; none = the base model.

Bounds (the project's own, tests/test_gpu_engine.py):
  float32-KV (oracle: paged cache)  greedy ids exact, logprobs within 1e-3, logits within 4e-3
  model-dtype KV                    logits within 0.08; logprobs of mi_score_tokens within 0.1 (MODEL_KV_LOGPROB_TOL there)
A mix-up of adapters cannot hide inside a bound: every test first shows, on the oracle alone and for its own prompts, that the
adapters it uses move the last position's logits of every row by at least 5 x the tolerance of the mode."""
import ctypes as C

import numpy as np
import pytest

import row_adapter_cases as cases
from oracle import ref_generate, ref_sample

pytestmark = pytest.mark.gpu

from mlx_parallm_amd import _lib as L  # noqa: E402
from mlx_parallm_amd import utils  # noqa: E402
from mlx_parallm_amd.engine import SampleArgs  # noqa: E402

MAX_POS = 256
NAMES = ["llama_q4_bf16", "qwen3_bf16"]
# mode -> (kv dtype of the engine, oracle paged cache, logit tolerance)
MODES = {"float32": ("float32", True, 4e-3), "model": ("model", False, 0.08)}
LOGPROB_TOL_F32KV, MODEL_KV_LOGPROB_TOL, MODEL_KV_MARGIN = 1e-3, 0.1, 0.13
SLOTS = {"P": 0, "Q": 3, "R1": 7, "R5": 9, "R64": L.MI_MAX_ADAPTERS - 1, None: -1}
CASE1 = ["P", None, "R5", "Q", "R64", "R1"]


class Bank:
    """Adapter directories, oracles and oracle results, made on first use and shared (read-only) by the tests."""

    def __init__(self, tiny_dirs, root):
        self.tiny, self.root = tiny_dirs, root
        self._dir, self._ref, self._want = {}, {}, {}

    def cfg(self, name):
        return self.tiny[name][1]

    def adapter(self, name, ad):
        if (name, ad) not in self._dir:
            self._dir[(name, ad)] = cases.write(self.root / f"{name}_{ad}", self.cfg(name), ad)
        return self._dir[(name, ad)]

    def ref(self, name, ad):
        if (name, ad) not in self._ref:
            kw = {} if ad is None else {"adapter_path": self.adapter(name, ad)}
            self._ref[(name, ad)] = ref_generate.load(self.tiny[name][0], max_pos=MAX_POS, **kw)
        return self._ref[(name, ad)]

    def model(self, name, slots=None):
        """an engine with adapter `ad` resident in slot s for every s: ad of `slots` (default: all five, at SLOTS)"""
        model = utils.load_model(self.tiny[name][0], max_positions=MAX_POS)
        for s, ad in (slots if slots is not None else {SLOTS[a]: a for a in cases.ADAPTERS}).items():
            utils.load_adapter_into(model, s, self.adapter(name, ad))
        return model

    def oracle_run(self, name, mode, toks, ads, steps, all_positions=False):
        """Row b of `toks` on the oracle of ads[b], alone: the prompt, then `steps` teacher-forced greedy tokens.
        -> (feeds: the token arrays a batched engine is fed, want: the logits behind each, [B][V] or [B][L][V])"""
        key = (name, mode, toks.tobytes(), toks.shape, tuple(ads), steps, all_positions)
        if key not in self._want:
            paged = MODES[mode][1]
            B = toks.shape[0]
            rows = []
            for b in range(B):
                ref = self.ref(name, ads[b])
                cache = ref.make_cache(1, paged=paged)
                lg = ref(toks[b:b + 1], cache=cache)[0]
                out, fed = [lg if all_positions else lg[-1]], []
                for _ in range(steps):
                    nxt = int(np.argmax(lg[-1]))
                    fed.append(nxt)
                    lg = ref(np.asarray([[nxt]], dtype=np.int32), cache=cache)[0]
                    out.append(lg[-1])
                rows.append((out, fed))
            feeds = [toks] + [np.asarray([[rows[b][1][s]] for b in range(B)], dtype=np.int32) for s in range(steps)]
            want = [np.stack([rows[b][0][s] for b in range(B)]) for s in range(steps + 1)]
            self._want[key] = (feeds, want)
        return self._want[key]

    def assert_distinct(self, name, mode, toks, ads):
        """On the oracle alone: every row's last-position logits under its own adapter differ from those under every other
        adapter of the test by at least 5 x the mode's tolerance."""
        paged, tol = MODES[mode][1], MODES[mode][2]
        least = np.inf
        for b in range(toks.shape[0]):
            last = {}
            for ad in set(ads):
                ref = self.ref(name, ad)
                last[ad] = ref(toks[b:b + 1], cache=ref.make_cache(1, paged=paged))[0, -1]
            for ad in set(ads) - {ads[b]}:
                least = min(least, float(np.abs(last[ads[b]] - last[ad]).max()))
        print(f"{name} {mode}: adapters differ by >= {least:.3f} on the oracle (5 x tolerance = {5 * tol:.3f})")
        assert least >= 5 * tol, least


@pytest.fixture(scope="module")
def bank(tiny_dirs, tmp_path_factory):
    return Bank(tiny_dirs, tmp_path_factory.mktemp("row_adapters"))


def _toks(cfg, B, L0, seed):
    return np.random.default_rng([seed, B, L0]).integers(3, cfg["vocab_size"], size=(B, L0)).astype(np.int32)


def _new_kv(eng, B, cap, kvd, ads):
    kv = eng.new_kv(B, capacity=cap, kv_dtype=kvd)
    for b, ad in enumerate(ads):
        kv.set_row_adapter(b, SLOTS.get(ad, ad))        # (an adapter name of SLOTS, or a slot number)
    return kv


def _forward_run(eng, mode, feeds, ads, all_positions=False):
    """the feeds through Engine.forward on a cache whose row b names ads[b] -> the logits behind each feed"""
    kv = _new_kv(eng, feeds[0].shape[0], sum(f.shape[1] for f in feeds) + 1, MODES[mode][0], ads)
    out = [eng.forward(feeds[0], kv, all_positions=all_positions)] + [eng.forward(f, kv) for f in feeds[1:]]
    kv.close()
    return out


def _check_rows(bank, model, name, mode, toks, ads, steps=3, all_positions=False, what=""):
    """the batch against every row's own oracle: logits in both modes; ids and logprobs of the sampler in the float32-KV mode"""
    bank.assert_distinct(name, mode, toks, ads)
    feeds, want = bank.oracle_run(name, mode, toks, ads, steps, all_positions)
    got = _forward_run(model.engine, mode, feeds, ads, all_positions)
    err = max(float(np.abs(g - w).max()) for g, w in zip(got, want))
    print(f"{what} {mode}: max |logit - oracle| = {err:.3e}")
    assert err <= MODES[mode][2], (what, mode, err, [float(np.abs(g - w).reshape(len(ads), -1).max(axis=1).max()) for g, w in zip(got, want)])
    if mode == "float32":
        kv = _new_kv(model.engine, len(ads), sum(f.shape[1] for f in feeds) + 1, "float32", ads)
        wrong, lp_err = 0, 0.0
        for f, w in zip(feeds, want):
            res = model.engine.decode_sample(kv, f, SampleArgs(temp=0.0))
            ws = ref_sample.sample(w[:, -1] if w.ndim == 3 else w, temp=0.0)
            wrong += int((res["tokens"] != ws["tokens"][:, 0]).sum())
            lp_err = max(lp_err, float(np.abs(res["logprobs"] - ws["logprobs"].reshape(-1)).max()))
        kv.close()
        print(f"{what} {mode}: ids off {wrong}, max |logprob - oracle| = {lp_err:.3e}")
        assert wrong == 0 and lp_err <= LOGPROB_TOL_F32KV, (what, wrong, lp_err)
    return got


# ------------------------------------------------------------------------------------ 1. rows against the oracle
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_rows_against_their_own_oracles(bank, name, mode):
    """Six unpadded sequences of 7 tokens on [P, none, R5, Q, R64, R1] (slots 0, 3, 7, 9 and the last): the prefill and three
    teacher-forced decode steps."""
    model = bank.model(name)
    _check_rows(bank, model, name, mode, _toks(bank.cfg(name), 6, 7, seed=1), CASE1, what=f"{name} 6x7")
    model.engine.close()


# ------------------------------------------------------------------------------------ 2. regimes
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_row_regimes(bank, name, mode):
    """decode at B = 12, the adapters cycling (the 9..128-row kernels); a prefill of 3 x 60 = 180 rows, one adapter per
    sequence, all positions (the tile GEMM)."""
    cfg = bank.cfg(name)
    model = bank.model(name)
    _check_rows(bank, model, name, mode, _toks(cfg, 12, 3, seed=2), ["P", "Q", None, "R1", "R5", "R64"] * 2, what=f"{name} B=12")
    _check_rows(bank, model, name, mode, _toks(cfg, 3, 60, seed=3), ["P", "R5", "R64"], steps=1, all_positions=True, what=f"{name} 3x60")
    model.engine.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_mixed_step(bank, name, mode):
    """mi_step_enqueue_mixed: two decode rows on P and Q plus a 5-token chunk on R5 in one pass over the weights; then one plain
    forward over the three rows (its logits depend on the K / V the mixed step wrote)."""
    cfg = bank.cfg(name)
    kvd, paged, tol = MODES[mode]
    ads = ["P", "Q", "R5"]
    rng = np.random.default_rng(9)
    prompts = [rng.integers(3, cfg["vocab_size"], size=n).astype(np.int32) for n in (6, 4, 5)]
    for b, p in enumerate(prompts):
        bank.assert_distinct(name, mode, p[None], [ads[b]] + [a for a in ads if a != ads[b]])
    model = bank.model(name)
    eng = model.engine
    greedy = SampleArgs(temp=0.0)
    kv = _new_kv(eng, 3, 32, kvd, ads)
    refs = [bank.ref(name, a) for a in ads]
    caches = [r.make_cache(1, paged=paged) for r in refs]

    def oracle(i, toks):
        lg = refs[i](np.asarray(toks, dtype=np.int32)[None], cache=caches[i])[0, -1]
        return lg, ref_sample.sample(lg[None], temp=0.0)

    def compare(res, wants):
        for j, (lg, w) in enumerate(wants):
            gt, wt = int(res["tokens"][j]), int(w["tokens"][0, 0])
            if mode == "float32":
                assert gt == wt, (j, gt, wt)
                assert abs(float(res["logprobs"][j]) - float(w["logprobs"].reshape(-1)[0])) <= LOGPROB_TOL_F32KV
            else:
                assert gt == wt or float(lg[wt] - lg[gt]) <= MODEL_KV_MARGIN, (j, gt, wt)
                if gt == wt:
                    assert abs(float(res["logprobs"][j]) - float(w["logprobs"].reshape(-1)[0])) <= MODEL_KV_LOGPROB_TOL

    res = eng.step_wait(eng.step_enqueue_mixed(kv, [0, 1], [prompts[0], prompts[1]], [1, 1], greedy), 2)
    w0, w1 = oracle(0, prompts[0]), oracle(1, prompts[1])
    compare(res, [w0, w1])
    t0, t1 = int(w0[1]["tokens"][0, 0]), int(w1[1]["tokens"][0, 0])
    res = eng.step_wait(eng.step_enqueue_mixed(kv, [0, 1, 2], [[t0], [t1], prompts[2]], [1, 1, 1], greedy), 3)   # THE mixed step
    assert kv.offsets == [7, 5, 5]
    wants = [oracle(0, [t0]), oracle(1, [t1]), oracle(2, prompts[2])]
    compare(res, wants)
    nxt = np.asarray([[int(w[1]["tokens"][0, 0])] for w in wants], dtype=np.int32)
    got = eng.forward(nxt, kv)
    want = np.stack([oracle(i, nxt[i])[0] for i in range(3)])
    err = float(np.abs(got - want).max())
    print(f"{name} {mode}: forward behind the mixed step, max |logit - oracle| = {err:.3e}")
    assert err <= tol, err
    kv.close()
    eng.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_score_tokens_with_two_adapters(bank, name, mode):
    """mi_score_tokens on two rows with different adapters: every position's logprob of its target against the row's oracle."""
    cfg = bank.cfg(name)
    kvd, paged, _ = MODES[mode]
    ads = ["Q", "R64"]
    toks = _toks(cfg, 2, 9, seed=4)
    targets = _toks(cfg, 2, 9, seed=5)
    bank.assert_distinct(name, mode, toks, ads)
    want = np.empty((2, 9), dtype=np.float64)
    for b in range(2):
        ref = bank.ref(name, ads[b])
        lg = ref(toks[b:b + 1], cache=ref.make_cache(1, paged=paged))[0].astype(np.float64)
        lse = np.log(np.exp(lg - lg.max(-1, keepdims=True)).sum(-1)) + lg.max(-1)
        want[b] = lg[np.arange(9), targets[b]] - lse
    model = bank.model(name)
    kv = _new_kv(model.engine, 2, 16, kvd, ads)
    got = model.engine.score_tokens(kv, toks, targets)["logprobs"]
    err = float(np.abs(got - want).max())
    print(f"{name} {mode}: score_tokens, max |logprob - oracle| = {err:.3e}")
    assert err <= (LOGPROB_TOL_F32KV if mode == "float32" else MODEL_KV_LOGPROB_TOL), err
    kv.close()
    model.engine.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_down_proj_row_above_48_kib_of_lds(tmp_path, mode):
    """down_proj's by-row down kernel stages a row of intermediate_size floats in LDS; above 12288 of them the launch opts in
    to more dynamic LDS than the default (Qwen3-14B: 17408).  A two-block model with intermediate_size 12544, rows on [P, none,
    R64]: the prefill and two decode steps against the rows' oracles."""
    from mlx_parallm_amd.tiny_model import build_tiny_model

    cfg = build_tiny_model(tmp_path / "wide", seed=33, vocab_size=512, dtype="bfloat16", quantize_model=False, hidden_size=128,
                           layers=2, heads=8, kv_heads=2, intermediate_size=12544, head_dim=16, tie_word_embeddings=False,
                           norm_jitter=0.1, with_tokenizer=False)
    bank = Bank({"wide": (str(tmp_path / "wide"), cfg)}, tmp_path / "adapters")
    model = bank.model("wide", {0: "P", 15: "R64"})
    ads = [0, None, 15]
    names = ["P", None, "R64"]
    toks = _toks(cfg, 3, 5, seed=7)
    bank.assert_distinct("wide", mode, toks, names)
    feeds, want = bank.oracle_run("wide", mode, toks, names, 2)
    got = _forward_run(model.engine, mode, feeds, ads)
    err = max(float(np.abs(g - w).max()) for g, w in zip(got, want))
    print(f"intermediate_size 12544 {mode}: max |logit - oracle| = {err:.3e}")
    assert err <= MODES[mode][2], err
    model.engine.close()


# ------------------------------------------------------------------------------------ 3. bits
def _bits(model, cfg, ads_of, seed=8):
    """logits of a 2 x 7 prefill with a decode step, and of a 12 x 3 one, in both KV modes; row b names ads_of(B)[b]"""
    out = []
    for mode in MODES:
        for B, L0 in ((2, 7), (12, 3)):
            toks = _toks(cfg, B, L0, seed)
            out += _forward_run(model.engine, mode, [toks, toks[:, -1:]], ads_of(B), all_positions=True)
    return out


def _assert_same_bits(a, b, what=""):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, float(np.abs(x - y).max()))


@pytest.mark.parametrize("name", NAMES)
def test_bits_resident_adapters_cost_unadapted_rows_nothing(bank, name):
    """(a) five adapters resident, every row on -1: the bits of an engine that never saw an adapter."""
    cfg = bank.cfg(name)
    plain, table = bank.model(name, {}), bank.model(name)
    _assert_same_bits(_bits(table, cfg, lambda B: [None] * B), _bits(plain, cfg, lambda B: [None] * B))
    plain.engine.close(); table.engine.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_bits_row_does_not_depend_on_its_neighbours_adapters(bank, name, mode):
    """(b) a row's logits in the mixed-adapter batch of case 1 are those of the same row in a batch where every row runs its
    adapter.  The row WITHOUT an adapter is compared with itself among five rows on P instead: a batch in which no row names
    an adapter runs the fused launches of an engine without adapters (bit test (a)), and those are not the by-row launches'
    bits by the project's own design -- the fused SwiGLU epilogue takes the sigmoid in float32, swiglu_rows_kernel in float64
    (linear_epilogue.h), one ulp apart in the float32-KV mode where nothing rounds behind it.  Measured, and printed below: max
    |logit| difference 2.6e-6 (llama_q4_bf16) and 4.5e-6 (qwen3_bf16) in the float32-KV mode, 0 in the model-KV mode -- a
    thousandth of the float32-KV logit bound that both forms meet against the oracle."""
    toks = _toks(bank.cfg(name), 6, 7, seed=1)
    feeds, _ = bank.oracle_run(name, mode, toks, CASE1, 3)
    model = bank.model(name)
    mixed = _forward_run(model.engine, mode, feeds, CASE1)
    for b, ad in enumerate(CASE1):
        if ad is None:
            other = ["P"] * 6
            other[b] = None
            alone = _forward_run(model.engine, mode, feeds, other)
            fused = _forward_run(model.engine, mode, feeds, [None] * 6)
            delta = max(float(np.abs(m[b] - f[b]).max()) for m, f in zip(mixed, fused))
            print(f"{name} {mode}: the row without an adapter, by-row launches against the fused ones: max |logit difference| = {delta:.3e}")
        else:
            alone = _forward_run(model.engine, mode, feeds, [ad] * 6)
        _assert_same_bits([m[b] for m in mixed], [a[b] for a in alone], what=(b, ad))
    model.engine.close()


@pytest.mark.parametrize("name", NAMES)
def test_bits_slot_number_and_hot_swap(bank, name):
    """(c) P in slot 0 gives the bits of P in slot 5.  (d) Q replaced by P in place, projection by projection on the live engine:
    the row gives the bits of a fresh engine with P.  And the engine-wide adapter of mi_engine_set_lora is a private column of
    the same table that every row runs: P there gives the bits of a batch whose rows all name P in a slot."""
    cfg = bank.cfg(name)
    m0, m5 = bank.model(name, {0: "P"}), bank.model(name, {5: "P"})
    p0 = _bits(m0, cfg, lambda B: [0] * B)
    _assert_same_bits(p0, _bits(m5, cfg, lambda B: [5] * B), "slot 0 / slot 5")
    m5.engine.close()
    live = bank.model(name, {3: "Q"})
    q3 = _bits(live, cfg, lambda B: [3] * B)
    assert any(not np.array_equal(x, y) for x, y in zip(p0, q3))
    fac = cases.factors(cfg, "P")
    for base in sorted({k.rsplit(".", 1)[0] for k in fac}):
        layer, proj = int(base.split(".")[2]), base.split(".", 3)[3]
        live.engine.set_adapter_lora(3, layer, proj, fac[base + ".lora_a"], fac[base + ".lora_b"], cases.SCALE)
    _assert_same_bits(p0, _bits(live, cfg, lambda B: [3] * B), "Q replaced by P")
    live.engine.close(); m0.engine.close()
    wide = utils.load_model(bank.tiny[name][0], max_positions=MAX_POS)
    utils.load_adapters(wide, bank.adapter(name, "P"))
    pw = _bits(wide, cfg, lambda B: [None] * B)
    delta = max(float(np.abs(x - y).max()) for x, y in zip(p0, pw))
    print(f"{name}: max |logit(table, every row on P) - logit(mi_engine_set_lora P)| = {delta:.3e}")
    _assert_same_bits(p0, pw, "every row on P / mi_engine_set_lora P")
    wide.engine.close()


# ------------------------------------------------------------------------------------ 4. prefix cache
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_prefix_cache_is_keyed_by_adapter(bank, name, mode):
    """Paged cache, 16-token blocks, a 40-token prompt: blocks published under P are reused under P alone, blocks published
    under none by rows without an adapter alone, and after one projection of P was hot-swapped nothing of the old P."""
    cfg = bank.cfg(name)
    kvd, paged, tol = MODES[mode]
    toks = np.random.default_rng(3).integers(3, cfg["vocab_size"], size=40).astype(np.int32)     # two full blocks + 8 tokens
    bank.assert_distinct(name, mode, toks[None], ["P", "Q", None])
    model = bank.model(name, {0: "P", 3: "Q"})
    eng = model.engine
    kv = eng.new_paged_kv(2, block_tokens=16, n_blocks=20, max_tokens_per_row=64, kv_dtype=kvd)
    greedy = SampleArgs(temp=0.0)

    def attach(row, slot):
        kv.reset_row(row)
        kv.set_row_adapter(row, slot)
        return kv.prefix_attach(row, toks)

    kv.set_row_adapter(0, 0)
    eng.step_wait(eng.step_enqueue_rows(kv, [0], toks[None], greedy), 1)
    kv.prefix_publish(0, toks)
    assert attach(1, 3) == 0 and attach(1, -1) == 0 and attach(1, 0) == 32
    got = eng.forward(np.stack([toks[32:], toks[32:]]), kv)[1]               # (row 0 runs on: both rows take 8 tokens)
    ref = bank.ref(name, "P")
    want = ref(toks[None], cache=ref.make_cache(1, paged=paged))[0, -1]
    err = float(np.abs(got - want).max())
    print(f"{name} {mode}: logits behind a prefix reused under P, max |logit - oracle| = {err:.3e}")
    assert err <= tol, err
    kv.reset_row(1)                                                                          # (the row names no adapter now)
    eng.step_wait(eng.step_enqueue_rows(kv, [1], toks[None], greedy), 1)
    kv.prefix_publish(1, toks)
    assert attach(0, -1) == 32 and attach(0, 3) == 0 and attach(0, 0) == 32
    last = cfg["num_hidden_layers"] - 1
    fac = cases.factors(cfg, "P")
    eng.set_adapter_lora(0, last, "self_attn.k_proj", fac[f"model.layers.{last}.self_attn.k_proj.lora_a"],
                         fac[f"model.layers.{last}.self_attn.k_proj.lora_b"], cases.SCALE)
    assert attach(0, 0) == 0 and attach(0, -1) == 32
    kv.close()
    eng.close()


# ------------------------------------------------------------------------------------ 5. fork
@pytest.mark.parametrize("kind", ["paged", "contiguous"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_fork_keeps_the_adapter(bank, name, mode, kind):
    """dst forks only while it names src's adapter (MI_ERR_INVALID naming dst otherwise, nothing changed); the fork continues on
    that adapter: the next step's logits of both rows against the oracle with P."""
    cfg = bank.cfg(name)
    kvd, paged, tol = MODES[mode]
    prompt = np.random.default_rng(6).integers(3, cfg["vocab_size"], size=20).astype(np.int32)
    bank.assert_distinct(name, mode, prompt[None], ["P", "Q", None])
    model = bank.model(name, {0: "P", 3: "Q"})
    eng = model.engine
    kv = (eng.new_paged_kv(2, block_tokens=16, n_blocks=8, max_tokens_per_row=64, kv_dtype=kvd) if kind == "paged"
          else eng.new_kv(2, capacity=64, kv_dtype=kvd))
    kv.set_row_adapter(0, 0)
    eng.step_wait(eng.step_enqueue_rows(kv, [0], prompt[None], SampleArgs(temp=0.0)), 1)
    for slot in (-1, 3):
        kv.set_row_adapter(1, slot)
        with pytest.raises(ValueError, match="dst"):
            kv.fork_row(0, 1, 20)
        assert kv.offsets == [20, 0]
    kv.set_row_adapter(1, 0)
    kv.fork_row(0, 1, 20)
    assert kv.offsets == [20, 20]
    nxt = np.asarray([[5], [9]], dtype=np.int32)
    got = eng.forward(nxt, kv)
    ref = bank.ref(name, "P")
    for b in range(2):
        want = ref(np.concatenate([prompt, nxt[b]])[None], cache=ref.make_cache(1, paged=paged))[0, -1]
        err = float(np.abs(got[b] - want).max())
        print(f"{name} {mode} {kind}: row {b} behind the fork, max |logit - oracle| = {err:.3e}")
        assert err <= tol, (b, err)
    kv.close()
    eng.close()


# ------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_engine_usable(bank):
    name = "llama_q4_bf16"
    cfg = bank.cfg(name)
    model = bank.model(name, {0: "P", 3: "Q"})
    eng = model.engine
    ads_of = lambda B: [0, -1, 3] * (B // 3) + [0] * (B % 3)      # noqa: E731
    before = _bits(model, cfg, ads_of)
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    last = cfg["num_hidden_layers"] - 1
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal((H, 16)).astype(np.float32), rng.standard_normal((16, I)).astype(np.float32)
    for slot in (-2, L.MI_MAX_ADAPTERS):
        with pytest.raises(ValueError, match="adapter"):
            eng.set_adapter_lora(slot, last, "mlp.gate_proj", a, b, 10.0)
        with pytest.raises(ValueError, match="adapter"):
            eng.clear_adapter(slot)
    big_a, big_b = np.zeros((H, 65), dtype=np.float32), np.zeros((65, I), dtype=np.float32)
    for rank in (0, 65):                                          # (through the C ABI: a rank-0 array has no address to pass)
        rc = L.lib().mi_engine_set_adapter_lora(eng._h, 0, last, b"mlp.gate_proj", big_a.ctypes.data_as(C.c_void_p),
                                                big_b.ctypes.data_as(C.c_void_p), rank, 10.0, L.MI_F32, 0)
        assert rc == -3 and b"rank" in L.lib().mi_last_error(), (rank, rc)
    for proj in ("lm_head", "mlp.gate", "self_attn.qkv_proj"):
        with pytest.raises(NotImplementedError, match="not supported"):
            eng.set_adapter_lora(0, last, proj, a, b, 10.0)
    kv = eng.new_kv(3, capacity=16, kv_dtype="model")
    toks = _toks(cfg, 3, 4, seed=2)
    eng.forward(toks, kv)
    with pytest.raises(ValueError, match="empty"):                # a row that holds tokens
        kv.set_row_adapter(1, 0)
    for slot in (-2, L.MI_MAX_ADAPTERS):
        with pytest.raises(ValueError, match="adapter"):
            kv.set_row_adapter(1, slot)
    kv.reset()
    kv.set_row_adapter(1, 7)                                      # slot 7 is empty
    for call in (lambda: eng.forward(toks, kv), lambda: eng.decode_sample(kv, toks, SampleArgs(temp=0.0)),
                 lambda: eng.step_enqueue_mixed(kv, [1], [toks[1]]), lambda: eng.score_tokens(kv, toks, toks)):
        with pytest.raises(ValueError, match="empty slot"):
            call()
        assert kv.offsets == [0, 0, 0]
    with pytest.raises(NotImplementedError, match="exclude"):     # the engine-wide adapter after the table
        eng.set_lora(last, "mlp.gate_proj", a, b, 10.0)
    kv.reset()
    kv.set_row_adapter(2, 3)
    eng.clear_adapter(3)
    with pytest.raises(ValueError, match="empty slot"):           # a row that still names the cleared adapter
        eng.forward(toks, kv)
    kv.close()
    utils.load_adapter_into(model, 3, bank.adapter(name, "Q"))
    _assert_same_bits(before, _bits(model, cfg, ads_of), "after the refusals")
    eng.close()
    wide = utils.load_model(bank.tiny[name][0], max_positions=MAX_POS)
    wide.engine.set_lora(last, "mlp.gate_proj", a, b, 10.0)
    with pytest.raises(NotImplementedError, match="exclude"):     # the table after the engine-wide adapter
        wide.engine.set_adapter_lora(0, last, "mlp.gate_proj", a, b, 10.0)
    wide.engine.forward(toks, wide.engine.new_kv(3, capacity=16, kv_dtype="model"))
    wide.engine.close()
