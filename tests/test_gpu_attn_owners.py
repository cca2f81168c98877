"""Decode attention, matrix-core variant (-m gpu): the prologue runs in the lane groups that own a vector and nowhere else.

Lane group (wave, gq) owns vector 4 wave + gq: a query head (< G), the new key (G) or the new value (G + 1) -- the last two
only in the split that owns the new position (tests/attn_owner_cases.py restates the map; tests/test_attn_owners_cases.py
checks it without a device).  Everything else of the workgroup skips the prologue, and a split that does not own the new
position neither loads nor scores the new key: its ninth merge slot is written neutral.

B = 3 sequences, 2 kv heads, G in {1, 2, 3, 4, 5, 6, 8} (the G + 2 vectors end inside wave 0, at its end, inside wave 1, at
its end, in wave 2), head_dim 64 / 128 and 96 where it is served, float32 / bfloat16 / float16 caches, 0 .. 273 cached
tokens (nothing cached, one key, both sides of a 16-key tile, two rounds and a ragged tile behind them), 1, 2 and 4 splits,
through mi_op_attention_decode (rows and lengths from device memory) and mi_op_attention_decode_host (from the arguments).

Reference and bounds are those of the existing kernel-level tests of the same call: the float64 oracle of
tests/attn16_cases.py; float32 within rtol 1e-5 / atol 2e-6 and the new K row within rtol 2e-5 / atol 4e-5
(tests/test_gpu_attn_f32_blocks.py, tests/test_gpu_attn_gqa.py), 16-bit caches under cases.assert_rule and
attn16_cases.check_new_rows.  At every split count the same bounds hold, and in addition
  * the two entry points agree bit for bit, and so does the same call made twice;
  * the cache rows at pos are bit for bit what the call with one split appends;
  * every other cache row, and the sentinel margins around the output and both caches, are untouched.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn16_cases as cases  # noqa: E402
import attn_owner_cases as own  # noqa: E402
from gpu_helpers import TDT, attention_decode, attn_shape, dev_i32, host, rope_tables  # noqa: E402

B, HKV = 3, 2
POS = [0, 1, 15, 16, 17, 256, 273]
MIXED = [(0, 17, 273), (256, 1, 16), (15, 273, 0)]      # rows of different pos in one call: every value of POS once or twice
SPLITS = [1, 2, 4]
CAP = max(POS) + 8
MARGIN = 256                                           # sentinel elements on both sides of the output and of each cache
SENTINEL = 7.0
ACTS = ["float32", "bfloat16", "float16"]
GEOMS = [(G, D) for D in (64, 96, 128) for G in own.GS if own.served(D, G)]


class _Fenced:
    """A device array with MARGIN sentinel elements in front of it and behind it."""

    def __init__(self, a, act):
        self.n, self.shape = a.size, a.shape
        self.buf = torch.full((MARGIN + self.n + MARGIN,), SENTINEL, dtype=TDT[act], device="cuda")
        self.buf[MARGIN:MARGIN + self.n] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TDT[act]).cuda().flatten()

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + MARGIN * self.buf.element_size())

    def get(self):
        return host(self.buf[MARGIN:MARGIN + self.n]).reshape(self.shape)

    def margins_intact(self):
        return bool((self.buf[:MARGIN] == SENTINEL).all()) and bool((self.buf[MARGIN + self.n:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _case(G, D, act, lens):
    """Inputs and the float64 oracle's outputs / caches for one batch of lengths, computed once, shared, read-only."""
    Hq = G * HKV
    inp = cases.random_inputs(Hq, HKV, D, act, B, 1, B, CAP, seed=61 + sum(lens))
    want, kc_ref, vc_ref = cases.attention_oracle(inp, Hq, HKV, D, act, False, list(lens))
    for a in (want, kc_ref, vc_ref):
        a.setflags(write=False)
    return inp, want[:, 0], kc_ref, vc_ref


def _launch(G, D, act, lens, inp, nsplit, entry, repeat=1):
    """`repeat` launches on the same buffers -> ([outputs], K cache, V cache); margins and tickets checked after each."""
    Hq = G * HKV
    cos, sin = rope_tables(D, CAP + 8, cases.rope_base(False))
    s = attn_shape(B, 1, Hq, HKV, D, act, act, 0, CAP)
    kc, vc = _Fenced(inp["kc"], act), _Fenced(inp["vc"], act)
    out = _Fenced(np.zeros((B, Hq * D), np.float32), act)
    qkv_d = torch.from_numpy(inp["qkv"][:, 0]).to(TDT[act]).cuda().contiguous()
    if entry == "host":                                    # no device rows, zeroed device lengths: only the arguments can serve
        off_d, hrow, hoff = dev_i32(np.zeros(B)), (C.c_int32 * B)(*range(B)), (C.c_int32 * B)(*lens)
    else:
        off_d, hrow, hoff = dev_i32(lens), None, None

    def read():
        assert out.margins_intact() and kc.margins_intact() and vc.margins_intact(), (entry, nsplit, lens)
        return out.get()

    outs = attention_decode(s, qkv_d, kc.ptr(), vc.ptr(), off_d, cos, sin, nsplit, hrow=hrow, hoff=hoff, repeat=repeat,
                            out=out.ptr(), read=read)
    return (outs if repeat > 1 else [outs]), kc.get(), vc.get()


def _check_batch(G, D, act, lens):
    inp, want, kc_ref, vc_ref = _case(G, D, act, tuple(lens))
    what = f"owners G {G} D {D} {act} pos {list(lens)}"
    appended = None
    for nsplit in SPLITS:
        (dev_out,), gk, gv = _launch(G, D, act, lens, inp, nsplit, "device")
        (first, second), hk, hv = _launch(G, D, act, lens, inp, nsplit, "host", repeat=2)
        assert np.array_equal(first, dev_out), (what, nsplit, "entry points differ")
        assert np.array_equal(second, first), (what, nsplit, "the same call twice differs")
        assert np.array_equal(hk, gk) and np.array_equal(hv, gv), (what, nsplit)
        rows = (np.stack([gk[b, :, n] for b, n in enumerate(lens)]), np.stack([gv[b, :, n] for b, n in enumerate(lens)]))
        if appended is None:
            appended = rows
        assert np.array_equal(rows[0], appended[0]) and np.array_equal(rows[1], appended[1]), (what, nsplit, "appended rows")
        # the new rows within the bound of the existing tests, every other row exactly the input's
        if act == "float32":
            assert np.array_equal(gv, vc_ref), (what, nsplit)
            for b, n in enumerate(lens):
                assert np.allclose(gk[b, :, n], kc_ref[b, :, n], rtol=2e-5, atol=4e-5), (what, nsplit, b)
                gk[b, :, n] = kc_ref[b, :, n]
            assert np.array_equal(gk, kc_ref), (what, nsplit)
            err = np.abs(dev_out - want)
            print(f"{what} nsplit {nsplit}: max |err| {err.max():.3e}, max err / (1e-5 |want| + 2e-6) "
                  f"{float((err / (1e-5 * np.abs(want) + 2e-6)).max()):.3f}")
            assert np.allclose(dev_out, want, rtol=1e-5, atol=2e-6), (what, nsplit, err.max())
        else:
            cases.check_new_rows(gk, gv, kc_ref, vc_ref, range(B), lens, act)
            cases.assert_rule(dev_out, want, act, f"{what} nsplit {nsplit}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("G,D", GEOMS)
def test_every_pos_and_split_count_through_both_entry_points(G, D, act):
    for pos in POS:
        _check_batch(G, D, act, (pos,) * B)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("G,D", GEOMS)
def test_rows_of_different_pos_in_one_call(G, D, act):
    """Splits that own the new position of one row hold no key of another: the owner split of a short row is an empty
    split beside occupied ones of a long row in the same launch."""
    for lens in MIXED:
        _check_batch(G, D, act, lens)
