"""The oracle-backed fake engine (fake_engine.py) with per-request adapters, for the scheduler and server tests on CPU: a KV
whose rows name an adapter slot (``set_row_adapter``, cleared by ``reset_row``, checked by ``fork_row``), a paged form with a
prefix lookup that only records its calls, and an engine that runs every row on the oracle of the row's adapter.  Test
infrastructure: never importable from the product package."""
import copy

from fake_engine import FakeEngine, FakeModel, FakeSlotKV
from oracle import ref_generate


class RowCache(list):
    """One row's per-layer oracle caches, tagged with the adapter slot the row names."""
    adapter = -1


class _ByRow:
    """What the fake engine calls as its oracle: the oracle of the adapter that the fed row names."""

    def __init__(self, engine):
        self.engine = engine

    def __call__(self, tokens, cache=None):
        slot = getattr(cache, "adapter", -1)
        self.engine.ran.append(slot)
        return self.engine.refs[slot](tokens, cache=cache)

    def make_cache(self, batch, paged=False):
        return RowCache(self.engine.refs[-1].make_cache(batch, paged=paged))


class AdapterKV(FakeSlotKV):
    block_tokens = 16

    def __init__(self, engine, batch_size):
        super().__init__(engine, batch_size)
        self.forks = []

    @property
    def adapters(self):
        return [r.adapter for r in self.rows]

    def set_row_adapter(self, row, slot):
        if not -1 <= slot < 16 or self.offsets[row] != 0:
            raise ValueError("set_row_adapter: bad slot, or the row is not empty")
        self.rows[row].adapter = slot
        self.engine.trace.append(("set_row_adapter", row, slot))

    def fork_row(self, src, dst, n_tokens):
        offs = self.offsets
        if src == dst or offs[dst] != 0 or not 1 <= n_tokens <= offs[src]:
            raise ValueError("fork_row: bad argument")
        if self.rows[dst].adapter != self.rows[src].adapter:
            raise ValueError("fork_row: dst names another adapter than src")
        self.forks.append((src, dst, n_tokens))
        self.engine.trace.append(("fork_row", src, dst, n_tokens))
        row = copy.deepcopy(self.rows[src])
        for c in row:
            c.offset = n_tokens
        self.rows[dst] = row

    # the paged surface the scheduler uses; nothing is ever reused
    def prefix_attach(self, row, tokens):
        self.engine.trace.append(("prefix_attach", row, self.rows[row].adapter))
        return 0

    def prefix_publish(self, row, tokens):
        self.engine.trace.append(("prefix_publish", row, self.rows[row].adapter))

    def stats(self):
        return {"free_blocks": 1 << 20, "usable_blocks": 1 << 20, "cached_blocks": 0, "reused_tokens": 0, "lookup_tokens": 0,
                "evictions": 0, "evictable_blocks": 0}


class _Engine(FakeEngine):
    """``refs``: adapter slot -> oracle (-1: the base model).  ``loaded`` records what ``load_adapter_into`` sent."""

    def __init__(self, refs):
        super().__init__(None)
        self.refs = refs
        self.ref = _ByRow(self)
        self.ran = []                          # the adapter slot of every oracle call, in order
        self.loaded = []

    def clear_adapter(self, slot):
        self.loaded.append(("clear", slot))

    def set_adapter_lora(self, slot, layer, proj, a, b, scale):
        self.loaded.append((slot, layer, proj, tuple(a.shape), tuple(b.shape), scale))


class AdapterEngine(_Engine):
    def new_kv(self, batch_size, capacity=256, kv_dtype="model", step=256):
        return AdapterKV(self, batch_size)

    def new_paged_kv(self, slots, block_tokens=64, n_blocks=None, max_tokens_per_row=None, kv_dtype="model"):
        return AdapterKV(self, slots)


class PlainKVEngine(_Engine):
    """An engine whose caches know no adapters (and no paging)."""

    def new_kv(self, batch_size, capacity=256, kv_dtype="model", step=256):
        return FakeSlotKV(self, batch_size)


def adapter_model(model_dir, adapter_dirs, engine_class=AdapterEngine, max_pos=2048):
    """A FakeModel whose engine runs slot s on the oracle loaded with adapter_dirs[s]"""
    m = FakeModel(model_dir, max_pos=max_pos)
    refs = {-1: m.ref}
    for slot, path in adapter_dirs.items():
        refs[slot] = ref_generate.load(model_dir, adapter_path=path, max_pos=max_pos)
    m.engine = engine_class(refs)
    return m
