"""Stored recurrent states: prefill a shared prefix once, start every later request from it.

An RWKV state has a fixed size -- per cache row and layer two bf16 [D] vectors and one fp32 [H,64,64] -- so the state after a voice
prompt or an instruction block can be kept and reused: ContinuousDecoder(model, state_store=store).submit(state="voice", input_ids=
suffix) continues from the stored row instead of prefilling the prefix again.

A StateStore is a Cache of `capacity` rows plus host bookkeeping (name -> row, a free list, tokens per row, pin counts).  Rows get
in by capture() (the model's own packed-row forward into the row), by put() (a row of any compatible Cache, for instance a tuned
initial state) or by load(); they get out through rwkv7_cache_rows_seed_bf16 (csrc/cache_rows.hip), which copies stored rows and
zero rows into an engine's rows in one launch with the choice as device data.  A running engine can also write a row itself: a
request submitted with retain=name holds a PENDING row (reserve_pending) that the engine's captured step fills when the request ends
(rwkv7_cache_rows_retain_bf16) and publish() then turns into an ordinary stored state.

The store issues its device work on the current stream and is meant to be used from the stream the engine steps on: a capture()
issued before a submit() is then visible to the admission that reads it (overlapped admission orders its side stream after that
stream).  A name is pinned while queued requests refer to it; evict() of a pinned name raises, so a row is never reused under a
request that has not read it yet.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .backbone import Cache

FORMAT = 1


def fingerprint(cfg, dtype) -> dict:
    """What a stored row depends on: the cache geometry and the element type of the token-shift rows."""
    return {"format": FORMAT, "layers": int(cfg.num_hidden_layers), "D": int(cfg.hidden_size), "H": int(cfg.num_heads),
            "dtype": str(dtype)}


class StateStore:
    """store = StateStore(model, capacity); store.capture("voice", input_ids=prefix); eng = ContinuousDecoder(model, state_store=store)

    model: the RWKV7ForSpeech / RWKV7ForCausalLM the engines run (its config, device and dtype size the cache; capture() runs its
    backbone).  capacity: rows, fixed at construction; a full store raises rather than evicting on its own."""

    def __init__(self, model, capacity: int):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("capacity must be >= 1")
        self.model, self.capacity = model, capacity
        self.config, self.device, self.dtype = model.config, model.device, model.dtype
        self.cache = Cache.zeros(self.config, capacity, self.device, self.dtype)
        self.fingerprint = fingerprint(self.config, self.dtype)
        self._rows: Dict[str, int] = {}          # name -> row, in insertion order
        self._free: List[int] = list(range(capacity))   # ascending; a new name takes the lowest free row
        self.tokens: List[int] = [0] * capacity  # per row: tokens the state has seen (bookkeeping only)
        self._pins: Dict[str, int] = {}          # name -> queued requests that refer to it
        self._pending: Dict[str, int] = {}       # name -> row held for a state an engine has yet to write (reserve_pending)
        self._table = None

    # ---- bookkeeping (host only) ---------------------------------------------------------------------------------------------------
    def __contains__(self, name) -> bool:
        return name in self._rows

    def __len__(self) -> int:
        return len(self._rows)

    def names(self) -> List[str]:
        return list(self._rows)

    def row(self, name: str) -> int:
        try:
            return self._rows[name]
        except KeyError:
            raise KeyError(f"no stored state named {name!r} (stored: {self.names()})") from None

    def reserve(self, name: str, tokens: int = 0) -> int:
        """Bind `name` to the lowest free row without writing the row (put / capture / load fill it): the row.  A name that is
        already stored keeps its row unless it is pinned; a full store raises."""
        if not isinstance(name, str) or not name:
            raise ValueError(f"a state's name is a non-empty string, got {name!r}")
        if name in self._pending:
            raise ValueError(f"state {name!r} is pending: a running request will write it (publish or abandon it first)")
        if name in self._rows:
            if self._pins.get(name):
                raise RuntimeError(f"state {name!r} is pinned by {self._pins[name]} queued request(s): it cannot be replaced")
            row = self._rows[name]
        else:
            if not self._free:
                raise RuntimeError(f"the state store is full ({self.capacity} rows): evict a name first")
            row = self._free.pop(0)
            self._rows[name] = row
        self.tokens[row] = int(tokens)
        return row

    def evict(self, name: str):
        """Forget `name` and free its row.  KeyError for an unknown name, RuntimeError while queued requests refer to it."""
        row = self.row(name)
        if self._pins.get(name):
            raise RuntimeError(f"state {name!r} is pinned by {self._pins[name]} queued request(s): it cannot be evicted")
        del self._rows[name]
        self.tokens[row] = 0
        self._free.append(row)
        self._free.sort()

    def pin(self, name: str) -> int:
        """A queued request refers to `name` from now on (ContinuousDecoder.submit): its row."""
        row = self.row(name)
        self._pins[name] = self._pins.get(name, 0) + 1
        return row

    def unpin(self, name: str):
        """The request's admission has read the row."""
        n = self._pins.get(name, 0)
        if n < 1:
            raise RuntimeError(f"state {name!r} is not pinned")
        if n == 1:
            del self._pins[name]
        else:
            self._pins[name] = n - 1

    def pinned(self, name: str) -> int:
        return self._pins.get(name, 0)

    # A PENDING name holds a row that a running request will write when it ends (ContinuousDecoder(..., retain=True).submit(retain=
    # name)).  Until publish() it is not servable: `in`, len(), names(), row(), pin() and save() do not see it, and the row is not free.
    def reserve_pending(self, name: str) -> int:
        """Take the lowest free row for `name` without making the name servable: the row.  ValueError for a name that is stored or
        already pending, RuntimeError when the store is full."""
        if not isinstance(name, str) or not name:
            raise ValueError(f"a state's name is a non-empty string, got {name!r}")
        if name in self._rows or name in self._pending:
            raise ValueError(f"state {name!r} is already {'stored' if name in self._rows else 'pending'}: evict it or choose another name")
        if not self._free:
            raise RuntimeError(f"the state store is full ({self.capacity} rows): evict a name first")
        row = self._free.pop(0)
        self._pending[name] = row
        return row

    def _take_pending(self, name: str) -> int:
        try:
            return self._pending.pop(name)
        except KeyError:
            raise KeyError(f"no pending state named {name!r} (pending: {self.pending()})") from None

    def publish(self, name: str, tokens: int = 0) -> int:
        """The pending row has been written: `name` is an ordinary stored state of `tokens` tokens from now on.  Its row."""
        row = self._take_pending(name)
        self._rows[name] = row
        self.tokens[row] = int(tokens)
        return row

    def abandon(self, name: str):
        """Give a pending name's row back (its request will never finish, for instance because its engine was dropped)."""
        self._free.append(self._take_pending(name))
        self._free.sort()

    def pending(self) -> List[str]:
        return list(self._pending)

    def compatible(self, cfg, dtype, device) -> Optional[str]:
        """None if rows of this store fit a cache of (cfg, dtype) on `device`, else why not."""
        fp = fingerprint(cfg, dtype)
        if fp != self.fingerprint:
            return f"the store holds states of {self.fingerprint}, the model needs {fp}"
        if torch.device(device) != torch.device(self.device):
            return f"the store lives on {self.device}, the model on {device}"
        return None

    # ---- device side ---------------------------------------------------------------------------------------------------------------
    @property
    def table(self) -> torch.Tensor:
        """The store's field table (prefill.cache_field_table), built on first use."""
        if self._table is None:
            from .prefill import cache_field_table
            self._table = cache_field_table(self.cache)
        return self._table

    def _seed_row(self, src_tbl, src_row: int, row: int):
        from .prefill import cache_rows_seed
        rows = torch.tensor([[src_row], [row]], dtype=torch.int32).to(self.device, non_blocking=True)
        cache_rows_seed(src_tbl, self.table, rows[0], rows[1], 1, len(self.cache), self.config.hidden_size, self.config.num_heads)

    @torch.no_grad()
    def put(self, name: str, cache: Cache, row: int = 0, tokens: int = 0) -> int:
        """Copy row `row` of `cache` (same depth, widths, dtype and device, for instance a tuned initial state) in as `name`, through
        rwkv7_cache_rows_seed_bf16: the store's row."""
        from .prefill import cache_field_table
        if cache is self.cache:
            raise ValueError("put copies a row of ANOTHER cache in")
        if len(cache) != len(self.cache) or not 0 <= int(row) < cache[0].att_kv.shape[0]:
            raise ValueError(f"put: a cache of {len(cache)} layers, row {row}: expected {len(self.cache)} layers and a row inside it")
        if cache[0].att_x_prev.shape[1:] != self.cache[0].att_x_prev.shape[1:] or cache[0].att_kv.shape[1:] != self.cache[0].att_kv.shape[1:]:
            raise ValueError("put: the cache's widths differ from the store's")
        plain = Cache([type(s)(s.att_x_prev.detach(), s.att_kv.detach(), s.ffn_x_prev.detach()) for s in cache.states])
        src_tbl = cache_field_table(plain)   # ValueError for a dtype, layout or device the kernel does not cover
        dst = self.reserve(name, tokens)
        self._seed_row(src_tbl, int(row), dst)
        return dst

    @torch.no_grad()
    def capture(self, name: str, input_ids=None, inputs_embeds=None) -> int:
        """Prefill a prompt (T ids [T] / [1, T] or embeddings [T, D] / [1, T, D]) from a zero state into a free row, as `name`: the row."""
        from .prefill import SEED_ZERO
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("pass exactly one of input_ids or inputs_embeds")
        m = self.model
        if inputs_embeds is None:
            e = m.get_input_embeddings()(torch.as_tensor(input_ids).reshape(-1).to(self.device))
        else:
            e = inputs_embeds.reshape(-1, inputs_embeds.shape[-1]).to(self.device, self.dtype)
        T = e.shape[0]
        if T < 1 or e.shape[1] != self.config.hidden_size:
            raise ValueError(f"prompt of shape {tuple(e.shape)}")
        row = self.reserve(name, T)
        self._seed_row(self.table, SEED_ZERO, row)   # a zero entry reads no source
        was = m.training
        m.eval()
        try:
            m.model(inputs_embeds=e.detach().unsqueeze(0), cu_seqlens=torch.tensor([0, T], dtype=torch.int32), past_key_values=self.cache,
                    cache_rows=torch.tensor([row]))
        except BaseException:
            self.evict(name)   # the row holds no finished state
            raise
        finally:
            m.train(was)
        return row

    # ---- persistence ---------------------------------------------------------------------------------------------------------------
    def save(self, path):
        """torch.save of the used rows (in name order of insertion), their names and tokens, and the fingerprint: tensors and plain
        Python data only."""
        names = self.names()
        idx = torch.tensor([self._rows[n] for n in names], dtype=torch.int64).to(self.device)
        pick = lambda f: torch.stack([getattr(s, f).index_select(0, idx) for s in self.cache.states]).cpu()
        torch.save({"fingerprint": dict(self.fingerprint), "names": names, "tokens": [self.tokens[self._rows[n]] for n in names],
                    "att_x_prev": pick("att_x_prev"), "att_kv": pick("att_kv"), "ffn_x_prev": pick("ffn_x_prev")}, path)

    @classmethod
    def load(cls, path, model, capacity: Optional[int] = None) -> "StateStore":
        """A store for `model` holding what save() wrote (capacity: at least the saved rows; default exactly those, at least 1).
        ValueError when the file was written for another geometry or dtype."""
        blob = torch.load(path, map_location="cpu", weights_only=True)
        want = fingerprint(model.config, model.dtype)
        if blob.get("fingerprint") != want:
            raise ValueError(f"{path}: stored states of {blob.get('fingerprint')}, the model needs {want}")
        names, tokens = list(blob["names"]), list(blob["tokens"])
        n = len(names)
        if len(tokens) != n or len(set(names)) != n or any(blob[f].shape[:2] != (want["layers"], n) for f in ("att_x_prev", "att_kv", "ffn_x_prev")):
            raise ValueError(f"{path}: names, tokens and rows do not match")
        if capacity is not None and capacity < n:
            raise ValueError(f"{path} holds {n} states, capacity = {capacity}")
        store = cls(model, max(1, n) if capacity is None else capacity)
        for name, t in zip(names, tokens):
            store.reserve(name, t)              # rows 0 .. n - 1, in the saved order
        with torch.no_grad():
            for l, s in enumerate(store.cache.states):
                for f in ("att_x_prev", "att_kv", "ffn_x_prev"):
                    if getattr(s, f).shape[1:] != blob[f].shape[2:] or getattr(s, f).dtype != blob[f].dtype:
                        raise ValueError(f"{path}: field {f} of {tuple(blob[f].shape)} / {blob[f].dtype} does not fit the model")
                    getattr(s, f)[:n].copy_(blob[f][l])
        return store
