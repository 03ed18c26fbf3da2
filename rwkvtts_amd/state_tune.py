"""State tuning: every weight frozen, the initial recurrent states of named voices are the trained tensors.

A tuned voice is exactly one StateStore row, so serving it costs what ContinuousDecoder.submit(state=name) costs already.  A
StateTuner keeps, per voice, an fp32 MASTER of the three state fields of every layer (att_x_prev [D], att_kv [H,64,64], ffn_x_prev
[D]) and fp32 AdamW moments for the tuned fields, trains many voices at once on mixed batches through the model's own differentiable
stateful forward, and writes every updated state straight into the store row a running engine serves from.

One step is: rwkv7_state_rows_expand_f32 (master rows -> a B-row bf16 cache, one row per sequence, zeros for a sequence without a
voice), the model's forward with past_key_values = that cache, loss.backward(), rwkv7_state_rows_adamw_f32 (the gradients of a voice's
rows added in a fixed order, AdamW with the voice's own step count, the new state into master and store row) -- two launches beside
the model's, no atomics, nothing read back on the host.  On a CPU model the same arithmetic runs in torch so that the host logic is
testable; on the HIP device there is no fallback.

Out of scope: more than one rank (no gradient exchange), the XY and Cosy engines (they have no store), gradient clipping, and what
the existing autograd nodes compute while the weights are frozen.

Like the store, the tuner issues its device work on the current stream and is meant to be used from the stream the engine steps on.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch

from .backbone import Cache, LayerState
from .state_store import StateStore

FORMAT = 1
FIELDS = ("att_x_prev", "att_kv", "ffn_x_prev")   # the order of the kernels' tables


def build_csr(voice: Sequence[int], store_row: Dict[int, int], steps: Dict[int, int]):
    """The device CSR of rwkv7_state_rows_adamw_f32 from host knowledge.  voice[i]: the master row of batch row i, or -1 for a
    sequence without a voice; store_row / steps: per master row its store row and the updates it has had.  Returns (seg_start
    [A + 1], seg_rows, seg_info [A][3] = {master row, store row, step count of THIS update}) as lists; active voices in ascending
    master row, a voice's batch rows ascending."""
    rows: Dict[int, List[int]] = {}
    for i, v in enumerate(voice):
        if v >= 0:
            rows.setdefault(int(v), []).append(i)
    seg_start, seg_rows, seg_info = [0], [], []
    for v in sorted(rows):
        seg_rows += rows[v]
        seg_start.append(len(seg_rows))
        seg_info.append([v, int(store_row[v]), int(steps[v]) + 1])
    return seg_start, seg_rows, seg_info


class StateTuner:
    """tuner = StateTuner(model, store, lr=1e-2); tuner.add("anna"); loss = tuner.step(voices=["anna", None, ...], **batch)

    model: the RWKV7ForSpeech / RWKV7ForCausalLM the store was built for (bf16 on the HIP device).  store: the StateStore whose rows
    receive the tuned states.  lr, betas, eps, weight_decay: torch.optim.AdamW's (decoupled decay); `lr` is a plain attribute and
    may be changed between steps.  fields: which of att_x_prev / att_kv / ffn_x_prev are tuned -- the WKV state alone by default;
    the other fields of a voice stay what they were when it was added.  capacity: voices the tuner can hold (default: the store's
    rows)."""

    def __init__(self, model, store: StateStore, lr: float = 1e-2, betas=(0.9, 0.95), eps: float = 1e-18, weight_decay: float = 0.0,
                 fields: Sequence[str] = ("att_kv",), capacity: Optional[int] = None):
        why = store.compatible(model.config, model.dtype, model.device)
        if why is not None:
            raise ValueError(f"StateTuner: {why}")
        fields = tuple(fields)
        if not fields or any(f not in FIELDS for f in fields) or len(set(fields)) != len(fields):
            raise ValueError(f"fields must be a non-empty subset of {FIELDS}, got {fields}")
        self.model, self.store, self.config = model, store, model.config
        self.device, self.dtype = torch.device(model.device), model.dtype
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.fields = tuple(f for f in FIELDS if f in fields)
        self.capacity = int(store.capacity if capacity is None else capacity)
        if self.capacity < 1:
            raise ValueError("capacity must be >= 1")
        self.hip = self.device.type == "cuda"
        cfg, V = self.config, self.capacity
        shape = {"att_x_prev": (V, cfg.hidden_size), "att_kv": (V, cfg.num_heads, 64, 64), "ffn_x_prev": (V, cfg.hidden_size)}
        new = lambda f: torch.zeros(shape[f], dtype=torch.float32, device=self.device)
        L = cfg.num_hidden_layers
        self.master = [{f: new(f) for f in FIELDS} for _ in range(L)]
        self.exp_avg = [{f: new(f) for f in self.fields} for _ in range(L)]       # moments exist for the tuned fields only
        self.exp_avg_sq = [{f: new(f) for f in self.fields} for _ in range(L)]
        self._rows: Dict[str, int] = {}                  # name -> master row
        self._free: List[int] = list(range(V))
        self.steps: List[int] = [0] * V                  # per master row: updates so far
        self.nan_flag = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.last_leaves = None                          # per layer {field: leaf} of the last step's cache; .grad is its gradient
        self._tables = None

    # ---- bookkeeping (host only) ---------------------------------------------------------------------------------------------------
    def names(self) -> List[str]:
        return list(self._rows)

    def __contains__(self, name) -> bool:
        return name in self._rows

    def row(self, name: str) -> int:
        try:
            return self._rows[name]
        except KeyError:
            raise KeyError(f"no tuned voice named {name!r} (tuned: {self.names()}): add() it first") from None

    def step_count(self, name: str) -> int:
        return self.steps[self.row(name)]

    @torch.no_grad()
    def add(self, name: str, init: str = "store") -> int:
        """Start tuning `name`: its master row.  init="store": from the row the store holds under that name (a captured voice
        prompt); init="zeros": from the zero state, which is also written to the store (the name is reserved there if it is new).
        Moments and step count start at zero.  A name that is already tuned, or pinned by queued requests, raises."""
        if init not in ("store", "zeros"):
            raise ValueError(f"init must be 'store' or 'zeros', got {init!r}")
        if name in self._rows:
            raise ValueError(f"voice {name!r} is tuned already")
        if not self._free:
            raise RuntimeError(f"the tuner is full ({self.capacity} voices)")
        if init == "store":
            srow = self.store.row(name)                  # KeyError for a name the store does not hold
            self._not_pinned(name)
        else:
            srow = self.store.reserve(name)              # RuntimeError for a pinned name or a full store
        v = self._free.pop(0)
        self._rows[name] = v
        self.steps[v] = 0
        for l, st in enumerate(self.store.cache.states):
            for f in FIELDS:
                if init == "zeros":
                    getattr(st, f)[srow].zero_()
                self.master[l][f][v].copy_(getattr(st, f)[srow])
            for f in self.fields:
                self.exp_avg[l][f][v].zero_()
                self.exp_avg_sq[l][f][v].zero_()
        return v

    def remove(self, name: str):
        """Stop tuning `name` and free its master row; the store keeps the state it holds."""
        v = self.row(name)
        del self._rows[name]
        self._free.append(v)
        self._free.sort()

    def _not_pinned(self, name: str):
        if self.store.pinned(name):
            raise RuntimeError(f"state {name!r} is pinned by {self.store.pinned(name)} queued request(s): it cannot be tuned now")

    def _store_row(self, name: str) -> int:
        if name not in self.store:
            raise KeyError(f"voice {name!r} was evicted from the state store: put it back (StateTuner.publish) or remove() it")
        self._not_pinned(name)
        return self.store.row(name)

    def plan(self, voices: Sequence[Optional[str]]):
        """Host side of a step: (voice [B] -- master row or -1 per sequence --, seg_start, seg_rows, seg_info) for build_csr's
        kernel arguments.  Raises for a name that is not tuned, was evicted from the store or is pinned there."""
        voice = [-1 if n is None else self.row(n) for n in voices]
        store_row = {self._rows[n]: self._store_row(n) for n in dict.fromkeys(n for n in voices if n is not None)}
        return (voice,) + build_csr(voice, store_row, {v: self.steps[v] for v in store_row})

    # ---- device side ---------------------------------------------------------------------------------------------------------------
    def _table(self, per_layer, fields=FIELDS):
        """A device table of 3 L addresses from per-layer {field: tensor} dicts; a field outside `fields` is NULL.  Uploaded
        non-blocking: a step waits for nothing."""
        ptrs = []
        for d in per_layer:
            for f in FIELDS:
                t = d[f] if f in fields else None
                if t is not None and (not t.is_contiguous() or t.data_ptr() % 16):
                    raise ValueError(f"state tuning: field {f} of {tuple(t.shape)} is not contiguous and 16-byte aligned")
                ptrs.append(0 if t is None else t.data_ptr())
        return torch.tensor(ptrs, dtype=torch.int64).to(self.device, non_blocking=True)

    @property
    def tables(self):
        """(master, exp_avg, exp_avg_sq) device tables, built on first use (the tensors never move)."""
        if self._tables is None:
            self._tables = (self._table(self.master), self._table(self.exp_avg, self.fields), self._table(self.exp_avg_sq, self.fields))
        return self._tables

    def _geom(self):
        return self.config.num_hidden_layers, self.config.hidden_size, self.config.num_heads

    @torch.no_grad()
    def expand(self, voice: Sequence[int], cache: Optional[Cache] = None, voice_dev=None) -> Cache:
        """Rows of a bf16 cache from master rows: entry i is master row voice[i], -1 a zero row, below -1 row i of `cache` is kept.
        cache: None = a new len(voice)-row cache (every entry >= -1 then).  The hand-over of a step, and of publish()."""
        n, (L, D, H) = len(voice), self._geom()
        if any(v >= self.capacity for v in voice):
            raise ValueError(f"voice rows {list(voice)}: the master holds {self.capacity}")
        if cache is None:
            if any(v < -1 for v in voice):
                raise ValueError("a new cache has no rows to keep")
            new = lambda dt, *s: torch.empty(n, *s, dtype=dt, device=self.device)
            cache = Cache([LayerState(new(self.dtype, D), new(torch.float32, H, 64, 64), new(self.dtype, D)) for _ in range(L)])
        if cache[0].att_kv.shape[0] != n:
            raise ValueError(f"{n} entries for a cache of {cache[0].att_kv.shape[0]} rows")
        if self.hip:
            from . import _lib
            if voice_dev is None:
                voice_dev = torch.tensor(list(voice), dtype=torch.int32).to(self.device, non_blocking=True)
            if cache is self.store.cache:
                dst = self.store.table
            else:
                dst = self._table([{f: getattr(st, f) for f in FIELDS} for st in cache.states])
            _lib.call("rwkv7_state_rows_expand_f32", dst, L, n, self.tables[0], dst, voice_dev, D, H)
            return cache
        keep = [i for i, v in enumerate(voice) if v >= -1]
        if keep:
            at = torch.tensor(keep)
            src = torch.tensor([max(voice[i], 0) for i in keep])
            zero = torch.tensor([voice[i] < 0 for i in keep])
            for l, st in enumerate(cache.states):
                for f in FIELDS:
                    dst = getattr(st, f)
                    rows = self.master[l][f].index_select(0, src).to(dst.dtype)   # one round-to-nearest-even for the shift rows
                    rows[zero] = 0
                    dst.index_copy_(0, at, rows)
        return cache

    @torch.no_grad()
    def publish(self, names: Optional[Sequence[str]] = None):
        """Write the masters of `names` (default: every tuned voice) into their store rows, reserving a row for a name the store
        does not hold: after load_state_dict() into a fresh store, or after an eviction."""
        names = self.names() if names is None else list(names)
        voice = [-2] * self.store.capacity
        for n in names:
            v = self.row(n)
            voice[self.store.reserve(n, self.store.tokens[self.store.row(n)] if n in self.store else 0)] = v
        self.expand(voice, self.store.cache)

    def _leaf_cache(self, voice, voice_dev) -> Cache:
        cache = self.expand(voice, voice_dev=voice_dev)
        for st in cache.states:
            for f in self.fields:
                getattr(st, f).requires_grad_()
        return cache

    def step(self, voices: Sequence[Optional[str]], **batch) -> torch.Tensor:
        """One optimisation step of the voices named in `voices` (one entry per sequence of the batch: batch row b of a padded
        [B, T] batch, sequence s of a packed cu_seqlens row; None: that sequence starts from zero and tunes nothing, but counts in
        the loss mean).  batch: what model.forward takes, labels included; past_key_values is the tuner's.  Every parameter is
        frozen and the model is in eval mode for the duration of the call; both are restored, also on an exception.  A non-finite
        loss makes the step run on a zero gradient (a device flag; nothing is read back).  Returns the detached loss."""
        if "past_key_values" in batch:
            raise ValueError("step builds past_key_values itself")
        B = self._batch_rows(batch)
        voices = list(voices)
        if len(voices) != B:
            raise ValueError(f"{len(voices)} voices for a batch of {B} sequences: one entry (a name or None) per sequence")
        voice, seg_start, seg_rows, seg_info = self.plan(voices)
        A, n_act = len(seg_info), len(seg_rows)
        host = torch.tensor(voice + seg_start + seg_rows + [x for info in seg_info for x in info], dtype=torch.int32)
        dev = host.to(self.device, non_blocking=True)
        voice_dev, seg_start_dev = dev[:B], dev[B:B + A + 1]
        seg_rows_dev, seg_info_dev = dev[B + A + 1:B + A + 1 + n_act], dev[B + A + 1 + n_act:]
        cache = self._leaf_cache(voice, voice_dev)
        # the forward rebinds a differentiable cache's fields to the new states: the leaves are kept here
        leaves = [{f: getattr(st, f) for f in self.fields} for st in cache.states]
        model = self.model
        flags = [(p, p.requires_grad) for p in model.parameters()]
        was = model.training
        try:
            for p, _ in flags:
                p.requires_grad_(False)
            model.eval()
            with torch.enable_grad():
                loss = model(past_key_values=cache, **batch).loss
                if loss is None:
                    raise ValueError("the batch carries no labels: the model returned no loss")
                self.nan_flag.copy_((~torch.isfinite(loss.detach())).reshape(1))
                if A:
                    loss.backward()
        finally:
            for p, f in flags:
                p.requires_grad_(f)
            model.train(was)
        self.last_leaves = leaves
        if A:
            grads = [{f: self._grad(t) for f, t in d.items()} for d in leaves]
            self._apply(grads, B, seg_start, seg_rows, seg_info, (seg_start_dev, seg_rows_dev, seg_info_dev), self.nan_flag)
            for v, _, t in seg_info:
                self.steps[v] = t
        return loss.detach()

    @staticmethod
    def _batch_rows(batch) -> int:
        cu = batch.get("cu_seqlens")
        if cu is not None:
            return int(cu.numel()) - 1
        x = batch.get("input_ids")
        x = batch.get("inputs_embeds") if x is None else x
        if x is None:
            raise ValueError("the batch needs input_ids or inputs_embeds")
        return int(x.shape[0])

    @staticmethod
    def _grad(leaf):
        g = leaf.grad
        if g is None:                                    # the field did not reach the loss: a zero gradient, as AdamW sees it
            return torch.zeros_like(leaf)
        return g if g.is_contiguous() and g.data_ptr() % 16 == 0 else g.contiguous().clone()

    @torch.no_grad()
    def _apply(self, grads, n, seg_start, seg_rows, seg_info, dev, skip_flag, grad_scale: float = 1.0):
        """The optimizer step: grads per layer {field: leaf gradient [n, ...]}, the CSR as host lists and (HIP) as device tensors."""
        L, D, H = self._geom()
        b1, b2 = self.betas
        if self.hip:
            from . import _lib
            gtbl = self._table(grads, self.fields)
            _lib.call("rwkv7_state_rows_adamw_f32", gtbl, L, n, len(seg_info), gtbl, *self.tables, self.store.table, *dev, skip_flag,
                      self.lr, b1, b2, self.eps, self.weight_decay, grad_scale, D, H)
            return
        skip = bool(skip_flag.item()) if skip_flag is not None else False
        for a, (v, srow, t) in enumerate(seg_info):
            rows = torch.tensor(seg_rows[seg_start[a]:seg_start[a + 1]])
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
            for l in range(L):
                for f in self.fields:
                    picked = grads[l][f].index_select(0, rows).float()
                    g = torch.zeros_like(picked[0])
                    for r in range(picked.shape[0]):     # sequentially, in the listed order
                        g = g + picked[r]
                    g = torch.zeros_like(g) if skip else g * grad_scale
                    p, m, s = self.master[l][f][v], self.exp_avg[l][f][v], self.exp_avg_sq[l][f][v]
                    p.mul_(1.0 - self.lr * self.weight_decay)
                    m.mul_(b1).add_(g, alpha=1.0 - b1)
                    s.mul_(b2).addcmul_(g, g, value=1.0 - b2)
                    p.addcdiv_(m, (s.sqrt() / math.sqrt(bc2)).add_(self.eps), value=-self.lr / bc1)
                    if srow >= 0:
                        dst = getattr(self.store.cache[l], f)
                        dst[srow].copy_(p)               # one round-to-nearest-even for the shift rows

    # ---- persistence ---------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """Masters, moments, per-voice step counts, names, fields, hyper-parameters and the store's fingerprint: tensors (on the
        CPU, the used rows in the order of `names`) and plain Python data only."""
        names = self.names()
        idx = torch.tensor([self._rows[n] for n in names], dtype=torch.int64).to(self.device)
        pick = lambda per_layer, f: torch.stack([d[f].index_select(0, idx) for d in per_layer]).cpu()
        return {"format": FORMAT, "fingerprint": dict(self.store.fingerprint), "names": names, "fields": list(self.fields),
                "steps": [self.steps[self._rows[n]] for n in names],
                "hyper": {"lr": self.lr, "betas": list(self.betas), "eps": self.eps, "weight_decay": self.weight_decay},
                "master": {f: pick(self.master, f) for f in FIELDS},
                "exp_avg": {f: pick(self.exp_avg, f) for f in self.fields},
                "exp_avg_sq": {f: pick(self.exp_avg_sq, f) for f in self.fields}}

    @torch.no_grad()
    def load_state_dict(self, sd: dict, publish: bool = True):
        """Replace what the tuner holds by what state_dict() returned (hyper-parameters included).  ValueError for another format,
        geometry or dtype, other tuned fields, or more voices than the capacity.  publish: write the masters into the store's rows
        (reserving rows for names it does not hold), so that the store serves what the tuner continues from."""
        if sd.get("format") != FORMAT or sd.get("fingerprint") != self.store.fingerprint:
            raise ValueError(f"tuned states of {sd.get('fingerprint')} (format {sd.get('format')}), the store holds {self.store.fingerprint}")
        if tuple(sd["fields"]) != self.fields:
            raise ValueError(f"the saved tuner tuned {tuple(sd['fields'])}, this one tunes {self.fields}")
        names, steps = list(sd["names"]), [int(t) for t in sd["steps"]]
        n = len(names)
        if len(steps) != n or len(set(names)) != n or n > self.capacity:
            raise ValueError(f"{n} saved voices ({len(steps)} step counts) for a tuner of {self.capacity}")
        L = self.config.num_hidden_layers
        for key, per_layer, fields in (("master", self.master, FIELDS), ("exp_avg", self.exp_avg, self.fields), ("exp_avg_sq", self.exp_avg_sq, self.fields)):
            for f in fields:
                t = sd[key][f]
                if t.dtype != torch.float32 or tuple(t.shape) != (L, n) + tuple(per_layer[0][f].shape[1:]):
                    raise ValueError(f"{key}[{f}] of {tuple(t.shape)} / {t.dtype} does not fit the model")
        self._rows = {name: i for i, name in enumerate(names)}
        self._free = list(range(n, self.capacity))
        self.steps = steps + [0] * (self.capacity - n)
        for key, per_layer, fields in (("master", self.master, FIELDS), ("exp_avg", self.exp_avg, self.fields), ("exp_avg_sq", self.exp_avg_sq, self.fields)):
            for f in fields:
                for l in range(L):
                    per_layer[l][f][:n].copy_(sd[key][f][l])
        h = sd["hyper"]
        self.lr, self.betas, self.eps, self.weight_decay = float(h["lr"]), (float(h["betas"][0]), float(h["betas"][1])), float(h["eps"]), float(h["weight_decay"])
        if publish:
            self.publish()
