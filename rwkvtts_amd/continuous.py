"""Continuous batching: a decode batch that admits new requests while it runs ("persistent multi-request decode").

GraphDecoder runs a closed batch until its longest sequence ends, so a slot whose request finished early idles until then.  Here
every one of up to 128 SLOTS (rows of the step kernel's batch) runs its own request:

  * one captured step: DecodeStep (WideDecodeStep above 32 slots: decode.step_for) on the live cache, then rwkv7_sample_slots_f32 (csrc/sampling.hip) on its logits, which draws
    every live slot's id with that slot's own key, step counter and sampling parameters and does the slot's bookkeeping (output
    column, next input embedding, step, live flag);
  * admission, eagerly between replays on the same stream: pending requests in FIFO order take free slots, their cache rows are
    reset to zero and prefilled as ONE packed row (RWKV7Model(..., cu_seqlens, past_key_values, cache_rows)), the head runs on each
    sequence's last position, and the same per-slot entry (with row_slot) draws the first id; with admission="graph" the prefill
    is prefill.PackedPrefill instead: graphs captured once per size class, replayed on this cache, no device read-back; with
    admission="overlap" that prefill runs on a side stream into a staging cache while the step keeps replaying, and the decode stream
    later copies the staged rows into the slots' rows in one launch (rwkv7_cache_rows_commit_bf16) and draws the first ids;
  * retirement: without EOS the host knows every budget and retires slots on the exact step with no read-back; with EOS it reads
    the live flags and step counters back every `check_every` replays;
  * with retain=True a last launch of the captured step (rwkv7_cache_rows_retain_bf16, csrc/cache_rows.hip) copies the cache row of a
    slot whose request just ended into a row of the attached StateStore, for requests submitted with retain=name.

A request's draws use (its seed, its step) only, so its ids do not depend on its slot or on when it was admitted.  Slots without a
request keep stepping on stale state; admission resets the row.  The scheduling lives in SlotScheduler, which never touches the
device.
"""
from __future__ import annotations

import collections
import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .backbone import Cache
from .decode import check_slots, step_class, step_for
from .sampling import MAX_TOP_K, RowSampler, fresh_seed


@dataclass
class Request:
    handle: int
    embeds: object            # [T, D] prompt embeddings (device tensor) -- opaque to the scheduler
    max_new_tokens: int
    min_new_tokens: int = 0
    do_sample: bool = False
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0
    group_size: int = 1             # candidates of one prompt that are admitted together (GroupScheduler); 1: a request of its own
    leader: Optional[int] = None    # handle of the group's first candidate, whose prefill this one shares; None: it prefills itself
    state: Optional[str] = None     # name of the stored state the prompt continues from (state_store.StateStore); None: from zero
    state_row: Optional[int] = None  # that state's row in the store, resolved (and pinned) at submit
    base_tokens: int = 0            # the tokens that stored state had seen, read at submit
    retain: Optional[str] = None    # name under which the state this request leaves behind is published (ContinuousDecoder retain=True)
    retain_row: Optional[int] = None  # the pending row of the store held for it since submit


def candidate_seed(seed: int, i: int) -> int:
    """The Philox key of candidate i of submit_n(..., seed=seed): (seed + i) mod 2^64.  Candidate i draws what a stand-alone
    submit(..., seed=candidate_seed(seed, i)) draws."""
    return (int(seed) + int(i)) & ((1 << 64) - 1)


def retained_tokens(base_tokens: int, prompt_len: int, n_ids: int) -> int:
    """Tokens a retained state has seen: those of the stored state the request continued from (0: from zero), its prompt, and all of
    its n_ids returned ids but the last, which was drawn and never fed back."""
    if prompt_len < 1 or n_ids < 1 or base_tokens < 0:
        raise ValueError(f"base_tokens = {base_tokens}, prompt_len = {prompt_len}, n_ids = {n_ids}: a request has a prompt and at least one id")
    return int(base_tokens) + int(prompt_len) + int(n_ids) - 1


def rank_candidates(cum_lp, lengths, length_normalize: bool = True) -> List[int]:
    """Candidate indices, best first: by the mean log-probability per generated id (length_normalize) or by the sum, largest first;
    ties go to the lower index.  cum_lp / lengths: one number per candidate (sequences, numpy arrays or tensors of any device; they
    are small, the ranking runs on the host)."""
    lp = [float(v) for v in (cum_lp.tolist() if hasattr(cum_lp, "tolist") else cum_lp)]
    ln = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if len(lp) != len(ln):
        raise ValueError(f"{len(lp)} log-probabilities for {len(ln)} lengths")
    if any(n < 1 for n in ln):
        raise ValueError(f"every candidate has at least one id, got lengths {ln}")
    score = [v / n for v, n in zip(lp, ln)] if length_normalize else lp
    score = [float("-inf") if s != s else s for s in score]   # a NaN ranks with the impossible candidates
    return sorted(range(len(lp)), key=lambda i: (-score[i], i))


class SlotScheduler:
    """Device-free bookkeeping of ContinuousDecoder: the FIFO queue of pending requests, the free slots, and every busy slot's budget.

    A request admitted into a slot has drawn its first id; `remaining[slot]` is the number of replays until its budget
    (max_new_tokens) is exhausted.  advance(n) accounts for n replays."""

    def __init__(self, slots: int):
        if slots < 1:
            raise ValueError("slots must be >= 1")
        self.slots = slots
        self.pending: collections.deque = collections.deque()
        self.free: List[int] = list(range(slots))     # ascending; admission takes the lowest free slot
        self.busy: Dict[int, Request] = {}            # slot -> request
        self.remaining: Dict[int, int] = {}           # slot -> replays left in its budget
        self._next = 0

    def submit(self, **fields) -> int:
        h = self._next
        self._next += 1
        req = Request(handle=h, **fields)
        if req.max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        self.pending.append(req)
        return h

    def admit(self) -> List[Tuple[int, Request]]:
        """Pending requests in FIFO order into the free slots: [(slot, request)]."""
        out = []
        while self.pending and self.free:
            slot = self.free.pop(0)
            req = self.pending.popleft()
            self.busy[slot] = req
            self.remaining[slot] = req.max_new_tokens - 1
            out.append((slot, req))
        return out

    def advance(self, n: int):
        for s in self.remaining:
            self.remaining[s] = max(0, self.remaining[s] - n)

    def due(self) -> List[int]:
        """Busy slots whose budget is exhausted."""
        return sorted(s for s, r in self.remaining.items() if r == 0)

    def replays_until_due(self) -> int:
        """Replays until the next busy slot exhausts its budget (0: one already has; 0 too when nothing is busy)."""
        return min(self.remaining.values(), default=0)

    def longest(self) -> int:
        return max(self.remaining.values(), default=0)

    def retire(self, slot: int) -> Request:
        req = self.busy.pop(slot)
        del self.remaining[slot]
        self.free.append(slot)
        self.free.sort()
        return req

    @property
    def idle(self) -> bool:
        return not self.pending and not self.busy


class OverlapScheduler(SlotScheduler):
    """SlotScheduler with a two-stage admission for ContinuousDecoder(admission="overlap"): reserve() takes pending requests into the
    lowest free slots as ONE staged group (their prefill is in flight on a side stream), commit() makes the group busy.  A staged
    request is neither free nor busy and has no `remaining`: advance() leaves it alone and due() cannot name it.  The scheduler counts
    the replays since reserve(), so the commit step is a function of host counters only.  admit() and everything else behave as in
    SlotScheduler."""

    def __init__(self, slots: int):
        super().__init__(slots)
        self.staged: List[Tuple[int, Request]] = []   # the group in flight: [(slot, request)]
        self.since = 0                                # replays since reserve()

    def reserve(self, limit: int) -> List[Tuple[int, Request]]:
        """Up to `limit` pending requests in FIFO order into the lowest free slots, as the staged group: [(slot, request)]."""
        if self.staged:
            raise RuntimeError("a group is already staged: commit() it first")
        if limit < 1:
            raise ValueError("limit must be >= 1")
        while self.pending and self.free and len(self.staged) < limit:
            self.staged.append((self.free.pop(0), self.pending.popleft()))
        self.since = 0
        return list(self.staged)

    def commit(self) -> List[Tuple[int, Request]]:
        """The staged group becomes busy (each request has drawn its first id): [(slot, request)]."""
        took, self.staged = self.staged, []
        for slot, req in took:
            self.busy[slot] = req
            self.remaining[slot] = req.max_new_tokens - 1
        return took

    def advance(self, n: int):
        super().advance(n)
        if self.staged:
            self.since += n

    def replays_until_commit(self, lag: int) -> int:
        """Replays until the staged group has seen `lag` replays since reserve() (0: it has; 0 too when nothing is staged)."""
        return max(0, lag - self.since) if self.staged else 0

    def commit_due(self, lag: int) -> bool:
        """The commit rule: a group is staged, and `lag` replays have been issued since its launch or nothing is busy."""
        return bool(self.staged) and (self.since >= lag or not self.busy)

    def can_launch(self) -> bool:
        return not self.staged and bool(self.pending) and bool(self.free)

    def next_replays(self, check_every: int, lag: int, budgets_known: bool = True) -> int:
        """Replays to issue now: up to check_every, not past the next budget end (budgets_known: the no-EOS case; else not past the
        longest budget) and not past the staged group's commit."""
        n = min(check_every, self.replays_until_due() if budgets_known else self.longest())
        return min(n, self.replays_until_commit(lag)) if self.staged else n

    @property
    def idle(self) -> bool:
        return not self.pending and not self.busy and not self.staged


class GroupScheduler(SlotScheduler):
    """SlotScheduler whose queue may hold GROUPS: n candidates of one prompt (ContinuousDecoder.submit_n) that are admitted together
    or not at all, because the prompt is prefilled once and its cache row copied to the siblings.  Admission stays FIFO: a group at
    the head of the queue waits until n slots are free and holds back everything behind it.  A request outside a group is a group of
    one, and for those admit() is SlotScheduler's."""

    def submit_group(self, n: int, seeds: Sequence[int], **fields) -> List[int]:
        """Queue n candidates of one prompt, candidate i with seeds[i]: their handles in candidate order."""
        if n < 1 or len(seeds) != n:
            raise ValueError(f"n = {n} with {len(seeds)} seeds: n must be >= 1, one seed per candidate")
        if n > self.slots:
            raise ValueError(f"a group of {n} candidates can never be admitted into {self.slots} slots")
        first = self.submit(seed=seeds[0], group_size=n, **fields)
        return [first] + [self.submit(seed=s, group_size=n, leader=first, **fields) for s in seeds[1:]]

    def admit(self) -> List[Tuple[int, Request]]:
        """Pending groups in FIFO order into the free slots, each whole or not at all: [(slot, request)], a group's candidates in
        order and its first candidate (leader None) ahead of those that name it."""
        out = []
        while self.pending and len(self.free) >= self.pending[0].group_size:
            for _ in range(self.pending[0].group_size):
                slot = self.free.pop(0)
                req = self.pending.popleft()
                self.busy[slot] = req
                self.remaining[slot] = req.max_new_tokens - 1
                out.append((slot, req))
        return out


def fan_out_rows(cache, tbl, n_rows, cfg, device, took, heads, logits):
    """submit_n in every engine: the prefilled rows of the groups' first candidates (`heads`, the requests of `took` without a
    leader) -> their siblings' rows of `cache` (n_rows rows), every field of every layer, for all groups admitted together in ONE
    rwkv7_cache_rows_commit_bf16 launch over the cache's own field table `tbl` (prefill.cache_field_table; a repeated source row fans
    out; no row is both read and written: sources are first candidates, destinations are not).  Returns (one logits row per admitted
    request -- its prompt's, gathered --, every admitted slot in `took` order)."""
    from .prefill import cache_rows_commit, check_commit_rows
    slot_of = {r.handle: s for s, r in heads}
    row_of = {r.handle: i for i, (_, r) in enumerate(heads)}
    sibs = [(slot_of[r.leader], s) for s, r in took if r.leader is not None]
    src, dst = check_commit_rows([a for a, _ in sibs], [b for _, b in sibs], n_rows, n_rows)
    if set(src) & set(dst):
        raise RuntimeError(f"fan-out rows {src} -> {dst}: a row is both read and written")
    rows = torch.tensor([src, dst], dtype=torch.int32).to(device, non_blocking=True)
    cache_rows_commit(tbl, tbl, rows[0], rows[1], len(sibs), len(cache), cfg.hidden_size, cfg.num_heads)
    pick = torch.tensor([row_of[r.handle if r.leader is None else r.leader] for _, r in took], dtype=torch.int64).to(device, non_blocking=True)
    return logits.index_select(0, pick), [s for s, _ in took]


class SlotState(ctypes.Structure):
    """rwkv7_slot_state (include/rwkv7_hip.h)."""
    _fields_ = [("step", ctypes.c_void_p), ("limit", ctypes.c_void_p), ("min_until", ctypes.c_void_p), ("seed", ctypes.c_void_p),
                ("inv_temp", ctypes.c_void_p), ("top_k", ctypes.c_void_p), ("top_p", ctypes.c_void_p), ("do_sample", ctypes.c_void_p),
                ("live", ctypes.c_void_p), ("ids", ctypes.c_void_p), ("seq", ctypes.c_void_p), ("seq_ld", ctypes.c_long),
                ("emb", ctypes.c_void_p), ("x", ctypes.c_void_p), ("D", ctypes.c_int), ("slots", ctypes.c_int),
                ("top_k_max", ctypes.c_int), ("eos", ctypes.c_long)]


class SlotLogprob(ctypes.Structure):
    """rwkv7_slot_logprob (include/rwkv7_hip.h)."""
    _fields_ = [("tok_lp", ctypes.c_void_p), ("cum_lp", ctypes.c_void_p)]


def sample_slots(logits: torch.Tensor, st: SlotState, row_slot: Optional[torch.Tensor] = None, allow_lo=None, allow_hi=None,
                 suppress=None, max_domain: Optional[int] = None, lp: Optional[SlotLogprob] = None):
    """rwkv7_sample_slots_f32 on the current stream: logits fp32 [rows, >= max_domain] (unit column stride); row_slot int32 [rows] or
    None (row r is slot r); allow_lo / allow_hi int32 [1] device tensors or None; suppress int32 device tensor or None.  With lp
    (tok_lp fp32 [slots, seq_ld], cum_lp fp64 [slots]): rwkv7_sample_slots_lp_f32, the same draw plus the drawn ids' log-probabilities."""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    if row_slot is not None:
        assert row_slot.dtype == torch.int32 and row_slot.is_contiguous() and row_slot.numel() == logits.shape[0]
    args = (logits.shape[0], logits, logits.stride(0), row_slot, allow_lo, allow_hi, suppress, 0 if suppress is None else suppress.numel(),
            int(logits.shape[1] if max_domain is None else max_domain), ctypes.byref(st))
    if lp is None:
        _lib.call("rwkv7_sample_slots_f32", logits, *args)
    else:
        _lib.call("rwkv7_sample_slots_lp_f32", logits, *args, ctypes.byref(lp))


class ContinuousDecoder:
    """eng = ContinuousDecoder(model, slots=32, ...); h = eng.submit(...); eng.step() -> [(handle, ids)]; eng.run() -> {handle: ids}.

    model: a bf16 RWKV7ForSpeech / RWKV7ForCausalLM on the HIP device that the step kernel covers (DecodeStep.supported); slots in 1..32, or 64, 96 or 128.
    A request's ids run up to and including its EOS, or up to its max_new_tokens (<= max_new_tokens_cap), with no pad tail; they are
    device int64 tensors.  pad_token_id is accepted for signature compatibility with GraphDecoder and not used: no pad is emitted.

    admission: "eager" (default) prefills admitted prompts through RWKV7Model(..., cache_rows=...), one torch op at a time; "graph"
    through prefill.PackedPrefill on the engine's cache: graphs captured once per size class and replayed, the rows reset inside the
    kernels, no device read-back.  In "graph" mode a request's ids do not depend on its slot or on when it is admitted FOR THE SAME PACK
    COMPOSITION (the prompts admitted together, in order): the composition decides the bucket and with it the GEMM shapes, whose
    library kernels may round differently from bucket to bucket.  prefill_max_seqs / prefill_buckets: PackedPrefill's.

    admission="overlap": the same PackedPrefill, on a staging cache of prefill_max_seqs rows and on a side stream.  step() reserves
    the lowest free slots for up to prefill_max_seqs pending requests and starts their prefill; `overlap_replays` replays later (or
    as soon as nothing is busy) the decode stream waits for it on the device, commits the staged rows into the slots' rows and draws
    the first ids.  Until then a reserved slot is an idle slot: the step overwrites its rows with stale values and the commit
    replaces all of them.  Only one group is in flight at a time; every decision reads host counters, never the device, so a
    submission sequence gives the same schedule on every run.  Every bucket is captured at construction.  Ids equal
    admission="graph"'s for the same pack composition; admission_log lists per group (replays at launch, replays at commit, [handles]).

    Best-of-n: submit_n(n, ...) queues n candidates of one prompt, admitted together (GroupScheduler), the prompt prefilled once and
    its cache row copied to the siblings' rows (_fan_out); logprobs=True makes the captured step and the admission draw call
    rwkv7_sample_slots_lp_f32, which also writes every drawn id's log-probability (tok_lp [slots, cap] fp32) and the running fp64
    sum (cum_lp [slots]); take_logprobs(handle) hands them out once the handle has been returned, rank_candidates orders them.
    logprobs=True changes no id; with logprobs=False and no submit_n every code path and launch is the one of before.

    Stored states: with state_store=StateStore(model, ...) a request may name a stored state, submit(state="voice", input_ids=suffix):
    its prompt is the SUFFIX and continues from the stored row, which one rwkv7_cache_rows_seed_bf16 launch copies into the slot's
    row (eager: together with the zero rows of the fresh requests of the same admission, instead of the index_fill_ loop; graph /
    overlap: ahead of a PackedPrefill whose zero marks are per sequence; overlap: on the side stream into the staging rows).  The
    name is pinned in the store from submit() until its admission has read the row.  A seeded request's ids do not depend on its
    slot or on when it is admitted, as for any request (graph / overlap: for the same pack composition).  Without a store every
    code path and launch is the one of before.

    Retained states: with state_store=store and retain=True a request may name the state it leaves behind, submit(..., retain="turn1"),
    and that state becomes an ordinary stored state "turn1" when step() / run() returns the handle.  The store row is taken at submit
    (StateStore.reserve_pending: not servable, not free); the captured step ends with one rwkv7_cache_rows_retain_bf16 launch, which
    copies the row of a slot it finds armed and dead into the slot's store row and disarms the slot -- in the very step in which the
    request ends, because later steps run the dead slot's row through stale inputs and, with an EOS, the host learns of the end up to
    check_every replays late.  Admission issues the same launch after its draw, so a request that ends with its first id is retained
    too.  THE RETAINED STATE is the state after the prompt and all returned ids BUT THE LAST: the last id was drawn and never fed
    back.  To continue, submit(state="turn1", input_ids=[ids[-1], ...]) -- without ids[-1] if it is the EOS; store.tokens counts base
    state + prompt + n - 1 (retained_tokens).  retain= and state= may be combined: the source row stays pinned until admission, the
    target is another, pending row.  retain=True needs a store and is not supported with admission="overlap" (ValueError), nor is
    submit_n(n > 1, retain=...).  An engine that is dropped with requests in flight leaves their names pending: store.abandon(name)
    frees the rows (store.pending() lists them).  retain=True changes no id; without it every code path and launch is the one of before."""

    logprobs = False   # the default of the constructor's switch; nothing below looks at tok_lp / cum_lp without it
    lp = None          # SlotLogprob with logprobs=True: the draws go through rwkv7_sample_slots_lp_f32
    store = None       # the attached StateStore; without one nothing below seeds a row
    retain = False     # the default of the constructor's switch; without it no launch below retains a row

    def __init__(self, model, slots: int = 32, max_new_tokens_cap: int = 3000, eos_token_id: Optional[int] = None,
                 pad_token_id: Optional[int] = None, suppress_tokens: Optional[Sequence[int]] = None, check_every: int = 16,
                 admission: str = "eager", prefill_max_seqs: int = 8, prefill_buckets: Sequence[int] = (256, 512, 1024, 2048, 4096),
                 overlap_replays: int = 8, logprobs: bool = False, state_store=None, retain: bool = False):
        if admission not in ("eager", "graph", "overlap"):
            raise ValueError(f"admission = {admission!r}: 'eager', 'graph' or 'overlap'")
        if retain and state_store is None:
            raise ValueError("retain=True needs a state_store: retained states are rows of it")
        if retain and admission == "overlap":
            raise ValueError("retain=True is not supported with admission='overlap': its commit step does not carry the slots' retain "
                             "rows; use admission='eager' or 'graph'")
        self.retain = bool(retain)
        if overlap_replays < 0:
            raise ValueError("overlap_replays must be >= 0")
        self.admission, self.overlap_replays, self.logprobs = admission, int(overlap_replays), bool(logprobs)
        check_slots(slots)   # 1..32, or 64 / 96 / 128: ValueError before anything touches the device
        if max_new_tokens_cap < 1 or check_every < 1:
            raise ValueError("max_new_tokens_cap and check_every must be >= 1")
        self.model = model.eval()
        m = self.model
        dev = m.device
        self.device, self.slots, self.cap, self.check_every = dev, slots, int(max_new_tokens_cap), int(check_every)
        self.eos = None if eos_token_id is None else int(eos_token_id)
        self.pad = pad_token_id
        self.store = state_store
        if state_store is not None:
            why = state_store.compatible(m.config, m.dtype, dev)
            if why:
                raise ValueError("state_store: " + why)
            state_store.table   # built here, on this stream, not by the first admission (which may run on the side stream)
        self.cache = Cache.zeros(m.config, slots, dev, m.dtype)
        why = step_class(slots).supported(m.model, m.lm_head, self.cache)
        if why is None and m.dtype != torch.bfloat16:
            why = "the model must be bf16"
        emb_w = m.get_input_embeddings().weight.detach()
        if why is None and not (emb_w.dtype == torch.bfloat16 and emb_w.is_contiguous() and emb_w.shape[1] % 8 == 0):
            why = "the input embedding table must be a contiguous bf16 [V, D] with D % 8 == 0"
        if why:
            raise ValueError("ContinuousDecoder needs the persistent decode step: " + why)
        self.emb_w = emb_w
        self.V = m.lm_head.weight.shape[0]
        allow, sup = RowSampler.fold_suppress(self.V, None if not suppress_tokens else list(suppress_tokens))
        self.allow = None if allow is None else [allow]
        self.sup = sup
        i32 = dict(dtype=torch.int32, device=dev)
        self.allow_lo = self.allow_hi = None
        if allow is not None:
            self.allow_lo, self.allow_hi = torch.tensor([allow[0]], **i32), torch.tensor([allow[1]], **i32)
        self.max_domain = (allow[1] - allow[0]) if allow is not None else self.V
        if emb_w.shape[0] < (allow[1] if allow is not None else self.V):
            raise ValueError("the input embedding table has fewer rows than the head draws ids")
        self.suppress = torch.tensor([int(t) for t in sup], **i32) if sup else None
        why = RowSampler.supported(dev, [self.V], self.allow, self.sup)
        if why:
            raise ValueError("rwkv7_sample_slots_f32: " + why)

        S, D = slots, m.config.hidden_size
        l64 = dict(dtype=torch.int64, device=dev)
        self.step_t = torch.zeros(S, **l64)
        self.live = torch.zeros(S, dtype=torch.uint8, device=dev)
        self.ids = torch.zeros(S, **l64)
        self.seq = torch.zeros(S, self.cap, **l64)
        self.x = torch.zeros(S, D, dtype=torch.bfloat16, device=dev)
        # the parameters the device never writes: one block, mirrored on the host and copied whole at admission
        self._par_host = {"limit": torch.ones(S, dtype=torch.int64), "min_until": torch.zeros(S, dtype=torch.int64),
                          "seed": torch.zeros(S, dtype=torch.int64), "inv_temp": torch.ones(S, dtype=torch.float32),
                          "top_k": torch.zeros(S, dtype=torch.int32), "top_p": torch.ones(S, dtype=torch.float32),
                          "do_sample": torch.zeros(S, dtype=torch.uint8)}
        self._par_dev = {k: torch.empty_like(v, device=dev) for k, v in self._par_host.items()}
        for k, v in self._par_host.items():
            self._par_dev[k].copy_(v)
        st = SlotState()
        pd = self._par_dev
        st.step, st.limit, st.min_until, st.seed = (t.data_ptr() for t in (self.step_t, pd["limit"], pd["min_until"], pd["seed"]))
        st.inv_temp, st.top_k, st.top_p, st.do_sample = (pd[k].data_ptr() for k in ("inv_temp", "top_k", "top_p", "do_sample"))
        st.live, st.ids, st.seq, st.seq_ld = self.live.data_ptr(), self.ids.data_ptr(), self.seq.data_ptr(), self.cap
        st.emb, st.x, st.D, st.slots, st.top_k_max = emb_w.data_ptr(), self.x.data_ptr(), D, S, MAX_TOP_K
        st.eos = -1 if self.eos is None else self.eos
        self.st = st
        if self.logprobs:   # what rwkv7_sample_slots_lp_f32 writes next to seq / step
            self.tok_lp = torch.zeros(S, self.cap, dtype=torch.float32, device=dev)
            self.cum_lp = torch.zeros(S, dtype=torch.float64, device=dev)
            self.lp = SlotLogprob(self.tok_lp.data_ptr(), self.cum_lp.data_ptr())
        self._lp_done: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}   # handle -> (tok_lp[:n], cum_lp) until take_logprobs()
        self._fan_tbl = None   # submit_n: the cache's own field table, source and destination of the fan-out copy
        if self.retain:   # what rwkv7_cache_rows_retain_bf16 reads and writes; retain_row crosses with the parameter block
            self.armed = torch.zeros(S, dtype=torch.uint8, device=dev)
            self.ticket = torch.zeros(S, dtype=torch.int32, device=dev)
            self._par_host["retain_row"] = torch.full((S,), -1, dtype=torch.int32)
            self._par_dev["retain_row"] = self.retain_row = torch.full((S,), -1, dtype=torch.int32, device=dev)
            self._cache_tbl()   # built here, not under the capture

        self.sched = OverlapScheduler(slots) if admission == "overlap" else GroupScheduler(slots)
        self.dstep = step_for(m.model, m.lm_head, self.cache)
        # capture the step.  Every slot is idle (live = 0): the draw writes nothing, and the warm-up's change to the state of idle
        # rows does not matter (admission resets a row before it is used)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._step()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._step()
        self.replays = 0   # captured steps run so far
        self.prefill = None
        if admission == "graph":
            from .prefill import PackedPrefill
            self.prefill = PackedPrefill(m.model, self.cache, max_seqs=prefill_max_seqs, buckets=prefill_buckets)
        self.admission_log: List[Tuple[int, int, List[int]]] = []   # overlap: (replays at launch, replays at commit, [handles]) per group
        if admission == "overlap":
            self._init_overlap(int(prefill_max_seqs), prefill_buckets)

    def _step(self):
        sample_slots(self.dstep(self.x), self.st, None, self.allow_lo, self.allow_hi, self.suppress, self.max_domain, self.lp)
        if self.retain:
            self._retain_rows()

    def _retain_rows(self):
        """The rows of the slots that the draw just ended (armed, dead) -> their store rows, and those slots disarmed: one launch."""
        from .prefill import cache_rows_retain
        cfg = self.model.config
        cache_rows_retain(self._cache_tbl(), self.store.table, self.live, self.armed, self.retain_row, self.ticket, len(self.cache),
                          cfg.hidden_size, cfg.num_heads)

    # ---- public interface ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def submit(self, input_ids=None, inputs_embeds=None, max_new_tokens: int = 256, min_new_tokens: int = 0, do_sample: bool = False,
               temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: Optional[int] = None, state: Optional[str] = None,
               retain: Optional[str] = None) -> int:
        """Queue one request (a prompt of T ids [T] / [1, T] or embeddings [T, D] / [1, T, D]); returns its handle.  Non-blocking.
        state: the name of a state in the attached store; the prompt (>= 1 token) is then the suffix that continues from it.
        ValueError without a store, KeyError for a name the store does not hold.
        retain: the name under which the state this request leaves behind is stored once step() / run() has returned the handle: the
        state after the prompt and all returned ids but the last (continue with state=name, input_ids=[ids[-1], ...]).  ValueError
        without ContinuousDecoder(..., retain=True) or for a name that is stored or pending, RuntimeError when the store is full."""
        seed = int(fresh_seed() if seed is None else seed) & ((1 << 64) - 1)
        fields = self._request_fields(input_ids, inputs_embeds, max_new_tokens, min_new_tokens, do_sample, temperature, top_k, top_p)
        return self.sched.submit(seed=seed, **fields, **self._store_fields(state, retain))

    @torch.no_grad()
    def submit_n(self, n: int, input_ids=None, inputs_embeds=None, max_new_tokens: int = 256, min_new_tokens: int = 0,
                 do_sample: bool = False, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: Optional[int] = None,
                 state: Optional[str] = None, retain: Optional[str] = None) -> List[int]:
        """Queue n candidates of ONE prompt (submit()'s arguments): their handles in candidate order.  Candidate i draws with the key
        candidate_seed(seed, i) and is, id for id, the request submit(..., seed=candidate_seed(seed, i)) would be.  The group is admitted
        whole, when n slots are free: the prompt is prefilled once and its cache row copied to the other candidates' rows.
        n > slots: ValueError.  n > 1 with admission="overlap": ValueError (the staging index arrays hold one entry per prompt).
        state: as for submit(); the group's first candidate is seeded from the stored row and its row fans out as ever.
        retain: as for submit(), for n = 1 only; n > 1: ValueError (one name cannot hold the states of several candidates)."""
        n = int(n)
        if n < 1 or n > self.slots:
            raise ValueError(f"n = {n} candidates outside 1..{self.slots} (slots): a group is admitted whole")
        if n > 1 and retain is not None:
            raise ValueError(f"submit_n with n = {n} and retain = {retain!r}: one name holds one state; retain a single request")
        if n > 1 and self.admission == "overlap":
            raise ValueError("submit_n with n > 1 is not supported with admission='overlap': its staging rows and index arrays are sized "
                             "to prompts; use admission='eager' or 'graph'")
        fields = self._request_fields(input_ids, inputs_embeds, max_new_tokens, min_new_tokens, do_sample, temperature, top_k, top_p)
        seed = int(fresh_seed() if seed is None else seed) & ((1 << 64) - 1)
        fields.update(self._store_fields(state, retain))   # pinned once per group: the first candidate's admission unpins
        if n == 1:
            return [self.sched.submit(seed=seed, **fields)]
        return self.sched.submit_group(n, [candidate_seed(seed, i) for i in range(n)], **fields)

    def take_logprobs(self, handle: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(tok_lp [n] fp32, cum_lp fp64 scalar) of a request that step() / run() has returned, both on the device: the log-probability
        of each of its n ids under the raw logits (temperature 1, before top-k / top-p, over the ids the draw could produce) and their
        sum, added in step order in fp64.  Needs logprobs=True; a handle's result can be taken once."""
        if not self.logprobs:
            raise ValueError("take_logprobs needs ContinuousDecoder(..., logprobs=True)")
        try:
            return self._lp_done.pop(handle)
        except KeyError:
            raise KeyError(f"handle {handle}: not finished yet (step() / run() has not returned it), unknown, or already taken") from None

    def _state_fields(self, state) -> dict:
        """submit(state=...): the name's row, pinned until the request's admission has read it.  Call it last: nothing after it may raise."""
        if state is None:
            return {}
        if self.store is None:
            raise ValueError(f"state = {state!r} needs ContinuousDecoder(..., state_store=...)")
        row = self.store.pin(state)   # KeyError for an unknown name
        return dict(state=state, state_row=row, base_tokens=self.store.tokens[row])

    def _store_fields(self, state, retain) -> dict:
        """submit(state=..., retain=...): _state_fields plus the pending row of the name to retain under.  Call it last too."""
        if retain is None:
            return self._state_fields(state)
        if not self.retain:
            raise ValueError(f"retain = {retain!r} needs ContinuousDecoder(..., state_store=..., retain=True)")
        keep = dict(retain=retain, retain_row=self.store.reserve_pending(retain))   # ValueError: stored or pending; RuntimeError: full
        try:
            return dict(keep, **self._state_fields(state))
        except BaseException:
            self.store.abandon(retain)
            raise

    def _unpin(self, took):
        for _, r in took:
            if r.state is not None and r.leader is None:
                self.store.unpin(r.state)

    def _seed(self, heads, dst_tbl, dst_rows, n_dst: int, zero_fresh: bool):
        """One rwkv7_cache_rows_seed_bf16 launch on the current stream for the admitted `heads`: the stored row of every seeded
        request -> its row dst_rows[i] of the cache behind dst_tbl (of n_dst rows); a fresh request's row gets zeros (zero_fresh) or
        is left to the prefill kernels' zero marks (its entry is skipped)."""
        from .prefill import SEED_ZERO, cache_rows_seed, check_seed_rows
        cfg = self.model.config
        src = [SEED_ZERO if r.state_row is None else r.state_row for _, r in heads]
        dst = [d if (zero_fresh or r.state_row is not None) else -1 for d, (_, r) in zip(dst_rows, heads)]
        src, dst = check_seed_rows(src, dst, self.store.capacity, n_dst)
        rows = torch.tensor([src, dst], dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
        cache_rows_seed(self.store.table, dst_tbl, rows[0], rows[1], len(heads), len(self.cache), cfg.hidden_size, cfg.num_heads)

    def _cache_tbl(self):
        """The live cache's own field table (built once)."""
        if self._fan_tbl is None:
            from .prefill import cache_field_table
            self._fan_tbl = cache_field_table(self.cache)
        return self._fan_tbl

    def _request_fields(self, input_ids, inputs_embeds, max_new_tokens, min_new_tokens, do_sample, temperature, top_k, top_p) -> dict:
        """submit()'s argument checks and the prompt's embeddings: Request's fields but the handle and the seed."""
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("pass exactly one of input_ids or inputs_embeds")
        if not 1 <= int(max_new_tokens) <= self.cap:
            raise ValueError(f"max_new_tokens = {max_new_tokens} outside 1..{self.cap} (max_new_tokens_cap)")
        top_k, top_p = int(top_k or 0), 1.0 if top_p is None else float(top_p)
        why = RowSampler.supported(self.device, [self.V], self.allow, self.sup, do_sample, top_k, top_p, temperature)
        if why:
            raise ValueError("rwkv7_sample_slots_f32: " + why)
        if inputs_embeds is None:
            ids = torch.as_tensor(input_ids).reshape(-1).to(self.device)
            e = self.model.get_input_embeddings()(ids)
        else:
            e = inputs_embeds.reshape(-1, inputs_embeds.shape[-1]).to(self.device, self.model.dtype)
        if e.shape[0] < 1 or e.shape[1] != self.model.config.hidden_size:
            raise ValueError(f"prompt of shape {tuple(e.shape)}")
        return dict(embeds=e.detach(), max_new_tokens=int(max_new_tokens), min_new_tokens=int(min_new_tokens or 0),
                    do_sample=bool(do_sample), temperature=float(temperature or 1.0), top_k=top_k, top_p=top_p)

    @torch.no_grad()
    def step(self) -> List[Tuple[int, torch.Tensor]]:
        """Admit what fits, run up to check_every replays, retire what finished: [(handle, ids)] of the requests that finished."""
        if self.admission == "overlap":
            return self._step_overlap()
        done = []
        if self.eos is None:
            done += self._retire(self.sched.due(), None)
        self._admit()
        if self.eos is None:
            done += self._retire(self.sched.due(), None)   # max_new_tokens = 1: finished with its first id
            n = min(self.check_every, self.sched.replays_until_due())
        else:
            n = min(self.check_every, self.sched.longest())
        if not self.sched.busy:
            return done
        for _ in range(n):
            self.graph.replay()
        self.replays += n
        self.sched.advance(n)
        if self.eos is None:
            done += self._retire(self.sched.due(), None)
        else:
            both = torch.stack([self.live.to(torch.int64), self.step_t]).cpu()   # one small read-back
            done += self._retire([s for s in sorted(self.sched.busy) if not both[0, s]], both[1])
        if self.dstep.barrier_timed_out():
            raise _lib.Rwkv7HipError("rwkv7_decode_step_bf16: a grid barrier timed out; the generated ids are invalid")
        return done

    @torch.no_grad()
    def run(self) -> Dict[int, torch.Tensor]:
        """Step until everything submitted so far has finished: {handle: ids}."""
        out = {}
        while not self.sched.idle:
            for h, ids in self.step():
                out[h] = ids
        return out

    # ---- internals -----------------------------------------------------------------------------------------------------------
    def _retire(self, slots, steps) -> List[Tuple[int, torch.Tensor]]:
        out = []
        for s in slots:
            req = self.sched.retire(s)
            n = req.max_new_tokens if steps is None else int(steps[s])
            out.append((req.handle, self.seq[s, :n].clone()))
            if self.logprobs:
                self._lp_done[req.handle] = (self.tok_lp[s, :n].clone(), self.cum_lp[s].clone())
            if req.retain is not None:   # the step in which the request ended has written the row; the slot's entry goes back to rest
                self.store.publish(req.retain, retained_tokens(req.base_tokens, req.embeds.shape[0], n))
                self._par_host["retain_row"][s] = -1
                self.retain_row[s:s + 1].fill_(-1)
        return out

    def _admit(self):
        took = self.sched.admit()
        if not took:
            return
        m, dev = self.model, self.device
        # the requests that prefill: all of them, but for the candidates of a submit_n group after its first, which get a copy of its rows
        heads = [(s, r) for s, r in took if r.leader is None]
        slots = [s for s, _ in heads]
        if self.prefill is not None:
            return self._admit_graph(took, heads, slots)
        lens = [r.embeds.shape[0] for _, r in heads]
        cu = [0]
        for n in lens:
            cu.append(cu[-1] + n)
        rows64 = torch.tensor(slots, dtype=torch.int64).to(dev, non_blocking=True)
        if self.store is not None:     # a stored state or a fresh one for every admitted request, in one launch
            self._seed(heads, self._cache_tbl(), slots, self.slots, zero_fresh=True)
            self._unpin(took)
        else:
            for st in self.cache.states:   # a fresh state for every admitted request
                st.att_x_prev.index_fill_(0, rows64, 0)
                st.att_kv.index_fill_(0, rows64, 0)
                st.ffn_x_prev.index_fill_(0, rows64, 0)
        packed = torch.cat([r.embeds for _, r in heads], 0).unsqueeze(0)
        cu_t = torch.tensor(cu, dtype=torch.int32)
        h = m.model(inputs_embeds=packed, cu_seqlens=cu_t, past_key_values=self.cache, cache_rows=torch.tensor(slots)).last_hidden_state
        last = torch.tensor([c - 1 for c in cu[1:]], dtype=torch.int64).to(dev, non_blocking=True)
        logits = m.lm_head(h[0].index_select(0, last)).float()
        if len(heads) < len(took):
            logits, slots = self._fan_out(took, heads, logits)
            rows64 = torch.tensor(slots, dtype=torch.int64).to(dev, non_blocking=True)
        self._admit_draw(took, logits, rows64, torch.tensor(slots, dtype=torch.int32).to(dev, non_blocking=True))

    def _admit_graph(self, took, heads, slots):
        """Admission through PackedPrefill: the rows are reset by the kernels (zero marks), the layout goes over as one pinned index
        block per replay, and nothing is read back."""
        fresh = True
        if any(r.state_row is not None for _, r in heads):   # stored rows in; the fresh requests keep the kernels' zero marks
            self._seed(heads, self._cache_tbl(), slots, self.slots, zero_fresh=False)
            fresh = [r.state_row is None for _, r in heads]
        if self.store is not None:
            self._unpin(took)
        h_last = self.prefill.run([r.embeds for _, r in heads], slots, fresh=fresh)
        logits = self.model.lm_head(h_last).float()
        if len(heads) < len(took):
            logits, slots = self._fan_out(took, heads, logits)
        row_slot = torch.tensor(slots, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
        self._admit_draw(took, logits, row_slot.long(), row_slot)

    def _fan_out(self, took, heads, logits):
        """submit_n: the prefilled rows of the groups' first candidates -> their siblings' rows, every field of every layer, for all groups
        admitted together in ONE rwkv7_cache_rows_commit_bf16 launch over the cache's own field table (a repeated source row fans out; no
        row is both read and written: sources are first candidates, destinations are not).  Returns (one logits row per admitted
        request -- its prompt's, gathered --, every admitted slot in `took` order)."""
        return fan_out_rows(self.cache, self._cache_tbl(), self.slots, self.model.config, self.device, took, heads, logits)

    # ---- admission="overlap" -------------------------------------------------------------------------------------------------
    def _init_overlap(self, max_seqs, buckets):
        """Everything overlapped work touches is allocated HERE, once: the staging cache and its PackedPrefill with every bucket
        captured (no capture may happen while the other stream has work in flight), the staged logits, the row indices, the two
        pointer tables, the pinned index blocks, the side stream and the events."""
        from .prefill import PackedPrefill, cache_field_table
        m, dev = self.model, self.device
        P = self.stage_rows = max_seqs
        self.stage_cache = Cache.zeros(m.config, P, dev, m.dtype)
        self.prefill = PackedPrefill(m.model, self.stage_cache, max_seqs=max_seqs, buckets=buckets).warm()
        self.logits_stage = torch.zeros(P, self.V, dtype=torch.float32, device=dev)
        self._src_row = torch.arange(P, dtype=torch.int32, device=dev)        # stage row of entry i: always i
        self._dst_row = torch.full((P,), -1, dtype=torch.int32, device=dev)   # its slot; -1 past the group
        self._rows64 = torch.zeros(P, dtype=torch.int64, device=dev)
        self._src_tbl, self._dst_tbl = cache_field_table(self.stage_cache), cache_field_table(self.cache)
        # the slots of a group cross in one of two pinned blocks, alternately; a block is rewritten only after the copy that read it
        self._pin = [torch.full((P,), -1, dtype=torch.int32).pin_memory() for _ in range(2)]
        self._pin_ev = [torch.cuda.Event(), torch.cuda.Event()]
        self._pin_used = [False, False]
        self._ready = torch.cuda.Event()
        self._side = torch.cuda.Stream(device=dev)
        self._launched_at = 0
        self._groups = 0
        torch.cuda.current_stream(dev).synchronize()   # the tables and the warm-up are complete before any side-stream work

    def _step_overlap(self) -> List[Tuple[int, torch.Tensor]]:
        """step() with the prefill of the next group on the side stream.  Every decision reads host counters only (never whether the
        prefill has finished), so a submission sequence gives the same schedule on every run."""
        s, lag, done = self.sched, self.overlap_replays, []
        if self.eos is None:
            done += self._retire(s.due(), None)
        if s.commit_due(lag):
            self._commit()
        if s.can_launch():
            self._launch()
            if s.commit_due(lag):
                self._commit()
        if self.eos is None:
            done += self._retire(s.due(), None)   # max_new_tokens = 1: finished with its first id
        if not s.busy:
            return done
        n = s.next_replays(self.check_every, lag, self.eos is None)
        for _ in range(n):
            self.graph.replay()
        self.replays += n
        s.advance(n)
        if self.eos is None:
            done += self._retire(s.due(), None)
        else:
            both = torch.stack([self.live.to(torch.int64), self.step_t]).cpu()   # one small read-back
            done += self._retire([b for b in sorted(s.busy) if not both[0, b]], both[1])
        if self.dstep.barrier_timed_out():
            raise _lib.Rwkv7HipError("rwkv7_decode_step_bf16: a grid barrier timed out; the generated ids are invalid")
        return done

    def _launch(self):
        """Reserve a group (host) and start its prefill (device)."""
        took = self.sched.reserve(self.stage_rows)
        self._launched_at = self.replays
        self._launch_device(took)

    def _commit(self):
        """The staged group becomes busy (host) and its rows and first ids reach the slots (device)."""
        took = self.sched.commit()
        self._commit_device(took)
        self.admission_log.append((self._launched_at, self.replays, [r.handle for _, r in took]))

    def _launch_device(self, took):
        """The group's prefill into stage rows 0 .. n - 1 on the side stream.  The side stream first waits for the decode stream: for
        the prompts' embeddings, for the previous commit's read of the stage rows and of logits_stage, and for whatever wrote the
        stored states the group continues from (a StateStore.capture issued on the decode stream just before)."""
        main, side = torch.cuda.current_stream(self.device), self._side
        side.wait_stream(main)
        with torch.cuda.stream(side):
            for _, r in took:
                r.embeds.record_stream(side)
            fresh = True
            if any(r.state_row is not None for _, r in took):   # stored rows -> staging rows; the names stay pinned until the commit
                self._seed(took, self._src_tbl, list(range(len(took))), self.stage_rows, zero_fresh=False)
                fresh = [r.state_row is None for _, r in took]
            h_last = self.prefill.run([r.embeds for _, r in took], list(range(len(took))), fresh=fresh)
            self.logits_stage[:len(took)].copy_(self.model.lm_head(h_last).float())
            self._ready.record(side)

    def _commit_device(self, took):
        """On the decode stream: wait (on the device, the host never blocks on it) for the staged prefill, copy the stage rows into the
        slots' rows in one launch, then the parameter block, step = 0, live = 1 and the first draw, as the other admission modes do."""
        from .prefill import cache_rows_commit, check_commit_rows
        n, k = len(took), self._groups % 2
        main = torch.cuda.current_stream(self.device)
        _, slots = check_commit_rows(range(n), [sl for sl, _ in took], self.stage_rows, self.slots)
        if self._pin_used[k]:
            self._pin_ev[k].synchronize()   # the copy that read this block two groups ago (long complete)
        self._pin[k].fill_(-1)
        self._pin[k][:n] = torch.tensor(slots, dtype=torch.int32)
        self._dst_row.copy_(self._pin[k], non_blocking=True)
        self._pin_ev[k].record(main)
        self._pin_used[k] = True
        self._groups += 1
        main.wait_event(self._ready)
        if self.store is not None:
            self._unpin(took)   # the decode stream is now ordered after the side stream's read of the stored rows
        cfg = self.model.config
        cache_rows_commit(self._src_tbl, self._dst_tbl, self._src_row, self._dst_row, n, len(self.cache), cfg.hidden_size, cfg.num_heads)
        row_slot = self._dst_row[:n]
        self._rows64[:n].copy_(row_slot)
        self._admit_draw(took, self.logits_stage[:n], self._rows64[:n], row_slot)

    def _admit_draw(self, took, logits, rows64, row_slot):
        # the slots' parameters: host mirror -> one copy per field; step = 0 and live = 1 for the admitted slots only (the device
        # advances the other slots' counters)
        ph = self._par_host
        for s, r in took:
            ph["limit"][s] = r.max_new_tokens
            ph["min_until"][s] = r.min_new_tokens
            ph["seed"][s] = r.seed - (1 << 64) if r.seed >= (1 << 63) else r.seed
            ph["inv_temp"][s] = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(r.temperature, dtype=torch.float32)
                                 if r.do_sample else torch.tensor(1.0))
            ph["top_k"][s] = r.top_k if r.do_sample else 0
            ph["top_p"][s] = r.top_p
            ph["do_sample"][s] = int(r.do_sample)
            if self.retain:
                ph["retain_row"][s] = -1 if r.retain_row is None else r.retain_row
        if self.retain:
            from .prefill import check_retain_rows
            check_retain_rows(ph["retain_row"].tolist(), self.store.capacity)
        for k, v in ph.items():
            self._par_dev[k].copy_(v.pin_memory(), non_blocking=True)
        self.step_t.index_fill_(0, rows64, 0)
        self.live.index_fill_(0, rows64, 1)
        if self.logprobs:
            self.cum_lp.index_fill_(0, rows64, 0)
        arm = [s for s, r in took if r.retain_row is not None]
        if arm:
            self.armed.index_fill_(0, torch.tensor(arm, dtype=torch.int64).to(self.device, non_blocking=True), 1)
        sample_slots(logits, self.st, row_slot, self.allow_lo, self.allow_hi, self.suppress, self.max_domain, self.lp)
        if self.retain:
            self._retain_rows()   # a request that ends with its first id leaves the state after its prompt
