"""Continuous batching for the Cosy model (RWKV7CosyLM): the engine of continuous.py with CosyVoice's repetition-aware draw per slot.

RWKV7CosyLM.inference serves one utterance per process: one ring of recent ids, one loop index, one EOS bar, one key, and the id
crosses to the host every token.  Here every one of up to 128 SLOTS runs its own utterance:

  * one captured step: DecodeStep (WideDecodeStep above 32 slots: decode.step_for) on the live cache, then rwkv7_ras_slots_f32 (csrc/ras_slots.hip) on its logits, which draws every
    live slot's id as rwkv7_ras_step_f32 does for B = 1 -- with the slot's own key, loop index, n_ignore, top_k / top_p / tau_r and
    ring -- and does the streaming loop's bookkeeping (ring, emitted ids, next input embedding, loop index, end of utterance);
  * admission as in ContinuousDecoder ("eager": packed prefill through RWKV7Model(..., cache_rows=...); "graph":
    prefill.PackedPrefill), the head on each last position, and the same entry with row_slot for the first id;
  * retirement: EOS is always possible, so `live`, `step` and `n_out` are read back in one small copy every `check_every` replays.

A request's draws use (its seed, its loop index, its own ring) only, so its ids do not depend on its slot or on when it was admitted
(graph admission: for the same pack composition, see ContinuousDecoder).  cosy_request is the host part of inference(): the prompt
layout and the length bounds.  The reference zeroes the token-shift rows of the cache at the end of an utterance (cosy_llm.py:247-251);
that is not repeated here, because admission resets a slot's rows before they are used again.

Best-of-n (submit_n, logprobs=True, take_logprobs): n candidates of one utterance share one prefill -- the first candidate's cache
row is copied to its siblings' rows in one rwkv7_cache_rows_commit_bf16 launch -- and rwkv7_ras_slots_lp_f32 writes every drawn id's
log-probability at draw time, so rank_candidates orders the candidates without a teacher-forced pass.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .backbone import Cache
from .decode import check_slots, step_class, step_for
from .continuous import GroupScheduler, candidate_seed, fan_out_rows
from .sampling import MAX_DOMAIN, fresh_seed

MAX_WIN = 128          # entries of a slot's ring (rwkv7_ras_slots_f32)
MAX_RAS_TOP_K = 128    # candidates of the nucleus
END_OF_PROMPT = 65531  # <|endofprompt|>: an instruction prefix ends here and does not count towards the length budget


class RasSlotState(ctypes.Structure):
    """rwkv7_ras_slot_state (include/rwkv7_hip.h)."""
    _fields_ = [("step", ctypes.c_void_p), ("limit", ctypes.c_void_p), ("n_ignore", ctypes.c_void_p), ("seed", ctypes.c_void_p),
                ("top_k", ctypes.c_void_p), ("top_p", ctypes.c_void_p), ("tau_r", ctypes.c_void_p), ("live", ctypes.c_void_p),
                ("recent", ctypes.c_void_p), ("win_ld", ctypes.c_long), ("ptr", ctypes.c_void_p), ("ids", ctypes.c_void_p),
                ("n_out", ctypes.c_void_p), ("seq", ctypes.c_void_p), ("seq_ld", ctypes.c_long), ("emb", ctypes.c_void_p),
                ("x", ctypes.c_void_p), ("D", ctypes.c_int), ("slots", ctypes.c_int), ("win_size", ctypes.c_int),
                ("top_k_max", ctypes.c_int), ("eos", ctypes.c_long)]


class RasSlotLogprob(ctypes.Structure):
    """rwkv7_ras_slot_logprob (include/rwkv7_hip.h)."""
    _fields_ = [("tok_lp", ctypes.c_void_p), ("cum_lp", ctypes.c_void_p), ("end_lp", ctypes.c_void_p)]


def ras_slots(logits: torch.Tensor, st: RasSlotState, row_slot: Optional[torch.Tensor] = None, lp: Optional[RasSlotLogprob] = None):
    """rwkv7_ras_slots_f32 on the current stream: logits fp32 [rows, V] (unit column stride); row_slot int32 [rows] or None (row r
    is slot r).  With lp (tok_lp fp32 [slots, seq_ld], cum_lp fp64 [slots], end_lp fp32 [slots]): rwkv7_ras_slots_lp_f32, the same
    draw plus the drawn ids' log-probabilities."""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    if row_slot is not None:
        assert row_slot.dtype == torch.int32 and row_slot.is_contiguous() and row_slot.numel() == logits.shape[0]
    args = (logits.shape[0], logits.shape[1], logits, logits.stride(0), row_slot, ctypes.byref(st))
    if lp is None:
        _lib.call("rwkv7_ras_slots_f32", logits, *args)
    else:
        _lib.call("rwkv7_ras_slots_lp_f32", logits, *args, ctypes.byref(lp))


@dataclass
class CosyRequest:
    """The host part of RWKV7CosyLM.inference for one utterance."""
    embeds: torch.Tensor        # [T, D]: sos, prompt_text + text, task_id, prompt speech
    min_len: int
    max_len: int
    original_text_len: int

    @property
    def n_ignore(self) -> int:
        """EOS is rejected while the loop index is below this (inference: i + original_text_len < min_len)."""
        return self.min_len - self.original_text_len

    @property
    def limit(self) -> int:
        return self.max_len


def _ids_row(t, device) -> torch.Tensor:
    t = torch.as_tensor(t if t is not None else [], dtype=torch.int64).reshape(-1)
    return t.to(device)


@torch.no_grad()
def cosy_request(model, text, prompt_text=None, prompt_speech_token=None, sampling: int = 25, max_token_text_ratio: float = 20,
                 min_token_text_ratio: float = 0.5) -> CosyRequest:
    """The prompt of one utterance as RWKV7CosyLM.inference lays it out -- [sos, prompt_text + text, task_id, prompt speech]
    embeddings [T, D] -- and its length bounds: the text after an <|endofprompt|> (65531) instruction prefix is what counts.
    text / prompt_text / prompt_speech_token: int64 ids ([T] or [1, T]) or None.  Pure host code plus embedding lookups.
    `sampling` (the top_k of the draw) is validated here and passed on by ContinuousCosyDecoder.submit."""
    if not 1 <= int(sampling) <= MAX_RAS_TOP_K:
        raise ValueError(f"sampling = {sampling}: the nucleus holds 1..{MAX_RAS_TOP_K} candidates")
    dev = model.llm_embedding.weight.device
    ids = torch.cat([_ids_row(prompt_text, dev), _ids_row(text, dev)])
    n_text = int(ids.numel())
    hits = (ids == END_OF_PROMPT).nonzero()
    n_instr = int(hits[0, 0].item()) + 1 if hits.numel() else 0
    content_length = original_text_len = n_text - n_instr
    emb_w = model.llm_embedding.weight
    pieces = [emb_w[model.sos_eos].view(1, -1), model.text_embedding(ids), emb_w[model.task_id].view(1, -1)]
    speech = _ids_row(prompt_speech_token, dev)
    if speech.numel() != 0:
        pieces.append(model.speech_embedding(speech))
    min_len, max_len = int(content_length * min_token_text_ratio), int(content_length * max_token_text_ratio)
    return CosyRequest(torch.cat(pieces, 0).detach(), min_len, max_len, original_text_len)


class StreamCursor:
    """Device-free part of ContinuousCosyDecoder.stream: how many emitted ids of every running request have been handed out, and which
    columns of `seq` are new at a read-back."""

    def __init__(self, seq_ld: int):
        self.seq_ld = int(seq_ld)
        self.seen: Dict[int, int] = {}   # handle -> ids handed out so far

    def take(self, running: Sequence[Tuple[int, int, int]]) -> Tuple[List[int], List[Tuple[int, int]]]:
        """running: [(slot, handle, n_out)] of the busy slots at a read-back.  Returns the flat indices into seq.view(-1) of all new
        ids, request after request, and [(handle, count)] in the same order; handles that no longer run are forgotten."""
        flat, counts = [], []
        for slot, handle, n_out in running:
            a, b = self.seen.get(handle, 0), min(int(n_out), self.seq_ld)
            flat.extend(range(slot * self.seq_ld + a, slot * self.seq_ld + b))
            counts.append((handle, max(b - a, 0)))
            self.seen[handle] = max(a, b)
        keep = {h for _, h, _ in running}
        self.seen = {h: n for h, n in self.seen.items() if h in keep}
        return flat, counts

    def finish(self, handle: int):
        self.seen.pop(handle, None)


class ContinuousCosyDecoder:
    """eng = ContinuousCosyDecoder(model, slots=32, ...); h = eng.submit(text=..., ...); eng.step() -> [(handle, ids)];
    eng.run() -> {handle: ids}; eng.stream() yields (handle, new_ids, finished) at every read-back.

    model: a bf16 RWKV7CosyLM on the HIP device that the step kernel covers, with a head of speech_token_size + 1 rows (the condition
    inference() uses for its fused path); slots in 1..32, or 64, 96 or 128.  A request's result is a device int64 tensor of its emitted ids -- the ids
    inference() would yield, without the EOS -- at most its max_len (<= max_len_cap).  win_size is the engine's; top_p and tau_r are
    defaults that submit() may override per request.  admission / prefill_max_seqs / prefill_buckets: as in ContinuousDecoder.

    The reference zeroes the token-shift rows at the end of an utterance; that is not repeated, because admission resets the slot's
    rows before they are reused.

    Best-of-n: submit_n(n, ...) queues n candidates of one utterance, admitted together (GroupScheduler), the prompt prefilled once
    and its cache row copied to the siblings' rows (_fan_out).  logprobs=True makes the captured step and the admission draw call
    rwkv7_ras_slots_lp_f32, which also writes every emitted id's log-probability under the raw logits (tok_lp [slots, cap] fp32),
    their running fp64 sum (cum_lp [slots]) and the log-probability of the EOS draw that ended the utterance (end_lp [slots]);
    take_logprobs(handle) hands them out once the handle has been reported finished, and continuous.rank_candidates orders a group:

        hs = eng.submit_n(4, text=..., prompt_speech_token=..., seed=7); out = eng.run()
        lp = [eng.take_logprobs(h) for h in hs]                                   # (tok_lp[:n], cum_lp, end_lp) per candidate
        best = hs[rank_candidates([c for _, c, _ in lp], [out[h].numel() for h in hs])[0]]

    cum_lp covers the emitted ids only; a caller who wants the EOS draw to count adds it: [c + e.double() for _, c, e in lp] (with
    out[h].numel() + 1 as the length for a candidate that ended on EOS; end_lp is 0 for one that ran to its max_len).  A candidate
    without an emitted id (EOS first) has length 0, which rank_candidates refuses: leave it out.  logprobs=True changes no id; with
    logprobs=False and no submit_n every code path and launch is the one of before."""

    logprobs = False   # the default of the constructor's switch; nothing below looks at tok_lp / cum_lp / end_lp without it
    lp = None          # RasSlotLogprob with logprobs=True: the draws go through rwkv7_ras_slots_lp_f32

    def __init__(self, model, slots: int = 32, max_len_cap: int = 3000, check_every: int = 16, admission: str = "eager",
                 win_size: int = 10, top_p: float = 0.8, tau_r: float = 0.1, prefill_max_seqs: int = 8,
                 prefill_buckets: Sequence[int] = (256, 512, 1024, 2048, 4096), logprobs: bool = False):
        if admission not in ("eager", "graph"):
            raise ValueError(f"admission = {admission!r}: 'eager' or 'graph'")
        self.logprobs = bool(logprobs)
        check_slots(slots)   # 1..32, or 64 / 96 / 128: ValueError before anything touches the device
        if max_len_cap < 1 or check_every < 1:
            raise ValueError("max_len_cap and check_every must be >= 1")
        if not 1 <= win_size <= MAX_WIN:
            raise ValueError(f"win_size = {win_size}: 1..{MAX_WIN}")
        self.admission = admission
        self.model = m = model.eval()
        self.eos = int(m.speech_token_size)
        self.V = V = m.lm_head.weight.shape[0]
        if V != self.eos + 1:
            raise ValueError(f"the head has {V} rows, not speech_token_size + 1 = {self.eos + 1}: ids above EOS are outside the fused draw")
        if V > MAX_DOMAIN:
            raise ValueError(f"the head has {V} rows: the draw covers at most {MAX_DOMAIN} ids")
        dev = m.lm_head.weight.device
        dtype = m.lm_head.weight.dtype
        if dtype != torch.bfloat16:
            raise ValueError("ContinuousCosyDecoder needs a bf16 model")
        if dev.type != "cuda":
            raise ValueError("ContinuousCosyDecoder needs the model on the HIP device")
        self.device, self.slots, self.cap, self.check_every = dev, slots, int(max_len_cap), int(check_every)
        self.win_size, self.top_p, self.tau_r = int(win_size), float(top_p), float(tau_r)
        self.cache = Cache.zeros(m.config, slots, dev, dtype)
        why = step_class(slots).supported(m.model, m.lm_head, self.cache)
        emb_w = m.speech_embedding.weight.detach()
        if why is None and not (emb_w.dtype == torch.bfloat16 and emb_w.is_contiguous() and emb_w.shape[1] % 8 == 0 and emb_w.shape[0] >= V):
            why = "the speech embedding table must be a contiguous bf16 [>= V, D] with D % 8 == 0"
        if why:
            raise ValueError("ContinuousCosyDecoder needs the persistent decode step: " + why)
        self.emb_w = emb_w

        S, D = slots, m.config.hidden_size
        l64 = dict(dtype=torch.int64, device=dev)
        self.step_t, self.n_out, self.ptr, self.ids = (torch.zeros(S, **l64) for _ in range(4))
        self.live = torch.zeros(S, dtype=torch.uint8, device=dev)
        self.recent = torch.full((S, self.win_size), -1, **l64)
        self.seq = torch.zeros(S, self.cap, **l64)
        self.x = torch.zeros(S, D, dtype=torch.bfloat16, device=dev)
        # the parameters the device never writes: one block, mirrored on the host and copied whole at admission
        self._par_host = {"limit": torch.ones(S, dtype=torch.int64), "n_ignore": torch.zeros(S, dtype=torch.int64),
                          "seed": torch.zeros(S, dtype=torch.int64), "top_k": torch.ones(S, dtype=torch.int32),
                          "top_p": torch.ones(S, dtype=torch.float32), "tau_r": torch.ones(S, dtype=torch.float32)}
        self._par_dev = {k: torch.empty_like(v, device=dev) for k, v in self._par_host.items()}
        for k, v in self._par_host.items():
            self._par_dev[k].copy_(v)
        st, pd = RasSlotState(), self._par_dev
        st.step, st.limit, st.n_ignore, st.seed = (t.data_ptr() for t in (self.step_t, pd["limit"], pd["n_ignore"], pd["seed"]))
        st.top_k, st.top_p, st.tau_r, st.live = pd["top_k"].data_ptr(), pd["top_p"].data_ptr(), pd["tau_r"].data_ptr(), self.live.data_ptr()
        st.recent, st.win_ld, st.ptr, st.ids = self.recent.data_ptr(), self.win_size, self.ptr.data_ptr(), self.ids.data_ptr()
        st.n_out, st.seq, st.seq_ld = self.n_out.data_ptr(), self.seq.data_ptr(), self.cap
        st.emb, st.x, st.D, st.slots = emb_w.data_ptr(), self.x.data_ptr(), D, S
        st.win_size, st.top_k_max, st.eos = self.win_size, MAX_RAS_TOP_K, self.eos
        self.st = st
        if self.logprobs:   # what rwkv7_ras_slots_lp_f32 writes next to seq / n_out
            self.tok_lp = torch.zeros(S, self.cap, dtype=torch.float32, device=dev)
            self.cum_lp = torch.zeros(S, dtype=torch.float64, device=dev)
            self.end_lp = torch.zeros(S, dtype=torch.float32, device=dev)
            self.lp = RasSlotLogprob(self.tok_lp.data_ptr(), self.cum_lp.data_ptr(), self.end_lp.data_ptr())
        self._lp_done: Dict[int, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}   # handle -> its values until take_logprobs()
        self._fan_tbl = None   # submit_n: the cache's own field table, source and destination of the fan-out copy

        self.sched = GroupScheduler(slots)   # for groups of one its admit() is SlotScheduler's
        self._extra: Dict[int, float] = {}   # handle -> tau_r: what the scheduler's request does not carry
        self.dstep = step_for(m.model, m.lm_head, self.cache)
        # capture the step with every slot idle (live = 0): the draw writes nothing, and what the warm-up does to the state of idle
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

    def _step(self):
        ras_slots(self.dstep(self.x), self.st, None, self.lp)

    # ---- public interface ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def submit(self, text=None, prompt_text=None, prompt_speech_token=None, sampling: int = 25, max_token_text_ratio: float = 20,
               min_token_text_ratio: float = 0.5, seed: Optional[int] = None, inputs_embeds=None, min_len: Optional[int] = None,
               max_len: Optional[int] = None, original_text_len: Optional[int] = None, top_p: Optional[float] = None,
               tau_r: Optional[float] = None) -> int:
        """Queue one utterance; returns its handle.  Non-blocking.  Either text (+ prompt_text, prompt_speech_token and the length
        ratios: cosy_request builds the prompt), or the low-level form inputs_embeds [T, D] / [1, T, D] with min_len, max_len and
        original_text_len.  sampling: the top_k of the nucleus."""
        fields, tau_r = self._request_fields(text, prompt_text, prompt_speech_token, sampling, max_token_text_ratio, min_token_text_ratio,
                                             inputs_embeds, min_len, max_len, original_text_len, top_p, tau_r)
        seed = int(fresh_seed() if seed is None else seed) & ((1 << 64) - 1)
        h = self.sched.submit(seed=seed, **fields)
        self._extra[h] = tau_r
        return h

    @torch.no_grad()
    def submit_n(self, n: int, text=None, prompt_text=None, prompt_speech_token=None, sampling: int = 25, max_token_text_ratio: float = 20,
                 min_token_text_ratio: float = 0.5, seed: Optional[int] = None, inputs_embeds=None, min_len: Optional[int] = None,
                 max_len: Optional[int] = None, original_text_len: Optional[int] = None, top_p: Optional[float] = None,
                 tau_r: Optional[float] = None) -> List[int]:
        """Queue n candidates of ONE utterance (submit()'s arguments; one cosy_request, one embeds tensor): their handles in
        candidate order.  Candidate i draws with the key candidate_seed(seed, i) and is, id for id, the request
        submit(..., seed=candidate_seed(seed, i)) would be.  The group is admitted whole, when n slots are free: the prompt is
        prefilled once and its cache row copied to the other candidates' rows.  n < 1 or n > slots: ValueError, nothing is queued."""
        n = int(n)
        if n < 1 or n > self.slots:
            raise ValueError(f"n = {n} candidates outside 1..{self.slots} (slots): a group is admitted whole")
        fields, tau_r = self._request_fields(text, prompt_text, prompt_speech_token, sampling, max_token_text_ratio, min_token_text_ratio,
                                             inputs_embeds, min_len, max_len, original_text_len, top_p, tau_r)
        seed = int(fresh_seed() if seed is None else seed) & ((1 << 64) - 1)
        if n == 1:
            hs = [self.sched.submit(seed=seed, **fields)]
        else:
            hs = self.sched.submit_group(n, [candidate_seed(seed, i) for i in range(n)], **fields)
        for h in hs:   # the scheduler's request does not carry tau_r: one entry per candidate
            self._extra[h] = tau_r
        return hs

    def take_logprobs(self, handle: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(tok_lp [n] fp32, cum_lp fp64 scalar, end_lp fp32 scalar) of a request that step() / run() / stream() has reported
        finished, all on the device: the log-probability of each of its n emitted ids under the raw logits (temperature 1, before
        top-k / top-p and the repetition test, over the ids the draw could produce), their sum, added in emission order in fp64, and
        the log-probability of the EOS draw that ended it (0 when it ran to its max_len instead).  Needs logprobs=True; a handle's
        result can be taken once."""
        if not self.logprobs:
            raise ValueError("take_logprobs needs ContinuousCosyDecoder(..., logprobs=True)")
        try:
            return self._lp_done.pop(handle)
        except KeyError:
            raise KeyError(f"handle {handle}: not finished yet (step() / run() / stream() has not reported it), unknown, or already taken") from None

    def _request_fields(self, text, prompt_text, prompt_speech_token, sampling, max_token_text_ratio, min_token_text_ratio, inputs_embeds,
                        min_len, max_len, original_text_len, top_p, tau_r) -> Tuple[dict, float]:
        """submit()'s argument checks and the prompt: (the scheduler request's fields but the handle and the seed, tau_r)."""
        if (text is None) == (inputs_embeds is None):
            raise ValueError("pass exactly one of text or inputs_embeds")
        if not 1 <= int(sampling) <= MAX_RAS_TOP_K:
            raise ValueError(f"sampling = {sampling}: the nucleus holds 1..{MAX_RAS_TOP_K} candidates")
        if text is not None:
            req = cosy_request(self.model, text, prompt_text, prompt_speech_token, sampling, max_token_text_ratio, min_token_text_ratio)
        else:
            if min_len is None or max_len is None or original_text_len is None:
                raise ValueError("inputs_embeds needs min_len, max_len and original_text_len")
            e = inputs_embeds.reshape(-1, inputs_embeds.shape[-1]).to(self.device, torch.bfloat16)
            req = CosyRequest(e.detach(), int(min_len), int(max_len), int(original_text_len))
        if req.embeds.shape[0] < 1 or req.embeds.shape[1] != self.model.config.hidden_size:
            raise ValueError(f"prompt of shape {tuple(req.embeds.shape)}")
        if not 1 <= req.limit <= self.cap:
            raise ValueError(f"max_len = {req.limit} outside 1..{self.cap} (max_len_cap)")
        fields = dict(embeds=req.embeds, max_new_tokens=req.limit, min_new_tokens=req.n_ignore, do_sample=True, top_k=int(sampling),
                      top_p=self.top_p if top_p is None else float(top_p))
        return fields, self.tau_r if tau_r is None else float(tau_r)

    @torch.no_grad()
    def step(self) -> List[Tuple[int, torch.Tensor]]:
        """Admit what fits, run up to check_every replays, retire what finished: [(handle, ids)] of the requests that finished."""
        rb = self._cycle()
        if rb is None:
            return []
        return [(self._retire(s, int(rb[2, s])), self.seq[s, :int(rb[2, s])].clone()) for s in self._ended(rb)]

    @torch.no_grad()
    def run(self) -> Dict[int, torch.Tensor]:
        """Step until everything submitted so far has finished: {handle: ids}."""
        out = {}
        while not self.sched.idle:
            for h, ids in self.step():
                out[h] = ids
        return out

    @torch.no_grad()
    def stream(self) -> Iterator[Tuple[int, torch.Tensor, bool]]:
        """Step until everything submitted so far has finished; at every read-back yield (handle, new_ids, finished) for each running
        request: the ids it emitted since the previous yield (a device int64 tensor, possibly empty).  The batched counterpart of
        inference() being a generator.  Costs the retirement's read-back and one gather of the new columns per read-back."""
        cur = StreamCursor(self.cap)
        while not self.sched.idle:
            rb = self._cycle()
            if rb is None:
                continue
            ended = set(self._ended(rb))
            running = [(s, self.sched.busy[s].handle, int(rb[2, s])) for s in sorted(self.sched.busy)]
            flat, counts = cur.take(running)
            idx = torch.tensor(flat, dtype=torch.int64).to(self.device, non_blocking=True)
            pieces = self.seq.view(-1).index_select(0, idx).split([n for _, n in counts])
            for s in sorted(ended):
                cur.finish(self._retire(s, int(rb[2, s])))
            for (s, h, _), piece in zip(running, pieces):
                yield h, piece, s in ended

    # ---- internals -----------------------------------------------------------------------------------------------------------
    def _ended(self, rb) -> List[int]:
        return [s for s in sorted(self.sched.busy) if not rb[0, s]]

    def _retire(self, s: int, n: int) -> int:
        """Slot s is free again: the handle of its request, whose n emitted ids' log-probabilities are kept for take_logprobs()."""
        h = self.sched.retire(s).handle
        if self.logprobs:
            self._lp_done[h] = (self.tok_lp[s, :n].clone(), self.cum_lp[s].clone(), self.end_lp[s].clone())
        return h

    def _cycle(self):
        """Admission, up to check_every replays, and the read-back: host int64 [3, slots] = (live, step, n_out), or None when no
        request runs."""
        self._admit()
        if not self.sched.busy:
            return None
        n = min(self.check_every, self.sched.longest())
        for _ in range(n):
            self.graph.replay()
        self.replays += n
        self.sched.advance(n)
        rb = torch.stack([self.live.to(torch.int64), self.step_t, self.n_out]).cpu()   # one small read-back
        if self.dstep.barrier_timed_out():
            raise _lib.Rwkv7HipError("rwkv7_decode_step_bf16: a grid barrier timed out; the generated ids are invalid")
        return rb

    def _admit(self):
        took = self.sched.admit()
        if not took:
            return
        m, dev = self.model, self.device
        # the requests that prefill: all of them, but for the candidates of a submit_n group after its first, which get a copy of its rows
        heads = [(s, r) for s, r in took if r.leader is None]
        slots = [s for s, _ in heads]
        if self.prefill is not None:
            h_last = self.prefill.run([r.embeds for _, r in heads], slots, fresh=True)
            logits = m.lm_head(h_last).float()
            if len(heads) < len(took):
                logits, slots = self._fan_out(took, heads, logits)
            row_slot = torch.tensor(slots, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
            return self._admit_draw(took, logits, row_slot.long(), row_slot)
        cu = [0]
        for _, r in heads:
            cu.append(cu[-1] + r.embeds.shape[0])
        rows64 = torch.tensor(slots, dtype=torch.int64).to(dev, non_blocking=True)
        for st in self.cache.states:   # a fresh state for every admitted request
            st.att_x_prev.index_fill_(0, rows64, 0)
            st.att_kv.index_fill_(0, rows64, 0)
            st.ffn_x_prev.index_fill_(0, rows64, 0)
        packed = torch.cat([r.embeds for _, r in heads], 0).unsqueeze(0)
        h = m.model(inputs_embeds=packed, cu_seqlens=torch.tensor(cu, dtype=torch.int32), past_key_values=self.cache,
                    cache_rows=torch.tensor(slots)).last_hidden_state
        last = torch.tensor([c - 1 for c in cu[1:]], dtype=torch.int64).to(dev, non_blocking=True)
        logits = m.lm_head(h[0].index_select(0, last)).float()
        if len(heads) < len(took):
            logits, slots = self._fan_out(took, heads, logits)
            rows64 = torch.tensor(slots, dtype=torch.int64).to(dev, non_blocking=True)
        self._admit_draw(took, logits, rows64, torch.tensor(slots, dtype=torch.int32).to(dev, non_blocking=True))

    def _fan_out(self, took, heads, logits):
        """submit_n: the prefilled rows of the groups' first candidates -> their siblings' rows, every field of every layer, for all
        groups admitted together in ONE rwkv7_cache_rows_commit_bf16 launch over the cache's own field table (a repeated source row
        fans out; no row is both read and written: sources are first candidates, destinations are not).  Returns (one logits row per
        admitted request -- its prompt's, gathered --, every admitted slot in `took` order)."""
        from .prefill import cache_field_table
        if self._fan_tbl is None:
            self._fan_tbl = cache_field_table(self.cache)
        return fan_out_rows(self.cache, self._fan_tbl, self.slots, self.model.config, self.device, took, heads, logits)

    def _admit_draw(self, took, logits, rows64, row_slot):
        # the slots' parameters: host mirror -> one copy per field; loop index, emitted count and ring pointer 0, an empty ring and
        # live = 1 for the admitted slots only (the device advances the other slots' state)
        ph = self._par_host
        for s, r in took:
            ph["limit"][s] = r.max_new_tokens
            ph["n_ignore"][s] = r.min_new_tokens
            ph["seed"][s] = r.seed - (1 << 64) if r.seed >= (1 << 63) else r.seed
            ph["top_k"][s] = r.top_k
            ph["top_p"][s] = r.top_p
            ph["tau_r"][s] = self._extra.pop(r.handle)
        for k, v in ph.items():
            self._par_dev[k].copy_(v.pin_memory(), non_blocking=True)
        self.step_t.index_fill_(0, rows64, 0)
        self.n_out.index_fill_(0, rows64, 0)
        self.ptr.index_fill_(0, rows64, 0)
        self.recent.index_fill_(0, rows64, -1)
        self.live.index_fill_(0, rows64, 1)
        if self.logprobs:
            self.cum_lp.index_fill_(0, rows64, 0)
            self.end_lp.index_fill_(0, rows64, 0)
        ras_slots(logits.contiguous(), self.st, row_slot, self.lp)
