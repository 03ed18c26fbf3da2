"""Continuous batching for the multi-channel XY model (RWKV7XYLM): the engine of continuous.py with an XY FRAME as its unit.

RWKV7XYLM.generate is a closed batch: one position counter and one `all finished` flag for the batch, one seed and one set of
sampling parameters, and a Philox counter that contains the batch row.  Here every one of up to 128 SLOTS runs its own request:

  * one captured step: DecodeStep (WideDecodeStep above 32 slots: decode.step_for) on the live cache with the C heads as ONE concatenated projection (channel 0 sliced to its audio
    rows, as generate does), then the two launches of csrc/xy_slots.hip: rwkv7_xy_slots_draw_f32 draws the C ids of every live
    slot with the slot's own key, frame counter and sampling parameters, rwkv7_xy_slots_frame_bf16 applies the frame rules
    (flush countdown, EOS / pad substitution, stopping) per slot, appends the frame, forms the next input embedding sum and
    advances the slot's counters;
  * admission as in ContinuousDecoder ("eager": packed prefill through RWKV7Model(..., cache_rows=...); "graph":
    prefill.PackedPrefill), the concatenated head on the last hidden rows, and the same two entries with row_slot for frame 0;
  * retirement: XY requests end on data (flush, EOS) as well as on budget.  Without an EOS id, and with channel 0 restricted to the
    audio range (so that the flush cannot start), the host knows every end and retires without read-back; otherwise it reads `live`
    and `step` back every `check_every` replays.

A request's draws use (its seed, its frame index, the channel) only, so its frames do not depend on its slot or on when it was
admitted (graph admission: for the same pack composition, see ContinuousDecoder).  head_column_map is the device-free part of the
setup: where each channel's logits sit in a row of the concatenated head.

Best-of-n (submit_n, logprobs=True, take_logprobs): n candidates of one prompt share one prefill -- the first candidate's cache row
is copied to its siblings' rows in one rwkv7_cache_rows_commit_bf16 launch (continuous.fan_out_rows) -- and the LP entries
rwkv7_xy_slots_draw_lp_f32 / rwkv7_xy_slots_frame_lp_bf16 write the log-probability of what every frame drew.  The frame rules may
replace a drawn id by a forced one (eos0 on channel 0 while flushing, the pad id on channel i once the countdown has passed it), so
a frame's value is known only after them: channel 0 COUNTS iff the flush had not started before the frame (the frame that starts it
still counts: the non-audio id was the model's choice), channel i >= 1 counts iff the frame keeps its drawn id; a forced entry is
+0.0 in frame_lp and adds nothing to cum_lp / n_lp.  rank_candidates orders a group by cum_lp with n_lp as the lengths; XY has no
teacher-forced scoring pass, so this is the model's only cheap ranking signal.  Not supported: stored states and overlapped
admission (this engine has neither).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .backbone import Cache
from .decode import check_slots, step_class, step_for
from .continuous import GroupScheduler, candidate_seed, fan_out_rows
from .sampling import MAX_DOMAIN, MAX_TOP_K, RowSampler, XYEmbed, fresh_seed

MAX_CHANNELS = 16


@dataclass(frozen=True)
class HeadColumns:
    """The concatenated XY head with channel 0 sliced to its audio rows: one logits row holds the audio range of channel 0, then
    channels 1.. back to back."""
    sizes: Tuple[int, ...]                  # ids of each channel's vocabulary (segment lengths of the draw)
    allow: Tuple[Tuple[int, int], ...]      # allowed id range per channel (channel 0: the audio range, in vocabulary ids)
    col0: Tuple[int, ...]                   # column at which each channel's allowed logits start
    seg_off: Tuple[int, ...]                # column of each channel's id 0 (negative for channel 0: ids keep vocabulary values)
    head0_rows: Tuple[int, int]             # rows of channel 0's head that are kept
    width: int                              # columns of a logits row
    max_domain: int                         # largest allowed range


def head_column_map(vocab_size: int, speech_vocab_size: int, num_channels: int, text_shift_size: int) -> HeadColumns:
    """Segment offsets, lengths and allowed ranges of the concatenated head for an XY configuration.  Pure: no device, no model."""
    V0, SV, C, shift = int(vocab_size), int(speech_vocab_size), int(num_channels), int(text_shift_size)
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"num_channels = {C}: 1..{MAX_CHANNELS}")
    if SV < 1 or shift < 0:
        raise ValueError(f"speech_vocab_size = {SV}, text_shift_size = {shift}")
    lo0, hi0 = shift, shift + SV
    if hi0 > V0:
        raise ValueError(f"the audio range [{lo0}, {hi0}) of channel 0 does not fit its vocabulary of {V0} ids")
    if SV > MAX_DOMAIN:
        raise ValueError(f"speech_vocab_size = {SV}: the draw covers at most {MAX_DOMAIN} ids per channel")
    sizes = (V0,) + (SV,) * (C - 1)
    allow = ((lo0, hi0),) + ((0, SV),) * (C - 1)
    col0 = tuple(SV * c for c in range(C))
    seg_off = tuple(c - a[0] for c, a in zip(col0, allow))
    return HeadColumns(sizes, allow, col0, seg_off, (lo0, hi0), SV * C, SV)


class XYSlotState(ctypes.Structure):
    """rwkv7_xy_slot_state (include/rwkv7_hip.h)."""
    _fields_ = [("step", ctypes.c_void_p), ("limit", ctypes.c_void_p), ("seed", ctypes.c_void_p), ("inv_temp", ctypes.c_void_p),
                ("top_k", ctypes.c_void_p), ("top_p", ctypes.c_void_p), ("do_sample", ctypes.c_void_p), ("live", ctypes.c_void_p),
                ("needs", ctypes.c_void_p), ("nt", ctypes.c_void_p), ("row", ctypes.c_void_p), ("seq", ctypes.c_void_p),
                ("seq_ld", ctypes.c_long), ("tables", ctypes.c_void_p * MAX_CHANNELS), ("x", ctypes.c_void_p), ("D", ctypes.c_int),
                ("C", ctypes.c_int), ("slots", ctypes.c_int), ("top_k_max", ctypes.c_int), ("text_shift", ctypes.c_long),
                ("speech_vocab", ctypes.c_long), ("pad", ctypes.c_long), ("eos0", ctypes.c_long), ("eos_list", ctypes.c_void_p),
                ("n_eos", ctypes.c_int), ("reference_termination", ctypes.c_int)]


class XYSlotLogprob(ctypes.Structure):
    """rwkv7_xy_slot_logprob (include/rwkv7_hip.h)."""
    _fields_ = [("ch_lp", ctypes.c_void_p), ("frame_lp", ctypes.c_void_p), ("cum_lp", ctypes.c_void_p), ("n_lp", ctypes.c_void_p)]


def xy_slots_draw(logits: torch.Tensor, st: XYSlotState, seg_off, seg_len, allow_lo, allow_hi, max_domain: int,
                  row_slot: Optional[torch.Tensor] = None, lp: Optional[XYSlotLogprob] = None):
    """rwkv7_xy_slots_draw_f32 on the current stream: logits fp32 [rows, width] (unit column stride); seg_off / seg_len / allow_lo /
    allow_hi int32 [C] device tensors (allow_*: both or None); row_slot int32 [rows] or None (row r is slot r).  With lp (ch_lp fp32
    [slots, C], frame_lp fp32 [slots, seq_ld, C], cum_lp fp64 [slots], n_lp int64 [slots]): rwkv7_xy_slots_draw_lp_f32, the same
    draw plus ch_lp."""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    if row_slot is not None:
        assert row_slot.dtype == torch.int32 and row_slot.is_contiguous() and row_slot.numel() == logits.shape[0]
    args = (logits.shape[0], logits, logits.stride(0), row_slot, seg_off, seg_len, allow_lo, allow_hi, int(max_domain), ctypes.byref(st))
    if lp is None:
        _lib.call("rwkv7_xy_slots_draw_f32", logits, *args)
    else:
        _lib.call("rwkv7_xy_slots_draw_lp_f32", logits, *args, ctypes.byref(lp))


def xy_slots_frame(rows: int, st: XYSlotState, device, row_slot: Optional[torch.Tensor] = None, lp: Optional[XYSlotLogprob] = None):
    """rwkv7_xy_slots_frame_bf16 on the current stream of `device`, for `rows` rows (row_slot as in xy_slots_draw).  With lp:
    rwkv7_xy_slots_frame_lp_bf16, the same frame plus the accounting of the counted channels (frame_lp, cum_lp, n_lp)."""
    if row_slot is not None:
        assert row_slot.dtype == torch.int32 and row_slot.is_contiguous() and row_slot.numel() == rows
    if lp is None:
        _lib.call("rwkv7_xy_slots_frame_bf16", device, int(rows), row_slot, ctypes.byref(st))
    else:
        _lib.call("rwkv7_xy_slots_frame_lp_bf16", device, int(rows), row_slot, ctypes.byref(st), ctypes.byref(lp))


class ContinuousXYDecoder:
    """eng = ContinuousXYDecoder(model, slots=32, ...); h = eng.submit(input_ids [T, C], ...); eng.step() -> [(handle, frames)];
    eng.run() -> {handle: frames}.

    model: a bf16 RWKV7XYLM on the HIP device that the step kernel covers; slots in 1..32, or 64, 96 or 128.  A request's frames are a device int64
    [n, C] tensor: the frames up to and including the one on which the request ended (budget, EOS on channel 0, or the end of a
    flush) -- the rows RWKV7XYLM.generate would append for B = 1.  Channel 0 is restricted to the audio range, as in generate, and
    its head is sliced to those rows (the full 66 661-id head is outside the draw's domain).  eos_token_id: a channel-0 id that ends a
    request when it is drawn.  admission / prefill_max_seqs / prefill_buckets: as in ContinuousDecoder.

    Best-of-n: submit_n(n, ...) queues n candidates of one prompt, admitted together (GroupScheduler), the prompt prefilled once and
    its cache row copied to the siblings' rows (_fan_out).  logprobs=True makes the captured step and the admission draw call the
    LP entries, which also write, per emitted frame, the log-probability under the raw logits of every channel whose drawn id the
    frame rules kept (frame_lp [slots, cap, C] fp32; +0.0 where the id was forced -- see the module docstring for the rule), their
    running fp64 sum (cum_lp [slots]) and their number (n_lp [slots]).  take_logprobs(handle) hands them out once the handle has
    been reported finished, and continuous.rank_candidates orders a group:

        hs = eng.submit_n(4, prompt, do_sample=True, top_k=50, seed=7); out = eng.run()
        lp = [eng.take_logprobs(h) for h in hs]                                   # (frame_lp[:n], cum_lp, n_lp) per candidate
        best = hs[rank_candidates([c for _, c, _ in lp], [n for _, _, n in lp])[0]]

    logprobs=True changes no frame; with logprobs=False and no submit_n every launch is the one of before.  Stored states and
    overlapped admission are not supported (this engine has neither)."""

    logprobs = False   # the default of the constructor's switch; nothing below looks at frame_lp / cum_lp / n_lp without it
    lp = None          # XYSlotLogprob with logprobs=True: the frames go through the LP entries

    def __init__(self, model, slots: int = 32, max_new_frames_cap: int = 3000, eos_token_id: Optional[int] = None, check_every: int = 16,
                 admission: str = "eager", prefill_max_seqs: int = 8, prefill_buckets: Sequence[int] = (256, 512, 1024, 2048, 4096),
                 logprobs: bool = False):
        if admission not in ("eager", "graph"):
            raise ValueError(f"admission = {admission!r}: 'eager' or 'graph'")
        self.logprobs = bool(logprobs)
        check_slots(slots)   # 1..32, or 64 / 96 / 128: ValueError before anything touches the device
        if max_new_frames_cap < 1 or check_every < 1:
            raise ValueError("max_new_frames_cap and check_every must be >= 1")
        cfg = model.config
        self.cols = cm = head_column_map(cfg.vocab_size, cfg.speech_vocab_size, cfg.num_channels, cfg.text_shift_size)
        self.eos = None if eos_token_id is None else int(eos_token_id)
        if self.eos is not None and not 0 <= self.eos < cfg.vocab_size:
            raise ValueError(f"eos_token_id = {self.eos} is not a channel-0 id (0..{cfg.vocab_size - 1})")
        if not 0 <= int(cfg.speech_pad_token) < cfg.speech_vocab_size:
            raise ValueError(f"speech_pad_token = {cfg.speech_pad_token} is not a speech id")
        self.admission = admission
        self.model = m = model.eval()
        dev = m.device
        if dev.type != "cuda":
            raise ValueError("ContinuousXYDecoder needs the model on the HIP device")
        self.device, self.slots, self.cap, self.check_every = dev, slots, int(max_new_frames_cap), int(check_every)
        C, D = cfg.num_channels, cfg.hidden_size
        self.C = C
        if [h.weight.shape[0] for h in m.heads] != list(cm.sizes):
            raise ValueError("the model's heads do not match its configuration")
        lo0, hi0 = cm.head0_rows
        self.head = SimpleNamespace(
            weight=torch.cat([m.heads[0].weight.detach()[lo0:hi0]] + [h.weight.detach() for h in m.heads[1:]], 0).contiguous(),
            bias=torch.cat([m.heads[0].bias.detach()[lo0:hi0]] + [h.bias.detach() for h in m.heads[1:]], 0).contiguous())
        self.cache = Cache.zeros(cfg, slots, dev, m.dtype)
        why = step_class(slots).supported(m.model, self.head, self.cache)
        if why is None and m.dtype != torch.bfloat16:
            why = "the model must be bf16"
        self.tables = [e.weight.detach() for e in m.embs]
        if why is None and not XYEmbed.supported(self.tables):
            why = "the channel embedding tables must be contiguous bf16 [V_c, D] with D % 8 == 0, at most 16 of them"
        if why is None:
            why = RowSampler.supported(dev, list(cm.sizes), list(cm.allow), None)
        if why is None and any(t.shape[0] < hi for t, (_, hi) in zip(self.tables, cm.allow)):
            why = "an embedding table has fewer rows than its channel draws ids"
        if why:
            raise ValueError("ContinuousXYDecoder needs the persistent decode step and the fused frame: " + why)
        # ends that only the device sees: an EOS id, or a flush (a non-audio id on channel 0: impossible while it is restricted to the audio range)
        self.data_end = self.eos is not None or cm.allow[0] != cm.head0_rows

        i32 = dict(dtype=torch.int32, device=dev)
        l64 = dict(dtype=torch.int64, device=dev)
        self.seg_off, self.seg_len = torch.tensor(cm.seg_off, **i32), torch.tensor(cm.sizes, **i32)
        self.allow_lo, self.allow_hi = torch.tensor([a[0] for a in cm.allow], **i32), torch.tensor([a[1] for a in cm.allow], **i32)
        S = slots
        self.step_t = torch.zeros(S, **l64)
        self.needs = torch.full((S,), -1, **l64)
        self.live = torch.zeros(S, dtype=torch.uint8, device=dev)
        self.nt = torch.zeros(S, C, **l64)
        self.row = torch.zeros(S, C, **l64)
        self.seq = torch.zeros(S, self.cap, C, **l64)
        self.x = torch.zeros(S, D, dtype=torch.bfloat16, device=dev)
        self.eos_list = None if self.eos is None else torch.tensor([self.eos], **l64)
        # the parameters the device never writes: one block, mirrored on the host and copied whole at admission
        self._par_host = {"limit": torch.ones(S, dtype=torch.int64), "seed": torch.zeros(S, dtype=torch.int64),
                          "inv_temp": torch.ones(S, dtype=torch.float32), "top_k": torch.zeros(S, dtype=torch.int32),
                          "top_p": torch.ones(S, dtype=torch.float32), "do_sample": torch.zeros(S, dtype=torch.uint8)}
        self._par_dev = {k: torch.empty_like(v, device=dev) for k, v in self._par_host.items()}
        for k, v in self._par_host.items():
            self._par_dev[k].copy_(v)
        st, pd = XYSlotState(), self._par_dev
        st.step, st.limit, st.seed = self.step_t.data_ptr(), pd["limit"].data_ptr(), pd["seed"].data_ptr()
        st.inv_temp, st.top_k, st.top_p, st.do_sample = (pd[k].data_ptr() for k in ("inv_temp", "top_k", "top_p", "do_sample"))
        st.live, st.needs, st.nt, st.row, st.seq = (t.data_ptr() for t in (self.live, self.needs, self.nt, self.row, self.seq))
        st.seq_ld = self.cap
        for c, t in enumerate(self.tables):
            st.tables[c] = t.data_ptr()
        st.x, st.D, st.C, st.slots, st.top_k_max = self.x.data_ptr(), D, C, S, MAX_TOP_K
        st.text_shift, st.speech_vocab, st.pad = cfg.text_shift_size, cfg.speech_vocab_size, int(cfg.speech_pad_token)
        st.eos0 = -1 if self.eos is None else self.eos
        st.eos_list, st.n_eos = (None, 0) if self.eos_list is None else (self.eos_list.data_ptr(), 1)
        st.reference_termination = 0
        self.st = st
        if self.logprobs:   # what the LP entries write next to nt / seq
            self.ch_lp = torch.zeros(S, C, dtype=torch.float32, device=dev)
            self.frame_lp = torch.zeros(S, self.cap, C, dtype=torch.float32, device=dev)
            self.cum_lp = torch.zeros(S, dtype=torch.float64, device=dev)
            self.n_lp = torch.zeros(S, **l64)
            self.lp = XYSlotLogprob(self.ch_lp.data_ptr(), self.frame_lp.data_ptr(), self.cum_lp.data_ptr(), self.n_lp.data_ptr())
        self._lp_done: Dict[int, Tuple[torch.Tensor, torch.Tensor, int]] = {}   # handle -> its values until take_logprobs()
        self._fan_tbl = None   # submit_n: the cache's own field table, source and destination of the fan-out copy

        self.sched = GroupScheduler(slots)   # for groups of one its admit() is SlotScheduler's
        self.dstep = step_for(m.model, self.head, self.cache)
        # capture the step with every slot idle (live = 0): the frame kernels write nothing, and what the warm-up does to the state
        # of idle rows does not matter (admission resets a row before it is used)
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

    def _frame(self, logits, row_slot=None):
        xy_slots_draw(logits, self.st, self.seg_off, self.seg_len, self.allow_lo, self.allow_hi, self.cols.max_domain, row_slot, self.lp)
        xy_slots_frame(logits.shape[0], self.st, self.device, row_slot, self.lp)

    def _step(self):
        self._frame(self.dstep(self.x))

    # ---- public interface ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def submit(self, input_ids, max_new_frames: int = 256, do_sample: bool = False, temperature: float = 1.0, top_k: int = 0,
               top_p: float = 1.0, seed: Optional[int] = None) -> int:
        """Queue one request (a prompt of T frames: int64 ids [T, C] or [1, T, C]); returns its handle.  Non-blocking."""
        fields = self._request_fields(input_ids, max_new_frames, do_sample, temperature, top_k, top_p)
        seed = int(fresh_seed() if seed is None else seed) & ((1 << 64) - 1)
        return self.sched.submit(seed=seed, **fields)

    @torch.no_grad()
    def submit_n(self, n: int, input_ids, max_new_frames: int = 256, do_sample: bool = False, temperature: float = 1.0, top_k: int = 0,
                 top_p: float = 1.0, seed: Optional[int] = None) -> List[int]:
        """Queue n candidates of ONE prompt (submit()'s arguments): their handles in candidate order.  Candidate i draws with the key
        candidate_seed(seed, i) and is, frame for frame, the request submit(..., seed=candidate_seed(seed, i)) would be.  The group is
        admitted whole, when n slots are free: the prompt is prefilled once and its cache row copied to the other candidates' rows.
        n < 1 or n > slots: ValueError; n > 1 needs a seed (the candidates' keys are derived from it, and a result that cannot be
        reproduced cannot be ranked again): ValueError without one.  Nothing is queued then."""
        n = int(n)
        if n < 1 or n > self.slots:
            raise ValueError(f"n = {n} candidates outside 1..{self.slots} (slots): a group is admitted whole")
        if n > 1 and seed is None:
            raise ValueError(f"submit_n with n = {n} needs a seed: candidate i draws with candidate_seed(seed, i)")
        fields = self._request_fields(input_ids, max_new_frames, do_sample, temperature, top_k, top_p)
        seed = int(fresh_seed() if seed is None else seed) & ((1 << 64) - 1)
        if n == 1:
            return [self.sched.submit(seed=seed, **fields)]
        return self.sched.submit_group(n, [candidate_seed(seed, i) for i in range(n)], **fields)

    def take_logprobs(self, handle: int) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """(frame_lp [n, C] fp32, cum_lp fp64 scalar, n_lp int) of a request that step() / run() has reported finished, the tensors on
        the device: per emitted frame and channel the log-probability of the drawn id under the raw logits (temperature 1, before
        top-k / top-p, over the channel's allowed ids) where the frame rules kept the draw and +0.0 where they forced the id; the sum
        of the counted values, added in (frame, channel) order in fp64; and their number, the length for
        rank_candidates(length_normalize=True).  Needs logprobs=True; a handle's result can be taken once."""
        if not self.logprobs:
            raise ValueError("take_logprobs needs ContinuousXYDecoder(..., logprobs=True)")
        try:
            return self._lp_done.pop(handle)
        except KeyError:
            raise KeyError(f"handle {handle}: not finished yet (step() / run() has not reported it), unknown, or already taken") from None

    def _request_fields(self, input_ids, max_new_frames, do_sample, temperature, top_k, top_p) -> dict:
        """submit()'s argument checks and the prompt's embeddings: the scheduler request's fields but the handle and the seed."""
        if not 1 <= int(max_new_frames) <= self.cap:
            raise ValueError(f"max_new_frames = {max_new_frames} outside 1..{self.cap} (max_new_frames_cap)")
        top_k, top_p = int(top_k or 0), 1.0 if top_p is None else float(top_p)
        why = RowSampler.supported(self.device, list(self.cols.sizes), list(self.cols.allow), None, do_sample, top_k, top_p, temperature)
        if why:
            raise ValueError("rwkv7_xy_slots_draw_f32: " + why)
        ids = torch.as_tensor(input_ids)
        if ids.dim() == 3 and ids.shape[0] == 1:
            ids = ids[0]
        if ids.dim() != 2 or ids.shape[1] != self.C or ids.shape[0] < 1 or ids.dtype != torch.int64:
            raise ValueError(f"input_ids must be int64 of shape (T, {self.C}) with T >= 1, got {tuple(ids.shape)} {ids.dtype}")
        e = self.model.embed(ids.to(self.device).unsqueeze(0))[0]
        return dict(embeds=e.detach(), max_new_tokens=int(max_new_frames), do_sample=bool(do_sample),
                    temperature=float(temperature or 1.0), top_k=top_k, top_p=top_p)

    @torch.no_grad()
    def step(self) -> List[Tuple[int, torch.Tensor]]:
        """Admit what fits, run up to check_every replays, retire what finished: [(handle, frames)] of the requests that finished."""
        done = []
        if not self.data_end:
            done += self._retire(self.sched.due(), None)
        self._admit()
        if not self.data_end:
            done += self._retire(self.sched.due(), None)   # max_new_frames = 1: finished with its first frame
            n = min(self.check_every, self.sched.replays_until_due())
        else:
            n = min(self.check_every, self.sched.longest())
        if not self.sched.busy:
            return done
        for _ in range(n):
            self.graph.replay()
        self.replays += n
        self.sched.advance(n)
        if not self.data_end:
            done += self._retire(self.sched.due(), None)
        else:
            both = torch.stack([self.live.to(torch.int64), self.step_t]).cpu()   # one small read-back
            done += self._retire([s for s in sorted(self.sched.busy) if not both[0, s]], both[1])
        if self.dstep.barrier_timed_out():
            raise _lib.Rwkv7HipError("rwkv7_decode_step_bf16: a grid barrier timed out; the generated frames are invalid")
        return done

    @torch.no_grad()
    def run(self) -> Dict[int, torch.Tensor]:
        """Step until everything submitted so far has finished: {handle: frames}."""
        out = {}
        while not self.sched.idle:
            for h, frames in self.step():
                out[h] = frames
        return out

    # ---- internals -----------------------------------------------------------------------------------------------------------
    def _retire(self, slots, steps) -> List[Tuple[int, torch.Tensor]]:
        out, counted = [], None
        for s in slots:
            req = self.sched.retire(s)
            n = req.max_new_tokens if steps is None else int(steps[s])
            out.append((req.handle, self.seq[s, :n].clone()))
            if self.logprobs:
                counted = self.n_lp.cpu() if counted is None else counted   # one read-back for all slots retired together
                self._lp_done[req.handle] = (self.frame_lp[s, :n].clone(), self.cum_lp[s].clone(), int(counted[s]))
        return out

    def _head(self, h):
        return torch.nn.functional.linear(h, self.head.weight, self.head.bias).float()

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
            logits = self._head(h_last)
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
        logits = self._head(h[0].index_select(0, last))
        if len(heads) < len(took):
            logits, slots = self._fan_out(took, heads, logits)
            rows64 = torch.tensor(slots, dtype=torch.int64).to(dev, non_blocking=True)
        self._admit_draw(took, logits, rows64, torch.tensor(slots, dtype=torch.int32).to(dev, non_blocking=True))

    def _fan_out(self, took, heads, logits):
        """submit_n: continuous.fan_out_rows over this engine's cache -- the first candidates' prefilled rows -> their siblings' rows
        in one launch; (one logits row per admitted request, every admitted slot in `took` order)."""
        if self._fan_tbl is None:
            from .prefill import cache_field_table
            self._fan_tbl = cache_field_table(self.cache)
        return fan_out_rows(self.cache, self._fan_tbl, self.slots, self.model.config, self.device, took, heads, logits)

    def _admit_draw(self, took, logits, rows64, row_slot):
        # the slots' parameters: host mirror -> one copy per field; step = 0, needs = -1 and live = 1 for the admitted slots only (the
        # device advances the other slots' counters)
        ph = self._par_host
        for s, r in took:
            ph["limit"][s] = r.max_new_tokens
            ph["seed"][s] = r.seed - (1 << 64) if r.seed >= (1 << 63) else r.seed
            ph["inv_temp"][s] = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(r.temperature, dtype=torch.float32)
                                 if r.do_sample else torch.tensor(1.0))
            ph["top_k"][s] = r.top_k if r.do_sample else 0
            ph["top_p"][s] = r.top_p
            ph["do_sample"][s] = int(r.do_sample)
        for k, v in ph.items():
            self._par_dev[k].copy_(v.pin_memory(), non_blocking=True)
        self.step_t.index_fill_(0, rows64, 0)
        self.needs.index_fill_(0, rows64, -1)
        self.live.index_fill_(0, rows64, 1)
        if self.logprobs:
            self.cum_lp.index_fill_(0, rows64, 0)
            self.n_lp.index_fill_(0, rows64, 0)
        self._frame(logits.contiguous(), row_slot)
