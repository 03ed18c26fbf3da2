"""CPU: the continuous-batching pieces that need no device -- the per-slot draw entry rejects bad arguments before it launches,
and SlotScheduler (the FIFO queue, free slots and budgets of rwkvtts_amd/continuous.ContinuousDecoder) admits, retires and
returns requests correctly."""
import ctypes
import random

import pytest

from rwkvtts_amd import _lib
from rwkvtts_amd.continuous import SlotScheduler, SlotState


def _state(**kw):
    st = SlotState()
    for name in ("step", "limit", "min_until", "seed", "inv_temp", "top_k", "top_p", "do_sample", "live", "ids", "seq", "emb", "x"):
        setattr(st, name, 16)   # never dereferenced: the checks fire first
    st.seq_ld, st.D, st.slots, st.top_k_max, st.eos = 8, 64, 4, 64, -1
    for k, v in kw.items():
        setattr(st, k, v)
    return st


def test_sample_slots_is_exported(hip_lib):
    assert "rwkv7_sample_slots_f32" in _lib.exported_symbols()
    assert hasattr(hip_lib, "rwkv7_sample_slots_f32")


def test_sample_slots_argument_errors_do_not_launch(hip_lib):
    one = ctypes.c_void_p(16)
    f = hip_lib.rwkv7_sample_slots_f32

    def call(rows=4, st=None, max_domain=1024, nsuppress=0, suppress=None, allow=(None, None), logits=one):
        st = _state() if st is None else st
        return f(rows, logits, ctypes.c_long(1024), None, allow[0], allow[1], suppress, nsuppress, max_domain,
                 ctypes.byref(st) if st is not False else None, None)

    assert call(rows=0) == -1
    assert call(rows=-3) == -1
    assert call(st=False) == -1                               # null st
    assert call(logits=None) == -1
    assert call(max_domain=0) == -1
    assert call(nsuppress=2) == -1                            # suppress count without the list
    assert call(allow=(one, None)) == -1                      # half an allowed range
    assert call(st=_state(step=None)) == -1
    assert call(st=_state(live=None)) == -1
    assert call(st=_state(seq_ld=0)) == -1
    assert call(st=_state(slots=0)) == -1
    assert call(st=_state(x=None)) == -1                      # emb without x
    assert call(st=_state(top_k_max=65)) == -4                # top_k out of range
    assert call(st=_state(top_k_max=-1)) == -4
    assert call(max_domain=15361) == -4
    assert call(nsuppress=257, suppress=one) == -4
    assert call(st=_state(D=100)) == -4                       # D % 8 != 0


def _sched(slots, budgets):
    s = SlotScheduler(slots)
    hs = [s.submit(embeds=None, max_new_tokens=b) for b in budgets]
    return s, hs


def test_admits_in_fifo_order_and_never_shares_a_slot():
    s, hs = _sched(3, [5, 5, 5, 5, 5])
    took = s.admit()
    assert [r.handle for _, r in took] == hs[:3]
    assert sorted(slot for slot, _ in took) == [0, 1, 2]
    assert s.admit() == []                                    # no free slot: nothing more is admitted
    assert [r.handle for r in s.pending] == hs[3:]
    assert len(set(s.busy)) == len(s.busy) == 3


def test_reuses_a_slot_only_after_retirement():
    s, hs = _sched(2, [3, 10, 4])
    s.admit()
    s.advance(1)
    assert s.admit() == []
    s.advance(1)                                              # the 3-token request has drawn its 3rd id
    assert s.due() == [0]
    assert s.retire(0).handle == hs[0]
    (slot, req), = s.admit()
    assert slot == 0 and req.handle == hs[2]
    assert s.retire(0).handle == hs[2]                        # (EOS: retired before its budget)
    with pytest.raises(KeyError):
        s.retire(0)                                           # once per admission
    assert s.free == [0]


def test_retires_budget_limited_requests_on_the_exact_step():
    budgets = [1, 2, 7, 16, 33]
    s, hs = _sched(len(budgets), budgets)
    s.admit()
    assert s.due() == [0]                                     # max_new_tokens = 1: done with the id drawn at admission
    s.retire(0)
    replays, finished = 0, {}
    while s.busy:
        n = s.replays_until_due()
        assert n >= 1
        s.advance(n)
        replays += n
        for slot in s.due():
            finished[s.retire(slot).handle] = replays
    # a request of budget b is retired after exactly b - 1 replays (its first id comes from admission)
    assert finished == {h: b - 1 for h, b in zip(hs[1:], budgets[1:])}


def test_submit_during_a_run_and_every_handle_returns_once():
    rng = random.Random(3)
    s = SlotScheduler(4)
    expected, returned, replays = {}, [], 0
    for _ in range(6):
        b = rng.randint(1, 20)
        expected[s.submit(embeds=None, max_new_tokens=b)] = b
    started = {}
    while not s.idle:
        for slot in s.due():
            req = s.retire(slot)
            returned.append(req.handle)
            assert replays - started[req.handle] == req.max_new_tokens - 1
        for slot, req in s.admit():
            started[req.handle] = replays
        for slot in s.due():   # budget 1
            req = s.retire(slot)
            returned.append(req.handle)
        if s.busy:
            n = min(4, s.replays_until_due())
            s.advance(n)
            replays += n
        if len(expected) < 20:   # more requests arrive while the batch runs
            b = rng.randint(1, 20)
            expected[s.submit(embeds=None, max_new_tokens=b)] = b
    assert sorted(returned) == sorted(expected) and len(returned) == len(set(returned)) == 20
    assert s.free == [0, 1, 2, 3]


def test_bad_budget_is_rejected():
    with pytest.raises(ValueError):
        SlotScheduler(2).submit(embeds=None, max_new_tokens=0)
    with pytest.raises(ValueError):
        SlotScheduler(0)
