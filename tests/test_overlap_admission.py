"""CPU: the device-free parts of ContinuousDecoder(admission="overlap") -- OverlapScheduler (reserve / commit next to SlotScheduler's
admit / advance / retire), the engine's step loop with its two device halves stubbed out, against a hand-rolled model of the schedule
rule, and the argument checks of rwkv7_cache_rows_commit_bf16 and of the host-side row check."""
import ctypes
import random

import pytest
import torch

from rwkvtts_amd import _lib
from rwkvtts_amd.continuous import ContinuousDecoder, OverlapScheduler, SlotScheduler
from rwkvtts_amd.prefill import check_commit_rows


def _sched(slots, budgets):
    s = OverlapScheduler(slots)
    return s, [s.submit(embeds=None, max_new_tokens=b) for b in budgets]


# ---------------------------------------------------------------------------------------------------------------- scheduler
def test_reserve_is_fifo_into_the_lowest_free_slots_up_to_the_limit():
    s, hs = _sched(4, [5, 6, 7, 8, 9, 10])
    took = s.reserve(3)
    assert [(slot, r.handle) for slot, r in took] == [(0, hs[0]), (1, hs[1]), (2, hs[2])]   # limit 3 < 4 free slots
    assert s.free == [3] and not s.busy and not s.remaining and s.staged == took
    with pytest.raises(RuntimeError):
        s.reserve(3)                                          # one staged group at a time
    assert [r.handle for r in s.pending] == hs[3:]
    assert s.commit() == took and sorted(s.busy) == [0, 1, 2]
    assert s.remaining == {0: 4, 1: 5, 2: 6}                  # max_new_tokens - 1: the first id comes with the commit
    took2 = s.reserve(8)                                      # one free slot: one request
    assert [(slot, r.handle) for slot, r in took2] == [(3, hs[3])]
    with pytest.raises(ValueError):
        OverlapScheduler(2).reserve(0)


def test_a_staged_request_is_neither_free_nor_busy_nor_due():
    s, hs = _sched(2, [1, 1, 3])
    s.reserve(2)
    assert s.due() == [] and not s.busy and s.free == []      # budget 1, but nothing is due before the commit
    assert not s.idle and not s.can_launch()
    s.advance(5)                                              # replays of the other slots leave the staged group alone
    assert s.since == 5 and s.due() == [] and s.remaining == {}
    s.commit()
    assert s.due() == [0, 1]                                  # now they are: finished with their first id
    for slot in (0, 1):
        s.retire(slot)
    assert s.free == [0, 1] and s.can_launch()


def test_idle_is_false_while_a_group_is_staged():
    s, _ = _sched(2, [4])
    assert not s.idle
    s.reserve(2)
    assert not s.pending and not s.busy and not s.idle
    s.commit()
    s.advance(3)
    s.retire(0)
    assert s.idle


def test_replays_until_commit_counts_from_reserve():
    s, _ = _sched(3, [20, 20, 20])
    s.reserve(1)
    s.commit()                                                # slot 0 busy
    assert s.replays_until_commit(8) == 0                     # nothing staged
    s.reserve(1)
    assert s.replays_until_commit(8) == 8 and not s.commit_due(8) and s.commit_due(0)
    s.advance(3)
    assert s.replays_until_commit(8) == 5 and s.next_replays(16, 8) == 5
    s.advance(5)
    assert s.replays_until_commit(8) == 0 and s.commit_due(8)
    s.commit()
    s.reserve(1)
    assert s.since == 0 and s.replays_until_commit(8) == 8    # the count restarts with every group
    s2, _ = _sched(2, [9])
    s2.reserve(2)
    assert s2.commit_due(64)                                  # nothing busy: commit at once, whatever the lag


def test_the_base_scheduler_is_unchanged_by_the_subclass():
    a, b = SlotScheduler(3), OverlapScheduler(3)
    for s in (a, b):
        for n in (3, 1, 7, 2):
            s.submit(embeds=None, max_new_tokens=n)
    assert [(sl, r.handle) for sl, r in a.admit()] == [(sl, r.handle) for sl, r in b.admit()]
    for s in (a, b):
        s.advance(2)
    assert a.due() == b.due() == [0, 1] and a.remaining == b.remaining and b.since == 0
    assert not hasattr(a, "staged")


# ---------------------------------------------------------------------------------------------------------------- schedule
class _Graph:
    def __init__(self):
        self.count = 0

    def replay(self):
        self.count += 1


class _NoBarrier:
    def barrier_timed_out(self):
        return False


class HostOnlyEngine(ContinuousDecoder):
    """ContinuousDecoder's overlap step loop with the two device halves of an admission stubbed out: what remains is host code."""

    def __init__(self, slots, overlap_replays, check_every=16, stage_rows=2, cap=64):
        self.admission, self.overlap_replays, self.check_every, self.eos = "overlap", overlap_replays, check_every, None
        self.slots, self.stage_rows, self.replays, self.admission_log = slots, stage_rows, 0, []
        self.sched, self.graph, self.dstep = OverlapScheduler(slots), _Graph(), _NoBarrier()
        self.seq = torch.zeros(slots, cap, dtype=torch.int64)
        self._launched_at = 0
        self.events, self.retired_at = [], {}

    def submit(self, budget):
        return self.sched.submit(embeds=None, max_new_tokens=budget)

    def _retire(self, slots, steps):
        for s in slots:
            self.retired_at[self.sched.busy[s].handle] = self.replays
        return super()._retire(slots, steps)

    def _launch_device(self, took):
        self.events.append(("launch", self.replays, sorted(self.sched.busy), [(s, r.handle) for s, r in took]))

    def _commit_device(self, took):
        before = sorted(set(self.sched.busy) - {s for s, _ in took})   # the scheduler has already made the group busy
        assert len(before) + len(took) == len(self.sched.busy)
        self.events.append(("commit", self.replays, before, [(s, r.handle) for s, r in took]))


def _model(budgets, slots, lag, check_every, stage_rows):
    """The rule of ContinuousDecoder._step_overlap restated on plain lists: per step() retire what is due; commit the group in flight
    once `lag` replays have been issued since its launch or nothing is busy; with nothing in flight, pending requests and free slots,
    launch (and commit at once under the same condition); replay min(check_every, until the next budget end, until the commit).
    Returns (total replays, log of (launch, commit, handles), {handle: (slot, replay count at retirement)})."""
    pending, free, rem, owner = list(range(len(budgets))), list(range(slots)), {}, {}
    staged, since, launched, replays, log, retired = [], 0, 0, 0, [], {}

    def retire():
        for s in sorted(s for s, r in rem.items() if r == 0):
            retired[owner.pop(s)] = (s, replays)
            del rem[s]
            free.append(s)
            free.sort()

    def commit():
        nonlocal staged
        for s, h in staged:
            rem[s], owner[s] = budgets[h] - 1, h
        log.append((launched, replays, [h for _, h in staged]))
        staged = []

    while pending or rem or staged:
        retire()
        if staged and (since >= lag or not rem):
            commit()
        if not staged and pending and free:
            while pending and free and len(staged) < stage_rows:
                staged.append((free.pop(0), pending.pop(0)))
            since, launched = 0, replays
            if since >= lag or not rem:
                commit()
        retire()
        if not rem:
            continue
        n = min(check_every, min(rem.values()))
        if staged:
            n = min(n, lag - since)
            since += n
        assert n >= 1
        for s in rem:
            rem[s] -= n
        replays += n
    return replays, log, retired


@pytest.mark.parametrize("lag", [0, 3, 8])
def test_schedule_of_forty_requests_through_four_slots(lag):
    rng = random.Random(100 + lag)
    budgets = [rng.choice([1, 2, 5, 9, 17, 30, 41]) if i % 3 else rng.randint(1, 60) for i in range(40)]

    def run():
        eng = HostOnlyEngine(4, lag)
        hs = [eng.submit(b) for b in budgets[:25]]
        out, steps = {}, 0
        while not eng.sched.idle:
            for h, ids in eng.step():
                assert h not in out                           # every handle returns once
                out[h] = ids
            steps += 1
            assert steps < 10000
        return eng, hs, out

    eng, hs, out = run()
    # the rest arrives after the first batch has drained: the engine starts again from idle
    more = [eng.submit(b) for b in budgets[25:]]
    for h, ids in eng.run().items():
        assert h not in out
        out[h] = ids
    assert hs + more == list(range(40)) and sorted(out) == list(range(40))
    assert all(out[h].numel() == budgets[h] for h in out)
    # every request admitted exactly once, in FIFO order, at most stage_rows per group
    admitted = [h for _, _, g in eng.admission_log for h in g]
    assert admitted == list(range(40)) and all(1 <= len(g) <= 2 for _, _, g in eng.admission_log)
    # no slot double-booked: a launch never takes a busy slot or one still staged, and a commit fills only slots that are not busy
    held = {}
    for kind, at, busy, took in eng.events:
        for s, h in took:
            assert s not in busy, (kind, at, s, busy)
            if kind == "launch":
                assert s not in held
                held[s] = h
            else:
                assert held.pop(s) == h
    assert not held
    # a commit comes `lag` replays after its launch, or earlier only when nothing was busy
    launches = [e for e in eng.events if e[0] == "launch"]
    commits = [e for e in eng.events if e[0] == "commit"]
    assert len(launches) == len(commits) == len(eng.admission_log)
    for (_, a, _, _), (_, b, busy, _), (la, lb, _) in zip(launches, commits, eng.admission_log):
        assert (a, b) == (la, lb) and 0 <= b - a <= lag
        assert b - a == lag or not busy
    # the engine's total and its log equal the hand-rolled model (two batches: 25 requests, then 15 into the drained engine)
    r1, log1, _ = _model(budgets[:25], 4, lag, 16, 2)
    r2, log2, _ = _model(budgets[25:], 4, lag, 16, 2)
    assert eng.replays == eng.graph.count == r1 + r2
    want = log1 + [(a + r1, b + r1, [h + 25 for h in g]) for a, b, g in log2]
    assert eng.admission_log == want
    if lag:
        assert any(b > a for a, b, _ in eng.admission_log)    # some prefill did run next to replays
    # two runs give identical logs
    eng2, _, _ = run()
    for b in budgets[25:]:
        eng2.submit(b)
    eng2.run()
    assert eng2.admission_log == eng.admission_log and eng2.events == eng.events and eng2.replays == eng.replays


def test_every_request_gets_exactly_its_budget_of_replays():
    budgets = [1, 7, 1, 12, 3, 30, 2, 2, 19, 1, 5]
    eng = HostOnlyEngine(3, 4, check_every=5)
    for b in budgets:
        eng.submit(b)
    committed = {}
    while not eng.sched.idle:
        eng.step()
    for _, at, g in eng.admission_log:
        committed.update({h: at for h in g})
    # a request of budget b is retired exactly b - 1 replays after its commit (its first id comes with the commit)
    assert {h: eng.retired_at[h] - committed[h] for h in committed} == {h: b - 1 for h, b in enumerate(budgets)}
    assert eng.replays == _model(budgets, 3, 4, 5, 2)[0]


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_bogus_admission_mode_names_all_three():
    with pytest.raises(ValueError) as e:
        ContinuousDecoder(None, admission="bogus")
    assert all(repr(mode) in str(e.value) for mode in ("eager", "graph", "overlap"))
    with pytest.raises(ValueError):
        ContinuousDecoder(None, admission="overlap", overlap_replays=-1)


def test_row_commit_is_exported_and_rejects_bad_arguments_without_launching(hip_lib):
    assert "rwkv7_cache_rows_commit_bf16" in _lib.exported_symbols()
    f = hip_lib.rwkv7_cache_rows_commit_bf16
    one = ctypes.c_void_p(16)   # never dereferenced: the checks fire first

    def call(layers=2, n=3, src=one, dst=one, sr=one, dr=one, D=128, H=2):
        return f(layers, n, src, dst, sr, dr, D, H, None)

    assert call(D=100, H=1) == -4                             # D % 8 != 0
    assert call(D=8200, H=128) == -4                          # wider than the row kernels
    assert call(D=128, H=3) == -3                             # D != 64 H
    assert call(D=72, H=1) == -3
    assert call(n=-1) == -1
    assert call(src=None) == -1 and call(dst=None) == -1
    assert call(sr=None) == -1 and call(dr=None) == -1        # index arrays are needed once n > 0
    assert call(layers=0) == -1 and call(n=70000) == -1 and call(H=0, D=0) == -1
    assert call(n=0, sr=None, dr=None) == 0                   # nothing to do: no launch either


def test_row_lists_are_checked_on_the_host():
    assert check_commit_rows([0, 1, 2], [3, -1, 0], 8, 4) == ([0, 1, 2], [3, -1, 0])
    assert check_commit_rows([0, 9], [2, -1], 8, 4) == ([0, 9], [2, -1])   # a skipped entry's source is not read
    for src, dst in (([0, 1], [1]), ([0, 8], [0, 1]), ([-1, 1], [0, 1]), ([0, 1], [4, 0]), ([0, 1], [2, 2])):
        with pytest.raises(ValueError):
            check_commit_rows(src, dst, 8, 4)
