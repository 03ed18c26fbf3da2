"""GPU (-m gpu): continuous batching for the Cosy model -- the per-slot repetition-aware draw (rwkv7_ras_slots_f32) against the
one-slot entry it must equal bit for bit (rwkv7_ras_step_f32), its end conditions and argument checks, and ContinuousCosyDecoder:
wiring of ring / counter / seed / embedding against the one-slot sampler on the step's own logits, slot and admission-time
invariance, the EOS bar with retirement and slot reuse, stream(), and the real head size at 0.4B widths."""
import ctypes
import math
import random

import pytest
import torch

from cosy_slots_ref import new_slot, slot_bookkeeping
from rwkvtts_amd.continuous_cosy import ContinuousCosyDecoder, RasSlotState, cosy_request, ras_slots
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7CosyLM
from rwkvtts_amd.sampling import ras_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIN = 10


# ---------------------------------------------------------------------------------------------------------------- 1. kernel
class _Slots:
    """S slots over a vocabulary of V ids (EOS = V - 1) with per-slot parameters P[s] and device state."""

    def __init__(self, V, P, D=64, LD=16, WLD=12, seed=0):
        self.V, self.eos, self.P, self.S, self.D, self.LD = V, V - 1, P, len(P), D, LD
        S = self.S
        g = self.g = torch.Generator().manual_seed(seed)
        l64 = dict(dtype=torch.int64, device=DEV)
        t = lambda key, dt: torch.tensor([p[key] for p in P], dtype=dt, device=DEV)
        self.step, self.limit, self.n_ignore = t("step", torch.int64), t("limit", torch.int64), t("n_ignore", torch.int64)
        self.seed = torch.tensor([p["seed"] - (1 << 64) if p["seed"] >= 1 << 63 else p["seed"] for p in P], **l64)
        self.top_k, self.top_p, self.tau_r = t("top_k", torch.int32), t("top_p", torch.float32), t("tau_r", torch.float32)
        self.live = t("live", torch.uint8)
        self.recent = torch.full((S, WLD), -1, **l64)
        self.ptr, self.n_out = torch.zeros(S, **l64), torch.zeros(S, **l64)
        self.ids = torch.full((S,), -9, **l64)
        self.seq = torch.full((S, LD), -7, **l64)
        self.emb = torch.randn(V, D, generator=g).to(DEV, torch.bfloat16)
        self.x = torch.randn(S, D, generator=g).to(DEV, torch.bfloat16)
        st = self.st = RasSlotState()
        st.step, st.limit, st.n_ignore, st.seed = (v.data_ptr() for v in (self.step, self.limit, self.n_ignore, self.seed))
        st.top_k, st.top_p, st.tau_r, st.live = (v.data_ptr() for v in (self.top_k, self.top_p, self.tau_r, self.live))
        st.recent, st.win_ld, st.ptr, st.ids = self.recent.data_ptr(), WLD, self.ptr.data_ptr(), self.ids.data_ptr()
        st.n_out, st.seq, st.seq_ld = self.n_out.data_ptr(), self.seq.data_ptr(), LD
        st.emb, st.x, st.D, st.slots, st.win_size, st.top_k_max, st.eos = self.emb.data_ptr(), self.x.data_ptr(), D, S, WIN, 128, self.eos
        self.host = [new_slot(p["limit"], WIN, step=p["step"], live=p["live"]) for p in P]   # the Python restatement, slot by slot

    def state(self):
        return dict(step=self.step, live=self.live, recent=self.recent, ptr=self.ptr, n_out=self.n_out, ids=self.ids, seq=self.seq, x=self.x)

    def snapshot(self):
        return {k: v.clone() for k, v in self.state().items()}

    def one_slot(self, logits_row, s, before, tau_r=None):
        """The ONE rwkv7_ras_step_f32 call the slot's draw must equal, on clones of the slot's ring, pointer and step."""
        p = self.P[s]
        tok = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        ring, ptr, step = before["recent"][s, :WIN].clone(), before["ptr"][s:s + 1].clone(), before["step"][s:s + 1].clone()
        ras_step(logits_row.contiguous(), tok, ring, ptr, step, p["n_ignore"], self.eos, top_p=p["top_p"], top_k=p["top_k"], win_size=WIN,
                 tau_r=p["tau_r"] if tau_r is None else tau_r, seed=p["seed"])
        return int(tok), ring, int(ptr), int(step)

    def check_slot(self, s, before, tok, ring, ptr, step, tag):
        """Device state of slot s after a call against the one-slot entry's results and the Python restatement."""
        h = slot_bookkeeping(self.host[s], tok, self.eos, WIN)
        assert int(self.ids[s]) == tok, (tag, int(self.ids[s]), tok)
        assert torch.equal(self.recent[s, :WIN], ring) and int(self.ptr[s]) == ptr and int(self.step[s]) == step, tag
        assert torch.equal(self.recent[s, WIN:], before["recent"][s, WIN:]), tag
        assert ring.tolist() == h["recent"] and ptr == h["ptr"] and step == h["step"], tag
        assert int(self.n_out[s]) == h["n_out"] and int(self.live[s]) == h["live"], tag
        n = h["n_out"]
        assert self.seq[s, :n].tolist() == h["seq"] and torch.equal(self.seq[s, n:], before["seq"][s, n:]), tag
        want_x = self.emb[tok] if tok != self.eos else before["x"][s]
        assert torch.equal(self.x[s].view(torch.int16), want_x.view(torch.int16)), tag


@pytest.mark.parametrize("V", [97, 1281, 6562, 8449])
def test_slot_draws_equal_the_one_slot_entry(V):
    """One size inside each EPT class and one just past each class boundary (1280, 8448).  Slot 0: top_k = 1 with its argmax in the
    ring, so the fallback draw is taken; slot 1: a nucleus that is EOS alone while EOS is ignored (the `alt` draw); slot 3: a heavy
    EOS across the n_ignore boundary, a key >= 2^63, the widest nucleus; slots 2 and 4 are not named by row_slot, slot 5 is idle."""
    eos = V - 1
    P = [dict(step=0, limit=1000, n_ignore=0, seed=11, top_k=1, top_p=0.8, tau_r=0.1, live=1),
         dict(step=3, limit=1000, n_ignore=100, seed=12, top_k=25, top_p=0.8, tau_r=0.5, live=1),
         dict(step=4, limit=1000, n_ignore=2, seed=13, top_k=25, top_p=1.0, tau_r=0.1, live=1),
         dict(step=2, limit=1000, n_ignore=5, seed=(1 << 63) + 14, top_k=128, top_p=1.0, tau_r=0.5, live=1),
         dict(step=1, limit=1000, n_ignore=0, seed=15, top_k=25, top_p=0.8, tau_r=0.1, live=1),
         dict(step=6, limit=1000, n_ignore=0, seed=16, top_k=128, top_p=0.8, tau_r=0.1, live=0)]
    z = _Slots(V, P, seed=V)
    rows = [3, 0, 9, 5, 1]                                                 # row r -> slot rows[r]; 9 is no slot
    row_slot = torch.tensor(rows, dtype=torch.int32, device=DEV)
    A0 = 5                                                                 # slot 0's argmax
    peak = math.log(1.65 * V) - 0.5                                        # well above every unit normal, about 0.4 of the row's mass
    fallback_calls, fallback_moved = 0, 0
    for call in range(12):                                                 # the ring of ten wraps
        lg = torch.randn(len(rows), V, generator=z.g)
        lg[1, A0], lg[1, eos] = peak, -30.0                                # slot 0
        lg[4, eos] = lg[4].max() + 20.0                                    # slot 1: P(EOS) = 1 - 1e-5 > top_p
        lg[0] *= 3.0
        lg[0, eos] = lg[0, :eos].max() - 1.0                               # slot 3
        logits = lg.to(DEV)
        before = z.snapshot()
        ras_slots(logits, z.st, row_slot)
        torch.cuda.synchronize()
        for r, s in enumerate(rows):
            if s >= z.S or not z.host[s]["live"]:
                continue
            tok, ring, ptr, step = z.one_slot(logits[r], s, before)
            if s == 0 and A0 in z.host[0]["recent"]:
                # the nucleus is the argmax alone and it is in the ring: the one-slot entry's id is its full-distribution draw
                assert tok == z.one_slot(logits[r], s, before, tau_r=0.0)[0]
                assert z.one_slot(logits[r], s, before, tau_r=2.0)[0] == A0
                fallback_calls += 1
                fallback_moved += tok != A0
            if s == 1:
                assert tok != eos and z.one_slot(logits[r], s, before, tau_r=2.0)[0] == tok
            z.check_slot(s, before, tok, ring, ptr, step, (V, call, s))
        for s in (2, 4, 5):                                                # unmapped and idle slots: byte for byte unchanged
            for k, v in z.state().items():
                assert torch.equal(v[s], before[k][s]), (call, s, k)
    assert z.host[1]["n_out"] == 12 and z.host[0]["n_out"] == 12          # both rings wrapped
    assert fallback_calls >= 8 and fallback_moved >= 1, (fallback_calls, fallback_moved)
    # the same draws without row_slot (row r is slot r) on a fresh copy of the state: ids depend on the slot's own fields only
    z2 = _Slots(V, P, seed=V)
    lg = torch.randn(6, V, generator=torch.Generator().manual_seed(1)).to(DEV)
    b1, b2 = z.snapshot(), z2.snapshot()
    z2.live.copy_(torch.tensor([1, 0, 0, 1, 0, 0], dtype=torch.uint8))
    z2.step.copy_(z.step), z2.recent.copy_(z.recent), z2.ptr.copy_(z.ptr)
    z.live.copy_(z2.live)
    ras_slots(lg, z2.st)
    ras_slots(lg[[3, 0]].contiguous(), z.st, torch.tensor([3, 0], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(z.ids[[0, 3]], z2.ids[[0, 3]]) and torch.equal(z.recent, z2.recent) and torch.equal(z.step, z2.step)
    assert torch.equal(z2.ids[[1, 2, 4, 5]], b2["ids"][[1, 2, 4, 5]]) and torch.equal(z.ids[[1, 2, 4, 5]], b1["ids"][[1, 2, 4, 5]])


def test_end_conditions():
    V = 97
    eos = V - 1
    P = [dict(step=4, limit=1000, n_ignore=0, seed=1, top_k=25, top_p=0.8, tau_r=0.1, live=1),    # draws EOS
         dict(step=7, limit=9, n_ignore=0, seed=2, top_k=25, top_p=0.8, tau_r=0.1, live=1),       # two draws left
         dict(step=0, limit=1000, n_ignore=0, seed=3, top_k=25, top_p=0.8, tau_r=0.1, live=1)]    # keeps running
    z = _Slots(V, P, seed=1)
    lives = []
    for call in range(3):
        lg = torch.randn(3, V, generator=z.g)
        lg[0, eos] = 40.0                                                  # the nucleus is EOS alone and EOS is allowed
        lg[1:, eos] = -40.0
        logits = lg.to(DEV)
        before = z.snapshot()
        ras_slots(logits, z.st)
        torch.cuda.synchronize()
        for s in range(3):
            if not z.host[s]["live"]:                                      # a dead slot stays untouched on later calls
                for k, v in z.state().items():
                    assert torch.equal(v[s], before[k][s]), (call, s, k)
                continue
            tok, ring, ptr, step = z.one_slot(logits[s], s, before)
            z.check_slot(s, before, tok, ring, ptr, step, (call, s))
            if s == 0:   # EOS ends the slot without appending to the ring, seq or x
                assert tok == eos and int(z.live[0]) == 0 and int(z.step[0]) == 5 and int(z.n_out[0]) == 0 and int(z.ptr[0]) == 0
                for k in ("recent", "seq", "x"):
                    assert torch.equal(z.state()[k][0], before[k][0]), k
        lives.append(z.live.tolist())
    assert lives == [[0, 1, 1], [0, 0, 1], [0, 0, 1]]                      # the limit ends slot 1 on the exact step
    assert int(z.step[1]) == 9 and int(z.n_out[1]) == 2 and int(z.step[2]) == 3


def test_argument_errors_do_not_launch(hip_lib):
    one = 16   # never dereferenced: the checks fire first
    p = ctypes.c_void_p
    per_slot = ("step", "limit", "n_ignore", "seed", "top_k", "top_p", "tau_r", "live", "recent", "ptr", "ids", "n_out", "seq")

    def state(**kw):
        st = RasSlotState()
        for f in per_slot + ("emb", "x"):
            setattr(st, f, one)
        st.win_ld, st.seq_ld, st.D, st.slots, st.win_size, st.top_k_max, st.eos = 10, 8, 128, 32, 10, 128, 96
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    call = lambda st, rows=1, V=97, logits=one: hip_lib.rwkv7_ras_slots_f32(rows, V, p(logits), ctypes.c_long(V), None,
                                                                            ctypes.byref(st) if st is not None else None, None)
    EINVAL, ESHAPE = -1, -4
    assert call(None) == EINVAL and call(state(), rows=0) == EINVAL and call(state(), logits=None) == EINVAL
    for f in per_slot:
        assert call(state(**{f: None})) == EINVAL, f
    assert call(state(slots=0)) == EINVAL and call(state(seq_ld=0)) == EINVAL and call(state(x=None)) == EINVAL
    assert call(state(), V=15361) == ESHAPE
    for bad in (dict(win_size=0), dict(win_size=129, win_ld=200), dict(win_size=11), dict(top_k_max=0), dict(top_k_max=129), dict(D=100)):
        assert call(state(**bad)) == ESHAPE, bad
    torch.cuda.synchronize()                                               # nothing was launched, so nothing can have faulted


# ---------------------------------------------------------------------------------------------------------------- 2. engine
def _model(L=2, seed=5, ST=96, vocab=300, **dims):
    d = dict(hidden_size=128, num_hidden_layers=L, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=32)
    d.update(dims)
    m = RWKV7CosyLM(RWKV7CosyConfig(vocab_size=vocab, speech_token_size=ST, **d)).init_weights(seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        m.lm_head.weight.copy_(torch.randn(m.lm_head.weight.shape, generator=g) * 0.05)
        m.lm_head.bias.copy_(torch.randn(m.lm_head.bias.shape, generator=g) * 0.1)
        for e in (m.llm_embedding, m.text_embedding, m.speech_embedding):
            e.weight.copy_(torch.randn(e.weight.shape, generator=g) * 0.5)
    return m.to(DEV).to(torch.bfloat16).eval()


def _requests(m, n, seed, lo=3, hi=40, vocab=300):
    """n utterances: (kwargs of the low-level submit) with prompts of lo..hi text ids and some prompt speech."""
    rng, g = random.Random(seed), torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        text = torch.randint(0, vocab, (rng.randint(lo, hi),), generator=g)
        speech = torch.randint(0, m.speech_token_size, (rng.randint(0, 12),), generator=g)
        out.append(cosy_request(m, text, None, speech).embeds)
    return out


SAMPLED = [dict(sampling=25, seed=11), dict(sampling=1, seed=12, tau_r=0.5), dict(sampling=128, top_p=1.0, seed=13),
           dict(sampling=25, top_p=0.5, seed=(1 << 63) + 14)]
BOUNDS = [dict(min_len=9, max_len=30, original_text_len=5), dict(min_len=0, max_len=50, original_text_len=0),
          dict(min_len=40, max_len=33, original_text_len=0), dict(min_len=12, max_len=64, original_text_len=2)]


def test_engine_draws_equal_the_one_slot_sampler_on_the_step_logits():
    """After every replay: the id each live slot drew is rwkv7_ras_step_f32 on that row of the step's logits buffer, with ring, step,
    n_ignore and seed from this test's own tracking of the request; x[s] is the speech embedding of that id.  The admission draw is
    checked the same way on the logits the engine hands to it.  No prefill path is compared with another."""
    m = _model()
    eos = m.speech_token_size
    eng = ContinuousCosyDecoder(m, slots=3, max_len_cap=64, check_every=1)
    embeds = _requests(m, 5, 7)
    kws = [dict(SAMPLED[i % 4], **BOUNDS[i % 4]) for i in range(5)]
    kws[4].update(seed=99, max_len=12)
    handles = [eng.submit(inputs_embeds=e, **kw) for e, kw in zip(embeds, kws)]
    par = {h: dict(n_ignore=kw["min_len"] - kw["original_text_len"], top_k=kw["sampling"], top_p=kw.get("top_p", 0.8),
                   tau_r=kw.get("tau_r", 0.1), seed=kw["seed"]) for h, kw in zip(handles, kws)}
    host, slot_of = {}, {}                                                 # handle -> restated slot; slot -> handle

    def one_slot(row, h):
        s, p = host[h], par[h]
        tok = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        ring = torch.tensor(s["recent"], dtype=torch.int64, device=DEV)
        ptr, step = torch.tensor([s["ptr"]], device=DEV), torch.tensor([s["step"]], device=DEV)
        ras_step(row.contiguous(), tok, ring, ptr, step, p["n_ignore"], eos, top_p=p["top_p"], top_k=p["top_k"], win_size=WIN,
                 tau_r=p["tau_r"], seed=p["seed"])
        return int(tok)

    def check(slot, h, row, tag):
        tok = one_slot(row, h)
        s = slot_bookkeeping(host[h], tok, eos, WIN)
        assert int(eng.ids[slot]) == tok, (tag, slot, h, int(eng.ids[slot]), tok)
        assert eng.recent[slot].tolist() == s["recent"] and int(eng.ptr[slot]) == s["ptr"] and int(eng.step_t[slot]) == s["step"], tag
        assert int(eng.n_out[slot]) == s["n_out"] and int(eng.live[slot]) == s["live"], tag
        assert eng.seq[slot, :s["n_out"]].tolist() == s["seq"], tag
        if tok != eos:
            assert torch.equal(eng.x[slot].view(torch.int16), m.speech_embedding.weight[tok].view(torch.int16)), tag

    inner = eng._admit_draw

    def admit_draw(took, logits, rows64, row_slot):
        logits = logits.contiguous()
        inner(took, logits, rows64, row_slot)
        torch.cuda.synchronize()
        for r, (slot, req) in enumerate(took):
            host[req.handle] = new_slot(req.max_new_tokens, WIN)
            slot_of[slot] = req.handle
            check(slot, req.handle, logits[r], ("admission", req.handle))
    eng._admit_draw = admit_draw

    got, draws = {}, 0
    while not eng.sched.idle:
        ran = eng.replays
        done = eng.step()
        if eng.replays != ran:                                             # one replay: every slot that was live drew on its row
            assert eng.replays == ran + 1
            for slot, h in sorted(slot_of.items()):
                if host[h]["live"]:
                    check(slot, h, eng.dstep.logits[slot], ("replay", eng.replays, slot, h))
                    draws += 1
        for h, ids in done:
            assert h not in got and not host[h]["live"]
            got[h] = ids
            assert ids.tolist() == host[h]["seq"] and eos not in ids.tolist() and ids.dtype == torch.int64
            del slot_of[next(s for s, hh in slot_of.items() if hh == h)]
        assert all(host[h]["live"] for h in slot_of.values())             # whatever ended was retired at this read-back
    assert sorted(got) == sorted(handles) and draws > 40
    assert len(got[handles[2]]) == 33                                      # EOS barred up to its limit: it ran to max_len


@pytest.mark.parametrize("admission", ["eager", "graph"])
def test_ids_do_not_depend_on_slot_or_admission_time(admission):
    """Graph admission: for the same pack composition (the four requests are admitted together, in order, in both engines)."""
    m = _model()
    embeds = _requests(m, 4, 5)
    kws = [dict(SAMPLED[i], **BOUNDS[i]) for i in range(4)]
    ekw = dict(slots=8, max_len_cap=128, admission=admission, prefill_buckets=(256, 512))
    a = ContinuousCosyDecoder(m, **ekw)
    ha = [a.submit(inputs_embeds=e, **kw) for e, kw in zip(embeds, kws)]
    ra = a.run()
    b = ContinuousCosyDecoder(m, **ekw)
    # four requests that cannot end before their limit (EOS is barred throughout) hold slots 0..3 and run 16 steps
    busy = [b.submit(inputs_embeds=e, min_len=100, max_len=100, original_text_len=0, seed=i) for i, e in enumerate(_requests(m, 4, 9))]
    out = dict(b.step())
    assert not out and sorted(b.sched.busy) == [0, 1, 2, 3] and b.replays == 16
    hb = [b.submit(inputs_embeds=e, **kw) for e, kw in zip(embeds, kws)]
    b._admit()
    assert sorted(b.sched.busy) == list(range(8))                         # admitted together, into slots 4..7, 16 steps later
    out.update(b.run())
    assert sorted(out) == sorted(busy + hb)
    for h in busy:
        assert out[h].numel() == 100
    for x, y, kw in zip(ha, hb, kws):
        assert ra[x].dtype == torch.int64 and 0 <= ra[x].numel() <= kw["max_len"]
        assert torch.equal(ra[x], out[y]), (kw, ra[x], out[y])
        assert ((ra[x] >= 0) & (ra[x] < m.speech_token_size)).all()
    assert ra[ha[2]].numel() == 33                                         # EOS barred up to its limit: it ran to max_len


def test_min_len_bars_eos_then_eos_retires_and_the_slot_is_reused():
    """lm_head.bias[eos] = +30: P(EOS) differs from 1 by < 1e-9, so every nucleus is EOS alone.  While step < n_ignore the draw comes
    from the rest of the distribution; on step n_ignore it is EOS.  Nothing here is statistical."""
    m = _model()
    eos = m.speech_token_size
    with torch.no_grad():
        m.lm_head.bias[eos] = 30.0
    eng = ContinuousCosyDecoder(m, slots=2, max_len_cap=64, check_every=4)
    n_ignore = [3, 0, 7, 17, 5]
    hs = [eng.submit(inputs_embeds=e, min_len=n + 2, max_len=40, original_text_len=2, seed=50 + i)
          for i, (e, n) in enumerate(zip(_requests(m, 5, 3), n_ignore))]
    got = {}
    while not eng.sched.idle:
        for h, ids in eng.step():
            assert h not in got                                            # every handle is returned once
            got[h] = ids
    assert sorted(got) == sorted(hs)
    for h, n in zip(hs, n_ignore):
        assert got[h].numel() == n and eos not in got[h].tolist(), (h, n, got[h])   # n ids, then EOS on the next step
    # 2 slots, check_every = 4: the slots were reused, and no slot ran on to its limit of 40
    assert eng.replays < 40 and not eng.sched.busy and eng.sched.free == [0, 1]


def test_stream_pieces_concatenate_to_the_results_of_run():
    m = _model()
    embeds = _requests(m, 5, 17)
    kws = [dict(SAMPLED[i % 4], **BOUNDS[i % 4]) for i in range(5)]
    kws[4].update(seed=77)
    ekw = dict(slots=2, max_len_cap=64, check_every=4)
    a = ContinuousCosyDecoder(m, **ekw)
    ha = [a.submit(inputs_embeds=e, **kw) for e, kw in zip(embeds, kws)]
    want = a.run()
    b = ContinuousCosyDecoder(m, **ekw)
    hb = [b.submit(inputs_embeds=e, **kw) for e, kw in zip(embeds, kws)]
    pieces, finished = {h: [] for h in hb}, []
    for h, new, fin in b.stream():
        assert h not in finished and new.dtype == torch.int64 and new.dim() == 1 and new.numel() <= 4 + 1
        pieces[h].append(new)
        if fin:
            finished.append(h)
    assert sorted(finished) == sorted(hb) and b.sched.idle
    for x, y in zip(ha, hb):
        assert torch.equal(torch.cat(pieces[y]), want[x]), (x, pieces[y], want[x])
    assert sum(len(p) for p in pieces.values()) > len(hb)                  # ids came in more than one piece per request


def test_real_head_size_every_handle_once():
    """The default head (speech_token_size + 1 = 6562 ids) at 0.4B widths and a depth of 2 layers: the draw does not depend on the
    depth.  32 slots, 40 short utterances."""
    cfg = RWKV7CosyConfig(vocab_size=1000, hidden_size=1024, num_hidden_layers=2)
    assert cfg.speech_token_size + 1 == 6562
    m = _model(ST=cfg.speech_token_size, vocab=1000, hidden_size=1024, decay_low_rank_dim=cfg.decay_low_rank_dim,
               a_low_rank_dim=cfg.a_low_rank_dim, v_low_rank_dim=cfg.v_low_rank_dim, gate_low_rank_dim=cfg.gate_low_rank_dim)
    eng = ContinuousCosyDecoder(m, slots=32, max_len_cap=64)
    rng, g = random.Random(7), torch.Generator().manual_seed(7)
    want, got = {}, {}
    for i in range(40):
        n = rng.randint(2, 12)
        text = torch.randint(0, 1000, (n,), generator=g)
        speech = torch.randint(0, 6561, (rng.randint(0, 20),), generator=g)
        want[eng.submit(text=text, prompt_speech_token=speech, sampling=rng.choice([1, 25, 128]), max_token_text_ratio=5, seed=i)] = 5 * n
        if i % 16 == 15:
            for h, ids in eng.step():
                assert h not in got
                got[h] = ids
    for h, ids in eng.run().items():
        assert h not in got
        got[h] = ids
    assert sorted(got) == sorted(want)
    for h, n in want.items():
        ids = got[h]
        assert ids.dim() == 1 and ids.dtype == torch.int64 and ids.numel() <= n and ((ids >= 0) & (ids < 6561)).all()
    assert sum(ids.numel() for ids in got.values()) > 40
