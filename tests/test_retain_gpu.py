"""GPU (-m gpu): retaining a finished request's state -- rwkv7_cache_rows_retain_bf16 alone (which slots it copies, bit for bit, that
it copies them once and leaves everything else alone), and ContinuousDecoder(state_store=..., retain=True) in eager and graph
admission: the row published for a request that ends on an EOS, on its budget or with its first id equals the slot's row at the
moment the request ended, later steps do not touch it, a second turn from it draws the ids of a turn from that row, and the switch
changes no id, step count or log-probability.  Every comparison is bit-exact."""
import pytest
import torch

from rwkvtts_amd.backbone import Cache, LayerState
from rwkvtts_amd.continuous import ContinuousDecoder
from rwkvtts_amd.prefill import cache_field_table, cache_rows_retain, check_retain_rows
from rwkvtts_amd.state_store import StateStore

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------- 1. kernel
def _pattern_cache(L, S, D, H, seed):
    """A cache whose fields hold random BITS (so NaN and Inf patterns of every kind occur), with quiet / signalling NaNs, infinities
    and negative zero planted at the head of every row."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    bf = torch.tensor([0x7FC0, 0x7F81, 0xFFFF, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x7FFF], dtype=torch.int32).to(torch.int16).to(DEV)
    f32 = torch.tensor([0x7FC00000, 0x7F800001, -1, 0x7F800000, -0x800000, -0x80000000, 1, 0x7FFFFFFF], dtype=torch.int64).to(torch.int32).to(DEV)
    states = []
    for _ in range(L):
        xs = [torch.randint(-32768, 32768, (S, D), generator=g, device=DEV, dtype=torch.int32).to(torch.int16) for _ in range(2)]
        kv = torch.randint(-2 ** 31, 2 ** 31, (S, H, 64, 64), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
        for x in xs:
            x[:, :8] = bf
        kv[:, :, 0, :8] = f32
        states.append(LayerState(xs[0].view(torch.bfloat16), kv.view(torch.float32), xs[1].view(torch.bfloat16)))
    return Cache(states)


def _bits(c):
    return [t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) for s in c.states for t in (s.att_x_prev, s.att_kv, s.ffn_x_prev)]


def _snap(c):
    return [t.clone() for t in _bits(c)]


def _flags(live, armed, rows):
    u8, i32 = dict(dtype=torch.uint8, device=DEV), dict(dtype=torch.int32, device=DEV)
    return torch.tensor(live, **u8), torch.tensor(armed, **u8), torch.tensor(rows, **i32), torch.zeros(len(live), **i32)


@pytest.mark.parametrize("spare", ["armed and live", "unarmed and dead"])   # which of the two holds the third row
@pytest.mark.parametrize("L,D,H", [(2, 64, 1), (2, 128, 2), (1, 4096, 64)])
def test_retain_copies_the_armed_dead_slots_once_and_nothing_else(L, D, H, spare):
    S, R = 5, 3
    src, dst = _pattern_cache(L, S, D, H, 1), _pattern_cache(L, R, D, H, 2)
    src0, dst0 = _snap(src), _snap(dst)
    # slot:   0 armed, live | 1 armed, dead -> row 2 | 2 unarmed, dead | 3 armed, dead, no row | 4 armed, dead -> row 0
    live = [1, 0, 0, 0, 0]
    armed = [1, 7, 0, 1, 255]
    rows = [1 if spare == "armed and live" else -1, 2, 1 if spare == "unarmed and dead" else -1, -1, 0]
    copies = {1: 2, 4: 0}
    check_retain_rows(rows, R)
    live_t, armed_t, rows_t, ticket = _flags(live, armed, rows)
    tabs = cache_field_table(src), cache_field_table(dst)
    cache_rows_retain(*tabs, live_t, armed_t, rows_t, ticket, L, D, H)
    want_armed = [0 if s in copies else a for s, a in enumerate(armed)]

    def check():
        for got, d0, s0 in zip(_bits(dst), dst0, src0):
            for s, r in copies.items():
                assert torch.equal(got[r], s0[s])             # integer views, so NaNs compare
            assert torch.equal(got[1], d0[1])                 # the row of the slot that is not copied keeps every bit
        assert armed_t.tolist() == want_armed                 # cleared exactly for the copied slots
        assert not ticket.any()
        assert live_t.tolist() == live and rows_t.tolist() == rows

    check()
    for s, s0 in zip(_bits(src), src0):
        assert torch.equal(s, s0)                             # the source is only read
    # scramble the source and launch again: the slots are disarmed, so nothing changes -- the copy happened once
    again = _pattern_cache(L, S, D, H, 3)
    for s, a in zip(_bits(src), _bits(again)):
        s.copy_(a)
    cache_rows_retain(*tabs, live_t, armed_t, rows_t, ticket, L, D, H)
    check()


def test_retain_with_nothing_to_copy_touches_only_flags_at_128_slots():
    L, D, H, S, R = 2, 64, 1, 128, 4
    src, dst = _pattern_cache(L, S, D, H, 4), _pattern_cache(L, R, D, H, 5)
    src0, dst0 = _snap(src), _snap(dst)
    # every reason not to copy, over all 128 slots: live, unarmed, no row; only rows 0 .. 3 exist, held by live or unarmed slots
    live = [1 if s % 3 == 0 else 0 for s in range(S)]
    armed = [1 if s % 3 != 1 else 0 for s in range(S)]
    rows = [-1] * S
    rows[0], rows[127], rows[3], rows[126] = 0, 1, 2, 3     # 0, 126, 3: live; 127: 127 % 3 == 1, unarmed
    assert all(live[s] or not armed[s] for s in (0, 127, 3, 126))
    assert any(armed[s] and not live[s] for s in range(S))   # armed and dead slots there are: they have no row
    live_t, armed_t, rows_t, ticket = _flags(live, armed, check_retain_rows(rows, R))
    cache_rows_retain(cache_field_table(src), cache_field_table(dst), live_t, armed_t, rows_t, ticket, L, D, H)
    for got, want in list(zip(_bits(dst), dst0)) + list(zip(_bits(src), src0)):
        assert torch.equal(got, want)
    assert armed_t.tolist() == armed and live_t.tolist() == live and rows_t.tolist() == rows and not ticket.any()


def test_retain_wrapper_raises_for_a_geometry_without_a_kernel():
    c = _pattern_cache(1, 2, 64, 1, 6)
    live_t, armed_t, rows_t, ticket = _flags([0, 0], [0, 0], [-1, -1])
    tab = cache_field_table(c)
    with pytest.raises(ValueError, match="RWKV7_EHEAD"):
        cache_rows_retain(tab, tab, live_t, armed_t, rows_t, ticket, 1, 64, 2)
    with pytest.raises(ValueError, match="RWKV7_ESHAPE"):
        cache_rows_retain(tab, tab, live_t, armed_t, rows_t, ticket, 1, 8200, 128)


# ---------------------------------------------------------------------------------------------------------------- 2.. engine
def _model(L=2, V=300, seed=0, **dims):
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
    d = dict(hidden_size=128, num_hidden_layers=L, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=64)
    d.update(dims)
    cfg = RWKV7SpeechConfig(vocab_size=V, text_vocab_size=300, audio_global_vocab_size=64, **d)
    m = RWKV7ForSpeech(cfg).init_weights(seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        m.lm_head.weight.copy_(torch.randn(m.lm_head.weight.shape, generator=g) * 0.05)
        m.model.embeddings.weight.copy_(torch.randn(m.model.embeddings.weight.shape, generator=g) * 0.5)
    return m.to(DEV).to(torch.bfloat16).eval()


@pytest.fixture(scope="module")
def model():
    return _model()


SMALL = dict(slots=4, max_new_tokens_cap=64, prefill_buckets=(64, 128, 256))
ADMISSIONS = ["eager", "graph"]


def _engine(m, admission, **kw):
    return ContinuousDecoder(m, admission=admission, **{**SMALL, **kw})


def _ids(n, seed):
    return torch.randint(0, 300, (n,), generator=torch.Generator().manual_seed(seed))


def _clone(cache):
    return Cache([LayerState(s.att_x_prev.clone(), s.att_kv.clone(), s.ffn_x_prev.clone()) for s in cache.states])


def _row_equal(a, ra, b, rb):
    for x, y in zip(_bits(a), _bits(b)):
        assert torch.equal(x[ra], y[rb])


def _until(eng, h):
    """step() until handle h has been returned: everything returned so far."""
    got = {}
    while h not in got:
        assert not eng.sched.idle
        got.update(dict(eng.step()))
    return got


def _composition(filler, budget=40):
    """(requests, index of the target): the target, then two neighbours that run `budget` ids whatever they draw; behind a filler that
    ends with its first id when the target is to sit in slot 1 rather than slot 0."""
    reqs = [dict(input_ids=_ids(5, 300), max_new_tokens=1)] if filler else []
    t = len(reqs)
    reqs.append(dict(input_ids=_ids(23, 301), max_new_tokens=12))
    reqs += [dict(input_ids=_ids(9 + 30 * i, 302 + i), max_new_tokens=budget, min_new_tokens=budget, do_sample=True, top_k=50, seed=11 + i)
             for i in range(2)]
    return reqs, t


def _submit_all(eng, reqs, t=None, retain=None):
    return [eng.submit(**kw, **({"retain": retain} if i == t else {})) for i, kw in enumerate(reqs)]


def _retaining(m, admission, **kw):
    """(engine with retain=True, its store): three rows, row 0 held by a name that is never written."""
    store = StateStore(m, 3)
    store.reserve("held")
    return _engine(m, admission, state_store=store, retain=True, **kw), store


def _at_rest(eng, store, slot):
    assert int(eng.armed[slot]) == 0 and int(eng.retain_row[slot]) == -1 and not eng.ticket.any() and store.pending() == []
    assert not any(t[0].any() for t in _bits(store.cache))    # the held row was never written


@pytest.mark.parametrize("filler", [False, True])
@pytest.mark.parametrize("admission", ADMISSIONS)
def test_a_request_that_ends_on_eos_leaves_the_row_it_ended_with(model, admission, filler):
    reqs, t = _composition(filler)
    # the EOS: an id the greedy target first emits at position 2 .. 10, found by a run of the same composition without an EOS
    free = _engine(model, admission)
    hf = _submit_all(free, reqs)
    ids = free.run()[hf[t]].tolist()
    k = next((k for k in range(2, 11) if ids[k] not in ids[:k]), None)
    assert k is not None, ids
    E = ids[k]
    # reference: no retain, and the host looks after every replay, so the slot's row is still the one the request ended with
    ref = _engine(model, admission, eos_token_id=E, check_every=1)
    hr = _submit_all(ref, reqs)
    assert _until(ref, hr[t])[hr[t]].tolist() == ids[:k + 1] and ref.replays == k
    want = _clone(ref.cache)
    # under test: the host looks every 16 replays; by then the dead slot's row has been run through stale inputs
    eng, store = _retaining(model, admission, eos_token_id=E, check_every=16)
    he = _submit_all(eng, reqs, t, "turn1")
    assert store.pending() == ["turn1"] and "turn1" not in store
    got = _until(eng, he[t])
    assert got[he[t]].tolist() == ids[:k + 1] and eng.replays == 16 and len(eng.sched.busy) == 2
    assert store.names() == ["held", "turn1"] and store.row("turn1") == 1 and store.tokens[1] == 23 + k
    _row_equal(store.cache, 1, want, t)
    assert any(not torch.equal(x[t], y[t]) for x, y in zip(_bits(eng.cache), _bits(want)))   # the slot's own row has moved on
    _at_rest(eng, store, t)
    eng.run()                                                 # the neighbours finish: later steps do not touch the stored row
    assert eng.replays >= 39
    _row_equal(store.cache, 1, want, t)
    _at_rest(eng, store, t)


class _Budget:
    """A target that ends on its budget of 6 ids next to two running neighbours, no EOS: the reference row (a retain-less engine
    stops on the exact step), and the engine under test after everything has finished.  Computed once per admission mode."""

    def __init__(self, m, admission):
        reqs, t = _composition(False)
        reqs[t]["max_new_tokens"] = 6
        ref = _engine(m, admission, check_every=1)
        hr = _submit_all(ref, reqs)
        self.ids = _until(ref, hr[t])[hr[t]]
        assert ref.replays == 5 and len(ref.sched.busy) == 2
        self.want, self.slot = _clone(ref.cache), t
        self.eng, self.store = _retaining(m, admission, check_every=16)
        he = _submit_all(self.eng, reqs, t, "turn1")
        self.got = _until(self.eng, he[t])[he[t]]
        self.busy_then = len(self.eng.sched.busy)
        self.first = [t.clone() for t in _bits(self.store.cache)]
        self.eng.run()


_budget_cases = {}


@pytest.fixture
def budget(model, request):
    a = request.param
    if a not in _budget_cases:
        _budget_cases[a] = _Budget(model, a)
    return a, _budget_cases[a]


@pytest.mark.parametrize("budget", ADMISSIONS, indirect=True)
def test_a_request_that_ends_on_its_budget_leaves_the_row_it_ended_with(budget):
    _, b = budget
    assert torch.equal(b.got, b.ids) and b.got.numel() == 6 and b.busy_then == 2
    assert b.store.row("turn1") == 1 and b.store.tokens[1] == 23 + 5
    for x, y in zip(b.first, _bits(b.want)):
        assert torch.equal(x[1], y[b.slot])                   # when the handle came back
    _row_equal(b.store.cache, 1, b.want, b.slot)              # and after the neighbours have finished
    _at_rest(b.eng, b.store, b.slot)


@pytest.mark.parametrize("budget", ADMISSIONS, indirect=True)
def test_turn_two_from_the_retained_state_draws_what_the_reference_row_gives(model, budget):
    admission, b = budget
    turn2 = dict(input_ids=torch.cat([b.got[-1:].cpu(), _ids(8, 310)]), max_new_tokens=12, do_sample=True, top_k=50, top_p=0.9, seed=77)
    assert b.eng.sched.idle
    h = b.eng.submit(state="turn1", **turn2)
    got = b.eng.run()[h]
    other = StateStore(model, 2)
    other.reserve("first")
    assert other.put("ref", b.want, row=b.slot, tokens=28) == 1
    ref = _engine(model, admission, state_store=other)
    hr = ref.submit(state="ref", **turn2)
    assert torch.equal(got, ref.run()[hr]) and got.numel() == 12
    _row_equal(b.store.cache, 1, b.want, b.slot)              # serving from the row only reads it


@pytest.mark.parametrize("admission", ADMISSIONS)
def test_a_request_that_ends_with_its_first_id_leaves_the_state_after_its_prompt(model, admission):
    prompt = _ids(37, 320)
    plain = _engine(model, admission)
    hp = plain.submit(input_ids=prompt, max_new_tokens=1)
    (done,) = plain.step()
    assert done[0] == hp and plain.replays == 0
    eng, store = _retaining(model, admission)
    h = eng.submit(input_ids=prompt, max_new_tokens=1, retain="p")
    (got,) = eng.step()
    assert got[0] == h and eng.replays == 0 and torch.equal(got[1], done[1])
    assert store.row("p") == 1 and store.tokens[1] == 37
    _row_equal(store.cache, 1, plain.cache, 0)
    _at_rest(eng, store, 0)
    if admission == "eager":   # eager admission of one prompt is the call capture() makes
        assert store.capture("c", input_ids=prompt) == 2
        _row_equal(store.cache, 1, store.cache, 2)


def _workload():
    reqs = []
    for i in range(6):
        kw = dict(input_ids=_ids(5 + 13 * i, 330 + i), max_new_tokens=(9, 30, 1, 17, 25, 12)[i])
        if i % 2:
            kw.update(do_sample=True, seed=900 + i, top_k=(0, 5, 50)[i % 3], top_p=1.0 if i % 3 == 0 else 0.9, temperature=(0.8, 1.0, 1.3)[i % 3])
        reqs.append(kw)
    return reqs


@pytest.mark.parametrize("admission", ADMISSIONS)
def test_the_switch_changes_no_id_step_count_or_logprob(model, admission):
    reqs, out = _workload(), []
    for retain, name_on in ((False, None), (True, None), (True, 3)):
        store = StateStore(model, 2)
        eng = _engine(model, admission, state_store=store, retain=retain, logprobs=True, check_every=4)
        hs = _submit_all(eng, reqs, name_on, "kept")
        got = eng.run()
        out.append(([got[h] for h in hs], [eng.take_logprobs(h) for h in hs], eng.replays))
        assert store.names() == (["kept"] if name_on is not None else [])
    for ids, lps, replays in out[1:]:
        assert replays == out[0][2]
        for a, b in zip(ids, out[0][0]):
            assert torch.equal(a, b)
        for (tok, cum), (tok0, cum0) in zip(lps, out[0][1]):
            assert torch.equal(tok, tok0) and torch.equal(cum, cum0)


@pytest.mark.parametrize("admission", ADMISSIONS)
def test_state_and_retain_in_one_request(model, admission):
    eng, store = _retaining(model, admission)
    assert store.capture("v", input_ids=_ids(20, 340)) == 1
    before = [t[1].clone() for t in _bits(store.cache)]
    h = eng.submit(state="v", input_ids=_ids(7, 341), max_new_tokens=5, retain="t")
    assert store.pinned("v") == 1 and store.pending() == ["t"]
    got = eng.run()[h]
    assert got.numel() == 5 and store.pinned("v") == 0
    assert store.row("t") == 2 and store.tokens[2] == 20 + 7 + 5 - 1
    for x, y in zip(_bits(store.cache), before):
        assert torch.equal(x[1], y)                           # the source row keeps every bit
    assert any(not torch.equal(x[2], y) for x, y in zip(_bits(store.cache), before))
    _at_rest(eng, store, 0)
