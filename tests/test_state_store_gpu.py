"""GPU (-m gpu): serving from stored states -- rwkv7_cache_rows_seed_bf16 bit for bit against index_copy_ / index_fill_ (and the
commit entry, which shares its kernel body, still against index_copy_ alone), and ContinuousDecoder(state_store=...) in its three
admission modes: the state a seeded admission leaves equals the model's own forward over prefix then suffix, seeded requests do not
disturb their neighbours, do not depend on slot or time, fan out under submit_n, and come back from put / save / load unchanged."""
import random

import pytest
import torch

from rwkvtts_amd import backbone
from rwkvtts_amd.backbone import Cache, LayerState
from rwkvtts_amd.continuous import ContinuousDecoder, candidate_seed
from rwkvtts_amd.prefill import (SEED_ZERO, PackedPrefill, cache_field_table, cache_rows_commit, cache_rows_seed, check_commit_rows,
                                 check_seed_rows)
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


def _entries(S):
    """(src_row, dst_row) lists that mix copy, zero (src -1), a skipped destination (dst -1) and a skipped source (src -2): the
    last row is copied, row 0 zeroed, the order is not monotonic, a source row repeats."""
    rng = random.Random(S)
    mid = rng.sample(range(1, S - 1), min(4, S - 2))
    ent = [(5, S - 1), (-2, mid[0]), (SEED_ZERO, 0), (3, -1)]   # copy, skipped source (a valid destination stays), zero, skipped destination
    if len(mid) == 4:
        ent += [(5, mid[1]), (SEED_ZERO, mid[2]), (-7, -1), (0, mid[3])]
    return [s for s, _ in ent], [d for _, d in ent]


@pytest.mark.parametrize("S", [3, 32, 128])
@pytest.mark.parametrize("D,H", [(64, 1), (192, 3), (1024, 16)])
@pytest.mark.parametrize("L", [1, 3])
def test_row_seed_equals_index_copy_and_index_fill_bit_for_bit(L, D, H, S):
    src, dst = _pattern_cache(L, 8, D, H, 1), _pattern_cache(L, S, D, H, 2)
    src0 = [t.clone() for t in _bits(src)]
    before = [t.clone() for t in _bits(dst)]
    src_row, dst_row = _entries(S)
    assert S - 1 in dst_row and 0 in dst_row and -1 in dst_row and -2 in src_row and SEED_ZERO in src_row
    copies = [(s, d) for s, d in zip(src_row, dst_row) if s >= 0 and d >= 0]
    zeros = [d for s, d in zip(src_row, dst_row) if s == SEED_ZERO and d >= 0]
    kept = [r for r in range(S) if r not in {d for _, d in copies} | set(zeros)]
    assert any(d >= 0 and s < -1 for s, d in zip(src_row, dst_row)) and set(kept) >= {d for s, d in zip(src_row, dst_row) if s < -1 and d >= 0}
    i32 = dict(dtype=torch.int32, device=DEV)
    si, di = (torch.tensor(v, device=DEV) for v in zip(*copies))
    zi, ki = torch.tensor(zeros, device=DEV), torch.tensor(kept, dtype=torch.int64, device=DEV)

    # the seed entry
    check_seed_rows(src_row, dst_row, 8, S)
    cache_rows_seed(cache_field_table(src), cache_field_table(dst), torch.tensor(src_row, **i32), torch.tensor(dst_row, **i32),
                    len(src_row), L, D, H)
    for got, b, s in zip(_bits(dst), before, src0):
        want = b.clone()
        want.index_copy_(0, di, s[si])
        want.index_fill_(0, zi, 0)
        assert torch.equal(got, want)                         # integer views, so NaNs compare
        assert torch.equal(got[ki], b[ki])                    # rows not named, and the entries skipped either way: unchanged
        assert not got[zi].any()
    for s, s0 in zip(_bits(src), src0):
        assert torch.equal(s, s0)                             # the source is only read

    # the commit entry on the same inputs, on a fresh copy of the destination: a negative source of either kind skips
    dst2 = _pattern_cache(L, S, D, H, 2)
    cache_rows_commit(cache_field_table(src), cache_field_table(dst2), torch.tensor(src_row, **i32), torch.tensor(dst_row, **i32),
                      len(src_row), L, D, H)
    for got, b, s in zip(_bits(dst2), before, src0):
        want = b.clone()
        want.index_copy_(0, di, s[si])
        assert torch.equal(got, want)
        assert torch.equal(got[zi], b[zi])                    # -1 is no zero mark there


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


def _embeds(n, D, seed):
    return (torch.randn(n, D, generator=torch.Generator().manual_seed(seed)) * 0.5).to(DEV, torch.bfloat16)


SMALL = dict(slots=4, max_new_tokens_cap=64, prefill_buckets=(64, 128, 256))
TP = 50   # tokens of the stored prefix


class _Ctx:
    """The small model, a prefix P, a store that captured it as "v", and the test's own state after P: a 1-row Cache filled by the
    same public model call.  Computed once and left unchanged."""

    def __init__(self):
        self.m = m = _model()
        self.D = D = m.config.hidden_size
        self.P = _embeds(TP, D, 100)
        self.store = StateStore(m, 3)
        self.row = self.store.capture("v", inputs_embeds=self.P)
        self.after_p = Cache.zeros(m.config, 1, DEV, torch.bfloat16)
        self.forward(self.after_p, self.P)

    def forward(self, cache, e, row=0):
        with torch.no_grad():
            return self.m.model(inputs_embeds=e.unsqueeze(0), cu_seqlens=torch.tensor([0, e.shape[0]], dtype=torch.int32),
                                past_key_values=cache, cache_rows=torch.tensor([row])).last_hidden_state[0]

    def engine(self, admission="eager", store="own", **kw):
        return ContinuousDecoder(self.m, admission=admission, state_store=self.store if store == "own" else store, **{**SMALL, **kw})


@pytest.fixture(scope="module")
def ctx():
    return _Ctx()


def _row_equal(a: Cache, ra: int, b: Cache, rb: int):
    for x, y in zip(_bits(a), _bits(b)):
        assert torch.equal(x[ra], y[rb])


def _sampled(i, **kw):
    return dict(do_sample=True, seed=900 + i, top_k=(0, 5, 50)[i % 3], top_p=1.0 if i % 3 == 0 else 0.9, temperature=(0.8, 1.0, 1.3)[i % 3], **kw)


def test_capture_leaves_the_models_own_state_and_bookkeeping(ctx):
    st = ctx.store
    assert ctx.row == 0 and st.names() == ["v"] and st.tokens[0] == TP and st.pinned("v") == 0
    _row_equal(st.cache, 0, ctx.after_p, 0)
    for r in (1, 2):
        assert not any(t[r].any() for t in _bits(st.cache))   # the other rows were never written


def test_seeded_admission_state_eager(ctx):
    S = _embeds(21, ctx.D, 101)
    eng = ctx.engine("eager")
    h = eng.submit(state="v", inputs_embeds=S, max_new_tokens=1)
    assert eng.sched.pending[0].state_row == 0 and ctx.store.pinned("v") == 1
    done = eng.step()                                         # admission retires it: no replay touches the rows
    assert [x for x, _ in done] == [h] and eng.replays == 0 and ctx.store.pinned("v") == 0
    ref = ctx.after_p.detach()
    hid = ctx.forward(ref, S)
    _row_equal(eng.cache, 0, ref, 0)
    want = ctx.m.lm_head(hid[-1:]).float().argmax(-1)
    assert torch.equal(done[0][1], want)
    _row_equal(ctx.store.cache, 0, ctx.after_p, 0)            # the stored row is only read


def test_seeded_admission_state_graph(ctx):
    S = _embeds(21, ctx.D, 101)
    eng = ctx.engine("graph")
    h = eng.submit(state="v", inputs_embeds=S, max_new_tokens=1)
    done = eng.step()
    assert [x for x, _ in done] == [h] and eng.replays == 0 and ctx.store.pinned("v") == 0
    own = Cache.zeros(ctx.m.config, SMALL["slots"], DEV, torch.bfloat16)
    pp = PackedPrefill(ctx.m.model, own, max_seqs=8, buckets=SMALL["prefill_buckets"])
    idx = torch.tensor([0], device=DEV)
    for d, s in zip(own.states, ctx.after_p.states):
        for f in ("att_x_prev", "att_kv", "ffn_x_prev"):
            getattr(d, f).index_copy_(0, idx, getattr(s, f))
    h_last = pp.run([S], [0], fresh=False)
    _row_equal(eng.cache, 0, own, 0)
    assert torch.equal(done[0][1], ctx.m.lm_head(h_last).float().argmax(-1))
    _row_equal(ctx.store.cache, 0, ctx.after_p, 0)


def test_no_cross_talk_in_a_mixed_graph_pack(ctx):
    prompts = [_embeds(n, ctx.D, 110 + i) for i, n in enumerate((17, 40, 9))]
    kws = [_sampled(i, inputs_embeds=p, max_new_tokens=20) for i, p in enumerate(prompts)]
    with_store, plain = ctx.engine("graph"), ctx.engine("graph", store=None)
    hs = [with_store.submit(state="v" if i == 0 else None, **kw) for i, kw in enumerate(kws)]
    hp = [plain.submit(**kw) for kw in kws]                   # the same three prompts: the same bucket and GEMM shapes
    a, b = with_store.run(), plain.run()
    for i in (1, 2):
        assert torch.equal(a[hs[i]], b[hp[i]])
    assert a[hs[0]].numel() == 20
    # and the seeded one is what it is alone in a pack of the same composition: its neighbours did not leak into it either
    again = ctx.engine("graph")
    hs2 = [again.submit(state="v" if i == 0 else None, **{**kw, "seed": kw["seed"] + (50 if i else 0)}) for i, kw in enumerate(kws)]
    assert torch.equal(again.run()[hs2[0]], a[hs[0]])


def test_seeded_ids_do_not_depend_on_slot_or_time(ctx):
    S = _embeds(30, ctx.D, 120)
    kw = _sampled(1, inputs_embeds=S, max_new_tokens=24, state="v")
    alone = ctx.engine("eager")
    h = alone.submit(**kw)
    want = alone.run()[h]
    busy = ctx.engine("eager", check_every=4)
    others = [busy.submit(**_sampled(i, inputs_embeds=_embeds(12 + i, ctx.D, 121 + i), max_new_tokens=60)) for i in (0, 2)]
    busy.step()
    busy.step()
    assert sorted(busy.sched.busy) == [0, 1] and busy.replays == 8
    h2 = busy.submit(**kw)
    got = busy.run()
    assert busy.replays > 8 and torch.equal(got[h2], want) and all(got[o].numel() == 60 for o in others)


@pytest.mark.parametrize("admission", ["eager", "graph"])
def test_a_store_that_is_attached_but_unused_changes_no_id(ctx, admission):
    kws = [(_sampled(i) if i % 2 else {}) | dict(inputs_embeds=_embeds(5 + 13 * i, ctx.D, 130 + i), max_new_tokens=10 + 3 * i) for i in range(6)]
    out = []
    for store in ("own", None):
        eng = ctx.engine(admission, store=store)
        hs = [eng.submit(**kw) for kw in kws]
        got = eng.run()
        out.append([got[h] for h in hs])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_submit_n_from_a_stored_state(ctx):
    S, s = _embeds(11, ctx.D, 140), 4242
    kw = dict(inputs_embeds=S, max_new_tokens=16, do_sample=True, top_k=50, top_p=0.9, temperature=1.2, state="v")
    eng = ctx.engine("eager")
    hs = eng.submit_n(3, seed=s, **kw)
    assert ctx.store.pinned("v") == 1
    group = eng.run()
    assert ctx.store.pinned("v") == 0
    for i, h in enumerate(hs):
        one = eng.submit(seed=candidate_seed(s, i), **kw)
        assert torch.equal(eng.run()[one], group[h]), i
    assert len({tuple(group[h].tolist()) for h in hs}) > 1    # the candidates do differ
    lp = ctx.engine("eager", logprobs=True)
    hl = lp.submit_n(3, seed=s, **kw)
    got = lp.run()
    for a, b in zip(hs, hl):
        assert torch.equal(group[a], got[b])
        tok, cum = lp.take_logprobs(b)
        assert tok.numel() == 16 and torch.isfinite(cum)


def _mixed_requests(n, D, seed, hi=80, budgets=(5, 40)):
    """n requests, every third one a suffix of "v", every other one sampled."""
    rng = random.Random(seed)
    reqs = []
    for i in range(n):
        kw = dict(inputs_embeds=_embeds(rng.randint(3, hi), D, seed * 100 + i), max_new_tokens=rng.randint(*budgets))
        if i % 2:
            kw.update(_sampled(i))
        if i % 3 == 0:
            kw["state"] = "v"
        reqs.append(kw)
    return reqs


def _check_against_graph(eng, got, ref_eng, reqs):
    """Every group of the overlap engine's admission_log, submitted alone to a graph-mode engine: equal ids, request by request."""
    n = 0
    for _, _, group in eng.admission_log:
        assert ref_eng.sched.idle
        hs = [ref_eng.submit(**reqs[h]) for h in group]
        out = ref_eng.run()
        for h, r in zip(group, hs):
            assert torch.equal(got[h], out[r]), (h, group)
            n += 1
    return n


@pytest.fixture(scope="module")
def graph_ref(ctx):
    return ctx.engine("graph")


@pytest.mark.parametrize("lag", [0, 8])
def test_overlap_equals_graph_mode_per_composition_with_stored_states(ctx, graph_ref, lag):
    reqs = _mixed_requests(12, ctx.D, 7)
    eng = ctx.engine("overlap", overlap_replays=lag)
    hs = [eng.submit(**kw) for kw in reqs]
    assert ctx.store.pinned("v") == 4
    got = eng.run()
    assert ctx.store.pinned("v") == 0
    assert sorted(got) == hs and [got[h].numel() for h in hs] == [kw["max_new_tokens"] for kw in reqs]
    mixed = [g for _, _, g in eng.admission_log if {"state" in reqs[h] for h in g} == {True, False}]
    assert mixed, eng.admission_log                           # seeded and fresh requests did share a pack
    if lag:
        assert any(b > a for a, b, _ in eng.admission_log)    # and a prefill did run next to the step
    assert _check_against_graph(eng, got, graph_ref, reqs) == 12
    assert not eng.dstep.barrier_timed_out()


def test_put_equals_capture(ctx):
    S = _embeds(19, ctx.D, 150)
    kw = _sampled(2, inputs_embeds=S, max_new_tokens=20)
    eng = ctx.engine("eager")
    h = eng.submit(state="v", **kw)
    want = eng.run()[h]
    big = _pattern_cache(2, 3, ctx.D, ctx.m.config.num_heads, 9)   # rows 0 and 1 keep their noise
    for s in big.states:
        for t in (s.att_x_prev, s.att_kv, s.ffn_x_prev):
            t[2].zero_()
    ctx.forward(big, ctx.P, row=2)
    other = StateStore(ctx.m, 2)
    other.reserve("first")                                    # so that the row is not row 0
    assert other.put("p", big, row=2, tokens=TP) == 1 and other.tokens[1] == TP
    _row_equal(other.cache, 1, ctx.after_p, 0)
    assert not any(t[0].any() for t in _bits(other.cache))
    eng2 = ctx.engine("eager", store=other)
    h2 = eng2.submit(state="p", **kw)
    assert torch.equal(eng2.run()[h2], want)


def test_save_load_round_trip_gives_the_same_ids(ctx, tmp_path):
    S = _embeds(25, ctx.D, 160)
    kw = _sampled(1, inputs_embeds=S, max_new_tokens=20, state="v")
    eng = ctx.engine("graph")
    h = eng.submit(**kw)
    want = eng.run()[h]
    ctx.store.save(tmp_path / "voices.pt")
    back = StateStore.load(tmp_path / "voices.pt", ctx.m, capacity=2)
    assert back.names() == ["v"] and back.tokens[0] == TP and back.cache[0].att_kv.device == ctx.store.cache[0].att_kv.device
    _row_equal(back.cache, 0, ctx.after_p, 0)
    eng2 = ctx.engine("graph", store=back)
    h2 = eng2.submit(**kw)
    assert torch.equal(eng2.run()[h2], want)


def test_04b_widths_depth_4_with_stored_states():
    c = backbone.config_0p4b()
    m = _model(L=4, V=8193, hidden_size=c.hidden_size, decay_low_rank_dim=c.decay_low_rank_dim, a_low_rank_dim=c.a_low_rank_dim,
               v_low_rank_dim=c.v_low_rank_dim, gate_low_rank_dim=c.gate_low_rank_dim, intermediate_size=c.intermediate_size)
    D = m.config.hidden_size
    store = StateStore(m, 2)
    store.reserve("unused")
    assert store.capture("v", inputs_embeds=_embeds(200, D, 170)) == 1
    reqs = _mixed_requests(12, D, 17, hi=150, budgets=(1, 32))
    kw = dict(slots=8, max_new_tokens_cap=64, prefill_buckets=(256, 512), prefill_max_seqs=4, state_store=store)
    eng = ContinuousDecoder(m, admission="overlap", **kw)
    hs = [eng.submit(**r) for r in reqs]
    got = eng.run()                                           # raises on a barrier timeout
    assert sorted(got) == hs and all(got[h].numel() == r["max_new_tokens"] for h, r in zip(hs, reqs)) and store.pinned("v") == 0
    assert _check_against_graph(eng, got, ContinuousDecoder(m, admission="graph", **kw), reqs) == 12
    # and eager admission at these widths: the slot's rows after prefix + suffix are the model's own
    S = _embeds(40, D, 171)
    eager = ContinuousDecoder(m, admission="eager", **kw)
    h = eager.submit(state="v", inputs_embeds=S, max_new_tokens=1)
    done = eager.step()
    ref = Cache.zeros(m.config, 1, DEV, torch.bfloat16)
    hid = None
    with torch.no_grad():
        for e in (_embeds(200, D, 170), S):
            hid = m.model(inputs_embeds=e.unsqueeze(0), cu_seqlens=torch.tensor([0, e.shape[0]], dtype=torch.int32), past_key_values=ref,
                          cache_rows=torch.tensor([0])).last_hidden_state[0]
    _row_equal(eager.cache, 0, ref, 0)
    assert [x for x, _ in done] == [h] and torch.equal(done[0][1], m.lm_head(hid[-1:]).float().argmax(-1))
