"""GPU (-m gpu): continuous batching -- the per-slot draw entry (rwkv7_sample_slots_f32) against the one-row entry it must equal,
packed prefill into chosen cache rows (RWKV7Model(..., cache_rows=...)), and ContinuousDecoder: slot / admission-time invariance,
agreement with GraphDecoder, EOS retirement with slot reuse, and the 0.4B shape."""
import random

import pytest
import torch

from rwkvtts_amd import backbone
from rwkvtts_amd.backbone import Cache, LayerState
from rwkvtts_amd.continuous import ContinuousDecoder, SlotState, sample_slots
from rwkvtts_amd.decode import DecodeStep, GraphDecoder
from rwkvtts_amd.sampling import RowSampler, SampleTail

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DECISIVE = 0.03   # tests/test_bf16_greedy_gpu.py: top-1 / top-2 margin as a share of the logit range


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


def _prompts(n, D, seed, lo=3, hi=80):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(lo, hi, (n,), generator=g).tolist()
    return [(torch.randn(t, D, generator=g) * 0.5).to(DEV, torch.bfloat16) for t in lens]


# ---------------------------------------------------------------------------------------------------------------- 1. kernel
def test_slot_draws_equal_the_one_row_entry():
    V, D, S, LD, E = 8193, 128, 32, 64, 4242
    rng = random.Random(0)
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(S, V, generator=g) * 3).to(DEV)
    emb = torch.randn(V, D, generator=g).to(DEV, torch.bfloat16)
    perm = torch.randperm(S, generator=g).tolist()           # row r -> slot perm[r]
    sup = [5, 77, 8000]
    suppress = torch.tensor(sup, dtype=torch.int32, device=DEV)
    P = []
    for s in range(S):
        do_sample = s % 4 != 0
        top_k = rng.choice([0, 1, 7, 50, 64]) if do_sample else 0
        P.append(dict(do_sample=do_sample, top_k=top_k, top_p=rng.choice([1.0, 0.9, 0.5]) if top_k else 1.0,
                      temperature=rng.choice([0.6, 1.0, 1.37]), seed=rng.getrandbits(64), step=rng.randint(0, LD - 1),
                      min_until=0, live=s % 9 != 8))
        P[s]["limit"] = P[s]["step"] + 1 + rng.choice([0, 0, 1, 5])   # some slots reach their limit with this draw
    # EOS: boosted in a few rows; barred (min_until) in some of them
    for r, barred in ((1, False), (2, True), (3, True), (6, False)):
        logits[r, E] = 60.0
        P[perm[r]].update(min_until=P[perm[r]]["step"] + (1 if barred else 0), live=True)
    P[perm[2]]["do_sample"], P[perm[2]]["top_k"] = False, 0   # greedy and barred: the runner-up id
    P[perm[3]].update(do_sample=True, top_k=20, top_p=0.9)     # sampled and barred
    P[perm[1]].update(do_sample=False, top_k=0)                # greedy EOS: retires

    l64 = dict(dtype=torch.int64, device=DEV)
    t = lambda key, dt: torch.tensor([p[key] for p in P], dtype=dt, device=DEV)
    step, limit, min_until = t("step", torch.int64), t("limit", torch.int64), t("min_until", torch.int64)
    seed = torch.tensor([p["seed"] - (1 << 64) if p["seed"] >= 1 << 63 else p["seed"] for p in P], **l64)
    inv_temp = torch.tensor([(torch.tensor(1.0) / torch.tensor(p["temperature"], dtype=torch.float32)).item() for p in P],
                            dtype=torch.float32, device=DEV)
    top_k, top_p = t("top_k", torch.int32), t("top_p", torch.float32)
    do_sample, live = t("do_sample", torch.uint8), t("live", torch.uint8)
    ids = torch.full((S,), -3, **l64)
    seq = torch.full((S, LD), -7, **l64)
    x = torch.randn(S, D, generator=g).to(DEV, torch.bfloat16)
    before = dict(step=step.clone(), ids=ids.clone(), seq=seq.clone(), x=x.clone(), live=live.clone())
    st = SlotState()
    st.step, st.limit, st.min_until, st.seed = step.data_ptr(), limit.data_ptr(), min_until.data_ptr(), seed.data_ptr()
    st.inv_temp, st.top_k, st.top_p, st.do_sample = inv_temp.data_ptr(), top_k.data_ptr(), top_p.data_ptr(), do_sample.data_ptr()
    st.live, st.ids, st.seq, st.seq_ld = live.data_ptr(), ids.data_ptr(), seq.data_ptr(), LD
    st.emb, st.x, st.D, st.slots, st.top_k_max, st.eos = emb.data_ptr(), x.data_ptr(), D, S, 64, E
    row_slot = torch.tensor(perm, dtype=torch.int32, device=DEV)
    sample_slots(logits, st, row_slot, None, None, suppress, V)
    torch.cuda.synchronize()
    n_eos = 0
    for r in range(S):
        s, p = perm[r], P[perm[r]]
        if not p["live"]:
            cur = dict(step=step, ids=ids, seq=seq, x=x, live=live)
            for k, v in before.items():
                assert torch.equal(cur[k][s], v[s]), (k, s)
            continue
        rs = RowSampler(torch.device(DEV), [V], None, sup, p["do_sample"], p["top_k"], p["top_p"], p["temperature"], seed=p["seed"],
                        min_eos=(E, p["min_until"]))
        ids1, seq1 = torch.zeros(1, **l64), torch.full((1, LD), -7, **l64)
        unf, x1 = torch.ones(1, dtype=torch.bool, device=DEV), torch.zeros(1, D, dtype=torch.bfloat16, device=DEV)
        tail = SampleTail.make(ids1, seq1, unf, E, 0, emb, x1)
        rs(logits[r:r + 1], torch.tensor([p["step"]], **l64), tail=tail)
        torch.cuda.synchronize()
        want = int(ids1[0])
        assert int(ids[s]) == want, (r, s, p)
        assert torch.equal(seq[s], seq1[0]) and torch.equal(x[s].view(torch.int16), x1[0].view(torch.int16)), (r, s)
        assert int(step[s]) == p["step"] + 1
        assert int(live[s]) == int(want != E and p["step"] + 1 < p["limit"]), (r, s, want, p)
        if r in (2, 3):
            assert want != E
        n_eos += want == E
    assert int(ids[perm[1]]) == E and int(live[perm[1]]) == 0 and n_eos >= 2


# ---------------------------------------------------------------------------------------------------------------- 2. cache_rows
def _random_cache(cfg, N, seed):
    g = torch.Generator().manual_seed(seed)
    H, D = cfg.num_heads, cfg.hidden_size
    return Cache([LayerState((torch.randn(N, D, generator=g) * 0.5).to(DEV, torch.bfloat16), (torch.randn(N, H, 64, 64, generator=g) * 0.3).to(DEV),
                             (torch.randn(N, D, generator=g) * 0.5).to(DEV, torch.bfloat16)) for _ in range(cfg.num_hidden_layers)])


def _fields(c):
    return [t for s in c.states for t in (s.att_x_prev, s.att_kv, s.ffn_x_prev)]


def test_cache_rows_prefill():
    m = _model()
    cfg = m.config
    big = _random_cache(cfg, 7, 1)
    rows = [5, 0, 3]
    lens = [40, 1, 77]
    x = (torch.randn(1, sum(lens), cfg.hidden_size, generator=torch.Generator().manual_seed(2)) * 0.5).to(DEV, torch.bfloat16)
    cu = torch.tensor([0, 40, 41, 118], dtype=torch.int32)
    small = Cache([LayerState(*(t[rows].clone() for t in (s.att_x_prev, s.att_kv, s.ffn_x_prev))) for s in big.states])
    before = [t.clone() for t in _fields(big)]
    ptrs = [t.data_ptr() for t in _fields(big)]
    with torch.no_grad():
        h_ref = m.model(inputs_embeds=x, cu_seqlens=cu, past_key_values=small).last_hidden_state
        h = m.model(inputs_embeds=x, cu_seqlens=cu, past_key_values=big, cache_rows=torch.tensor(rows)).last_hidden_state
    assert torch.equal(h, h_ref)
    assert [t.data_ptr() for t in _fields(big)] == ptrs   # in place
    other = [i for i in range(7) if i not in rows]
    for b, a, s in zip(_fields(big), before, _fields(small)):
        assert torch.equal(b[rows], s)                    # named rows: as the N-row cache
        assert torch.equal(b[other], a[other])            # the rest: untouched
    with torch.no_grad():
        for bad in ([5, 0], [5, 5, 3], [5, 0, 7], [-1, 0, 3]):
            with pytest.raises(ValueError):
                m.model(inputs_embeds=x, cu_seqlens=cu, past_key_values=big, cache_rows=torch.tensor(bad))
    diff = _random_cache(cfg, 7, 1)
    diff.differentiable = True
    with pytest.raises(ValueError):
        m.model(inputs_embeds=x, cu_seqlens=cu, past_key_values=diff, cache_rows=torch.tensor(rows))


# ---------------------------------------------------------------------------------------------------------------- 3. invariance
REQ = [dict(max_new_tokens=30), dict(max_new_tokens=50, min_new_tokens=3), dict(max_new_tokens=33), dict(max_new_tokens=64)]
SAMPLED = [dict(do_sample=True, top_k=50, top_p=0.95, temperature=0.8, seed=11), dict(do_sample=True, seed=12),
           dict(do_sample=True, top_k=5, temperature=1.3, seed=13), dict(do_sample=True, top_k=64, top_p=0.5, seed=14)]


@pytest.mark.parametrize("sampled", [False, True])
def test_ids_do_not_depend_on_slot_or_admission_time(sampled):
    m = _model()
    prompts = _prompts(4, m.config.hidden_size, 5)
    kws = [dict(r, **(SAMPLED[i] if sampled else {})) for i, r in enumerate(REQ)]
    a = ContinuousDecoder(m, slots=8, max_new_tokens_cap=128)
    ha = [a.submit(inputs_embeds=p, **kw) for p, kw in zip(prompts, kws)]
    ra = a.run()
    b = ContinuousDecoder(m, slots=8, max_new_tokens_cap=128)
    busy = [b.submit(inputs_embeds=p, max_new_tokens=100, do_sample=True, seed=i) for i, p in enumerate(_prompts(4, m.config.hidden_size, 9))]
    out = dict(b.step())                                   # the four busy requests hold slots 0..3 and run 16 steps
    assert not out and sorted(b.sched.busy) == [0, 1, 2, 3]
    hb = [b.submit(inputs_embeds=p, **kw) for p, kw in zip(prompts, kws)]
    out.update(b.step())
    assert sorted(b.sched.busy) == list(range(8))         # admitted together, into slots 4..7, 16 steps later
    out.update(b.run())
    assert sorted(out) == sorted(busy + hb)
    for x, y, kw in zip(ha, hb, kws):
        assert ra[x].shape == (kw["max_new_tokens"],)
        assert torch.equal(ra[x], out[y]), (kw, ra[x], out[y])


# ---------------------------------------------------------------------------------------------------------------- 4. vs GraphDecoder
def _margins(m, prompt, ids):
    """The logits GraphDecoder decides on (same prefill call, same step kernel), teacher-forced along its ids: relative top-2 margin."""
    cache = Cache.zeros(m.config, 1, DEV, torch.bfloat16)
    out = []
    with torch.no_grad():
        lg = m(inputs_embeds=prompt.unsqueeze(0), past_key_values=cache, use_cache=True, logits_to_keep=1).logits[:, -1].float()
        step = DecodeStep(m.model, m.lm_head, cache)
        emb = m.get_input_embeddings().weight
        for t in range(len(ids)):
            top = lg[0].topk(2).values
            out.append(((top[0] - top[1]) / (lg[0].max() - lg[0].min())).item())
            if t + 1 < len(ids):
                lg = step(emb[ids[t:t + 1]].contiguous())
    return out


def test_greedy_agrees_with_graph_decoder():
    m = _model()
    prompts = _prompts(6, m.config.hidden_size, 21, lo=8, hi=100)
    eng = ContinuousDecoder(m, slots=4, max_new_tokens_cap=64)   # six requests through four slots: two are admitted later
    hs = [eng.submit(inputs_embeds=p, max_new_tokens=40 + 4 * i) for i, p in enumerate(prompts)]
    got = eng.run()
    for i, (h, p) in enumerate(zip(hs, prompts)):
        ref = GraphDecoder(m, 1, step_kernel=True).generate(inputs_embeds=p.unsqueeze(0), max_new_tokens=40 + 4 * i)[0]
        mg = _margins(m, p, ref)
        first_indecisive = next((t for t, v in enumerate(mg) if v <= DECISIVE), len(mg))
        ne = (got[h] != ref).nonzero()
        prefix = int(ne[0]) if len(ne) else len(ref)
        assert prefix >= first_indecisive, (i, prefix, first_indecisive)


# ---------------------------------------------------------------------------------------------------------------- 5. EOS
def test_eos_retires_and_the_slot_is_reused():
    m = _model()
    p0, p1 = _prompts(2, m.config.hidden_size, 31)
    kw0 = dict(max_new_tokens=40, do_sample=True, top_k=50, seed=3)
    kw1 = dict(max_new_tokens=40, do_sample=True, top_k=50, seed=4)
    solo = ContinuousDecoder(m, slots=1, max_new_tokens_cap=64)
    h = solo.submit(inputs_embeds=p0, **kw0)
    ids0 = solo.run()[h]
    # EOS = the id the request emits at step 5 (or the first later step whose id is new)
    t = next(t for t in range(5, 40) if int(ids0[t]) not in ids0[:t].tolist())
    E = int(ids0[t])
    solo1 = ContinuousDecoder(m, slots=1, max_new_tokens_cap=64, eos_token_id=E)
    h = solo1.submit(inputs_embeds=p1, **kw1)
    ids1 = solo1.run()[h]
    eng = ContinuousDecoder(m, slots=1, max_new_tokens_cap=64, eos_token_id=E)
    h0 = eng.submit(inputs_embeds=p0, **kw0)
    h1 = eng.submit(inputs_embeds=p1, **kw1)      # pending until the first request retires
    got = eng.run()
    assert got[h0].shape == (t + 1,) and int(got[h0][-1]) == E and torch.equal(got[h0], ids0[:t + 1])
    assert torch.equal(got[h1], ids1)


# ---------------------------------------------------------------------------------------------------------------- 6. 0.4B shape
def test_04b_shape_every_handle_once():
    c = backbone.config_0p4b()
    m = _model(L=c.num_hidden_layers, V=8193, hidden_size=c.hidden_size, decay_low_rank_dim=c.decay_low_rank_dim,
               a_low_rank_dim=c.a_low_rank_dim, v_low_rank_dim=c.v_low_rank_dim, gate_low_rank_dim=c.gate_low_rank_dim,
               intermediate_size=c.intermediate_size)
    rng = random.Random(7)
    eng = ContinuousDecoder(m, slots=32, max_new_tokens_cap=96)
    prompts = _prompts(64, m.config.hidden_size, 41, lo=4, hi=200)
    want = {}
    got = {}
    for i, p in enumerate(prompts):
        n = rng.randint(1, 96)
        want[eng.submit(inputs_embeds=p, max_new_tokens=n, do_sample=bool(i % 2), top_k=20, seed=i)] = n
        if i % 16 == 15:
            for h, ids in eng.step():
                assert h not in got
                got[h] = ids
    for h, ids in eng.run().items():
        assert h not in got
        got[h] = ids
    assert sorted(got) == sorted(want)
    for h, n in want.items():
        assert got[h].shape == (n,) and got[h].dtype == torch.int64
        assert int(got[h].min()) >= 0 and int(got[h].max()) < 8193
