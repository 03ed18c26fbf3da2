"""GPU (-m gpu): best-of-n requests in the continuous decoder.

Kernel: rwkv7_sample_slots_lp_f32 against rwkv7_sample_slots_f32 on cloned state (every field bit for bit), its log-probabilities
against an fp64 log_softmax on the CPU over the ids the draw could produce, the fields of skipped slots, placement independence and
the fp64 running sum -- for the three register-count instantiations, three draw kinds, the restrictions and the edge rows.

Engine: ContinuousDecoder(logprobs=True) changes no id; candidate i of submit_n is the stand-alone request with candidate_seed(seed,
i); the siblings' cache rows equal the first candidate's right after admission; cum_lp is the sequential fp64 sum of tok_lp.

Tolerance of the log-probabilities: 5e-5 absolute for logits with |x| <= 30.  x[id] - max is one fp32 subtraction at magnitude <= 64
(half an ulp: 4e-6), the exp-sum of up to 15360 terms in [0, 1] and its log add a few 1e-6 -- a tenfold margin."""
import math

import pytest
import torch

from rwkvtts_amd.continuous import ContinuousDecoder, SlotLogprob, SlotState, candidate_seed, rank_candidates, sample_slots

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5
NEG = float("-inf")
PAD = 12            # logits columns beyond the domain: the row stride is not the width, and an allowed range can cut both ends
LO = 7              # ... its first id
S, LD, D = 6, 12, 64
KINDS = {"greedy": dict(do_sample=0, top_k=0, top_p=1.0, temperature=1.0),
         "topk": dict(do_sample=1, top_k=50, top_p=0.8, temperature=0.7),
         "multinomial": dict(do_sample=1, top_k=0, top_p=1.0, temperature=1.3)}
LAYOUT = [4, -1, 6, 2]   # 4 rows over 6 slots: slot 2 is not live, one row has no slot, one names a slot past the end


# ---------------------------------------------------------------------------------------------------------------- kernel
class _Slots:
    """Device state of S slots for one call, and a clone()."""

    def __init__(self, kind, steps, live, eos=-1, min_until=None, seeds=None, t=None):
        if t is None:
            i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
            k = KINDS[kind]
            g = torch.Generator().manual_seed(99)
            seeds = [0x1234567 + 977 * s for s in range(S)] if seeds is None else seeds
            t = dict(step=i64(steps), limit=i64([st + 3 for st in steps]), min_until=i64([0] * S if min_until is None else min_until),
                     seed=i64(seeds), inv_temp=torch.full((S,), 1.0 / k["temperature"], dtype=torch.float32, device=DEV),
                     top_k=torch.full((S,), k["top_k"], dtype=torch.int32, device=DEV),
                     top_p=torch.full((S,), k["top_p"], dtype=torch.float32, device=DEV),
                     do_sample=torch.full((S,), k["do_sample"], dtype=torch.uint8, device=DEV),
                     live=torch.tensor(live, dtype=torch.uint8, device=DEV), ids=i64([-3] * S), seq=torch.full((S, LD), -7, dtype=torch.int64, device=DEV),
                     x=torch.randn(S, D, generator=g).to(DEV, torch.bfloat16),
                     tok_lp=torch.full((S, LD), 777.0, dtype=torch.float32, device=DEV),
                     cum_lp=torch.full((S,), 5.5, dtype=torch.float64, device=DEV))
        self.t, self.eos = t, eos

    def clone(self):
        return _Slots(None, None, None, self.eos, t={k: v.clone() for k, v in self.t.items()})

    def draw(self, logits, row_slot, emb, allow, suppress, domain, lp):
        t, st = self.t, SlotState()
        for k in ("step", "limit", "min_until", "seed", "inv_temp", "top_k", "top_p", "do_sample", "live", "ids", "seq", "x"):
            setattr(st, k, t[k].data_ptr())
        st.seq_ld, st.emb, st.D, st.slots, st.top_k_max, st.eos = LD, emb.data_ptr(), D, S, 64, self.eos
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
        keep = [i32([allow[0]]), i32([allow[1]])] if allow else [None, None]
        sup = i32(suppress) if suppress else None
        sample_slots(logits, st, i32(row_slot), keep[0], keep[1], sup, domain,
                     SlotLogprob(t["tok_lp"].data_ptr(), t["cum_lp"].data_ptr()) if lp else None)
        torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else \
        t.view(torch.int64) if t.dtype == torch.float64 else t


def _rows(domain):
    """Four logits rows [4, domain + PAD], |x| <= 30: a plain one, one with a dominant logit, one with -inf entries, and one that is
    -inf over the whole domain.  Column A is the argmax of rows 0 and 2, C their runner-up; B dominates row 1."""
    g = torch.Generator().manual_seed(domain)
    x = (torch.randn(4, domain + PAD, generator=g) * 4).clamp_(-30, 30)
    A, B, C = LO + domain // 2, LO + domain // 3, LO + 5
    x[:, A], x[:, C] = 25.0, 24.0
    x[1, B] = 30.0
    x[2, LO + 1::3] = NEG
    x[2, A], x[2, C] = 25.0, 24.0
    x[3] = NEG
    return x, A, B, C


def _restrictions(domain, A, C):
    """(name, allow, suppress, eos): the ids [lo, hi) the draw may use, minus `suppress`, minus eos (barred at the step of every call)"""
    V = domain + PAD
    return [("none", None, [], -1), ("allow", (LO, LO + domain), [], -1), ("suppress", None, [A, 3, domain - 1], -1),
            ("eos_bar", None, [], A), ("all", (LO, LO + domain), [A, LO + 3, V - 1], C)]


def _want_lp(row, lo, hi, suppress, eos, barred, id_):
    """fp64 log_softmax over the allowed ids of one row on the CPU, at the drawn id; -inf when nothing is allowed"""
    x = row.double().clone()
    keep = torch.zeros_like(x, dtype=torch.bool)
    keep[lo:hi] = True
    for t in suppress:
        keep[t] = False
    if eos >= 0 and barred:
        keep[eos] = False
    x[~keep] = NEG
    if torch.isneginf(x).all():
        return NEG
    assert keep[id_], "the draw chose an id outside the set it may use"
    return float(torch.log_softmax(x, 0)[id_])


@pytest.mark.parametrize("domain", [1025, 8193, 15360])
def test_lp_entry_equals_the_plain_entry_and_an_fp64_log_softmax(domain):
    logits_cpu, A, B, C = _rows(domain)
    for name, allow, suppress, eos in _restrictions(domain, A, C):
        x_cpu = logits_cpu.clone()
        lo, hi = allow if allow else (0, domain)
        # whatever lies outside the allowed range is the largest logit of its row: it must not be drawn and not be summed
        x_cpu[:, :lo], x_cpu[:, hi:] = 30.0, 30.0
        logits = x_cpu.to(DEV)
        emb = torch.randn(domain + PAD, D, generator=torch.Generator().manual_seed(3)).to(DEV, torch.bfloat16)
        steps = [3, 0, 9, 5, 1, 7]
        # the prescribed layout with each row in turn as the one that is drawn, then all four rows live on permuted slots
        layouts = [(LAYOUT[-r:] + LAYOUT[:-r], [1, 1, 0, 1, 1, 1]) for r in range(4)] + [([3, 5, 0, 1], [1] * S)]
        for kind in KINDS:
            for row_slot, live in layouts:
                barred = [st + 1 for st in steps]                              # EOS barred at this step in every slot
                a = _Slots(kind, steps, live, eos, barred)
                b = a.clone()
                before = a.clone()
                a.draw(logits, row_slot, emb, allow, suppress, hi - lo, lp=True)
                b.draw(logits, row_slot, emb, allow, suppress, hi - lo, lp=False)
                what = (domain, name, kind, row_slot)
                for k in ("seq", "ids", "step", "live", "x"):                  # check 1
                    assert torch.equal(_bits(a.t[k]), _bits(b.t[k])), (k, what)
                drawn = {s: r for r, s in enumerate(row_slot) if 0 <= s < S and live[s]}
                assert drawn, what
                for s in range(S):
                    if s not in drawn:                                         # check 3: every field of a skipped slot, sentinels included
                        for k, v in a.t.items():
                            assert torch.equal(_bits(v[s]), _bits(before.t[k][s])), (k, s, what)
                        continue
                    r, st = drawn[s], steps[s]
                    id_ = int(a.t["ids"][s])
                    assert int(a.t["step"][s]) == st + 1 and int(a.t["seq"][s, st]) == id_
                    got = float(a.t["tok_lp"][s, st])
                    want = _want_lp(x_cpu[r], lo, hi, suppress, eos, True, id_)   # check 2
                    if r == 3:
                        assert want == NEG and got == NEG and id_ == lo, (got, id_, what)   # nothing allowed: -inf and the first id
                    else:
                        assert math.isfinite(want) and abs(got - want) <= TOL, (got, want, s, what)
                        if r == 1 and kind == "greedy":
                            assert id_ == B and got > -0.02                                 # the dominant logit: 99 % of the mass
                    other = torch.ones(LD, dtype=torch.bool)
                    other[st] = False
                    assert bool((a.t["tok_lp"][s].cpu()[other] == 777.0).all()), what        # only the step's column is written
                    assert _bits(a.t["cum_lp"][s]).item() == _bits(before.t["cum_lp"][s] + a.t["tok_lp"][s, st].double()).item()


@pytest.mark.parametrize("domain", [1025, 8193, 15360])
@pytest.mark.parametrize("kind", list(KINDS))
def test_tok_lp_does_not_depend_on_row_slot_or_grid(domain, kind):
    """check 4: the same logits row, key and step at two rows / slots of one call and in a call with another grid: the same bits"""
    x_cpu, A, B, C = _rows(domain)
    x_cpu[3] = x_cpu[0]
    logits = x_cpu.to(DEV)
    emb = torch.zeros(domain + PAD, D, dtype=torch.bfloat16, device=DEV)
    seeds, steps = [42] * S, [4] * S
    a = _Slots(kind, steps, [1] * S, seeds=seeds)
    a.draw(logits, [5, 2, 1, 0], emb, None, [A], domain, lp=True)              # row 0 -> slot 5, its copy (row 3) -> slot 0
    b = _Slots(kind, steps, [1] * S, seeds=seeds)
    b.draw(logits[2:4], [0, 3], emb, None, [A], domain, lp=True)               # two rows: the copy -> slot 3
    lp = [a.t["tok_lp"][5, 4], a.t["tok_lp"][0, 4], b.t["tok_lp"][3, 4]]
    assert int(a.t["ids"][5]) == int(a.t["ids"][0]) == int(b.t["ids"][3])
    assert math.isfinite(float(lp[0])) and float(lp[0]) < 0
    assert _bits(lp[0]).item() == _bits(lp[1]).item() == _bits(lp[2]).item()
    assert _bits(a.t["tok_lp"][1, 4]).item() == _bits(b.t["tok_lp"][0, 4]).item()   # row 2, in both calls


@pytest.mark.parametrize("kind", list(KINDS))
def test_cum_lp_is_the_sequential_fp64_sum(kind):
    """check 5: five consecutive calls; cum_lp equals the host's fp64 sum of the fp32 values in step order, bit for bit"""
    domain = 8193
    x_cpu, A, B, C = _rows(domain)
    emb = torch.zeros(domain + PAD, D, dtype=torch.bfloat16, device=DEV)
    steps = [3, 0, 6, 5, 1, 7]
    a = _Slots(kind, steps, [1] * S)
    a.t["limit"].fill_(100)
    a.t["cum_lp"].zero_()
    g = torch.Generator().manual_seed(8)
    row_slot = [3, 5, 0, 1]
    for call in range(5):                                                      # other logits every step; what is -inf stays -inf
        x = (x_cpu + torch.randn(4, domain + PAD, generator=g)).clamp_(-30, 30)
        x[torch.isneginf(x_cpu)] = NEG
        a.draw(x.to(DEV), row_slot, emb, None, [], domain, lp=True)
    tok, cum = a.t["tok_lp"].cpu(), a.t["cum_lp"].cpu()
    for r, s in enumerate(row_slot):
        assert int(a.t["step"][s]) == steps[s] + 5
        want = torch.zeros((), dtype=torch.float64)
        for c in range(steps[s], steps[s] + 5):
            assert tok[s, c] != 777.0
            want = want + tok[s, c].double()
        assert _bits(cum[s]).item() == _bits(want).item(), (s, cum[s], want)
        assert (cum[s] == NEG) == (r == 3)
    for s in (2, 4):                                                            # slots without a row
        assert float(cum[s]) == 0.0 and bool((tok[s] == 777.0).all())


# ---------------------------------------------------------------------------------------------------------------- engine
def tiny_model(L=2, V=300, seed=0, **dims):
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


def teacher_forced_gap(m, prompt, ids, tok_lp):
    """max |(-tok_lp) - CE| where CE is the per-token cross-entropy of the eager bf16 forward over prompt + generated ids.  A figure
    to record, not a bound: the decode step and the prefill kernels round differently."""
    emb = m.get_input_embeddings().weight
    x = torch.cat([prompt, emb[ids[:-1]]], 0).unsqueeze(0)
    with torch.no_grad():
        lg = m(inputs_embeds=x).logits[0, prompt.shape[0] - 1:].float()
    ce = -torch.log_softmax(lg.double(), -1).gather(1, ids.view(-1, 1))[:, 0]
    return float(((-tok_lp.double()) - ce).abs().max())


@pytest.fixture(scope="module")
def small():
    return tiny_model()


@pytest.fixture(scope="module")
def prompts(small):
    g = torch.Generator().manual_seed(17)
    return [(torch.randn(t, small.config.hidden_size, generator=g) * 0.5).to(DEV, torch.bfloat16) for t in (17, 40)]


KW = dict(slots=4, max_new_tokens_cap=24, check_every=2, prefill_buckets=(64, 128), prefill_max_seqs=4)
SAMPLED = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.8)


def _check_sum(eng, handles, out):
    """guarantee 4 on every finished handle: cum_lp is the fp64 sum of tok_lp in step order, bit for bit"""
    res = {}
    for h in handles:
        tok, cum = eng.take_logprobs(h)
        assert tok.dtype == torch.float32 and tok.shape == out[h].shape and cum.dtype == torch.float64 and cum.dim() == 0
        want = torch.zeros((), dtype=torch.float64)
        for v in tok.cpu():
            want = want + v.double()
        assert _bits(cum.cpu()).item() == _bits(want).item(), (h, cum, want)
        assert bool((tok <= 0).all()) and bool(torch.isfinite(tok).all())
        with pytest.raises(KeyError):
            eng.take_logprobs(h)
        res[h] = (tok, cum)
    return res


_eos = {}


def _eos_id(small, prompts):
    """An id the first sampled request emits after a few steps: with it as EOS the batch below ends some requests early."""
    if "id" not in _eos:
        eng = ContinuousDecoder(small, **KW)
        h = eng.submit(inputs_embeds=prompts[0], max_new_tokens=24, seed=5, **SAMPLED)
        ids = eng.run()[h].tolist()
        t = next(t for t in range(4, 24) if ids[t] not in ids[:t])
        _eos["id"] = ids[t]
    return _eos["id"]


@pytest.mark.parametrize("admission", ["eager", "graph", "overlap"])
def test_logprobs_change_no_id(small, prompts, admission):
    """guarantee 1: a mixed greedy / sampled batch with an EOS id, six requests through four slots"""
    E = _eos_id(small, prompts)
    reqs = [dict(inputs_embeds=prompts[0], max_new_tokens=24, seed=5, **SAMPLED), dict(inputs_embeds=prompts[1], max_new_tokens=20),
            dict(inputs_embeds=prompts[1], max_new_tokens=24, do_sample=True, seed=6, min_new_tokens=3),
            dict(inputs_embeds=prompts[0], max_new_tokens=9), dict(inputs_embeds=prompts[0], max_new_tokens=24, seed=7, **SAMPLED),
            dict(inputs_embeds=prompts[1], max_new_tokens=1, seed=8, **SAMPLED)]
    res = []
    for logprobs in (False, True):
        eng = ContinuousDecoder(small, admission=admission, eos_token_id=E, logprobs=logprobs, **KW)
        hs = [eng.submit(**kw) for kw in reqs]
        out = eng.run()
        assert sorted(out) == hs
        res.append((out, eng.step_t.clone(), eng.live.clone(), eng.replays))
        if logprobs:
            _check_sum(eng, hs, out)
        else:
            with pytest.raises(ValueError):
                eng.take_logprobs(hs[0])
    (a, step_a, live_a, rep_a), (b, step_b, live_b, rep_b) = res
    for h in a:
        assert torch.equal(a[h], b[h]), (h, a[h], b[h])
    assert torch.equal(step_a, step_b) and torch.equal(live_a, live_b) and rep_a == rep_b
    if admission == "eager":   # (the EOS id was taken from an eager run; another admission mode may round the prefill differently)
        assert any(int(a[h][-1]) == E and a[h].numel() < kw["max_new_tokens"] for h, kw in zip(hs, reqs)), "no request ended on EOS"


@pytest.mark.parametrize("admission", ["eager", "graph"])
def test_candidates_equal_stand_alone_requests(small, prompts, admission):
    """guarantee 2 (and 4): a group of 3 waits behind busy slots, lands on slots 0, 1 and 3 around a running request, and every
    candidate is the stand-alone submit(seed=candidate_seed(seed, i)) admitted alone -- ids and log-probabilities bit for bit"""
    seed = (1 << 64) - 2                                       # candidate 2 wraps to key 0
    kw = dict(inputs_embeds=prompts[1], max_new_tokens=20, min_new_tokens=2, **SAMPLED)
    eng = ContinuousDecoder(small, admission=admission, logprobs=True, **KW)
    others = [eng.submit(inputs_embeds=prompts[0], max_new_tokens=n, do_sample=True, seed=30 + n) for n in (7, 3, 24, 3)]
    out = dict(eng.step())                                     # slots 0..3 busy
    group = eng.submit_n(3, seed=seed, **kw)
    waited = 0
    while any(r.handle in group for r in eng.sched.pending):
        assert all(r.handle in group for r in eng.sched.pending) and len(eng.sched.pending) == 3   # whole or not at all
        waited += bool(eng.sched.free)
        out.update(eng.step())
    assert waited >= 1, "the group never waited with some, but not enough, slots free"
    where = {r.handle: s for s, r in eng.sched.busy.items()}
    assert [where[h] for h in group] == [0, 1, 3] and where[others[2]] == 2
    out.update(eng.run())
    lp = _check_sum(eng, others + group, out)
    solo = ContinuousDecoder(small, admission=admission, logprobs=True, **KW)
    for i, h in enumerate(group):
        hs = solo.submit(seed=candidate_seed(seed, i), **kw)
        want = solo.run()[hs]
        assert torch.equal(out[h], want), (i, out[h], want)
        tok, cum = solo.take_logprobs(hs)
        assert torch.equal(_bits(lp[h][0]), _bits(tok)) and _bits(lp[h][1]).item() == _bits(cum).item()
    assert len({tuple(out[h].tolist()) for h in group}) == 3, "three keys, one id sequence: the candidates did not draw on their own"
    order = rank_candidates(torch.stack([lp[h][1] for h in group]), [out[h].numel() for h in group])
    assert sorted(order) == [0, 1, 2]


@pytest.mark.parametrize("admission", ["eager", "graph"])
@pytest.mark.parametrize("layout", ["one_and_three", "two_and_two"])
def test_sibling_rows_equal_the_first_candidates(small, prompts, admission, layout):
    """guarantee 3: max_new_tokens = 1 and no EOS, so no replay runs before the rows are read; two prompts admitted together"""
    eng = ContinuousDecoder(small, admission=admission, **KW)
    kw = dict(max_new_tokens=1, do_sample=True)
    if layout == "one_and_three":
        eng.submit(inputs_embeds=prompts[0], seed=1, **kw)
        eng.submit_n(3, inputs_embeds=prompts[1], seed=2, **kw)
        same, heads = [(1, 2), (1, 3)], (0, 1)
    else:
        eng.submit_n(2, inputs_embeds=prompts[0], seed=1, **kw)
        eng.submit_n(2, inputs_embeds=prompts[1], seed=2, **kw)
        same, heads = [(0, 1), (2, 3)], (0, 2)
    done = eng.step()
    assert len(done) == 4 and eng.replays == 0
    for st in eng.cache.states:
        for t in (st.att_x_prev, st.att_kv, st.ffn_x_prev):
            for a, b in same:
                assert torch.equal(_bits(t[a]), _bits(t[b])), (a, b, tuple(t.shape))
            assert not torch.equal(t[heads[0]], t[heads[1]]) and bool(t[heads[1]].ne(0).any())


@pytest.mark.parametrize("admission", ["eager", "graph"])
def test_greedy_candidates(small, prompts, admission, capsys):
    """greedy candidates: n equal id sequences, every log-probability in [-log(domain), 0]; the distance to the teacher-forced
    cross-entropy of the eager forward is printed (tools/bench_best_of.py records it), not asserted"""
    eng = ContinuousDecoder(small, admission=admission, logprobs=True, **KW)
    hs = eng.submit_n(3, inputs_embeds=prompts[0], max_new_tokens=24)
    out = eng.run()
    lp = _check_sum(eng, hs, out)
    for h in hs[1:]:
        assert torch.equal(out[h], out[hs[0]]) and torch.equal(_bits(lp[h][0]), _bits(lp[hs[0]][0]))
    tok = lp[hs[0]][0]
    assert float(tok.min()) >= -math.log(eng.max_domain) and float(tok.max()) <= 0.0
    assert rank_candidates([float(lp[h][1]) for h in hs], [24] * 3) == [0, 1, 2]
    gap = teacher_forced_gap(small, prompts[0], out[hs[0]], tok)
    with capsys.disabled():
        print(f"\n[best-of] {admission}: max |-tok_lp - teacher-forced CE| over 24 greedy ids = {gap:.4f}")
