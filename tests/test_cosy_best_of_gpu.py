"""GPU (-m gpu): best-of-n utterances in the Cosy engine.

Kernel: rwkv7_ras_slots_lp_f32 against rwkv7_ras_slots_f32 on cloned state (every field bit for bit), its log-probabilities against
an fp64 log_softmax on the CPU over the ids the draw could produce, the EOS draw's end_lp, the fields of skipped slots, placement
independence and the fp64 running sum -- for the three elements-per-thread classes, Cosy's real head and the first size of the next
class.

Engine: ContinuousCosyDecoder(logprobs=True) changes no id; candidate i of submit_n is the stand-alone request with
candidate_seed(seed, i); the siblings' cache rows equal the first candidate's right after admission; every tok_lp entry is the fp64
log-softmax of the logits its step produced and cum_lp their sequential fp64 sum; take_logprobs' contract; rank_candidates.

Tolerance of the log-probabilities: 5e-5 absolute for logits with |x| <= 30 (TOL of tests/test_best_of_gpu.py: the same arithmetic
and logit range).  x[id] - max is one fp32 subtraction at magnitude <= 60 (half an ulp: 2e-6); the exp-sum of up to 8449 terms and
its log add about 1e-5 when the sum is as small as exp(-60) (a barred EOS that holds the row's maximum) and a few 1e-6 otherwise."""
import ctypes
import math

import pytest
import torch

from rwkvtts_amd import _lib
from rwkvtts_amd.continuous import candidate_seed, rank_candidates
from rwkvtts_amd.continuous_cosy import ContinuousCosyDecoder, RasSlotLogprob, RasSlotState, cosy_request, ras_slots
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7CosyLM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5
NEG = float("-inf")
PAD = 12                  # logits columns beyond V: the row stride is wider than the row
S, LD, WLD, D, WIN = 6, 12, 12, 64, 10
LAYOUT = [4, -1, 6, 2]    # 4 rows over 6 slots: slot 2 is not live, one row has no slot, one names a slot past the end
STEPS = [3, 0, 9, 5, 1, 7]
N_OUT = [2, 0, 5, 3, 1, 4]   # emitted so far: not the loop index, so a value written at column `step` is caught
SENT_TOK, SENT_CUM, SENT_END = 777.0, 5.5, -123.0
STATE = ("step", "live", "recent", "ptr", "n_out", "ids", "seq", "x")
LPS = ("tok_lp", "cum_lp", "end_lp")


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else \
        t.view(torch.int64) if t.dtype == torch.float64 else t


# ---------------------------------------------------------------------------------------------------------------- kernel
class _Slots:
    """Device state of S slots over V ids (EOS = V - 1) for one call, and a clone()."""

    def __init__(self, V, top_k=25, top_p=1.0, tau_r=0.5, n_ignore=0, live=(1,) * S, seeds=None, steps=STEPS, n_out=N_OUT, ring=-1, t=None):
        self.V, self.eos = V, V - 1
        if t is None:
            i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
            full = lambda v, dt: torch.full((S,), v, dtype=dt, device=DEV)
            g = torch.Generator().manual_seed(99)
            seeds = [0x1234567 + 977 * s for s in range(S)] if seeds is None else seeds
            t = dict(step=i64(list(steps)), limit=i64([st + 30 for st in steps]), n_ignore=i64([st + 1 if n_ignore else 0 for st in steps]),
                     seed=i64(seeds), top_k=full(top_k, torch.int32), top_p=full(top_p, torch.float32), tau_r=full(tau_r, torch.float32),
                     live=torch.tensor(list(live), dtype=torch.uint8, device=DEV),
                     recent=torch.full((S, WLD), ring, dtype=torch.int64, device=DEV), ptr=i64([n % WIN for n in n_out]), ids=i64([-3] * S),
                     n_out=i64(list(n_out)), seq=torch.full((S, LD), -7, dtype=torch.int64, device=DEV),
                     x=torch.randn(S, D, generator=g).to(DEV, torch.bfloat16),
                     emb=torch.randn(V, D, generator=g).to(DEV, torch.bfloat16),
                     tok_lp=torch.full((S, LD), SENT_TOK, dtype=torch.float32, device=DEV),
                     cum_lp=torch.full((S,), SENT_CUM, dtype=torch.float64, device=DEV),
                     end_lp=torch.full((S,), SENT_END, dtype=torch.float32, device=DEV))
        self.t = t

    def clone(self):
        return _Slots(self.V, t={k: (v if k == "emb" else v.clone()) for k, v in self.t.items()})

    def structs(self):
        t, st = self.t, RasSlotState()
        for k in ("step", "limit", "n_ignore", "seed", "top_k", "top_p", "tau_r", "live", "recent", "ptr", "ids", "n_out", "seq", "emb", "x"):
            setattr(st, k, t[k].data_ptr())
        st.win_ld, st.seq_ld, st.D, st.slots, st.win_size, st.top_k_max, st.eos = WLD, LD, D, S, WIN, 128, self.eos
        return st, RasSlotLogprob(t["tok_lp"].data_ptr(), t["cum_lp"].data_ptr(), t["end_lp"].data_ptr())

    def draw(self, logits, row_slot, lp):
        """logits [rows, V + PAD]: the entry gets the first V columns, with the stride of the wider row"""
        st, lps = self.structs()
        rs = None if row_slot is None else torch.tensor(row_slot, dtype=torch.int32, device=DEV)
        ras_slots(logits[:, :self.V], st, rs, lps if lp else None)
        torch.cuda.synchronize()


def _rows(V, case):
    """Four logits rows [4, V + PAD], |x| <= 30, and the column A that is the argmax of every row without a dominant EOS.  The pad
    columns hold the largest value: nothing past V may be read."""
    g = torch.Generator().manual_seed(V + len(case))
    x = (torch.randn(4, V + PAD, generator=g) * 4).clamp_(-30, 30)
    A, eos = V // 2, V - 1
    x[:, eos] = -30.0
    x[:, A] = x[:, :V].max(1).values + (0.01 if case == "fallback" else 1.0)
    if case in ("eos_barred", "eos_drawn"):
        x[:, eos] = 30.0
    if case == "neg_inf":
        x[:, :V] = NEG
    x[:, V:] = 30.0
    return x, A


CASES = {"top_k_1": dict(top_k=1), "top_k_25": dict(top_k=25), "top_k_128": dict(top_k=128),
         "fallback": dict(top_k=1, tau_r=0.1),            # + a ring full of the argmax: the draw from the full distribution is taken
         "eos_barred": dict(top_k=25, n_ignore=1),        # EOS is the row's argmax while step < n_ignore
         "eos_drawn": dict(top_k=25, top_p=0.8),          # EOS holds the row's mass and is not barred
         "neg_inf": dict(top_k=25)}


def _want_lp(row, V, eos, barred, id_):
    """fp64 log_softmax over the ids the draw may produce, at the drawn id; -inf for a row without a finite logit"""
    x = row[:V].double().clone()
    if barred:
        x[eos] = NEG
    if torch.isneginf(x).all():
        return NEG
    assert x[id_] > NEG, "the draw chose an id outside the set it may use"
    return float(torch.log_softmax(x, 0)[id_])


@pytest.mark.parametrize("V", [97, 1281, 6562, 8449])
def test_lp_entry_equals_the_plain_entry_and_an_fp64_log_softmax(V):
    eos = V - 1
    # the prescribed layout with each row in turn as the one that is drawn, then all four rows live on permuted slots
    layouts = [(LAYOUT[-r:] + LAYOUT[:-r], [1, 1, 0, 1, 1, 1]) for r in range(4)] + [([3, 5, 0, 1], [1] * S)]
    for case, kw in CASES.items():
        x_cpu, A = _rows(V, case)
        logits = x_cpu.to(DEV)
        barred = bool(kw.get("n_ignore"))
        moved = 0
        for row_slot, live in layouts:
            a = _Slots(V, live=live, ring=A if case == "fallback" else -1, **kw)
            b, before = a.clone(), a.clone()
            a.draw(logits, row_slot, lp=True)
            b.draw(logits, row_slot, lp=False)
            what = (V, case, row_slot)
            for k in STATE:                                                    # every st field as the plain entry writes it
                assert torch.equal(_bits(a.t[k]), _bits(b.t[k])), (k, what)
            for k in LPS:
                assert torch.equal(_bits(b.t[k]), _bits(before.t[k])), (k, what)
            drawn = {s: r for r, s in enumerate(row_slot) if 0 <= s < S and live[s]}
            assert drawn, what
            for s in range(S):
                if s not in drawn:                                             # every field of a skipped slot, sentinels included
                    for k in STATE + LPS:
                        assert torch.equal(_bits(a.t[k][s]), _bits(before.t[k][s])), (k, s, what)
                    continue
                r, n = drawn[s], N_OUT[s]
                id_ = int(a.t["ids"][s])
                assert int(a.t["step"][s]) == STEPS[s] + 1
                want = _want_lp(x_cpu[r], V, eos, barred, id_)
                tok, cum, end = a.t["tok_lp"][s].cpu(), a.t["cum_lp"][s].cpu(), a.t["end_lp"][s].cpu()
                if id_ != eos:                                                 # emitted
                    assert int(a.t["n_out"][s]) == n + 1 and int(a.t["seq"][s, n]) == id_, what
                    got = float(tok[n])
                    print(f"[cosy best-of] V={V} {case} slot {s}: id {id_} lp {got!r} fp64 {want!r}")
                    if case == "neg_inf":
                        assert want == NEG and got == NEG, (got, what)
                    else:
                        assert math.isfinite(want) and abs(got - want) <= TOL, (got, want, s, what)
                    other = torch.ones(LD, dtype=torch.bool)
                    other[n] = False
                    assert bool((tok[other] == SENT_TOK).all()), what          # only the emitted column is written
                    assert _bits(cum).item() == _bits(torch.tensor(SENT_CUM, dtype=torch.float64) + tok[n].double()).item(), what
                    assert float(end) == SENT_END, what
                else:                                                          # EOS drawn: end_lp, and nothing else
                    got = float(end)
                    print(f"[cosy best-of] V={V} {case} slot {s}: EOS end_lp {got!r} fp64 {want!r}")
                    assert (got == NEG and want == NEG) if case == "neg_inf" else abs(got - want) <= TOL, (got, want, s, what)
                    assert bool((tok == SENT_TOK).all()) and float(cum) == SENT_CUM and int(a.t["n_out"][s]) == n, what
                    assert int(a.t["live"][s]) == 0, what
                assert case != "eos_drawn" or id_ == eos, (id_, what)
                assert case != "eos_barred" or (id_ != eos and x_cpu[r, :V].argmax() == eos), (id_, what)
                if case == "top_k_1":
                    assert id_ == A, (id_, what)
                moved += id_ != A
        if case == "fallback":
            assert moved >= 1, "the ring held the argmax ten times and the draw never left it: the fallback was not taken"


def test_null_lp_is_refused_and_nothing_is_launched():
    V = 97
    x_cpu, A = _rows(V, "top_k_25")
    logits = x_cpu.to(DEV)
    a = _Slots(V)
    before = a.clone()
    st, lps = a.structs()
    fn = _lib.lib().rwkv7_ras_slots_lp_f32
    call = lambda lp: fn(4, V, logits.data_ptr(), logits.stride(0), None, ctypes.byref(st), lp, torch.cuda.current_stream().cuda_stream)
    assert call(None) == -1
    for k in LPS:
        bad = RasSlotLogprob(lps.tok_lp, lps.cum_lp, lps.end_lp)
        setattr(bad, k, None)
        assert call(ctypes.byref(bad)) == -1, k
    torch.cuda.synchronize()
    for k in STATE + LPS:
        assert torch.equal(_bits(a.t[k]), _bits(before.t[k])), k
    assert call(ctypes.byref(lps)) == 0                                        # the same call with every member: it draws
    torch.cuda.synchronize()
    assert a.t["step"].tolist() == [s + 1 for s in STEPS[:4]] + STEPS[4:] and bool((a.t["cum_lp"][:4] != SENT_CUM).all())


@pytest.mark.parametrize("V", [97, 1281, 6562, 8449])
@pytest.mark.parametrize("case", ["top_k_25", "eos_barred", "eos_drawn"])
def test_lp_bits_do_not_depend_on_row_slot_or_grid(V, case):
    """the same logits row, key, step and ring at two rows / slots of one call and in a call with another grid: the same bits"""
    x_cpu, A = _rows(V, case)
    x_cpu[3] = x_cpu[0]
    logits = x_cpu.to(DEV)
    same = dict(seeds=[42] * S, steps=[4] * S, n_out=[3] * S, **CASES[case])
    a = _Slots(V, **same)
    a.draw(logits, [5, 2, 1, 0], lp=True)                                      # row 0 -> slot 5, its copy (row 3) -> slot 0
    b = _Slots(V, **same)
    b.draw(logits[2:4], [0, 3], lp=True)                                       # two rows: the copy -> slot 3
    assert int(a.t["ids"][5]) == int(a.t["ids"][0]) == int(b.t["ids"][3])
    vals = lambda z, s: [_bits(z.t["tok_lp"][s, 3]).item(), _bits(z.t["cum_lp"][s]).item(), _bits(z.t["end_lp"][s]).item()]
    assert vals(a, 5) == vals(a, 0) == vals(b, 3)
    assert vals(a, 1) == vals(b, 0)                                            # row 2, in both calls
    k = "end_lp" if case == "eos_drawn" else "tok_lp"
    got = float(a.t[k][5] if case == "eos_drawn" else a.t[k][5, 3])
    assert math.isfinite(got) and got <= 0 and got not in (SENT_TOK, SENT_END)


def test_cum_lp_is_the_sequential_fp64_sum():
    """five consecutive calls; cum_lp equals the host's fp64 sum of the fp32 values in emission order, bit for bit"""
    V = 6562
    x_cpu, A = _rows(V, "top_k_25")
    a = _Slots(V, top_k=25, top_p=0.8)
    a.t["cum_lp"].zero_()
    g = torch.Generator().manual_seed(8)
    row_slot = [3, 5, 0, 1]
    for call in range(5):                                                      # other logits every step; EOS stays out of reach
        x = (x_cpu + torch.randn(4, V + PAD, generator=g)).clamp_(-30, 30)
        x[:, V - 1] = -30.0
        a.draw(x.to(DEV), row_slot, lp=True)
    tok, cum = a.t["tok_lp"].cpu(), a.t["cum_lp"].cpu()
    for s in row_slot:
        assert int(a.t["n_out"][s]) == N_OUT[s] + 5 and int(a.t["step"][s]) == STEPS[s] + 5
        want = torch.zeros((), dtype=torch.float64)
        for c in range(N_OUT[s], N_OUT[s] + 5):
            assert tok[s, c] != SENT_TOK and tok[s, c] < 0
            want = want + tok[s, c].double()
        assert _bits(cum[s]).item() == _bits(want).item(), (s, cum[s], want)
        assert float(a.t["end_lp"][s]) == SENT_END
    for s in (2, 4):                                                            # slots without a row
        assert float(cum[s]) == 0.0 and bool((tok[s] == SENT_TOK).all())


# ---------------------------------------------------------------------------------------------------------------- engine
def _model(L=2, seed=5, ST=96, vocab=300):
    """The tiny model of tests/test_continuous_cosy_gpu.py: 2 layers, hidden size 128, a head of 97 rows."""
    d = dict(hidden_size=128, num_hidden_layers=L, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=32)
    m = RWKV7CosyLM(RWKV7CosyConfig(vocab_size=vocab, speech_token_size=ST, **d)).init_weights(seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        m.lm_head.weight.copy_(torch.randn(m.lm_head.weight.shape, generator=g) * 0.05)
        m.lm_head.bias.copy_(torch.randn(m.lm_head.bias.shape, generator=g) * 0.1)
        for e in (m.llm_embedding, m.text_embedding, m.speech_embedding):
            e.weight.copy_(torch.randn(e.weight.shape, generator=g) * 0.5)
    return m.to(DEV).to(torch.bfloat16).eval()


@pytest.fixture(scope="module")
def small():
    """... with EOS at about a tenth of every step's mass (the random head alone gives it 1 / 97): utterances end on EOS soon after
    their bar, so end_lp and the early retirement are exercised by every engine test"""
    m = _model()
    with torch.no_grad():
        m.lm_head.bias[m.speech_token_size] += 2.5
    return m


@pytest.fixture(scope="module")
def prompts(small):
    g = torch.Generator().manual_seed(17)
    out = []
    for n_text, n_speech in ((9, 4), (30, 12), (17, 0)):
        text = torch.randint(0, 300, (n_text,), generator=g)
        speech = torch.randint(0, small.speech_token_size, (n_speech,), generator=g)
        out.append(cosy_request(small, text, None, speech).embeds)
    return out


KW = dict(slots=4, max_len_cap=40, check_every=2, prefill_buckets=(64, 128), prefill_max_seqs=4)
# the bounds leave room for EOS to end an utterance early and bar it at the start
REQS = [dict(sampling=25, seed=11, min_len=9, max_len=30, original_text_len=5), dict(sampling=1, seed=12, tau_r=0.5, min_len=0, max_len=40, original_text_len=0),
        dict(sampling=128, top_p=1.0, seed=13, min_len=40, max_len=33, original_text_len=0),
        dict(sampling=25, top_p=0.5, seed=(1 << 63) + 14, min_len=12, max_len=36, original_text_len=2),
        dict(sampling=25, seed=15, min_len=0, max_len=1, original_text_len=0), dict(sampling=128, top_p=1.0, seed=16, min_len=3, max_len=25, original_text_len=0)]


def _check_sum(eng, handles, out):
    """on every finished handle: cum_lp is the fp64 sum of tok_lp in emission order, bit for bit; a second take raises"""
    res = {}
    for h in handles:
        tok, cum, end = eng.take_logprobs(h)
        assert tok.dtype == torch.float32 and tok.shape == out[h].shape and cum.dtype == torch.float64 and cum.dim() == 0
        assert end.dtype == torch.float32 and end.dim() == 0 and float(end) <= 0
        want = torch.zeros((), dtype=torch.float64)
        for v in tok.cpu():
            want = want + v.double()
        assert _bits(cum.cpu()).item() == _bits(want).item(), (h, cum, want)
        assert bool((tok <= 0).all()) and bool(torch.isfinite(tok).all())
        with pytest.raises(KeyError):
            eng.take_logprobs(h)
        res[h] = (tok, cum, end)
    return res


@pytest.mark.parametrize("admission", ["eager", "graph"])
def test_logprobs_change_no_id(small, prompts, admission):
    """six requests through four slots: ids, n_out and the order in which the handles finish"""
    res = []
    for logprobs in (False, True):
        eng = ContinuousCosyDecoder(small, admission=admission, logprobs=logprobs, **KW)
        hs = [eng.submit(inputs_embeds=prompts[i % 3], **kw) for i, kw in enumerate(REQS)]
        out, order = {}, []
        while not eng.sched.idle:
            for h, ids in eng.step():
                assert h not in out
                out[h] = ids
                order.append(h)
        assert sorted(out) == hs
        res.append((out, order, eng.n_out.clone(), eng.step_t.clone(), eng.live.clone(), eng.replays))
        if logprobs:
            _check_sum(eng, hs, out)
        else:
            with pytest.raises(ValueError):
                eng.take_logprobs(hs[0])
    (a, order_a, *state_a, rep_a), (b, order_b, *state_b, rep_b) = res
    for h in a:
        assert torch.equal(a[h], b[h]), (h, a[h], b[h])
    assert order_a == order_b and rep_a == rep_b and all(torch.equal(x, y) for x, y in zip(state_a, state_b))
    assert a[2].numel() == 33 and a[4].numel() <= 1                            # EOS barred up to the limit; a budget of one draw


@pytest.mark.parametrize("admission", ["eager", "graph"])
def test_candidates_equal_stand_alone_requests(small, prompts, admission):
    """candidate i of submit_n(3, seed=s) is submit(seed=candidate_seed(s, i)) admitted alone (the same pack composition: the one
    prompt): ids and tok_lp bit for bit; the per-request tau_r reaches every candidate"""
    seed = (1 << 64) - 2                                                       # candidate 2 wraps to key 0
    kw = dict(inputs_embeds=prompts[1], sampling=25, top_p=0.9, tau_r=0.3, min_len=6, max_len=40, original_text_len=2)
    eng = ContinuousCosyDecoder(small, admission=admission, logprobs=True, **KW)
    group = eng.submit_n(3, seed=seed, **kw)
    assert len(group) == 3 and len(eng.sched.pending) == 3
    out = eng.run()
    lp = _check_sum(eng, group, out)
    assert all(out[h].numel() >= 4 for h in group)                             # EOS is barred for four draws
    solo = ContinuousCosyDecoder(small, admission=admission, logprobs=True, **KW)
    for i, h in enumerate(group):
        hs = solo.submit(seed=candidate_seed(seed, i), **kw)
        want = solo.run()[hs]
        assert torch.equal(out[h], want), (i, out[h], want)
        tok, cum, end = solo.take_logprobs(hs)
        assert torch.equal(_bits(lp[h][0]), _bits(tok)) and _bits(lp[h][1]).item() == _bits(cum).item()
        assert _bits(lp[h][2]).item() == _bits(end).item()
    assert len({tuple(out[h].tolist()) for h in group}) == 3, "three keys, one id sequence: the candidates did not draw on their own"
    assert eng.submit_n(1, seed=3, **kw) == [group[-1] + 1] and eng.sched.pending[0].group_size == 1   # n == 1 is submit


@pytest.mark.parametrize("admission", ["eager", "graph"])
@pytest.mark.parametrize("layout", ["one_and_three", "two_and_two"])
def test_sibling_rows_equal_the_first_candidates(small, prompts, admission, layout):
    """the admission is called directly and the rows are read before any replay; two prompts admitted together"""
    eng = ContinuousCosyDecoder(small, admission=admission, **KW)
    kw = dict(min_len=0, max_len=20, original_text_len=0)
    if layout == "one_and_three":
        eng.submit(inputs_embeds=prompts[0], seed=1, **kw)
        eng.submit_n(3, inputs_embeds=prompts[1], seed=2, **kw)
        same, heads = [(1, 2), (1, 3)], (0, 1)
    else:
        eng.submit_n(2, inputs_embeds=prompts[0], seed=1, **kw)
        eng.submit_n(2, inputs_embeds=prompts[1], seed=2, **kw)
        same, heads = [(0, 1), (2, 3)], (0, 2)
    eng._admit()
    torch.cuda.synchronize()
    assert sorted(eng.sched.busy) == [0, 1, 2, 3] and eng.replays == 0 and not eng._extra
    for st in eng.cache.states:
        for t in (st.att_x_prev, st.att_kv, st.ffn_x_prev):
            for a, b in same:
                assert torch.equal(_bits(t[a]), _bits(t[b])), (a, b, tuple(t.shape))
            assert not torch.equal(t[heads[0]], t[heads[1]]) and bool(t[heads[1]].ne(0).any())
    assert eng.step_t.tolist() == [1] * 4                                      # every candidate drew its first id


def test_engine_logprobs_equal_the_fp64_log_softmax_of_the_step_logits(small, prompts):
    """After the admission draw and after every replay: the value the draw wrote for each slot that was live is the fp64
    log-softmax (EOS left out while it is barred) of that row of the logits the draw read, at the id it drew.  take_logprobs then
    returns exactly the values read here, and cum_lp is their sequential fp64 sum."""
    eos, V = small.speech_token_size, small.speech_token_size + 1
    eng = ContinuousCosyDecoder(small, logprobs=True, **dict(KW, slots=3, check_every=1))
    hs = [eng.submit(inputs_embeds=prompts[i % 3], **kw) for i, kw in enumerate(REQS)]
    rec = {h: dict(tok=[], end=None) for h in hs}
    snap, checked = {}, [0, 0]

    def check(slot, h, row, step, n, tag):
        id_ = int(eng.ids[slot])
        barred = step < int(eng._par_host["n_ignore"][slot])
        want = _want_lp(row.float().cpu(), V, eos, barred, id_)
        if id_ != eos:
            assert int(eng.n_out[slot]) == n + 1, tag
            got = eng.tok_lp[slot, n].cpu()
            rec[h]["tok"].append(got)
            checked[0] += 1
        else:
            assert int(eng.n_out[slot]) == n and int(eng.live[slot]) == 0, tag
            got = rec[h]["end"] = eng.end_lp[slot].cpu()
            checked[1] += 1
        assert abs(float(got) - want) <= TOL, (tag, float(got), want)

    inner_draw, inner_admit = eng._admit_draw, eng._admit

    def admit_draw(took, logits, rows64, row_slot):
        logits = logits.contiguous()
        inner_draw(took, logits, rows64, row_slot)
        torch.cuda.synchronize()
        for r, (slot, req) in enumerate(took):
            check(slot, req.handle, logits[r], 0, 0, ("admission", req.handle))

    def admit():
        inner_admit()
        snap.update(live=eng.live.tolist(), step=eng.step_t.tolist(), n_out=eng.n_out.tolist(),
                    handle={s: r.handle for s, r in eng.sched.busy.items()})
    eng._admit_draw, eng._admit = admit_draw, admit

    out = {}
    while not eng.sched.idle:
        ran = eng.replays
        done = eng.step()
        if eng.replays != ran:                                                 # one replay: every slot that was live drew on its row
            assert eng.replays == ran + 1
            for slot, h in sorted(snap["handle"].items()):
                if snap["live"][slot]:
                    check(slot, h, eng.dstep.logits[slot], snap["step"][slot], snap["n_out"][slot], ("replay", eng.replays, slot, h))
        for h, ids in done:
            out[h] = ids
            tok, cum, end = eng.take_logprobs(h)
            assert tok.numel() == ids.numel() == len(rec[h]["tok"])
            want = torch.zeros((), dtype=torch.float64)
            for got, v in zip(tok.cpu(), rec[h]["tok"]):
                assert _bits(got).item() == _bits(v).item()
                want = want + v.double()
            assert _bits(cum.cpu()).item() == _bits(want).item(), (h, cum, want)
            assert _bits(end.cpu()).item() == _bits(rec[h]["end"] if rec[h]["end"] is not None else torch.zeros(())).item()
    assert sorted(out) == hs and checked[0] >= 50 and checked[1] >= 1, checked


def test_take_logprobs_contract(small, prompts):
    eng = ContinuousCosyDecoder(small, logprobs=True, **KW)
    for bad in (0, KW["slots"] + 1):
        with pytest.raises(ValueError):
            eng.submit_n(bad, inputs_embeds=prompts[0], **REQS[0])
    assert not eng.sched.pending and not eng._extra
    hs = [eng.submit(inputs_embeds=prompts[i % 3], **kw) for i, kw in enumerate(REQS[:3])]
    with pytest.raises(KeyError):
        eng.take_logprobs(hs[0])                                               # not finished yet
    out = eng.run()
    after_run = _check_sum(eng, hs, out)                                       # after run(); a second take raises KeyError
    with pytest.raises(KeyError):
        eng.take_logprobs(max(hs) + 10)                                        # unknown
    hs2 = [eng.submit(inputs_embeds=prompts[i % 3], **kw) for i, kw in enumerate(REQS[:3])]
    pieces, finished = {h: [] for h in hs2}, []
    for h, new, fin in eng.stream():
        pieces[h].append(new)
        if fin:
            finished.append(h)
    assert sorted(finished) == hs2
    streamed = {h: torch.cat(pieces[h]) for h in hs2}
    after_stream = _check_sum(eng, hs2, streamed)                              # after stream()
    for a, b in zip(hs, hs2):                                                  # the same requests: the same ids and values
        assert torch.equal(out[a], streamed[b]) and torch.equal(_bits(after_run[a][0]), _bits(after_stream[b][0]))
        assert _bits(after_run[a][1]).item() == _bits(after_stream[b][1]).item()
    plain = ContinuousCosyDecoder(small, **KW)
    h = plain.submit(inputs_embeds=prompts[0], **REQS[4])
    plain.run()
    with pytest.raises(ValueError):
        plain.take_logprobs(h)


def test_rank_candidates_over_a_finished_group(small, prompts):
    eng = ContinuousCosyDecoder(small, logprobs=True, **KW)
    hs = eng.submit_n(4, inputs_embeds=prompts[2], sampling=25, seed=21, min_len=5, max_len=40, original_text_len=0)
    out = eng.run()
    lp = _check_sum(eng, hs, out)
    cum, lens = [float(lp[h][1]) for h in hs], [out[h].numel() for h in hs]
    assert all(n >= 5 for n in lens)
    order = rank_candidates(torch.stack([lp[h][1] for h in hs]), lens)
    assert sorted(order) == [0, 1, 2, 3]
    mean = [c / n for c, n in zip(cum, lens)]
    assert all(mean[a] >= mean[b] for a, b in zip(order, order[1:]))
    by_sum = rank_candidates(cum, lens, length_normalize=False)
    assert sorted(by_sum) == [0, 1, 2, 3] and all(cum[a] >= cum[b] for a, b in zip(by_sum, by_sum[1:]))
    # the EOS draw counted in: the caller adds end_lp and one to the length of a candidate that ended on EOS
    with_end = rank_candidates([c + float(lp[h][2]) for c, h in zip(cum, hs)], [n + (float(lp[h][2]) != 0) for n, h in zip(lens, hs)])
    assert sorted(with_end) == [0, 1, 2, 3]
