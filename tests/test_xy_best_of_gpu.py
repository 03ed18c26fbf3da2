"""GPU (-m gpu): best-of-n in the XY engine.

Kernels: rwkv7_xy_slots_draw_lp_f32 / rwkv7_xy_slots_frame_lp_bf16 against the plain entries on cloned state (every field bit for
bit), ch_lp against an fp64 log_softmax on the CPU over each channel's allowed range, the frame accounting (which channels COUNT
once the frame rules have replaced drawn ids by forced ones) over a scripted flush, the buffers of skipped slots, an all -inf
channel, and placement independence -- for the three elements-per-thread classes of sampling_common.h and the first size of the
next class.

Engine: ContinuousXYDecoder(logprobs=True) changes no frame; candidate i of submit_n is the stand-alone request with
candidate_seed(seed, i); the siblings' cache rows equal the first candidate's right after admission; every frame_lp entry is the
fp64 log-softmax of the logits its step produced and cum_lp their sequential fp64 sum; groups wait whole; take_logprobs' contract;
rank_candidates.

Tolerance of the log-probabilities: TOL = 5e-5 absolute for logits with |x| <= 30, the bar of tests/test_best_of_gpu.py and
tests/test_cosy_best_of_gpu.py for the same arithmetic, argued there for sums of up to 8449 terms.  Here the largest class sums up
to 15 360 terms.  The argument restated for that count: the value is (x[id] - m) - log(sum_j exp(x[j] - m)) in fp32.
  * x[id] - m: one subtraction at magnitude <= 60, half an ulp of 64: 3.8e-6.
  * the exp-sum: every term is positive, so the error of the sum is bounded by the ADDITION DEPTH, not by the number of terms: a
    thread adds its 60 elements (33 in the class the 8449-term bar was argued for), the wave butterfly adds 6 levels and the four
    waves 2 more -- 68 roundings of 6e-8 relative each: 4.1e-6 of the sum, against 2.5e-6 at depth 41.  A term's own error
    (the exponent's product with log2(e) rounded at magnitude <= 87, then the hardware exp2) is below 1e-6 relative for the terms
    within 16 of the maximum, which carry all but e^-16 of the sum.  Relative 5.1e-6 of the sum is absolute 5.1e-6 of its log.
  * the log: the sum lies in [1, 15360] (the maximum is one of the terms -- the XY draw has no barred id, unlike the Cosy draw,
    so the sum is never as small as exp(-60)): hardware log2 within an ulp at magnitude <= 14, times ln 2: 1e-6.
  * the final subtraction at magnitude <= 60 + ln 15360 = 69.7 < 128, half an ulp: 7.6e-6 at most.
Together below 1.8e-5: the argument holds at 15 360 terms and the bar stays 5e-5 for every class.  The measured maxima are printed
and recorded in profiles/xy_best_of_parity.txt."""
import ctypes
import math

import pytest
import torch

from rwkvtts_amd import _lib
from rwkvtts_amd.continuous import candidate_seed, rank_candidates
from rwkvtts_amd.continuous_xy import (ContinuousXYDecoder, XYSlotLogprob, XYSlotState, head_column_map, xy_slots_draw,
                                       xy_slots_frame)
from rwkvtts_amd.xy_llm import RWKV7XYConfig, RWKV7XYLM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5
NEG = float("-inf")
S, D, LD = 6, 64, 12
LAYOUT = [4, -1, 6, 2]    # 4 rows over 6 slots: slot 2 is not live, one row has no slot, one names a slot past the end
LIVE = [1, 1, 0, 1, 1, 1]
STEPS = [3, 0, 9, 5, 1, 7]
# slot 0 greedy, 1 sampled from the whole distribution (top_k = 0), 2 dead, 3 / 4 / 5 top-k with and without top-p
PARAMS = [dict(do_sample=0), dict(do_sample=1, top_k=0, temperature=1.3), dict(do_sample=1, top_k=5),
          dict(do_sample=1, top_k=50, top_p=0.9, temperature=0.8), dict(do_sample=1, top_k=7, temperature=0.7),
          dict(do_sample=1, top_k=64, top_p=0.5)]
SENT_CH, SENT_FR, SENT_CUM, SENT_N = 777.0, -555.0, 5.5, 1234
STATE = ("step", "needs", "live", "nt", "row", "seq", "x")
LPS = ("ch_lp", "frame_lp", "cum_lp", "n_lp")
DOMAINS = [97, 1280, 1281, 8448, 8449, 15360]   # each elements-per-thread class (5, 33, 60 x 256) and the first size of the next


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else \
        t.view(torch.int64) if t.dtype == torch.float64 else t


# ---------------------------------------------------------------------------------------------------------------- kernels
class _Slots:
    """Device state of S slots of C channels.  Channel 0's allowed range [lo0, lo0 + doms[0]) starts above 0 (allow_lo > 0) and is
    the audio range unless `shift` says otherwise; a logits row holds the allowed parts back to back."""

    def __init__(self, doms, live=LIVE, steps=STEPS, seeds=None, params=PARAMS, lo0=37, shift=None, eos=None, like=None):
        self.C, self.doms, self.lo0 = len(doms), list(doms), lo0
        self.allow = [(lo0, lo0 + doms[0])] + [(0, d) for d in doms[1:]]
        self.col0 = [sum(doms[:c]) for c in range(self.C)]
        self.width, self.max_domain = sum(doms), max(doms)
        self.shift, self.sv, self.eos = lo0 if shift is None else shift, doms[0] if shift is None else lo0 + doms[0] - shift, eos
        self.pad = min(doms[1:]) - 1
        if like is not None:
            self.t, self.tables, self.const = {k: v.clone() for k, v in like.t.items()}, like.tables, like.const
            return
        i32, l64 = dict(dtype=torch.int32, device=DEV), dict(dtype=torch.int64, device=DEV)
        g = torch.Generator().manual_seed(99)
        seeds = [0x1234567 + 977 * s + ((1 << 63) if s == 1 else 0) for s in range(S)] if seeds is None else seeds
        par = lambda k, d, dt: torch.tensor([p.get(k, d) for p in params], dtype=dt, device=DEV)
        C = self.C
        self.t = dict(step=torch.tensor(list(steps), **l64), needs=torch.full((S,), -1, **l64),
                      live=torch.tensor(list(live), dtype=torch.uint8, device=DEV), nt=torch.full((S, C), -5, **l64),
                      row=torch.full((S, C), -3, **l64), seq=torch.full((S, LD, C), -7, **l64),
                      x=torch.randn(S, D, generator=g).to(DEV, torch.bfloat16),
                      ch_lp=torch.full((S, C), SENT_CH, dtype=torch.float32, device=DEV),
                      frame_lp=torch.full((S, LD, C), SENT_FR, dtype=torch.float32, device=DEV),
                      cum_lp=torch.full((S,), SENT_CUM, dtype=torch.float64, device=DEV), n_lp=torch.full((S,), SENT_N, **l64))
        self.const = dict(limit=torch.full((S,), 100, **l64),
                          seed=torch.tensor([v - (1 << 64) if v >= 1 << 63 else v for v in seeds], **l64),
                          inv_temp=(1.0 / par("temperature", 1.0, torch.float32)), top_k=par("top_k", 0, torch.int32),
                          top_p=par("top_p", 1.0, torch.float32), do_sample=par("do_sample", 0, torch.uint8),
                          seg_off=torch.tensor([c - a[0] for c, a in zip(self.col0, self.allow)], **i32),
                          seg_len=torch.tensor([a[1] for a in self.allow], **i32),
                          allow_lo=torch.tensor([a[0] for a in self.allow], **i32), allow_hi=torch.tensor([a[1] for a in self.allow], **i32),
                          eos_list=torch.tensor([0 if eos is None else eos], **l64))
        self.tables = [torch.randn(a[1], D, generator=g).to(DEV, torch.bfloat16) for a in self.allow]

    def clone(self):
        return _Slots(self.doms, lo0=self.lo0, shift=self.shift, eos=self.eos, like=self)

    def structs(self):
        t, k, st = self.t, self.const, XYSlotState()
        st.step, st.limit, st.seed, st.inv_temp = t["step"].data_ptr(), k["limit"].data_ptr(), k["seed"].data_ptr(), k["inv_temp"].data_ptr()
        st.top_k, st.top_p, st.do_sample, st.live = k["top_k"].data_ptr(), k["top_p"].data_ptr(), k["do_sample"].data_ptr(), t["live"].data_ptr()
        st.needs, st.nt, st.row, st.seq, st.seq_ld = t["needs"].data_ptr(), t["nt"].data_ptr(), t["row"].data_ptr(), t["seq"].data_ptr(), LD
        for c, tb in enumerate(self.tables):
            st.tables[c] = tb.data_ptr()
        st.x, st.D, st.C, st.slots, st.top_k_max = t["x"].data_ptr(), D, self.C, S, 64
        st.text_shift, st.speech_vocab, st.pad, st.eos0 = self.shift, self.sv, self.pad, -1 if self.eos is None else self.eos
        st.eos_list, st.n_eos, st.reference_termination = (None if self.eos is None else k["eos_list"].data_ptr()), int(self.eos is not None), 0
        return st, XYSlotLogprob(t["ch_lp"].data_ptr(), t["frame_lp"].data_ptr(), t["cum_lp"].data_ptr(), t["n_lp"].data_ptr())

    def draw(self, logits, row_slot, lp):
        st, lps = self.structs()
        rs = None if row_slot is None else torch.tensor(row_slot, dtype=torch.int32, device=DEV)
        k = self.const
        xy_slots_draw(logits, st, k["seg_off"], k["seg_len"], k["allow_lo"], k["allow_hi"], self.max_domain, rs, lps if lp else None)
        torch.cuda.synchronize()

    def frame(self, rows, row_slot, lp):
        st, lps = self.structs()
        rs = None if row_slot is None else torch.tensor(row_slot, dtype=torch.int32, device=DEV)
        xy_slots_frame(rows, st, torch.device(DEV), rs, lps if lp else None)
        torch.cuda.synchronize()

    def want_lp(self, row, c, id_):
        """fp64 log_softmax over channel c's allowed range of one CPU logits row, at the drawn id; -inf for a range without a finite logit"""
        x = row[self.col0[c]:self.col0[c] + self.doms[c]].double()
        if torch.isneginf(x).all():
            return NEG
        j = id_ - self.allow[c][0]
        assert 0 <= j < self.doms[c] and x[j] > NEG, "the draw chose an id outside the set it may use"
        return float(torch.log_softmax(x, 0)[j])


def _doms(C, dom):
    """C per-channel domains with the largest = dom (it decides the elements-per-thread class of the launch), sizes that are no
    multiple of the 256 threads, a tiny one, and a second channel of the full size"""
    return ([dom, max(dom // 2 + 1, 2), 5, dom, max(dom - 255, 2), 33, max(dom // 3, 2), 2])[:C]


def _rows(z, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, z.width, generator=g) * 4).clamp_(-30, 30)


@pytest.mark.parametrize("dom", DOMAINS)
@pytest.mark.parametrize("C", [3, 8])
def test_lp_entries_equal_the_plain_entries_and_an_fp64_log_softmax(C, dom):
    z0 = _Slots(_doms(C, dom))
    x_cpu = _rows(z0, 4, dom + C)
    logits = x_cpu.to(DEV)
    # the prescribed layout with each row in turn as the one that is drawn, then all four rows on permuted live slots
    layouts = [(LAYOUT[-r:] + LAYOUT[:-r], LIVE) for r in range(4)] + [([3, 5, 0, 1], LIVE)]
    worst = 0.0
    for row_slot, live in layouts:
        a = z0.clone()
        b, before = a.clone(), a.clone()
        a.draw(logits, row_slot, lp=True)
        b.draw(logits, row_slot, lp=False)
        what = (C, dom, row_slot)
        drawn = {s: r for r, s in enumerate(row_slot) if 0 <= s < S and live[s]}
        assert drawn, what
        assert torch.equal(a.t["nt"], b.t["nt"]), what                        # 1. the drawn ids, bit for bit
        for k in STATE + LPS:                                                 # the draw writes nt and ch_lp, and nothing else
            if k not in ("nt", "ch_lp"):
                assert torch.equal(_bits(a.t[k]), _bits(before.t[k])), (k, what)
        for k in LPS:
            assert torch.equal(_bits(b.t[k]), _bits(before.t[k])), (k, what)   # the plain entry knows nothing of them
        ch = a.t["ch_lp"].cpu()
        for s in range(S):
            if s not in drawn:                                                # 4. skipped: sentinels and all
                assert torch.equal(a.t["nt"][s], before.t["nt"][s]) and bool((ch[s] == SENT_CH).all()), (s, what)
                continue
            for c in range(C):                                                # 2. fp64 parity
                id_ = int(a.t["nt"][s, c])
                got, want = float(ch[s, c]), a.want_lp(x_cpu[drawn[s]], c, id_)
                assert math.isfinite(want) and abs(got - want) <= TOL, (got, want, s, c, what)
                worst = max(worst, abs(got - want))
        ch_after = a.t["ch_lp"].clone()
        a.frame(4, row_slot, lp=True)
        b.frame(4, row_slot, lp=False)
        for k in STATE:                                                       # 1. every state field after the frame, bit for bit
            assert torch.equal(_bits(a.t[k]), _bits(b.t[k])), (k, what)
        assert torch.equal(_bits(a.t["ch_lp"]), _bits(ch_after)), what         # the frame reads ch_lp
        fr, cum, n = a.t["frame_lp"].cpu(), a.t["cum_lp"].cpu(), a.t["n_lp"].cpu()
        for s in range(S):
            if s not in drawn:                                                # 4. every field of a skipped slot, sentinels included
                for k in STATE + LPS:
                    assert torch.equal(_bits(a.t[k][s]), _bits(before.t[k][s])), (k, s, what)
                continue
            # channel 0 stays in the audio range: no flush, every channel counts
            assert torch.equal(_bits(fr[s, STEPS[s]]), _bits(ch[s])), (s, what)
            other = torch.ones(LD, dtype=torch.bool)
            other[STEPS[s]] = False
            assert bool((fr[s, other] == SENT_FR).all()), (s, what)           # only the frame's row is written
            want = torch.tensor(SENT_CUM, dtype=torch.float64)
            for c in range(C):
                want = want + ch[s, c].double()
            assert _bits(cum[s]).item() == _bits(want).item() and int(n[s]) == SENT_N + C, (s, what)
            assert int(a.t["step"][s]) == STEPS[s] + 1
    print(f"[xy best-of parity] C={C} max_domain={dom}: max |ch_lp - fp64 log_softmax| = {worst:.3e} (TOL {TOL:.0e})")


@pytest.mark.parametrize("C", [3, 8])
def test_frame_accounting_over_a_scripted_flush(C):
    """One greedy slot, C + 2 frames and one more launch.  Channel 0 may draw ONE non-audio id (the first of its range); a +30 logit
    on it at frame F0 = 2 starts the flush.  From the counting rule: frames 0 .. F0 count every channel -- frame F0 too, although
    eos0 is written over its channel 0 --; frame F0 + j (j >= 1) has channel 0 forced and counts channel i iff i > j; frame
    F0 + C - 1 counts nothing and ends the slot.  At frame 0 channel 1 draws the pad id itself: it counts (ids are never compared)."""
    SV, F0, s0 = 40, 2, 3
    z = _Slots([SV + 1] + [SV] * (C - 1), live=[0, 0, 0, 1, 0, 0], steps=[0] * S, params=[dict(do_sample=0)] * S, lo0=9, shift=10, eos=15)
    assert z.sv == SV and z.pad == SV - 1 and z.allow[0] == (9, 50)
    z.t["cum_lp"].zero_()
    z.t["n_lp"].zero_()
    g = torch.Generator().manual_seed(C)
    frames = F0 + C
    assert frames >= C + 2 and frames <= LD
    exp_fr, cum, n = [], torch.zeros((), dtype=torch.float64), 0
    for f in range(frames + 1):
        x = (torch.randn(1, z.width, generator=g) * 4).clamp_(-30, 30)
        x[0, 0] = 30.0 if f == F0 else -30.0                                   # column 0: the non-audio id 9 of channel 0
        x[0, 15 - 9] = -30.0                                                   # the EOS id is never drawn: only the flush writes it
        if f == 0:
            x[0, z.col0[1] + z.pad] = 30.0                                     # channel 1 draws the pad id of its own accord
        before = z.clone()
        z.draw(x.to(DEV), [s0], lp=True)
        z.frame(1, [s0], lp=True)
        if f == frames:                                                        # the slot has ended: one more launch writes nothing
            for k in STATE + LPS:
                assert torch.equal(_bits(z.t[k]), _bits(before.t[k])), k
            break
        nt, ch = z.t["nt"][s0].tolist(), z.t["ch_lp"][s0].cpu()
        for c in range(C):
            assert abs(float(ch[c]) - z.want_lp(x[0], c, nt[c])) <= TOL, (f, c)
        j = f - F0
        counts = [True] * C if j <= 0 else [False] + [i > j for i in range(1, C)]
        row = z.t["seq"][s0, f].tolist()
        assert (nt[0] == row[0] != 15) if f < F0 else (row[0] == 15 and (f > F0 or nt[0] == 9)), (f, nt, row)   # eos0 over channel 0 from F0 on
        assert row[1:] == [nt[i] if counts[i] else z.pad for i in range(1, C)], (f, nt, row)
        if f == 0:
            assert nt[1] == z.pad and counts[1]
        if f == F0:
            assert counts[0] and row[0] == 15 and float(ch[0]) > -1e-3        # the flush start: channel 0's free choice counts
        got = z.t["frame_lp"][s0, f].cpu()
        for c in range(C):
            if counts[c]:
                assert _bits(got[c]).item() == _bits(ch[c]).item(), (f, c)
                cum, n = cum + ch[c].double(), n + 1
            else:
                assert _bits(got[c]).item() == 0, (f, c, float(got[c]))        # exactly +0.0
        exp_fr.append(counts)
        assert _bits(z.t["cum_lp"][s0].cpu()).item() == _bits(cum).item() and int(z.t["n_lp"][s0]) == n, (f, cum, n)
        assert int(z.t["live"][s0]) == int(f < frames - 1) and int(z.t["step"][s0]) == f + 1, f
    assert exp_fr[F0] == [True] * C and not any(exp_fr[-1]) and n == (F0 + 1) * C + sum(C - 1 - j for j in range(1, C))
    assert bool((z.t["frame_lp"][s0, frames:] == SENT_FR).all())
    for s in range(S):                                                         # 4. the other slots never moved
        if s != s0:
            assert bool((z.t["ch_lp"][s] == SENT_CH).all()) and bool((z.t["frame_lp"][s] == SENT_FR).all())
            assert float(z.t["cum_lp"][s]) == 0.0 and int(z.t["n_lp"][s]) == 0 and bool((z.t["nt"][s] == -5).all())


def test_an_all_neg_inf_channel_gives_neg_inf_not_nan():
    z = _Slots(_doms(3, 97))
    x = _rows(z, 4, 5)
    x[:, z.col0[1]:z.col0[1] + z.doms[1]] = NEG
    row_slot = [3, 5, 0, 1]
    z.t["cum_lp"].zero_()
    z.draw(x.to(DEV), row_slot, lp=True)
    z.frame(4, row_slot, lp=True)
    ch, fr, cum = z.t["ch_lp"].cpu(), z.t["frame_lp"].cpu(), z.t["cum_lp"].cpu()
    assert not bool(torch.isnan(ch).any()) and not bool(torch.isnan(fr).any()) and not bool(torch.isnan(cum).any())
    for s in row_slot:
        assert float(ch[s, 1]) == NEG and float(fr[s, STEPS[s], 1]) == NEG and float(cum[s]) == NEG
        assert math.isfinite(float(ch[s, 0])) and math.isfinite(float(ch[s, 2]))
        assert 0 <= int(z.t["nt"][s, 1]) < z.doms[1]                           # the fall-back id is inside the range


def test_null_lp_is_refused_and_nothing_is_launched():
    z = _Slots(_doms(3, 97))
    logits = _rows(z, S, 1).to(DEV)
    before = z.clone()
    st, lps = z.structs()
    k, lib, stream = z.const, _lib.lib(), torch.cuda.current_stream().cuda_stream
    draw = lambda lp: lib.rwkv7_xy_slots_draw_lp_f32(S, logits.data_ptr(), logits.stride(0), None, k["seg_off"].data_ptr(), k["seg_len"].data_ptr(),
                                                    k["allow_lo"].data_ptr(), k["allow_hi"].data_ptr(), z.max_domain, ctypes.byref(st), lp, stream)
    frame = lambda lp: lib.rwkv7_xy_slots_frame_lp_bf16(S, None, ctypes.byref(st), lp, stream)
    assert draw(None) == -1 and frame(None) == -1
    for name in LPS:
        bad = XYSlotLogprob(lps.ch_lp, lps.frame_lp, lps.cum_lp, lps.n_lp)
        setattr(bad, name, None)
        assert draw(ctypes.byref(bad)) == -1 and frame(ctypes.byref(bad)) == -1, name
    torch.cuda.synchronize()
    for name in STATE + LPS:
        assert torch.equal(_bits(z.t[name]), _bits(before.t[name])), name
    assert draw(ctypes.byref(lps)) == 0 and frame(ctypes.byref(lps)) == 0      # the same calls with every member: a frame
    torch.cuda.synchronize()
    assert z.t["step"].tolist() == [s + l for s, l in zip(STEPS, LIVE)] and z.t["n_lp"].tolist() == [SENT_N + 3 * l for l in LIVE]


@pytest.mark.parametrize("dom", [97, 1281, 8449])
def test_lp_bits_do_not_depend_on_row_slot_or_grid(dom):
    """the same logits row, key, step and parameters at two rows / slots of one launch and in a launch of another size: the same bits"""
    C = 3
    same = dict(seeds=[42] * S, steps=[4] * S, params=[PARAMS[3]] * S, live=[1] * S)
    a = _Slots(_doms(C, dom), **same)
    x = _rows(a, 4, dom)
    x[3] = x[0]
    logits = x.to(DEV)
    a.draw(logits, [5, 2, 1, 0], lp=True)                                      # row 0 -> slot 5, its copy (row 3) -> slot 0
    a.frame(4, [5, 2, 1, 0], lp=True)
    b = _Slots(_doms(C, dom), **same)
    b.draw(logits[2:4], [0, 3], lp=True)                                       # two rows: the copy -> slot 3
    b.frame(2, [0, 3], lp=True)
    assert torch.equal(a.t["nt"][5], a.t["nt"][0]) and torch.equal(a.t["nt"][5], b.t["nt"][3])
    vals = lambda z, s: _bits(z.t["ch_lp"][s]).tolist() + _bits(z.t["frame_lp"][s, 4]).tolist() + [_bits(z.t["cum_lp"][s]).item(), int(z.t["n_lp"][s])]
    assert vals(a, 5) == vals(a, 0) == vals(b, 3)
    assert vals(a, 1) == vals(b, 0)                                            # row 2, in both launches
    got = a.t["ch_lp"][5]
    assert bool(torch.isfinite(got).all()) and bool((got <= 0).all()) and bool((got != SENT_CH).all())


# ---------------------------------------------------------------------------------------------------------------- engine
def _model(L=2, seed=5, V0=300, SV=64, shift=200, C=4):
    """The tiny model of tests/test_continuous_xy_gpu.py, built the same way."""
    d = dict(hidden_size=128, num_hidden_layers=L, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=32)
    cfg = RWKV7XYConfig(vocab_size=V0, speech_vocab_size=SV, num_channels=C, text_shift_size=shift, **d)
    m = RWKV7XYLM(cfg).init_weights(seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for h in m.heads:
            h.weight.copy_(torch.randn(h.weight.shape, generator=g) * 0.05)
            h.bias.copy_(torch.randn(h.bias.shape, generator=g) * 0.1)
        for e in m.embs:
            e.weight.copy_(torch.randn(e.weight.shape, generator=g) * 0.5)
    m.zero_embs()
    return m.to(DEV).to(torch.bfloat16).eval()


@pytest.fixture(scope="module")
def small():
    """... with EOS at about a fifteenth of channel 0's mass at every frame (the random head alone gives it 1 / 64): some requests
    end on EOS well inside their budget, so the early retirement and the slot reuse are part of every engine test"""
    m = _model()
    with torch.no_grad():
        m.heads[0].bias[EOS] += 1.5
    return m


@pytest.fixture(scope="module")
def prompts(small):
    cfg, g, out = small.config, torch.Generator().manual_seed(17), []
    for t in (9, 41, 17):
        ch0 = torch.randint(0, cfg.text_shift_size + cfg.speech_vocab_size, (t, 1), generator=g)
        out.append(torch.cat([ch0, torch.randint(0, cfg.speech_vocab_size - 1, (t, cfg.num_channels - 1), generator=g)], 1).to(DEV))
    return out


EOS = 200 + 7   # an audio id of channel 0: about one frame in 64 draws it, so some requests end early and slots are reused
KW = dict(slots=4, max_new_frames_cap=40, check_every=2, prefill_buckets=(64, 128), prefill_max_seqs=4, eos_token_id=EOS)
REQS = [dict(max_new_frames=30, do_sample=True, top_k=50, top_p=0.95, temperature=0.8, seed=11), dict(max_new_frames=40),
        dict(max_new_frames=33, do_sample=True, seed=12), dict(max_new_frames=25, do_sample=True, top_k=5, temperature=1.3, seed=13),
        dict(max_new_frames=1, do_sample=True, top_k=64, top_p=0.5, seed=(1 << 63) + 14), dict(max_new_frames=36, do_sample=True, top_k=64, seed=15)]


def _check_sum(eng, handles, out):
    """on every finished handle: frame_lp [n, C] without a forced entry (channel 0 cannot leave the audio range in the engine), cum_lp
    its sequential fp64 sum in (frame, channel) order bit for bit, n_lp = n * C; a second take raises"""
    res = {}
    for h in handles:
        fr, cum, n = eng.take_logprobs(h)
        assert fr.dtype == torch.float32 and fr.shape == out[h].shape and cum.dtype == torch.float64 and cum.dim() == 0
        assert isinstance(n, int) and n == fr.numel()
        want = torch.zeros((), dtype=torch.float64)
        for v in fr.cpu().reshape(-1):
            want = want + v.double()
        assert _bits(cum.cpu()).item() == _bits(want).item(), (h, cum, want)
        assert bool((fr < 0).all()) and bool(torch.isfinite(fr).all())
        with pytest.raises(KeyError):
            eng.take_logprobs(h)
        res[h] = (fr, cum, n)
    return res


@pytest.mark.parametrize("admission", ["eager", "graph"])
def test_logprobs_change_no_frame(small, prompts, admission):
    """six requests through four slots: frames, counters and the order in which the handles finish"""
    res = []
    for logprobs in (False, True):
        eng = ContinuousXYDecoder(small, admission=admission, logprobs=logprobs, **KW)
        hs = [eng.submit(prompts[i % 3], **kw) for i, kw in enumerate(REQS)]
        out, order = {}, []
        while not eng.sched.idle:
            for h, frames in eng.step():
                assert h not in out
                out[h] = frames
                order.append(h)
        assert sorted(out) == hs
        res.append((out, order, eng.step_t.clone(), eng.live.clone(), eng.needs.clone(), eng.replays))
        if logprobs:
            _check_sum(eng, hs, out)
        else:
            with pytest.raises(ValueError):
                eng.take_logprobs(hs[0])
    (a, order_a, *state_a, rep_a), (b, order_b, *state_b, rep_b) = res
    for h in a:
        assert torch.equal(a[h], b[h]), (h, a[h], b[h])
    assert order_a == order_b and rep_a == rep_b and all(torch.equal(x, y) for x, y in zip(state_a, state_b))
    assert a[4].shape == (1, 4) and any(int(f[-1, 0]) == EOS for f in a.values()), "no request ended on EOS"


@pytest.mark.parametrize("admission", ["eager", "graph"])
def test_candidates_equal_stand_alone_requests(small, prompts, admission):
    """candidate i of submit_n(4, seed=s) is submit(seed=candidate_seed(s, i)) admitted alone (the same pack composition: the one
    prompt): frames and frame_lp bit for bit"""
    seed = (1 << 64) - 2                                                       # candidate 2 wraps to key 0
    kw = dict(max_new_frames=24, do_sample=True, top_k=50, top_p=0.95, temperature=0.8)
    eng = ContinuousXYDecoder(small, admission=admission, logprobs=True, **KW)
    group = eng.submit_n(4, prompts[1], seed=seed, **kw)
    assert len(group) == 4 and len(eng.sched.pending) == 4
    out = eng.run()
    lp = _check_sum(eng, group, out)
    solo = ContinuousXYDecoder(small, admission=admission, logprobs=True, **KW)
    for i, h in enumerate(group):
        hs = solo.submit(prompts[1], seed=candidate_seed(seed, i), **kw)
        want = solo.run()[hs]
        assert torch.equal(out[h], want), (i, out[h], want)
        fr, cum, n = solo.take_logprobs(hs)
        assert torch.equal(_bits(lp[h][0]), _bits(fr)) and _bits(lp[h][1]).item() == _bits(cum).item() and lp[h][2] == n
    assert len({tuple(out[h].reshape(-1).tolist()) for h in group}) == 4, "four keys, one frame sequence: the candidates did not draw on their own"
    assert eng.submit_n(1, prompts[1], seed=3, **kw) == [group[-1] + 1] and eng.sched.pending[0].group_size == 1   # n == 1 is submit


@pytest.mark.parametrize("admission", ["eager", "graph"])
@pytest.mark.parametrize("layout", ["one_and_three", "two_and_two"])
def test_sibling_rows_equal_the_first_candidates(small, prompts, admission, layout):
    """the admission is called directly and the rows are read before any replay; two prompts admitted together"""
    eng = ContinuousXYDecoder(small, admission=admission, **KW)
    kw = dict(max_new_frames=20, do_sample=True)
    if layout == "one_and_three":
        eng.submit(prompts[0], seed=1, **kw)
        eng.submit_n(3, prompts[1], seed=2, **kw)
        same, heads = [(1, 2), (1, 3)], (0, 1)
    else:
        eng.submit_n(2, prompts[0], seed=1, **kw)
        eng.submit_n(2, prompts[1], seed=2, **kw)
        same, heads = [(0, 1), (2, 3)], (0, 2)
    eng._admit()
    torch.cuda.synchronize()
    assert sorted(eng.sched.busy) == [0, 1, 2, 3] and eng.replays == 0
    for st in eng.cache.states:
        for t in (st.att_x_prev, st.att_kv, st.ffn_x_prev):
            for a, b in same:
                assert torch.equal(_bits(t[a]), _bits(t[b])), (a, b, tuple(t.shape))
            assert not torch.equal(t[heads[0]], t[heads[1]]) and bool(t[heads[1]].ne(0).any())
    assert eng.step_t.tolist() == [1] * 4                                      # every candidate drew its first frame
    assert len({tuple(eng.seq[s, 0].tolist()) for s in range(4)}) >= 3         # ... with its own key


def test_engine_logprobs_equal_the_fp64_log_softmax_of_the_step_logits(small, prompts):
    """After the admission draw and after every replay: the row of frame_lp written for each slot that was live is, channel by
    channel, the fp64 log-softmax of the logits the draw read, at the ids of the frame (no flush in the engine: the frame's ids are
    the drawn ones).  take_logprobs then returns exactly the values read here, and cum_lp is their sequential fp64 sum."""
    cfg = small.config
    cm = head_column_map(cfg.vocab_size, cfg.speech_vocab_size, cfg.num_channels, cfg.text_shift_size)
    C, SV = cfg.num_channels, cfg.speech_vocab_size
    eng = ContinuousXYDecoder(small, logprobs=True, **dict(KW, slots=3, check_every=1))
    hs = [eng.submit(prompts[i % 3], **kw) for i, kw in enumerate(REQS)]
    rec = {h: [] for h in hs}
    snap, checked = {}, [0]

    def check(slot, h, row, step, tag):
        row, ids, got = row.float().cpu(), eng.seq[slot, step].tolist(), eng.frame_lp[slot, step].cpu()
        for c in range(C):
            want = float(torch.log_softmax(row[cm.col0[c]:cm.col0[c] + SV].double(), 0)[ids[c] - cm.allow[c][0]])
            assert abs(float(got[c]) - want) <= TOL, (tag, c, float(got[c]), want)
        rec[h].append(got)
        checked[0] += C

    inner_draw, inner_admit = eng._admit_draw, eng._admit

    def admit_draw(took, logits, rows64, row_slot):
        logits = logits.contiguous()
        inner_draw(took, logits, rows64, row_slot)
        torch.cuda.synchronize()
        for r, (slot, req) in enumerate(took):
            check(slot, req.handle, logits[r], 0, ("admission", req.handle))

    def admit():
        inner_admit()
        snap.update(live=eng.live.tolist(), step=eng.step_t.tolist(), handle={s: r.handle for s, r in eng.sched.busy.items()})
    eng._admit_draw, eng._admit = admit_draw, admit

    out = {}
    while not eng.sched.idle:
        ran = eng.replays
        done = eng.step()
        if eng.replays != ran:                                                 # one replay: every slot that was live drew on its row
            assert eng.replays == ran + 1
            for slot, h in sorted(snap["handle"].items()):
                if snap["live"][slot]:
                    check(slot, h, eng.dstep.logits[slot], snap["step"][slot], ("replay", eng.replays, slot, h))
        for h, frames in done:
            out[h] = frames
            fr, cum, n = eng.take_logprobs(h)
            assert fr.shape == frames.shape and len(rec[h]) == frames.shape[0] and n == frames.numel()
            want = torch.zeros((), dtype=torch.float64)
            for got, v in zip(fr.cpu(), rec[h]):
                assert torch.equal(_bits(got), _bits(v))
                for e in v:
                    want = want + e.double()
            assert _bits(cum.cpu()).item() == _bits(want).item(), (h, cum, want)
    assert sorted(out) == hs and checked[0] >= 100, checked


def test_groups_wait_whole_and_the_take_logprobs_contract(small, prompts):
    eng = ContinuousXYDecoder(small, logprobs=True, **KW)
    for bad in (0, KW["slots"] + 1):
        with pytest.raises(ValueError, match="slots"):
            eng.submit_n(bad, prompts[0], seed=1)
    with pytest.raises(ValueError, match="seed"):
        eng.submit_n(2, prompts[0], do_sample=True)
    assert not eng.sched.pending
    busy = [eng.submit(prompts[i], max_new_frames=4 + 2 * i, do_sample=True, seed=i) for i in range(2)]
    group = eng.submit_n(3, prompts[2], max_new_frames=6, do_sample=True, top_k=20, seed=5)
    late = eng.submit(prompts[0], max_new_frames=3, seed=9)
    with pytest.raises(KeyError):
        eng.take_logprobs(busy[0])                                             # not finished yet
    admissions, inner_draw = [], eng._admit_draw

    def admit_draw(took, *args):
        admissions.append([r.handle for _, r in took])
        inner_draw(took, *args)
    eng._admit_draw = admit_draw
    out = dict(eng.step())                                                     # two free slots: the group of 3 waits, `late` behind it
    assert admissions == [busy] and [r.handle for r in eng.sched.pending] == group + [late]
    while not eng.sched.idle:
        out.update(eng.step())
    assert sorted(out) == sorted(busy + group + [late])
    at = {h: i for i, a in enumerate(admissions) for h in a}
    assert len({at[h] for h in group}) == 1 and at[group[0]] >= 1              # admitted whole, once three slots were free
    assert admissions[at[group[0]]][:3] == group and at[late] >= at[group[0]]  # in candidate order; nothing overtook it
    lp = _check_sum(eng, busy + group + [late], out)                           # after step(); a second take raises KeyError
    with pytest.raises(KeyError):
        eng.take_logprobs(max(out) + 10)                                       # unknown
    # rank_candidates over the finished group, with n_lp as the lengths
    cum, lens = [float(lp[h][1]) for h in group], [lp[h][2] for h in group]
    assert all(n == out[h].numel() and n >= 4 for n, h in zip(lens, group))
    order = rank_candidates(torch.stack([lp[h][1] for h in group]), lens)
    mean = [c / n for c, n in zip(cum, lens)]
    assert sorted(order) == [0, 1, 2] and all(mean[a] >= mean[b] for a, b in zip(order, order[1:]))
    by_sum = rank_candidates(cum, lens, length_normalize=False)
    assert sorted(by_sum) == [0, 1, 2] and all(cum[a] >= cum[b] for a, b in zip(by_sum, by_sum[1:]))
    plain = ContinuousXYDecoder(small, **KW)
    h = plain.submit(prompts[0], max_new_frames=2)
    plain.run()
    with pytest.raises(ValueError, match="logprobs=True"):
        plain.take_logprobs(h)
