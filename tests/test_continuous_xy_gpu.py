"""GPU (-m gpu): continuous batching for the XY model -- the per-slot frame entries (rwkv7_xy_slots_draw_f32,
rwkv7_xy_slots_frame_bf16) against the closed-batch entries they must equal for a batch of one (rwkv7_sample_rows_f32,
rwkv7_xy_frame_step, rwkv7_xy_embed_bf16), and ContinuousXYDecoder: slot / admission-time invariance, agreement with
RWKV7XYLM.generate, EOS retirement with slot reuse, and the widths of the 1.5B XY configuration."""
import random
from types import SimpleNamespace

import pytest
import torch

from rwkvtts_amd import backbone
from rwkvtts_amd.backbone import Cache
from rwkvtts_amd.continuous_xy import ContinuousXYDecoder, XYSlotState, head_column_map, xy_slots_draw, xy_slots_frame
from rwkvtts_amd.decode import DecodeStep
from rwkvtts_amd.sampling import RowSampler, XYEmbed, xy_frame_step
from rwkvtts_amd.xy_llm import RWKV7XYConfig, RWKV7XYLM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DECISIVE = 0.03   # tests/test_continuous_gpu.py: top-1 / top-2 margin as a share of the logit range


# ---------------------------------------------------------------------------------------------------------------- 1. kernels
class _Slots:
    """S slots of C channels with random tables and per-slot parameters; channel 0's allowed range [lo0, hi0) may be wider than the
    audio range [shift, shift + SV): its logits row holds the allowed part only (seg_off negative)."""

    def __init__(self, S, C, V0, SV, shift, lo0, D, LD, seed, eos=None):
        self.S, self.C, self.D, self.LD, self.SV, self.shift, self.eos = S, C, D, LD, SV, shift, eos
        hi0 = shift + SV
        self.sizes = [V0] + [SV] * (C - 1)
        self.allow = [(lo0, hi0)] + [(0, SV)] * (C - 1)
        col0 = [0] + [hi0 - lo0 + SV * (c - 1) for c in range(1, C)]
        self.off = [c - a[0] for c, a in zip(col0, self.allow)]
        self.width = col0[-1] + SV
        self.max_domain = max(hi - lo for lo, hi in self.allow)
        self.pad = SV - 1
        rng = self.rng = random.Random(seed)
        g = self.g = torch.Generator().manual_seed(seed)
        self.P = []
        for s in range(S):
            do_sample = s % 4 != 0
            top_k = rng.choice([0, 1, 7, 50, 64]) if do_sample else 0
            self.P.append(dict(do_sample=do_sample, top_k=top_k, top_p=rng.choice([1.0, 0.9, 0.5]) if top_k else 1.0,
                               temperature=rng.choice([0.6, 1.0, 1.37]), seed=rng.getrandbits(64), step=rng.randint(0, 5),
                               live=s % 9 != 8))
        self.P[1]["seed"] |= 1 << 63   # a key that does not fit a signed 64-bit integer
        self.P[1].update(do_sample=True, live=True)
        i32, l64 = dict(dtype=torch.int32, device=DEV), dict(dtype=torch.int64, device=DEV)
        t = lambda key, dt: torch.tensor([p[key] for p in self.P], dtype=dt, device=DEV)
        self.step, self.top_k, self.top_p = t("step", torch.int64), t("top_k", torch.int32), t("top_p", torch.float32)
        self.do_sample, self.live = t("do_sample", torch.uint8), t("live", torch.uint8)
        self.limit = torch.tensor([p["step"] + rng.randint(1, 12) for p in self.P], **l64)
        self.seed = torch.tensor([p["seed"] - (1 << 64) if p["seed"] >= 1 << 63 else p["seed"] for p in self.P], **l64)
        self.inv_temp = torch.tensor([(torch.tensor(1.0) / torch.tensor(p["temperature"], dtype=torch.float32)).item() for p in self.P],
                                     dtype=torch.float32, device=DEV)
        self.needs = torch.full((S,), -1, **l64)
        self.nt = torch.full((S, C), -5, **l64)
        self.row = torch.full((S, C), -3, **l64)
        self.seq = torch.full((S, LD, C), -7, **l64)
        self.x = torch.randn(S, D, generator=g).to(DEV, torch.bfloat16)
        self.tables = [torch.randn(n, D, generator=g).to(DEV, torch.bfloat16) for n in self.sizes]
        self.seg_off, self.seg_len = torch.tensor(self.off, **i32), torch.tensor(self.sizes, **i32)
        self.allow_lo, self.allow_hi = torch.tensor([a[0] for a in self.allow], **i32), torch.tensor([a[1] for a in self.allow], **i32)
        self.eos_list = None if eos is None else torch.tensor([eos], **l64)
        st = self.st = XYSlotState()
        st.step, st.limit, st.seed, st.inv_temp = (v.data_ptr() for v in (self.step, self.limit, self.seed, self.inv_temp))
        st.top_k, st.top_p, st.do_sample, st.live = (v.data_ptr() for v in (self.top_k, self.top_p, self.do_sample, self.live))
        st.needs, st.nt, st.row, st.seq, st.seq_ld = self.needs.data_ptr(), self.nt.data_ptr(), self.row.data_ptr(), self.seq.data_ptr(), LD
        for c, tb in enumerate(self.tables):
            st.tables[c] = tb.data_ptr()
        st.x, st.D, st.C, st.slots, st.top_k_max = self.x.data_ptr(), D, C, S, 64
        st.text_shift, st.speech_vocab, st.pad, st.eos0 = shift, SV, self.pad, -1 if eos is None else eos
        st.eos_list, st.n_eos, st.reference_termination = (None if eos is None else self.eos_list.data_ptr()), int(eos is not None), 0

    def state(self):
        return dict(step=self.step, needs=self.needs, live=self.live, nt=self.nt, row=self.row, seq=self.seq, x=self.x)

    def snapshot(self):
        return {k: v.clone() for k, v in self.state().items()}

    def draw(self, logits, row_slot=None):
        xy_slots_draw(logits, self.st, self.seg_off, self.seg_len, self.allow_lo, self.allow_hi, self.max_domain, row_slot)

    def one_row_ids(self, logits_row, s, step):
        """The ONE-row rwkv7_sample_rows_f32 call the slot's draws must equal: rows = 1, nseg = C, *step = step[s], seed = seed[s]."""
        p = self.P[s]
        rs = RowSampler(torch.device(DEV), self.sizes, self.allow, None, p["do_sample"], p["top_k"], p["top_p"], p["temperature"],
                        seed=p["seed"], seg_off=self.off)
        return rs(logits_row, torch.tensor([step], dtype=torch.int64, device=DEV))[0]


CASES = {"toy4": dict(C=4, V0=3000, SV=600, shift=2000, lo0=1900), "real8": dict(C=8, V0=66661, SV=1025, shift=65536, lo0=65536)}


@pytest.mark.parametrize("case", ["toy4", "real8"])
def test_slot_draws_equal_the_one_row_entry(case):
    S = 32
    z = _Slots(S, D=128, LD=16, seed=3, **CASES[case])
    perm = torch.randperm(S, generator=z.g).tolist()                      # row r -> slot perm[r]
    rows = perm + [-1, S + 5]                                             # two rows that belong to no slot
    logits = (torch.randn(len(rows), z.width, generator=z.g) * 3).to(DEV)
    row_slot = torch.tensor(rows, dtype=torch.int32, device=DEV)
    before = z.snapshot()
    z.draw(logits, row_slot)
    torch.cuda.synchronize()
    kinds = set()
    for r, s in enumerate(perm):
        p = z.P[s]
        if not p["live"]:
            assert torch.equal(z.nt[s], before["nt"][s]), s
            continue
        want = z.one_row_ids(logits[r:r + 1], s, p["step"])
        assert torch.equal(z.nt[s], want), (r, s, p, z.nt[s], want)
        lo, hi = z.allow[0]
        assert lo <= int(want[0]) < hi and all(0 <= int(v) < z.SV for v in want[1:])
        kinds.add((p["do_sample"], p["top_k"] > 0, p["top_k"] > 0 and p["top_p"] < 1.0))
    assert {(False, False, False), (True, False, False), (True, True, False), (True, True, True)} <= kinds
    for k, v in z.state().items():                                         # the draw writes nt and nothing else
        if k != "nt":
            assert torch.equal(v, before[k]), k
    # the same rows without row_slot (row r is slot r): the ids depend on the slot's own fields only, not on where the row sits
    nt_perm = z.nt.clone()
    z.nt.fill_(-5)
    inv = [perm.index(s) for s in range(S)]
    z.draw(logits[inv].contiguous(), None)
    torch.cuda.synchronize()
    assert torch.equal(z.nt, nt_perm)


@pytest.mark.parametrize("case", ["toy4", "real8"])
def test_slot_frames_equal_the_batch_of_one_entries(case):
    S, FRAMES = 32, 14
    kw = dict(CASES[case])
    kw["lo0"] = kw["shift"] - 40                                           # channel 0 may leave the audio range: flushes happen
    eos = kw["shift"] + 3                                                  # an EOS id inside the audio range
    z = _Slots(S, D=128, LD=24, seed=5, eos=eos, **kw)
    z.step.zero_()
    z.limit.copy_(torch.tensor([z.rng.choice([2, 3, 5, 9, 30, 30, 30]) for _ in range(S)]))
    embed1 = XYEmbed(z.tables, 1)
    ended = {"budget": 0, "eos": 0, "flush": 0}
    col_eos, n_text = eos + z.off[0], kw["shift"] - kw["lo0"]
    for f in range(FRAMES):
        logits = (torch.randn(S, z.width, generator=z.g) * 3).to(DEV)
        for s in range(S):                                                 # slot-specific frames for a flush start and an EOS
            if s % 3 == 0 and f == 1 + s % 5:
                logits[s, z.rng.randrange(n_text)] = 60.0                  # a non-audio id on channel 0
            if s % 3 == 1 and f == 2 + s % 4:
                logits[s, col_eos] = 60.0
        before = z.snapshot()
        z.draw(logits)
        nt = z.nt.clone()
        xy_slots_frame(S, z.st, torch.device(DEV))
        torch.cuda.synchronize()
        for s in range(S):
            if not int(before["live"][s]):                                 # not live before the frame: completely untouched
                for k, v in z.state().items():
                    assert torch.equal(v[s], before[k][s]), (f, s, k)
                continue
            out1, row1 = before["seq"][s:s + 1].clone(), before["row"][s:s + 1].clone()
            pos, unf, needs1 = before["step"][s:s + 1].clone(), torch.ones(1, dtype=torch.int64, device=DEV), before["needs"][s:s + 1].clone()
            all_done, n_rows = torch.zeros((), dtype=torch.bool, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
            xy_frame_step(nt[s:s + 1].contiguous(), out1, row1, pos, unf, needs1, all_done, n_rows, z.shift, z.SV, z.pad, eos,
                          int(z.limit[s]), z.eos_list, False)
            x1 = embed1(row1)
            torch.cuda.synchronize()
            assert torch.equal(z.seq[s], out1[0]), (f, s)
            assert torch.equal(z.row[s], row1[0]) and int(z.needs[s]) == int(needs1[0]), (f, s)
            assert int(z.live[s]) == int(unf[0]) and int(z.step[s]) == int(pos[0]) == int(before["step"][s]) + 1, (f, s)
            assert torch.equal(z.x[s].view(torch.int16), x1[0].view(torch.int16)), (f, s)
            if not int(z.live[s]):
                flushed = int(before["needs"][s]) >= 0 or not (z.shift <= int(nt[s, 0]) < z.shift + z.SV)
                ended["flush" if flushed and int(z.needs[s]) == -1 else "eos" if int(z.row[s, 0]) == eos and not flushed else "budget"] += 1
    assert int(z.live.sum()) < S and min(ended.values()) >= 1, ended      # slots ended on their budget, on EOS and after a flush


# ---------------------------------------------------------------------------------------------------------------- 2. engine
def _model(L=2, seed=5, V0=300, SV=64, shift=200, C=4, **dims):
    d = dict(hidden_size=128, num_hidden_layers=L, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=32)
    d.update(dims)
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


def _prompts(n, cfg, seed, lo=3, hi=60):
    g = torch.Generator().manual_seed(seed)
    out = []
    for t in torch.randint(lo, hi, (n,), generator=g).tolist():
        ch0 = torch.randint(0, cfg.text_shift_size + cfg.speech_vocab_size, (t, 1), generator=g)
        out.append(torch.cat([ch0, torch.randint(0, cfg.speech_vocab_size - 1, (t, cfg.num_channels - 1), generator=g)], 1).to(DEV))
    return out


REQ = [dict(max_new_frames=30), dict(max_new_frames=50), dict(max_new_frames=33), dict(max_new_frames=64)]
SAMPLED = [dict(do_sample=True, top_k=50, top_p=0.95, temperature=0.8, seed=11), dict(do_sample=True, seed=12),
           dict(do_sample=True, top_k=5, temperature=1.3, seed=13), dict(do_sample=True, top_k=64, top_p=0.5, seed=(1 << 63) + 14)]


@pytest.mark.parametrize("sampled,admission", [(False, "eager"), (True, "eager"), (False, "graph"), (True, "graph")])
def test_frames_do_not_depend_on_slot_or_admission_time(sampled, admission):
    """Graph admission: for the same pack composition (the four requests are admitted together, in order, in both engines)."""
    m = _model()
    prompts = _prompts(4, m.config, 5)
    kws = [dict(r, **(SAMPLED[i] if sampled else {})) for i, r in enumerate(REQ)]
    ekw = dict(slots=8, max_new_frames_cap=128, admission=admission, prefill_buckets=(256, 512))
    a = ContinuousXYDecoder(m, **ekw)
    ha = [a.submit(p, **kw) for p, kw in zip(prompts, kws)]
    ra = a.run()
    b = ContinuousXYDecoder(m, **ekw)
    busy = [b.submit(p, max_new_frames=100, do_sample=True, seed=i) for i, p in enumerate(_prompts(4, m.config, 9))]
    out = dict(b.step())                                   # the four busy requests hold slots 0..3 and run 16 steps
    assert not out and sorted(b.sched.busy) == [0, 1, 2, 3] and b.replays == 16
    hb = [b.submit(p, **kw) for p, kw in zip(prompts, kws)]
    out.update(b.step())
    assert sorted(b.sched.busy) == list(range(8))         # admitted together, into slots 4..7, 16 steps later
    out.update(b.run())
    assert sorted(out) == sorted(busy + hb)
    for x, y, kw in zip(ha, hb, kws):
        assert ra[x].shape == (kw["max_new_frames"], 4) and ra[x].dtype == torch.int64
        assert torch.equal(ra[x], out[y]), (kw, ra[x], out[y])
        assert ((ra[x][:, 0] >= 200) & (ra[x][:, 0] < 264)).all() and ((ra[x][:, 1:] >= 0) & (ra[x][:, 1:] < 64)).all()


def _margins(m, prompt, frames):
    """The logits generate() decides on, teacher-forced along its frames: per frame the smallest relative top-2 margin of the C channels
    (channel 0 over its audio range)."""
    cfg = m.config
    cm = head_column_map(cfg.vocab_size, cfg.speech_vocab_size, cfg.num_channels, cfg.text_shift_size)
    lo0, hi0 = cm.head0_rows
    cache = Cache.zeros(cfg, 1, DEV, torch.bfloat16)
    out = []
    with torch.no_grad():
        lg = [l[:, -1].float() for l in m(input_ids=prompt.unsqueeze(0), past_key_values=cache, use_cache=True).logits]
        lg = torch.cat([lg[0][:, lo0:hi0]] + lg[1:], 1)
        head = SimpleNamespace(weight=torch.cat([m.heads[0].weight[lo0:hi0]] + [h.weight for h in m.heads[1:]], 0).contiguous(),
                               bias=torch.cat([m.heads[0].bias[lo0:hi0]] + [h.bias for h in m.heads[1:]], 0).contiguous())
        step = DecodeStep(m.model, head, cache)
        for t in range(len(frames)):
            mg = []
            for c in range(cfg.num_channels):
                seg = lg[0, cm.col0[c]:cm.col0[c] + cfg.speech_vocab_size]
                top = seg.topk(2).values
                mg.append(((top[0] - top[1]) / (seg.max() - seg.min())).item())
            out.append(min(mg))
            if t + 1 < len(frames):
                lg = step(m.embed(frames[t].view(1, 1, -1))[:, 0].contiguous())
    return out


def test_greedy_agrees_with_generate():
    m = _model()
    prompts = _prompts(6, m.config, 21, lo=8, hi=100)
    eng = ContinuousXYDecoder(m, slots=4, max_new_frames_cap=64)   # six requests through four slots: two are admitted later
    hs = [eng.submit(p, max_new_frames=40 + 4 * i) for i, p in enumerate(prompts)]
    got = eng.run()
    for i, (h, p) in enumerate(zip(hs, prompts)):
        ref = m.generate(p.unsqueeze(0), max_new_tokens=40 + 4 * i, do_sample=False, use_graph=True)[0, p.shape[0]:]
        assert got[h].shape == ref.shape == (40 + 4 * i, 4)
        mg = _margins(m, p, ref)
        first_indecisive = next((t for t, v in enumerate(mg) if v <= DECISIVE), len(mg))
        ne = (got[h] != ref).any(1).nonzero()
        prefix = int(ne[0]) if len(ne) else len(ref)
        print(f"request {i}: equal frames {prefix} of {len(ref)}, first indecisive frame {first_indecisive}")
        assert prefix >= first_indecisive, (i, prefix, first_indecisive)


def test_eos_retires_and_the_slot_is_reused():
    m = _model()
    p0, p1 = _prompts(2, m.config, 31)
    kw0 = dict(max_new_frames=40, do_sample=True, top_k=50, seed=3)
    kw1 = dict(max_new_frames=40, do_sample=True, top_k=50, seed=4)
    solo = ContinuousXYDecoder(m, slots=1, max_new_frames_cap=64)
    h = solo.submit(p0, **kw0)
    f0 = solo.run()[h]
    ch0 = f0[:, 0].tolist()
    # EOS = the channel-0 id the request emits at frame 5 (or the first later frame whose id is new)
    t = next(t for t in range(5, 40) if ch0[t] not in ch0[:t])
    E = ch0[t]
    solo1 = ContinuousXYDecoder(m, slots=1, max_new_frames_cap=64, eos_token_id=E)
    h = solo1.submit(p1, **kw1)
    f1 = solo1.run()[h]
    eng = ContinuousXYDecoder(m, slots=1, max_new_frames_cap=64, eos_token_id=E)
    h0 = eng.submit(p0, **kw0)
    h1 = eng.submit(p1, **kw1)      # pending until the first request retires
    got = eng.run()
    assert got[h0].shape == (t + 1, 4) and int(got[h0][-1, 0]) == E and torch.equal(got[h0], f0[:t + 1])
    assert torch.equal(got[h1], f1)


def test_1p5b_widths_every_handle_once():
    """The widths of the 1.5B XY configuration (D = 2048, 32 heads, ranks 96/96/64/256, 8 channels, V0 = 66 661, 1 025 speech ids) at a
    depth of 4 layers instead of 24: the frame path does not depend on the depth, and the 24-layer model would make this test several
    times longer than the other full-shape tests."""
    c = backbone.config_1p5b()
    m = _model(L=4, V0=66661, SV=1025, shift=65536, C=8, hidden_size=c.hidden_size, decay_low_rank_dim=c.decay_low_rank_dim,
               a_low_rank_dim=c.a_low_rank_dim, v_low_rank_dim=c.v_low_rank_dim, gate_low_rank_dim=c.gate_low_rank_dim,
               intermediate_size=c.intermediate_size)
    rng = random.Random(7)
    E = 65536 + 7
    eng = ContinuousXYDecoder(m, slots=32, max_new_frames_cap=96, eos_token_id=E)
    prompts = _prompts(64, m.config, 41, lo=4, hi=200)
    want, got = {}, {}
    for i, p in enumerate(prompts):
        n = rng.randint(1, 96)
        want[eng.submit(p, max_new_frames=n, do_sample=bool(i % 2), top_k=20, seed=i)] = n
        if i % 16 == 15:
            for h, f in eng.step():
                assert h not in got
                got[h] = f
    for h, f in eng.run().items():
        assert h not in got
        got[h] = f
    assert sorted(got) == sorted(want)
    for h, n in want.items():
        f = got[h]
        assert f.dim() == 2 and 1 <= f.shape[0] <= n and f.shape[1] == 8 and f.dtype == torch.int64
        assert (((f[:, 0] >= 65536) & (f[:, 0] < 66561)) | (f[:, 0] == E)).all()
        assert ((f[:, 1:] >= 0) & (f[:, 1:] < 1025)).all()
        assert f.shape[0] == n or int(f[-1, 0]) == E       # ended on its budget or on EOS
