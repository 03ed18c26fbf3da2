"""GPU (-m gpu): every id the token-draw kernels emit against the host replay (tests/draw_replay.py: Philox + a float64 chain).
An unambiguous draw must equal its prediction; an ambiguous one (a uniform within fp32 rounding of a CDF step or of the top-p cut)
must lie in the admissible set; at most 3 % of a case's draws may be ambiguous.  Every case prints its ambiguous share and its
mismatch count (recorded in profiles/draw_replay_ids.txt).  The cases are those of tests/draw_cases.py, whose cap is shown on the
CPU in tests/test_draw_replay.py."""
import numpy as np
import pytest
import torch

import draw_cases as dc
import draw_replay as dr
from rwkvtts_amd.continuous import SlotState, sample_slots
from rwkvtts_amd.sampling import RowSampler, ras_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _verdict(name, pairs):
    """pairs: [(Draws, device ids)] of one case"""
    n = sum(d.amb.size for d, _ in pairs)
    amb = sum(int(d.amb.sum()) for d, _ in pairs)
    res = [d.compare(ids) for d, ids in pairs]
    wrong, out = sum(r[0] for r in res), sum(r[1] for r in res)
    print(f"{name}: {n} draws, ambiguous {amb / max(n, 1):.4%}, mismatches {wrong}, outside the admissible set {out}")
    assert wrong == 0, f"{name}: {wrong} unambiguous draws differ from the prediction"
    assert out == 0, f"{name}: {out} ambiguous draws outside their admissible set"
    assert amb <= dr.CAP * n, f"{name}: {amb} of {n} draws ambiguous"


def _run_rows(lg, kw, launches):
    """the raw draws of one RowSampler per seed for every (seed, step)"""
    lgd = lg.to(DEV)
    step = torch.zeros(1, dtype=torch.long, device=DEV)
    out, smp = [], {}
    for seed, s in launches:
        if seed not in smp:
            smp[seed] = RowSampler(lgd.device, seed=seed, **kw)
        step.fill_(s)
        out.append(smp[seed](lgd, step).cpu())
    return out


@pytest.mark.parametrize("n", dc.CLOSED_SIZES)
def test_closed_batch_ids_equal_the_replay(n):
    for name, lg, kw, launches in dc.closed_cases(n):
        got = _run_rows(lg, kw, launches)
        draws = dr.replay_rows(lg, launches=launches, **kw)
        _verdict(name, list(zip(draws, got)))
        if kw.get("do_sample") and kw.get("top_k") != 1:
            for a, b in dc.DIFFER:       # launches that differ only in the high word of the step / of the seed
                assert not torch.equal(got[a], got[b]) and (draws[a].pred != draws[b].pred).any(), (name, a, b)


def test_segment_ids_equal_the_replay():
    for name, lg, kw, _ in dc.segment_cases(256):
        kw = dict(kw)
        seed = kw.pop("seed")
        launches = [(seed, s) for s in (0, 5, dc.BIG_STEP)]
        _verdict(name, list(zip(dr.replay_rows(lg, launches=launches, **kw), _run_rows(lg, kw, launches))))


def test_selection_path_ids_equal_the_replay():
    for name, lg, kw, launches in dc.selection_cases():
        got = _run_rows(lg, kw, launches)
        draws = dr.replay_rows(lg, launches=launches, **kw)
        _verdict(name, list(zip(draws, got)))
        if name == "constant_and_200_tied":          # the candidates are the 128 smallest tied indices
            assert all(int(g[:32].max()) < 128 for g in got)
        if name.startswith("all_dropped"):
            assert all((g == kw["allow"][0][0]).all() for g in got)
        if name.startswith("few_finite"):
            assert all((g[:8] == kw["allow"][0][0]).all() for g in got)


@pytest.mark.parametrize("group", list(dc.groups()))
def test_recorded_groups_equal_the_replay(group):
    """draw_cases.run_groups(): every raw id, and for the tail cases what the loop keeps (ids, seq, unfinished, embedding rows)"""
    res = dc.groups()[group](DEV)
    if group.startswith("ras"):
        pairs = []
        for name, lg, ring, ptr, kw in dc.ras_cases(int(group[3:])):
            row = dr.RasRow(lg, kw["eos"], 0.8, 25)
            seq = dr.replay_ras_sequence(row, kw["seed"], ring.tolist(), ptr, dc.RAS_STEPS, kw["n_ignore"], kw["win_size"], 0.1,
                                         observed=res[name + "/tok"])
            pairs += _ras_compare(name, seq, res[name + "/tok"], res[name + "/ring"], res[name + "/ptr"], res[name + "/step"])
        _verdict(group, pairs)
        return
    pairs = []
    for name, lg, kw, tail in (dc.segment_cases() if group == "nseg4" else dc.row_cases(int(group[4:]))):
        kw = dict(kw)
        steps = list(range(dc.STEPS))
        seed = kw.pop("seed")
        draws = dr.replay_rows(lg, launches=[(seed, s) for s in steps], **kw)
        got = res[name + "/ids"]
        pairs += [(d, got[s]) for s, d in enumerate(draws)]
        if tail is not None:     # the decode tail follows from the raw ids (the observed ones: an ambiguous draw does not end it)
            kept, unf, seq = dr.replay_tail([got[s][:, 0] for s in steps], steps, tail["eos"], tail["pad"], tail["seq_ld"])
            assert np.array_equal(np.stack(kept), res[name + "/kept"]) and np.array_equal(np.stack(unf), res[name + "/unfinished"] != 0), name
            assert np.array_equal(seq, res[name + "/seq"]), name
            emb = torch.randn(kw["seg_len"][0], dc.TAIL_D, generator=torch.Generator().manual_seed(tail["emb_seed"])).to(torch.bfloat16)
            assert np.array_equal(emb[torch.from_numpy(kept[-1])].view(torch.int16).numpy(), res[name + "/x"]), name
            # and from the predicted ids wherever the draws are unambiguous
            if not any(d.amb.any() for d in draws):
                kept_p, _, seq_p = dr.replay_tail([d.pred[:, 0] for d in draws], steps, tail["eos"], tail["pad"], tail["seq_ld"])
                assert np.array_equal(seq_p, res[name + "/seq"]) and np.array_equal(np.stack(kept_p), res[name + "/kept"]), name
    _verdict(group, pairs)


def _ras_compare(name, seq, tok, ring, ptr, step):
    """device state after every step against the host sequence -> [(Draws, ids)] of one step each"""
    pairs = []
    for i, (pred, amb, adm, ring_h, ptr_h, step_h) in enumerate(seq):
        pairs.append((dr.Draws([pred], [amb], {(0,): adm}), np.array([tok[i]])))
        if amb and int(tok[i]) not in adm:
            break                                              # reported by _verdict; the host cannot follow from here
        assert ring[i].tolist() == ring_h and int(ptr[i]) == ptr_h and int(step[i]) == step_h, (name, i)
    return pairs


@pytest.mark.parametrize("V", dc.RAS_SIZES)
def test_ras_sequences_equal_the_replay(V):
    for name, lg, ring, ptr, kw in dc.ras_cases(V):
        row = dr.RasRow(lg, kw["eos"], 0.8, 25)
        lgd = lg.to(DEV)
        pairs = []
        for seed in dc.RAS_SEEDS:
            tok = torch.zeros(1, dtype=torch.long, device=DEV)
            recent, p, step_i = ring.to(DEV), torch.tensor([ptr], device=DEV), torch.tensor(0, device=DEV)
            rec = []
            for _ in range(dc.RAS_LONG):
                ras_step(lgd, tok, recent, p, step_i, **dict(kw, seed=seed))
                rec.append(torch.cat([tok, p, step_i.reshape(1), recent]))
            rec = torch.stack(rec).cpu().numpy()
            seq = dr.replay_ras_sequence(row, seed, ring.tolist(), ptr, dc.RAS_LONG, kw["n_ignore"], kw["win_size"], 0.1, observed=rec[:, 0])
            pairs += _ras_compare(f"{name}/seed{seed:x}", seq, rec[:, 0], rec[:, 3:], rec[:, 1], rec[:, 2])
        _verdict(name, pairs)


def _slot_seed(seed):
    return seed - (1 << 64) if seed >= 1 << 63 else seed


def test_slot_ids_equal_the_replay():
    """rwkv7_sample_slots_f32: every slot its own seed, step, top_k, top_p, inverse temperature and min_until; counter word 2 = 0"""
    lg, rows, P, sup, E = dc.slot_case()
    S, V, D, LD = len(P), lg.shape[1] - 3, 64, 8
    l64 = dict(dtype=torch.int64, device=DEV)
    t = lambda key, dt: torch.tensor([p[key] for p in P], dtype=dt, device=DEV)
    step, limit, min_until = t("step", torch.int64), t("limit", torch.int64), t("min_until", torch.int64)
    seed = torch.tensor([_slot_seed(p["seed"]) for p in P], **l64)
    inv_temp = torch.tensor([dc.slot_inv_temp(p) for p in P], dtype=torch.float32, device=DEV)
    top_k, top_p = t("top_k", torch.int32), t("top_p", torch.float32)
    do_sample, live = t("do_sample", torch.uint8), t("live", torch.uint8)
    ids, seq = torch.full((S,), -3, **l64), torch.full((S, LD), -7, **l64)
    emb = torch.randn(V, D, generator=torch.Generator().manual_seed(1)).to(DEV, torch.bfloat16)
    x = torch.zeros(S, D, dtype=torch.bfloat16, device=DEV)
    st = SlotState()
    st.step, st.limit, st.min_until, st.seed = step.data_ptr(), limit.data_ptr(), min_until.data_ptr(), seed.data_ptr()
    st.inv_temp, st.top_k, st.top_p, st.do_sample = inv_temp.data_ptr(), top_k.data_ptr(), top_p.data_ptr(), do_sample.data_ptr()
    st.live, st.ids, st.seq, st.seq_ld = live.data_ptr(), ids.data_ptr(), seq.data_ptr(), LD
    st.emb, st.x, st.D, st.slots, st.top_k_max, st.eos = emb.data_ptr(), x.data_ptr(), D, S, 64, E
    sample_slots(lg.to(DEV), st, torch.tensor(rows, dtype=torch.int32, device=DEV), None, None, torch.tensor(sup, dtype=torch.int32, device=DEV), V)
    torch.cuda.synchronize()
    pairs, kinds = [], set()
    for r, s in enumerate(rows):
        if s >= S or not P[s]["live"]:
            continue
        p = P[s]
        d = dr.replay_rows(lg[r:r + 1], [V], [(p["seed"], p["step"])], suppress=sup, do_sample=p["do_sample"], top_k=p["top_k"], top_p=p["top_p"],
                           inv_temp=dc.slot_inv_temp(p), min_eos=(E, p["min_until"]), word2=np.zeros((1, 1), dtype=np.uint64))[0]
        pairs.append((d, ids[s:s + 1].cpu()))
        got = int(ids[s])
        assert int(step[s]) == p["step"] + 1 and int(live[s]) == int(got != E and p["step"] + 1 < p["limit"]), (r, s)
        assert torch.equal(x[s].view(torch.int16), emb[got].view(torch.int16)), (r, s)
        if p["step"] < LD:
            assert int(seq[s, p["step"]]) == got
        kinds.add((p["do_sample"], p["top_k"] > 0))
    assert kinds == {(False, False), (True, False), (True, True)}
    assert int(ids[5]) == -3 and int(step[5]) == P[5]["step"]                      # the dead slot is untouched
    _verdict("slots", pairs)


def test_xy_slot_ids_equal_the_replay():
    """the XY slot draw through the call ContinuousXYDecoder makes: counter word 2 = channel, key = the slot's seed"""
    from test_continuous_xy_gpu import CASES, _Slots
    S = 16
    z = _Slots(S, D=128, LD=16, seed=3, **CASES["toy4"])
    perm = torch.randperm(S, generator=z.g).tolist()
    rows = perm + [-1, S + 5]
    lg = torch.randn(len(rows), z.width, generator=z.g) * 3
    z.draw(lg.to(DEV), torch.tensor(rows, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    pairs = []
    for r, s in enumerate(perm):
        p = z.P[s]
        if not p["live"]:
            continue
        d = dr.replay_rows(lg[r:r + 1], z.sizes, [(p["seed"], p["step"])], seg_off=z.off, allow=z.allow, do_sample=p["do_sample"], top_k=p["top_k"],
                           top_p=p["top_p"], inv_temp=dc.slot_inv_temp(p))[0]                   # one row: word 2 = the channel
        pairs.append((d, z.nt[s].cpu()))
    _verdict("xy_slots", pairs)


def test_ras_slot_ids_equal_the_replay():
    """the RAS slot entry through the call ContinuousCosyDecoder makes, over 12 calls (the ring of ten wraps)"""
    from test_continuous_cosy_gpu import WIN, _Slots
    V = 1281
    P = [dict(step=0, limit=1000, n_ignore=0, seed=11, top_k=25, top_p=0.8, tau_r=0.1, live=1),
         dict(step=3, limit=1000, n_ignore=100, seed=(1 << 63) + 14, top_k=25, top_p=0.8, tau_r=0.1, live=1),
         dict(step=dc.BIG_STEP, limit=dc.BIG_STEP + 1000, n_ignore=0, seed=13, top_k=128, top_p=1.0, tau_r=0.5, live=1),
         dict(step=6, limit=1000, n_ignore=0, seed=16, top_k=25, top_p=0.8, tau_r=0.1, live=0)]
    z = _Slots(V, P, seed=V)
    rows = [2, 0, 9, 1]
    row_slot = torch.tensor(rows, dtype=torch.int32, device=DEV)
    from rwkvtts_amd.continuous_cosy import ras_slots
    pairs = []
    host = {s: dict(ring=[-1] * WIN, ptr=0, step=P[s]["step"]) for s in (0, 1, 2)}
    for call in range(12):
        lg = torch.randn(len(rows), V, generator=z.g) * 3.0
        ras_slots(lg.to(DEV), z.st, row_slot)
        torch.cuda.synchronize()
        for r, s in enumerate(rows):
            if s not in host:
                continue
            h, p = host[s], P[s]
            row = dr.RasRow(lg[r], V - 1, p["top_p"], p["top_k"])
            pred, amb, adm = dr.replay_ras(row, p["seed"], h["step"], h["ring"], p["n_ignore"], WIN, p["tau_r"])
            got = int(z.ids[s])
            pairs.append((dr.Draws([pred], [amb], {(0,): adm}), np.array([got])))
            assert got in adm or not amb
            h["ring"], h["ptr"], h["step"] = dr.ras_bookkeeping(got, h["ring"], h["ptr"], h["step"], V - 1, WIN)
            assert z.recent[s, :WIN].tolist() == h["ring"] and int(z.ptr[s]) == h["ptr"] and int(z.step[s]) == h["step"], (call, s)
            if got == V - 1:
                del host[s]
    assert int(z.ids[3]) == -9
    _verdict("ras_slots", pairs)
