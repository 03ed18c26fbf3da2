"""CPU: the host replay of the token draws (tests/draw_replay.py) on its own evidence, before a GPU is involved: Philox known-answer
vectors, the u -> id map of the replay against the float64 laws (interval lengths = probabilities), the share of ambiguous draws in
every case tests/test_draw_replay_gpu.py runs (at most 3 %), and agreement with an fp32 twin of the chain in the kernel's order of
operations on every unambiguous draw."""
import numpy as np
import pytest
import torch

import draw_cases as dc
import draw_replay as dr
from sampling_laws import exact_probs, ras_factors


def test_philox_known_answers_and_the_uniform():
    # Random123 kat_vectors (philox4x32, 10 rounds): counter, key -> output
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert " ".join("%08x" % int(w) for w in dr.philox4x32_10(ctr, key)) == want
    c = np.array([[0, 0xffffffff], [0x243f6a88, 0]], dtype=np.uint64)           # vectorised: same words as one at a time
    out = dr.philox4x32_10((c, 0xffffffff - c, 5, 0x5a17), (7, c))
    for i in range(2):
        for j in range(2):
            one = dr.philox4x32_10((int(c[i, j]), 0xffffffff - int(c[i, j]), 5, 0x5a17), (7, int(c[i, j])))
            assert [int(w[i, j]) for w in out] == [int(w) for w in one]
    assert dr.u01(0xffffffff) == 1 - 2.0 ** -24 and dr.u01(0xff) == 0.0 and dr.u01(0x100) == 2.0 ** -24
    assert dr.split64(-1) == (0xffffffff, 0xffffffff) and dr.split64(dc.BIG_STEP) == (3, 1)
    assert dr.split64(dc.SEED_HI)[1] >> 31 == 1
    assert dr.kernel_order(600)[:4].tolist() == [0, 256, 512, 1]


def _rows_like_the_distribution_tests():
    """the parameter sets and rows of tests/test_sampling_gpu.py"""
    out = []
    for V, k, p, T in ((200, 50, 0.95, 0.8), (8193, 20, 0.7, 1.3), (300, 5, 1.0, 1.0), (64, 64, 0.5, 2.0), (1025, 1, 0.9, 0.7)):
        row = torch.randn(V, generator=torch.Generator().manual_seed(V + k)) * 2.0
        row[3] = row[7]
        out.append((row, k, p, T))
    out.append((torch.tensor([5.0, 1.0, 4.0, 4.0, 4.0, 0.0, -1.0]), 2, 1.0, 1.0))
    row = torch.randn(8193, generator=torch.Generator().manual_seed(5)) * 1e-2 + 10.0
    row[100] = -1000.0
    out.append((row, 20, 0.9, 0.01))
    out.append((torch.tensor([0.3, -1.0, 2.0, 0.1, 1.5]), 50, 0.9, 1.0))
    return out


def _shifted(x):
    """float32(x - max x) as float64: the exponents of the kernel's weights"""
    return torch.from_numpy((x - x.max()).astype(np.float32)).double()


@pytest.mark.parametrize("i", range(8))
def test_interval_lengths_equal_the_warper_chain(i):
    """For a fixed row the replay's u -> id map is piecewise constant; the total length of each id's interval is its probability.
    The law is evaluated on what the kernel exponentiates, d_j = float32(x_j - max x) with x = float32(logit) * float32(1 / T) (the
    chain is invariant under the shift, and d_j is monotone in x_j), and with the fp32 top_p."""
    row, k, p, T = _rows_like_the_distribution_tests()[i]
    x = dr.scaled_rows(row.unsqueeze(0), 0, 0, row.numel(), dr.inv_temperature(T))
    law = dr.TopK(x, k, p)
    got = dr.interval_law(law, 0, row.numel())
    want = exact_probs(_shifted(x[0]), k, float(np.float32(p)), 1.0).numpy()
    assert np.abs(got - want).max() <= 1e-12
    # ... and the map itself: sweeping u across [0, 1) visits the ids in candidate order, each for its interval
    u = (np.arange(4096) + 0.5) / 4096
    rep = dr.TopK(np.repeat(x, u.size, 0), k, p).draw(u)
    freq = np.bincount(rep.pred, minlength=row.numel()) / u.size
    assert np.abs(freq - want).max() <= 1.0 / 4096 + 1e-12 and (freq[want == 0] == 0).all()


def test_interval_lengths_equal_the_softmax_for_plain_multinomial():
    row = torch.randn(5000, generator=torch.Generator().manual_seed(4)) * 3.0
    x = dr.scaled_rows(row.unsqueeze(0), 0, 0, 5000, dr.inv_temperature(0.6))
    law = dr.Full(x, dr.ept_class(5000))
    want = _shifted(x[0]).softmax(-1).numpy()
    assert np.abs(dr.interval_law(law, 0, 5000) - want).max() <= 1e-12
    # the CDF runs in the kernel's element order: thread t = j % 256 major
    order = dr.kernel_order(5000)
    u = np.array([0.0, want[0] * 0.999, want[0] * 1.001, 1 - 2.0 ** -24])
    got = dr.Full(np.repeat(x, 4, 0), 60).draw(u).pred.tolist()
    assert got[:3] == [0, 0, 256] and got[3] in order[-50:]


@pytest.mark.parametrize("case", ["plain", "ignore_eos", "eos_alone", "repeat"])
def test_ras_laws_equal_the_factors_of_the_exact_law(case):
    V, eos, win = 51, 50, 10
    lg = torch.randn(V, generator=torch.Generator().manual_seed(11)) * 1.5
    recent = torch.full((win,), -1, dtype=torch.long)
    ignore = case in ("ignore_eos", "eos_alone")
    if case == "ignore_eos":
        lg[eos] = lg.max() + 0.5
    if case == "eos_alone":
        lg[eos] = lg.max() + 12.0
    if case == "repeat":
        recent[:3] = torch.tensor([int(lg.argmax()), 4, int(lg.argmax())])
    pc, full, redo = ras_factors(_shifted(lg.numpy()), recent, ignore, eos, float(np.float32(0.8)), 25, win, 0.1)
    row = dr.RasRow(lg, eos, 0.8, 25)
    got_full = dr.interval_law(row.full(ignore), 0, V)
    assert np.abs(got_full - full.numpy()).max() <= 1e-12
    nuc = row.nucleus(ignore)
    if case == "eos_alone":                      # the kept set holds nothing but EOS: the candidate comes from the whole row (word y)
        assert nuc.draw(np.array([0.3])).pred[0] == -1
        assert np.abs(got_full - pc.numpy()).max() <= 1e-12
    else:
        assert np.abs(dr.interval_law(nuc, 0, V) - pc.numpy()).max() <= 1e-12
    # the step: candidate from word z, replaced by the whole-row draw (word x) when the ring holds it win * tau_r times
    for step in range(40):
        pred, amb, adm = dr.replay_ras(row, 77, step, recent.tolist(), 10 ** 9 if ignore else 0, win, 0.1)
        wx, wy, wz, _ = dr.draw_words(77, step, 0, dr.CTR_RAS)
        c = int(nuc.draw(dr.u01(wz).reshape(1)).pred[0])
        if c < 0:
            c = int(row.full(ignore).draw(dr.u01(wy).reshape(1)).pred[0])
        want = int(row.full(ignore).draw(dr.u01(wx).reshape(1)).pred[0]) if redo[c] else c
        assert pred == want and pred in adm and (not ignore or pred != eos)


# ---- every case of the GPU file: the cap on ambiguous draws, and the fp32 twin --------------------------------------------------
def _check_rows(name, lg, kw, launches, min_draws=1):
    draws = dr.replay_rows(lg, launches=launches, **kw)
    twin = dr.twin_rows(lg, launches=launches, **kw)
    n = sum(d.amb.size for d in draws)
    amb = sum(int(d.amb.sum()) for d in draws)
    wrong = sum(d.compare(t)[0] for d, t in zip(draws, twin))
    out = sum(d.compare(t)[1] for d, t in zip(draws, twin))
    print(f"{name}: {n} draws, ambiguous {amb / n:.4%}, twin mismatches {wrong}, twin outside the admissible set {out}")
    assert wrong == 0 and out == 0, name
    return n, amb, draws


@pytest.mark.parametrize("n", dc.CLOSED_SIZES)
def test_closed_batch_cases_meet_the_cap_and_the_twin_agrees(n):
    for name, lg, kw, launches in dc.closed_cases(n):
        total, amb, draws = _check_rows(name, lg, kw, launches)
        assert amb <= dr.CAP * total, name
        if kw.get("do_sample") and kw.get("top_k") != 1:
            for a, b in dc.DIFFER:                       # the high words of step and seed reach the prediction
                assert (draws[a].pred != draws[b].pred).any(), (name, a, b)


def _steps(seed):
    return [(seed, s) for s in range(dc.STEPS)]


def test_segment_and_selection_cases_meet_the_cap_and_the_twin_agrees():
    for name, lg, kw, _ in dc.segment_cases(256):
        kw = dict(kw)
        seed = kw.pop("seed")
        total, amb, _ = _check_rows(name, lg, kw, [(seed, s) for s in (0, 5, dc.BIG_STEP)])
        assert amb <= dr.CAP * total, name
    for name, lg, kw, launches in dc.selection_cases():
        total, amb, draws = _check_rows(name, lg, kw, launches)
        assert amb <= dr.CAP * total, name
        if name.startswith("all_dropped") or name.startswith("few_finite"):
            lo = kw["allow"][0][0]
            rows = slice(0, 8) if name.startswith("few_finite") else slice(None)
            assert all((d.pred[rows] == lo).all() for d in draws), name


@pytest.mark.parametrize("group", ["rows97", "rows1281", "rows8449", "nseg4"])
def test_recorded_row_groups_meet_the_cap_and_the_twin_agrees(group):
    """the groups of draw_cases.run_groups(): 4 rows x 8 steps per case, so the cap is taken over the group (one test case)"""
    cases = dc.segment_cases() if group == "nseg4" else dc.row_cases(int(group[4:]))
    total = amb = 0
    for name, lg, kw, tail in cases:
        kw = dict(kw)
        seed = kw.pop("seed")
        n, a, _ = _check_rows(name, lg, kw, _steps(seed))
        total, amb = total + n, amb + a
    print(f"{group}: ambiguous {amb / total:.4%}")
    assert amb <= dr.CAP * total


def test_slot_case_meets_the_cap():
    lg, rows, P, sup, E = dc.slot_case()
    amb = n = 0
    for r, s in enumerate(rows):
        if s >= len(P) or not P[s]["live"]:
            continue
        p = P[s]
        d = dr.replay_rows(lg[r:r + 1], [lg.shape[1] - 3], [(p["seed"], p["step"])], suppress=sup, do_sample=p["do_sample"], top_k=p["top_k"],
                           top_p=p["top_p"], inv_temp=dc.slot_inv_temp(p), min_eos=(E, p["min_until"]), word2=np.zeros((1, 1), dtype=np.uint64))[0]
        n, amb = n + 1, amb + int(d.amb.sum())
    print(f"slots: {n} draws, {amb} ambiguous")
    assert amb <= dr.CAP * n


@pytest.mark.parametrize("V", dc.RAS_SIZES)
def test_ras_cases_meet_the_cap_and_the_twin_agrees(V):
    for name, lg, ring, ptr, kw in dc.ras_cases(V):
        row = dr.RasRow(lg, kw["eos"], 0.8, 25)
        n = amb = 0
        for seed in dc.RAS_SEEDS:
            seq = dr.replay_ras_sequence(row, seed, ring.tolist(), ptr, dc.RAS_LONG, kw["n_ignore"], kw["win_size"], 0.1)
            cur = ring.tolist()
            for step, (pred, a, adm, ring_after, _, _) in enumerate(seq):
                t = dr.twin_ras(row, seed, step, cur, kw["n_ignore"], kw["win_size"], 0.1)
                assert t == pred if not a else t in adm, (name, seed, step, t, pred, a)
                n, amb, cur = n + 1, amb + a, ring_after
        print(f"{name}: {n} steps, ambiguous {amb / n:.4%}")
        assert amb <= dr.CAP * n, name
