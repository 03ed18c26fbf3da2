"""Fixed inputs and calls for the token draws of csrc/sampling.hip (rwkv7_sample_rows_f32, rwkv7_sample_rows_tail_f32,
rwkv7_ras_step_f32) and their per-slot forms (test infrastructure).  The inputs are built on the CPU from seeded generators (the same
on every machine).  Their ids are pinned by the host replay of the draw (tests/draw_replay.py), which predicts every id from Philox
and a float64 chain, not by a recorded file: tests/test_draw_replay.py shows on the CPU that the replay is the law and that every
case below leaves at most 3 % of its draws ambiguous, tests/test_draw_replay_gpu.py runs the cases (run_groups() included) on the
device and compares id for id."""
import numpy as np
import torch

from rwkvtts_amd.sampling import RowSampler, SampleTail, ras_step

# allowed-range sizes: a small segment, the first size of the 33-per-thread class, the first of the 60-per-thread class
ROW_SIZES = (97, 1281, 8449)
RAS_SIZES = (97, 6562, 8449)
ROWS, STEPS, RAS_STEPS, TAIL_D = 4, 8, 12, 128
SEED_LO, SEED_HI = 0x1234567, (1 << 63) | 0x0fedcba987654321   # the second one has bit 63 set


def _modes():
    """greedy, plain multinomial, top_k x top_p; both temperatures and both seeds occur among the sampled modes of every size"""
    out = [("greedy", dict(), SEED_LO), ("multinomial", dict(do_sample=True, temperature=0.6), SEED_HI)]
    i = 0
    for k in (1, 7, 64):
        for p in (1.0, 0.9, 0.5):
            out.append((f"k{k}_p{p}", dict(do_sample=True, top_k=k, top_p=p, temperature=(0.6, 1.37)[i % 2]), (SEED_LO, SEED_HI)[(i // 2) % 2]))
            i += 1
    return out


def row_cases(n):
    """[(name, logits [ROWS, >= n], RowSampler keywords, tail keywords or None)] for an allowed range of n ids"""
    g = torch.Generator().manual_seed(1000 + n)
    base = torch.randn(ROWS, n + 3, generator=g) * 2.0            # a wider buffer than the segment: row stride != width
    cases = [(name, base, dict(seg_len=[n], seed=seed, **kw), None) for name, kw, seed in _modes()]
    # suppressed ids, one of which is every row's argmax
    sup = base.clone()
    sup[:, n // 2] = 50.0
    for name, kw in (("greedy", dict()), ("k7", dict(do_sample=True, top_k=7, top_p=0.9, temperature=1.37))):
        cases.append(("suppress_" + name, sup, dict(seg_len=[n], suppress=[n // 2, 5, n - 1], seed=SEED_HI, **kw), None))
    # min-EOS bar with the EOS logit boosted: barred on steps 0..3, allowed from step 4
    eos = n - 2
    bar = base.clone()
    bar[:, eos] = 30.0
    for name, kw in (("greedy", dict()), ("k7", dict(do_sample=True, top_k=7, top_p=0.9, temperature=0.6)),
                     ("multinomial", dict(do_sample=True, temperature=1.37))):
        cases.append(("min_eos_" + name, bar, dict(seg_len=[n], min_eos=(eos, 4), seed=SEED_LO, **kw), None))
    # rows that leave the one-pass selection: clustered logits (radix select), a constant row (a round per candidate), a row of
    # -inf (no candidate survives), a row that is half -inf (tests/test_sampling_gpu.py::test_clustered_and_constant_rows_...)
    odd = torch.randn(ROWS, n, generator=g) * 1e-2 + 10.0
    odd[0, n // 3] = -1000.0
    odd[1] = 3.0
    odd[2] = float("-inf")
    odd[3, ::2] = float("-inf")
    for name, kw in (("greedy", dict()), ("k20", dict(do_sample=True, top_k=20, top_p=0.9, temperature=0.01)),
                     ("k5", dict(do_sample=True, top_k=5)), ("multinomial", dict(do_sample=True))):
        cases.append(("odd_rows_" + name, odd, dict(seg_len=[n], seed=SEED_LO, **kw), None))
    # the decode loop's tail: row 1 draws EOS at once and emits the pad id from then on, row 2 may end later; 6 columns for 8 steps
    end = base.clone()
    end[1, eos] = 40.0
    end[2, eos] = float(end[2].max())
    for name, kw in (("greedy", dict()), ("k7", dict(do_sample=True, top_k=7, top_p=0.9, temperature=1.37))):
        cases.append(("tail_" + name, end, dict(seg_len=[n], seed=SEED_HI, **kw), dict(eos=eos, pad=1, seq_ld=6, emb_seed=2000 + n)))
    cases.append(("tail_min_eos", end, dict(seg_len=[n], min_eos=(eos, 3), do_sample=True, top_k=7, top_p=0.9, temperature=0.6, seed=SEED_LO),
                  dict(eos=eos, pad=1, seq_ld=6, emb_seed=2000 + n)))
    return [(f"rows{n}/{name}", lg, kw, tail) for name, lg, kw, tail in cases]


def segment_cases(rows=ROWS):
    """four unequal segments with allowed ranges (lo > 0 on segment 0): the Philox counter holds the workgroup index"""
    sizes, allow = [97, 1281, 33, 700], [(10, 90), (0, 1281), (0, 33), (100, 400)]
    g = torch.Generator().manual_seed(77)
    lg = torch.randn(rows, sum(sizes) + 5, generator=g) * 2.0
    modes = (("greedy", dict()), ("multinomial", dict(do_sample=True, temperature=0.6)),
             ("k7_p0.9", dict(do_sample=True, top_k=7, top_p=0.9, temperature=1.37)), ("k64_p0.5", dict(do_sample=True, top_k=64, top_p=0.5)))
    return [(f"nseg4/{name}", lg, dict(seg_len=sizes, allow=allow, suppress=[12, 5], seed=SEED_HI, **kw), None) for name, kw in modes]


def run_row_case(lg, kw, tail, dev):
    """ids after each of STEPS launches (+ what the tail kept, and the seq and x rows it left) as numpy arrays"""
    lg = lg.to(dev)
    smp = RowSampler(lg.device, **kw)
    step = torch.zeros(1, dtype=torch.long, device=dev)
    out = {"ids": []}
    t = None
    if tail is not None:
        g = torch.Generator().manual_seed(tail["emb_seed"])
        emb = torch.randn(kw["seg_len"][0], TAIL_D, generator=g).to(torch.bfloat16).to(dev)
        ids = torch.zeros(ROWS, dtype=torch.long, device=dev)
        seq = torch.full((ROWS, tail["seq_ld"]), -7, dtype=torch.long, device=dev)
        unf = torch.ones(ROWS, dtype=torch.bool, device=dev)
        x = torch.zeros(ROWS, TAIL_D, dtype=torch.bfloat16, device=dev)
        t = SampleTail.make(ids, seq=seq, unfinished=unf, eos=tail["eos"], pad=tail["pad"], emb=emb, x=x)
        out.update(kept=[], unfinished=[])
    for s in range(STEPS):
        step.fill_(s)
        out["ids"].append(smp(lg, step, tail=t).clone())
        if t is not None:
            out["kept"].append(ids.clone())
            out["unfinished"].append(unf.clone())
    res = {k: torch.stack(v).cpu().numpy().astype(np.uint8 if k == "unfinished" else np.int32) for k, v in out.items()}
    if t is not None:   # what the last step left: the generated columns and the next input rows (bf16 bit patterns)
        res["seq"] = seq.cpu().numpy().astype(np.int32)
        res["x"] = x.view(torch.int16).cpu().numpy()
    return res


def ras_cases(V):
    """[(name, logits [V], ring, ptr, ras_step keywords)]: both ring registers (win_size 10 / 128) x the three special paths"""
    eos = V - 1
    cases = []
    for win in (10, 128):
        g = torch.Generator().manual_seed(3000 + V + win)
        base = torch.randn(V, generator=g) * 5.0    # (a spread at which under 3 % of the whole-row draws fall within the fp32 margin)
        ring = torch.randint(0, V - 1, (win,), generator=g)
        ptr = 3 if win == 10 else 70
        lg = base.clone()
        lg[eos] = lg.max() + 0.5                    # EOS leads the nucleus: barred on steps 0..5, allowed from step 6
        cases.append((f"win{win}_n_ignore", lg, ring, ptr, dict(n_ignore=6, eos=eos, win_size=win, seed=SEED_LO)))
        lg = base.clone()
        lg[eos] = lg.max() + 12.0                   # the nucleus holds nothing but EOS
        cases.append((f"win{win}_eos_alone", lg, ring, ptr, dict(n_ignore=10 ** 9, eos=eos, win_size=win, seed=SEED_HI)))
        lg = base.clone()
        hot = int(lg.argmax())
        lg[hot] += 4.0                              # the likeliest candidate fills half the ring: the repetition fallback fires
        rep = ring.clone()
        rep[::2] = hot
        cases.append((f"win{win}_repeat", lg, rep, ptr, dict(n_ignore=0, eos=eos, win_size=win, seed=SEED_LO)))
    return [(f"ras{V}/{name}", lg, ring, ptr, kw) for name, lg, ring, ptr, kw in cases]


def run_ras_case(lg, ring, ptr, kw, dev):
    """tok, the ring, ptr and the step counter after each of RAS_STEPS consecutive calls"""
    lg = lg.to(dev)
    tok = torch.zeros(1, dtype=torch.long, device=dev)
    recent, p, step_i = ring.to(dev), torch.tensor([ptr], device=dev), torch.tensor(0, device=dev)
    out = {"tok": [], "ring": [], "ptr": [], "step": []}
    for _ in range(RAS_STEPS):
        ras_step(lg, tok, recent, p, step_i, **kw)
        for k, v in (("tok", tok[0]), ("ring", recent), ("ptr", p[0]), ("step", step_i)):
            out[k].append(v.clone())
    return {k: torch.stack(v).cpu().numpy().astype(np.int32) for k, v in out.items()}


def groups():
    """group name -> function(dev) returning {key: array}; one group is one test case"""
    def rows(cases):
        return lambda dev: {f"{name}/{k}": v for name, lg, kw, tail in cases() for k, v in run_row_case(lg, kw, tail, dev).items()}

    def ras(V):
        return lambda dev: {f"{name}/{k}": v for name, lg, ring, ptr, kw in ras_cases(V) for k, v in run_ras_case(lg, ring, ptr, kw, dev).items()}

    out = {f"rows{n}": rows(lambda n=n: row_cases(n)) for n in ROW_SIZES}
    out["nseg4"] = rows(segment_cases)
    out.update({f"ras{V}": ras(V) for V in RAS_SIZES})
    return out


def run_groups(dev):
    res = {}
    for run in groups().values():
        res.update(run(dev))
    return res


# ---- cases whose every id the host replay predicts (tests/test_draw_replay.py, tests/test_draw_replay_gpu.py) -------------------
# both sides of each elements-per-thread class boundary (1280 | 1281, 8448 | 8449), a small range and the largest one
CLOSED_SIZES = (97, 1280, 1281, 8448, 8449, 15360)
CLOSED_ROWS = 1024
BIG_STEP = 2 ** 32 + 3
RAS_SEEDS = (SEED_LO, SEED_HI, 77)
RAS_LONG = 64


def closed_launches(seed):
    """(seed, step) of the launches of one closed-batch case; DIFFER: pairs of launches that differ only in the high word of the
    step (BIG_STEP | 3) or of the seed (bit 63) and must not draw the same ids"""
    return [(seed, 0), (seed, 5), (seed, BIG_STEP), (seed, 3), (seed ^ (1 << 63), 5)]


DIFFER = ((2, 3), (1, 4))
_closed = {}


def closed_logits(n):
    """CLOSED_ROWS different rows for an allowed range of n ids (shared by every mode, never written).  The spread (3.0) keeps
    the whole-row CDF steps of the multinomial mode far enough apart that under 3 % of its draws fall within the fp32 margin."""
    if n not in _closed:
        _closed[n] = torch.randn(CLOSED_ROWS, n + 3, generator=torch.Generator().manual_seed(5000 + n)) * 3.0
    return _closed[n]


def closed_cases(n):
    """[(name, logits, replay / RowSampler keywords, launches)]"""
    return [(f"closed{n}/{name}", closed_logits(n), dict(seg_len=[n], **kw), closed_launches(seed)) for name, kw, seed in _modes()]


def selection_cases():
    """rows that leave the one-pass selection or have no candidate at all, with the id of every draw asserted
    [(name, logits, keywords, launches)]"""
    g = torch.Generator().manual_seed(91)
    L = [(SEED_LO, 0), (SEED_HI, 7)]
    out = []
    R, n = 256, 8449                                  # clustered: one far outlier, the rest within 1e-2 (the radix select)
    lg = torch.randn(R, n, generator=g) * 1e-2 + 10.0
    lg[torch.arange(R), torch.randint(0, n, (R,), generator=g)] = -1000.0
    out.append(("clustered", lg, dict(seg_len=[n], do_sample=True, top_k=20, top_p=0.9, temperature=0.01), L))
    R, n = 64, 1000                                   # constant rows; three leaders and 200 ids tied at the k-th value (k = 5)
    lg = torch.full((R, n), 3.0)
    for r in range(32, R):
        lg[r] = torch.randn(n, generator=g)
        tied = torch.randperm(n, generator=g)[:203]
        lg[r, tied[3:]] = 6.0
        lg[r, tied[:3]] = torch.tensor([9.0, 8.0, 7.0])
    out.append(("constant_and_200_tied", lg, dict(seg_len=[n], do_sample=True, top_k=5), L))
    R, n = 256, 1281                                  # three more ids equal to the 7th largest value of a random row
    lg = torch.randn(R, n, generator=g) * 2.0
    kth = lg.topk(7, 1).values[:, -1]
    for r in range(R):
        lg[r, torch.randperm(n, generator=g)[:3]] = kth[r]
    out.append(("ties_at_kth", lg, dict(seg_len=[n], do_sample=True, top_k=7, top_p=0.9, temperature=0.6), L))
    half = torch.randn(R, n, generator=g) * 3.0      # half of every row is -inf
    half[:, ::2] = float("-inf")
    out.append(("half_inf_k7", half, dict(seg_len=[n], do_sample=True, top_k=7, top_p=0.9), L))
    out.append(("half_inf_multinomial", half, dict(seg_len=[n], do_sample=True), L))
    R, n = 64, 97                                     # five finite ids per row, top_k = 64; rows 0..7 hold nothing but -inf
    few = torch.full((R, n), float("-inf"))
    for r in range(8, R):
        few[r, torch.randperm(n, generator=g)[:5]] = torch.randn(5, generator=g) * 2.0
    for name, kw in (("greedy", dict()), ("k64", dict(do_sample=True, top_k=64, top_p=0.9)), ("multinomial", dict(do_sample=True))):
        out.append(("few_finite_" + name, few, dict(seg_len=[n], allow=[(10, 90)], **kw), L))
    lg = torch.randn(R, n, generator=g)               # suppression and the min-EOS bar cover the whole allowed range
    for name, kw in (("greedy", dict()), ("k7", dict(do_sample=True, top_k=7)), ("multinomial", dict(do_sample=True))):
        out.append(("all_dropped_" + name, lg, dict(seg_len=[n], allow=[(10, 13)], suppress=[10, 11], min_eos=(12, 100), **kw), L))
    return out


def slot_case():
    """rwkv7_sample_slots_f32 with heterogeneous slots: (logits [rows, V + 3], row -> slot (one entry names no slot), per-slot
    parameter dicts, suppressed ids, EOS id).  Slot 5 is dead; sampled slots with top_k = 0 and greedy slots occur."""
    import random
    S, V = 24, 1281
    E = V - 2
    rng = random.Random(17)
    g = torch.Generator().manual_seed(321)
    P = []
    for s in range(S):
        do_sample = s % 4 != 0
        top_k = rng.choice([0, 1, 7, 64]) if do_sample else 0
        step = rng.choice([0, 3, BIG_STEP])
        P.append(dict(do_sample=do_sample, top_k=top_k, top_p=rng.choice([1.0, 0.9, 0.5]) if top_k else 1.0,
                      temperature=rng.choice([0.6, 1.0, 1.37]), seed=rng.getrandbits(64) | ((s % 2) << 63), step=step,
                      min_until=step + (s % 3 == 0), limit=step + 5, live=s != 5))
    perm = torch.randperm(S, generator=g).tolist()
    rows = perm[:10] + [S + 3] + perm[10:]
    lg = torch.randn(len(rows), V + 3, generator=g) * 3.0
    lg[::3, E] = 30.0                                   # EOS leads a third of the rows; barred in the slots with min_until > step
    return lg, rows, P, [7, 640], E


def slot_inv_temp(p):
    """the fp32 factor a slot stores for temperature p["temperature"]"""
    return (torch.tensor(1.0) / torch.tensor(p["temperature"], dtype=torch.float32)).item() if p["do_sample"] else 1.0
