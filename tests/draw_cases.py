"""Fixed inputs and calls for pinning the closed-batch token draws of csrc/sampling.hip (rwkv7_sample_rows_f32,
rwkv7_sample_rows_tail_f32, rwkv7_ras_step_f32) bit for bit (test infrastructure).  The per-slot kernels are required to equal these
entries (tests/test_continuous*_gpu.py), so once the draw bodies are shared only a record of these ids can see a change in a shared
body.  The inputs are built on the CPU from seeded generators (the same on every machine); only results are meant to be stored.

tools/pin_draw_ids.py records `run_groups()` into tests/golden/draw_ids.npz and compares a later run against it.  No record has
been written yet."""
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


def segment_cases():
    """four unequal segments with allowed ranges (lo > 0 on segment 0): the Philox counter holds the workgroup index"""
    sizes, allow = [97, 1281, 33, 700], [(10, 90), (0, 1281), (0, 33), (100, 400)]
    g = torch.Generator().manual_seed(77)
    lg = torch.randn(ROWS, sum(sizes) + 5, generator=g) * 2.0
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
        base = torch.randn(V, generator=g) * 1.5
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
