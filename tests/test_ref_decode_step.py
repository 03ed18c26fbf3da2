"""CPU: keeps the fp64 one-step reference of tests/test_decode_step_parity_gpu.py (tests/ref_decode_step.py) honest without a
GPU, and proves that the GPU test can fail:
  * anchor: ref_step(rounded=False) equals oracle/rwkv7_ref.py run statefully at T = 1 (the oracle the pin_*.py scripts pin against
    the reference project) to fp32 round-off of the oracle;
  * generator guard: in every case of the GPU test's list no per-channel parameter vector repeats from head to head, no two
    sequences share an input row or a state, and every regime is where its name says;
  * sensitivity: each single fault of ref_decode_step.FAULTS, planted into the rounded reference, pushes at least one observable
    beyond 2 x its bar in at least one case of the list;
  * the secondary (closer to rounded than to exact) check is skipped, by its reference-only rule, for at most one observable in four.
One sweep over the case list (module fixture) feeds the last three."""
import math

import pytest
import torch

import ref_decode_step as RD
from oracle import rwkv7_ref as R


def _p64(p):
    return {k: v.double() for k, v in p.items()}


# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,ranks,F,B", [(128, (32, 96, 64, 128), 512, 5), (192, (64, 32, 96, 160), 320, 2)])
def test_exact_reference_equals_the_stateful_oracle_at_T1(D, ranks, F, B):
    case = RD.Case("trained_like", D, B, 3, ranks, F, 77, False)
    p, states, ids = RD.make_case(case)
    x_in = p["model.embeddings.weight"][ids]
    got = RD.ref_step(_p64(p), states, x_in, case, rounded=False)
    cfg = R.RefConfig(hidden_size=D, num_hidden_layers=3, vocab_size=77, decay_low_rank_dim=ranks[0], a_low_rank_dim=ranks[1],
                      v_low_rank_dim=ranks[2], gate_low_rank_dim=ranks[3], intermediate_size=F)
    with torch.no_grad():
        _, lo, st = R.spark_forward(p, cfg, x_in[:, None], None, None, states=[s.clone() for s in states])
    # the oracle computes in fp32: 8 * 2^-24 * sqrt(K) of each tensor's maximum, K the longest reduction
    tol = 8 * RD.U24 * math.sqrt(max(D, F))
    pairs = [("logits", got["logits"], lo[:, -1])] + [(f"state{i}", a, b) for i, (a, b) in enumerate(zip(got["states"], st))]
    for name, a, b in pairs:
        err, scale = (a - b.double()).abs().max().item(), b.abs().max().item()
        print(f"anchor {name}: err {err:.3e} bar {tol * scale:.3e}")
        assert err <= tol * scale, (name, err, tol * scale)


# ----------------------------------------------------------------------------------------------------------------------------
def _guard(case, p, states, x_in, exact):
    """problems of the generated case, as strings"""
    bad = []
    D, H, N = case.D, case.H, RD.N
    per_channel = [k for k, v in p.items() if v.numel() == D and ("proj" not in k)]
    assert any(k.endswith("k_a") for k in per_channel) and any(k.endswith("g_norm.bias") for k in per_channel)
    assert any(k.endswith("w_lora.lora.2.bias") for k in per_channel) and any(k.endswith("ffn.x_k") for k in per_channel)
    for k in per_channel:
        v = p[k].reshape(H, N)
        if v.unique().numel() < N // 2:
            bad.append(f"{k}: (nearly) constant")
        for sh in range(1, H):   # read one (or more) heads off, more than half of the channels must change
            if (torch.roll(v, sh, 0) != v).float().mean().item() < 0.5:
                bad.append(f"{k}: repeats after {sh} heads")
    B = case.B
    rows = [("x_in", x_in)] + [(f"state{i}", s.reshape(B, -1)) for i, s in enumerate(states)]
    for name, t in rows:
        if case.regime == "fresh" and name != "x_in":
            if t.abs().max().item() != 0.0:   # the regime's definition: the all-zero state of a sequence just admitted
                bad.append(f"{name}: fresh state not zero")
            continue
        for i in range(B):
            for j in range(i + 1, B):
                if torch.equal(t[i], t[j]):
                    bad.append(f"{name}: sequences {i} and {j} are equal")
    # the regime is where its name says (exact reference, first step)
    reg = case.regime
    for l, it in enumerate(exact["inter"]):
        w, w_pre, a = it["w"], it["w_pre"], it["a"]
        if reg == "max_decay" and not (w.min().item() > -0.5 - 1e-3 and (w_pre > 17).any() and (w_pre < 16).any()):
            bad.append(f"layer {l}: max_decay w in [{w.min().item()}, {w.max().item()}]")
        if reg == "no_decay" and not (w_pre.max().item() <= -12 and (w_pre < -20).any() and (w_pre > -20).any()):
            bad.append(f"layer {l}: no_decay w_pre max {w_pre.max().item()}")
        if reg == "mixed_decay" and not ((w_pre > 17).any() and (w_pre < -12).any() and ((w_pre > -8) & (w_pre < 4)).any()):
            bad.append(f"layer {l}: mixed_decay misses an end")
        if reg == "gates_saturated" and ((a < 1e-4) | (a > 1 - 1e-4)).float().mean().item() < 0.99:
            bad.append(f"layer {l}: a not saturated")
        if reg == "small_state":
            med = it["var_y"].median().item()
            if not RD.GN_EPS / 8 <= med <= RD.GN_EPS * 8:
                bad.append(f"layer {l}: small_state median var_head(y) = {med:.2e}, gn_eps = {RD.GN_EPS:.2e}")
        if reg == "dead_head":
            hd = min(1, H - 1)
            kk = it["kk"].reshape(B, H, N)
            if kk[:, hd].abs().max().item() != 0.0 or not torch.isfinite(kk).all():
                bad.append(f"layer {l}: dead head's kk is not 0")
    if reg.startswith("large_state"):
        want = 10.0 if reg.endswith("_10x") else 100.0
        for i in range(case.L):
            ratio = states[3 * i + 1].std().item() / 0.5
            if not 0.9 * want < ratio < 1.1 * want:
                bad.append(f"layer {i}: state scale {ratio:.1f}x, not {want}x")
    return bad


@pytest.fixture(scope="module")
def sweep():
    """One pass over the GPU test's case list: guard findings, skip counts of the secondary check over three chained steps (the
    rounded reference's state standing in for the kernel's), and per fault the best ratio to the bar (first step)."""
    torch.manual_seed(0)
    guard, skipped, total = {}, 0, 0
    best = {f: (0.0, None, None) for f in RD.FAULTS}   # fault -> (ratio, case id, observable)
    for case in sorted(RD.CASES, key=lambda c: c.D * c.D * c.L + c.D * c.F):
        p, states, ids = RD.make_case(case)
        emb = p["model.embeddings.weight"]
        p = _p64(p)
        x_in = emb[ids]
        st = states
        for step in range(3):
            exact = RD.ref_step(p, st, x_in, case, rounded=False)
            rnd = RD.ref_step(p, st, x_in, case, rounded=True)
            bars = RD.bars(exact, rnd, st, case)
            for (name, l), b in bars.items():
                if name in ("att_kv", "logits"):
                    total += 1
                    skipped += not RD.rms_check_applies(b)
            if step == 0:
                guard[case.id] = _guard(case, p, states, x_in, exact)
                ex_obs = RD.observables(exact, case)
                for f in RD.FAULTS:
                    if case.D > 1024 and best[f][0] >= 2.0:   # the wide cases only where something is still open
                        continue
                    bad = RD.ref_step(p, st, x_in, case, rounded=True, fault=f)
                    for (name, l, xf), (_, _, xe) in zip(RD.observables(bad, case), ex_obs):
                        ratio = (xf - xe).abs().max().item() / bars[(name, l)]["bar"]
                        if not math.isfinite(ratio):
                            ratio = float("inf")
                        if ratio > best[f][0]:
                            best[f] = (ratio, case.id, f"{name}[{l}]" if l is not None else name)
            st = [bf if i % 3 != 1 else bf.float() for i, bf in enumerate(rnd["states"])]
            x_in = emb[exact["logits"].argmax(-1)]
    return dict(guard=guard, skipped=skipped, total=total, best=best)


def test_case_list_covers_the_shapes_and_regimes():
    cs = RD.CASES
    assert {c.regime for c in cs} == set(RD.REGIMES)
    assert {c.D for c in cs} == {64, 128, 768, 1024, 2048, 4096}
    assert {c.B for c in cs} == {1, 2, 3, 31, 32}
    assert {c.L for c in cs} == {2, 3}
    assert {c.V for c in cs} == {77, 8193} and {c.bias for c in cs} == {True, False}
    assert all(len(set(c.ranks)) == 4 and sum(c.ranks) <= 512 and all(r in (32, 64, 96, 128, 160, 256) for r in c.ranks) for c in cs)
    assert any(max(c.ranks) > 128 for c in cs) and any(c.L == 3 and max(c.ranks) > 128 for c in cs)
    assert any(c.F == 320 for c in cs) and any(c.F >= 8192 and c.F != 4 * c.D for c in cs) and any(c.F == 4 * c.D for c in cs)
    for D in {c.D for c in cs}:   # every width: trained_like and a hard regime
        regs = {c.regime for c in cs if c.D == D}
        assert "trained_like" in regs and len(regs) >= 2, D
    for reg in RD.REGIMES:        # every regime: a small width and the 0.4B width
        Ds = {c.D for c in cs if c.regime == reg}
        assert 1024 in Ds and min(Ds) <= 128, reg
    assert len({c.id for c in cs}) == len(cs)


def test_regime_generator_guard(sweep):
    bad = {k: v for k, v in sweep["guard"].items() if v}
    assert not bad, bad


def test_every_planted_fault_is_beyond_twice_its_bar(sweep):
    print("\nfault                   ratio to bar   observable        case")
    for f in RD.FAULTS:
        ratio, cid, obs = sweep["best"][f]
        print(f"{f:22s} {ratio:13.1f}   {str(obs):16s}  {cid}")
    missed = [f for f in RD.FAULTS if not sweep["best"][f][0] >= 2.0]
    assert not missed, missed


def test_secondary_check_is_skipped_for_at_most_one_observable_in_four(sweep):
    print(f"\nsecondary check skipped (e_round <= floor) for {sweep['skipped']} of {sweep['total']} fp32 observables")
    assert 4 * sweep["skipped"] <= sweep["total"]
