"""GPU (-m gpu): the decode-step kernel (csrc/decode_step.hip through decode.DecodeStep, host-table entry) against the fp64
restatement of one step in tests/ref_decode_step.py, observable by observable and layer by layer, in the regimes and shapes of
ref_decode_step.CASES.

Per case: an RWKV7ForCausalLM holding the generator's parameters (so DecodeStep's own table building is under test), the cache
filled with the generator's states, three consecutive steps.  Every step is compared with the reference started FROM THE STATE
THE KERNEL ITSELF HAD BEFORE THAT STEP, so every bar is a one-step bar; steps 2 and 3 read what step 1 wrote.  The next input row
is the embedding of the exact reference's argmax.

Bars (ref_decode_step.bars; nothing tuned on the kernel): max |X_hip - X_exact| <= 2 e_round(X) + floor(X) on every element of
every observable, all values finite.  Secondary, on the fp32 observables (att_kv, logits) where e_round > floor: the kernel is
closer in RMS to the rounded reference than to the exact one.

Each case prints `RATIO <case> <observable> <max over layers and steps of max|X_hip - X_exact| / bar>`; the record of one run is
profiles/decode_step_parity.txt."""
import pytest
import torch

import ref_decode_step as RD
from rwkvtts_amd.backbone import Cache, RWKV7Config, RWKV7ForCausalLM
from rwkvtts_amd.decode import DecodeStep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 3


def _build(case, p):
    cfg = RWKV7Config(hidden_size=case.D, num_hidden_layers=case.L, vocab_size=case.V, decay_low_rank_dim=case.ranks[0],
                      a_low_rank_dim=case.ranks[1], v_low_rank_dim=case.ranks[2], gate_low_rank_dim=case.ranks[3],
                      intermediate_size=case.F)
    m = RWKV7ForCausalLM(cfg, head_bias=case.bias)
    m.load_state_dict(p, strict=True)
    return cfg, m.to(DEV).to(torch.bfloat16).eval()


def _read(cache):
    """the cache as the reference takes it: [att_x_prev, att_kv, ffn_x_prev] * L on the CPU (bf16 rows as fp32 values)"""
    out = []
    for s in cache.states:
        out += [s.att_x_prev.float().cpu(), s.att_kv.cpu().clone(), s.ffn_x_prev.float().cpu()]
    return out


def _rms(x):
    return x.pow(2).mean().sqrt().item()


def _diagnose(case, name, l, idx, hip, rnd, exact):
    """layer, observable, worst (sequence, channel), the triple (HIP, rounded, exact), and the reference's intermediates there"""
    xr = dict((n, t) for n, ll, t in RD.observables(rnd, case) if ll == l)[name]
    xe = dict((n, t) for n, ll, t in RD.observables(exact, case) if ll == l)[name]
    msg = f"layer {l} {name} worst at {idx}: hip {hip[idx].item():.9g} rounded {xr[idx].item():.9g} exact {xe[idx].item():.9g}"
    if l is None:
        return msg
    b = idx[0]
    if name == "att_kv":       # (sequence, head, value row i, key column j)
        chans = dict(w=idx[1] * RD.N + idx[3], a=idx[1] * RD.N + idx[3], kk=idx[1] * RD.N + idx[3], k2=idx[1] * RD.N + idx[3],
                     v=idx[1] * RD.N + idx[2], y=idx[1] * RD.N + idx[2])
    else:
        chans = {k: idx[1] for k in ("w", "a", "kk", "k2", "v", "y")}
    parts = [f"{k}[{b},{c}] rounded {rnd['inter'][l][k][b, c].item():.9g} exact {exact['inter'][l][k][b, c].item():.9g}"
             for k, c in chans.items()]
    return msg + "\n    reference intermediates of that layer: " + "; ".join(parts)


@pytest.mark.parametrize("case", RD.CASES, ids=lambda c: c.id)
def test_decode_step_against_fp64_reference(case):
    p, states, ids = RD.make_case(case)
    cfg, model = _build(case, p)
    emb = p["model.embeddings.weight"]
    p64 = {k: v.double() for k, v in p.items()}
    cache = Cache.zeros(cfg, case.B, DEV, torch.bfloat16)
    for i, s in enumerate(cache.states):
        s.att_x_prev.copy_(states[3 * i].to(torch.bfloat16))
        s.att_kv.copy_(states[3 * i + 1])
        s.ffn_x_prev.copy_(states[3 * i + 2].to(torch.bfloat16))
    assert DecodeStep.supported(model.model, model.lm_head, cache) is None
    step = DecodeStep(model.model, model.lm_head, cache)
    x_in = emb[ids]
    failures, worst_ratio, skipped, checked = [], {}, 0, 0
    for it in range(STEPS):
        before = _read(cache)
        logits = step(x_in.to(DEV).to(torch.bfloat16).contiguous()).double().cpu()
        torch.cuda.synchronize()
        after = _read(cache)
        exact = RD.ref_step(p64, before, x_in, case, rounded=False)
        rnd = RD.ref_step(p64, before, x_in, case, rounded=True)
        bars = RD.bars(exact, rnd, before, case)
        hip = {("logits", None): logits}
        for l in range(case.L):
            hip[("att_x_prev", l)], hip[("att_kv", l)], hip[("ffn_x_prev", l)] = (t.double() for t in after[3 * l:3 * l + 3])
        for (name, l, xe), (_, _, xr) in zip(RD.observables(exact, case), RD.observables(rnd, case)):
            xh, b = hip[(name, l)], bars[(name, l)]
            assert xh.shape == xe.shape
            if not torch.isfinite(xh).all():
                failures.append(f"step {it} layer {l} {name}: non-finite values")
                continue
            err, idx = RD.worst(xh, xe)
            ratio = err / b["bar"]
            worst_ratio[name] = max(worst_ratio.get(name, 0.0), ratio)
            if err > b["bar"]:
                failures.append(f"step {it}: error {err:.4g} > bar {b['bar']:.4g} (e_round {b['e_round']:.4g}, floor {b['floor']:.4g})\n    "
                                + _diagnose(case, name, l, idx, xh, rnd, exact))
            if name in ("att_kv", "logits"):
                if RD.rms_check_applies(b):
                    checked += 1
                    to_r, to_e = _rms(xh - xr), _rms(xh - xe)
                    worst_ratio["rms " + name] = max(worst_ratio.get("rms " + name, 0.0), to_r / to_e)
                    if not to_r < to_e:
                        failures.append(f"step {it} layer {l} {name}: rms to rounded {to_r:.4g} >= rms to exact {to_e:.4g}")
                else:
                    skipped += 1
        x_in = emb[exact["logits"].argmax(-1)]
    for name, r in worst_ratio.items():
        print(f"RATIO {case.id} {name} {r:.3f}")
    print(f"RATIO {case.id} secondary check applied to {checked}, skipped for {skipped} fp32 observables")
    assert not failures, "\n".join(failures[:12]) + (f"\n... {len(failures)} failures" if len(failures) > 12 else "")
