"""Closed-form output laws used as yardsticks by the sampler tests (test infrastructure).  `exact_probs` is the float64 warper chain
the GPU distribution tests compare frequencies against (tests/test_sampling_gpu.py); tests/test_sampling.py ties it to the HF warpers
the reference's generate runs (transformers, requirements.txt:245) on CPU.  `ras_exact` is the law of the repetition-aware sampler; its
factors are also what the draw replay's candidate and whole-row laws are held against (tests/test_draw_replay.py)."""
import torch


def exact_probs(logits64, top_k, top_p, temperature):
    """the warper chain (temperature -> top-k -> top-p) in float64 on one row -> probability of every id"""
    x = logits64 / temperature
    if top_k > 0:
        kth = torch.topk(x, min(top_k, x.numel())).values[-1]
        x = x.masked_fill(x < kth, float("-inf"))
    if top_p < 1.0:
        sv, si = torch.sort(x, descending=False)
        cum = sv.softmax(-1).cumsum(-1)
        rem = cum <= (1 - top_p)
        rem[-1] = False
        x = x.masked_fill(torch.zeros_like(rem).scatter(0, si, rem), float("-inf"))
    return x.softmax(-1)


def ras_factors(logp64, recent, ignore_eos, eos, top_p, top_k, win, tau_r):
    """the factors of ras_exact: P(candidate = id) of the nucleus draw, the law of the whole-row draw that replaces a repeated
    candidate, and which candidates are replaced (1.0 / 0.0 per id)"""
    probs = logp64.softmax(0)
    sv, si = probs.sort(descending=True, stable=True)
    cum_before = sv.cumsum(0) - sv
    keep = ((cum_before < top_p) & (torch.arange(sv.numel()) < top_k)).long().cumprod(0).double()
    pk = sv * keep
    if ignore_eos:
        pk = pk.masked_fill(si == eos, 0.0)
        if pk.sum() == 0:
            pk = sv.masked_fill(si == eos, 0.0)
    pc = torch.zeros_like(probs).scatter(0, si, pk / pk.sum())          # P(candidate = id)
    full = probs.clone()
    if ignore_eos:
        full[eos] = 0
    full = full / full.sum()
    rep = torch.tensor([(recent == i).sum().item() for i in range(probs.numel())])
    redo = (rep >= win * tau_r).double()
    return pc, full, redo


def ras_exact(logp64, recent, ignore_eos, eos, top_p, top_k, win, tau_r):
    """probability of every output id of ras_sampling + EOS rejection (the semantics of cosy_llm.ras_sampling_device)"""
    pc, full, redo = ras_factors(logp64, recent, ignore_eos, eos, top_p, top_k, win, tau_r)
    return pc * (1 - redo) + (pc * redo).sum() * full
