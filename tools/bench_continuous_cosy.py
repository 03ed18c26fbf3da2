"""Continuous batching for the Cosy model (synthetic weights, bf16, the stock repetition-aware sampler; EOS is barred through
n_ignore = limit so that every request runs to its max_len and both sides do the same work).

  * captured step: time per token of ContinuousCosyDecoder with 32 live slots against ContinuousDecoder's captured step on a causal
    model of the same widths and a head of the same number of rows, both as the difference of two run lengths (so prefill and
    capture cancel), in one process, alternating --repeats times; median and spread.  Bar: <= 1.02 x.  The difference between the
    two is one sampling launch against another, and the Cosy engine's read-back every 16 replays.
  * useful tokens/s: --requests utterances, prompts uniform in 50..300 rows, max_len uniform in 128..1024, 32 slots, under both
    admission modes, against sequential RWKV7CosyLM.inference calls (the only path without the engine); admission share of the wall
    time (a second run with a device sync around every admission).

    python tools/bench_continuous_cosy.py [--layers L] [--requests 128] [--baseline-requests N] [--repeats 3] [--skip-useful] [--out FILE]
"""
import argparse
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rwkvtts_amd import backbone
from rwkvtts_amd.continuous import ContinuousDecoder
from rwkvtts_amd.continuous_cosy import ContinuousCosyDecoder
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7CosyLM
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig

DEV = torch.device("cuda:0")
TEXT_VOCAB = 1000
N_TEXT = 20   # text ids of every utterance; the rest of a prompt is prompt speech


def base_kw(layers):
    c = backbone.config_0p4b()
    kw = {k: v for k, v in c.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    if layers:
        kw.update(num_hidden_layers=layers)
    return kw


def cosy_model(layers):
    kw = base_kw(layers)
    kw.update(vocab_size=TEXT_VOCAB)
    return RWKV7CosyLM(RWKV7CosyConfig(**kw)).init_weights(seed=0).to(DEV, torch.bfloat16).eval()


def causal_model(layers, head_rows):
    kw = base_kw(layers)
    kw.update(vocab_size=head_rows)
    return RWKV7ForSpeech(RWKV7SpeechConfig(**kw)).init_weights(0).to(DEV, torch.bfloat16).eval()


def utterance(rows, max_len, g, speech_ids):
    """An utterance whose prompt has `rows` rows and that runs to exactly max_len ids: the ratios put max_len and the EOS bar there."""
    text = torch.randint(0, TEXT_VOCAB, (1, N_TEXT), generator=g).to(DEV)
    speech = torch.randint(0, speech_ids, (1, rows - 2 - N_TEXT), generator=g).to(DEV)
    return dict(text=text, speech=speech, max_len=max_len, max_ratio=(max_len + 0.5) / N_TEXT, min_ratio=(max_len + N_TEXT + 0.5) / N_TEXT)


def workload(n, speech_ids, seed=0):
    rng, g = random.Random(seed), torch.Generator().manual_seed(seed)
    return [utterance(rng.randint(50, 300), rng.randint(128, 1024), g, speech_ids) for _ in range(n)]


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def submit(eng, u, seed):
    return eng.submit(text=u["text"], prompt_speech_token=u["speech"], max_token_text_ratio=u["max_ratio"],
                      min_token_text_ratio=u["min_ratio"], seed=seed)


def step_times(m, say, repeats, layers, n1=64, n2=576, rows=64):
    g = torch.Generator().manual_seed(1)
    V = m.lm_head.weight.shape[0]
    eng = ContinuousCosyDecoder(m, slots=32, max_len_cap=n2)
    mc = causal_model(layers, V)
    ref = ContinuousDecoder(mc, slots=32, max_new_tokens_cap=n2)
    prompts = [(torch.randn(rows, m.config.hidden_size, generator=g) * 0.5).to(DEV, torch.bfloat16) for _ in range(32)]

    def cosy(n):
        for i in range(32):
            submit(eng, utterance(rows, n, g, V - 1), i)
        t, out = wall(eng.run)
        assert all(v.numel() == n for v in out.values())
        return t

    def causal(n):
        for p in prompts:
            ref.submit(inputs_embeds=p, max_new_tokens=n, do_sample=True, top_k=25, top_p=0.8, seed=1)
        return wall(ref.run)[0]

    cosy(n1), causal(n1)   # warm-up
    te, ts = [], []
    for r in range(repeats):
        e = (cosy(n2) - cosy(n1)) / (n2 - n1) * 1e3
        s = (causal(n2) - causal(n1)) / (n2 - n1) * 1e3
        te.append(e)
        ts.append(s)
        say(f"  round {r}: ContinuousCosyDecoder {e:.4f} ms/step, ContinuousDecoder {s:.4f} ms/step -> {e / s:.3f} x")
    me, ms = statistics.median(te), statistics.median(ts)
    say(f"captured step, 32 live slots, head of {V} rows: Cosy engine {me:.4f} ms (spread {max(te) - min(te):.4f}), causal engine "
        f"{ms:.4f} ms (spread {max(ts) - min(ts):.4f}) -> {me / ms:.3f} x; bar <= 1.02 x: {'met' if me <= 1.02 * ms else 'MISSED'}")
    del ref, mc


def sequential_inference(m, reqs):
    """What exists without the engine: one RWKV7CosyLM.inference call after the other."""
    def run():
        total = 0
        for u in reqs:
            z = torch.zeros(1, 0, dtype=torch.int64, device=DEV)
            n = sum(1 for _ in m.inference(u["text"], torch.tensor([N_TEXT], device=DEV), z, torch.tensor([0], device=DEV), u["speech"],
                                           torch.tensor([u["speech"].shape[1]], device=DEV), max_token_text_ratio=u["max_ratio"],
                                           min_token_text_ratio=u["min_ratio"]))
            assert n == u["max_len"], (n, u["max_len"])
            total += n
        return total
    return wall(run)


def engine_run(m, reqs, admission, time_admission=False):
    eng = ContinuousCosyDecoder(m, slots=32, max_len_cap=1024, admission=admission)
    if admission == "graph":
        eng.prefill.warm()   # every bucket captured before the timed window
    spent = [0.0, 0]
    if time_admission:
        inner = eng._admit

        def timed_admit():
            if not (eng.sched.pending and eng.sched.free):
                return
            torch.cuda.synchronize()
            t = time.perf_counter()
            inner()
            torch.cuda.synchronize()
            spent[0] += time.perf_counter() - t
            spent[1] += 1
        eng._admit = timed_admit

    def run():
        hs = [submit(eng, u, i) for i, u in enumerate(reqs)]
        out = eng.run()
        assert all(out[h].numel() == u["max_len"] for h, u in zip(hs, reqs))
        return eng.replays
    sec, replays = wall(run)
    return sec, replays, spent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0, help="depth (default: the configuration's 24)")
    ap.add_argument("--requests", type=int, default=128)
    ap.add_argument("--baseline-requests", type=int, default=0, help="utterances of the sequential baseline (default: all)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-useful", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m = cosy_model(a.layers)
    cfg = m.config
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"Cosy 0.4B widths (D = {cfg.hidden_size}, {cfg.num_hidden_layers} layers, head of {cfg.speech_token_size + 1} rows), synthetic bf16, "
        f"repetition-aware sampling (top_k 25, top_p 0.8, win 10, tau_r 0.1), EOS barred; 32 slots")
    step_times(m, say, a.repeats, a.layers)
    if not a.skip_useful:
        reqs = workload(a.requests, cfg.speech_token_size)
        useful = sum(u["max_len"] for u in reqs)
        say(f"{len(reqs)} utterances, prompts 50..300 rows (mean {statistics.mean(u['speech'].shape[1] + 2 + N_TEXT for u in reqs):.0f}), max_len "
            f"128..1024 (mean {useful / len(reqs):.0f})")
        engine_run(m, reqs[:4], "eager")   # warm-up
        sequential_inference(m, reqs[:1])
        base = reqs[:a.baseline_requests] if a.baseline_requests else reqs
        tb, nb = sequential_inference(m, base)
        rate_b = nb / tb
        say(f"sequential inference() ({len(base)} utterances): {tb:8.2f} s {rate_b:9.0f} useful tokens/s")
        for mode in ("eager", "graph"):
            te, replays, _ = engine_run(m, reqs, mode)
            ta, _, sp = engine_run(m, reqs, mode, time_admission=True)
            say(f"ContinuousCosyDecoder ({mode:5s})     : {te:8.2f} s {useful / te:9.0f} useful tokens/s ({useful / (replays * 32) * 100:.1f} % of "
                f"slot-steps useful, {replays} replays) -> {useful / te / rate_b:.1f} x sequential; admission {sp[0] / ta * 100:.1f} % of "
                f"{ta:.2f} s synced wall ({sp[1]} admissions, {sp[0] / max(sp[1], 1) * 1e3:.1f} ms each)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
