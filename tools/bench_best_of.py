"""Best-of-n requests in the continuous decoder: what the drawn ids' log-probabilities cost per step and what the fork saves per
admission (0.4B Spark widths, synthetic weights, bf16, 32 slots, EOS disabled).  Two A/Bs, each inside one process and alternating,
repeated so that they show their own spread:

  * step cost: ms per replay of the captured step with 32 live slots, ContinuousDecoder(logprobs=True) against logprobs=False (the
    engine as it was), alternating blocks of replays.  Expectation (not a bar: the switch is opt-in): the difference stays inside
    the A/B's own spread plus 1 % of the step.
  * admission cost: one best-of-4 group by submit_n(4) against four submit() calls of the same prompt, device-synced around the
    admission, in eager and in graph admission.  No bar: the fan-out has not been measured before.

It also records the largest distance between -tok_lp and the teacher-forced per-token cross-entropy of the eager bf16 forward over
prompt + generated ids (greedy, 24 ids; a figure, not a bound: the decode step and the prefill kernels round differently).

    python tools/bench_best_of.py [--out profiles/best_of_bench.txt] [--rounds 5] [--replays 200] [--prompt 600]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch

from rwkvtts_amd import backbone
from rwkvtts_amd.continuous import ContinuousDecoder
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig

DEV = torch.device("cuda:0")


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def med_spread(v):
    return statistics.median(v), max(v) - min(v)


def step_cost(m, prompts, rounds, n):
    """ms per replay at 32 live slots, per engine: [logprobs=False], [logprobs=True], one entry per round, alternating"""
    engs = []
    for logprobs in (False, True):
        eng = ContinuousDecoder(m, slots=32, max_new_tokens_cap=2048, logprobs=logprobs)
        for i, p in enumerate(prompts):
            eng.submit(inputs_embeds=p, max_new_tokens=2048, do_sample=bool(i % 2), top_k=50, top_p=0.9, temperature=0.8, seed=i)
        eng._admit()
        engs.append(eng)

    def rep(g):
        for _ in range(n):
            g.replay()
    for eng in engs:
        wall(lambda: rep(eng.graph))   # warm-up
    res = ([], [])
    for _ in range(rounds):
        for eng, acc in zip(engs, res):
            acc.append(wall(lambda: rep(eng.graph)) / n * 1e3)
    assert all(int(eng.live.sum()) == 32 for eng in engs)
    return res


def admission_cost(m, prompt, mode, rounds):
    """ms of one admission (device-synced): [four submit() calls of one prompt], [one submit_n(4)], alternating"""
    eng = ContinuousDecoder(m, slots=32, max_new_tokens_cap=64, admission=mode, logprobs=True)
    if mode == "graph":
        eng.prefill.warm()

    def four():
        for i in range(4):
            eng.submit(inputs_embeds=prompt, max_new_tokens=2, do_sample=True, seed=100 + i)

    def fork():
        eng.submit_n(4, inputs_embeds=prompt, max_new_tokens=2, do_sample=True, seed=100)
    res = ([], [])
    for r in range(rounds + 1):   # round 0: warm-up
        for queue, acc in zip((four, fork), res):
            queue()
            t = wall(eng._admit)
            assert len(eng.sched.busy) == 4
            eng.run()
            if r:
                acc.append(t * 1e3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--prompt", type=int, default=600)
    a = ap.parse_args()
    c = backbone.config_0p4b()
    base = {k: v for k, v in c.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    base["vocab_size"] = 8193
    cfg = RWKV7SpeechConfig(**base)
    m = RWKV7ForSpeech(cfg).init_weights(0).to(DEV, torch.bfloat16).eval()
    g = torch.Generator().manual_seed(0)
    prompts = [(torch.randn(200, cfg.hidden_size, generator=g) * 0.5).to(DEV, torch.bfloat16) for _ in range(32)]
    prompt = (torch.randn(a.prompt, cfg.hidden_size, generator=g) * 0.5).to(DEV, torch.bfloat16)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"0.4B synthetic bf16, EOS off, 32 slots; {a.rounds} alternating rounds")
    off, on = step_cost(m, prompts, a.rounds, a.replays)
    (mo, so), (mn, sn) = med_spread(off), med_spread(on)
    say(f"captured step at 32 live slots, {a.replays} replays per block: logprobs=False {mo:.4f} ms (spread {so:.4f}) | "
        f"logprobs=True {mn:.4f} ms (spread {sn:.4f})")
    say("  rounds, False: " + " ".join(f"{v:.4f}" for v in off))
    say("  rounds, True : " + " ".join(f"{v:.4f}" for v in on))
    room = max(so, sn) + 0.01 * mo
    say(f"log-probabilities cost {mn - mo:+.4f} ms per step ({(mn - mo) / mo * 100:+.2f} %); expectation (A/B spread + 1 % of the step = "
        f"{room:.4f} ms): {'met' if mn - mo <= room else 'missed'}")
    for mode in ("eager", "graph"):
        four, fork = admission_cost(m, prompt, mode, a.rounds)
        (mf, sf), (mk, sk) = med_spread(four), med_spread(fork)
        say(f"best-of-4 of one {a.prompt}-token prompt, {mode} admission: four submit() {mf:.2f} ms (spread {sf:.2f}) | submit_n(4) {mk:.2f} ms "
            f"(spread {sk:.2f}) -> {mf / mk:.2f} x")
    from test_best_of_gpu import teacher_forced_gap
    eng = ContinuousDecoder(m, slots=32, max_new_tokens_cap=64, logprobs=True)
    hs = eng.submit_n(2, inputs_embeds=prompt[:200], max_new_tokens=24)
    out = eng.run()
    tok, cum = eng.take_logprobs(hs[0])
    say(f"greedy, 24 ids after a 200-token prompt: sum of log-probabilities {float(cum):.4f}; max |-tok_lp - teacher-forced CE of the eager "
        f"bf16 forward| = {teacher_forced_gap(m, prompt[:200], out[hs[0]], tok):.4f} (recorded, not a bound)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
