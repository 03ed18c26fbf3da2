"""Best-of-n in the XY engine: what the frames' log-probabilities cost per step and what the fork saves per admission (0.4B widths,
8 channels, V0 = 66 661, 1 025 speech ids, synthetic weights, bf16, 32 slots, no EOS id so that every slot stays live).  Three
measurements, each inside one process with alternating rounds, so that they show their own spread:

  (a) step cost: ms per replay of the captured step with 32 live slots, ContinuousXYDecoder(logprobs=True) against logprobs=False
      (the engine as it was: its two launches are the LP = false instantiations), alternating blocks of replays.  No bar: the
      switch is opt-in.
  (b) admission cost: one best-of-4 group by submit_n(4) (one prefill plus the fan-out) against four submit() calls of the same
      prompt, device-synced around the admission, in eager and in graph admission.
  (c) the fan-out launch alone: rwkv7_cache_rows_commit_bf16 copying one row to three siblings over the engine's own cache table.

    python tools/bench_xy_best_of.py [--layers L] [--out profiles/xy_best_of_bench.txt] [--rounds 5] [--replays 200] [--prompt 600]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rwkvtts_amd import backbone
from rwkvtts_amd.continuous_xy import ContinuousXYDecoder
from rwkvtts_amd.prefill import cache_field_table, cache_rows_commit
from rwkvtts_amd.xy_llm import RWKV7XYConfig, RWKV7XYLM

DEV = torch.device("cuda:0")
SAMPLING = dict(do_sample=True, top_k=50, top_p=0.95, temperature=0.8)


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
    cap = (rounds + 2) * n + 8
    engs = []
    for logprobs in (False, True):
        eng = ContinuousXYDecoder(m, slots=32, max_new_frames_cap=cap, logprobs=logprobs)
        for i, p in enumerate(prompts):
            eng.submit(p, max_new_frames=cap, seed=i, **SAMPLING)
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
    assert torch.equal(engs[0].seq, engs[1].seq), "logprobs=True changed a frame"
    return res


def admission_cost(m, prompt, mode, rounds):
    """ms of one admission (device-synced): [four submit() calls of one prompt], [one submit_n(4)], alternating"""
    eng = ContinuousXYDecoder(m, slots=32, max_new_frames_cap=64, admission=mode, logprobs=True)
    if mode == "graph":
        eng.prefill.warm()

    def four():
        for i in range(4):
            eng.submit(prompt, max_new_frames=2, seed=100 + i, **SAMPLING)

    def fork():
        eng.submit_n(4, prompt, max_new_frames=2, seed=100, **SAMPLING)
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


def fan_out_alone(m, rounds, n=50):
    """us per rwkv7_cache_rows_commit_bf16 launch that copies row 0 to rows 1..3 of a 32-row cache, n launches per round"""
    eng = ContinuousXYDecoder(m, slots=32, max_new_frames_cap=8)
    tbl = cache_field_table(eng.cache)
    rows = torch.tensor([[0, 0, 0], [1, 2, 3]], dtype=torch.int32, device=DEV)
    cfg = m.config

    def go():
        for _ in range(n):
            cache_rows_commit(tbl, tbl, rows[0], rows[1], 3, len(eng.cache), cfg.hidden_size, cfg.num_heads)
    wall(go)
    return [wall(go) / n * 1e6 for _ in range(rounds)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0, help="depth (default: the configuration's 24)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--prompt", type=int, default=600)
    a = ap.parse_args()
    c = backbone.config_0p4b()
    kw = {k: v for k, v in c.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    kw.update(vocab_size=66661, speech_vocab_size=1025, num_channels=8, text_shift_size=65536)
    if a.layers:
        kw.update(num_hidden_layers=a.layers)
    m = RWKV7XYLM(RWKV7XYConfig(**kw)).init_weights(seed=0)
    m.zero_embs()
    m = m.to(DEV).to(torch.bfloat16).eval()
    cfg = m.config
    g = torch.Generator().manual_seed(0)

    def ids(t):
        ch0 = torch.randint(0, cfg.text_shift_size + cfg.speech_vocab_size, (t, 1), generator=g)
        return torch.cat([ch0, torch.randint(0, cfg.speech_vocab_size - 1, (t, cfg.num_channels - 1), generator=g)], 1).to(DEV)
    prompts = [ids(200) for _ in range(32)]
    prompt = ids(a.prompt)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"XY 0.4B widths (D = {cfg.hidden_size}, {cfg.num_hidden_layers} layers, {cfg.num_channels} channels, concatenated head of "
        f"{cfg.speech_vocab_size * cfg.num_channels} rows), synthetic bf16, top_k 50 / top_p 0.95 / temperature 0.8, no EOS id; 32 slots; "
        f"{a.rounds} alternating rounds")
    off, on = step_cost(m, prompts, a.rounds, a.replays)
    (mo, so), (mn, sn) = med_spread(off), med_spread(on)
    say(f"(a) captured step at 32 live slots, {a.replays} replays per block: logprobs=False {mo:.4f} ms (spread {so:.4f}) | "
        f"logprobs=True {mn:.4f} ms (spread {sn:.4f})")
    say("  rounds, False: " + " ".join(f"{v:.4f}" for v in off))
    say("  rounds, True : " + " ".join(f"{v:.4f}" for v in on))
    say(f"  log-probabilities cost {mn - mo:+.4f} ms per step ({(mn - mo) / mo * 100:+.2f} %); the A/B's own spread is {max(so, sn):.4f} ms: "
        f"{'inside it' if abs(mn - mo) <= max(so, sn) else 'OUTSIDE it'}")
    for mode in ("eager", "graph"):
        four, fork = admission_cost(m, prompt, mode, a.rounds)
        (mf, sf), (mk, sk) = med_spread(four), med_spread(fork)
        say(f"(b) best-of-4 of one {a.prompt}-frame prompt, {mode} admission: four submit() {mf:.2f} ms (spread {sf:.2f}) | submit_n(4) {mk:.2f} ms "
            f"(spread {sk:.2f}) -> {mf / mk:.2f} x")
    fan = fan_out_alone(m, a.rounds)
    mf, sf = med_spread(fan)
    say(f"(c) fan-out alone (one row to three siblings, every field of {cfg.num_hidden_layers} layers, 50 launches per round): {mf:.1f} us per "
        f"launch (spread {sf:.1f})")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
