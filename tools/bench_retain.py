"""What retaining finished requests' states costs and saves (0.4B Spark widths, synthetic weights, bf16, EOS off, 32 slots), all in
one process with alternating rounds:

  * captured step: ContinuousDecoder(retain=True) with nothing armed against retain=False, all 32 slots live: blocks of replays,
    host-timed over a synced block.  The difference is the price of the switch: one rwkv7_cache_rows_retain_bf16 launch per step
    whose workgroups read three flags and return.  (The retain=False step is not timed against an earlier build: its launches are
    the same ones.)
  * finishing step: the replay in which 1 slot, or all 32, end and are copied into the store, against the replays around it
    (device events around every replay);
  * turn two: admission of submit(state=retained, input_ids=[last id] + 32 new ids) against admission of the whole conversation
    (512-token prompt + 512 generated ids + the 32 new ids) from zero, eager and graph admission, wall time around the admission
    with a device sync on both sides.

    python tools/bench_retain.py [--rounds 5] [--out profiles/retain_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rwkvtts_amd import backbone
from rwkvtts_amd.continuous import ContinuousDecoder
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
from rwkvtts_amd.state_store import StateStore

DEV = torch.device("cuda:0")
SLOTS, V = 32, 8193


def ids(n, seed):
    return torch.randint(0, V - 1, (n,), generator=torch.Generator().manual_seed(seed))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def med_spread(xs):
    return statistics.median(xs), max(xs) - min(xs)


def replays(eng, n):
    """n replays outside step(), the scheduler's counters kept right: per-replay device times in ms."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for i in range(n):
        eng.graph.replay()
        ev[i + 1].record()
    torch.cuda.synchronize()
    eng.replays += n
    eng.sched.advance(n)
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]


def step_cost(m, say, rounds, block=200):
    engs = {}
    for retain in (False, True):
        eng = ContinuousDecoder(m, slots=SLOTS, max_new_tokens_cap=3000, state_store=StateStore(m, 1), retain=retain)
        for i in range(SLOTS):
            eng.submit(input_ids=ids(16, i), max_new_tokens=3000)
        eng._admit()
        replays(eng, 50)   # warm
        engs[retain] = eng
    t = {False: [], True: []}
    for _ in range(rounds):
        for retain in (False, True):
            t[retain].append(wall(lambda: replays(engs[retain], block))[0] / block * 1e6)
    (a, sa), (b, sb) = med_spread(t[False]), med_spread(t[True])
    diffs = [y - x for x, y in zip(t[False], t[True])]
    say(f"captured step, {SLOTS} live slots, nothing armed ({rounds} alternating blocks of {block} replays, synced wall per replay): "
        f"retain=False {a:.1f} us (spread {sa:.1f}) | retain=True {b:.1f} us (spread {sb:.1f}) | difference {b - a:+.1f} us "
        f"({(b - a) / a * 100:+.2f} %), per-round differences {min(diffs):+.1f} .. {max(diffs):+.1f} us")
    say("  the retain=False step issues the launches it issued before this switch existed; it is not timed against an earlier build")


def finishing_step(m, say, rounds, budget=8, window=14):
    store = StateStore(m, SLOTS)
    eng = ContinuousDecoder(m, slots=SLOTS, max_new_tokens_cap=64, state_store=store, retain=True)
    res = {}
    for ending in (1, SLOTS):
        fin, rest = [], []
        for r in range(rounds + 1):   # round 0 warms
            for i in range(SLOTS):
                kw = dict(max_new_tokens=budget, retain=f"s{i}") if i < ending else dict(max_new_tokens=64)
                eng.submit(input_ids=ids(16, 100 + i), **kw)
            eng._admit()
            ms = replays(eng, window)
            eng.run()
            assert store.names() == [f"s{i}" for i in range(ending)]
            for n in store.names():
                store.evict(n)
            if r:
                fin.append(ms[budget - 2] * 1e3)   # replay j draws id j + 1: the budget's last id comes with replay budget - 2
                rest.append(statistics.median(ms[:budget - 2] + ms[budget - 1:]) * 1e3)
        res[ending] = (med_spread(fin), med_spread(rest))
    row = m.config.num_hidden_layers * (2 * m.config.hidden_size * 2 + m.config.num_heads * 64 * 64 * 4)
    for ending, ((f, sf), (o, so)) in res.items():
        say(f"finishing step, {ending:2d} of {SLOTS} slots end and are copied ({row * ending / 1e6:.2f} MB): {f:.1f} us (spread {sf:.1f}) | the "
            f"replays around it {o:.1f} us (spread {so:.1f}) | difference {f - o:+.1f} us  ({rounds} rounds, device events)")


def turn_two(m, say, rounds, admission):
    store = StateStore(m, 2)
    eng = ContinuousDecoder(m, slots=SLOTS, max_new_tokens_cap=512, admission=admission, state_store=store, retain=True)
    if admission == "graph":
        eng.prefill.warm()
    prompt, new = ids(512, 7), ids(32, 8)
    h = eng.submit(input_ids=prompt, max_new_tokens=512, retain="turn1")
    out = eng.run()[h].cpu()
    assert store.tokens[store.row("turn1")] == 512 + 511
    variants = {"state": dict(state="turn1", input_ids=torch.cat([out[-1:], new])), "whole": dict(input_ids=torch.cat([prompt, out, new]))}
    t = {k: [] for k in variants}
    for r in range(rounds + 1):   # round 0 warms
        for name, kw in variants.items():
            eng.submit(max_new_tokens=1, **kw)
            sec = wall(eng._admit)[0]
            eng.run()
            if r:
                t[name].append(sec * 1e3)
    (a, sa), (b, sb) = med_spread(t["state"]), med_spread(t["whole"])
    say(f"turn-two admission, {admission:5s}: from the retained state (1 + 32 tokens) {a:.2f} ms (spread {sa:.2f}) | the whole conversation "
        f"from zero (512 + 512 + 32 tokens) {b:.2f} ms (spread {sb:.2f}) -> {b / a:.2f} x  ({rounds} alternating rounds)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = backbone.config_0p4b()
    base = {k: v for k, v in c.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    base["vocab_size"] = V
    cfg = RWKV7SpeechConfig(**base)
    m = RWKV7ForSpeech(cfg).init_weights(0).to(DEV, torch.bfloat16).eval()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"0.4B synthetic bf16 (L = {cfg.num_hidden_layers}, D = {cfg.hidden_size}), greedy, EOS off, {SLOTS} slots")
    step_cost(m, say, a.rounds)
    finishing_step(m, say, a.rounds)
    for admission in ("eager", "graph"):
        turn_two(m, say, a.rounds, admission)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
