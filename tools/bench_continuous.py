"""Continuous batching against static batching (0.4B Spark widths, synthetic weights, bf16, greedy, EOS disabled so that every
request runs to its budget and the run is deterministic): 128 requests, prompts uniform in 200..1000 tokens, max_new_tokens uniform
in 128..2048, 32 slots.

  * useful tokens/s (tokens within each request's budget, prefill included in the wall time) of static GraphDecoder groups of 32 in
    submission order (each group runs to its longest budget) and of ContinuousDecoder;
  * the captured step at 32 live slots, engine against GraphDecoder (fused tail), interleaved in one process;
  * the share of the engine's wall time spent in admission (a second run with a device sync around every admission);
  * MultiGroupDecoder(4 x 32) on the same requests, for context.

    python tools/bench_continuous.py [--requests 128] [--out FILE] [--admission eager|graph|both] [--repeats 3]

--admission graph / both: ContinuousDecoder(admission="graph") (prefill.PackedPrefill) instead of / alternating with the eager
admission, in one process on the same workload, every bucket captured before the timed window.  `both` prints per mode the median
and the repeat-to-repeat spread (max - min over the alternations) of useful tokens/s, time per admission (device-synced), the
admission share of the wall time, and the device kernels the profiler counts inside one admission of eight prompts.
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
from rwkvtts_amd.decode import GraphDecoder, MultiGroupDecoder
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig

DEV = torch.device("cuda:0")


def workload(n, D, seed=0):
    rng = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    reqs = []
    for _ in range(n):
        T, budget = rng.randint(200, 1000), rng.randint(128, 2048)
        reqs.append(((torch.randn(T, D, generator=g) * 0.5).to(DEV, torch.bfloat16), budget))
    return reqs


def left_pad(prompts):
    T = max(p.shape[0] for p in prompts)
    x = torch.zeros(len(prompts), T, prompts[0].shape[1], dtype=torch.bfloat16, device=DEV)
    mask = torch.zeros(len(prompts), T, dtype=torch.long, device=DEV)
    for i, p in enumerate(prompts):
        x[i, T - p.shape[0]:] = p
        mask[i, T - p.shape[0]:] = 1
    return x, mask


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def static_groups(m, reqs, G=32):
    def run():
        for a in range(0, len(reqs), G):
            grp = reqs[a:a + G]
            x, mask = left_pad([p for p, _ in grp])
            GraphDecoder(m, len(grp), step_kernel=True).generate(inputs_embeds=x, attention_mask=mask,
                                                                 max_new_tokens=max(b for _, b in grp))
    return wall(run)[0]


def engine(m, reqs, slots=32, time_admission=False, admission="eager"):
    eng = ContinuousDecoder(m, slots=slots, max_new_tokens_cap=2048, admission=admission)
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
        hs = [eng.submit(inputs_embeds=p, max_new_tokens=b) for p, b in reqs]
        out = eng.run()
        assert all(out[h].numel() == b for h, (_, b) in zip(hs, reqs))
        return eng.replays
    sec, replays = wall(run)
    return sec, replays, spent


def admission_launches(m, reqs, admission):
    """Kernels the profiler sees on the device inside ONE admission of eight prompts (a graph replay's kernels are traced too)."""
    from torch.profiler import ProfilerActivity, profile
    eng = ContinuousDecoder(m, slots=8, max_new_tokens_cap=2048, admission=admission)
    if admission == "graph":
        eng.prefill.warm()
    for p, _ in reqs[:8]:
        eng.submit(inputs_embeds=p, max_new_tokens=4)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        eng._admit()
        torch.cuda.synchronize()
    n = sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None and "Memcpy" not in e.key and "Memset" not in e.key
            and (getattr(e, "device_time_total", 0) or getattr(e, "cuda_time_total", 0)) > 0)
    eng.run()
    return n


def compare(m, reqs, useful, say, repeats):
    """eager and graph admission alternately, `repeats` times each: an unsynced run (tokens/s) and a synced one (admission time)."""
    res = {"eager": [], "graph": []}
    for r in range(repeats):
        for mode in ("eager", "graph"):
            te, replays, _ = engine(m, reqs, admission=mode)
            ta, _, sp = engine(m, reqs, time_admission=True, admission=mode)
            adm, n_adm = sp[0], sp[1]
            res[mode].append((useful / te, adm / max(n_adm, 1) * 1e3, adm / ta * 100, n_adm, replays))
            say(f"  round {r} {mode:5s}: {te:6.2f} s {useful / te:8.0f} useful tokens/s | admission {adm / max(n_adm, 1) * 1e3:6.2f} ms each "
                f"({n_adm}), {adm / ta * 100:5.1f} % of {ta:.2f} s synced wall")
    med = lambda mode, i: statistics.median(x[i] for x in res[mode])
    spr = lambda mode, i: max(x[i] for x in res[mode]) - min(x[i] for x in res[mode])
    for mode in ("eager", "graph"):
        say(f"{mode:5s} admission: {med(mode, 0):8.0f} useful tokens/s (spread {spr(mode, 0):.0f}) | {med(mode, 1):6.2f} ms per admission "
            f"(spread {spr(mode, 1):.2f}) | {med(mode, 2):5.1f} % of the wall (spread {spr(mode, 2):.1f})")
    for mode in ("eager", "graph"):
        try:
            say(f"kernel launches in one admission of 8 prompts, {mode} (profiler, device kernels): {admission_launches(m, reqs, mode)}")
        except Exception as e:   # the profiler is optional equipment
            say(f"kernel launches per admission, {mode}: not counted ({type(e).__name__}: {e})")
    s_t, s_a, s_w = (max(spr("eager", i), spr("graph", i)) for i in range(3))
    say(f"time per admission lower by more than the spread: {med('eager', 1) - med('graph', 1) > s_a} "
        f"({med('eager', 1):.2f} -> {med('graph', 1):.2f} ms, spread {s_a:.2f})")
    say(f"admission share lower by more than the spread   : {med('eager', 2) - med('graph', 2) > s_w} "
        f"({med('eager', 2):.1f} -> {med('graph', 2):.1f} %, spread {s_w:.1f})")
    say(f"useful tokens/s not below eager's minus spread  : {med('graph', 0) >= med('eager', 0) - s_t} "
        f"({med('eager', 0):.0f} -> {med('graph', 0):.0f}, spread {s_t:.0f})")
    return med("graph", 0)


def step_times(m, reqs, rounds=5, n=200):
    """ms per replay of the captured step with 32 live slots: engine vs GraphDecoder, alternating blocks of n replays."""
    eng = ContinuousDecoder(m, slots=32, max_new_tokens_cap=2048)
    for p, _ in reqs[:32]:
        eng.submit(inputs_embeds=p[:200], max_new_tokens=2048)
    eng._admit()
    x, mask = left_pad([p[:200] for p, _ in reqs[:32]])
    gd = GraphDecoder(m, 32, step_kernel=True)
    gd.prepare(inputs_embeds=x, attention_mask=mask, max_new_tokens=2048)
    assert gd.tail is not None
    te, tg = [], []
    for _ in range(rounds):
        for g, acc in ((eng.graph, te), (gd.graph, tg)):
            def rep():
                for _ in range(n):
                    g.replay()
            acc.append(wall(rep)[0] / n * 1e3)
    live = int(eng.live.sum())
    return statistics.median(te), statistics.median(tg), live


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=128)
    ap.add_argument("--out", default=None)
    ap.add_argument("--admission", choices=("eager", "graph", "both"), default="eager")
    ap.add_argument("--repeats", type=int, default=3, help="alternations of --admission both (at least three for a spread)")
    a = ap.parse_args()
    c = backbone.config_0p4b()
    base = {k: v for k, v in c.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    base["vocab_size"] = 8193
    cfg = RWKV7SpeechConfig(**base)
    m = RWKV7ForSpeech(cfg).init_weights(0).to(DEV, torch.bfloat16).eval()
    reqs = workload(a.requests, cfg.hidden_size)
    useful = sum(b for _, b in reqs)
    lines = [f"0.4B synthetic bf16 greedy, EOS off; {len(reqs)} requests, prompts 200..1000 (mean "
             f"{statistics.mean(p.shape[0] for p, _ in reqs):.0f}), max_new_tokens 128..2048 (mean {useful / len(reqs):.0f}); 32 slots"]

    def say(s):
        print(s, flush=True)
        lines.append(s)
    print(lines[0], flush=True)
    # warm-up: kernels, graph pools, the packed prefill's first calls
    mode = "graph" if a.admission == "graph" else "eager"
    engine(m, reqs[:4], slots=4, admission=mode)
    static_groups(m, reqs[:2], G=2)
    ts = static_groups(m, reqs)
    say(f"static GraphDecoder groups of 32: {ts:8.2f} s  {useful / ts:9.0f} useful tokens/s")
    te, replays, _ = engine(m, reqs, admission=mode)
    say(f"ContinuousDecoder, 32 slots ({mode}): {te:8.2f} s  {useful / te:9.0f} useful tokens/s  ({replays} replays, "
        f"{useful / (replays * 32) * 100:.1f} % of slot-steps useful)  -> {ts / te:.2f} x static")
    ta, _, sp = engine(m, reqs, time_admission=True, admission=mode)
    adm, n_adm = sp[0], sp[1]
    say(f"admission (synced run)          : {adm:8.2f} s of {ta:.2f} s wall = {adm / ta * 100:.1f} %  ({n_adm} admissions, "
        f"{adm / max(n_adm, 1) * 1e3:.1f} ms each)")
    if a.admission == "both":
        say(f"eager and graph admission, alternating, {a.repeats} rounds:")
        tg = compare(m, reqs, useful, say, a.repeats)
        say(f"graph admission against static groups: {tg / (useful / ts):.2f} x (bar of DESIGN.md 7.1: >= 1.4 x: "
            f"{'met' if tg / (useful / ts) >= 1.4 else 'missed'})")
    se, sg, live = step_times(m, reqs)
    say(f"captured step at {live} live slots: engine {se:.3f} ms, GraphDecoder (fused tail) {sg:.3f} ms -> {se / sg:.3f} x")
    mg = MultiGroupDecoder(m, 32, step_kernel=True)
    x, mask = left_pad([p for p, _ in reqs])
    tm = wall(lambda: mg.generate(inputs_embeds=x, attention_mask=mask, max_new_tokens=max(b for _, b in reqs)))[0]
    say(f"MultiGroupDecoder(4 x 32), context: {tm:8.2f} s  {useful / tm:9.0f} useful tokens/s")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
