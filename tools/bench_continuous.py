"""Continuous batching against static batching (0.4B Spark widths, synthetic weights, bf16, greedy, EOS disabled so that every
request runs to its budget and the run is deterministic): 128 requests, prompts uniform in 200..1000 tokens, max_new_tokens uniform
in 128..2048, 32 slots.

  * useful tokens/s (tokens within each request's budget, prefill included in the wall time) of static GraphDecoder groups of 32 in
    submission order (each group runs to its longest budget) and of ContinuousDecoder;
  * the captured step at 32 live slots, engine against GraphDecoder (fused tail), interleaved in one process;
  * the share of the engine's wall time spent in admission (a second run with a device sync around every admission);
  * MultiGroupDecoder(4 x 32) on the same requests, for context.

    python tools/bench_continuous.py [--requests 128] [--out FILE] [--admission eager|graph|both|overlap|all] [--repeats 3]

--admission graph / both: ContinuousDecoder(admission="graph") (prefill.PackedPrefill) instead of / alternating with the eager
admission, in one process on the same workload, every bucket captured before the timed window.  `both` prints per mode the median
and the repeat-to-repeat spread (max - min over the alternations) of useful tokens/s, time per admission (device-synced), the
admission share of the wall time, and the device kernels the profiler counts inside one admission of eight prompts.

--admission overlap / all: ContinuousDecoder(admission="overlap") (the prefill on a side stream next to the replays, committed by
rwkv7_cache_rows_commit_bf16) alone / alternating with eager and graph admission.  Per round an untimed-inside run gives useful
tokens/s and an instrumented run (an event pair around every commit and around every replay) gives the share of the wall time during
which the decode stream was stopped for admission and the mean step time of the replays issued while a staged group's prefill was in
flight against the others.  `all` ends with a sweep of overlap_replays over 4, 8, 16, alternating --repeats times.  The bar, written
before the run: overlap's median useful tokens/s exceeds graph's by more than the spread of either.
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


class _TimedGraph:
    """eng.graph with an event pair around every replay, tagged by whether a staged group's prefill was in flight when it was issued."""

    def __init__(self, eng):
        self.graph, self.eng, self.marks = eng.graph, eng, []

    def replay(self):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self.graph.replay()
        b.record()
        self.marks.append((bool(self.eng.sched.staged), a, b))


def overlap_engine(m, reqs, lag=8, instrument=False, slots=32):
    """One run of the overlap engine: (wall s, replays, groups, info).  instrument: events around every commit (the time the decode
    stream is stopped for an admission: the wait for the staged prefill, the row commit, the parameter copies, the first draw) and
    around every replay; info = (ms stopped in commits, commits, mean ms of replays next to a prefill, their count, mean ms of the
    other replays, their count)."""
    eng = ContinuousDecoder(m, slots=slots, max_new_tokens_cap=2048, admission="overlap", overlap_replays=lag)
    commits, timed = [], None
    if instrument:
        inner = eng._commit_device

        def timed_commit(took):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            inner(took)
            b.record()
            commits.append((a, b))
        eng._commit_device = timed_commit
        timed = eng.graph = _TimedGraph(eng)

    def run():
        hs = [eng.submit(inputs_embeds=p, max_new_tokens=b) for p, b in reqs]
        out = eng.run()
        assert all(out[h].numel() == b for h, (_, b) in zip(hs, reqs))
        return eng.replays
    sec, replays = wall(run)
    info = None
    if instrument:
        stopped = sum(a.elapsed_time(b) for a, b in commits)
        near = [a.elapsed_time(b) for f, a, b in timed.marks if f]
        alone = [a.elapsed_time(b) for f, a, b in timed.marks if not f]
        info = (stopped, len(commits), statistics.mean(near) if near else float("nan"), len(near),
                statistics.mean(alone) if alone else float("nan"), len(alone))
    return sec, replays, len(eng.admission_log), info


def compare_all(m, reqs, useful, say, repeats, static_tps):
    """eager, graph and overlap admission alternately, `repeats` times each; then the sweep of overlap_replays."""
    res = {"eager": [], "graph": [], "overlap": []}
    extra = []
    for r in range(repeats):
        for mode in ("eager", "graph"):
            te, replays, _ = engine(m, reqs, admission=mode)
            ta, _, sp = engine(m, reqs, time_admission=True, admission=mode)
            res[mode].append((useful / te, sp[0] / ta * 100))
            say(f"  round {r} {mode:7s}: {te:6.2f} s {useful / te:8.0f} useful tokens/s | admission {sp[0] / max(sp[1], 1) * 1e3:6.2f} ms each "
                f"({sp[1]}), {sp[0] / ta * 100:5.1f} % of {ta:.2f} s synced wall")
        te, replays, groups, _ = overlap_engine(m, reqs)
        ti, _, _, (stopped, ncommit, near, n_near, alone, n_alone) = overlap_engine(m, reqs, instrument=True)
        res["overlap"].append((useful / te, stopped / (ti * 1e3) * 100))
        extra.append((near, alone, stopped / max(ncommit, 1)))
        say(f"  round {r} overlap: {te:6.2f} s {useful / te:8.0f} useful tokens/s ({replays} replays, {groups} groups) | decode stream stopped "
            f"{stopped / max(ncommit, 1):6.3f} ms per commit ({ncommit}), {stopped / (ti * 1e3) * 100:5.2f} % of {ti:.2f} s instrumented wall | "
            f"step {near:.3f} ms next to a prefill ({n_near} replays), {alone:.3f} ms otherwise ({n_alone})")
    med = lambda mode, i: statistics.median(x[i] for x in res[mode])
    spr = lambda mode, i: max(x[i] for x in res[mode]) - min(x[i] for x in res[mode])
    for mode in res:
        say(f"{mode:7s} admission: {med(mode, 0):8.0f} useful tokens/s (spread {spr(mode, 0):.0f}) = {med(mode, 0) / static_tps:.2f} x static | "
            f"decode stopped for admission {med(mode, 1):5.2f} % of the wall (spread {spr(mode, 1):.2f})")
    say(f"overlap: step next to a prefill {statistics.median(e[0] for e in extra):.3f} ms against {statistics.median(e[1] for e in extra):.3f} ms "
        f"otherwise; {statistics.median(e[2] for e in extra):.3f} ms stopped per commit")
    s_t = max(spr("graph", 0), spr("overlap", 0))
    say(f"bar: overlap useful tokens/s above graph's by more than the spread of either: {med('overlap', 0) - med('graph', 0) > s_t} "
        f"({med('graph', 0):.0f} -> {med('overlap', 0):.0f}, spread {s_t:.0f})")
    ratio = med("overlap", 0) / static_tps
    say(f"overlap admission against static groups: {ratio:.2f} x (bar of DESIGN.md 7.1: >= 1.4 x: {'met' if ratio >= 1.4 else 'missed'})")
    sweep = {4: [], 8: [], 16: []}
    for r in range(repeats):
        for lag in sweep:
            te, replays, _, _ = overlap_engine(m, reqs, lag=lag)
            sweep[lag].append(useful / te)
            say(f"  sweep round {r} overlap_replays = {lag:2d}: {te:6.2f} s {useful / te:8.0f} useful tokens/s ({replays} replays)")
    for lag, v in sweep.items():
        say(f"overlap_replays = {lag:2d}: {statistics.median(v):8.0f} useful tokens/s (spread {max(v) - min(v):.0f})")
    s_w = max(max(v) - min(v) for v in sweep.values())
    best = max(sweep, key=lambda lag: statistics.median(sweep[lag]))
    say(f"sweep: best overlap_replays = {best}; beats 8 by more than the spread ({s_w:.0f}): "
        f"{statistics.median(sweep[best]) - statistics.median(sweep[8]) > s_w}")


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
    ap.add_argument("--admission", choices=("eager", "graph", "both", "overlap", "all"), default="eager")
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
    mode = a.admission if a.admission in ("graph", "overlap") else "eager"
    engine(m, reqs[:4], slots=4, admission=mode)
    static_groups(m, reqs[:2], G=2)
    ts = static_groups(m, reqs)
    say(f"static GraphDecoder groups of 32: {ts:8.2f} s  {useful / ts:9.0f} useful tokens/s")
    te, replays, _ = engine(m, reqs, admission=mode)
    say(f"ContinuousDecoder, 32 slots ({mode}): {te:8.2f} s  {useful / te:9.0f} useful tokens/s  ({replays} replays, "
        f"{useful / (replays * 32) * 100:.1f} % of slot-steps useful)  -> {ts / te:.2f} x static")
    if mode == "overlap":
        ti, _, _, (stopped, ncommit, near, n_near, alone, n_alone) = overlap_engine(m, reqs, instrument=True)
        say(f"decode stream stopped for admission (events around every commit): {stopped / 1e3:6.3f} s of {ti:.2f} s wall = "
            f"{stopped / (ti * 1e3) * 100:.2f} %  ({ncommit} commits, {stopped / max(ncommit, 1):.3f} ms each)")
        say(f"step next to a prefill          : {near:.3f} ms ({n_near} replays) against {alone:.3f} ms otherwise ({n_alone})")
    else:
        ta, _, sp = engine(m, reqs, time_admission=True, admission=mode)
        adm, n_adm = sp[0], sp[1]
        say(f"admission (synced run)          : {adm:8.2f} s of {ta:.2f} s wall = {adm / ta * 100:.1f} %  ({n_adm} admissions, "
            f"{adm / max(n_adm, 1) * 1e3:.1f} ms each)")
    if a.admission == "both":
        say(f"eager and graph admission, alternating, {a.repeats} rounds:")
        tg = compare(m, reqs, useful, say, a.repeats)
        say(f"graph admission against static groups: {tg / (useful / ts):.2f} x (bar of DESIGN.md 7.1: >= 1.4 x: "
            f"{'met' if tg / (useful / ts) >= 1.4 else 'missed'})")
    if a.admission == "all":
        say(f"eager, graph and overlap admission, alternating, {a.repeats} rounds:")
        compare_all(m, reqs, useful, say, a.repeats, useful / ts)
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
