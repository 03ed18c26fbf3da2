"""Continuous batching for the XY model against RWKV7XYLM.generate (synthetic weights, bf16, greedy, no EOS id, channel 0 restricted to
the audio range: every request runs to its budget and the run is deterministic).

  * captured step: time per frame of ContinuousXYDecoder with 32 live slots and fixed budgets against generate(B = 32,
    use_graph = True) over the same frames, both as the difference of two run lengths (so prefill and graph capture cancel), in one
    process, alternating --repeats times; median and spread.  Bar: engine step <= 1.02 x static step.
  * useful frames/s: --requests requests, prompts uniform in 200..1000 rows, budgets uniform in 128..2048 frames, 32 slots: static
    generate groups of 32 in submission order (each group runs to its longest budget) against the engine under both admission
    modes; share of useful slot-steps and admission share of the wall time (a second run with a device sync around every admission).

    python tools/bench_continuous_xy.py [--width 0.4b|1.5b] [--layers L] [--requests 128] [--repeats 3] [--skip-useful] [--out FILE]
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
from rwkvtts_amd.continuous_xy import ContinuousXYDecoder
from rwkvtts_amd.xy_llm import RWKV7XYConfig, RWKV7XYLM

DEV = torch.device("cuda:0")


def model(width, layers):
    base = backbone.config_1p5b() if width == "1.5b" else backbone.config_0p4b()
    kw = {k: v for k, v in base.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    kw.update(vocab_size=66661)
    if layers:
        kw.update(num_hidden_layers=layers)
    cfg = RWKV7XYConfig(speech_vocab_size=1025, num_channels=8, text_shift_size=65536, **kw)
    m = RWKV7XYLM(cfg).init_weights(seed=0)
    m.zero_embs()
    return m.to(DEV, torch.bfloat16).eval()


def prompt(T, cfg, g):
    ch0 = torch.randint(0, cfg.text_shift_size + cfg.speech_vocab_size, (T, 1), generator=g)
    return torch.cat([ch0, torch.randint(0, cfg.speech_vocab_size - 1, (T, cfg.num_channels - 1), generator=g)], 1).to(DEV)


def workload(n, cfg, seed=0):
    rng, g = random.Random(seed), torch.Generator().manual_seed(seed)
    return [(prompt(rng.randint(200, 1000), cfg, g), rng.randint(128, 2048)) for _ in range(n)]


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def left_pad(prompts, cfg):
    """Left padding with the ids whose embedding rows are zero, and the mask that goes with it."""
    T = max(p.shape[0] for p in prompts)
    ids = torch.empty(len(prompts), T, cfg.num_channels, dtype=torch.int64, device=DEV)
    ids[:, :, 0], ids[:, :, 1:] = cfg.vocab_size - 1, cfg.speech_vocab_size - 1
    mask = torch.zeros(len(prompts), T, dtype=torch.long, device=DEV)
    for i, p in enumerate(prompts):
        ids[i, T - p.shape[0]:] = p
        mask[i, T - p.shape[0]:] = 1
    return ids, mask


def step_times(m, say, repeats, n1=64, n2=576, T=64):
    g = torch.Generator().manual_seed(1)
    ids = torch.stack([prompt(T, m.config, g) for _ in range(32)])
    eng = ContinuousXYDecoder(m, slots=32, max_new_frames_cap=n2)

    def engine(n):
        for p in ids:
            eng.submit(p, max_new_frames=n)
        return wall(eng.run)[0]

    static = lambda n: wall(lambda: m.generate(ids, max_new_tokens=n, do_sample=False, use_graph=True))[0]
    engine(n1), static(n1)   # warm-up
    te, ts = [], []
    for r in range(repeats):
        e = (engine(n2) - engine(n1)) / (n2 - n1) * 1e3
        s = (static(n2) - static(n1)) / (n2 - n1) * 1e3
        te.append(e)
        ts.append(s)
        say(f"  round {r}: engine {e:.4f} ms/frame, generate(B=32) {s:.4f} ms/frame -> {e / s:.3f} x")
    me, ms = statistics.median(te), statistics.median(ts)
    say(f"captured step, 32 live slots: engine {me:.4f} ms (spread {max(te) - min(te):.4f}), static {ms:.4f} ms (spread "
        f"{max(ts) - min(ts):.4f}) -> {me / ms:.3f} x; bar <= 1.02 x: {'met' if me <= 1.02 * ms else 'MISSED'}; launches per frame after "
        f"the decode step: engine 2 (draw, frame), static 3 (draw, frame, embed)")


def static_groups(m, reqs, G=32):
    def run():
        for a in range(0, len(reqs), G):
            grp = reqs[a:a + G]
            ids, mask = left_pad([p for p, _ in grp], m.config)
            m.generate(ids, attention_mask=mask, max_new_tokens=max(b for _, b in grp), do_sample=False, use_graph=True)
    return wall(run)[0]


def engine_run(m, reqs, admission, time_admission=False):
    eng = ContinuousXYDecoder(m, slots=32, max_new_frames_cap=2048, admission=admission)
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
        hs = [eng.submit(p, max_new_frames=b) for p, b in reqs]
        out = eng.run()
        assert all(out[h].shape[0] == b for h, (_, b) in zip(hs, reqs))
        return eng.replays
    sec, replays = wall(run)
    return sec, replays, spent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", choices=("0.4b", "1.5b"), default="1.5b")
    ap.add_argument("--layers", type=int, default=0, help="depth (default: the configuration's 24)")
    ap.add_argument("--requests", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-useful", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m = model(a.width, a.layers)
    cfg = m.config
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"XY {a.width} widths (D = {cfg.hidden_size}, {cfg.num_hidden_layers} layers, 8 channels, V0 = 66661), synthetic bf16, greedy, no EOS; 32 slots")
    step_times(m, say, a.repeats)
    if not a.skip_useful:
        reqs = workload(a.requests, cfg)
        useful = sum(b for _, b in reqs)
        say(f"{len(reqs)} requests, prompts 200..1000 rows (mean {statistics.mean(p.shape[0] for p, _ in reqs):.0f}), budgets 128..2048 "
            f"frames (mean {useful / len(reqs):.0f})")
        engine_run(m, reqs[:4], "eager")   # warm-up
        static_groups(m, reqs[:2], G=2)
        ts = static_groups(m, reqs)
        steps_static = sum(max(b for _, b in reqs[i:i + 32]) * 32 for i in range(0, len(reqs), 32))
        say(f"static generate groups of 32 : {ts:8.2f} s {useful / ts:9.0f} useful frames/s ({useful / steps_static * 100:.1f} % of slot-steps useful)")
        for mode in ("eager", "graph"):
            te, replays, _ = engine_run(m, reqs, mode)
            ta, _, sp = engine_run(m, reqs, mode, time_admission=True)
            say(f"ContinuousXYDecoder ({mode:5s})  : {te:8.2f} s {useful / te:9.0f} useful frames/s ({useful / (replays * 32) * 100:.1f} % of slot-steps "
                f"useful, {replays} replays) -> {ts / te:.2f} x static; admission {sp[0] / ta * 100:.1f} % of {ta:.2f} s synced wall "
                f"({sp[1]} admissions, {sp[0] / max(sp[1], 1) * 1e3:.1f} ms each)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
