"""The wide decode step (B = 33 .. 128, csrc/decode_step_wide.hip) against what it replaces: synthetic bf16 weights, greedy, 24
layers, 0.4B or 1.5B widths, everything in one process.

  closed batch   GraphDecoder B = 32 | MultiGroupDecoder 4 x 32 | GraphDecoder B = 64 (wide) | GraphDecoder B = 128 (wide), alternating
                 `--rounds` times.  Each figure is the difference of a 576-step and a 64-step generate() (prefill and capture cancel):
                 ms per step and tokens/s = sequences / step time; spread = max - min over the rounds.
  ragged         (--ragged) the 128-request workload of tools/bench_continuous.py once through ContinuousDecoder(admission="graph") with
                 slots = 32 and with slots = 128: useful tokens/s.

Bars, written down before the first measurement; the contenders are the parent's code paths in the same process:
  (a) tokens/s of the wide step at B = 128 exceeds MultiGroupDecoder 4 x 32 by more than the spread, at both widths;
  (b) the B = 64 step takes less than two B = 32 steps by more than the spread.

    python tools/bench_decode_wide.py --width 0.4b|1.5b [--rounds 3] [--ragged] [--out FILE]   (--out appends)
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rwkvtts_amd import backbone
from rwkvtts_amd.decode import GraphDecoder, MultiGroupDecoder, WideDecodeStep
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig

DEV = torch.device("cuda:0")
N1, N2, P = 64, 576, 64


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def model(width):
    c = backbone.config_1p5b() if width == "1.5b" else backbone.config_0p4b()
    base = {k: v for k, v in c.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    base["vocab_size"] = 8193
    return RWKV7ForSpeech(RWKV7SpeechConfig(**base)).init_weights(0).to(DEV, torch.bfloat16).eval()


def closed_batch(m, say, rounds):
    g = torch.Generator().manual_seed(1234)
    emb = (torch.randn(128, P, m.config.hidden_size, generator=g) * 0.5).to(DEV, torch.bfloat16)
    mask = torch.ones(128, P, dtype=torch.long, device=DEV)
    eos = m.config.vocab_size - 1   # suppressed: every sequence runs to its budget

    def single(B):
        def run(n):
            d = GraphDecoder(m, B, step_kernel=True)
            t = wall(lambda: d.generate(inputs_embeds=emb[:B], attention_mask=mask[:B], max_new_tokens=n + 1, suppress_tokens=[eos]))
            assert (B > 32) == isinstance(d.step, WideDecodeStep)
            return t
        return run

    def groups(n):
        d = MultiGroupDecoder(m, 32, step_kernel=True)
        return wall(lambda: d.generate(inputs_embeds=emb, attention_mask=mask, max_new_tokens=n + 1, suppress_tokens=[eos]))

    contenders = [("GraphDecoder B=32", 32, single(32)), ("MultiGroupDecoder 4x32", 128, groups), ("wide step B=64", 64, single(64)),
                  ("wide step B=128", 128, single(128))]
    for _, _, run in contenders:   # warm-up: kernels, graph pools
        run(8)
    ms = {name: [] for name, _, _ in contenders}
    for r in range(rounds):
        for name, B, run in contenders:
            step = (run(N2) - run(N1)) / (N2 - N1) * 1e3
            ms[name].append(step)
            say(f"  round {r} {name:24s}: {step:7.4f} ms/step {B / step * 1e3:9.0f} tokens/s")
    med = {k: statistics.median(v) for k, v in ms.items()}
    seqs = {name: B for name, B, _ in contenders}
    tps = {k: [seqs[k] / x * 1e3 for x in v] for k, v in ms.items()}
    spread_ms = {k: max(v) - min(v) for k, v in ms.items()}
    spread_tps = {k: max(v) - min(v) for k, v in tps.items()}
    for k in ms:
        say(f"{k:24s}: {med[k]:7.4f} ms/step (spread {spread_ms[k]:.4f}) {statistics.median(tps[k]):9.0f} tokens/s (spread {spread_tps[k]:.0f})")
    w, g4 = statistics.median(tps["wide step B=128"]), statistics.median(tps["MultiGroupDecoder 4x32"])
    sa = max(spread_tps["wide step B=128"], spread_tps["MultiGroupDecoder 4x32"])
    say(f"bar (a) wide B=128 tokens/s > MultiGroupDecoder 4x32 by more than the spread: {'met' if w - g4 > sa else 'MISSED'} "
        f"({w:.0f} against {g4:.0f}, spread {sa:.0f})")
    t64, t32 = med["wide step B=64"], med["GraphDecoder B=32"]
    sb = spread_ms["wide step B=64"] + 2 * spread_ms["GraphDecoder B=32"]
    say(f"bar (b) B=64 step < two B=32 steps by more than the spread: {'met' if 2 * t32 - t64 > sb else 'MISSED'} "
        f"({t64:.4f} ms against 2 x {t32:.4f} ms, spread {sb:.4f})")


def ragged(m, say, requests):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bench_continuous as bc
    reqs = bc.workload(requests, m.config.hidden_size)
    useful = sum(b for _, b in reqs)
    bc.engine(m, reqs[:4], slots=4, admission="graph")   # warm-up
    for slots in (32, 128):
        sec, replays, _ = bc.engine(m, reqs, slots=slots, admission="graph")
        say(f"ragged workload ({len(reqs)} requests, graph admission), slots = {slots:3d}: {sec:7.2f} s {useful / sec:9.0f} useful tokens/s "
            f"({replays} replays, {useful / (replays * slots) * 100:.1f} % of slot-steps useful)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", choices=("0.4b", "1.5b"), default="0.4b")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--requests", type=int, default=128)
    ap.add_argument("--skip-closed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    m = model(a.width)
    say(f"{a.width} widths, 24 layers, synthetic bf16, greedy; prompt {P} tokens; step = (generate({N2}) - generate({N1})) / {N2 - N1}")
    if not a.skip_closed:
        closed_batch(m, say, a.rounds)
    if a.ragged:
        ragged(m, say, a.requests)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
