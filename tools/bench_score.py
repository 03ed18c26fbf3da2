"""Same-process A/B of the per-utterance scores, in one process:
  1. trainer : DataParallelTrainer.score against DataParallelTrainer.evaluate on the SAME synthetic batches, RWKV7-0.4B in the Spark
               layout at B = 8, L = 4096 (both run the backbone once per batch and the chunked head; score keeps 16 bytes per row and
               adds one rwkv7_seq_scores_f32 launch), with torch.cuda.max_memory_allocated above what was live beside each.
  2. kernel  : rwkv7_seq_scores_f32 alone on N = 32 768 rows (8 sequences of 4096: one workgroup each) and on the same rows cut into
               512 sequences of 64; it reads 16 N bytes (fp32 loss, int32 correct, int64 label per row).
Three alternations per case; per side the median of the three and the spread (max - min).

    python tools/bench_score.py [--iters 5] [--batches 2] [--out profiles/score_bench.txt]

No speed bar is fixed in advance: evaluate on the same batches in the same process is the yardstick, and the record states the ratio."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rwkvtts_amd import _lib, backbone, layouts, trainer  # noqa: E402
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig  # noqa: E402

DEV = "cuda:0"


def timed(fn, iters):
    """ms per call (events around `iters` calls) and the peak allocation above what was live before"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def alternate(sides, iters):
    """{name: (median ms, spread ms, peak MiB)} after one warm-up round and three alternations"""
    for fn in sides.values():
        timed(fn, 1)
    res = {n: [] for n in sides}
    for _ in range(3):
        for n, fn in sides.items():
            res[n].append(timed(fn, iters))
    return {n: (statistics.median(r[0] for r in v), max(r[0] for r in v) - min(r[0] for r in v), max(r[1] for r in v))
            for n, v in res.items()}


def trainer_case(iters, n_batches, lines):
    base = backbone.config_0p4b()
    kw = {k: v for k, v in base.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    model = RWKV7ForSpeech(RWKV7SpeechConfig(**kw)).init_weights(seed=0).to(device=DEV, dtype=torch.bfloat16).train()
    tr = trainer.DataParallelTrainer(model, lr=1e-4, warmup_steps=10, total_steps=1000)
    B, T = 8, 4096
    batches = [layouts.synthetic_spark_batch(model, B, T, seed=70 + i) for i in range(n_batches)]
    r = alternate({"score": lambda: tr.score(batches), "evaluate": lambda: tr.evaluate(batches)}, iters)
    for n in ("score", "evaluate"):
        lines.append(f"0.4B Spark B={B} L={T}, {n_batches} batches | trainer.{n:8s} | {r[n][0]:9.3f} ms | spread {r[n][1]:.3f} | "
                     f"peak {r[n][2]:8.1f} MiB above what was live")
    ratio = r["score"][0] / r["evaluate"][0]
    lines.append(f"score / evaluate = {ratio:.4f} (spread of the two: {max(r['score'][1], r['evaluate'][1]):.3f} ms); "
                 f"rows kept by score per batch: {16 * B * T / 2 ** 10:.0f} KiB (16 bytes x {B * T} rows)")
    s, e = tr.score(batches), tr.evaluate(batches)
    lines.append(f"check: sum loss_sum / sum tokens = {s['loss_sum'].sum() / s['tokens'].sum():.6f}, evaluate loss = {e['loss']:.6f}; "
                 f"utterances {s['tokens'].size}, tokens {int(s['tokens'].sum())} = {e['tokens']}")


def kernel_case(iters, lines):
    N = 8 * 4096
    g = torch.Generator().manual_seed(1)
    loss = (torch.rand(N, generator=g) * 10).to(DEV)
    corr = torch.randint(0, 2, (N,), generator=g, dtype=torch.int32).to(DEV)
    lab = torch.randint(0, 8193, (N,), generator=g)
    lab[::10] = -100
    lab = lab.to(DEV)
    for n_seq in (8, 512):
        st = torch.arange(n_seq + 1, dtype=torch.int64, device=DEV) * (N // n_seq)
        out = [torch.empty(n_seq, dtype=t, device=DEV) for t in (torch.float64, torch.int64, torch.int64, torch.float32, torch.int64)]
        fn = lambda: _lib.call("rwkv7_seq_scores_f32", loss, n_seq, st, loss, corr, lab, -100, *out)
        ms, spread, _ = alternate({"k": fn}, iters * 20)["k"]
        lines.append(f"rwkv7_seq_scores_f32 N={N} n_seq={n_seq:4d} | {ms * 1e3:8.2f} us | spread {spread * 1e3:.2f} us | reads 16 N = {16 * N} bytes "
                     f"({16 * N / (ms * 1e-3) / 1e9:.1f} GB/s; back-to-back launches, the rows stay in cache)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "score_bench.txt"))
    a = ap.parse_args()
    lines = ["# tools/bench_score.py: DataParallelTrainer.score against .evaluate on the same batches; rwkv7_seq_scores_f32 alone",
             f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.iters} calls per timing, 3 alternations per case"]
    kernel_case(a.iters, lines)
    trainer_case(a.iters, a.batches, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
