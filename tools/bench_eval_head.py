"""Same-process A/B of the held-out evaluation head, in one process:
  1. kernel : rwkv7_head_eval_bf16 against the training entry of the same kind on the same chunk of bf16 logits
              (the three kernels of csrc/head_loss.hip; kind 0: rwkv7_ce_fwd_bwd_ld_bf16 in place; kind 1: rwkv7_kl_acc_fwd_bwd_bf16 in place), chunk shapes 8192 x 8193,
              8192 x 6562 and 2048 x 66661, rows padded to 16 bytes, smoothing 0.1, a tenth of the rows ignored.  The in-place entries
              overwrite the logits with their gradient: after the first call they time on those values (the work per element is the same).
  2. model  : RWKV7ForSpeech.eval_metrics against the eval-mode forward(labels=...) it replaces, Spark head (V = 8193) at B = 8,
              L = 4096 on a two-layer D = 1024 backbone, with torch.cuda.max_memory_allocated above the inputs beside each.
Three alternations A / B per case; per side the median of the three and the spread (max - min).

    python tools/bench_eval_head.py [--iters 20] [--out profiles/eval_head_bench.txt]

Bar (stated before the first run): the eval kernel reads what the training kernel reads and writes almost nothing, so its time must not
exceed the training entry's on the same shape by more than the larger same-process spread."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rwkvtts_amd import _lib, layouts  # noqa: E402
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig  # noqa: E402

S, DEV = 0.1, "cuda:0"


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
        timed(fn, 2)
    res = {n: [] for n in sides}
    for _ in range(3):
        for n, fn in sides.items():
            res[n].append(timed(fn, iters))
    return {n: (statistics.median(r[0] for r in v), max(r[0] for r in v) - min(r[0] for r in v), max(r[1] for r in v))
            for n, v in res.items()}


def kernel_cases(iters, lines):
    ok = []
    for rows, V in ((8192, 8193), (8192, 6562), (2048, 66661)):
        ld = -(-V // 8) * 8
        g = torch.Generator().manual_seed(V)
        labels = torch.randint(0, V, (rows,), generator=g)
        labels[::10] = -1
        labels = labels.to(DEV)
        x = torch.zeros(rows, ld, dtype=torch.bfloat16, device=DEV)
        x[:, :V] = (torch.randn(rows, V, generator=g) * 3).bfloat16().to(DEV)
        work = x.clone()
        loss = torch.empty(rows, dtype=torch.float32, device=DEV)
        corr = torch.empty(rows, dtype=torch.int32, device=DEV)
        for kind, name in ((0, "rwkv7_ce_fwd_bwd_ld_bf16"), (1, "rwkv7_kl_acc_fwd_bwd_bf16")):
            work.copy_(x)
            if kind == 0:
                train = lambda: _lib.call(name, work, rows, V, ld, work, labels, -1, 1.0, loss, S)
            else:
                train = lambda: _lib.call(name, work, rows, V, ld, work, work, labels, -1, S, 1.0, loss, corr)
            ev = lambda: _lib.call("rwkv7_head_eval_bf16", x, rows, V, ld, x, labels, -1, kind, S, loss, corr, None)
            r = alternate({"eval": ev, "train": train}, iters)
            gb = rows * V * 2 / 1e9
            for n in ("eval", "train"):
                lines.append(f"{rows:6d} x {V:6d} kind {kind} | {n:5s} | {r[n][0]:8.4f} ms | spread {r[n][1]:.4f} | "
                             f"{gb / (r[n][0] * 1e-3):7.1f} GB/s of logits read")
            over, spread = r["eval"][0] - r["train"][0], max(r["eval"][1], r["train"][1])
            ok.append(over <= spread)
            lines.append(f"{rows:6d} x {V:6d} kind {kind} | eval - train = {over:+.4f} ms (spread {spread:.4f}): "
                         f"{'meets' if ok[-1] else 'MISSES'} the bar")
        del x, work
        torch.cuda.empty_cache()
    return all(ok)


def model_case(iters, lines):
    cfg = RWKV7SpeechConfig(vocab_size=8193, text_vocab_size=65536, audio_global_vocab_size=4096, hidden_size=1024, num_hidden_layers=2)
    m = RWKV7ForSpeech(cfg).init_weights(seed=3).to(DEV).to(torch.bfloat16).train()
    batch = layouts.synthetic_spark_batch(m, 8, 4096, seed=5)

    def parent():
        m.eval()
        with torch.no_grad():
            out = m(**batch).loss
        m.train()
        return out

    r = alternate({"eval_metrics": lambda: m.eval_metrics(**batch), "forward": parent}, iters)
    a, b = m.eval_metrics(**batch)["loss"].item(), parent().item()
    for n in ("eval_metrics", "forward"):
        lines.append(f"Spark head B=8 L=4096 V=8193 (2 layers, D=1024) | {n:12s} | {r[n][0]:8.3f} ms | spread {r[n][1]:.3f} | "
                     f"peak {r[n][2]:8.1f} MiB above the inputs")
    lines.append(f"loss: eval_metrics {a:.6f}, eval-mode forward {b:.6f}; bf16 logits of the batch: {8 * 4096 * 8193 * 2 / 2 ** 20:.0f} MiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "eval_head_bench.txt"))
    a = ap.parse_args()
    lines = ["# tools/bench_eval_head.py: rwkv7_head_eval_bf16 against the training entries; eval_metrics against the eval-mode forward",
             f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.iters} calls per timing, 3 alternations per case"]
    met = kernel_cases(a.iters, lines)
    lines.append("# bar: eval kernel not slower than the training entry by more than the same-process spread, every shape and kind: "
                 + ("MET" if met else "NOT MET"))
    model_case(max(2, a.iters // 4), lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
