"""Same-process A/B of the Cosy training head alone (loss + accuracy, forward + backward):
    fused  : losses.fused_linear_kl_accuracy on the hidden states (rwkv7_kl_acc_fwd_bwd_bf16 on one chunk of bf16 logits at a time)
    parent : lm_head -> losses.label_smoothing_kl + losses.th_accuracy on the materialised [rows, V] logits, autograd backward
Cosy sizes: rows in {4096, 32768}, D in {768, 1024}, V = 6562, smoothing 0.1, a tenth of the rows ignored.  Three alternations
fused / parent per shape; per side the median of the three, the spread (max - min) and torch.cuda.max_memory_allocated.

    python tools/bench_cosy_head.py [--iters 20] [--out profiles/cosy_head_bench.txt]

Bar (stated before the first run): fused faster than parent by more than the larger spread at both row counts, and a lower peak."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rwkvtts_amd import losses  # noqa: E402

V, S, DEV = 6562, 0.1, "cuda:0"


def fused_step(h, w, b, labels):
    loss, acc = losses.fused_linear_kl_accuracy(h, labels, w, b, 8, S, True, ignore_index=-1)
    loss.backward()
    return loss, acc


def parent_step(h, w, b, labels):
    logits = torch.nn.functional.linear(h, w, b)
    loss = losses.label_smoothing_kl(logits.unsqueeze(0), labels.unsqueeze(0), V, -1, S, True)
    acc = losses.th_accuracy(logits, labels.unsqueeze(0), -1)
    loss.backward()
    return loss, acc


def timed(step, args, iters):
    """ms per call (events around `iters` calls) and the peak allocation above what was live before"""
    for t in args[:3]:
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        for t in args[:3]:
            t.grad = None
        out = step(*args)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters, (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "cosy_head_bench.txt"))
    a = ap.parse_args()
    lines = ["# tools/bench_cosy_head.py: Cosy head alone, loss + accuracy, forward + backward, bf16, V = 6562, smoothing 0.1",
             f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.iters} calls per timing, 3 alternations fused / parent",
             "# rows D | side | median ms | spread ms (max - min) | peak MiB above the inputs | loss acc"]
    verdict = []
    for rows in (4096, 32768):
        for D in (768, 1024):
            g = torch.Generator().manual_seed(rows + D)
            h = (torch.randn(rows, D, generator=g)).bfloat16().to(DEV).requires_grad_(True)
            w = (torch.randn(V, D, generator=g) * 0.05).bfloat16().to(DEV).requires_grad_(True)
            b = (torch.randn(V, generator=g) * 0.1).bfloat16().to(DEV).requires_grad_(True)
            labels = torch.randint(0, V, (rows,), generator=g)
            labels[::10] = -1
            args = (h, w, b, labels.to(DEV))
            for step in (fused_step, parent_step):   # warm-up: library handles, GEMM selection, allocator
                timed(step, args, 2)
            res = {"fused": [], "parent": []}
            for _ in range(3):
                for name, step in (("fused", fused_step), ("parent", parent_step)):
                    res[name].append(timed(step, args, a.iters))
            row = {}
            for name in ("fused", "parent"):
                ms = [r[0] for r in res[name]]
                loss, acc = res[name][-1][2]
                row[name] = (statistics.median(ms), max(ms) - min(ms), max(r[1] for r in res[name]))
                lines.append(f"{rows:6d} {D:5d} | {name:6s} | {row[name][0]:9.3f} | {row[name][1]:7.3f} | {row[name][2]:10.1f} | "
                             f"{loss.item():.5f} {acc.item():.5f}")
            gain, spread = row["parent"][0] - row["fused"][0], max(row["fused"][1], row["parent"][1])
            ok = gain > spread and row["fused"][2] < row["parent"][2]
            verdict.append(ok)
            lines.append(f"{rows:6d} {D:5d} | parent - fused = {gain:.3f} ms (spread {spread:.3f}), peak {row['fused'][2]:.0f} vs "
                         f"{row['parent'][2]:.0f} MiB: {'meets' if ok else 'MISSES'} the bar")
            del h, w, b, args
            torch.cuda.empty_cache()
    lines.append("# bar: fused faster than parent by more than the spread at both row counts and a lower peak: "
                 + ("MET" if all(verdict) else "NOT MET -- fused_loss stays experimental"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
