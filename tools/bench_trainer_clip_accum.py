"""Cost of gradient clipping and micro-batch accumulation in DataParallelTrainer, one GPU.

    python tools/bench_trainer_clip_accum.py [--model 0.4b] [--batch 8] [--seq-len 4096] [--steps 6] [--warmup 3] [--rounds 3]

Prints one JSON line:
  step_ms            trainer.step() with neither feature used (median / min / max over --rounds x --steps) -- run it from a checkout of
                     the parent commit with --plain-only for the other half of the A/B
  adamw_pass_ms      rwkv7_adamw_groups_bf16 over the whole flat buffer, alone on the stream
  sumsq_pass_ms      rwkv7_grad_sumsq_bf16 (both launches) over the same buffer; sumsq_over_adamw is the ratio
  accum_pass_ms / fold_pass_ms   the accumulate (not first) and fold passes over the same buffer
  clip_step_ms       step() with max_grad_norm set (clip active)
  accumulate_ms      accumulate() per call
Times are device times between events around the timed region, median over the repetitions; every number is a steady-state one
(warm-up steps absorb the first-pass bucket re-cut and the allocator)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="0.4b", choices=["0.1b", "0.4b", "1.5b"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true", help="time the plain step only (works on a tree without the features)")
    a = ap.parse_args()

    import torch
    from rwkvtts_amd import _lib, backbone, trainer
    from rwkvtts_amd.layouts import synthetic_spark_batch
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    base = {"0.1b": backbone.config_0p1b, "0.4b": backbone.config_0p4b, "1.5b": backbone.config_1p5b}[a.model]()
    base_kw = {k: v for k, v in base.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    kw = dict(lr=1e-4, warmup_steps=10, total_steps=1000)

    def make(**extra):
        model = RWKV7ForSpeech(RWKV7SpeechConfig(**base_kw)).init_weights(seed=0).to(device=dev, dtype=torch.bfloat16).train()
        return model, trainer.DataParallelTrainer(model, **kw, **extra)

    model, tr = make()

    def timed(fn, reps, warm, two=False):
        """Per-call device milliseconds of fn(batch), the batch built outside the timed region."""
        out = []
        for i in range(warm + reps):
            b = synthetic_spark_batch(model, a.batch, a.seq_len, seed=1234 + 1000 * i)
            b2 = synthetic_spark_batch(model, a.batch, a.seq_len, seed=1235 + 1000 * i) if two else None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(b, b2) if two else fn(b)
            e1.record()
            e1.synchronize()
            if i >= warm:
                out.append(e0.elapsed_time(e1))
        return out

    def stats(xs):
        return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}

    res = {"model": a.model, "batch": a.batch, "seq_len": a.seq_len, "numel": tr.flat.numel, "device": torch.cuda.get_device_name(dev)}
    plain = []
    for r in range(a.rounds):
        plain += timed(lambda b: tr.step(**b), a.steps, a.warmup if r == 0 else 1)
    res["step_ms"] = stats(plain)
    if a.plain_only:
        print(json.dumps(res))
        return

    # the passes alone, over the whole flat buffer
    lib = _lib.lib()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    f = ctypes.c_float
    n = tr.flat.numel
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ws = torch.empty(lib.rwkv7_grad_sumsq_workspace_bytes(n) // 4, dtype=torch.float32, device=dev)
    ss = torch.zeros(1, device=dev)
    acc = torch.zeros(n, dtype=torch.float32, device=dev)
    g = tr.flat.flat_grad.clone()
    one = torch.ones(1, device=dev)     # skip flag set: the pass moves the same bytes and leaves the weights alone but for the momentum

    def pass_ms(call, reps=20, warm=3):
        out = []
        for i in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = call()
            e1.record()
            e1.synchronize()
            assert rc == 0
            if i >= warm:
                out.append(e0.elapsed_time(e1))
        return stats(out)

    state = [tr.master.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.flat.flat_param.clone()]
    res["adamw_pass_ms"] = pass_ms(lambda: lib.rwkv7_adamw_groups_bf16(
        ctypes.c_long(n), P(state[0]), P(g), P(state[1]), P(state[2]), P(state[3]), P(tr.slab_group), P(tr.group_tab), len(tr.group_defs),
        P(one), f(1e-4), f(0.9), f(0.95), f(1e-18), 5, st))
    res["sumsq_pass_ms"] = pass_ms(lambda: lib.rwkv7_grad_sumsq_bf16(ctypes.c_long(n), P(g), P(ws), P(ss), 0, st))
    res["adamw_clip_pass_ms"] = pass_ms(lambda: lib.rwkv7_adamw_groups_clip_bf16(
        ctypes.c_long(n), P(state[0]), P(g), P(state[1]), P(state[2]), P(state[3]), P(tr.slab_group), P(tr.group_tab), len(tr.group_defs),
        P(one), P(ss), f(1.0), f(1e-4), f(0.9), f(0.95), f(1e-18), 5, st))
    res["accum_pass_ms"] = pass_ms(lambda: lib.rwkv7_grad_accum_bf16(ctypes.c_long(n), P(acc), P(g), 0, st))
    res["fold_pass_ms"] = pass_ms(lambda: lib.rwkv7_grad_fold_bf16(ctypes.c_long(n), P(acc), P(g), f(0.5), st))
    res["sumsq_over_adamw"] = round(res["sumsq_pass_ms"]["median"] / res["adamw_pass_ms"]["median"], 4)
    res["grad_norm"] = round(float(ss.sqrt().item()), 6)
    del state, acc, g, tr, model

    # a fresh model and trainer: step with the clip active (half the observed norm), then accumulate() per call
    model, t2 = make(max_grad_norm=0.5 * res["grad_norm"])
    res["clip_step_ms"] = stats(timed(lambda b: t2.step(**b), a.steps, a.warmup))
    res["accumulate_ms"] = stats(timed(lambda b: t2.accumulate(**b), a.steps, 2))
    t2.step(**synthetic_spark_batch(model, a.batch, a.seq_len, seed=1))
    torch.cuda.synchronize()
    res["accum_window_step_ms"] = stats(timed(lambda b, b2: (t2.accumulate(**b), t2.step(**b2)), 3, 1, two=True))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
