"""State tuning on RWKV7-0.4B in the Spark layout (synthetic weights, bf16), B = 8, L = 4096, 8 voices, everything in one process:

  (a) StateTuner.step (all three fields tuned) against DataParallelTrainer.step on the SAME batch: what a step that trains 8 states
      costs next to a step that trains 0.4B weights;
  (b) rwkv7_state_rows_adamw_f32 against the torch route it replaces on the same gradients: per layer and field an index_add_ into
      a per-voice fp32 sum, one foreach AdamW over the masters, and an index_copy_ into the store's rows.

Both alternate (one warm-up round, three alternations, bench_score.alternate) and report the median, the spread (max - min) and the
peak memory above what was live.  A record, not a gate: no bar is fixed in advance.

    python tools/bench_state_tune.py [--iters 5] [--out profiles/state_tune_bench.txt]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rwkvtts_amd import backbone, layouts, trainer  # noqa: E402
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig  # noqa: E402
from rwkvtts_amd.state_store import StateStore  # noqa: E402
from rwkvtts_amd.state_tune import FIELDS, StateTuner  # noqa: E402
from bench_score import alternate  # noqa: E402

DEV = "cuda:0"


def torch_route(t, grads, voice_idx, store_idx, step):
    """The step in torch ops, all voices at the same step count: what the kernel replaces."""
    b1, b2 = t.betas
    ps, ms, vs, gs = [], [], [], []
    for l, d in enumerate(grads):
        for f, g in d.items():
            s = torch.zeros_like(t.master[l][f])
            s.index_add_(0, voice_idx, g.float())
            ps.append(t.master[l][f]), ms.append(t.exp_avg[l][f]), vs.append(t.exp_avg_sq[l][f]), gs.append(s)
    torch._foreach_mul_(ps, 1.0 - t.lr * t.weight_decay)
    torch._foreach_mul_(ms, b1)
    torch._foreach_add_(ms, gs, alpha=1.0 - b1)
    torch._foreach_mul_(vs, b2)
    torch._foreach_addcmul_(vs, gs, gs, value=1.0 - b2)
    den = torch._foreach_sqrt(vs)
    torch._foreach_div_(den, math.sqrt(1.0 - b2 ** step))
    torch._foreach_add_(den, t.eps)
    torch._foreach_addcdiv_(ps, ms, den, value=-t.lr / (1.0 - b1 ** step))
    for l, d in enumerate(grads):
        for f in d:
            dst = getattr(t.store.cache[l], f)
            dst.index_copy_(0, store_idx, t.master[l][f].to(dst.dtype))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "state_tune_bench.txt"))
    a = ap.parse_args()
    base = backbone.config_0p4b()
    kw = {k: v for k, v in base.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    model = RWKV7ForSpeech(RWKV7SpeechConfig(**kw)).init_weights(seed=0).to(device=DEV, dtype=torch.bfloat16).train()
    tr = trainer.DataParallelTrainer(model, lr=1e-5, warmup_steps=10, total_steps=100000)
    B, T = 8, 4096
    batch = layouts.synthetic_spark_batch(model, B, T, seed=70)
    batch["inputs_embeds"] = batch["inputs_embeds"].detach()
    names = [f"voice{i}" for i in range(B)]
    store = StateStore(model, B)
    tuner = StateTuner(model, store, lr=1e-3, fields=FIELDS)
    for n in names:
        tuner.add(n, init="zeros")
    lines = ["# tools/bench_state_tune.py: state tuning at 0.4B, B = 8, L = 4096, 8 voices, all three fields tuned",
             f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.iters} calls per timing, 3 alternations"]
    r = alternate({"trainer.step": lambda: tr.step(**batch), "tuner.step": lambda: tuner.step(voices=names, **batch)}, a.iters)
    for n, v in r.items():
        lines.append(f"(a) {n:12s} | {v[0]:9.3f} ms | spread {v[1]:.3f} | peak {v[2]:8.1f} MiB above what was live")
    lines.append(f"(a) tuner.step / trainer.step = {r['tuner.step'][0] / r['trainer.step'][0]:.4f}")
    # (b) the optimizer step alone, on the gradients of the last tuner.step
    grads = [{f: t.grad for f, t in d.items()} for d in tuner.last_leaves]
    voice, seg_start, seg_rows, seg_info = tuner.plan(names)
    dev = [torch.tensor(x, dtype=torch.int32, device=DEV).reshape(-1) for x in (seg_start, seg_rows, seg_info)]
    vi = torch.tensor(voice, device=DEV)
    si = torch.tensor([store.row(n) for n in names], device=DEV)
    flag = torch.zeros(1, device=DEV)
    r = alternate({"kernel": lambda: tuner._apply(grads, B, seg_start, seg_rows, seg_info, dev, flag),
                   "torch": lambda: torch_route(tuner, grads, vi, si, 1)}, a.iters * 4)
    for n, v in r.items():
        lines.append(f"(b) {n:12s} | {v[0]:9.3f} ms | spread {v[1]:.3f} | peak {v[2]:8.1f} MiB above what was live")
    lines.append(f"(b) torch / kernel = {r['torch'][0] / r['kernel'][0]:.3f} (spread of the two: {max(r['torch'][1], r['kernel'][1]):.3f} ms)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
