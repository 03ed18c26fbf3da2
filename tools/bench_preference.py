"""Same-process A/B of DataParallelTrainer.preference_step against DataParallelTrainer.step on the SAME synthetic batch: RWKV7-0.4B in
the Spark layout at B = 8 (four chosen / rejected pairs), L = 4096.  Both run the backbone backward once and AdamW once;
step's head forms d loss / d logits in its forward pass (one head GEMM per chunk), preference_step's head runs the GEMM again in
backward because the upstream gradient differs per utterance, and adds one rwkv7_seq_scores_f32 launch; its backbone runs forward twice
(under no_grad for the value, which is then score's bit for bit, and with autograd when backward arrives: losses.scored_forward).  Three alternations; per side
the median ms per step, the spread (max - min) and torch.cuda.max_memory_allocated above what was live before the call.

    python tools/bench_preference.py [--iters 5] [--out profiles/preference_bench.txt]

A record, not a gate: step on the same batch in the same process is the yardstick, and the record states the ratio."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rwkvtts_amd import backbone, layouts, trainer  # noqa: E402
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig  # noqa: E402
from bench_score import alternate  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "preference_bench.txt"))
    a = ap.parse_args()
    base = backbone.config_0p4b()
    kw = {k: v for k, v in base.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    model = RWKV7ForSpeech(RWKV7SpeechConfig(**kw)).init_weights(seed=0).to(device=DEV, dtype=torch.bfloat16).train()
    tr = trainer.DataParallelTrainer(model, lr=1e-5, warmup_steps=10, total_steps=100000)
    B, T = 8, 4096
    batch = layouts.synthetic_spark_batch(model, B, T, seed=70)
    batch["inputs_embeds"] = batch["inputs_embeds"].detach()   # one batch for every call: no graph into the embedders
    ref = -torch.from_numpy(tr.score([batch])["loss_sum"]).to(DEV)
    r = alternate({"step": lambda: tr.step(**batch),
                   "preference_step": lambda: tr.preference_step(beta=0.1, ref_logps=ref, **batch)}, a.iters)
    lines = ["# tools/bench_preference.py: DataParallelTrainer.preference_step against .step on the same batch",
             f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.iters} calls per timing, 3 alternations"]
    for n in ("step", "preference_step"):
        lines.append(f"0.4B Spark B={B} L={T} | trainer.{n:15s} | {r[n][0]:9.3f} ms | spread {r[n][1]:.3f} | "
                     f"peak {r[n][2]:8.1f} MiB above what was live")
    lines.append(f"preference_step / step = {r['preference_step'][0] / r['step'][0]:.4f} "
                 f"(spread of the two: {max(r['step'][1], r['preference_step'][1]):.3f} ms); "
                 f"peak preference_step / step = {r['preference_step'][2] / r['step'][2]:.4f}")
    out = tr.preference_step(beta=0.1, ref_logps=ref, **batch)
    lines.append(f"check: loss {out['loss'].item():.6f}, mean margin {out['margin'].item():.6f}, accuracy {out['accuracy'].item():.2f}, "
                 f"step_idx {tr.step_idx}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
