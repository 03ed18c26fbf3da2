"""Same-process A/B of DataParallelTrainer.policy_step against .step and .preference_step on the SAME synthetic batch: RWKV7-0.4B in the
Spark layout at B = 8 (one prompt's eight candidates), L = 4096.  All three run the backbone backward once and AdamW once.  step's and
policy_step's heads form d loss / d logits in their forward pass (one head GEMM per chunk; policy_step's kernel also looks up the row's
sequence and closes the row in double) and their backbones run forward once, on the tape; preference_step runs the head GEMM again in
backward and its backbone forward twice (losses.scored_forward).  Three alternations; per side the median ms per step, the spread
(max - min) and torch.cuda.max_memory_allocated above what was live before the call.

    python tools/bench_policy.py [--iters 5] [--out profiles/policy_bench.txt]

A record, not a gate: step on the same batch in the same process is the yardstick, and the record states the ratios."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rwkvtts_amd import backbone, layouts, losses, trainer  # noqa: E402
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig  # noqa: E402
from bench_score import alternate  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "policy_bench.txt"))
    a = ap.parse_args()
    base = backbone.config_0p4b()
    kw = {k: v for k, v in base.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    model = RWKV7ForSpeech(RWKV7SpeechConfig(**kw)).init_weights(seed=0).to(device=DEV, dtype=torch.bfloat16).train()
    tr = trainer.DataParallelTrainer(model, lr=1e-5, warmup_steps=10, total_steps=100000)
    B, T = 8, 4096
    batch = layouts.synthetic_spark_batch(model, B, T, seed=70)
    batch["inputs_embeds"] = batch["inputs_embeds"].detach()   # one batch for every call: no graph into the embedders
    ref_seq = -torch.from_numpy(tr.score([batch])["loss_sum"]).to(DEV)
    old = tr.token_logprobs([batch])[0]   # the policy before tuning: the sampling policy and the frozen reference at once
    adv = losses.group_advantages(torch.linspace(0, 1, B), B).to(DEV)
    kwargs = dict(advantages=adv, old_logps=old, ref_logps=old, kl_beta=0.04)
    r = alternate({"step": lambda: tr.step(**batch),
                   "policy_step": lambda: tr.policy_step(**kwargs, **batch),
                   "preference_step": lambda: tr.preference_step(beta=0.1, ref_logps=ref_seq, **batch)}, a.iters)
    lines = ["# tools/bench_policy.py: DataParallelTrainer.policy_step against .step and .preference_step on the same batch",
             f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.iters} calls per timing, 3 alternations"]
    for n in ("step", "policy_step", "preference_step"):
        lines.append(f"0.4B Spark B={B} L={T} | trainer.{n:15s} | {r[n][0]:9.3f} ms | spread {r[n][1]:.3f} | "
                     f"peak {r[n][2]:8.1f} MiB above what was live")
    spread = max(r[n][1] for n in r)
    lines.append(f"policy_step / step = {r['policy_step'][0] / r['step'][0]:.4f}; preference_step / step = "
                 f"{r['preference_step'][0] / r['step'][0]:.4f} (largest spread of the three: {spread:.3f} ms); "
                 f"peak policy_step / step = {r['policy_step'][2] / r['step'][2]:.4f}")
    out = tr.policy_step(**kwargs, **batch)
    lines.append(f"check: loss {out['loss'].item():.6f}, clip_frac {out['clip_frac'].item():.4f}, kl {out['kl'].item():.3e}, "
                 f"ratio_mean {out['ratio_mean'].item():.6f}, step_idx {tr.step_idx}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
