"""Same-process A/B of the logit regularisers against the plain head, alternating rounds:
  head : losses.fused_linear_cross_entropy forward + backward alone at N = 32 768 rows, V = 8193, D = 1024 (the padded route) -- the plain
         call (rwkv7_ce_fwd_bwd_ld_bf16) against z_loss / max_logit / stats on (rwkv7_ce_reg_fwd_bwd_bf16 and the three row sums);
  step : DataParallelTrainer.step of RWKV7-0.4B in the Spark layout at B = 8, L = 4096 on the same batch -- the model's config with the
         coefficients 0 against the coefficients on (which also keeps last_logit_stats).
Three alternations; per side the median ms per call and the spread (max - min).  The yardstick is the plain kernel in the same process.

    python tools/bench_logit_reg.py [--iters 5] [--skip-step] [--out profiles/logit_reg_bench.txt]

A record, not a gate."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rwkvtts_amd import backbone, layouts, losses, trainer  # noqa: E402
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig  # noqa: E402
from bench_score import alternate  # noqa: E402

DEV = "cuda:0"
Z, C = 1e-4, 1e-4


def head_sides(N=32768, V=8193, D=1024):
    g = torch.Generator().manual_seed(1)
    h = (torch.randn(N, D, generator=g) * 0.5).to(DEV, torch.bfloat16).requires_grad_()
    w = (torch.randn(V, D, generator=g) * D ** -0.5).to(DEV, torch.bfloat16).requires_grad_()
    lab = torch.randint(0, V, (N,), generator=g).to(DEV)
    lab[::7] = -100
    stats = torch.zeros(4, device=DEV)

    def run(**kw):
        h.grad = w.grad = None
        losses.fused_linear_cross_entropy(h, lab, w, None, -100, **kw).backward()

    return {"plain": run, "regularised": lambda: run(z_loss=Z, max_logit=C, stats=stats)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "logit_reg_bench.txt"))
    a = ap.parse_args()
    lines = ["# tools/bench_logit_reg.py: z_loss / max_logit / stats on against the plain head, same process, alternating rounds",
             f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.iters} calls per timing, 3 alternations; z = {Z}, c = {C}"]

    def record(what, r):
        for n in ("plain", "regularised"):
            lines.append(f"{what} | {n:11s} | {r[n][0]:9.3f} ms | spread {r[n][1]:.3f}")
        d, spread = r["regularised"][0] - r["plain"][0], max(r["plain"][1], r["regularised"][1])
        lines.append(f"{what} | regularised - plain = {d:+.3f} ms ({100 * d / r['plain'][0]:+.2f} %); larger spread {spread:.3f} ms: "
                     + ("inside the spread" if abs(d) <= spread else "OUTSIDE the spread"))

    hits = losses.PADDED_HEAD_HITS[0]
    record("head N=32768 V=8193 D=1024", alternate(head_sides(), a.iters))
    assert losses.PADDED_HEAD_HITS[0] > hits, "the head A/B is meant to take the padded route"
    if not a.skip_step:
        base = backbone.config_0p4b()
        kw = {k: v for k, v in base.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
        model = RWKV7ForSpeech(RWKV7SpeechConfig(z_loss=Z, max_logit=C, **kw)).init_weights(seed=0).to(device=DEV, dtype=torch.bfloat16)
        tr = trainer.DataParallelTrainer(model.train(), lr=1e-5, warmup_steps=10, total_steps=100000)
        batch = layouts.synthetic_spark_batch(model, 8, 4096, seed=70)
        batch["inputs_embeds"] = batch["inputs_embeds"].detach()   # one batch for every call: no graph into the embedders

        def step(z, c):
            model.config.z_loss, model.config.max_logit = z, c
            model.logit_stats = tr._logit_stats if z or c else None   # off: the call the parent made
            tr.step(**batch)

        record("trainer.step 0.4B Spark B=8 L=4096", alternate({"plain": lambda: step(0.0, 0.0), "regularised": lambda: step(Z, C)},
                                                                a.iters))
        s = {k: round(v.item(), 4) for k, v in tr.last_logit_stats.items()}
        lines.append(f"check: last_logit_stats {s}, step_idx {tr.step_idx}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
