"""Serving from a stored state against prefilling the shared prefix with every request (0.4B Spark widths, synthetic weights, bf16,
greedy, EOS disabled so that every request runs to its budget): 128 requests of ONE 512-token voice prefix, ragged suffixes of
32..128 tokens, max_new_tokens uniform in 128..512, 32 slots.

  * `state`: the prefix is captured once into a StateStore (outside the timed window: it is paid once per voice, not per request)
    and every request is submit(state="voice", inputs_embeds=suffix);
  * `whole`: every request is submit(inputs_embeds=cat(prefix, suffix)), on an engine without a store.

Per admission mode (eager, graph) the two variants alternate in one process, --repeats rounds; per round an unsynced run gives useful
tokens/s and a run with a device sync around every admission gives the wall time spent in admission.  Reported: medians, the
round-to-round spread (max - min), and the ratio state / whole.  No bar is fixed in advance.

Then the seed launch against what it replaces in eager admission: rwkv7_cache_rows_seed_bf16 zeroing 8 rows of a 32-row cache
(L = 24) against the 3 L index_fill_ calls, alternating blocks, host-timed over a synced block (both are launch-bound: the host's
time to issue the launches is what admission pays).

    python tools/bench_state_store.py [--requests 128] [--repeats 3] [--out profiles/state_store_bench.txt]
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
from rwkvtts_amd.backbone import Cache
from rwkvtts_amd.continuous import ContinuousDecoder
from rwkvtts_amd.prefill import SEED_ZERO, cache_field_table, cache_rows_seed
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
from rwkvtts_amd.state_store import StateStore

DEV = torch.device("cuda:0")
PREFIX = 512


def workload(n, D, seed=0):
    rng = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    mk = lambda t: (torch.randn(t, D, generator=g) * 0.5).to(DEV, torch.bfloat16)
    prefix = mk(PREFIX)
    return prefix, [(mk(rng.randint(32, 128)), rng.randint(128, 512)) for _ in range(n)]


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def engine(m, reqs, store, prefix, admission, time_admission=False, slots=32):
    """One run: (wall s, replays, [s in admission, admissions]).  store: the `state` variant; None: `whole`."""
    eng = ContinuousDecoder(m, slots=slots, max_new_tokens_cap=512, admission=admission, state_store=store)
    if admission == "graph":
        eng.prefill.warm()   # every bucket captured before the timed window
    prompts = [s for s, _ in reqs] if store is not None else [torch.cat([prefix, s]) for s, _ in reqs]
    kw = dict(state="voice") if store is not None else {}
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
        hs = [eng.submit(inputs_embeds=p, max_new_tokens=b, **kw) for p, (_, b) in zip(prompts, reqs)]
        out = eng.run()
        assert all(out[h].numel() == b for h, (_, b) in zip(hs, reqs))
        return eng.replays
    sec, replays = wall(run)
    return sec, replays, spent


def seed_against_index_fill(cfg, say, rounds=5, n=100, rows=8, slots=32):
    cache = Cache.zeros(cfg, slots, DEV, torch.bfloat16)
    tbl = cache_field_table(cache)
    picks = random.Random(1).sample(range(slots), rows)
    rows64 = torch.tensor(picks, dtype=torch.int64, device=DEV)
    dst = torch.tensor(picks, dtype=torch.int32, device=DEV)
    src = torch.full((rows,), SEED_ZERO, dtype=torch.int32, device=DEV)
    L, D, H = len(cache), cfg.hidden_size, cfg.num_heads

    def fills():
        for _ in range(n):
            for st in cache.states:
                st.att_x_prev.index_fill_(0, rows64, 0)
                st.att_kv.index_fill_(0, rows64, 0)
                st.ffn_x_prev.index_fill_(0, rows64, 0)

    def seeds():
        for _ in range(n):
            cache_rows_seed(tbl, tbl, src, dst, rows, L, D, H)
    fills(), seeds()
    tf, ts = [], []
    for _ in range(rounds):
        tf.append(wall(fills)[0] / n * 1e3)
        ts.append(wall(seeds)[0] / n * 1e3)
    mf, ms = statistics.median(tf), statistics.median(ts)
    say(f"reset of {rows} rows of a {slots}-row cache, L = {L}: {3 * L} index_fill_ calls {mf:.3f} ms (spread {max(tf) - min(tf):.3f}) | one "
        f"rwkv7_cache_rows_seed_bf16 launch {ms:.3f} ms (spread {max(ts) - min(ts):.3f}) -> {mf / ms:.1f} x  ({rounds} alternating blocks of {n})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3, help="alternating rounds (at least three for a spread)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = backbone.config_0p4b()
    base = {k: v for k, v in c.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    base["vocab_size"] = 8193
    cfg = RWKV7SpeechConfig(**base)
    m = RWKV7ForSpeech(cfg).init_weights(0).to(DEV, torch.bfloat16).eval()
    prefix, reqs = workload(a.requests, cfg.hidden_size)
    useful = sum(b for _, b in reqs)
    lines = [f"0.4B synthetic bf16 greedy, EOS off; {len(reqs)} requests of one {PREFIX}-token prefix, suffixes 32..128 (mean "
             f"{statistics.mean(s.shape[0] for s, _ in reqs):.0f}), max_new_tokens 128..512 (mean {useful / len(reqs):.0f}); 32 slots"]

    def say(s):
        print(s, flush=True)
        lines.append(s)
    print(lines[0], flush=True)
    store = StateStore(m, 4)
    tc = wall(lambda: store.capture("voice", inputs_embeds=prefix))[0]
    tc = wall(lambda: store.capture("voice", inputs_embeds=prefix))[0]   # the second call: kernels loaded
    say(f"StateStore.capture of the {PREFIX}-token prefix (once per voice, outside the timed runs): {tc * 1e3:.1f} ms")
    for mode in ("eager", "graph"):   # warm-up: kernels, graph pools, the allocator
        for st in (store, None):
            engine(m, reqs[:4], st, prefix, mode, slots=4)
    for mode in ("eager", "graph"):
        res = {"state": [], "whole": []}
        for r in range(a.repeats):
            for name, st in (("state", store), ("whole", None)):
                te, replays, _ = engine(m, reqs, st, prefix, mode)
                ta, _, sp = engine(m, reqs, st, prefix, mode, time_admission=True)
                res[name].append((useful / te, sp[0], sp[0] / max(sp[1], 1) * 1e3, sp[0] / ta * 100))
                say(f"  {mode:5s} round {r} {name}: {te:6.2f} s {useful / te:8.0f} useful tokens/s ({replays} replays) | admission "
                    f"{sp[0]:6.3f} s in {sp[1]} admissions, {sp[0] / max(sp[1], 1) * 1e3:6.2f} ms each, {sp[0] / ta * 100:5.1f} % of {ta:.2f} s synced wall")
        med = lambda name, i: statistics.median(x[i] for x in res[name])
        spr = lambda name, i: max(x[i] for x in res[name]) - min(x[i] for x in res[name])
        for name in res:
            say(f"{mode:5s} {name}: {med(name, 0):8.0f} useful tokens/s (spread {spr(name, 0):.0f}) | admission {med(name, 1):6.3f} s of the wall "
                f"(spread {spr(name, 1):.3f}), {med(name, 2):6.2f} ms each (spread {spr(name, 2):.2f}), {med(name, 3):5.1f} % (spread {spr(name, 3):.1f})")
        say(f"{mode:5s} state / whole: useful tokens/s {med('state', 0) / med('whole', 0):.3f} x (spreads {spr('state', 0):.0f} / {spr('whole', 0):.0f} "
            f"tokens/s) | wall time in admission {med('state', 1) / med('whole', 1):.3f} x ({med('whole', 1):.3f} s -> {med('state', 1):.3f} s)")
    seed_against_index_fill(cfg, say)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
