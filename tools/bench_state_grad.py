"""Cost of training through the recurrent state (ops.wkv7_state_chunked), two parts, one process.

1. Same-process A/B of the two sequential chunked kernels at the configs[1] layer shape (B = 8, T = 4096, H = 16): the stateless
   entries (rwkv7_wkv_chunk_fwd_seq_bf16 / rwkv7_wkv_chunk_bseq_bf16) against the stateful ones with all state pointers set
   (h0 + hT / dhT + dh0), launches interleaved, HIP events on the launch stream; median of `iters` pairs per kernel.
2. One truncated-BPTT forward + backward of the 0.4B Spark model (B = 8, two 2048-token segments through a differentiable cache, cut
   with Cache.detach() between them) against the stateless 4096-token forward + backward (no optimizer in either; median of `steps`).

    python tools/bench_state_grad.py [iters] [steps]        (steps = 0: the kernel A/B only)"""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rwkvtts_amd import _lib, ops
from rwkvtts_amd.synthetic import make_wkv_inputs

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 30
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = "cuda:0"
L = _lib.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr())


def kernel_ab():
    B, T, H = 8, 4096, 16
    w, q, k, v, a, b = make_wkv_inputs(B, T, H, 1234, torch.bfloat16, dev)
    dy = torch.randn(B, T, H, 64, device=dev).bfloat16()
    tinv = ops.wkv7_chunk_prep(w, a, b)
    y, sa = torch.empty_like(v), torch.empty(B, T, H, 64, device=dev)
    hs = torch.empty(B, H, T // 32, ops.Q15_REC, dtype=torch.int16, device=dev)
    e_vk, z = torch.empty_like(hs), torch.empty(B, T, H, 64, device=dev)
    h0, hT, dhT, dh0 = [torch.randn(B, H, 64, 64, device=dev) * 0.1 for _ in range(4)]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fio = (P(w), P(q), P(k), P(v), P(a), P(b), P(tinv), P(y), P(sa), P(hs))
    bio = (P(w), P(q), P(a), P(b), P(dy), P(tinv), P(e_vk), P(z))
    pairs = {
        "wkv7c_fwd9": (lambda: L.rwkv7_wkv_chunk_fwd_seq_bf16(B, T, H, *fio, None, 0, st),
                       lambda: L.rwkv7_wkv_chunk_fwd_state_bf16(B, T, H, *fio, P(h0), P(hT), st)),
        "wkv7c_bseq": (lambda: L.rwkv7_wkv_chunk_bseq_bf16(B, T, H, *bio, None, 0, st),
                       lambda: L.rwkv7_wkv_chunk_bseq_state_bf16(B, T, H, *bio, P(dhT), P(dh0), st)),
    }
    out = {}
    for name, fns in pairs.items():
        for fn in fns:
            for _ in range(3):
                assert fn() == 0
        torch.cuda.synchronize()
        ts = [[], []]
        for _ in range(iters):
            for i, fn in enumerate(fns):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                assert fn() == 0
                e.record()
                ts[i].append((s, e))
        torch.cuda.synchronize()
        med = [statistics.median(s.elapsed_time(e) for s, e in t) * 1e3 for t in ts]
        out[name] = {"stateless_us": round(med[0], 1), "state_us": round(med[1], 1), "delta_pct": round(100 * (med[1] / med[0] - 1), 2)}
        print(json.dumps({"kernel": name, "B": B, "T": T, "H": H, "iters": iters, **out[name]}), flush=True)
    return out


def step_times():
    from rwkvtts_amd import backbone
    from rwkvtts_amd.backbone import Cache
    from rwkvtts_amd.layouts import synthetic_spark_batch
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
    base = backbone.config_0p4b()
    kw = {k: v for k, v in base.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    model = RWKV7ForSpeech(RWKV7SpeechConfig(**kw)).init_weights(seed=0).to(device=dev, dtype=torch.bfloat16).train()
    B, T = 8, 4096
    with torch.no_grad():
        batch = synthetic_spark_batch(model, B, T, seed=1234)
    backbone.mark_all_ones(batch["attention_mask"], True)

    def stateless():
        model(**batch).loss.backward()

    def tbptt():
        cache = Cache.zeros(model.config, B, dev, torch.bfloat16, differentiable=True)
        for lo in (0, T // 2):
            seg = {n: t[:, lo:lo + T // 2] for n, t in batch.items()}
            backbone.mark_all_ones(seg["attention_mask"], True)
            model(**seg, past_key_values=cache, use_cache=True).loss.backward()
            cache = cache.detach()

    res = {}
    for name, fn in (("stateless_4096", stateless), ("tbptt_2x2048", tbptt)):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(steps):
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = round(statistics.median(ts), 2)
    res["ratio"] = round(res["tbptt_2x2048"] / res["stateless_4096"], 3)
    print(json.dumps({"step_fwd_bwd_ms": res, "model": "0.4b spark", "B": B, "T": T, "steps": steps}), flush=True)
    return res


if __name__ == "__main__":
    kernel_ab()
    if steps > 0:
        step_times()
