"""Cost of carrying per-sequence states through packed cu_seqlens rows, two parts, one process.

(a) Same-process A/B of the two sequential chunked kernels on a configs[1]-sized packed row (total 32768 tokens, H = 16, lengths
    drawn from 200 .. 4000, laid out by ops.packed_state_layout): the stateless packed entries (rwkv7_wkv_chunk_fwd_seq_bf16 /
    rwkv7_wkv_chunk_bseq_bf16) against the state+seq ones with every state pointer set (h0 + hT / dhT + dh0), launches interleaved,
    HIP events on the launch stream; median of `iters` pairs per kernel.
(b) Prefill of 32 ragged prompts (lengths 200 .. 1000, the 0.4B Spark backbone, bf16, no grad) from a zero cache: packed into one
    cu_seqlens row with the cache against today's left-padded [32, Tmax] stateful prefill (median of `steps`), and how far the two
    resulting caches are apart.

    python tools/bench_varlen_state.py [iters] [steps]        (steps = 0: the kernel A/B only)"""
import ctypes
import json
import os
import random
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


def ragged(total, lo, hi, seed):
    rng = random.Random(seed)
    lens = []
    while sum(lens) < total:
        lens.append(min(rng.randint(lo, hi), total - sum(lens)))
    return lens


def kernel_ab():
    H = 16
    lens = ragged(32768, 200, 4000, 7)
    lay = ops.packed_state_layout(lens, train=False)
    T, N = lay.t_al, len(lens)
    w, q, k, v, a, b = make_wkv_inputs(1, T, H, 1234, torch.bfloat16, dev)
    dy = torch.randn(1, T, H, 64, device=dev).bfloat16()
    so = lay.seq_off.to(dev)
    tinv = ops.wkv7_chunk_prep(w, a, b)
    y, sa = torch.empty_like(v), torch.empty(1, T, H, 64, device=dev)
    hs = torch.empty(1, H, T // 32, ops.Q15_REC, dtype=torch.int16, device=dev)
    e_vk, z = torch.empty_like(hs), torch.empty(1, T, H, 64, device=dev)
    h0, hT, dhT, dh0 = [torch.randn(N, H, 64, 64, device=dev) * 0.1 for _ in range(4)]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fio = (P(w), P(q), P(k), P(v), P(a), P(b), P(tinv), P(y), P(sa), P(hs))
    bio = (P(w), P(q), P(a), P(b), P(dy), P(tinv), P(e_vk), P(z))
    pairs = {
        "wkv7c_fwd9": (lambda: L.rwkv7_wkv_chunk_fwd_seq_bf16(1, T, H, *fio, P(so), N, st),
                       lambda: L.rwkv7_wkv_chunk_fwd_state_seq_bf16(1, T, H, *fio, P(so), N, P(h0), P(hT), st)),
        "wkv7c_bseq": (lambda: L.rwkv7_wkv_chunk_bseq_bf16(1, T, H, *bio, P(so), N, st),
                       lambda: L.rwkv7_wkv_chunk_bseq_state_seq_bf16(1, T, H, *bio, P(so), N, P(dhT), P(dh0), st)),
    }
    out = {"shape": {"total": sum(lens), "T_aligned": T, "H": H, "nseq": N}}
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
                e.synchronize()
                ts[i].append(s.elapsed_time(e) * 1e3)
        m0, m1 = statistics.median(ts[0]), statistics.median(ts[1])
        out[name] = {"stateless_seq_us": round(m0, 1), "state_seq_us": round(m1, 1), "delta_pct": round(100 * (m1 / m0 - 1), 2)}
    return out


def prefill():
    from rwkvtts_amd import backbone
    from rwkvtts_amd.backbone import Cache, RWKV7Model
    cfg = backbone.config_0p4b()
    torch.manual_seed(0)
    model = RWKV7Model(cfg)
    backbone.init_weights(model, cfg, seed=0)
    model = model.to(dev).to(torch.bfloat16).eval()
    lens = [random.Random(11 + i).randint(200, 1000) for i in range(32)]
    B, Tmax, D = len(lens), max(lens), cfg.hidden_size
    g = torch.Generator().manual_seed(3)
    xs = [(torch.randn(n, D, generator=g) * 0.5).to(dev, torch.bfloat16) for n in lens]
    xpad = torch.zeros(B, Tmax, D, device=dev, dtype=torch.bfloat16)
    mask = torch.zeros(B, Tmax, dtype=torch.long, device=dev)
    for i, (n, x) in enumerate(zip(lens, xs)):
        xpad[i, Tmax - n:] = x        # left-padded, as generate prefills
        mask[i, Tmax - n:] = 1
    xpk = torch.cat(xs, 0).unsqueeze(0)
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)

    def padded():
        c = Cache.zeros(cfg, B, dev, torch.bfloat16)
        model(inputs_embeds=xpad, attention_mask=mask, past_key_values=c, use_cache=True)
        return c

    def packed():
        c = Cache.zeros(cfg, B, dev, torch.bfloat16)
        model(inputs_embeds=xpk, cu_seqlens=cu, past_key_values=c)
        return c

    res = {}
    with torch.no_grad():
        for name, fn in (("left_padded", padded), ("packed", packed)):
            fn()
            torch.cuda.synchronize()
        t = {"left_padded": [], "packed": []}
        for _ in range(steps):
            for name, fn in (("left_padded", padded), ("packed", packed)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) * 1e3)
        cp, cl = padded(), packed()
    kv = max(((a.att_kv - b.att_kv).norm() / b.att_kv.norm()).item() for a, b in zip(cl.states, cp.states))
    xp = max(((a.ffn_x_prev.float() - b.ffn_x_prev.float()).norm() / b.ffn_x_prev.float().norm()).item()
             for a, b in zip(cl.states, cp.states))
    res = {"prompts": B, "tokens": sum(lens), "Tmax": Tmax, "padded_positions": B * Tmax,
           "left_padded_ms": round(statistics.median(t["left_padded"]), 2), "packed_ms": round(statistics.median(t["packed"]), 2),
           "cache_rel_l2_att_kv_worst_layer": float(f"{kv:.3g}"), "cache_rel_l2_ffn_x_prev_worst_layer": float(f"{xp:.3g}")}
    res["speedup"] = round(res["left_padded_ms"] / res["packed_ms"], 2)
    return res


if __name__ == "__main__":
    r = {"device": torch.cuda.get_device_name(0), "kernel_ab": kernel_ab()}
    print(json.dumps(r["kernel_ab"]), flush=True)
    if steps > 0:
        r["prefill"] = prefill()
        print(json.dumps(r["prefill"]), flush=True)
    print(json.dumps(r))
