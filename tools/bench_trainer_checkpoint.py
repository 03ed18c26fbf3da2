"""Cost of DataParallelTrainer.save_checkpoint / load_checkpoint and of the digest kernel, one GPU.

    python tools/bench_trainer_checkpoint.py [--model 0.4b] [--batch 2] [--seq-len 2048] [--dir DIR] [--rounds 2]

Prints one JSON line:
  digest_pass_ms     rwkv7_buf_digest_u32 (both launches) over the fp32 masters, alone on the stream; digest_gbps = bytes read / time
  sumsq_pass_ms      rwkv7_grad_sumsq_bf16 over a bf16 buffer of the SAME number of bytes, in the same process: the yardstick, both
                     being one-pass two-launch reductions; sumsq_gbps likewise; digest_over_sumsq is the ratio of the times
  digest_call_ms     trainer.digest(): four buffers and the read-back, host clock
  save_s / load_s    wall time of save_checkpoint / load_checkpoint (host clock; both end synchronised), per round, and the
                     checkpoint's size -- disk and page cache of the machine are part of these two
Nothing here is on the training step; there is no bar, the numbers are recorded (profiles/trainer_checkpoint_bench.txt)."""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="0.4b", choices=["0.1b", "0.4b", "1.5b"])
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--seq-len", type=int, default=2048)
    ap.add_argument("--dir", default=None, help="where the checkpoints go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()

    import torch
    from rwkvtts_amd import _lib, backbone, digest, trainer
    from rwkvtts_amd.layouts import synthetic_spark_batch
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    base = {"0.1b": backbone.config_0p1b, "0.4b": backbone.config_0p4b, "1.5b": backbone.config_1p5b}[a.model]()
    base_kw = {k: v for k, v in base.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    kw = dict(lr=1e-4, warmup_steps=10, total_steps=1000)

    def make(seed):
        model = RWKV7ForSpeech(RWKV7SpeechConfig(**base_kw)).init_weights(seed=seed).to(device=dev, dtype=torch.bfloat16).train()
        return model, trainer.DataParallelTrainer(model, **kw)

    model, tr = make(0)
    for i in range(2):   # non-trivial moments
        tr.step(**synthetic_spark_batch(model, a.batch, a.seq_len, seed=1234 + i))
    torch.cuda.synchronize()
    n = tr.flat.numel
    res = {"model": a.model, "numel": n, "device": torch.cuda.get_device_name(dev)}

    def stats(xs):
        return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}

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

    lib = _lib.lib()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nbytes = 4 * n
    ws = digest.workspace(n, dev)
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    g16 = torch.randn(2 * n, device=dev, dtype=torch.bfloat16)   # as many bytes as the fp32 masters
    ws32 = torch.empty(lib.rwkv7_grad_sumsq_workspace_bytes(2 * n) // 4, dtype=torch.float32, device=dev)
    ss = torch.zeros(1, device=dev)
    # alternate the two, so that a drift of the clock shows in both
    d1 = pass_ms(lambda: lib.rwkv7_buf_digest_u32(n, 0, P(tr.master), P(ws), P(out), 0, st))
    s1 = pass_ms(lambda: lib.rwkv7_grad_sumsq_bf16(2 * n, P(g16), P(ws32), P(ss), 0, st))
    d2 = pass_ms(lambda: lib.rwkv7_buf_digest_u32(n, 0, P(tr.master), P(ws), P(out), 0, st))
    s2 = pass_ms(lambda: lib.rwkv7_grad_sumsq_bf16(2 * n, P(g16), P(ws32), P(ss), 0, st))
    res["bytes_per_pass"] = nbytes
    res["digest_pass_ms"], res["sumsq_pass_ms"] = [d1, d2], [s1, s2]
    dm, sm = min(d1["median"], d2["median"]), min(s1["median"], s2["median"])
    res["digest_gbps"], res["sumsq_gbps"] = round(nbytes / dm / 1e6, 1), round(nbytes / sm / 1e6, 1)
    res["digest_over_sumsq"] = round(dm / sm, 3)
    assert int(out.item()) & digest.MASK64 == tr.digest()["master"]
    del g16, ws32

    calls = []
    for _ in range(5):
        t0 = time.perf_counter()
        tr.digest()
        calls.append((time.perf_counter() - t0) * 1e3)
    res["digest_call_ms"] = stats(calls[1:])

    d = a.dir or tempfile.mkdtemp(prefix="rwkv7_ckpt_bench_")
    try:
        saves, loads = [], []
        model2, t2 = make(1)
        for r in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            path = tr.save_checkpoint(d, tag=f"round_{r}", extra={"round": r}, keep_last=1)
            saves.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            t2.load_checkpoint(d)
            torch.cuda.synchronize()
            loads.append(time.perf_counter() - t0)
        res["checkpoint_bytes"] = sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))
        res["save_s"], res["load_s"] = [round(x, 3) for x in saves], [round(x, 3) for x in loads]
        assert t2.digest() == tr.digest() and torch.equal(t2.master, tr.master)
    finally:
        if a.dir is None:
            shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
