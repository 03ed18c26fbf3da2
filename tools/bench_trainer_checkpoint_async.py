"""Cost of the non-blocking checkpoints, one GPU, one process, series alternated.

    python tools/bench_trainer_checkpoint_async.py [--model 0.4b] [--batch 2] [--seq-len 2048] [--dir DIR] [--rounds 2] [--steps 12]

Prints one JSON line:
  fused_pass_ms      rwkv7_buf_snapshot_digest_u32 (both launches) over the fp32 masters into a second buffer, alone on the stream
  unfused_pass_ms    dst.copy_(src) followed by rwkv7_buf_digest_u32 over the same buffer: the route the fused pass replaces (3 passes
                     of traffic against 2); fused_over_unfused is the ratio of the better medians
  step_ms            one step() (the synthetic batch's embedding lookups included), synchronised, nothing pending: median of --steps
  blocking_s         wall time of save_checkpoint(blocking=True), per round
  stall_s            wall time of save_checkpoint(blocking=False) up to its return, per round (round 0 allocates the staging buffers);
                     finalise_s: the checkpoint_wait() that follows at once, i.e. the writer's duration seen from the caller
  interference       steps taken while a writer is active: their median against step_ms, how many there were, the writer's duration
                     (save's return until checkpoint_done(), resolved to one step), and extra_s = the sum over those steps of
                     (step time - step_ms): what the overlapped save cost the run, to be read against blocking_s
  step_ms_after      the same series as step_ms, taken after the overlapped save: the second baseline (ratio_vs_after, extra_s_vs_after)
No bar is set for these; the numbers are recorded (profiles/trainer_checkpoint_async_bench.txt)."""
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
    ap.add_argument("--steps", type=int, default=12)
    a = ap.parse_args()

    import torch
    from rwkvtts_amd import _lib, backbone, digest, trainer
    from rwkvtts_amd.layouts import synthetic_spark_batch
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    base = {"0.1b": backbone.config_0p1b, "0.4b": backbone.config_0p4b, "1.5b": backbone.config_1p5b}[a.model]()
    base_kw = {k: v for k, v in base.to_dict().items() if k in backbone.RWKV7Config.__dataclass_fields__ and k != "extra"}
    model = RWKV7ForSpeech(RWKV7SpeechConfig(**base_kw)).init_weights(seed=0).to(device=dev, dtype=torch.bfloat16).train()
    tr = trainer.DataParallelTrainer(model, lr=1e-4, warmup_steps=10, total_steps=1000)

    def timed_step(i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.step(**synthetic_spark_batch(model, a.batch, a.seq_len, seed=1234 + i % 4))   # the embedding lookups belong to the step
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for i in range(3):   # non-trivial moments, the reducer's bucket cut, warm kernels
        timed_step(i)
    n = tr.flat.numel
    res = {"model": a.model, "numel": n, "device": torch.cuda.get_device_name(dev), "bytes_per_buffer": 4 * n}

    def stats(xs):
        return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}

    def pass_ms(call, reps=20, warm=3):
        out = []
        for i in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if i >= warm:
                out.append(e0.elapsed_time(e1))
        return stats(out)

    # ---- the kernel against the route it replaces ----
    lib = _lib.lib()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ws = digest.workspace(n, dev)
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    dst = torch.empty_like(tr.master)

    def fused():
        assert lib.rwkv7_buf_snapshot_digest_u32(n, 0, P(tr.master), P(dst), P(ws), P(out), 0, st) == 0

    def unfused():
        dst.copy_(tr.master)
        assert lib.rwkv7_buf_digest_u32(n, 0, P(dst), P(ws), P(out), 0, st) == 0

    f1, u1, f2, u2 = pass_ms(fused), pass_ms(unfused), pass_ms(fused), pass_ms(unfused)   # alternated: a drift shows in both
    res["fused_pass_ms"], res["unfused_pass_ms"] = [f1, f2], [u1, u2]
    fm, um = min(f1["median"], f2["median"]), min(u1["median"], u2["median"])
    res["fused_gbps_read_plus_write"] = round(8 * n / fm / 1e6, 1)
    res["fused_over_unfused"] = round(fm / um, 3)
    fused()
    assert int(out.item()) & digest.MASK64 == tr.digest()["master"] and torch.equal(dst, tr.master)
    del dst

    # ---- the stall and the interference ----
    res["step_ms"] = stats([timed_step(i) for i in range(a.steps)])
    idle = res["step_ms"]["median"]
    d = a.dir or tempfile.mkdtemp(prefix="rwkv7_ckpt_async_bench_")
    try:
        blocking, stall, finalise = [], [], []
        for r in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.save_checkpoint(d, tag=f"blocking_{r}", keep_last=1)
            blocking.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            tr.save_checkpoint(d, tag=f"async_{r}", keep_last=1, blocking=False)
            t1 = time.perf_counter()
            tr.checkpoint_wait()
            stall.append(t1 - t0)
            finalise.append(time.perf_counter() - t1)
        res["blocking_s"], res["stall_s"], res["finalise_s"] = ([round(x, 4) for x in xs] for xs in (blocking, stall, finalise))
        res["stall_in_steps"] = round(min(stall) * 1e3 / idle, 3)
        t0 = time.perf_counter()
        tr.save_checkpoint(d, tag="overlapped", keep_last=1, blocking=False)
        t1 = time.perf_counter()
        during, i = [], 0
        while not tr.checkpoint_done():
            during.append(timed_step(i))
            i += 1
        writer_s = time.perf_counter() - t1
        path = tr.checkpoint_wait()
        res["interference"] = {"stall_s": round(t1 - t0, 4), "steps": len(during), "writer_s": round(writer_s, 3),
                               "step_ms_during": stats(during) if during else None,
                               "ratio": round(statistics.median(during) / idle, 3) if during else None,
                               "extra_s": round(sum(x - idle for x in during) / 1e3, 3)}
        res["step_ms_after"] = stats([timed_step(i) for i in range(a.steps)])   # the second baseline: a drift of the clock shows here
        after = res["step_ms_after"]["median"]
        if during:
            res["interference"]["ratio_vs_after"] = round(statistics.median(during) / after, 3)
            res["interference"]["extra_s_vs_after"] = round(sum(x - after for x in during) / 1e3, 3)
        t2 = trainer.DataParallelTrainer(
            RWKV7ForSpeech(RWKV7SpeechConfig(**base_kw)).init_weights(seed=1).to(device=dev, dtype=torch.bfloat16).train(),
            lr=1e-4, warmup_steps=10, total_steps=1000)
        t2.load_checkpoint(d)   # `overlapped`: the state before the steps taken during its write
        meta = json.load(open(os.path.join(path, "meta.json")))
        assert meta["digest"] == {k: "%016x" % v for k, v in t2.digest().items()} and t2.step_idx == meta["step_idx"] == tr.step_idx - len(during) - a.steps
        res["checkpoint_bytes"] = sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))
    finally:
        tr.checkpoint_wait()
        if a.dir is None:
            shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
