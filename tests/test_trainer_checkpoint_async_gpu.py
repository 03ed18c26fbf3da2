"""GPU (-m gpu): rwkv7_buf_snapshot_digest_u32 (csrc/buf_digest.hip) -- the copy bit for bit, the digest against the numpy
restatement and against rwkv7_buf_digest_u32, nothing written behind n_words -- and DataParallelTrainer.save_checkpoint(
blocking=False) on the HIP AdamW path: the tiny bf16 Spark model of test_trainer_checkpoint_gpu.py with its dropout on, the writer
thread held inside trainer._write_synced until the later steps have RUN (torch.cuda.synchronize()), so that the result shows that
later steps do not reach the files, whatever the timing."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from rwkvtts_amd import _lib, digest
from test_trainer_checkpoint import ref_digest
from test_trainer_checkpoint_async import Gate, _hex, _same_files
from test_trainer_checkpoint_gpu import DEV, FIRSTS, K, KW, M, SIZES, TILE, P, _advance, _model, _state, words  # noqa: F401  (words: a fixture)
from test_trainer_gpu import _free_port

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a5aa5a5
SEED = 0xfedcba9876543210


def _snap(src, n, first, dst, accumulate=0, start=0, null=()):
    """One call of the C entry on the first n words of the int32 tensor src into dst; returns (rc, out[0] as an unsigned int).  The
    workspace is filled with garbage first; `null`: the pointers to pass as NULL."""
    lib = _lib.lib()
    ws = torch.full((max(1, lib.rwkv7_buf_digest_workspace_bytes(n) // 8),), -1, dtype=torch.int64, device=DEV)
    out = torch.tensor([start - (1 << 64) if start >> 63 else start], dtype=torch.int64, device=DEV)
    ptr = lambda name, t: None if name in null or (n == 0 and name != "out") else P(t)
    rc = lib.rwkv7_buf_snapshot_digest_u32(n, first, ptr("src", src), ptr("dst", dst), ptr("ws", ws), ptr("out", out), accumulate,
                                           ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    return rc, int(out.item()) & digest.MASK64


def _sentinels(n=SIZES[-1]):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.timeout(120)
def test_the_library_exports_the_entry():
    assert "rwkv7_buf_snapshot_digest_u32" in _lib.exported_symbols() and hasattr(_lib.lib(), "rwkv7_buf_snapshot_digest_u32")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("n", SIZES)
def test_snapshot_copies_bit_for_bit_and_digests_what_it_wrote(n, first, words):
    host, dev = words
    want = ref_digest(host[:n], first)
    dst = _sentinels()
    rc, got = _snap(dev, n, first, dst)                          # a prefix of a longer buffer into a prefix of a longer buffer
    assert rc == 0 and got == want, (n, first, hex(got), hex(want))
    d = _u32(dst)
    assert np.array_equal(d[:n], host[:n]), "the copy must be exact"
    assert (d[n:] == SENTINEL).all(), "words behind n_words must not be written"
    assert np.array_equal(_u32(dev), host), "src is only read"
    lib = _lib.lib()
    ws = torch.full((max(1, lib.rwkv7_buf_digest_workspace_bytes(n) // 8),), -1, dtype=torch.int64, device=DEV)
    out = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert lib.rwkv7_buf_digest_u32(n, first, P(dev) if n else None, P(ws) if n else None, P(out), 0, None) == 0
    torch.cuda.synchronize()
    assert int(out.item()) & digest.MASK64 == got, "the digest entry gives the same word over the same buffer"
    assert _snap(dev, n, first, dst) == (0, want), "two calls must give the same word"
    assert _snap(dev, n, first, dst, accumulate=1, start=SEED) == (0, (SEED + want) & digest.MASK64)
    assert _snap(dev, n, first, dst, accumulate=0, start=SEED) == (0, want)
    assert np.array_equal(_u32(dst)[:n], host[:n]) and (_u32(dst)[n:] == SENTINEL).all()
    if n == 0:
        assert want == 0


@pytest.mark.timeout(120)
def test_views_of_bf16_and_fp32_tensors_snapshot_their_raw_words():
    g = torch.Generator().manual_seed(0)
    f = torch.randn(TILE + 64, generator=g).to(DEV)
    fd = torch.zeros_like(f)
    assert digest.snapshot_digest(f, fd, 5) == ref_digest(_u32(f), 5) == digest.buf_digest(f, 5)
    assert np.array_equal(_u32(fd), _u32(f))
    b = torch.randn(2 * TILE + 1024, generator=g).bfloat16().to(DEV)
    raw = b.cpu().view(torch.int16).numpy().view(np.uint32)
    bd = torch.zeros_like(b)
    assert digest.snapshot_digest(b, bd, 7) == ref_digest(raw, 7)
    assert torch.equal(bd.view(torch.int16), b.view(torch.int16))
    bd.zero_()
    # a slice: two bf16 elements are one word; what surrounds the destination slice stays as it was
    assert digest.snapshot_digest(b[256:1280], bd[512:1536], 128) == ref_digest(raw[128:640], 128) == digest.buf_digest(b[256:1280], 128)
    assert torch.equal(bd[512:1536].view(torch.int16), b[256:1280].view(torch.int16)) and not bd[:512].any() and not bd[1536:].any()
    with pytest.raises(ValueError):
        digest.snapshot_digest(b[:6], bd[:6])                   # 3 words: not a multiple of 4
    with pytest.raises(ValueError):
        digest.snapshot_digest(b[:8], fd[:8])                   # another dtype


@pytest.mark.timeout(120)
def test_bad_arguments_return_an_error_and_launch_nothing(words):
    host, dev = words
    dst = _sentinels()
    assert _snap(dev, 6, 0, dst, start=77) == (-4, 77)                  # n_words % 4 != 0
    assert _snap(dev[1:], 4, 0, dst, start=77) == (-4, 77)              # src not 16-byte aligned
    assert _snap(dev, 4, 0, dst[1:], start=77) == (-4, 77)              # dst not 16-byte aligned
    assert _snap(dev, -4, 0, dst, start=77) == (-1, 77)
    assert _snap(dev, 4, -1, dst, start=77) == (-1, 77)
    for name in ("src", "dst", "ws"):
        assert _snap(dev, 4, 0, dst, start=77, null=(name,)) == (-1, 77), name
    lib = _lib.lib()
    ws = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert lib.rwkv7_buf_snapshot_digest_u32(4, 0, P(dev), P(dst), P(ws), None, 0, None) == -1
    both = torch.cat([dev[:64], _sentinels(64)])                        # dst = src + 16 bytes: the ranges overlap
    before = _u32(both).copy()
    assert _snap(both, 8, 0, both[4:], start=77) == (-1, 77)
    assert _snap(both[4:], 8, 0, both, start=77) == (-1, 77)
    assert _snap(both, 64, 0, both[60:], start=77) == (-1, 77)
    torch.cuda.synchronize()
    assert (_u32(dst) == SENTINEL).all() and np.array_equal(_u32(both), before)
    assert _snap(both, 64, 3, both[64:]) == (0, ref_digest(host[:64], 3))   # adjacent ranges do not overlap
    assert np.array_equal(_u32(both)[64:], host[:64])


# ---- the non-blocking save on the HIP AdamW path ------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", ["plain", "allreduce"])
def test_non_blocking_save_on_the_hip_path_holds_the_state_at_step_k(mode, tmp_path, monkeypatch):
    from rwkvtts_amd import trainer
    kw = dict(KW)
    if mode == "allreduce":                       # one-rank RCCL group with the collectives forced on, as test_trainer_gpu.py does
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
        kw.update(bucket_bytes=64 << 10, force_allreduce=True)
    monkeypatch.setattr(trainer, "CHECKPOINT_PIECE_BYTES", 100_003)     # many pieces per buffer, a ragged last one
    tb = None
    try:
        ta = trainer.DataParallelTrainer(_model(3), **kw)
        assert ta.hip_adamw and ta.reducer.enabled == (mode == "allreduce")
        assert ta.flat.numel * 4 > 3 * trainer.CHECKPOINT_PIECE_BYTES
        torch.manual_seed(11)
        _advance(ta, range(K + M))
        a = _state(ta)
        tb = trainer.DataParallelTrainer(_model(3), **kw)
        torch.manual_seed(11)
        _advance(tb, range(K))
        at_k, digest_k = _state(tb), tb.digest()
        d, blocking_dir = tmp_path / "async", tmp_path / "blocking"
        gate = Gate(monkeypatch)
        path = tb.save_checkpoint(str(d), extra={"cursor": K}, blocking=False)
        _advance(tb, range(K, K + M))
        torch.cuda.synchronize()                  # the M later steps have run; the writer has not copied a byte yet
        assert gate.entered.wait(120) and gate.calls == 0
        assert (d / f"step_{K}.tmp").is_dir() and not (d / f"step_{K}").exists() and not (d / "latest").exists()
        p = tb.pending_checkpoint
        assert not tb.checkpoint_done() and (p.step_idx, p.path, p.digests) == (K, path, digest_k)
        gate.release.set()
        assert tb.checkpoint_wait() == path == str(d / f"step_{K}")
        assert tb.pending_checkpoint is None and tb.checkpoint_done() and (d / "latest").read_text() == f"step_{K}"
        b = _state(tb)
        for k in ("param", "master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a[k], b[k]), k     # the save did not disturb the run it was taken from
        torch.manual_seed(999)                    # the new process: other initial weights, another generator state
        mc = _model(5)
        tc = trainer.DataParallelTrainer(mc, **kw)
        assert tc.load_checkpoint(str(d)) == {"cursor": K}
        c = _state(tc)
        for k in ("param", "master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(at_k[k], c[k]), k  # the state at step K, not at K + M
        assert (c["step_idx"], c["last_lr"]) == (at_k["step_idx"], at_k["last_lr"])
        stored = json.loads((d / f"step_{K}" / "meta.json").read_text())["digest"]
        assert stored == _hex(digest_k) == _hex(tc.digest())            # tc.digest(): the kernel, on what is in device memory now
        tc.save_checkpoint(str(blocking_dir), extra={"cursor": K})      # the same state, the blocking way
        _same_files(str(d / f"step_{K}"), str(blocking_dir / f"step_{K}"))
        _advance(tc, range(K, K + M))
        c = _state(tc)
        for k in ("param", "master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a[k], c[k]), k
        assert (a["step_idx"], a["last_lr"]) == (c["step_idx"], c["last_lr"])
        lo = tc.flat.flat_param.data_ptr()
        hi = lo + tc.flat.flat_param.numel() * 2
        assert all(lo <= q.data_ptr() < hi for q in mc.parameters()), "the parameters must stay views of flat_param"
        # staging: same dtype and length as the range, released and allocated again
        staged = tb._ckpt_staging["bufs"]
        assert sorted(staged) == ["exp_avg", "exp_avg_sq", "master", "param"]
        assert staged["param"].dtype == torch.bfloat16 and staged["master"].dtype == torch.float32
        assert all(s.numel() == tb.flat.numel and s.is_cuda for s in staged.values())
        assert torch.equal(staged["master"], at_k["master"]) and torch.equal(staged["param"], at_k["param"])
        tb.release_checkpoint_staging()
        assert tb._ckpt_staging is None
        again = tb.save_checkpoint(str(d), tag="again", blocking=False)
        assert tb.checkpoint_wait() == again and (d / "latest").read_text() == "again"
        assert json.loads((d / "again" / "meta.json").read_text())["digest"] == _hex(tb.digest())
        raw = np.fromfile(str(d / "again" / f"range_{0:012d}_{tb.flat.numel:012d}.master.bin"), dtype=np.uint32)
        assert np.array_equal(raw, _u32(tb.master))
    finally:
        if tb is not None and tb.pending_checkpoint is not None:        # a failed assertion must not leave the writer held
            gate.release.set()
            tb.pending_checkpoint.thread.join()
        if mode == "allreduce":
            dist.destroy_process_group()
