"""GPU (-m gpu): rwkv7_buf_digest_u32 (csrc/buf_digest.hip) against the numpy restatement of test_trainer_checkpoint.py, bit for
bit, and the resume guarantee of DataParallelTrainer.save_checkpoint / load_checkpoint on the HIP AdamW path: a tiny bf16 Spark
model WITH its Dropout(0.02) on inputs_embeds left on, so the run depends on the device RNG and the test fails unless it is restored.
Like its neighbours this file relies on run-to-run bit reproducibility of the step."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from rwkvtts_amd import _lib, digest
from test_trainer_checkpoint import ref_digest
from test_trainer_gpu import _free_port

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TILE = digest.TILE_WORDS
SIZES = [0, 4, TILE - 4, TILE, TILE + 4, 5 * TILE + 12]
FIRSTS = [0, 12, 2 ** 32 + 8]
P = lambda t: ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def words():
    """5 tiles + 12 random 32-bit patterns (NaN and Inf encodings of both float formats among them), on the host and on the device.
    Read-only for the tests that share it."""
    w = np.random.default_rng(0).integers(0, 2 ** 32, size=SIZES[-1], dtype=np.uint64).astype(np.uint32)
    w[:8] = [0x7fc00000, 0x7f800000, 0xff800000, 0xffffffff, 0x7f807fc0, 0, 0x80000000, 1]
    return w, torch.from_numpy(w.view(np.int32)).to(DEV)


def _kernel(t, n, first, accumulate=0, start=0):
    """One call of the C entry on the first n words of the int32 tensor t; returns (rc, out[0] as an unsigned int)."""
    lib = _lib.lib()
    ws = torch.full((max(1, lib.rwkv7_buf_digest_workspace_bytes(n) // 8),), -1, dtype=torch.int64, device=DEV)   # garbage: never read before written
    out = torch.tensor([start - (1 << 64) if start >> 63 else start], dtype=torch.int64, device=DEV)
    rc = lib.rwkv7_buf_digest_u32(n, first, P(t) if n else None, P(ws) if n else None, P(out),
                                  accumulate, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    return rc, int(out.item()) & digest.MASK64


@pytest.mark.timeout(120)
def test_workspace_query_follows_the_documented_tile():
    q = _lib.lib().rwkv7_buf_digest_workspace_bytes
    assert [q(0), q(4), q(TILE), q(TILE + 4), q(5 * TILE + 12)] == [0, 8, 8, 16, 48]
    assert q(2 ** 33) == 8 * (2 ** 33 // TILE)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_the_restatement_bit_for_bit(n, first, words):
    host, dev = words
    want = ref_digest(host[:n], first)
    rc, got = _kernel(dev, n, first)              # a prefix of a longer buffer: what lies behind it must not count
    assert rc == 0 and got == want, (n, first, hex(got), hex(want))
    assert _kernel(dev, n, first) == (0, want), "two calls must give the same word"
    seed = 0xfedcba9876543210
    assert _kernel(dev, n, first, accumulate=1, start=seed) == (0, (seed + want) & digest.MASK64)
    assert _kernel(dev, n, first, accumulate=0, start=seed) == (0, want)
    if n == 0:
        assert want == 0


@pytest.mark.timeout(120)
def test_three_unequal_slabs_with_global_indices_add_to_the_whole(words):
    host, dev = words
    first = 2 ** 32 + 8
    whole = digest.buf_digest(dev, first)
    assert whole == ref_digest(host, first)
    cuts = [(0, 8), (8, TILE + 20), (TILE + 20, host.size)]
    parts = [digest.buf_digest(dev[a:b], first + a) for a, b in cuts]
    assert parts == [ref_digest(host[a:b], first + a) for a, b in cuts]
    assert sum(parts) % 2 ** 64 == whole
    assert digest.buf_digest(dev.cpu(), first) == whole, "fallback and kernel must agree"
    # the buffer is only read
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), host)


@pytest.mark.timeout(120)
def test_views_of_bf16_and_fp32_tensors_digest_their_raw_words():
    g = torch.Generator().manual_seed(0)
    f = torch.randn(TILE + 64, generator=g).to(DEV)
    assert digest.buf_digest(f, 5) == ref_digest(f.cpu().numpy().view(np.uint32), 5)
    b = torch.randn(2 * TILE + 1024, generator=g).bfloat16().to(DEV)
    raw = b.cpu().view(torch.int16).numpy().view(np.uint32)
    assert digest.buf_digest(b, 7) == ref_digest(raw, 7)
    assert digest.buf_digest(b[256:1280], 128) == ref_digest(raw[128:640], 128)       # a slice: two bf16 elements are one word
    z = torch.zeros(TILE, device=DEV)
    assert digest.buf_digest(z) == ref_digest(np.zeros(TILE, np.uint32)) != 0
    one_bit = f.clone()
    one_bit.view(torch.int32)[TILE + 3] ^= 1 << 22
    assert digest.buf_digest(one_bit, 5) != digest.buf_digest(f, 5)


@pytest.mark.timeout(120)
def test_bad_arguments_return_an_error_and_launch_nothing(words):
    _, dev = words
    assert _kernel(dev, 6, 0, start=77) == (-4, 77)               # n_words % 4 != 0: out untouched
    assert _kernel(dev[1:], 4, 0, start=77) == (-4, 77)           # buf not 16-byte aligned
    assert _kernel(dev, -4, 0, start=77) == (-1, 77)
    assert _kernel(dev, 4, -1, start=77) == (-1, 77)
    lib = _lib.lib()
    ws = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert lib.rwkv7_buf_digest_u32(4, 0, P(dev), P(ws), None, 0, None) == -1
    assert lib.rwkv7_buf_digest_u32(4, 0, None, P(ws), P(ws), 0, None) == -1
    assert lib.rwkv7_buf_digest_u32(4, 0, P(dev), None, P(ws), 0, None) == -1
    with pytest.raises(ValueError):
        digest.buf_digest(dev[:6])


# ---- the resume guarantee on the HIP AdamW path -----------------------------------------------------------------------------------
KW = dict(lr=1e-3, warmup_steps=0, total_steps=10)
K = M = 2


def _model(seed):
    """The configuration of test_trainer_gpu.py::_model, with dropout.p left at its 0.02."""
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
    cfg = RWKV7SpeechConfig(vocab_size=257, text_vocab_size=300, audio_global_vocab_size=64, hidden_size=128, num_hidden_layers=2,
                            decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=32)
    m = RWKV7ForSpeech(cfg).init_weights(seed=seed).to(DEV).to(torch.bfloat16).train()
    assert m.dropout.p == 0.02
    return m


def _advance(tr, steps):
    from rwkvtts_amd.layouts import synthetic_spark_batch
    for step in steps:
        tr.step(**synthetic_spark_batch(tr.model, 2, 256, seed=100 * step, n_text=31, n_global=8))


def _state(tr):
    torch.cuda.synchronize()
    return dict(param=tr.flat.flat_param.clone(), master=tr.master.clone(), exp_avg=tr.exp_avg.clone(),
                exp_avg_sq=tr.exp_avg_sq.clone(), step_idx=tr.step_idx, last_lr=tr.last_lr)


@pytest.fixture(scope="module")
def observed_norm():
    """The gradient norm of the first step (measure-only clipping), computed once."""
    from rwkvtts_amd import trainer
    torch.manual_seed(11)
    t = trainer.DataParallelTrainer(_model(3), max_grad_norm=float("inf"), **KW)
    torch.manual_seed(11)
    _advance(t, [0])
    return t.last_grad_norm.item()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", ["plain", "clip", "allreduce"])
def test_resume_on_the_hip_path_is_bit_identical(mode, tmp_path, observed_norm):
    from rwkvtts_amd import trainer
    kw = dict(KW)
    if mode == "clip":
        kw["max_grad_norm"] = 0.25 * observed_norm      # well below every norm of the run: the clip is active throughout
    if mode == "allreduce":                       # one-rank RCCL group with the collectives forced on, as test_trainer_gpu.py does
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
        kw.update(bucket_bytes=64 << 10, force_allreduce=True)
    try:
        ta = trainer.DataParallelTrainer(_model(3), **kw)
        assert ta.hip_adamw and ta.reducer.enabled == (mode == "allreduce")
        torch.manual_seed(11)
        _advance(ta, range(K + M))
        a = _state(ta)
        if mode == "clip":
            assert ta.last_grad_norm.item() > kw["max_grad_norm"], "the case must clip"
        tb = trainer.DataParallelTrainer(_model(3), **kw)
        torch.manual_seed(11)
        _advance(tb, range(K))
        tb.save_checkpoint(str(tmp_path), extra={"cursor": K})
        at_save = tb.digest()
        del tb
        torch.manual_seed(999)                    # the new process: other initial weights, another generator state
        mc = _model(5)
        tc = trainer.DataParallelTrainer(mc, **kw)
        assert not torch.equal(tc.master, a["master"])
        assert tc.load_checkpoint(str(tmp_path)) == {"cursor": K}
        stored = json.loads((tmp_path / f"step_{K}" / "meta.json").read_text())["digest"]
        loaded = tc.digest()                      # the kernel, on what is in device memory now
        assert {k: "%016x" % v for k, v in loaded.items()} == stored and loaded == at_save
        assert loaded["master"] == digest.fallback_digest(tc.master) and loaded["param"] == digest.fallback_digest(tc.flat.flat_param)
        assert loaded["master"] != loaded["param"]
        _advance(tc, range(K, K + M))
        c = _state(tc)
        for k in ("param", "master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a[k], c[k]), k
        assert (a["step_idx"], a["last_lr"]) == (c["step_idx"], c["last_lr"]) == (K + M, tc.last_lr)
        assert ta.digest() == tc.digest()
        lo = tc.flat.flat_param.data_ptr()
        hi = lo + tc.flat.flat_param.numel() * 2
        assert all(lo <= p.data_ptr() < hi for p in mc.parameters()), "the parameters must stay views of flat_param"
        assert all(torch.equal(p.reshape(-1), tc.flat.flat_param[o:o + p.numel()]) for p, o in zip(tc.flat.params, tc.flat.offsets))
    finally:
        if mode == "allreduce":
            dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_without_the_device_rng_the_runs_differ(tmp_path):
    """The premise of the test above: with Dropout(0.02) on, two steps from the same weights under different device generator states
    end in different parameters -- so equality after a resume shows that the generator state was restored."""
    from rwkvtts_amd import trainer
    outs = []
    for seed in (11, 999):
        t = trainer.DataParallelTrainer(_model(3), **KW)
        torch.manual_seed(seed)
        _advance(t, [0])
        outs.append(_state(t)["master"])
    assert not torch.equal(outs[0], outs[1])
