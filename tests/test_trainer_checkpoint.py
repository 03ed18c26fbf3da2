"""CPU: DataParallelTrainer.save_checkpoint / load_checkpoint / digest on the toy fp32 network of test_trainer_dist.py (the torch
fallback of the trainer and the numpy fallback of the digest; the protocol -- who writes what, the rename, `latest`, the layout and
digest checks -- is the same code as on the GPU).

The resume guarantee: k steps, save, a FRESH model with other initial values and a fresh trainer, load, m more steps leave
flat_param, master, exp_avg, exp_avg_sq, step_idx and last_lr bit-identical to k + m uninterrupted steps (k = m = 2)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from rwkvtts_amd import digest, trainer
from test_trainer_dist import Toy, _data, _free_port

LR = dict(lr=1e-2, warmup_steps=0, total_steps=100)
K = M = 2


def ref_digest(words, first=0):
    """The digest restated on its own (include/rwkv7_hip.h): numpy uint64 arithmetic wraps mod 2^64."""
    w = np.asarray(words, dtype=np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = w + (np.uint64(first) + np.arange(1, w.size + 1, dtype=np.uint64)) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
        return int(np.add.reduce(x, dtype=np.uint64)) if w.size else 0


def _other_init(model, seed=7):
    """The 'new process': a model whose parameters are NOT those of Toy()'s fixed seed."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn(p.shape, generator=g))
    return model


def _state(tr):
    return dict(param=tr.flat.flat_param.clone(), master=tr.master.clone(), exp_avg=tr.exp_avg.clone(),
                exp_avg_sq=tr.exp_avg_sq.clone(), step_idx=tr.step_idx, last_lr=tr.last_lr)


def _assert_same_state(a, b):
    for k in ("param", "master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(a[k], b[k]), k
    assert a["step_idx"] == b["step_idx"] and a["last_lr"] == b["last_lr"]


def _advance(tr, rank, steps, accumulate=False):
    for step in steps:
        x, y = _data(rank, step)
        if accumulate:
            a, b = _data(rank, 50 + step)
            tr.accumulate(x=a, y=b)
        tr.step(x=x, y=y)


def _observed_norm():
    m = Toy()
    x, y = _data(0, 0)
    m(x, y).loss.backward()
    return torch.sqrt(sum(p.grad.double().pow(2).sum() for p in m.parameters() if p.grad is not None)).item()


@pytest.mark.parametrize("mode", ["plain", "clip", "reference-groups", "accumulate-after-resume"])
def test_resume_is_bit_identical_to_the_uninterrupted_run(mode, tmp_path):
    kw = dict(LR)
    if mode == "clip":
        kw["max_grad_norm"] = 0.5 * _observed_norm()          # below the observed norm: the clip is active
    if mode == "reference-groups":
        kw.update(param_groups="reference", weight_decay=0.1)
    acc = mode == "accumulate-after-resume"
    ta = trainer.DataParallelTrainer(Toy(), **kw)
    _advance(ta, 0, range(K))
    _advance(ta, 0, range(K, K + M), accumulate=acc)
    if mode == "clip":
        assert ta.last_grad_norm.item() > kw["max_grad_norm"], "the case must clip"
    if mode == "reference-groups":
        assert len(ta.group_defs) == 3
    tb = trainer.DataParallelTrainer(Toy(), **kw)
    _advance(tb, 0, range(K))
    extra = {"epoch": 3, "batch_index": 17, "cursor": [1, 2, {"shard": "a"}]}
    path = tb.save_checkpoint(str(tmp_path), extra=extra)
    assert path == str(tmp_path / f"step_{K}") and (tmp_path / "latest").read_text() == f"step_{K}"
    del tb
    mc = _other_init(Toy())
    tc = trainer.DataParallelTrainer(mc, **kw)
    assert not torch.equal(tc.master, ta.master)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                          # same world, same groups: nothing to warn about
        assert tc.load_checkpoint(str(tmp_path)) == extra
    assert tc.step_idx == K
    _advance(tc, 0, range(K, K + M), accumulate=acc)
    _assert_same_state(_state(ta), _state(tc))
    da, dc = ta.digest(), tc.digest()
    assert da == dc and set(da) == {"master", "exp_avg", "exp_avg_sq", "param"} and da["master"] == da["param"]   # fp32: one buffer
    assert da["master"] != da["exp_avg"] and all(0 <= v < 2 ** 64 for v in da.values())
    lo, hi = tc.flat.flat_param.data_ptr(), tc.flat.flat_param.data_ptr() + tc.flat.flat_param.numel() * 4
    assert all(lo <= p.data_ptr() < hi for p in mc.parameters()), "the parameters must stay views of flat_param"
    assert all(torch.equal(p.reshape(-1), tc.flat.flat_param[o:o + p.numel()]) for p, o in zip(tc.flat.params, tc.flat.offsets))


def test_save_inside_an_accumulation_window_raises_and_writes_nothing(tmp_path):
    tr = trainer.DataParallelTrainer(Toy(), **LR)
    x, y = _data(0, 0)
    tr.accumulate(x=x, y=y)
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.save_checkpoint(str(tmp_path / "ck"))
    assert not (tmp_path / "ck").exists()
    tr.step(x=x, y=y)
    tr.save_checkpoint(str(tmp_path / "ck"))                    # at the step boundary it works
    assert (tmp_path / "ck" / "step_1" / "meta.json").exists()


def test_unserialisable_extra_writes_nothing(tmp_path):
    tr = trainer.DataParallelTrainer(Toy(), **LR)
    with pytest.raises(TypeError):
        tr.save_checkpoint(str(tmp_path / "ck"), extra={"t": torch.zeros(1)})
    assert not (tmp_path / "ck").exists()


class WideToy(Toy):
    def __init__(self):
        super().__init__()
        self.b = torch.nn.Linear(64, 96)     # one layer widened (never run: only its layout matters)


@pytest.fixture
def saved(tmp_path):
    """A trainer two steps in, and its checkpoint."""
    tr = trainer.DataParallelTrainer(Toy(), **LR)
    _advance(tr, 0, range(K))
    tr.save_checkpoint(str(tmp_path))
    return tr, tmp_path


def test_layout_mismatch_is_a_value_error_and_touches_nothing(saved):
    _, d = saved
    tw = trainer.DataParallelTrainer(_other_init(WideToy()), **LR)
    before = _state(tw)
    with pytest.raises(ValueError, match="b.weight"):
        tw.load_checkpoint(str(d))
    _assert_same_state(before, _state(tw))
    assert tw.step_idx == 0


@pytest.mark.parametrize("buf", ["master", "exp_avg_sq"])
def test_one_flipped_byte_fails_the_digest_check(saved, buf):
    tr, d = saved
    f = d / f"step_{K}" / f"range_{0:012d}_{tr.flat.numel:012d}.{buf}.bin"
    raw = bytearray(f.read_bytes())
    raw[len(raw) // 3] ^= 0x10
    f.write_bytes(bytes(raw))
    t2 = trainer.DataParallelTrainer(Toy(), **LR)
    with pytest.raises(RuntimeError, match=f"digest mismatch in `{buf}`"):
        t2.load_checkpoint(str(d))


def test_truncated_file_is_a_runtime_error_naming_the_buffer(saved):
    tr, d = saved
    f = d / f"step_{K}" / f"range_{0:012d}_{tr.flat.numel:012d}.exp_avg.bin"
    f.write_bytes(f.read_bytes()[:-4])
    t2 = trainer.DataParallelTrainer(Toy(), **LR)
    before = _state(t2)
    with pytest.raises(RuntimeError, match="exp_avg"):
        t2.load_checkpoint(str(d))
    _assert_same_state(before, _state(t2))


def test_leftover_tmp_directory_is_never_loaded_and_is_removed_by_the_next_save(saved):
    tr, d = saved
    stale = d / "step_9.tmp"
    stale.mkdir()
    (stale / "meta.json").write_text((d / f"step_{K}" / "meta.json").read_text())
    t2 = trainer.DataParallelTrainer(_other_init(Toy()), **LR)
    t2.load_checkpoint(str(d))                                   # tag=None: `latest`, not the newest directory
    assert t2.step_idx == K and torch.equal(t2.master, tr.master)
    with pytest.raises(FileNotFoundError):
        t2.load_checkpoint(str(d), tag="step_9.tmp")
    assert trainer.complete_checkpoints(str(d)) == [(K, f"step_{K}")]
    _advance(tr, 0, [K])
    tr.save_checkpoint(str(d))
    assert not stale.exists()


def test_keep_last_two_over_four_saves(tmp_path):
    tr = trainer.DataParallelTrainer(Toy(), **LR)
    for step in range(4):
        _advance(tr, 0, [step])
        tr.save_checkpoint(str(tmp_path), keep_last=2)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["latest", "step_3", "step_4"]
    assert (tmp_path / "latest").read_text() == "step_4"
    t2 = trainer.DataParallelTrainer(_other_init(Toy()), **LR)
    t2.load_checkpoint(str(tmp_path), tag="step_3")
    assert t2.step_idx == 3
    t2.load_checkpoint(str(tmp_path))
    assert t2.step_idx == 4 and torch.equal(t2.master, tr.master)


def test_changed_parameter_groups_warn_and_the_new_ones_hold(saved):
    _, d = saved
    t2 = trainer.DataParallelTrainer(Toy(), param_groups="reference", weight_decay=0.1, **LR)
    with pytest.warns(UserWarning, match="parameter groups"):
        t2.load_checkpoint(str(d))
    assert len(t2.group_defs) == 3


def test_meta_holds_what_the_format_promises(saved):
    tr, d = saved
    meta = json.loads((d / f"step_{K}" / "meta.json").read_text())
    assert meta["format"] == trainer.CHECKPOINT_FORMAT and meta["world"] == 1 and meta["shard_optimizer"] is False
    assert meta["step_idx"] == K and meta["last_lr"] == tr.last_lr and meta["ranges"] == [[0, tr.flat.numel]]
    names = [n for n, p in tr.model.named_parameters() if p.requires_grad]
    assert [e["name"] for e in meta["layout"]] == names and [e["offset"] for e in meta["layout"]] == tr.flat.offsets
    assert meta["digest"] == {k: "%016x" % v for k, v in tr.digest().items()}
    assert meta["hyper"]["lr"] == 1e-2 and meta["hyper"]["schedule"] == "linear" and meta["group_defs"] == [["all", 1.0, 0.0]]
    assert (d / f"step_{K}" / "rng_rank0.pt").exists()


def test_host_rng_state_is_restored(saved):
    tr, d = saved
    torch.manual_seed(99)
    tr.save_checkpoint(str(d), tag="rng")
    want = torch.rand(4)
    t2 = trainer.DataParallelTrainer(Toy(), **LR)                # Toy() reseeds the generator
    t2.load_checkpoint(str(d), tag="rng")
    assert torch.equal(torch.rand(4), want)


# ---- the digest fallback against the restatement above ---------------------------------------------------------------------------
def _words(n, seed=0):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)


def test_digest_fallback_equals_the_restatement():
    for n, first in ((0, 0), (1, 0), (4, 12), (1000, 0), (4099, 2 ** 32 + 8), (3 * digest._CHUNK // 2, 5)):
        w = _words(n, seed=n)
        assert digest.digest_words(w, first) == ref_digest(w, first), (n, first)
    w = _words(12)
    # by hand, in Python integers, for one word
    x = (int(w[0]) + 1 * 0x9E3779B97F4A7C15) & digest.MASK64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & digest.MASK64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & digest.MASK64
    x ^= x >> 31
    assert digest.digest_words(w[:1]) == x


def test_digest_properties():
    w = _words(3000, seed=1)
    first = 2 ** 32 + 8                                          # global indices beyond 2^32
    whole = digest.digest_words(w, first)
    parts = [digest.digest_words(w[a:b], first + a) for a, b in ((0, 7), (7, 1900), (1900, 3000))]   # three unequal slabs
    assert sum(parts) % 2 ** 64 == whole
    assert digest.digest_words(w, 0) != whole                    # position-sensitive as a whole
    flipped = w.copy()
    flipped[1234] ^= np.uint32(1 << 17)
    assert digest.digest_words(flipped, first) != whole          # one bit
    assert w[10] != w[2000]
    swapped = w.copy()
    swapped[[10, 2000]] = swapped[[2000, 10]]
    assert digest.digest_words(swapped, first) != whole          # a plain sum of the words would not see this
    assert digest.digest_words(np.zeros(64, np.uint32)) != 0
    assert digest.digest_words(np.zeros(64, np.uint32)) != digest.digest_words(np.zeros(68, np.uint32))


def test_digest_of_tensors_is_the_digest_of_their_raw_words():
    g = torch.Generator().manual_seed(0)
    f = torch.randn(257, generator=g)
    assert digest.buf_digest(f, 3) == ref_digest(f.numpy().view(np.uint32), 3)
    b = torch.randn(512, generator=g).bfloat16()
    assert digest.buf_digest(b, 64) == ref_digest(b.view(torch.int16).numpy().view(np.uint32), 64)
    with pytest.raises(ValueError):
        digest.buf_digest(b[:3])                                 # not a whole number of words


# ---- two gloo ranks --------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, q, shard, d):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    trainer.init_distributed("gloo")
    torch.set_num_threads(1)
    kw = dict(bucket_bytes=4096, shard_optimizer=shard, **LR)
    ta = trainer.DataParallelTrainer(Toy(), **kw)
    _advance(ta, rank, range(K + M))
    tb = trainer.DataParallelTrainer(Toy(), **kw)
    _advance(tb, rank, range(K))
    at_save = _state(tb)
    whole_at_save = tb.digest(all_ranks=True)
    tb.save_checkpoint(d, extra={"cursor": 5})
    tc = trainer.DataParallelTrainer(_other_init(Toy(), seed=7 + rank), **kw)
    extra = tc.load_checkpoint(d)
    _advance(tc, rank, range(K, K + M))
    lo, hi = ta._own_range()
    same = all(torch.equal(getattr(ta, n)[lo:hi], getattr(tc, n)[lo:hi]) for n in ("master", "exp_avg", "exp_avg_sq")) \
        and torch.equal(ta.flat.flat_param, tc.flat.flat_param) and (ta.step_idx, ta.last_lr) == (tc.step_idx, tc.last_lr)
    diverged = None
    if not shard:                                                # the replica check: one rank's master is off by one bit
        if rank == 1:
            tc.master.view(torch.int32)[5] ^= 1
        try:
            tc.digest(all_ranks=True)
        except RuntimeError as e:
            diverged = str(e)
    q.put((rank, same, extra, (lo, hi), {k: v[lo:hi].numpy().copy() for k, v in at_save.items() if torch.is_tensor(v)},
           whole_at_save, ta.digest(all_ranks=True), tc.digest() if shard else None, diverged))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("shard", [False, True], ids=["allreduce", "shard"])
def test_two_ranks_resume_and_load_into_one(shard, tmp_path):
    world, d = 2, str(tmp_path)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, shard, d)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert all(r[1] for r in res), "the resumed 2-rank run differs from the uninterrupted one"
    assert all(r[2] == {"cursor": 5} for r in res)
    ck = tmp_path / f"step_{K}"
    range_files = sorted(p.name for p in ck.iterdir() if p.name.startswith("range_") and p.name.endswith(".json"))
    assert len(range_files) == (2 if shard else 1)
    assert sorted(p.name for p in ck.iterdir() if p.name.startswith("rng_")) == ["rng_rank0.pt", "rng_rank1.pt"]
    assert res[0][5] == res[1][5] and res[0][6] == res[1][6], "digest(all_ranks=True) must be the same word on every rank"
    if shard:
        assert res[0][3][1] == res[1][3][0] and res[0][3][0] == 0, "the slabs tile the buffer"
        assert res[0][7] != res[1][7], "each rank digests its own slab"
        assert {k: (res[0][7][k] + res[1][7][k]) % 2 ** 64 for k in res[0][7]} == res[0][6]          # additivity across ranks
    else:
        assert all(r[8] is not None and "`master`" in r[8] for r in res), "a one-bit divergence must raise on every rank"
    # the same checkpoint into ONE process: buffers equal the gathered 2-rank state at save time
    t1 = trainer.DataParallelTrainer(_other_init(Toy()), **LR)
    with pytest.warns(UserWarning, match="RNG"):
        assert t1.load_checkpoint(d) == {"cursor": 5}
    for name, buf in (("master", t1.master), ("exp_avg", t1.exp_avg), ("exp_avg_sq", t1.exp_avg_sq), ("param", t1.flat.flat_param)):
        pieces = [torch.from_numpy(r[4][name]) for r in res] if shard else [torch.from_numpy(res[0][4][name])]
        assert torch.equal(buf, torch.cat(pieces)), name
    assert {k: "%016x" % v for k, v in t1.digest().items()} == json.loads((ck / "meta.json").read_text())["digest"]
    assert t1.digest() == res[0][5]


@pytest.mark.timeout(300)
def test_one_rank_checkpoint_loads_into_two_sharded_ranks(tmp_path):
    tr = trainer.DataParallelTrainer(Toy(), **LR)
    _advance(tr, 0, range(K))
    tr.save_checkpoint(str(tmp_path))
    want = tr.digest()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_load_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert all(r == want for r in res)


def _load_worker(rank, world, port, q, d):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    trainer.init_distributed("gloo")
    torch.set_num_threads(1)
    tr = trainer.DataParallelTrainer(_other_init(Toy(), seed=rank), bucket_bytes=4096, shard_optimizer=True, **LR)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr.load_checkpoint(d)
    q.put(tr.digest(all_ranks=True))
    dist.barrier()
    dist.destroy_process_group()
