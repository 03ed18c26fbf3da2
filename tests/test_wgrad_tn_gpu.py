"""GPU (-m gpu): rwkv7_wgrad_tn_bf16 (csrc/wgrad_tn.hip) through fused.wgrad_splitk -- the dense projections' weight gradient
dW[N][K] = sum_t dy[t][N] x[t][K] (autograd of nn.Linear, rwkv_s2s_single_ffn.py:171-174, 195, 228-229) with both operands read
token-major, fp32 partials per row slab and rwkv7_sum_slabs_bf16 behind it.

Shapes are the smallest at which tile, slab and transpose indexing can go wrong: one 256 x 256 tile, two tiles along either axis, a
4 x 4 grid and two rectangles, at M = 4096 rows (the dispatch's minimum).  Bars of the random-data tests are those of
test_fused_gpu.py::test_weight_gradient_of_the_lerp_matrices: max error <= 2^-8 max|ref| (half a bf16 ulp of the largest element),
relative L2 <= 3e-3 against the fp32 product and against the library route."""
import ctypes

import pytest
import torch

from fused_parity import DEV
from rwkvtts_amd import _lib, fused

pytestmark = pytest.mark.gpu

M0 = 4096
SQUARE = [(256, 256), (512, 256), (256, 512), (1024, 1024)]
RECT = [(1024, 256), (256, 1024)]
SMALL_CLASSES = {nk: 4 for nk in SQUARE + RECT}
# every slab count the dispatch can choose: the shipped table's and the ones this file enables the small classes with
SLABS = sorted(set(fused.TN_WGRAD_CLASSES.values()) | set(SMALL_CLASSES.values()) | {16})

_cache = {}


def _classes(monkeypatch, extra=None):
    monkeypatch.setattr(fused, "TN_WGRAD", True)
    monkeypatch.setattr(fused, "TN_WGRAD_CLASSES", {**fused.TN_WGRAD_CLASSES, **SMALL_CLASSES, **(extra or {})})


def _integers(N, K):
    """dy, x with integers in [-4, 4] that differ by row and by column, no symmetry between N and K; fp64 product rounded once."""
    key = ("int", N, K)
    if key not in _cache:
        t = torch.arange(M0, device=DEV).view(-1, 1)
        n = torch.arange(N, device=DEV).view(1, -1)
        k = torch.arange(K, device=DEV).view(1, -1)
        dy = (t * 7 + n * 3 + (t * n) % 5 + (t // 256) * (n // 32)) % 9 - 4
        x = (t * 5 + k * 11 + (t // 3) * (k % 7) + (t // 128) * (k // 64)) % 9 - 4
        ref = (dy.double().t() @ x.double())
        assert ref.abs().max().item() < 2 ** 24
        _cache[key] = (dy.to(torch.bfloat16), x.to(torch.bfloat16), ref.to(torch.bfloat16))
    return _cache[key]


def _random(M, N, K):
    key = ("rnd", M, N, K)
    if key not in _cache:
        g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
        dy = torch.randn(M, N, generator=g).to(DEV, torch.bfloat16)
        x = torch.randn(M, K, generator=g).to(DEV, torch.bfloat16)
        _cache[key] = (dy, x, dy.float().t() @ x.float())
    return _cache[key]


def _bars(got, ref, what):
    got, ref = got.float(), ref.float()
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    l2 = (got - ref).norm().item() / ref.norm().item()
    print(f"{what}: max error {err:.4g} (bar {2 ** -8 * scale:.4g}), relative L2 {l2:.3g} (bar 3e-3)")
    assert err <= 2 ** -8 * scale, what
    assert l2 <= 3e-3, what


@pytest.mark.parametrize("S", [None] + SLABS)
@pytest.mark.parametrize("N,K", SQUARE)
def test_small_integers_are_exact(N, K, S, monkeypatch):
    """Every fp32 partial and sum is exact (|sum| <= 16 * 4096 < 2^24): bit-equal to the fp64 product rounded once to bf16."""
    _classes(monkeypatch)
    dy, x, ref = _integers(N, K)
    hits = fused.TN_WGRAD_HITS[0]
    got = fused.wgrad_splitk(dy, x, slabs=S)
    assert fused.TN_WGRAD_HITS[0] - hits == 1
    bad = (got != ref).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), got[tuple(bad[0])].item(), ref[tuple(bad[0])].item())


@pytest.mark.parametrize("N,K", SQUARE + RECT)
def test_random_data_against_the_fp32_product_and_the_library_route(N, K, monkeypatch):
    _classes(monkeypatch)
    dy, x, ref = _random(M0, N, K)
    hits = fused.TN_WGRAD_HITS[0]
    own = fused.wgrad_splitk(dy, x)
    again = fused.wgrad_splitk(dy, x)
    assert fused.TN_WGRAD_HITS[0] - hits == 2
    monkeypatch.setattr(fused, "TN_WGRAD", False)
    lib = fused.wgrad_splitk(dy, x)
    assert fused.TN_WGRAD_HITS[0] - hits == 2, "the counter moved with the switch off"
    _bars(own, ref, f"own [{N}][{K}] against fp32")
    l2 = (own.float() - lib.float()).norm().item() / lib.float().norm().item()
    print(f"own against library: relative L2 {l2:.3g} (bar 3e-3)")
    assert l2 <= 3e-3
    assert torch.equal(own, again), "two calls on the same inputs differ"


def test_result_lands_in_a_slice_of_the_gradient_buffer(monkeypatch):
    _classes(monkeypatch)
    N, K = 512, 256
    dy, x, ref = _random(M0, N, K)
    flat = torch.full((3 * N * K + 24,), 7.5, dtype=torch.bfloat16, device=DEV)
    lo = N * K + 8
    res = fused.wgrad_splitk(dy, x, out=flat[lo:lo + N * K].view(N, K))
    assert res.data_ptr() == flat[lo:].data_ptr()
    _bars(flat[lo:lo + N * K].view(N, K), ref, "gradient slot")
    assert (flat[:lo] == 7.5).all() and (flat[lo + N * K:] == 7.5).all()


def test_entry_rejects_what_the_kernel_does_not_take():
    L = _lib.lib()
    a = torch.zeros(8, device=DEV)
    p = ctypes.c_void_p(a.data_ptr())
    assert L.rwkv7_wgrad_tn_bf16(4096, 256, 256, 4, None, p, p, None) == -1     # null pointer
    assert L.rwkv7_wgrad_tn_bf16(4160, 256, 256, 4, p, p, p, None) == -4        # rows per slab not a multiple of the row step
    assert L.rwkv7_wgrad_tn_bf16(4096, 256, 256, 3, p, p, p, None) == -4        # slabs do not divide the rows
    assert L.rwkv7_wgrad_tn_bf16(4096, 320, 256, 4, p, p, p, None) == -4        # N not a multiple of the tile edge
    assert L.rwkv7_wgrad_tn_bf16(4096, 256, 384, 4, p, p, p, None) == -4        # K not a multiple of the tile edge
    torch.cuda.synchronize()
    assert (a == 0).all()


@pytest.mark.parametrize("M,N,K", [(M0 + 64, 256, 256), (M0, 320, 256), (M0, 256, 384)])
def test_rejected_shapes_take_the_library_route(M, N, K, monkeypatch):
    _classes(monkeypatch, {(N, K): 4})
    dy, x, ref = _random(M, N, K)
    hits = fused.TN_WGRAD_HITS[0]
    got = fused.wgrad_splitk(dy, x)
    assert fused.TN_WGRAD_HITS[0] == hits
    _bars(got, ref, f"library route M = {M} [{N}][{K}]")
    monkeypatch.setattr(fused, "TN_WGRAD", False)
    assert torch.equal(got, fused.wgrad_splitk(dy, x))


def test_only_listed_classes_take_the_kernel(monkeypatch):
    monkeypatch.setattr(fused, "TN_WGRAD", True)
    monkeypatch.setattr(fused, "TN_WGRAD_CLASSES", {(512, 256): 4})
    hits = fused.TN_WGRAD_HITS[0]
    for N, K, want in [(512, 256, 1), (256, 512, 0), (256, 256, 0)]:
        dy, x, _ = _random(M0, N, K)
        fused.wgrad_splitk(dy, x)
        assert fused.TN_WGRAD_HITS[0] - hits == want, (N, K)
        hits = fused.TN_WGRAD_HITS[0]


def test_training_step_of_the_two_layer_model(monkeypatch):
    """One backward of the 2-layer Spark model at width 256 (r / k / v / o 256 x 256, channel mix 1024 x 256 and 256 x 1024 enabled for
    the test), 2 x 2048 tokens, switch on against switch off, the three bars of the random-data test per tensor, each against the
    reference it is defined for there (test_fused_gpu.py:931-933): max error <= 2^-8 max|ref| and relative L2 <= 3e-3 against the fp32
    product of the very operands the backward handed to wgrad_splitk, relative L2 <= 3e-3 against the library route (switch off).
    Every other parameter gradient must meet both bars against the switch-off pass (measured: bit-identical).

    A first version held the switch-on bf16 gradient to the max-error bar against the switch-off bf16 gradient: that bar is half a bf16
    ulp of the largest element and is defined against the unrounded product; two correctly rounded results of fp32 sums taken in
    different orders differ by a whole ulp wherever a sum falls next to a rounding boundary (measured: layers.1.ffn.key.weight, one
    element, 9.537e-07 = 2^-20 against 9.462e-07; relative L2 of the twelve dense gradients 4e-6 ... 6e-5)."""
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
    cfg = RWKV7SpeechConfig(hidden_size=256, num_hidden_layers=2, vocab_size=257, text_vocab_size=300, audio_global_vocab_size=64,
                            decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=32)
    model = RWKV7ForSpeech(cfg).init_weights(seed=0).to(DEV).to(torch.bfloat16).train()
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(2, 2048, 256, generator=g) * 0.5).to(DEV, torch.bfloat16)
    labels = torch.randint(0, 256, (2, 2048), generator=g).to(DEV)
    _classes(monkeypatch)
    inner, seen = fused.wgrad_splitk, []

    def spy(dy2, x2, out=None, slabs=None):   # the dense classes' results beside the fp32 product of their operands
        res = inner(dy2, x2, out=out, slabs=slabs)
        if (dy2.shape[1], x2.shape[1]) in SMALL_CLASSES:
            seen.append((res.detach().clone(), dy2.float().t() @ x2.float()))
        return res

    monkeypatch.setattr(fused, "wgrad_splitk", spy)
    grads, calls = {}, {}
    for on in (False, True):
        monkeypatch.setattr(fused, "TN_WGRAD", on)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(0)   # the training-mode forward draws random numbers: the same ones for both passes
        hits = fused.TN_WGRAD_HITS[0]
        del seen[:]
        model(inputs_embeds=x, labels=labels).loss.backward()
        grads[on] = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        calls[on] = list(seen)
        fired = fused.TN_WGRAD_HITS[0] - hits
        assert fired == (len(seen) if on else 0), (fired, len(seen))
    assert len(calls[True]) == len(calls[False]) >= 2 * 6   # per layer: r, k, v, o, channel-mix key and value
    for i, ((own, ref), (lib, ref_off)) in enumerate(zip(calls[True], calls[False])):
        assert torch.equal(ref, ref_off), f"call {i}: the two passes handed different operands to the weight gradient"
        _bars(own, ref, f"dense weight gradient {i} {tuple(own.shape)} against the fp32 product")
        l2 = (own.float() - lib.float()).norm().item() / lib.float().norm().item()
        print(f"dense weight gradient {i} against the library route: relative L2 {l2:.3g} (bar 3e-3)")
        assert l2 <= 3e-3, i
    assert grads[True].keys() == grads[False].keys() and len(grads[True]) > 20
    dense = {n for n, p in model.named_parameters() if tuple(p.shape) in SMALL_CLASSES}
    assert len(dense) >= 2 * 6
    for n, ref in grads[False].items():
        if n in dense:
            l2 = (grads[True][n].float() - ref.float()).norm().item() / ref.float().norm().item()
            print(f"{n} on against off: relative L2 {l2:.3g} (bar 3e-3)")
            assert l2 <= 3e-3, n
        elif ref.abs().max().item() == 0:
            assert torch.equal(grads[True][n], ref), n
        else:
            _bars(grads[True][n], ref, n)
