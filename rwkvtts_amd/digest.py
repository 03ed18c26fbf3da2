"""Position-sensitive 64-bit digest of a buffer of 32-bit words (include/rwkv7_hip.h, rwkv7_buf_digest_u32):

    x_i  = uint64(w[i]) + (first + i + 1) * 0x9E3779B97F4A7C15
    x_i ^= x_i >> 30;  x_i *= 0xBF58476D1CE4E5B9;  x_i ^= x_i >> 27;  x_i *= 0x94D049BB133111EB;  x_i ^= x_i >> 31
    digest = sum_i x_i                                                      (mod 2^64)

`first` is the GLOBAL index of the buffer's first word, so the digest of a buffer is the wrapping sum of the digests of its
slabs.  Tensors on the HIP device go through the kernel (csrc/buf_digest.hip); host tensors -- the CPU trainers of the gloo
tests -- through the numpy restatement below.  Both are exact: they give the same 64 bits.

snapshot_launch / snapshot_digest copy the words to a second buffer in the same pass (rwkv7_buf_snapshot_digest_u32): what the
trainer's non-blocking checkpoints take of a state buffer before the next step overwrites it.
"""
import numpy as np
import torch

from . import _lib

MASK64 = (1 << 64) - 1
TILE_WORDS = 8192        # words per workgroup of the kernel's first launch (rwkv7_buf_digest_workspace_bytes(n) = 8 * ceil(n / TILE_WORDS))
_CHUNK = 1 << 20         # words per numpy pass of the fallback


def digest_words(words, first=0):
    """The digest of a numpy uint32 array whose first word has global index `first`, as a Python int."""
    words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    total = 0
    with np.errstate(over="ignore"):
        for s in range(0, words.size, _CHUNK):
            w = words[s:s + _CHUNK].astype(np.uint64)
            x = np.arange(first + s + 1, first + s + 1 + w.size, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + w
            x ^= x >> np.uint64(30)
            x *= np.uint64(0xBF58476D1CE4E5B9)
            x ^= x >> np.uint64(27)
            x *= np.uint64(0x94D049BB133111EB)
            x ^= x >> np.uint64(31)
            total = (total + int(x.sum(dtype=np.uint64))) & MASK64
    return total


def _n_words(t):
    nbytes = t.numel() * t.element_size()
    if not t.is_contiguous() or nbytes % 4:
        raise ValueError("digest: the tensor must be contiguous and a whole number of 32-bit words long")
    return nbytes // 4


def fallback_digest(t, first=0):
    """The digest of a tensor's raw words, computed on the host (the tensor is copied there if it lives on a device)."""
    n = _n_words(t)
    if n == 0:
        return 0
    raw = t.detach().reshape(-1).cpu().view(torch.uint8).numpy()
    return digest_words(raw.view("<u4"), first)


def workspace(n_words, device):
    """The partials buffer the kernel needs for up to n_words words."""
    nbytes = _lib.lib().rwkv7_buf_digest_workspace_bytes(max(int(n_words), 1))
    return torch.empty(nbytes // 8, dtype=torch.int64, device=device)


def launch(t, first, out, ws, accumulate=False):
    """Enqueue the kernel: out[0] (int64 device tensor, read as unsigned) = digest of t's raw words.  Nothing is read back."""
    n = _n_words(t)
    _lib.call("rwkv7_buf_digest_u32", out, n, int(first), t if n else None, ws if n else None, out, int(bool(accumulate)))


def buf_digest(t, first=0):
    """The digest of a tensor's raw words as a Python int: the kernel for a tensor on the HIP device (n_words % 4 == 0 and a
    16-byte aligned address, ValueError otherwise), the numpy restatement for a host tensor."""
    if not t.is_cuda:
        return fallback_digest(t, first)
    out = torch.zeros(1, dtype=torch.int64, device=t.device)
    launch(t, first, out, workspace(_n_words(t), t.device))
    return int(out.item()) & MASK64


def snapshot_launch(src, dst, first, out, ws, accumulate=False):
    """Enqueue the snapshot kernel: dst's raw words = src's, out[0] = their digest (as `launch`).  src and dst: device tensors of
    the same dtype and length that do not overlap.  Nothing is read back."""
    n = _n_words(src)
    if dst.dtype != src.dtype or dst.numel() != src.numel() or not dst.is_contiguous():
        raise ValueError("snapshot: dst must be a contiguous tensor of src's dtype and length")
    _lib.call("rwkv7_buf_snapshot_digest_u32", out, n, int(first), src if n else None, dst if n else None, ws if n else None, out,
              int(bool(accumulate)))


def snapshot_digest(src, dst, first=0):
    """dst = src bit for bit, and the digest of the copied words as a Python int: one kernel pass when both live on the HIP device,
    dst.copy_(src) and the numpy restatement over dst otherwise (host tensors)."""
    if not (src.is_cuda and dst.is_cuda):
        if dst.dtype != src.dtype or dst.shape != src.shape:
            raise ValueError("snapshot: dst must have src's dtype and shape")
        dst.copy_(src)
        return fallback_digest(dst, first)
    out = torch.zeros(1, dtype=torch.int64, device=src.device)
    snapshot_launch(src, dst, first, out, workspace(_n_words(src), src.device))
    return int(out.item()) & MASK64
