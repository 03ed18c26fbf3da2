"""CPU: the C ABI of rwkv7_seq_scores_f32 -- declared in include/rwkv7_hip.h, typed from it with no hand-written binding, exported by the
library, and RWKV7_EINVAL for bad arguments before any launch (no GPU is needed for that: the checks fire first)."""
import ctypes

from rwkvtts_amd import _lib

NAME = "rwkv7_seq_scores_f32"


def test_header_declares_the_entry_and_the_library_exports_it(hip_lib):
    assert NAME in _lib.exported_symbols()
    restype, argtypes = _lib.prototypes()[NAME]
    P, L = ctypes.c_void_p, ctypes.c_long
    # n_seq, seq_start, loss_rows, correct_rows, labels, ignore_index, the five outputs, the stream
    assert restype is ctypes.c_int and argtypes == [L, P, P, P, P, L, P, P, P, P, P, P]
    fn = getattr(hip_lib, NAME)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes


def test_entry_point_rejects_bad_arguments_before_any_launch(hip_lib):
    one = 16   # never dereferenced: the checks fire first
    names = ["seq_start", "loss_rows", "correct_rows", "labels", "loss_sum", "tokens", "correct", "worst_loss", "worst_row"]

    def call(n_seq=3, **null):
        p = {n: (None if n in null else one) for n in names}
        return getattr(hip_lib, NAME)(n_seq, p["seq_start"], p["loss_rows"], p["correct_rows"], p["labels"], -100, p["loss_sum"],
                                      p["tokens"], p["correct"], p["worst_loss"], p["worst_row"], None)

    for n in names:
        assert call(**{n: True}) == -1, n
    assert call(n_seq=0) == -1 and call(n_seq=-5) == -1
    assert call(n_seq=2 ** 31) == -1, "one workgroup per sequence: more than the grid's x extent is refused, not truncated"
