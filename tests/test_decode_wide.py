"""CPU: the parts of the wide decode step (B = 33 .. 128, csrc/decode_step_wide.hip) that need no device -- both entries are
declared and exported, bad arguments are answered before anything is launched, the workspace grows by row tile and not by row, and
the three continuous-batching engines accept exactly the slot counts the two step kernels cover."""
import ctypes

import pytest

from rwkvtts_amd import _lib
from rwkvtts_amd.decode import _Dims, check_slots

EINVAL, EHEAD, ESHAPE = -1, -3, -4


def _dims(B=64, D=128, H=None, L=2, F=None, V=77, ranks=(32, 32, 32, 32)):
    return _Dims(B, D, D // 64 if H is None else H, L, 4 * D if F is None else F, V, *ranks, 1e-5, 64e-5)


def _bytes(lib, dm):
    return lib.rwkv7_decode_wide_workspace_bytes(ctypes.byref(dm))


def test_wide_entries_are_declared_and_exported(hip_lib):
    for n in ("rwkv7_decode_wide_workspace_bytes", "rwkv7_decode_step_wide_bf16"):
        assert n in _lib.exported_symbols(), n      # declared in include/rwkv7_hip.h
        assert hasattr(hip_lib, n), n               # exported by the library


def test_wide_step_argument_errors_do_not_launch(hip_lib):
    one = ctypes.c_void_p(16)   # never dereferenced: the checks fire first
    f = hip_lib.rwkv7_decode_step_wide_bf16

    def call(dm, tbl=one, tbl_host=None, x=one, logits=one, ws=one):
        return f(ctypes.byref(dm) if dm is not None else None, tbl, tbl_host, x, one, one, one, None, logits, ws, None)

    assert call(_dims(B=32)) == ESHAPE                       # the 32-row entry's range
    assert call(_dims(B=129)) == ESHAPE
    assert call(_dims(B=0)) == ESHAPE
    assert call(_dims(D=96, H=1)) == EHEAD                   # D % 64 != 0 cannot be H heads of 64
    assert call(_dims(D=96, H=1, B=32)) == EHEAD
    assert call(_dims(ranks=(32, 32, 16, 32))) == ESHAPE     # rank 16
    assert call(_dims(ranks=(288, 32, 32, 32))) == ESHAPE
    assert call(_dims(F=4 * 128 + 32)) == ESHAPE
    assert call(_dims(L=0)) == ESHAPE
    assert call(_dims(), tbl=None) == EINVAL                 # NULL table
    assert call(_dims(), tbl=None, tbl_host=one) == EINVAL   # a host table does not replace the device table
    assert call(None) == EINVAL
    assert call(_dims(), x=None) == EINVAL
    assert call(_dims(), logits=None) == EINVAL
    assert call(_dims(), ws=None) == EINVAL
    # the 32-row entries keep their range
    g = hip_lib.rwkv7_decode_step_tbl_bf16
    assert g(ctypes.byref(_dims(B=33)), one, one, one, one, one, one, None, one, one, 0, None) == ESHAPE
    assert hip_lib.rwkv7_decode_step_bf16(ctypes.byref(_dims(B=33)), one, one, one, one, one, None, one, one, 0, None) == ESHAPE


@pytest.mark.parametrize("D,ranks,V", [(128, (32, 32, 32, 32), 77), (1024, (64, 64, 32, 128), 8193), (2048, (96, 96, 64, 256), 1025)])
def test_wide_workspace_grows_by_row_tile(hip_lib, D, ranks, V):
    size = {B: _bytes(hip_lib, _dims(B=B, D=D, V=V, ranks=ranks)) for B in (33, 40, 64, 65, 96, 97, 127, 128)}
    assert all(v > 0 for v in size.values()), size
    assert size[33] == size[40] == size[64]
    assert size[65] == size[96]
    assert size[97] == size[127] == size[128]
    assert size[64] < size[96] < size[128]
    narrow = hip_lib.rwkv7_decode_workspace_bytes(ctypes.byref(_dims(B=32, D=D, V=V, ranks=ranks)))
    assert 0 < narrow < size[64]
    # every plane doubles from one tile to two; only the 256-byte barrier block does not
    assert size[64] - 256 == 2 * (narrow - 256)


def test_wide_workspace_is_zero_outside_its_range(hip_lib):
    for dm in (_dims(B=1), _dims(B=32), _dims(B=129), _dims(B=0), _dims(D=96, H=1), _dims(ranks=(32, 32, 16, 32)), _dims(F=100)):
        assert _bytes(hip_lib, dm) == 0
    assert hip_lib.rwkv7_decode_wide_workspace_bytes(None) == 0
    assert hip_lib.rwkv7_decode_workspace_bytes(ctypes.byref(_dims(B=33))) == 0


GOOD = list(range(1, 33)) + [64, 96, 128]
BAD = [0, -1, 33, 48, 63, 65, 95, 100, 127, 129, 160, 256]


def test_check_slots():
    for s in GOOD:
        assert check_slots(s) == s
    for s in BAD:
        with pytest.raises(ValueError, match=f"slots = {s}:"):
            check_slots(s)


def _engines():
    from rwkvtts_amd.continuous import ContinuousDecoder
    from rwkvtts_amd.continuous_cosy import ContinuousCosyDecoder
    from rwkvtts_amd.continuous_xy import ContinuousXYDecoder
    return ContinuousDecoder, ContinuousXYDecoder, ContinuousCosyDecoder


class _NoModel:
    """Stands where the model goes: a constructor that passes the slot check touches it and fails with THIS error, not ValueError."""

    class Touched(Exception):
        pass

    def __getattr__(self, name):
        raise _NoModel.Touched(name)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_engines_validate_slots_before_the_device(which):
    eng = _engines()[which]
    for s in BAD:
        with pytest.raises(ValueError, match=f"slots = {s}:"):   # the slot check's own message
            eng(_NoModel(), slots=s)
    for s in (1, 32, 64, 96, 128):
        with pytest.raises(_NoModel.Touched):                    # past the slot check: the next thing is the model
            eng(_NoModel(), slots=s)
