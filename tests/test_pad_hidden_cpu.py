"""CPU-side checks of LSTM_HIP_PAD_HIDDEN: the flag makes any hidden size a valid shape, so create gets as far as the
device check (ENODEV on a machine without a gfx950), while the same N without the flag is still refused as a shape."""
import ctypes as C

import pytest

EINVAL, ENODEV = -1, -3


def _has_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


def _create(N, flags, S=7, B=16):
    import lstm_hip
    lib = lstm_hip.load_library()
    h = C.c_void_p()
    rc = lib.lstm_hip_create(C.byref(lstm_hip._Config(N, 256, S, B, 0, flags)), C.byref(h))
    if h.value:
        lib.lstm_hip_destroy(h)
    return rc, lib.lstm_hip_last_error().decode()


def test_flag_value_is_the_next_free_bit():
    import lstm_hip
    assert lstm_hip.PAD_HIDDEN == 256
    assert lstm_hip.PAD_HIDDEN & (2 | 8 | 32 | lstm_hip.FAST_MATH | lstm_hip.STEP_KERNELS | lstm_hip.DEBUG_STAMPS |
                                  lstm_hip.NO_FUSED_GRADS | lstm_hip.BF16_RECURRENCE) == 0


@pytest.mark.skipif(_has_gpu(), reason="checks the refusal order on a machine without a GPU")
@pytest.mark.parametrize("N", [500, 400, 200, 50, 1, 900, 1000])
def test_padded_shape_is_accepted_before_the_device_check(N):
    import lstm_hip
    rc, err = _create(N, lstm_hip.PAD_HIDDEN)
    assert rc == ENODEV, (N, rc, err)


@pytest.mark.parametrize("N", [500, 200, 50, 900, 1000])
def test_unpadded_odd_hidden_size_is_still_refused(N):
    rc, err = _create(N, 0)
    assert rc == EINVAL and "multiple of 16" in err, (N, rc, err)


@pytest.mark.parametrize("N,flags", [(0, 0), (-5, 0), (1025, 128), (1100, 128)])
def test_padded_shapes_that_stay_refused(N, flags):
    import lstm_hip
    rc, err = _create(N, lstm_hip.PAD_HIDDEN | flags, B=16)
    assert rc == EINVAL, (N, flags, rc, err)
