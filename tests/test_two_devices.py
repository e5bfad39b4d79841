"""Two handles on two devices in one process.

A kernel's grant of dynamic LDS (request_lds / grant_lds, csrc/kernels.h) belongs to a device, and the library remembers what
it was granted per kernel instantiation and per device.  A handle on device 1 must therefore get every grant a handle on device
0 got before it: one training window (the products of gemm.hip ask for their LDS once per device) and a generate call with
top_k (a FILTER head; at this width its LDS is below the size that needs a request, so only the products reach the per-device
table) on each, from the same parameters and window, give the same bytes on both.  Every op is synchronised
before the other handle's next one.  Skipped where fewer than two devices are visible."""
import numpy as np
import pytest

import gpu_util as gu

N, S, B = 64, 4, 2


def _two_devices():
    import torch  # (asking the library about a device that is not there would leave the runtime's last error set)
    return torch.cuda.device_count() >= 2


@pytest.mark.gpu
def test_a_handle_on_each_of_two_devices_gives_the_same_bytes():
    import lstm_hip
    if not _two_devices():
        pytest.skip("fewer than two devices visible")
    P, xi, ti, h0, c0 = gu.random_case(N, S, B, seed=7)
    u = np.random.RandomState(11).random_sample((4, B))
    handles = [lstm_hip.Lstm(N, S, B, device=d) for d in (0, 1)]
    try:
        seen = [{}, {}]

        def step(name, op):  # one op on device 0, finished, then the same on device 1, finished
            for L, got in zip(handles, seen):
                got[name] = op(L)
                L.synchronize()

        step("set", lambda L: (L.set_params(P), L.set_state(0, h0, c0), L.set_window(xi, ti)) and None)
        step("forward", lambda L: L.forward())
        step("loss", lambda L: L.loss())
        step("backward", lambda L: L.backward())
        step("grads", lambda L: L.get_grads())
        step("adagrad", lambda L: L.adagrad(0.1))
        step("params", lambda L: L.get_params())
        step("state", lambda L: np.concatenate(L.get_state(S - 1)))
        step("generate", lambda L: L.generate(prompts=[b"ab", b"c"], count=4, u=u, top_k=8, score=True))
    finally:
        for L in handles:
            L.close()
    a, b = seen
    assert a["loss"] == b["loss"] and np.isfinite(a["loss"])
    for name in ("grads", "params", "state"):
        assert a[name].tobytes() == b[name].tobytes(), name
    assert not np.array_equal(a["params"], P)  # the update ran
    for k, (x, y) in enumerate(zip(a["generate"], b["generate"])):
        assert x.tobytes() == y.tobytes(), ("generate", k)
