"""Root noise without a GPU: the ctypes bindings exist with the header's signatures, the C entry
points refuse bad arguments before any HIP call, the Python wrappers refuse a bad alpha before any
device call, and SelfPlay's argument handling follows the opt-in rule (the reference's
dirichlet_alpha / dirichlet_epsilon alone never enable the noise)."""
import ctypes as C

import pytest
import torch

EINVAL = -22


def test_bindings_and_c_argument_checks():
    import rvz
    sig = rvz._lib.SIGNATURES
    assert sig["rvz_search_root_noise"] == (C.c_int, [C.c_void_p, C.c_double, C.c_double,
                                                      C.c_uint32])
    assert len(sig["rvz_dirichlet_noise"][1]) == 10
    lib = rvz.load()
    p = 0x10000                                   # never dereferenced
    for alpha in (0.0, -0.3, float("nan"), float("inf"), 1e-60, 1e60):
        assert lib.rvz_dirichlet_noise(8, 4, p, p, p, 0, alpha, p, None, None) == EINVAL
    assert lib.rvz_dirichlet_noise(8, 4, p, p, p, 0, 0.3, None, None, None) == EINVAL   # null out
    assert lib.rvz_dirichlet_noise(8, 4, None, p, p, 0, 0.3, p, None, None) == EINVAL
    assert lib.rvz_dirichlet_noise(8, 4, p, p, p, 0, 0.3, p, p + 4, None) == EINVAL    # misaligned
    assert lib.rvz_dirichlet_noise(5, 4, p, p, p, 0, 0.3, p, None, None) == EINVAL
    assert lib.rvz_dirichlet_noise(8, -1, p, p, p, 0, 0.3, p, None, None) == EINVAL
    assert lib.rvz_dirichlet_noise(8, 0, None, None, None, 0, 0.3, None, None, None) == 0
    assert lib.rvz_search_root_noise(None, 0.3, 0.25, 0) == EINVAL


def test_python_rejects_bad_arguments_before_any_device_call():
    import rvz

    class NoDevice:                # Engine.root_noise must raise before it touches the handle
        pass

    for alpha, eps in ((0.0, 0.25), (-1.0, 0.25), (float("nan"), 0.25), (float("inf"), 0.25),
                       ("x", 0.25), (None, 0.25), (1e-60, 0.25), (0.3, -0.1), (0.3, 1.5),
                       (0.3, float("nan")), (0.3, None)):
        with pytest.raises(rvz.RvzError):
            rvz.Engine.root_noise(NoDevice(), alpha, eps)
    with pytest.raises(AttributeError):       # valid arguments reach the (absent) device call
        rvz.Engine.root_noise(NoDevice(), 0.3, 0.25)
    host = torch.zeros(2, dtype=torch.int64)  # host tensors: a device call would raise otherwise
    for alpha in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(rvz.RvzError, match="alpha"):
            rvz.dirichlet_noise(host, host, host, 0, alpha)
    with pytest.raises(rvz.RvzError, match="board_size"):
        rvz.dirichlet_noise(host, host, host, 0, 0.3, board_size=7)


def test_selfplay_argument_handling():
    from rvz.selfplay import root_noise_args
    import rvz
    # the reference's pipeline always passes these two; alone they must stay inert
    assert root_noise_args({"dirichlet_alpha": 0.03, "dirichlet_epsilon": 0.25}) is None
    assert root_noise_args({}) is None
    assert root_noise_args({"root_noise": False, "dirichlet_alpha": -1.0}) is None
    assert root_noise_args({"root_noise": True}) == (0.03, 0.25, 0)      # config.py:25-26
    assert root_noise_args({"root_noise": True, "dirichlet_alpha": 0.3, "dirichlet_salt": 7}) == \
        (0.3, 0.25, 7)
    assert root_noise_args({"root_noise": True, "dirichlet_epsilon": 0.0}) == (0.03, 0.0, 0)
    for bad in ({"dirichlet_alpha": 0.0}, {"dirichlet_alpha": float("nan")},
                {"dirichlet_epsilon": 1.5}, {"dirichlet_epsilon": -0.1}):
        with pytest.raises(rvz.RvzError):
            root_noise_args({"root_noise": True, **bad})
