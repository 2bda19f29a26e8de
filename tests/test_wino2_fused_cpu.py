"""CPU: what frcnn_winograd2_conv_x3 refuses before it touches a device -- null or non-positive arguments (FRCNN_E_ARG), an activation
other than NONE / RELU and a channel count other than 64 (FRCNN_E_UNSUPPORTED; the entry takes no channel count, so the ops wrapper
refuses it with the same code).  tests/test_abi.py covers header <-> exports <-> binding table."""
import ctypes

import pytest
import torch

E_ARG, E_UNSUPPORTED = -1, -3


def _call(x, N, H, W, planes, bias, act, y):
    import frcnn_hip
    p = ctypes.c_void_p
    return frcnn_hip.lib().frcnn_winograd2_conv_x3(p(x), N, H, W, p(planes), p(bias), act, p(y), p(0))


def test_null_and_non_positive_arguments_are_bad_arguments():
    fake = 4096                          # never dereferenced: every call below is refused before a launch
    assert _call(0, 1, 4, 4, fake, 0, 0, fake) == E_ARG
    assert _call(fake, 1, 4, 4, 0, 0, 0, fake) == E_ARG
    assert _call(fake, 1, 4, 4, fake, 0, 0, 0) == E_ARG
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, -1)):
        assert _call(fake, n, h, w, fake, 0, 1, fake) == E_ARG


def test_unknown_activation_and_oversized_tensor_are_unsupported():
    fake = 4096
    for act in (2, 3, -1):               # RELU6 and anything that is no activation id
        assert _call(fake, 1, 4, 4, fake, 0, act, fake) == E_UNSUPPORTED
    assert _call(fake, 2, 2048, 2048, fake, 0, 1, fake) == E_UNSUPPORTED          # N * H * W = 2^23: byte offsets would pass 2^31


def test_wrapper_refuses_other_channel_counts():
    import frcnn_hip
    from frcnn_hip import ops
    planes = torch.zeros(16 * 3 * 64 * 64 * 2, dtype=torch.uint8)
    for cin, cout in ((32, 32), (128, 128), (64, 128)):
        with pytest.raises(frcnn_hip.FrcnnHipError, match="not supported"):
            ops.winograd2_conv_x3(torch.zeros(1, 4, 4, cin), planes, None, 1, torch.zeros(1, 4, 4, cout))
    with pytest.raises(frcnn_hip.FrcnnHipError, match="not supported"):       # planes of another filter bank
        ops.winograd2_conv_x3(torch.zeros(1, 4, 4, 64), planes[:-2], None, 1, torch.zeros(1, 4, 4, 64))
