"""ops.conv_1d / ops.conv_2d (the node sequences of chatllm::ggml::conv_1d / conv_2d: IM2COL, MUL_MAT of the reshaped operands, RESHAPE, and in 2-D PERMUTE + CONT)
followed by the bias ADD of Conv1D::forward / Conv2D::forward, on the device, against the reference's own ggml_conv_1d / ggml_conv_2d graphs on its CPU backend
(tests/ref_conv.py): 0 differing words through a uint32 view."""
import numpy as np
import pytest

import ref_conv as RC
import ref_norm as N
from ref_ggml import GGML_TYPE_F16, GGML_TYPE_F32

pytestmark = pytest.mark.gpu


def _kernel(shape, seed, f16=True):
    k = (np.random.default_rng(seed).standard_normal(shape) * 0.5).astype(np.float32)
    return k.astype(np.float16) if f16 else k


def test_a_1d_stem_pair(gpu):
    """K3 s1 p1 then K3 s2 p1, IC 5 -> OC 8 -> 8, IW 20 (Whisper's stem at a small size); the second convolution reads the first one's device result"""
    x = RC.random_image((1, 5, 20), 1)
    k1, k2 = _kernel((8, 5, 3), 2), _kernel((8, 8, 3), 3)
    b1, b2 = RC.random_image((8,), 4), RC.random_image((8,), 5)
    want1 = RC.conv_1d_bias(k1.view(np.uint16), GGML_TYPE_F16, x, b1, 1, 1, 1)
    want2 = RC.conv_1d_bias(k2.view(np.uint16), GGML_TYPE_F16, want1, b2, 2, 1, 1)
    assert want1.shape == (1, 8, 20) and want2.shape == (1, 8, 10)
    y1 = gpu.ops.conv_1d(gpu.Tensor.from_numpy(k1), gpu.Tensor.from_numpy(x), 1, 1, 1)
    y1 = gpu.ops.add(y1, gpu.Tensor.from_numpy(b1.reshape(8, 1)))
    N.assert_same_words(y1.numpy().reshape(want1.shape), want1, "conv_1d K3 s1 p1 + bias")
    y2 = gpu.ops.conv_1d(gpu.Tensor.from_numpy(k2), y1, 2, 1, 1)
    y2 = gpu.ops.add(y2, gpu.Tensor.from_numpy(b2.reshape(8, 1)))
    N.assert_same_words(y2.numpy().reshape(want2.shape), want2, "conv_1d K3 s2 p1 + bias")


def _conv_2d(gpu, k, ktype, x, b, p):
    want = RC.conv_2d_bias(k.view(np.uint16) if ktype == GGML_TYPE_F16 else k, ktype, x, b, *p)
    y = gpu.ops.conv_2d(gpu.Tensor.from_numpy(k), gpu.Tensor.from_numpy(x), *p)
    y = gpu.ops.add(y, gpu.Tensor.from_numpy(b.reshape(-1, 1, 1)))
    return y.numpy().reshape(want.shape), want


def test_a_patch_embedding(gpu):
    """K == S == 4, IC 3, OC 12, an 8 x 12 image, two of them"""
    x = RC.random_image((2, 3, 8, 12), 6)
    got, want = _conv_2d(gpu, _kernel((12, 3, 4, 4), 7), GGML_TYPE_F16, x, RC.random_image((12,), 8), (4, 4, 0, 0, 1, 1))
    assert want.shape == (2, 12, 2, 3)
    N.assert_same_words(got, want, "conv_2d patch embedding + bias")


def test_an_f32_kernel(gpu):
    """an F32 kernel: F32 IM2COL followed by the F32 mat-mul that was there before; K3 s2 p1 with unequal sides"""
    x = RC.random_image((1, 3, 7, 9), 9)
    got, want = _conv_2d(gpu, _kernel((8, 3, 3, 3), 10, f16=False), GGML_TYPE_F32, x, RC.random_image((8,), 11), (2, 1, 1, 0, 1, 1))
    N.assert_same_words(got, want, "conv_2d with an F32 kernel + bias")
