"""Strided views of split tensors as yolo_conv_fwd's input, host side only (yolo_conv_kernel_name: no launch, no GPU).

The split kernels read every plane of x in whole 32-channel K-chunks: round_up(Cin, 32) channels from x and the same number from
x + x_lo_offset, whatever Cin is (include/yolo_amd.h, x_pixel_stride / x_lo_offset).  A descriptor whose lo-plane chunks would
leave the pixel is refused; the ragged slices tests/test_gpu_split_edges.py runs on the device are accepted.
"""
import pytest

from util import conv_variant, SPLIT

# (Ctot, c0, Cin, Cp) of test_gpu_split_edges.SLICES: channels [c0, c0 + Cin) of a split buffer with planes of Cp channels
SLICES = [(128, 16, 40, 128), (64, 0, 24, 64), (32, 16, 16, 64), (96, 48, 48, 128)]


def _case(cin, k=1, stride=1, cout=32):
    return (2, cin, 7, 9, cout, k, stride, False)


@pytest.mark.parametrize('dtype', SPLIT)
def test_split_lo_chunks_must_stay_inside_the_pixel(dtype):
    for algo in (0, 1):
        # unpadded planes: the hi plane of 40 channels directly followed by the lo plane
        assert conv_variant(_case(40), dtype, algo, fields=dict(x_pixel_stride=80, x_lo_offset=40)) is None
        # planes of 96 channels read from channel 48 on, Cin = 40: the lo plane's 40 channels end inside the pixel (96 + 40 <= 144),
        # the 64 the kernels read do not (96 + 64 > 144)
        assert conv_variant(_case(40), dtype, algo, fields=dict(x_pixel_stride=144, x_lo_offset=96)) is None
        assert conv_variant(_case(40), dtype, algo, fields=dict(x_pixel_stride=160, x_lo_offset=96)) is not None
        # Cin a multiple of 32: nothing is read beyond Cin, the tight layout stays valid
        assert conv_variant(_case(64), dtype, algo, fields=dict(x_pixel_stride=128, x_lo_offset=64)) is not None
        # a 3x3 stride 2 on 48 channels (the down-sampling conv behind a ragged pyramid level): one 32-channel chunk short
        assert conv_variant(_case(48, 3, 2), dtype, algo, fields=dict(x_pixel_stride=144, x_lo_offset=96)) is None
        assert conv_variant(_case(48, 3, 2), dtype, algo, fields=dict(x_pixel_stride=160, x_lo_offset=96)) is not None


@pytest.mark.parametrize('dtype', SPLIT)
@pytest.mark.parametrize('layout', SLICES)
def test_split_ragged_slices_are_accepted(dtype, layout):
    Ctot, c0, Cin, Cp = layout
    assert Cp >= c0 + -(-Cin // 32) * 32 and Cp >= Ctot
    for k, stride in ((1, 1), (3, 1), (3, 2)):
        for cout in (32, 64):
            for algo in (0, 1):
                assert conv_variant(_case(Cin, k, stride, cout), dtype, algo,
                                    fields=dict(x_pixel_stride=2 * Cp, x_lo_offset=Cp)) is not None, (k, stride, cout, algo)
