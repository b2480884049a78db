"""CPU: the block generators and the block loop of the reference's GPU DoG
(BlockGeneratorVariableSizeSimple.java:30-132, DifferenceOfGaussianCUDA.java:125-177)
as restated in spim_registration_amd.legacy, and the claim the fused border mode rests
on: the blocks of the approximate mode do not change a voxel."""
import numpy as np
import pytest

from oracle import dog_ref
from spim_registration_amd import legacy


def test_variable_size_simple_known_answer():
    """The reference's own main (BlockGeneratorVariableSizeSimple.java:136); the expected
    vectors are read off the Java by hand."""
    blocks = legacy.BlockGeneratorVariableSizeSimple((3, 2, 1)).divide_into_blocks((1025, 1024, 117), (17, 17, 4))
    assert len(blocks) == 6
    # dim 0 fastest (LocalizingZeroMinIntervalIterator)
    assert [b.effective_offset[0] > 0 for b in blocks] == [False, True, True, False, True, True]
    assert [b.effective_offset[1] > 0 for b in blocks] == [False, False, False, True, True, True]
    b = blocks[1]   # block (1, 0, 0): a middle block in x, the first in y, the only one in z
    assert b.offset == (333, 0, 0)
    assert b.effective_offset == (341, 0, 0)
    assert b.effective_local_offset == (8, 0, 0)
    assert b.effective_size == (341, 512, 117)
    assert b.block_size == (357, 520, 117)
    b = blocks[5]   # block (2, 1, 0): last in x (1025 % 3 = 2: the :112 remainder quirk) and in y
    assert b.offset == (678, 504, 0)
    assert b.effective_offset == (686, 512, 0)
    assert b.effective_local_offset == (8, 8, 0)
    assert b.effective_size == (343, 512, 117)
    assert b.block_size == (351, 520, 117)
    b = blocks[0]   # block (0, 0, 0): no halo towards the image border
    assert b.offset == (0, 0, 0) and b.effective_local_offset == (0, 0, 0)
    assert b.effective_size == (341, 512, 117) and b.block_size == (349, 520, 117)


@pytest.mark.parametrize("dims,nb,ks", [((24, 20, 18), (3, 2, 2), (7, 5, 3)), ((48, 40, 36), (2, 2, 3), (13, 13, 13)),
                                        ((9, 8, 7), (1, 1, 1), (7, 7, 7)), ((30, 7, 12), (5, 1, 4), (3, 9, 5))])
def test_variable_size_simple_tiles_divisible_dims_once(dims, nb, ks):
    """Block counts that divide the dims: the effective regions cover every voxel exactly
    once, and every block lies inside the image with its effective region at its local offset."""
    blocks = legacy.BlockGeneratorVariableSizeSimple(nb).divide_into_blocks(dims, ks)
    assert len(blocks) == int(np.prod(nb))
    hits = np.zeros(dims[::-1], np.int32)
    for b in blocks:
        eo, es = b.effective_offset, b.effective_size
        hits[eo[2]:eo[2] + es[2], eo[1]:eo[1] + es[1], eo[0]:eo[0] + es[0]] += 1
        for d in range(3):
            assert b.offset[d] >= 0 and b.offset[d] + b.block_size[d] <= dims[d]
            assert b.offset[d] + b.effective_local_offset[d] == eo[d]
            assert b.effective_local_offset[d] + es[d] <= b.block_size[d]
    assert hits.min() == 1 and hits.max() == 1


def test_variable_size_simple_too_many_blocks():
    """effectiveSize <= 0 returns null (:116-120)."""
    assert legacy.BlockGeneratorVariableSizeSimple((5, 1, 1)).divide_into_blocks((4, 8, 8), (3, 3, 3)) is None


class NumpyConvolution:
    """A numpy stand-in for CUDASeparableConvolution: ``_conv`` with the native call's
    arguments, computing in place with the oracle's separable convolution."""
    MODES = {0: "zero", 1: "value", 2: "border", 3: "mirror"}

    def __init__(self):
        self.calls = []

    def _conv(self, n, image, kx, ky, kz, w, h, d, cx, cy, cz, oob, oobv, dev):
        assert cx and cy and cz and len(kx) == len(ky) == len(kz) == n
        self.calls.append(((w, h, d), int(oob)))
        vol = image.reshape(d, h, w)
        vol[...] = dog_ref.gauss3d(vol, (kx, ky, kz), mode=self.MODES[int(oob)], value=oobv)
        return True


def test_gauss_blocks_remainder_reaches_outside_the_image():
    """1025 columns in 3 blocks: the last block's effectiveOffset (:112) puts it past the
    image, where the Java's access to the unextended image throws too."""
    img = np.zeros((2, 2, 1025), np.float32)
    with pytest.raises(ValueError, match=":112"):
        legacy.gauss_blocks_cuda(img, (1.0, 1.0, 1.0), (3, 1, 1), False, NumpyConvolution(), 0)


@pytest.mark.parametrize("sigma", [(1.7, 1.7, 1.7), (1.0, 2.1, 1.4)])
def test_blocks_do_not_change_the_approximate_result(sigma):
    """Blocked == single block == clamp-to-edge over the whole image, bit for bit: the
    halo inside the image is kernelSize / 2 of real voxels and the taps beyond the true
    kernel length are the zero padding."""
    rng = np.random.default_rng(5)
    img = rng.random((18, 20, 24), dtype=np.float32)
    keep = img.copy()
    cuda = NumpyConvolution()
    blocked = legacy.gauss_blocks_cuda(img, sigma, (2, 2, 3), False, cuda, 0)
    assert len(cuda.calls) == 12 and all(oob == 2 for _, oob in cuda.calls)
    assert len({dims for dims, _ in cuda.calls}) > 1    # genuinely smaller blocks
    single = legacy.gauss_blocks_cuda(img, sigma, (1, 1, 1), False, cuda, 0)
    assert cuda.calls[-1] == ((24, 20, 18), 2)
    np.testing.assert_array_equal(img, keep)             # the source is not modified
    np.testing.assert_array_equal(blocked, single)
    np.testing.assert_array_equal(single, dog_ref.gauss3d(img, dog_ref.cuda_kernels(sigma), mode="border"))
    assert not np.array_equal(single, dog_ref.gauss3d(img, dog_ref.cuda_kernels(sigma), mode="mirror"))


def test_accurate_blocks_are_the_mirror_extension():
    """accurate = true: full halos of the mirror-extended image, so the native border
    extension only ever meets zero taps and the result is the mirror-single Gaussian."""
    rng = np.random.default_rng(6)
    img = rng.random((18, 20, 24), dtype=np.float32)
    sigma = (1.7, 1.7, 1.7)
    got = legacy.gauss_blocks_cuda(img, sigma, (2, 2, 3), True, NumpyConvolution(), 0)
    np.testing.assert_array_equal(got, dog_ref.gauss3d(img, dog_ref.cuda_kernels(sigma), mode="mirror"))
