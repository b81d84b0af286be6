"""The serial twin of dvp_fuse_consistency (host/fusion.cpp's ConsistencyMaskHost, through tests/consistency_host) without a GPU: on
the fusion ABI test's scene it equals the pair test of the float64 model of tests/np_fusion.py at min_views 0, 1, 2 and num_src + 1.
The model is float64 and the twin binary32, so the model says per pixel whether its answer is certain (tests/np_fusion.py's margins);
every certain pixel must agree, and all but a few pixels are certain."""
import numpy as np
import pytest

import np_mesh_mask as K

pytestmark = pytest.mark.hostbox


@pytest.fixture(scope="module", autouse=True)
def built():
    K.build_program()


@pytest.fixture(scope="module")
def scene():
    return K.scene()


@pytest.mark.parametrize("ref, src", K.PAIRS)
def test_the_twin_equals_the_float64_pair_test(scene, tmp_path, ref, src):
    lo, hi, ref_pixel = K.model(scene, ref, src)
    for min_views in (0, 1, 2, len(src) + 1):
        mask = K.twin(scene, ref, src, min_views, tmp_path)
        assert mask.shape == (K.H * K.W,) and set(np.unique(mask).tolist()) <= {0, 1}
        assert not mask[~ref_pixel].any()
        certain = ref_pixel & ((lo >= min_views) | (hi < min_views))
        assert certain.sum() >= 0.97 * ref_pixel.sum()            # (the comparison is not to be vacuous: 99.7 % and more are certain)
        want = lo >= min_views
        assert (mask[certain] == want[certain]).all(), (min_views, int((mask[certain] != want[certain]).sum()))
        if min_views == 0:
            assert (mask == ref_pixel).all()
        if min_views == len(src) + 1:
            assert not mask.any()
        if (ref, src, min_views) == (0, [1, 2], 2):
            assert 0 < mask.sum() < ref_pixel.sum()               # the outliers, holes and tilted normals take pixels away
