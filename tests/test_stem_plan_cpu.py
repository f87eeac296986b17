"""conv2d_stem_plan is host arithmetic: the plan cases of
test_gpu_stem_fwd.py hold without a device."""
import pytest

from ddp_tricks_amd.ops import load_extension

from test_gpu_stem_fwd import FITS, MISFITS

ext = load_extension(required=True)


def test_plan_direct_where_it_fits():
    for N, H, W, Ko, pad in FITS:
        for stem in (-1, 1):
            assert ext.conv2d_stem_plan(N, 1, H, W, Ko, 3, 3, 1, pad,
                                        stem) == "direct"
        assert ext.conv2d_stem_plan(N, 1, H, W, Ko, 3, 3, 1, pad, 0) == "mfma"


@pytest.mark.parametrize("name", sorted(MISFITS))
def test_plan_mfma_for_misfits_even_when_forced(name):
    for stem in (-1, 0, 1):
        assert ext.conv2d_stem_plan(*MISFITS[name], stem) == "mfma"


def test_plan_rows_wider_than_the_lds_image_stay_on_mfma():
    assert ext.conv2d_stem_plan(1, 1, 8, 1363, 64, 3, 3, 1, 1) == "direct"
    assert ext.conv2d_stem_plan(1, 1, 8, 1364, 64, 3, 3, 1, 1) == "mfma"
