"""What the compiler reports for the kernels the 4:4:4 / 4:2:2 / 4:4:0 encode added to or changed in csrc/uhdr_jpeg.hip (device-only
compile for gfx950, no GPU needed): no kernel of the file uses scratch or spills; the new ones stay inside the bound their
neighbours keep; and the 4:2:0 / one-plane FDCT kernels, which carry none of the new geometry's code, stay inside theirs."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources  # noqa: E402

BAR = (128, 4)   # VGPRs at most, waves per SIMD at least (tests/test_kernel_resources.py)
# the kernels that take their block geometry from Job::hs, vs at run time, and the conversion kernel
INSIDE_THE_BAR = ("k_jpeg_opt_fdct_batch", "k_jpeg_sampled_opt_fdct_batch", "k_jpeg_emit_multi", "k_jpeg_opt_hist_batch", "k_jpeg_opt_count_batch",
                  "k_jpeg_opt_emit_batch", "k_jpeg_rst_hist_batch", "k_jpeg_rst_count_batch", "k_jpeg_rst_emit_batch", "k_rgba_to_ycc422",
                  "k_rgba_to_ycc420")
# The counting FDCT kernels hold a block's 64 coefficients and the predecessor's 64 samples at once: two waves per SIMD, as the
# 4:2:0 and the RGBA forms had before the sampled one joined them (197 VGPRs, the RGBA form's, is the bound they keep)
COUNTING_FDCT = ("k_jpeg_fdct_quant_count_multi", "k_jpeg_fdct_quant_count_multi_rgb", "k_jpeg_fdct_quant_count_multi_sampled")
NEW = ("k_jpeg_fdct_quant_count_multi_sampled", "k_jpeg_sampled_opt_fdct_batch", "k_rgba_to_ycc422")


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(kernel_resources.HIPCC):
        pytest.skip("hipcc not present")
    t = kernel_resources.resources(os.path.join(kernel_resources.CSRC, "uhdr_jpeg.hip"))
    return {k.split("(")[0].split("::")[-1]: v for k, v in t.items()}


def test_every_kernel_is_present(table):
    assert set(NEW) | set(INSIDE_THE_BAR) | set(COUNTING_FDCT) <= set(table)


def test_no_kernel_of_the_file_uses_scratch(table):
    for name, r in table.items():
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (name, r)


@pytest.mark.parametrize("kernel", INSIDE_THE_BAR)
def test_inside_the_bar(table, kernel):
    r = table[kernel]
    assert r["vgpr"] <= BAR[0] and r["occupancy"] >= BAR[1], r


@pytest.mark.parametrize("kernel", COUNTING_FDCT)
def test_counting_fdct_keeps_two_waves(table, kernel):
    r = table[kernel]
    assert r["vgpr"] <= 197 and r["occupancy"] >= 2, r


def test_single_image_fdct_keeps_its_four_waves(table):
    """uhdr_hip_jpeg_encode's kernel is the 4:2:0 / one-plane form alone"""
    r = table["k_jpeg_fdct_quant_count"]
    assert r["vgpr"] <= BAR[0] and r["occupancy"] >= BAR[1], r
