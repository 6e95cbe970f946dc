"""What the compiler reports for the scaled inverse DCT of csrc/uhdr_jpeg_dec.hip (device-only compile for gfx950, no GPU needed): the
kernel is in the code object, uses no scratch, spills nothing and stays inside the project's bar for such kernels -- with the 8x8
chroma blocks of a 4:2:0 image at 1/2 in it, which is why those are computed eight lanes to a block."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources  # noqa: E402

BAR = (128, 4)   # VGPRs at most, waves per SIMD at least (tests/test_kernel_resources.py)
KERNELS = ("k_jd_idct_scaled_multi",)


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(kernel_resources.HIPCC):
        pytest.skip("hipcc not present")
    t = kernel_resources.resources(os.path.join(kernel_resources.CSRC, "uhdr_jpeg_dec.hip"))
    return {k.split("(")[0].split("::")[-1]: v for k, v in t.items()}


def test_every_kernel_is_present(table):
    assert set(KERNELS) <= set(table), set(KERNELS) - set(table)
    assert {k for k in table if k.startswith("k_jd_idct_scaled")} == set(KERNELS)   # a new one is listed here


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_inside_the_bar(table, kernel):
    r = table[kernel]
    assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, r
    assert r["vgpr"] <= BAR[0] and r["occupancy"] >= BAR[1], r


def test_the_cooperative_tiles_fit_the_lds(table):
    """16 tiles of 73 words: far below what would cost the kernel a wave"""
    assert table["k_jd_idct_scaled_multi"]["lds"] == 16 * 73 * 4
