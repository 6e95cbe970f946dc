"""What the compiler reports for the kernels of the progressive path in csrc/uhdr_jpeg.hip (device-only compile for gfx950, no GPU
needed): every one is in the code object, none uses scratch or spills, and each stays inside the project's bar for such kernels."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources  # noqa: E402

BAR = (128, 4)   # VGPRs at most, waves per SIMD at least (tests/test_kernel_resources.py)
KERNELS = ("k_jpeg_prog_zero_batch", "k_jpeg_prog_info_batch", "k_jpeg_prog_prefix_batch", "k_jpeg_prog_walk_batch", "k_jpeg_prog_hist_batch",
           "k_jpeg_prog_tables_batch", "k_jpeg_prog_count_batch", "k_jpeg_prog_layout_batch", "k_jpeg_prog_clear_batch", "k_jpeg_prog_emit_batch",
           "k_jpeg_prog_stuff_count_batch", "k_jpeg_prog_stuff_copy_batch")


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(kernel_resources.HIPCC):
        pytest.skip("hipcc not present")
    t = kernel_resources.resources(os.path.join(kernel_resources.CSRC, "uhdr_jpeg.hip"))
    return {k.split("(")[0].split("::")[-1]: v for k, v in t.items()}


def test_every_kernel_is_present(table):
    assert set(KERNELS) <= set(table), set(KERNELS) - set(table)
    assert {k for k in table if k.startswith("k_jpeg_prog_")} == set(KERNELS)   # a new one is listed here


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_inside_the_bar(table, kernel):
    r = table[kernel]
    assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, r
    assert r["vgpr"] <= BAR[0] and r["occupancy"] >= BAR[1], r


def test_no_kernel_of_the_file_uses_scratch(table):
    assert [k for k, r in table.items() if r.get("scratch", 0) != 0] == []


def test_the_stuffing_piece_still_fits_the_lds(table):
    """the scans' DHT and SOS markers take no stuffed zero, as the restart markers: the copy's expansion buffer is the same"""
    assert table["k_jpeg_prog_stuff_copy_batch"]["lds"] == table["k_jpeg_opt_stuff_copy_batch"]["lds"]
