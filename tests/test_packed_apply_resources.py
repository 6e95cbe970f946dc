"""What the compiler reports for the kernels of csrc/uhdr_packed_apply.hip (device-only compile for gfx950, no GPU needed): every
template instance is there, none uses scratch, and the strip form stays inside the figures DESIGN.md section 4.2.5 states."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources  # noqa: E402

# the most registers and the least occupancy any strip kernel has, by what becomes of a gain
STRIP_LIMITS = {"FAST": (80, 6), "EXACT": (96, 5), "general metadata": (64, 8)}
STREAMING_BAR = (128, 4)   # the project's bar for streaming kernels (tests/test_kernel_resources.py)


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(kernel_resources.HIPCC):
        pytest.skip("hipcc not present")
    return kernel_resources.resources(os.path.join(kernel_resources.CSRC, "uhdr_packed_apply.hip"))


def _instances(table, kernel):
    out = {}
    for k, v in table.items():
        m = re.search(kernel + r"<(\d), (\d), (true|false)>", k)
        if m:
            out[(int(m.group(1)), int(m.group(2)), m.group(3) == "true")] = v
    return out


def test_every_instance_is_present_and_none_uses_scratch(table):
    want = {(fmt, kind, rgb) for fmt in (1, 2, 3, 4) for kind in (0, 1, 2, 3) for rgb in (False, True)}
    for kernel in ("k_apply_packed_s4", "k_apply_packed_px"):
        assert set(_instances(table, kernel)) == want, kernel
    assert any("k_build_srgb_codes" in k for k in table)
    bad = {k: v for k, v in table.items() if v.get("scratch", 0) != 0 or v.get("vgpr_spill", 0) != 0}
    assert not bad, bad


def test_strip_kernels_at_their_registers_and_occupancy(table):
    for (fmt, kind, rgb), r in _instances(table, "k_apply_packed_s4").items():
        vgpr, occ = STRIP_LIMITS["FAST" if kind == 0 else "EXACT" if kind == 1 else "general metadata"]
        assert r["vgpr"] <= vgpr and r["occupancy"] >= occ, (fmt, kind, rgb, r)
        assert r["vgpr"] <= STREAMING_BAR[0] and r["occupancy"] >= STREAMING_BAR[1]
        assert r["lds"] == 2048   # the 256-entry table and the four scale-4 weight tables, one copy each
    for key, r in _instances(table, "k_apply_packed_px").items():
        assert r["vgpr"] <= STREAMING_BAR[0] and r["occupancy"] >= STREAMING_BAR[1] and r["lds"] == 1024, (key, r)
