"""What the compiler reports for the two kernels of the packed adaptive generate (device-only compile for
gfx950, no GPU needed): every template instance of k_generate_packed_gains is there beside k_encode_gains_rgb, none uses scratch or
spills, and the aligned instances stay inside the project's bar for streaming kernels."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources  # noqa: E402

STREAMING_BAR = (128, 4)   # the project's bar for streaming kernels (tests/test_kernel_resources.py)


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(kernel_resources.HIPCC):
        pytest.skip("hipcc not present")
    return kernel_resources.resources(os.path.join(kernel_resources.CSRC, "uhdr_kernels.hip"))


def _pass1(table):
    """{(TF, F16, ALIGNED, TILES, RGB): resources}"""
    out = {}
    for k, v in table.items():
        m = re.search(r"k_generate_packed_gains<(\d), (true|false), (true|false), (\d), (true|false)>", k)
        if m:
            out[(int(m.group(1)), m.group(2) == "true", m.group(3) == "true", int(m.group(4)), m.group(5) == "true")] = v
    return out


def test_every_instance_is_present_and_none_uses_scratch(table):
    # F16 carries linear light, RGBA1010102 HLG or PQ; aligned or not; one span per block or four; one plane or RGB
    want = {(tf, tf == 0, al, tiles, rgb) for tf in (0, 1, 2) for al in (False, True) for tiles in (1, 4) for rgb in (False, True)}
    got = _pass1(table)
    assert set(got) == want
    rgb2 = [v for k, v in table.items() if re.search(r"\bk_encode_gains_rgb\b", k)]
    assert len(rgb2) == 1
    # no scratch memory and no VGPR spilled to it.  (The PQ instances that walk four spans keep 24 to 32 wave-uniform values in VGPR
    # lanes -- the compiler's "SGPR spill", no memory behind it -- as every PQ generate kernel does from gen_pair's inverse OETF on:
    # k_generate_packed 31 to 40; DESIGN.md section 4.1.9.  They may not exceed the kernel whose front end this is.)
    for key, r in list(got.items()) + [("k_encode_gains_rgb", rgb2[0])]:
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0, (key, r)
    base = {}
    for k, v in table.items():
        m = re.search(r"k_generate_packed<(\d), (true|false), (true|false), (\d), (true|false)>", k)
        if m:
            base[(int(m.group(1)), m.group(2) == "true", m.group(3) == "true", int(m.group(4)), m.group(5) == "true")] = v
    for key, r in got.items():
        assert r.get("sgpr_spill", 0) <= base[key].get("sgpr_spill", 0), (key, r, base[key])
    assert rgb2[0].get("sgpr_spill", 0) == 0


def test_aligned_instances_within_the_streaming_bar(table):
    for key, r in _pass1(table).items():
        if key[2]:
            assert r["vgpr"] <= STREAMING_BAR[0] and r["occupancy"] >= STREAMING_BAR[1] and r["lds"] == 0, (key, r)
    (r,) = [v for k, v in table.items() if re.search(r"\bk_encode_gains_rgb\b", k)]
    assert r["vgpr"] <= STREAMING_BAR[0] and r["occupancy"] >= STREAMING_BAR[1]
