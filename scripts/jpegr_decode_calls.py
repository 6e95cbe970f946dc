"""One untimed pass over the default-bound calls of tests/test_gpu_jpegr_decode_rounds.py, for a kernel trace
(profiles/r23_decode_rounds.txt):

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python scripts/jpegr_decode_calls.py
    UHDR_HIP_LIB=<another build's libuhdr_hip.so> rocprofv3 --kernel-trace ... -- python scripts/jpegr_decode_calls.py
    python scripts/jpegr_decode_calls.py --compare <dir A> <dir B>      # the ordered (kernel, grid, workgroup) lists of two traces

The calls, each made once, in this order: per entry point (uhdr_hip_jpegr_decode_batch, _batch_ex, _rgbmap_batch, _md_batch, then
_scaled_batch at 1/1 and 1/2) and memory space (device, host) the SDR and the HLG call of the test.  The corrupt file of the test is
found with single calls of the same library first, so those launches are in both traces too.

    python scripts/jpegr_decode_calls.py --even-only      # the same calls without their odd-sized 4:2:0 files (17x9, 45x37)

An odd-sized 4:2:0 image has the bytes its decoder does not write cleared in front of the decode launch, and a
kernel trace shows the runtime's fill kernels; a call without such a file must enqueue what it enqueued before
(profiles/r24_odd420_decode.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.tone_batch_calls import compare  # noqa: E402


def main(even_only=False):
    import torch

    from libultrahdr_dev_amd import api
    from tests import test_gpu_jpegr_decode_rounds as G
    torch.cuda.set_device(0)
    api.init(0)
    files, calls = G._files(api), 0
    for entry, scales in [(e, (1,)) for e in G.ENTRIES[:4]] + [(G.ENTRIES[4], (1, 2))]:
        for s in scales:
            batch = [files[k] for k in G._names(entry)] + ([files["sample"]] if s == 2 else [])
            if even_only:
                batch = [f for f in batch if (f.hs, f.vs) != (2, 2) or not (f.w | f.h) & 1]
            for device in (True, False):
                for fmt in (api.OUTPUT_SDR, api.OUTPUT_HDR_HLG):
                    rc, stat, _, _ = G._call(api, entry, batch, fmt, s, device)
                    assert stat == [G._status(api, f, fmt, s) for f in batch], (entry, s, device, fmt, rc, stat)
                    calls += 1
    torch.cuda.synchronize()
    print("%d batch calls%s made with %s" % (calls, " without odd-sized 4:2:0 files" if even_only else "", api.LIB_PATH))


if __name__ == "__main__":
    if "--compare" in sys.argv:
        i = sys.argv.index("--compare")
        sys.exit(compare(sys.argv[i + 1], sys.argv[i + 2]))
    main("--even-only" in sys.argv)
