"""One untimed pass over the batch calls of tests/test_gpu_tone_runs.py, for a kernel trace (profiles/r22_tone_driver.txt):

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python scripts/tone_batch_calls.py
    UHDR_HIP_LIB=<another build's libuhdr_hip.so> rocprofv3 --kernel-trace ... -- python scripts/tone_batch_calls.py
    python scripts/tone_batch_calls.py --compare <dir A> <dir B>      # the ordered (kernel, grid, workgroup) lists of two traces

The calls, each made once, in this order: per transfer function uhdr_hip_tonemap_sdr_batch on the 41-image run layout with peaks and
with hdr_peak_nits == NULL, then on the 515-image batch; per packed form the same three of uhdr_hip_tonemap_packed_batch; then
uhdr_hip_tonemap_batch, uhdr_hip_tonemap_sdr_batch with TONEMAP_SHIFT and uhdr_hip_convert_yuv_batch on the layout.  Every frame
of a call is uploaded before the call, so the launches of a call follow each other in the trace."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def launches(trace_dir):
    """[(kernel, grid, workgroup)] of the library's kernels (uhdr::) in a rocprofv3 --kernel-trace csv, in start order"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"]
            if "uhdr::" in name:
                rows.append((int(r["Start_Timestamp"]), name, tuple(int(r["Grid_Size_" + a]) for a in "XYZ"),
                             tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ")))
    return [r[1:] for r in sorted(rows)]


def compare(a, b):
    la, lb = launches(a), launches(b)
    names = {}
    for name, _, _ in la:
        names[name.split("(")[0]] = names.get(name.split("(")[0], 0) + 1
    print("%d launches in %s, %d in %s" % (len(la), a, len(lb), b))
    for name in sorted(names):
        print("  %5d  %s" % (names[name], name))
    first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None)
    if first is None and len(la) == len(lb) and la:
        print("the ordered lists of (kernel, grid, workgroup) are identical")
        return 0
    print("the lists DIFFER, first at launch %r: %r against %r" % (first, la[first:first + 1], lb[first:first + 1]))
    return 1


def main():
    import torch

    from libultrahdr_dev_amd import api
    from tests import packed_tonemap_cases as K
    from tests import tone_run_cases as R
    from tests import tonemap_cases as T
    from tests import test_gpu_tone_runs as G
    from tests.gpu_util import stream_ptr
    torch.cuda.set_device(0)
    api.init(0)
    lib, calls = api.load(), 0
    for tf in (T.TF_HLG, T.TF_PQ, T.TF_LINEAR):
        for images, nulls in ((R.layout(False), (False, True)), (R.many(False), (False,))):
            frames = G.planar_frames(api, images, tf)
            for null in nulls:
                assert G.run_batch(api, frames, tf, R.peaks(images, null))[0] == 0
                calls += 1
    for form in K.FORMS:
        for images, nulls in ((R.layout(True), (False, True)), (R.many(True), (False,))):
            frames = G.packed_frames(api, images, form)
            for null in nulls:
                assert G.run_packed_batch(api, frames, form[1], R.peaks(images, null))[0] == 0
                calls += 1
    images = R.layout(False)
    frames = G.planar_frames(api, images, T.TF_PQ)
    sa, da = api.image_array([f.src for f in frames]), api.image_array([f.dst for f in frames])
    assert lib.uhdr_hip_tonemap_batch(len(frames), sa, da, stream_ptr()) == 0
    assert G.run_batch(api, frames, T.TF_PQ, None, op=T.SHIFT)[0] == 0
    assert lib.uhdr_hip_convert_yuv_batch(len(frames), da, api.CG_BT2100, api.CG_P3, stream_ptr()) == 0
    torch.cuda.synchronize()
    print("%d batch calls made with %s" % (calls + 3, api.LIB_PATH))


if __name__ == "__main__":
    if "--compare" in sys.argv:
        i = sys.argv.index("--compare")
        sys.exit(compare(sys.argv[i + 1], sys.argv[i + 2]))
    main()
