"""The constructed images of the restart-interval tests (tests/test_jpeg_restart_cpu.py states the facts each one is there for,
tests/test_gpu_jpeg_restart.py sends them through the encoder), and the settings of the matrix both files walk."""
import numpy as np

SIZES = ((8, 8), (16, 16), (40, 24), (72, 56), (130, 66), (17, 33), (272, 48))
QUALITIES = (50, 95, 100)
# (restart_interval, restart_in_rows)
SETTINGS = ((1, 0), (3, 0), (8, 0), (9, 0), (65535, 0), (0, 1), (0, 2))


def plane_item(y, q):
    """a one-plane image -> the encoder tests' item (tests/test_gpu_jpeg_optimize.py item())"""
    h, w = y.shape
    return dict(yb=np.ascontiguousarray(y.reshape(-1)), ub=None, w=w, h=h, ls=w, cs=0, q=q)


def yuv_item(y, u, v, q):
    h, w = y.shape
    return dict(yb=np.ascontiguousarray(y.reshape(-1)), ub=np.ascontiguousarray(np.concatenate([u.reshape(-1), v.reshape(-1)])), w=w, h=h, ls=w,
                cs=w // 2, q=q)


def uniform(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def base_file(orc, it):
    """the file without intervals, by the CPU oracle's encoder (tests/test_jpeg_oracle.py pins it to libjpeg)"""
    return orc.jpeg_encode("orc", it["yb"], it["ub"], it["w"], it["h"], it["q"], it["ls"], it["cs"], icc=it.get("icc"))


# 2055 markers: the numbering wraps 256 times, more intervals than a workgroup has threads, every padding from 0 to 7, data 0xFF in
# front of markers, markers across the 64-byte chunks of the stuffing kernels
MANY_SEED, MANY_W, MANY_H = 3, 2056, 64


def many_intervals():
    return plane_item(uniform(MANY_SEED, MANY_H, MANY_W), 100), 1


# one plane 520 x 64, quality 100, 5 MCUs per interval.  What each seed's packed stream holds:
STEERED_W, STEERED_H, STEERED_RI = 520, 64, 5
STEERED_DATA_PAIR = 1      # a DATA byte 0xFF followed by a DATA byte 0xD0 .. 0xD7: no marker, and it gets its zero
STEERED_FF_AT_EDGE = 25    # a marker whose 0xFF is the last byte of a 16 KiB piece of the stuffing kernels, its Dn in the next
STEERED_DN_AT_EDGE = 20    # a marker that ends at such an edge


def steered(seed):
    return plane_item(uniform(seed, STEERED_H, STEERED_W), 100), STEERED_RI
