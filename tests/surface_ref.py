"""A plain reference for jmhip_distortion_surface and jmhip_bipred_surface (include/jmhip.h): the definition restated in numpy with int64
arithmetic, whole windows at once, so that the kernels can be compared at every displacement of the ranges the walks really use (a comparison
through the oracle costs 84 calls per displacement). tests/test_surface_ranges.py pins this helper on the oracle. No tests in here.

A job is any mapping with the fields of jmhip_surface_job / jmhip_bipred_surface_job (a numpy record or a dict)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

H2 = np.array([[1, 1], [1, -1]], np.int64)
H4 = np.kron(H2, H2)                          # the +-1 Hadamard matrices; sum |H D H^T| does not depend on the order of the rows
H8 = np.kron(H2, H4)


def window(ref, x0, y0, w, h):
    """the w x h samples whose top-left one is (x0, y0), each clamped to the picture: UMV access on the integer plane"""
    H, W = ref.shape
    ys = np.clip(np.arange(y0, y0 + h, dtype=np.int64), 0, H - 1)
    xs = np.clip(np.arange(x0, x0 + w, dtype=np.int64), 0, W - 1)
    return ref[np.ix_(ys, xs)].astype(np.int64)


def _geometry(job):
    R = int(job["R"])
    return R, 2 * R + 1, 16 * int(job["mb_x"]), 16 * int(job["mb_y"])


def _swept(ref, job):
    """[UW, UW, 16, 16]: the 16x16 block at displacement (cx - R + ax, cy - R + ay), ay outer"""
    R, UW, ox, oy = _geometry(job)
    win = window(ref, ox + int(job["cx"]) - R, oy + int(job["cy"]) - R, UW + 15, UW + 15)
    return sliding_window_view(win, (16, 16))


def uni_prediction(ref, job, clip=True):
    """[UW, UW, 16, 16]: the reference block of every displacement, weighted when job["wp"]; clip=False leaves the weighted values unclipped"""
    s = _swept(ref, job)
    if not int(job["wp"]):
        return s
    v = ((int(job["weight"]) * s + int(job["wp_round"])) >> int(job["wp_denom"])) + int(job["offset"])
    return np.clip(v, 0, 255) if clip else v


def bipred_prediction(ref1, ref2, job, clip=True):
    """[UW, UW, 16, 16]: the fixed block of ref1 at s_mv combined with the block of ref2 at every displacement"""
    _, _, ox, oy = _geometry(job)
    a = window(ref1, ox + int(job["s_mv"][0]), oy + int(job["s_mv"][1]), 16, 16)
    b = _swept(ref2, job)
    if not int(job["wp"]):
        return (a + b + 1) >> 1
    v = ((int(job["weight1"]) * a + int(job["weight2"]) * b + 2 * int(job["wp_round"])) >> (int(job["wp_denom"]) + 1)) + int(job["offset_bi"])
    return np.clip(v, 0, 255) if clip else v


def _hadamard_sads(d, n, Hn, rnd, shift):
    """d [UW, UW, 16, 16] -> [UW, UW, (16 / n)^2]: (sum |Hn D Hn^T| + rnd) >> shift of the n x n blocks in raster order"""
    UW, k = d.shape[0], 16 // n
    blocks = d.reshape(UW, UW, k, n, k, n).transpose(0, 1, 2, 4, 3, 5)
    t = Hn @ blocks @ Hn.T
    return ((np.abs(t).sum(axis=(-1, -2)) + rnd) >> shift).reshape(UW, UW, k * k)


def _surfaces(cur, job, pred):
    _, UW, ox, oy = _geometry(job)
    d = cur[oy:oy + 16, ox:ox + 16].astype(np.int64) - pred
    sad = np.abs(d).reshape(UW, UW, 16, 4, 4).sum(axis=-1)
    satd4 = _hadamard_sads(d, 4, H4, 1, 1)
    satd8 = _hadamard_sads(d, 8, H8, 2, 2)
    for v in (sad, satd4, satd8):
        assert v.min() >= 0 and v.max() < 65536, "a surface entry does not fit in 16 bits"
    return sad, satd4, satd8


def uni_surfaces(cur, ref, job):
    """-> sad [UW, UW, 16, 4], satd4 [UW, UW, 16], satd8 [UW, UW, 4] (int64) of one jmhip_surface_job"""
    return _surfaces(cur, job, uni_prediction(ref, job))


def bipred_surfaces(cur, ref1, ref2, job):
    """the same of one jmhip_bipred_surface_job; the weighted 8x8 entries are the Hadamard SADs of the straight 8x8 blocks"""
    return _surfaces(cur, job, bipred_prediction(ref1, ref2, job))
