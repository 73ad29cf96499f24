"""The cases of tests/test_surface_ranges.py: one table for its CPU half (the numpy reference against the oracle, and what the cases can
tell) and its GPU half (the kernels against the numpy reference), so that both run the same inputs. No tests in here.

Ranges: 0 (one displacement); 1, 3, 7 (2R = 2 mod 4: the other window pitch); 7 / 8 (225 / 289 displacements: the last size one pass of 256
lanes covers and the first that needs a second, partial one); 16, 32 (the ranges of the walks); 64 (the interface's bound). Pictures: one
macroblock (from R = 16 on the window is larger than the picture both ways), 64x48, and 48x32 under the 144-sample window of R = 64."""
from collections import namedtuple

import numpy as np

from tests.test_me import make_pair

Case = namedtuple("Case", "name size kind R jobs wp seed")

FAR = 4096          # the accepted bound of |cx|, |cy|, |s_mv|: the whole window / block is one clamped sample per row and column

# ---- uni-directional jobs: (mb_x, mb_y, slot, cx, cy)
# an inner macroblock with a small centre, the top-left one pushed across the corner, the bottom-right one far outside, then the bounds
U64_A = [(1, 1, 1, 2, -1), (0, 0, 2, -14, -9), (3, 2, 0, 30, 25), (2, 1, 1, FAR, -FAR), (0, 2, 2, -FAR, FAR), (3, 0, 0, FAR, 2)]
U64_B = [(2, 1, 2, -3, 1), (0, 0, 0, -11, -13), (3, 2, 1, 90, 70), (1, 0, 2, -FAR, FAR), (2, 2, 0, FAR, -FAR), (0, 1, 1, -2, -FAR)]
U16 = [(0, 0, 2, 1, -2), (0, 0, 0, -14, -9), (0, 0, 1, 40, -35), (0, 0, 2, FAR, -FAR), (0, 0, 0, -FAR, FAR)]
U48 = [(1, 0, 1, 3, 2), (0, 0, 2, -14, -9), (2, 1, 0, 100, 90), (1, 1, 1, -FAR, FAR)]
# weight, offset, wp_round, wp_denom
UW_EXISTING, UW_NEGATIVE, UW_DENOM0, UW_DENOM15 = (37, -6, 16, 5), (-20, 200, 16, 5), (2, -90, 0, 0), (29000, 4, 16384, 15)
UW_SAT255, UW_SAT0 = (64, 90, 16, 5), (32, -60, 16, 5)          # 2s + 90 and s - 60
UNI_SATURATING = {"r8_sat255": 255, "r16_sat0": 0}

UNI_CASES = [
    Case("r0_noise", (64, 48), "noise", 0, U64_A, None, 101),
    Case("r1_shift_w", (64, 48), "shift", 1, U64_B, UW_EXISTING, 102),
    Case("r3_extremes", (16, 16), "extremes", 3, U16, None, 103),
    Case("r3_denom15", (64, 48), "noise", 3, U64_A, UW_DENOM15, 104),
    Case("r7_negative", (64, 48), "noise", 7, U64_B, UW_NEGATIVE, 105),
    Case("r8_extremes", (64, 48), "extremes", 8, U64_A, None, 106),
    Case("r8_denom0", (64, 48), "shift", 8, U64_B, UW_DENOM0, 107),
    Case("r8_sat255", (16, 16), "noise", 8, U16, UW_SAT255, 108),
    Case("r16_extremes", (16, 16), "extremes", 16, U16, None, 109),
    Case("r16_sat0", (64, 48), "noise", 16, U64_A, UW_SAT0, 110),
    Case("r32_shift_w", (64, 48), "shift", 32, U64_B[:4], UW_EXISTING, 111),
    Case("r64_noise", (48, 32), "noise", 64, U48, None, 112),
]
# the growth leg: three calls in ONE context (same pictures: size, kind and seed agree), each on other jobs -- a larger, a smaller inside the
# larger allocation, then the largest
UNI_GROWTH = [
    Case("grow_r32", (64, 48), "noise", 32, U64_A[:3], None, 120),
    Case("grow_r4", (64, 48), "noise", 4, U64_B[:3], UW_EXISTING, 120),
    Case("grow_r64", (64, 48), "noise", 64, [(1, 1, 0, -5, 6), (3, 0, 1, 20, -30), (0, 2, 2, -FAR, FAR)], None, 120),
]

# ---- bi-predictive jobs: (mb_x, mb_y, slot of the fixed block, slot of the swept picture, s_mv, cx, cy)
B64_A = [(1, 1, 0, 1, (1, -2), 2, -1), (0, 0, 1, 2, (-9, -6), -14, -9), (3, 2, 2, 0, (11, 9), 30, 25), (2, 1, 1, 1, (3, 2), -3, 4),
         (0, 2, 0, 2, (FAR, -FAR), 5, -2), (3, 0, 2, 1, (-FAR, FAR), FAR, -FAR)]
B64_B = [(2, 1, 2, 0, (-2, 3), -3, 1), (0, 0, 0, 1, (-12, -7), -11, -13), (3, 2, 1, 2, (9, 12), 90, 70), (1, 0, 2, 2, (4, -1), 1, 2),
         (2, 2, 1, 0, (-FAR, FAR), -4, 3), (0, 1, 0, 2, (6, 5), -FAR, FAR)]
B16 = [(0, 0, 2, 0, (1, 1), 1, -2), (0, 0, 0, 1, (-9, -6), -14, -9), (0, 0, 1, 2, (3, -2), 40, -35), (0, 0, 1, 1, (-2, 2), 2, 3),
       (0, 0, 2, 1, (FAR, -FAR), -FAR, FAR)]
B48 = [(1, 0, 1, 2, (2, -1), 3, 2), (0, 0, 2, 0, (-9, -6), -14, -9), (2, 1, 0, 1, (-FAR, FAR), 100, 90), (1, 1, 0, 0, (5, 3), FAR, -FAR)]
# weight1, weight2, offset_bi, wp_round, wp_denom
BW_EXISTING, BW_NEGATIVE, BW_DENOM0, BW_DENOM15 = (37, 24, -3, 16, 5), (80, -20, 10, 16, 5), (1, 2, -70, 0, 0), (20000, 12000, 2, 16384, 15)
BW_SAT255, BW_SAT0 = (32, 32, 100, 16, 5), (32, 32, -100, 16, 5)          # the plain average + 100 and - 100
BI_SATURATING = {"r8_sat255": 255, "r16_sat0": 0}

BI_CASES = [
    Case("r0_noise", (64, 48), "noise", 0, B64_A, None, 201),
    Case("r1_shift_w", (64, 48), "shift", 1, B64_B, BW_EXISTING, 202),
    Case("r3_extremes", (16, 16), "extremes", 3, B16, None, 203),
    Case("r3_denom15", (64, 48), "noise", 3, B64_A, BW_DENOM15, 204),
    Case("r7_negative", (64, 48), "noise", 7, B64_B, BW_NEGATIVE, 205),
    Case("r8_extremes", (64, 48), "extremes", 8, B64_A, None, 206),
    Case("r8_denom0", (64, 48), "shift", 8, B64_B, BW_DENOM0, 207),
    Case("r8_sat255", (16, 16), "noise", 8, B16, BW_SAT255, 208),
    Case("r16_extremes", (16, 16), "extremes", 16, B16, None, 209),
    Case("r16_sat0", (64, 48), "noise", 16, B64_A, BW_SAT0, 210),
    Case("r32_shift_w", (64, 48), "shift", 32, B64_B[:4], BW_EXISTING, 211),
    Case("r64_noise", (48, 32), "noise", 64, B48, None, 212),
]
BI_GROWTH = [
    Case("grow_r32", (64, 48), "noise", 32, B64_A[:3], None, 220),
    Case("grow_r4", (64, 48), "noise", 4, B64_B[:3], BW_EXISTING, 220),
    Case("grow_r64", (64, 48), "noise", 64, [(1, 1, 0, 2, (4, -3), -5, 6), (3, 0, 1, 1, (-8, 20), 20, -30), (0, 2, 2, 0, (1, 0), -FAR, FAR)], None, 220),
]


def pictures(case):
    """-> the current picture and the pictures of the three reference slots, each its own (a job that names one must not be served from another)"""
    w, h = case.size
    rng = np.random.default_rng(case.seed)
    if case.kind == "noise":
        planes = rng.integers(0, 256, (4, h, w)).astype(np.uint8)
        return planes[0], list(planes[1:])
    if case.kind == "extremes":           # every sample 0 or 255, all four pictures independent: entries near the maxima of the packed halves
        planes = (rng.integers(0, 2, (4, h, w)) * 255).astype(np.uint8)
        return planes[0], list(planes[1:])
    cur, ref = make_pair(rng, w, h, "shift")       # as three_refs of tests/test_dist.py
    return cur, [ref, np.roll(make_pair(rng, w, h, "shift")[1], (2, -3), (0, 1)), make_pair(rng, w, h, "noise")[1]]


def uni_jobs(case):
    """-> the jobs as dicts with the fields of jmhip_surface_job"""
    jobs = []
    for mx, my, slot, cx, cy in case.jobs:
        j = dict(mb_x=mx, mb_y=my, ref=slot, R=case.R, cx=cx, cy=cy, wp=0, weight=0, offset=0, wp_round=0, wp_denom=0, pad=0)
        if case.wp:
            j["wp"] = 1
            j["weight"], j["offset"], j["wp_round"], j["wp_denom"] = case.wp
        jobs.append(j)
    return jobs


def bi_jobs(case):
    """-> the jobs as dicts with the fields of jmhip_bipred_surface_job"""
    jobs = []
    for mx, my, slot1, slot2, smv, cx, cy in case.jobs:
        j = dict(mb_x=mx, mb_y=my, ref1=slot1, ref2=slot2, s_mv=smv, R=case.R, cx=cx, cy=cy, wp=0, weight1=0, weight2=0, offset_bi=0,
                 wp_round=0, wp_denom=0, pad=0)
        if case.wp:
            j["wp"] = 1
            j["weight1"], j["weight2"], j["offset_bi"], j["wp_round"], j["wp_denom"] = case.wp
        jobs.append(j)
    return jobs


def job_array(dtype, jobs):
    """the dicts as a numpy array of the binding's job dtype"""
    out = np.zeros(len(jobs), dtype=dtype)
    for i, j in enumerate(jobs):
        for k, v in j.items():
            out[i][k] = v
    return out


def distinct_samples(lo, n, size):
    """how many different picture coordinates the n window coordinates from lo on clamp to"""
    return len(np.unique(np.clip(np.arange(lo, lo + n), 0, size - 1)))


def window_varies(case, job):
    """the swept window of the job sees more than one sample of its picture (a window that is clamped throughout shows a single one)"""
    w, h = case.size
    R, n = job["R"], 2 * job["R"] + 16
    return distinct_samples(16 * job["mb_x"] + job["cx"] - R, n, w) > 1 and distinct_samples(16 * job["mb_y"] + job["cy"] - R, n, h) > 1


def fixed_varies(case, job):
    """the same of the fixed block of a bi-predictive job"""
    w, h = case.size
    return distinct_samples(16 * job["mb_x"] + job["s_mv"][0], 16, w) > 1 and distinct_samples(16 * job["mb_y"] + job["s_mv"][1], 16, h) > 1
