"""Lagrangian factors that tell the three levels apart, and pictures on which their magnitude decides.

Every search entry takes lambda[F_PEL, H_PEL, Q_PEL] (lambda_mf[] in the slice search). For JM's default metrics the three are equal, and
lambda_factors() of tests/test_me.py returns them so: a kernel that read the integer factor at the quarter-pel level, exchanged two levels or
took the skip bonus from the wrong one computes the same. LAMBDA_SETS["split"] / ["split_rev"] are three different values; mutated() applies
the ways of getting the triple wrong, and tests/test_lambda_levels.py shows on the oracle that each of them changes a compared output before
a device result is compared (the method of tests/quant_tables.py).

"split_rev" is "split" in the opposite order: the integer and the quarter-pel level are once the largest and once the smallest of the three.
The half-pel level keeps the middle value in both; what separates it from its neighbours are the mutations "F<->H" and "H<->Q", which must
bite in both sets.

The bounds are the package's (h.264_amd/jmhip.py, JMHIP_LAMBDA_MAX_* of include/jmhip.h)."""
import numpy as np

from tests.conftest import load_pkg
from tests.test_me import lambda_factors, make_pair

_pkg = load_pkg()
BOUNDS = {"me_frame": _pkg.LAMBDA_MAX_ME_FRAME, "me_subpel": _pkg.LAMBDA_MAX_ME_SUBPEL, "bipred": _pkg.LAMBDA_MAX_BIPRED,
          "slice": _pkg.LAMBDA_MAX_SLICE}

_SPLIT = [lambda_factors(qp)[0] for qp in (22, 30, 38)]
LAMBDA_SETS = {
    "split": list(_SPLIT),
    "split_rev": list(reversed(_SPLIT)),
    "jm_min": lambda_factors(0),           # JM's P-slice factors at QP 0 and QP 51 (RDOptimization on)
    "jm_max": lambda_factors(51),
    "bound": {entry: [b, b, b] for entry, b in BOUNDS.items()},
}

MUTATIONS = ("all=F", "all=Q", "F<->H", "H<->Q")
INTEGER_MUTATIONS = ("all=Q", "F<->H")     # change lambda[F_PEL]: the integer stage must notice
SUBPEL_MUTATIONS = ("all=F", "H<->Q")      # leave lambda[F_PEL] alone: only the refinement (and what else reads H_PEL / Q_PEL) can notice


def lambdas(name, entry):
    """LAMBDA_SETS[name] for the entry point `entry` ("me_frame", "me_subpel", "bipred", "slice")."""
    s = LAMBDA_SETS[name]
    return list(s[entry] if isinstance(s, dict) else s)


def mutated(lam, how):
    f, h, q = lam
    return {"all=F": [f, f, f], "all=Q": [q, q, q], "F<->H": [h, f, q], "H<->Q": [f, q, h]}[how]


def saturated_pair(rng, w, h):
    """(cur, ref): in the left half of the macroblock columns cur = 255 and ref = 0 -- every 16x16 candidate whose block stays in that half (or
    left of the picture: the padding repeats the 0) has SAD 65280, every 16x8 / 8x16 candidate 32640, so motion cost and spiral order alone
    decide, and a cost field one bit too narrow wraps and picks another vector. The right half is the "shift" clip of make_pair."""
    cur, ref = make_pair(rng, w, h, "shift")
    half = (w // 16 // 2) * 16
    cur[:, :half] = 255
    ref[:, :half] = 0
    return cur, ref


def mvbits(d):
    """mvbits[d] of mv-search.c:333-341"""
    d = abs(int(d))
    return 1 if d == 0 else 2 * (d.bit_length() - 1) + 3


def largest_mv_product(lam, preds, reach):
    """The largest lambda * (mvbits(dx) + mvbits(dy)) a search can form: candidates up to `reach` quarter-pels from zero in either
    direction, against the predictors `preds` (quarter-pel pairs). The oracle, like JM's WEIGHTED_COST, forms it in an int."""
    worst = 0
    for px, py in np.asarray(preds).reshape(-1, 2):
        worst = max(worst, max(mvbits(reach - px), mvbits(-reach - px)) + max(mvbits(reach - py), mvbits(-reach - py)))
    return int(lam) * worst
