"""Quantiser records whose tables depend on the position and change when row and column are swapped.

jmhip_flat_quant's tables come from JM's position classes, which are symmetric in (j, i), and carry one rounding offset for all positions: an
index written i*4+j for j*4+i, a table folded to its classes or an offset broadcast over the block would leave them -- and every result
computed from them -- unchanged. scaled_quant draws what a QmatrixFile / QOffsetMatrixFile gives JM instead; mutated() applies the ways of
getting such a table wrong that the tests show to bite (on the oracle, before a device result is compared).

Which entries a record's user reads: the AC loops read [j][i] of all three tables; every DC path (dct_16x16, dct_chroma, the 4:2:2 DC with
its qp + 3 set) reads position (0, 0) alone (block.c:643, :1143, :1263), which a transposition leaves in place. A DC-only table set can
therefore show the broadcast offset and nothing else."""
import numpy as np


def _asymmetric(rng, lo, hi, n):
    """An n x n draw from lo..hi-1 that differs from its transpose (a symmetric draw is redrawn: 1 in 35^6 for 4x4 at the least)."""
    while True:
        m = rng.integers(lo, hi, n * n)
        if not np.array_equal(m.reshape(n, n), m.reshape(n, n).T):
            return m


def scaled_quant(pkg, qp, rng, is8x8, offsets=True, **fields):
    """pkg.flat_quant with a scaling matrix M[j][i] drawn from 6..40, M != M.T: LevelScale = (quant_coef << 4) / M, InvLevelScale = dequant_coef * M
    (q_matrix.c CalculateQuantParam / CalculateQuant8Param; the flat tables, M = 16, give quant_coef and dequant_coef << 4). offsets: an 11-bit
    rounding offset per position from 171..853 (1/12 .. 5/12 of a step), O != O.T, shifted as q_offsets.c does."""
    n = 8 if is8x8 else 4
    q = pkg.flat_quant(qp, 342, is8x8, **fields)
    m = _asymmetric(rng, 6, 41, n)
    q["levelscale"][:n * n] = (q["levelscale"][:n * n] * 16) // m
    q["invlevelscale"][:n * n] = (q["invlevelscale"][:n * n] // 16) * m
    if offsets:
        o = _asymmetric(rng, 171, 854, n)
        q["leveloffset"][:n * n] = o << ((16 if is8x8 else 15) + qp // 6 - 11)
    return q


def is_asymmetric(table, n):
    t = np.asarray(table)[:n * n].reshape(n, n)
    return not np.array_equal(t, t.T)


def table_size(q):
    """4 or 8: the 8x8 records are the ones that say transform8x8_flag (every maker in the tests sets it for them and for no other)."""
    return 8 if int(q["transform8x8_flag"]) else 4


MUTATIONS = ("levelscale^T", "invlevelscale^T", "leveloffset^T", "leveloffset=mean")


def mutated(quants, ks, how):
    """A copy of the record array with one table of the records ks transposed, or their offsets replaced by their mean."""
    out = np.array(quants, copy=True)
    name = how.split("^")[0].split("=")[0]
    for k in ks:
        n = table_size(out[k])
        t = out[k][name][:n * n].reshape(n, n)
        out[k][name][:n * n] = (t.T if how.endswith("^T") else np.full((n, n), int(t.mean()))).reshape(-1)
    return out
