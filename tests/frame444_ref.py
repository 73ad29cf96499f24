"""Expectation for the 4:4:4 frame stage (jmhip_residual_frame in a JMHIP_YUV444 context), assembled from the oracle's wrappers only:
oracle.interp_luma on Y, Cb and Cr of every reference (UnifiedOneForthPix runs getSubImagesLuma per plane, image.c:1647-1656), the prediction
arithmetic of oracle.residual_frame's luma branch per plane (block-origin clamp, explicit weights per component), oracle.tq_reference
("luma4x4" / "luma8x8") with the plane's quantiser, and LumaResidualCoding8x8 / LumaResidualCoding's per-plane bookkeeping restated from
lencod/src/macroblock.c:1009-1449: _LUMA_COEFF_COST_ per 8x8 block (:1236-1290), _LUMA_MB_COEFF_COST_ per plane (:1386-1444), the zeroing of
the Cb / Cr coefficient lists of what a threshold clears (:1268-1270, :1283-1285, :1426-1429, :1440-1443; not for Y), cbp |= cmp_cbp[0..1] (:1446)."""
import numpy as np

from tests import oracle

LUMA_COEFF_COST, LUMA_MB_COEFF_COST = 4, 5


class Ref444:
    """The three 6-tap plane stacks of one 4:4:4 reference picture."""

    def __init__(self, Y, U, V):
        self.planes = [oracle.interp_luma(p) for p in (Y, U, V)]
        self.H, self.W = Y.shape


def synth444(rng, w, h, nrefs=1):
    """A current picture and its references: three planes with textures of their own, all moved by the same translation."""
    yy, xx = np.mgrid[0:h + 32, 0:w + 32]
    waves = (np.sin(xx / 6.0) * np.cos(yy / 9.0) * 70, np.cos(xx / 4.0 + yy / 7.0) * 45, np.sin(xx / 9.0 - yy / 5.0) * 28)
    bases = [(wv + 128 + rng.normal(0, s, (h + 32, w + 32))).clip(0, 255) for wv, s in zip(waves, (10, 7, 4))]
    refs = [tuple(b[16:16 + h, 16:16 + w].astype(np.uint8) for b in bases)]
    for k in range(1, nrefs):                               # further references: the first one shifted and dimmed
        refs.append(tuple(np.clip(np.roll(p, (k, -2 * k), (0, 1)).astype(int) - 6 * k, 0, 255).astype(np.uint8) for p in refs[0]))
    cur = tuple((b[13:13 + h, 21:21 + w] + rng.normal(0, s, (h, w))).clip(0, 255).astype(np.uint8) for b, s in zip(bases, (2, 2, 1.5)))
    return cur, refs


def _weigh(v, wp, slot, comp):
    if wp is None:
        return v
    rnd, den = (wp["luma_round"], wp["luma_denom"]) if comp == 0 else (wp["chroma_round"], wp["chroma_denom"])      # ChromaPrediction, macroblock.c:1784-1791
    return np.clip(((int(wp["weight"][slot][comp]) * v.astype(np.int64) + rnd) >> den) + int(wp["offset"][slot][comp]), 0, 255)


def _first_zero(levels):
    z = np.flatnonzero(levels == 0)
    return int(z[0]) if len(z) else len(levels)


def residual_frame444(pkg, refs, cur, mbs, mv, modes, quants, wp=None):
    """refs: list indexed by reference SLOT of Ref444 (None where unused); cur = (Y, U, V); mv (n, 41, 2) quarter-pel; quants: 3 or 6 QUANT_DTYPE records.
    Returns per-plane oracle results ("planes": list of tq dicts after the Cb / Cr list zeroing), the pictures, the coded bits and the records."""
    n = len(mbs)
    H, W = cur[0].shape
    Wp, Hp = W + 40, H + 40
    t8 = np.array([int(m["pad"][0]) for m in modes], bool)
    out = {"planes": [], "pred": [], "recon": [np.zeros((H, W), np.uint8) for _ in range(3)], "predpic": [np.zeros((H, W), np.uint8) for _ in range(3)],
           "plane_cbp": np.zeros((n, 3), np.int32), "plane_cbp_blk": np.zeros((n, 3), np.int32), "cleared8": np.zeros((n, 3), np.uint8),
           "cleared_mb": np.zeros((n, 3), np.uint8), "nonzero_before": [], "t8": t8}
    for pl in range(3):
        jobs = np.zeros(n, dtype=pkg.TQ_JOB_DTYPE)
        jobs["quant"] = pl
        for i, mb in enumerate(mbs):
            mbx, mby, slot = int(mb["mb_x"]), int(mb["mb_y"]), int(mb["ref"])
            stack = refs[slot].planes[pl]
            for y4 in range(4):
                for x4 in range(4):
                    p = oracle.covering_partition(modes[i], x4, y4)
                    # with the 8x8 transform the prediction runs per 8x8 block (macroblock.c:1143-1150): its origin is what UMVLine4X clamps
                    ox4, oy4 = ((x4 & 1) * 4, (y4 & 1) * 4) if t8[i] else (0, 0)
                    xq = ((mbx * 16 + 4 * x4 - ox4) << 2) + 80 + int(mv[i, p, 0])
                    yq = ((mby * 16 + 4 * y4 - oy4) << 2) + 80 + int(mv[i, p, 1])
                    xpos = min(max(xq >> 2, 0), Wp - 17) + ox4
                    ypos = min(max(yq >> 2, 0), Hp - 17) + oy4
                    v0 = stack[yq & 3, xq & 3, ypos:ypos + 4, xpos:xpos + 4]
                    jobs[i]["pred"][4 * y4:4 * y4 + 4, 4 * x4:4 * x4 + 4] = _weigh(v0, wp, slot, pl)
            jobs[i]["src"] = cur[pl][mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16]
        r = oracle.tq_reference("luma4x4", quants, jobs)
        if t8.any():
            jobs8 = jobs.copy()
            jobs8["quant"] = 3 + pl
            r8 = oracle.tq_reference("luma8x8", quants, jobs8)
            for k in r:
                r[k][t8] = r8[k][t8]
        out["nonzero_before"].append(r["nonzero"].copy())
        for i, mb in enumerate(mbs):
            mbx, mby = int(mb["mb_x"]), int(mb["mb_y"])
            c, cb, total, gone = 0, 0, 0, 0
            rec = r["recon"][i].copy()
            pred = jobs[i]["pred"]
            for b8 in range(4):
                mask = 51 << (4 * b8 - 2 * (b8 & 1))
                if t8[i]:                                       # :1185-1209
                    cost = int(r["coeff_cost"][i, b8])
                    if r["nonzero"][i, b8]:
                        c |= 1 << b8
                        cb |= mask
                else:                                           # :1093-1124
                    cost = int(r["coeff_cost"][i, 4 * b8:4 * b8 + 4].sum())
                    for b4 in range(4):
                        if r["nonzero"][i, 4 * b8 + b4]:
                            c |= 1 << b8
                            cb |= 1 << ((2 * (b8 & 1) + (b4 & 1)) + 4 * (2 * (b8 >> 1) + (b4 >> 1)))
                if cost <= LUMA_COEFF_COST:                    # :1236-1290
                    cost = 0
                    gone |= 1 << b8
                    c &= 63 - (1 << b8)
                    cb &= ~mask
                    ys, xs = 8 * (b8 >> 1), 8 * (b8 & 1)
                    rec[ys:ys + 8, xs:xs + 8] = pred[ys:ys + 8, xs:xs + 8]
                    if pl:                                      # memset(img->cofAC[block8x8 + 4 (+ 4)] ...): Cb / Cr only
                        for k in ("levels", "runs"):
                            r[k][i, 4 * b8:4 * b8 + 4] = 0
                            r[k + "8"][i, b8] = 0
                total += cost
            mb_gone = total <= LUMA_MB_COEFF_COST              # :1386-1444
            if mb_gone:
                c &= 0xfffff0
                cb &= 0xff0000
                rec = pred.copy()
                if pl:
                    for k in ("levels", "runs", "levels8", "runs8"):
                        r[k][i] = 0
            out["plane_cbp"][i, pl], out["plane_cbp_blk"][i, pl], out["cleared8"][i, pl], out["cleared_mb"][i, pl] = c, cb, gone, mb_gone
            out["recon"][pl][mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16] = rec
            out["predpic"][pl][mby * 16:mby * 16 + 16, mbx * 16:mbx * 16 + 16] = pred
        out["planes"].append(r)
        out["pred"].append(jobs["pred"].copy())
    out["cbp"] = out["plane_cbp"][:, 0] | out["plane_cbp"][:, 1] | out["plane_cbp"][:, 2]          # :1446-1447
    out["cbp_blk"] = out["plane_cbp_blk"][:, 0].astype(np.int64)
    out["records"], out["records8"] = _records(pkg, out, quants, n)
    return out


def _records(pkg, out, quants, n):
    """jmhip_mb_residual444 and the (n, 3) jmhip_mb_residual8 side records the stage must leave, every byte."""
    rec = np.zeros(n, pkg.MB_RESIDUAL444_DTYPE)
    rec8 = np.zeros((n, 3), pkg.MB_RESIDUAL8_DTYPE)
    t8 = out["t8"]
    for pl in range(3):
        r = out["planes"][pl]
        for i in range(n):
            rec[i]["recon"][pl] = r["recon"][i]
            if quants[3 + pl if t8[i] else pl]["adaptive_rounding"]:
                rec[i]["fadj"][pl] = r["fadjust"][i]
            if not t8[i]:
                for b in range(16):
                    k = _first_zero(r["levels"][i, b])
                    rec[i]["lev"][pl, b, :k], rec[i]["run"][pl, b, :k], rec[i]["cnt"][pl, b] = r["levels"][i, b, :k], r["runs"][i, b, :k], k
                rec[i]["coeff_cost"][pl] = r["coeff_cost"][i]
                rec[i]["nonzero"][pl] = sum(1 << b for b in range(16) if out["nonzero_before"][pl][i, b])
                continue
            s = rec8[i, pl]
            s["transform8x8"], s["interleaved"] = 1, int(quants[3 + pl]["cavlc"] != 0)
            for b8 in range(4):
                if s["interleaved"]:
                    for q in range(4):
                        k = _first_zero(r["levels"][i, 4 * b8 + q])
                        s["lev"][b8, 16 * q:16 * q + k], s["run"][b8, 16 * q:16 * q + k], s["cnt"][b8, q] = r["levels"][i, 4 * b8 + q, :k], r["runs"][i, 4 * b8 + q, :k], k
                else:
                    k = _first_zero(r["levels8"][i, b8])
                    s["lev"][b8, :k], s["run"][b8, :k], s["cnt"][b8, 0] = r["levels8"][i, b8, :k], r["runs8"][i, b8, :k], k
                s["coeff_cost"][b8], s["nonzero"][b8] = r["coeff_cost"][i, b8], out["nonzero_before"][pl][i, b8]
    rec["cleared8"], rec["cleared_mb"], rec["plane_cbp"], rec["plane_cbp_blk"], rec["cbp"] = out["cleared8"], out["cleared_mb"], out["plane_cbp"], out["plane_cbp_blk"], out["cbp"]
    return rec, rec8
