"""dct_4x4 / dct_8x8 / dct_16x16 / dct_chroma: jmhip_tq_batch vs the oracle, bit-exact on levels, runs (up to the
terminating zero level), reconstruction, coefficient cost, nonzero flags, adaptive-rounding residues, return values."""
import numpy as np
import pytest

from tests import oracle


def make_jobs(pkg, rng, n, nq, amp, chroma=False):
    jobs = np.zeros(n, dtype=pkg.TQ_JOB_DTYPE)
    pred = rng.integers(0, 256, (n, 16, 16))
    resid = np.round(rng.normal(0, amp, (n, 16, 16))).astype(int)
    # a few blocks with zero residual, a few with saturating recon
    resid[::7] = 0
    jobs["pred"] = pred
    jobs["src"] = np.clip(pred + resid, 0, 255)
    jobs["quant"] = rng.integers(0, nq, n)
    jobs["quant_dc"] = jobs["quant"]
    if chroma:
        jobs["uv"] = rng.integers(0, 2, n)
        jobs["cr_cbp_in"] = rng.integers(0, 3, n)
    return jobs


def compare_lists(got_lev, got_run, want_lev, want_run, what):
    """(level, run) lists are compared up to and including the terminating zero level."""
    g, w = got_lev.reshape(-1, got_lev.shape[-1]), want_lev.reshape(-1, want_lev.shape[-1])
    gr, wr = got_run.reshape(g.shape), want_run.reshape(w.shape)
    for r in range(g.shape[0]):
        nz = np.flatnonzero(w[r] == 0)
        k = nz[0] if len(nz) else w.shape[1] - 1
        assert np.array_equal(g[r, :k + 1], w[r, :k + 1]), "%s levels row %d: %s vs %s" % (what, r, g[r, :k + 2], w[r, :k + 2])
        assert np.array_equal(gr[r, :k], wr[r, :k]), "%s runs row %d" % (what, r)


def quant_set(pkg, qps, offset11, is8x8=False, **kw):
    return np.array([pkg.flat_quant(qp, offset11, is8x8, **kw) for qp in qps], dtype=pkg.QUANT_DTYPE)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(64, 48, yuv_format=1)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field_scan,adaptive,amp", [(0, 1, 6), (1, 0, 20), (0, 0, 60), (0, 1, 1)])
def test_dct_4x4(pkg, ctx, field_scan, adaptive, amp):
    rng = np.random.default_rng(amp + field_scan)
    quants = quant_set(pkg, [4, 17, 28, 36, 51], 342, adaptive_rounding=adaptive, adapt_rnd_weight=4, field_scan=field_scan, cavlc=1)
    jobs = make_jobs(pkg, rng, 300, len(quants), amp)
    got = ctx.tq_batch("luma4x4", quants, jobs)
    want = oracle.tq_reference("luma4x4", quants, jobs)
    compare_lists(got["levels"], got["runs"], want["levels"], want["runs"], "dct_4x4")
    for k in ("recon", "coeff_cost", "nonzero"):
        assert np.array_equal(got[k], want[k]), k
    if adaptive:
        assert np.array_equal(got["fadjust"], want["fadjust"])


@pytest.mark.gpu
@pytest.mark.parametrize("cavlc,flag,field_scan,adaptive", [(1, 1, 0, 1), (0, 1, 0, 0), (1, 0, 1, 1), (0, 1, 1, 1)])
def test_dct_8x8(pkg, ctx, cavlc, flag, field_scan, adaptive):
    rng = np.random.default_rng(cavlc * 8 + flag * 4 + field_scan)
    quants = quant_set(pkg, [6, 20, 28, 40], 342, True, adaptive_rounding=adaptive, adapt_rnd_weight=4, field_scan=field_scan,
                       cavlc=cavlc, transform8x8_flag=flag)
    jobs = make_jobs(pkg, rng, 200, len(quants), 15)
    got = ctx.tq_batch("luma8x8", quants, jobs)
    want = oracle.tq_reference("luma8x8", quants, jobs)
    if cavlc and flag:
        compare_lists(got["levels"], got["runs"], want["levels"], want["runs"], "dct_8x8 interleaved")
    else:
        compare_lists(got["levels8"], got["runs8"], want["levels8"], want["runs8"], "dct_8x8")
    for k in ("recon",):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["coeff_cost"][:, :4], want["coeff_cost"][:, :4])
    assert np.array_equal(got["nonzero"][:, :4], want["nonzero"][:, :4])
    if adaptive:
        assert np.array_equal(got["fadjust"], want["fadjust"])


@pytest.mark.gpu
@pytest.mark.parametrize("qps,cavlc,amp", [([5, 8, 28, 44], 1, 25), ([20, 30], 0, 8)])
def test_dct_16x16(pkg, ctx, qps, cavlc, amp):
    rng = np.random.default_rng(sum(qps))
    quants = quant_set(pkg, qps, 682, adaptive_rounding=1, adapt_rnd_weight=4, cavlc=cavlc)
    jobs = make_jobs(pkg, rng, 150, len(quants), amp)
    got = ctx.tq_batch("luma16x16", quants, jobs)
    want = oracle.tq_reference("luma16x16", quants, jobs)
    compare_lists(got["dc_levels"][:, None, :], got["dc_runs"][:, None, :], want["dc_levels"][:, None, :], want["dc_runs"][:, None, :], "dct_16x16 DC")
    compare_lists(got["levels"][:, :, :16], got["runs"][:, :, :16], want["levels"][:, :, :16], want["runs"][:, :, :16], "dct_16x16 AC")
    for k in ("recon", "ret", "fadjust"):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,amp", [(1, 10), (1, 2), (2, 10), (2, 2)])
def test_dct_chroma(pkg, ctx, fmt, amp):
    rng = np.random.default_rng(fmt * 100 + amp)
    qps = [3, 12, 24, 33, 39]
    quants = np.concatenate([quant_set(pkg, qps, 342, adaptive_rounding=1, adapt_rnd_weight=4, cavlc=1),
                             quant_set(pkg, [q + 3 for q in qps], 342, adaptive_rounding=1, adapt_rnd_weight=4, cavlc=1)])
    quants["img_qp"] = np.concatenate([qps, qps])
    jobs = make_jobs(pkg, rng, 300, len(qps), amp, chroma=True)
    jobs["quant_dc"] = jobs["quant"] + len(qps)      # the 4:2:2 DC quantiser is the qp+3 table set
    got = ctx.tq_batch("chroma", quants, jobs, yuv_format=fmt)
    want = oracle.tq_reference("chroma", quants, jobs, yuv_format=fmt)
    nblk = 4 if fmt == 1 else 8
    rows, cols = (8, 8) if fmt == 1 else (16, 8)
    compare_lists(got["dc_levels"][:, None, :], got["dc_runs"][:, None, :], want["dc_levels"][:, None, :], want["dc_runs"][:, None, :], "dct_chroma DC")
    compare_lists(got["levels"][:, :nblk, :16], got["runs"][:, :nblk, :16], want["levels"][:, :nblk, :16], want["runs"][:, :nblk, :16], "dct_chroma AC")
    assert np.array_equal(got["recon"][:, :rows, :cols], want["recon"][:, :rows, :cols])
    assert np.array_equal(got["ret"], want["ret"])
    assert np.array_equal(got["fadjust"][:, :rows, :cols], want["fadjust"][:, :rows, :cols])
    assert np.array_equal(got["cbp_blk"], want["cbp_blk"] & ~want["cbp_clear"])
    assert np.array_equal(got["cbp_clear"], want["cbp_clear"])


@pytest.mark.gpu
def test_flat_tables_match_oracle(pkg):
    for qp in (0, 7, 28, 51):
        for is8 in (False, True):
            q = pkg.flat_quant(qp, 342, is8)
            ls, ils, lo, n = oracle.flat_tables(qp, 342, is8)
            assert np.array_equal(q["levelscale"][:n], ls[:n]) and np.array_equal(q["invlevelscale"][:n], ils[:n])
            assert np.array_equal(q["leveloffset"][:n], lo[:n])


# ------------------------------------------------------------------ position-dependent, asymmetric tables (tests/quant_tables.py)

AR = dict(adaptive_rounding=1, adapt_rnd_weight=4)
TABLE_CASES = {
    "luma4x4_ar": dict(kind="luma4x4", qps=[4, 17, 28, 36, 45], n=300, amp=12, cavlc=1, **AR),
    "luma4x4_field": dict(kind="luma4x4", qps=[10, 22, 31], n=200, amp=25, cavlc=0, field_scan=1),
    "luma8x8_interleaved_ar": dict(kind="luma8x8", qps=[6, 20, 28, 40], n=200, amp=15, cavlc=1, transform8x8_flag=1, **AR),
    "luma8x8_lists64": dict(kind="luma8x8", qps=[12, 26, 33], n=200, amp=15, cavlc=0, transform8x8_flag=1),
    "luma8x8_lists64_field_ar": dict(kind="luma8x8", qps=[18, 30], n=200, amp=10, cavlc=0, transform8x8_flag=1, field_scan=1, **AR),
    "luma16x16_ar": dict(kind="luma16x16", qps=[5, 8, 28, 44], n=200, amp=25, cavlc=1, **AR),
    "luma16x16": dict(kind="luma16x16", qps=[20, 30], n=200, amp=8, cavlc=0),
    "chroma420_ar": dict(kind="chroma", fmt=1, qps=[3, 12, 24, 33, 39], n=300, amp=10, cavlc=1, **AR),
    "chroma420": dict(kind="chroma", fmt=1, qps=[16, 27], n=200, amp=6, cavlc=1),
    "chroma422_ar": dict(kind="chroma", fmt=2, qps=[3, 12, 24, 33, 39], n=300, amp=10, cavlc=1, **AR),
    "chroma422": dict(kind="chroma", fmt=2, qps=[9, 21, 30], n=200, amp=6, cavlc=0),
}


def table_case(pkg, name):
    """quants, jobs, groups of a TABLE_CASES entry, drawn on the host. groups: {name: (record indices, is a DC-only set)}. Chroma: the Cb jobs
    use records [0, n), the Cr jobs [n, 2n), and their DC quantisers (the qp + 3 sets, read by the 4:2:2 DC path alone) [2n, 3n) and [3n, 4n):
    four families of tables, no two alike."""
    from tests.quant_tables import scaled_quant
    kw = dict(TABLE_CASES[name])
    kind, qps, n, amp, fmt = kw.pop("kind"), kw.pop("qps"), kw.pop("n"), kw.pop("amp"), kw.pop("fmt", 1)
    rng = np.random.default_rng(7000 + sorted(TABLE_CASES).index(name))
    is8 = kind == "luma8x8"
    nq = len(qps)
    if kind != "chroma":
        quants = np.array([scaled_quant(pkg, qp, rng, is8, **kw) for qp in qps], dtype=pkg.QUANT_DTYPE)
        jobs = make_jobs(pkg, rng, n, nq, amp)
        return kind, fmt, quants, jobs, {"all": (list(range(nq)), False)}
    quants = np.array([scaled_quant(pkg, qp + d, rng, False, **kw) for d in (0, 0, 3, 3) for qp in qps], dtype=pkg.QUANT_DTYPE)
    quants["img_qp"] = qps * 4
    jobs = make_jobs(pkg, rng, n, nq, amp, chroma=True)
    jobs["quant"] += nq * jobs["uv"]
    jobs["quant_dc"] = jobs["quant"] + 2 * nq
    groups = {"cb": (list(range(nq)), False), "cr": (list(range(nq, 2 * nq)), False)}
    if fmt == 2:
        groups["cb_dc"], groups["cr_dc"] = (list(range(2 * nq, 3 * nq)), True), (list(range(3 * nq, 4 * nq)), True)
    return kind, fmt, quants, jobs, groups


def tq_differences(kind, fmt, got, want, adaptive):
    """The comparisons of test_dct_* as a list of the names that differ (empty: equal); got is the device's result or a second oracle run."""
    bad = []

    def lists(name, *a):
        try:
            compare_lists(*a, name)
        except AssertionError:
            bad.append(name)

    def same(name, a, b):
        if not np.array_equal(a, b):
            bad.append(name)
    if kind == "luma4x4":
        lists("levels", got["levels"], got["runs"], want["levels"], want["runs"])
        for k in ("recon", "coeff_cost", "nonzero"):
            same(k, got[k], want[k])
    elif kind == "luma8x8":
        lists("levels", got["levels"], got["runs"], want["levels"], want["runs"])
        lists("levels", got["levels8"], got["runs8"], want["levels8"], want["runs8"])
        same("recon", got["recon"], want["recon"])
        for k in ("coeff_cost", "nonzero"):
            same(k, got[k][:, :4], want[k][:, :4])
    elif kind == "luma16x16":
        lists("dc_levels", got["dc_levels"][:, None, :], got["dc_runs"][:, None, :], want["dc_levels"][:, None, :], want["dc_runs"][:, None, :])
        lists("levels", got["levels"][:, :, :16], got["runs"][:, :, :16], want["levels"][:, :, :16], want["runs"][:, :, :16])
        for k in ("recon", "ret"):
            same(k, got[k], want[k])
    else:
        nblk = 4 if fmt == 1 else 8
        rows, cols = (8, 8) if fmt == 1 else (16, 8)
        lists("dc_levels", got["dc_levels"][:, None, :], got["dc_runs"][:, None, :], want["dc_levels"][:, None, :], want["dc_runs"][:, None, :])
        lists("levels", got["levels"][:, :nblk, :16], got["runs"][:, :nblk, :16], want["levels"][:, :nblk, :16], want["runs"][:, :nblk, :16])
        same("recon", got["recon"][:, :rows, :cols], want["recon"][:, :rows, :cols])
        same("ret", got["ret"], want["ret"])
        same("cbp_blk", got["cbp_blk"], want["cbp_blk"] & ~want["cbp_clear"])
        same("cbp_clear", got["cbp_clear"], want["cbp_clear"])
    if adaptive:
        rows, cols = (16, 16) if kind != "chroma" else ((8, 8) if fmt == 1 else (16, 8))
        same("fadjust", got["fadjust"][:, :rows, :cols], want["fadjust"][:, :rows, :cols])
    return bad


def assert_tables_bite(differ, groups, what):
    """The condition on the inputs that makes a passing comparison mean something: every way of getting a table wrong (quant_tables.MUTATIONS)
    changes a compared output of the oracle. differ(ks, how) -> names of the compared outputs that change when the records ks are mutated."""
    from tests.quant_tables import MUTATIONS
    for gname, (ks, dc_only) in groups.items():
        for how in MUTATIONS:
            if dc_only and how != "leveloffset=mean":
                continue                                    # a DC-only set is read at (0, 0): transposing it is no change at all
            bad = differ(ks, how)
            assert bad, "%s: %s of the %s records changes nothing that is compared" % (what, how, gname)
            if how.startswith("leveloffset"):
                assert any("levels" in b for b in bad), "%s: %s of %s leaves every level in place (%s)" % (what, how, gname, bad)
            if how == "invlevelscale^T":
                assert any("recon" in b for b in bad), "%s: %s of %s leaves the reconstruction in place (%s)" % (what, how, gname, bad)


_table_refs = {}


def table_reference(pkg, name):
    """The oracle's result of a TABLE_CASES entry, checked once for the tables to bite and then shared (read-only) by the tests that need it."""
    if name not in _table_refs:
        from tests.quant_tables import is_asymmetric, mutated
        kind, fmt, quants, jobs, groups = table_case(pkg, name)
        n = 64 if kind == "luma8x8" else 16
        assert all(is_asymmetric(q[t], 8 if n == 64 else 4) for q in quants for t in ("levelscale", "invlevelscale", "leveloffset"))
        assert len({q[t][:n].tobytes() for q in quants for t in ("levelscale", "leveloffset")}) == 2 * len(quants), "two records share a table"
        want = oracle.tq_reference(kind, quants, jobs, yuv_format=fmt)
        for v in want.values():
            v.setflags(write=False)
        ar = int(quants[0]["adaptive_rounding"])
        if kind == "chroma":                                # as test_dct_chroma compares: the oracle's set bits less its cleared bits
            straight = dict(want, cbp_blk=want["cbp_blk"] & ~want["cbp_clear"])
        else:
            straight = want
        assert_tables_bite(lambda ks, how: tq_differences(kind, fmt, straight, oracle.tq_reference(kind, mutated(quants, ks, how), jobs, yuv_format=fmt), ar),
                           groups, name)
        _table_refs[name] = (kind, fmt, quants, jobs, want, ar)
    return _table_refs[name]


@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_tables_are_asymmetric_where_it_matters(pkg, name):
    """No GPU. Every table of every record differs from its transpose and from every other record's, and on the oracle a transposed
    levelscale, invlevelscale or leveloffset, or a leveloffset flattened to its mean, changes what test_tq_batch_asymmetric_tables compares
    (offsets: the levels; invlevelscale: the reconstruction), per family of records -- Cb, Cr and, in 4:2:2, their qp + 3 DC sets."""
    table_reference(pkg, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_tq_batch_asymmetric_tables(pkg, ctx, name):
    """jmhip_tq_batch on scaling matrices and rounding offsets that depend on (j, i) and are not symmetric: the fields the flat tests compare."""
    kind, fmt, quants, jobs, want, ar = table_reference(pkg, name)        # asserts that the tables bite before anything is compared
    got = ctx.tq_batch(kind, quants, jobs, yuv_format=fmt)
    assert tq_differences(kind, fmt, got, want, ar) == []
