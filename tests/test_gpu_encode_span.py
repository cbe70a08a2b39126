"""GPU: the row-filtered encode on every route, with the repair as the probe.

With every original present and one run [lo, hi) of recovery rows missing, rs_repair_device* runs
the encode with its destination map narrowed to the run, straight into the caller's
d_recovery_out.  Each case of tests/span_cases.py (one per encode route) is run over every span of
spans(): rows [lo, hi) of d_recovery_out must equal the CPU oracle's encode byte for byte, and
every other byte -- the other rows, the margins around the matrix, the row padding, all of
d_restored -- must still hold the poison it was filled with; d_original and d_recovery (junk in
its absent rows) must be unchanged.  The launch names are checked against the kernel family the
case is built to reach, so a case that silently ran on another route fails.
"""
import numpy as np
import pytest

import span_cases as SC

pytestmark = pytest.mark.gpu

RATE = {"high": 1, "low": 2}
POISON = SC.POISON


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def rs(torch):
    import reed_solomon_simd
    yield reed_solomon_simd
    reed_solomon_simd.mono_enable(1)


class Wide:
    """A [rows, S] view of a wider buffer filled with `fill`: `margin` bytes to the left of every
    row, the row padding and `margin` bytes to its right, the base `off` bytes into the buffer
    (off = 1: an address of 3 mod 4, the byte-wise path; otherwise the margins keep 4-byte
    alignment wherever S + pad does)."""

    def __init__(self, torch, rows, S, pad, fill, off=0):
        self.rows, self.S, self.off, self.fill = rows, S, off, fill
        self.margin = 6 if off else 8
        self.W = S + pad + 2 * self.margin
        self.buf = torch.full((off + rows * self.W + 8,), fill, dtype=torch.uint8, device="cuda")
        self.view = self.buf[off:off + rows * self.W].view(rows, self.W)[:, self.margin:self.margin + S]

    def host(self):
        return self.buf.cpu().numpy()

    def matrix(self, h):
        return h[self.off:self.off + self.rows * self.W].reshape(self.rows, self.W)[:, self.margin:self.margin + self.S]

    def check_outside(self, h, what):
        """Everything but the matrix itself still holds the fill byte."""
        body = h[self.off:self.off + self.rows * self.W].reshape(self.rows, self.W)
        assert (h[:self.off] == self.fill).all() and (h[self.off + self.rows * self.W:] == self.fill).all(), \
            what + ": a byte before or after the buffer's rows was written"
        left, right = body[:, :self.margin], body[:, self.margin + self.S:]
        if not (left == self.fill).all():
            r, b = np.argwhere(left != self.fill)[0]
            raise AssertionError(f"{what}: the left margin was written at (row {int(r)}, byte {int(b) - self.margin})")
        if not (right == self.fill).all():
            r, b = np.argwhere(right != self.fill)[0]
            raise AssertionError(f"{what}: the row padding / right margin was written at (row {int(r)}, byte {self.S + int(b)})")


def first_diff(got, want):
    r, b = np.argwhere(got != want)[0]
    return f"first difference at (row {int(r)}, byte {int(b)}): got {int(got[r, b]):#04x}, want {int(want[r, b]):#04x}"


def assert_span(got, rec, lo, hi, what):
    """Rows [lo, hi) of `got` are the oracle's; every other row is still poison."""
    if not np.array_equal(got[lo:hi], rec[lo:hi]):
        bad = lo + np.flatnonzero((got[lo:hi] != rec[lo:hi]).any(axis=1))
        unwritten = [int(r) for r in bad if (got[r] == POISON).all()]
        want = np.where(((np.arange(len(rec)) >= lo) & (np.arange(len(rec)) < hi))[:, None], rec, got)
        raise AssertionError(f"{what}: {bad.size} of {hi - lo} rows of the span differ, rows {bad[:8].tolist()} "
                             f"(never written: {unwritten[:8]}); " + first_diff(got, want))
    outside = np.ones(len(rec), bool)
    outside[lo:hi] = False
    if not (got[outside] == POISON).all():
        rows = np.flatnonzero(outside & (got != POISON).any(axis=1))
        want = np.where(outside[:, None], np.uint8(POISON), got)
        raise AssertionError(f"{what}: rows outside the span were written, rows {rows[:8].tolist()}; " + first_diff(got, want))


def dev(torch, a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()  # (the oracle's stripes are read-only)


def profiled(torch, rs, ctx, fn):
    rs.profile_enable(True, ctx)
    try:
        rs.profile_collect(ctx)
        fn()
        torch.cuda.synchronize()
        return [name for name, _, _ in rs.profile_collect(ctx)]
    finally:
        rs.profile_enable(False, ctx)


def context_of(rs, c, monkeypatch):
    """None (the default context), or a fresh one created under the case's environment."""
    if not c.env:
        return None
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    return rs.Context(0)


RUNS = [(c, S, pad, 0) for c in SC.CASES for S, pad in (c.layouts or SC.LAYOUTS)] + \
       [(c, S, pad, off) for c in SC.CASES if c.probe for S, pad, off in SC.PROBE_LAYOUTS]


@pytest.mark.parametrize("c,S,pad,off", RUNS,
                         ids=["%s-%d+%d%s" % (SC.case_id(c), S, pad, "-off1" if off else "") for c, S, pad, off in RUNS])
def test_span_repair_matches_oracle(torch, rs, monkeypatch, c, S, pad, off):
    N, M = c.N, c.M
    orig, rec = SC.stripe(c.rate, N, M, S)
    ctx = context_of(rs, c, monkeypatch)
    try:
        rs.mono_enable(c.mode, ctx)
        wo, wr = Wide(torch, N, S, pad, SC.JUNK_O, off), Wide(torch, M, S, pad, SC.JUNK_R, off)
        wx, wy = Wide(torch, N, S, pad, POISON, off), Wide(torch, M, S, pad, POISON, off)
        wo.view.copy_(dev(torch, orig))
        o_before = wo.host()
        assert np.array_equal(wo.matrix(o_before), orig)
        op = np.ones(N, np.uint8)
        for name, lo, hi in SC.spans(c.rate, N, M):
            what = f"{SC.case_id(c)} x {S}+{pad} off {off}, span {name} [{lo}, {hi})"
            rp = np.ones(M, np.uint8)
            rp[lo:hi] = 0
            wr.view.copy_(dev(torch, SC.held_recovery(rec, lo, hi)))
            wy.buf.fill_(POISON)
            r_before = wr.host()
            names = profiled(torch, rs, ctx, lambda: rs.repair_device(
                N, M, S, wo.view, op, wr.view, rp, wx.view, wy.view, rate_=RATE[c.rate], ctx=ctx))
            SC.check_launches(c, S, names)
            hy = wy.host()
            assert_span(wy.matrix(hy), rec, lo, hi, what)
            wy.check_outside(hy, what + ", d_recovery_out")
            assert (wx.host() == POISON).all(), what + ": d_restored was written"
            assert np.array_equal(wo.host(), o_before), what + ": d_original was written"
            assert np.array_equal(wr.host(), r_before), what + ": d_recovery was written"
            rs.check_device(ctx)
    finally:
        if ctx is not None:
            ctx.close()
        else:
            rs.mono_enable(1)


@pytest.mark.parametrize("rate,N,M,S,mode", SC.BATCH, ids=lambda v: str(v))
def test_span_repair_batch(torch, rs, rate, N, M, S, mode):
    """3 stripes with padded stripe strides (3 rows) and row padding (8 bytes), one span per call:
    every stripe as the single calls above, the stripe padding untouched."""
    c = next(c for c in SC.CASES if (c.rate, c.N, c.M, c.mode) == (rate, N, M, mode) and not c.env)
    B, extra, pad = 3, 3, 8
    data = [SC.stripe(rate, N, M, S, seed) for seed in range(B)]
    sp = {name: (lo, hi) for name, lo, hi in SC.spans(rate, N, M)}
    picked = ["first", "edge1" if "edge1" in sp else "mid", "all"]

    def padded(rows, fill):
        return torch.full((B, rows + extra, S + pad), fill, dtype=torch.uint8, device="cuda")

    try:
        rs.mono_enable(mode)
        d_o, d_r, d_x, d_y = padded(N, SC.JUNK_O), padded(M, SC.JUNK_R), padded(N, POISON), padded(M, POISON)
        for b in range(B):
            d_o[b, :N, :S] = dev(torch, data[b][0])
        o_before = d_o.cpu().numpy()
        op = np.ones(N, np.uint8)
        for name in picked:
            lo, hi = sp[name]
            what = f"{SC.case_id(c)} x {S} batch, span {name} [{lo}, {hi})"
            rp = np.ones(M, np.uint8)
            rp[lo:hi] = 0
            for b in range(B):
                d_r[b, :M, :S] = dev(torch, SC.held_recovery(data[b][1], lo, hi))
            d_y.fill_(POISON)
            r_before = d_r.cpu().numpy()
            names = profiled(torch, rs, None, lambda: rs.repair_device_batch(
                N, M, S, d_o[:, :N, :S], op, d_r[:, :M, :S], rp, d_x[:, :N, :S], d_y[:, :M, :S], rate_=RATE[rate]))
            SC.check_launches(c, S, names, stripes=B)
            y = d_y.cpu().numpy()
            for b in range(B):
                assert_span(y[b, :M, :S], data[b][1], lo, hi, f"{what}, stripe {b}")
            assert (y[:, :M, S:] == POISON).all(), what + ": the row padding of d_recovery_out was written"
            assert (y[:, M:] == POISON).all(), what + ": the stripe padding of d_recovery_out was written"
            assert (d_x.cpu().numpy() == POISON).all(), what + ": d_restored was written"
            assert np.array_equal(d_o.cpu().numpy(), o_before), what + ": d_original was written"
            assert np.array_equal(d_r.cpu().numpy(), r_before), what + ": d_recovery was written"
            rs.check_device()
    finally:
        rs.mono_enable(1)
