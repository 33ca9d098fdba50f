"""The split witness map's layout (zkg16_group_layout / zkg16_group_h_layout, host-only): for every two-pass domain 2^12 .. 2^24
and k = 1 .. 8 ranks, the rectangles of the row-pass exchange deliver every element of every rank's row-pass input exactly once,
from the rank that owns its column; the positions a rank's row pass writes are exactly those its next column pass reads; the
redistribution of h gives each shard of a zkg16_shard_plan plan its [h_lo, h_hi) exactly once; bad arguments are refused and
the replicated fallback is reported where the split cannot apply."""
import numpy as np
import pytest

from zksnark_finalproject_amd import Zkg16Error
from zksnark_finalproject_amd.device import group_h_layout, group_layout, shard_plan

SIZES = list(range(12, 25))
KS = list(range(1, 9))


def shape(log_n):
    """(N1, N2, tile) of the two-pass plan, restated from csrc/ntt.hip's plan choice (default ntt_mode)."""
    if log_n > 22:
        return 1 << (log_n - 12), 1 << 12, 1 << 12
    n2 = 1 << (log_n // 2)
    return (1 << log_n) // n2, n2, 1 << 11


def ranges_of(rects, key):
    out = {}
    for r in rects:
        out.setdefault(key(r), set()).add(r)
    return out


@pytest.mark.parametrize("log_n", SIZES)
def test_residues_even_and_aligned(log_n):
    n1, n2, tile = shape(log_n)
    m, unit = min(n1, n2), max(tile // n1, tile // n2)
    for k in KS:
        L = group_layout(log_n, k)
        assert (L["n1"], L["n2"], L["m"], L["unit"]) == (n1, n2, m, unit)
        units = m // unit
        assert L["applies"] == (k <= units), (log_n, k)
        if not L["applies"]:
            assert L["rects"] == []
            continue
        res = L["residues"]
        assert res[0][0] == 0 and res[-1][1] == m
        sizes = []
        for g in range(k):
            lo, hi = res[g]
            assert lo % unit == 0 and hi % unit == 0 and hi > lo
            if g:
                assert lo == res[g - 1][1]
            sizes.append((hi - lo) // unit)
        assert max(sizes) - min(sizes) <= 1


@pytest.mark.parametrize("log_n", SIZES)
def test_exchange_delivers_every_element_once_from_its_column_owner(log_n):
    n1, n2, _ = shape(log_n)
    for k in KS:
        L = group_layout(log_n, k)
        if not L["applies"]:
            continue
        m, res = L["m"], L["residues"]
        rows = [(res[g][1] - res[g][0]) * (n1 // m) for g in range(k)]     # rows a rank's row pass reads
        cols = [(res[g][1] - res[g][0]) * (n2 // m) for g in range(k)]     # columns its column pass writes
        owner = lambda i2: next(g for g in range(k) if res[g][0] <= i2 % m < res[g][1])
        per_pair = ranges_of(L["rects"], lambda r: (r[0], r[1]))
        assert len(L["rects"]) == k * (k - 1) * (n1 // m) * (n2 // m)
        for (src, dst), rs in per_pair.items():
            assert src != dst
            area = 0
            for (_, _, r0, r1, c0, c1, stride) in rs:
                assert stride == n2 and 0 <= r0 < r1 <= n1 and 0 <= c0 < c1 <= n2
                # every row is one of dst's, every column one of src's
                assert all(res[dst][0] <= r % m < res[dst][1] for r in (r0, r1 - 1))
                assert (r1 - 1) // m == r0 // m and (c1 - 1) // m == c0 // m
                assert owner(c0) == src and owner(c1 - 1) == src
                area += (r1 - r0) * (c1 - c0)
            boxes = sorted((r[2], r[3], r[4], r[5]) for r in rs)
            for a in range(len(boxes)):
                for b in range(a + 1, len(boxes)):
                    ra, rb = boxes[a], boxes[b]
                    assert ra[1] <= rb[0] or rb[1] <= ra[0] or ra[3] <= rb[2] or rb[3] <= ra[2], "overlapping rectangles"
            assert area == rows[dst] * cols[src]                  # disjoint, inside, same area: an exact cover
        if log_n <= 16 and k > 1:                                 # brute force: count arrivals per position, per destination
            for dst in range(k):
                cnt = np.zeros(n1 * n2, dtype=np.int32)
                for (src, d, r0, r1, c0, c1, stride) in L["rects"]:
                    if d == dst:
                        rr = np.arange(r0, r1)[:, None] * stride + np.arange(c0, c1)[None, :]
                        np.add.at(cnt, rr.ravel(), 1)
                pos = np.arange(n1 * n2)
                row_mine = (pos // n2) % m
                col_mine = (pos % n2) % m
                need = (row_mine >= res[dst][0]) & (row_mine < res[dst][1]) & ~((col_mine >= res[dst][0]) & (col_mine < res[dst][1]))
                assert np.array_equal(cnt, need.astype(np.int32)), (log_n, k, dst)


@pytest.mark.parametrize("log_n", SIZES)
def test_row_pass_output_is_next_column_pass_input(log_n):
    n1, n2, _ = shape(log_n)
    n = n1 * n2
    pos = np.arange(n, dtype=np.int64)
    for k in (2, 3, 5, 8):
        L = group_layout(log_n, k)
        if not L["applies"]:
            continue
        # the rows each rank's row pass runs and the columns each column pass runs, read off the exchange rectangles
        rows = {g: set() for g in range(k)}
        cols = {g: set() for g in range(k)}
        for (src, dst, r0, r1, c0, c1, _) in L["rects"]:
            rows[dst].update(range(r0, r1))
            cols[src].update(range(c0, c1))
        allowed_rows = np.zeros((k, n1), dtype=bool)
        allowed_cols = np.zeros((k, n2), dtype=bool)
        for g in range(k):
            allowed_rows[g, sorted(rows[g])] = True
            allowed_cols[g, sorted(cols[g])] = True
        assert allowed_rows.sum(axis=0).tolist() == [1] * n1 and allowed_cols.sum(axis=0).tolist() == [1] * n2
        for g in range(k):
            written = allowed_rows[g][pos % n1]          # row pass: X[k1 + N1 k2] for the rank's rows k1
            read = allowed_cols[g][pos % n2]             # next column pass: x[N2 i1 + i2] for the rank's columns i2
            assert np.array_equal(written, read), (log_n, k, g)


@pytest.mark.parametrize("log_n", [12, 13, 16, 19, 22, 23, 24])
def test_h_redistribution_covers_each_shard_once(log_n):
    n = 1 << log_n
    for n_ranks, h_ranks in ((2, 2), (3, 2), (4, 4), (6, 3), (8, 8), (8, 4)):
        plan, k = shard_plan(n_ranks, 100_000, n - 1, 0.0, h_ranks)
        hr = [(p[2], p[3]) for p in plan if p[3] > p[2]]
        assert len(hr) == k
        L = group_layout(log_n, k)
        if not L["applies"]:
            with pytest.raises(Zkg16Error) as e:
                group_h_layout(log_n, k, hr)
            assert e.value.status == 7
            continue
        m, res = L["m"], L["residues"]
        rects = group_h_layout(log_n, k, hr)
        for g in range(k):
            lo, hi = hr[g]
            got = 0
            spans = []
            for (src, dst, r0, r1, c0, c1, stride) in rects:
                if dst != g:
                    continue
                assert src != g and stride == m and res[src][0] <= c0 < c1 <= res[src][1]
                assert r0 * m + c0 >= lo and (r1 - 1) * m + c1 <= hi
                got += (r1 - r0) * (c1 - c0)
                spans.append((r0, r1, c0, c1))
            own_q = np.arange(lo, hi, dtype=np.int64) % m
            own = int(((own_q >= res[g][0]) & (own_q < res[g][1])).sum())
            assert got + own == hi - lo, (log_n, n_ranks, g)
            if log_n <= 16:
                cnt = np.zeros(n, dtype=np.int32)
                for (r0, r1, c0, c1) in spans:
                    np.add.at(cnt, (np.arange(r0, r1)[:, None] * m + np.arange(c0, c1)[None, :]).ravel(), 1)
                assert cnt.max(initial=0) <= 1 and cnt[:lo].sum() == 0 and cnt[hi:].sum() == 0


def test_refusals_and_fallback():
    for args in ((12, 0), (12, 65), (-1, 2), (32, 2)):
        with pytest.raises(Zkg16Error) as e:
            group_layout(*args)
        assert e.value.status == 1, args
    with pytest.raises(Zkg16Error) as e:
        group_layout(16, 2, ntt_mode=2)
    assert e.value.status == 1
    # the replicated map: single-pass and three-pass domains, 2^23 / 2^24 on the three-pass or saturated plan, k above the units
    for log_n, k, mode in ((10, 2, 1), (11, 2, 1), (25, 2, 1), (26, 4, 1), (23, 2, 3), (24, 2, 3), (24, 2, 0), (12, 3, 1), (14, 9, 1)):
        L = group_layout(log_n, k, mode)
        assert not L["applies"] and L["rects"] == [], (log_n, k, mode)
    assert group_layout(22, 2, 0)["applies"] and group_layout(22, 2, 3)["applies"]
    with pytest.raises(Zkg16Error) as e:
        group_h_layout(25, 2, [(0, 100), (100, 200)])
    assert e.value.status == 7
    for bad in ([(0, 3000), (2000, 4095)], [(0, 5000), (5000, 5000)], [(10, 5), (0, 4)]):
        with pytest.raises(Zkg16Error) as e:
            group_h_layout(12, 2, bad)
        assert e.value.status == 1, bad
