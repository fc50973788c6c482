"""An independent numpy restatement of place recognition (include/sageicp.h, sageicp_place_*): the descriptor of a frame
and the matcher of a database, written from the header's rules and nothing of the library's code.  The two tables
(squared ring edges, sector directions) are the library's own (sage.place_tables), so no decision is recomputed from a
libm that may differ; everything after them is plain fp64 (numpy ufuncs: no contraction) and Python integers.

    describe(rows, params, tables) -> (heights, classes), uint8 (R, S): the sector by brute force over all S, with the
        assertion that every kept row has exactly one s with f(s) and not f(s + 1); the cells by np.maximum.at
    match(db, desc, ...) -> list of dicts: three nested loops over entries, shifts and cells (the cells vectorised per
        shift), ranked with Python integers
    scores(entries, desc, h_tol) -> ((agree, shift, n_entry), n_query) of every entry: the same rules with one numpy pass
        over all entries per shift, for databases of thousands of entries; match(..., scores=) ranks them
    prior(pose, shift, S) -> (yaw, prior[7])
"""
import functools
import math

import numpy as np


def describe(rows, params, tables, return_kept=False):
    edge2, dirs = tables
    R, S = int(params.rings), int(params.sectors)
    rank = np.array(params.rank[:], dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    assert np.isfinite(rows[:, :3]).all()
    x, y, z, l = rows.T
    with np.errstate(invalid="ignore"):
        ok = (l > -1.0) & (l < 256.0)
    c = np.zeros(len(rows), dtype=np.int64)
    c[ok] = np.trunc(l[ok]).astype(np.int64)
    assert ((c >= 0) & (c <= 255)).all()
    ok &= rank[c] != 0
    r2 = x * x + y * y
    ok &= ~(r2 < edge2[0]) & ~(r2 >= edge2[R])
    x, y, z, c, r2 = x[ok], y[ok], z[ok], c[ok], r2[ok]
    ring = (r2[:, None] >= edge2[None, 1:R]).sum(axis=1) if R > 1 else np.zeros(len(x), dtype=np.int64)
    # f[i, s]; the sector is where f(s) holds and f(s + 1) does not: exactly one such s per kept row
    f = (dirs[None, :, 0] * y[:, None] - dirs[None, :, 1] * x[:, None]) >= 0.0
    edge = f & ~np.roll(f, -1, axis=1)
    assert (edge.sum(axis=1) == 1).all(), "a kept row without exactly one sector"
    sector = edge.argmax(axis=1)
    t = (z - params.z_lo) / (params.z_hi - params.z_lo)
    v = np.where(t > 0.0, np.where(t < 1.0, t, 1.0), 0.0)
    h = 1 + np.floor(v * 254.0).astype(np.int64)
    assert ((h >= 1) & (h <= 255)).all()
    key = rank[c] << 8 | c
    heights = np.zeros(R * S, dtype=np.int64)
    keys = np.zeros(R * S, dtype=np.int64)
    cell = ring * S + sector
    np.maximum.at(heights, cell, h)
    np.maximum.at(keys, cell, key)
    out = heights.astype(np.uint8).reshape(R, S), (keys & 0xFF).astype(np.uint8).reshape(R, S)
    return out + (np.flatnonzero(ok), ring, sector) if return_kept else out


def score(qh, qc, eh, ec, h_tol):
    """(agree, shift, n_query, n_entry) of one entry: shift the smallest of maximal agree"""
    qh, qc, eh, ec = (np.asarray(a).astype(np.int64) for a in (qh, qc, eh, ec))
    S = qh.shape[1]
    best, shift = -1, 0
    for k in range(S):
        sh, sc = np.roll(eh, -k, axis=1), np.roll(ec, -k, axis=1)        # sh[r, s] = eh[r, (s + k) % S]
        agree = int(((qh > 0) & (sh > 0) & (qc == sc) & (np.abs(qh - sh) <= h_tol)).sum())
        if agree > best:
            best, shift = agree, k
    return best, shift, int((qh > 0).sum()), int((eh > 0).sum())


def scores(entries, desc, h_tol):
    """((agree, shift, n_entry), n_query): int64 arrays over all entries, shift the smallest of maximal agree.  One pass
    over the entries per shift: an entry cell (r, s + k) agrees with the query cell (r, s) when both are occupied, the
    classes are equal and the heights differ by at most h_tol"""
    e = np.asarray(entries)
    assert e.ndim == 4 and e.shape[1] == 2, "entries: (N, 2, R, S), or a sequence of (heights, classes)"
    qh, qc = (np.asarray(a).astype(np.int16) for a in desc)
    N, S = len(e), qh.shape[1]
    assert e.shape[2:] == qh.shape == qc.shape
    e = e.astype(np.int16)
    e = np.concatenate([e, e], axis=3)                   # e[..., s + k] without a wrap
    agree, shift = np.full(N, -1, dtype=np.int64), np.zeros(N, dtype=np.int64)
    for k in range(S):
        sh, sc = e[:, 0, :, k:k + S], e[:, 1, :, k:k + S]
        a = ((qh > 0) & (sh > 0) & (qc == sc) & (np.abs(qh - sh) <= h_tol)).sum(axis=(1, 2), dtype=np.int64)
        better = a > agree                               # (strictly: a later shift of equal agreement does not replace)
        agree[better], shift[better] = a[better], k
    n_entry = (e[:, 0, :, :S] > 0).sum(axis=(1, 2), dtype=np.int64)
    return (agree, shift, n_entry), int((qh > 0).sum())


def prior(pose, shift, S):
    w = 2.0 * math.pi / S
    yaw = shift * w if shift <= S // 2 else (shift - S) * w
    p = [float(v) for v in pose]
    if shift:
        s, c = math.sin(yaw / 2.0), math.cos(yaw / 2.0)
        x, y, z, ww = p[:4]
        p[:4] = [c * x + s * y, c * y - s * x, c * z + s * ww, c * ww - s * z]
    return yaw, np.array(p)


def match(entries, desc, top_k=1, h_tol=0, exclude_last=0, min_similarity=0.0, tags=None, poses=None, scores=None):
    """entries: a sequence of (heights, classes); desc: (heights, classes).  The matches as dicts, best first.
    scores: what scores(entries, desc, h_tol) returned, in place of the loop over score(); the ranking is the same code"""
    size = len(entries)
    if exclude_last >= size:
        return []
    qh, qc = desc
    S = np.asarray(qh).shape[1]
    recs = []
    for i in range(size - exclude_last):
        if scores is not None:
            (agree, shift, ne), nq = (int(a[i]) for a in scores[0]), int(scores[1])
        else:
            agree, shift, nq, ne = score(qh, qc, entries[i][0], entries[i][1], h_tol)
        m = max(nq, ne)
        recs.append(dict(index=i, agree=agree, shift=shift, n_query=nq, n_entry=ne, m=m))

    def order(a, b):
        am, bm = (a["m"] or 1), (b["m"] or 1)
        aa, ba = (a["agree"] if a["m"] else 0), (b["agree"] if b["m"] else 0)
        if aa * bm != ba * am:
            return -1 if aa * bm > ba * am else 1
        return -1 if a["index"] < b["index"] else 1

    recs.sort(key=functools.cmp_to_key(order))
    out = []
    for r in recs[:top_k]:
        r["similarity"] = r["agree"] / r["m"] if r["m"] else 0.0
        if r["similarity"] < min_similarity:
            continue
        r["tag"] = int(tags[r["index"]]) if tags is not None else 0
        r["pose"] = np.array(poses[r["index"]], dtype=np.float64) if poses is not None else np.array([0, 0, 0, 1.0, 0, 0, 0])
        r["yaw"], r["prior"] = prior(r["pose"], r["shift"], S)
        out.append(r)
    return out


def same(device, ref):
    """the device's record array against the restatement's list: every field, the doubles bit for bit"""
    assert len(device) == len(ref), (len(device), len(ref))
    for d, r in zip(device, ref):
        for k in ("index", "agree", "shift", "n_query", "n_entry", "tag"):
            assert int(d[k]) == int(r[k]), (k, d, r)
        assert d["similarity"] == r["similarity"] and d["yaw"] == r["yaw"], (d, r)
        assert np.array_equal(d["pose"], r["pose"])
        assert np.allclose(d["prior"], r["prior"], rtol=0, atol=2.0 ** -52), (d["prior"], r["prior"])
    return True
