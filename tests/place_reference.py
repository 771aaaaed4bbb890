"""The numpy restatement of elo_scan_descriptor / elo_descriptor_search, written from include/elo.h (PLACE RECOGNITION), not from
the kernels: float64 and Python integers, one IEEE operation per step of the rule."""
import math

import numpy as np

LEVELS = 4095


def edge2(rings, max_range):
    """edge2[j] = e_j * e_j, e_j = (double)max_range * j / rings, j = 0 .. rings: the numbers the caller passes in."""
    out = []
    for j in range(rings + 1):
        e = float(max_range) * j / rings
        out.append(e * e)
    return np.array(out, np.float64)


def sector_of(W, sectors):
    """The sector of every column: (w * sectors) / W in integers."""
    return (np.arange(W, dtype=np.int64) * sectors) // W


def descriptor(xyz, rings, sectors, max_range, min_range=0.0, z_min=-3.0, z_step=0.005):
    """xyz (n,H,W,3) float32 -> (n, sectors, rings) uint16."""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32 and xyz.ndim == 4 and xyz.shape[3] == 3 and xyz.shape[2] >= sectors
    n, H, W, _ = xyz.shape
    e2 = edge2(rings, max_range)
    min2 = float(min_range) * float(min_range)
    x, y, z = (xyz[..., c].astype(np.float64) for c in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        empty = (xyz[..., 0] == 0) & (xyz[..., 1] == 0) & (xyz[..., 2] == 0)
        finite = np.isfinite(xyz).all(-1)
        r2 = x * x + y * y
        ring = np.zeros(r2.shape, np.int64)
        for j in range(1, rings + 1):
            ring += e2[j] <= r2
        keep = ~empty & finite & ~(r2 < min2) & ~(r2 >= e2[rings])
        f = np.floor((z - float(z_min)) / float(z_step))
        f = np.where(f < 0.0, 0.0, np.where(f > LEVELS - 1.0, LEVELS - 1.0, f))
    level = np.where(keep, f, 0.0).astype(np.int64) + 1
    sector = np.broadcast_to(sector_of(W, sectors)[None, None, :], r2.shape)
    out = np.zeros((n, sectors, rings), np.int64)
    b = np.broadcast_to(np.arange(n)[:, None, None], r2.shape)
    np.maximum.at(out, (b[keep], sector[keep], ring[keep]), level[keep])
    return out.astype(np.uint16)


def terms(Q, D):
    """(T, ok): T[j][c] = 1 - d / sqrt(a b) for column j of Q against column c of D, ok[j][c] False where the pair is skipped."""
    Q, D = np.asarray(Q).astype(np.int64), np.asarray(D).astype(np.int64)
    a, b = (Q * Q).sum(1), (D * D).sum(1)
    d = Q @ D.T
    ok = (a[:, None] != 0) & (b[None, :] != 0)
    prod = (a[:, None] * b[None, :]).astype(np.uint64).astype(np.float64)               # one conversion of the 64-bit product
    with np.errstate(divide="ignore", invalid="ignore"):
        T = 1.0 - d.astype(np.float64) / np.sqrt(prod)
    return np.where(ok, T, 0.0), ok


def shift_profile(Q, D):
    """dist of every shift s = 0 .. sectors - 1, (sectors,) float64: the terms of the pairs (j, (j + s) mod sectors) added in
    ascending j, one after the other (np.add.accumulate is that loop; a skipped pair adds +0.0, which changes nothing), divided by
    the number of pairs; +inf without one."""
    T, ok = terms(Q, D)
    S = T.shape[0]
    j = np.arange(S)
    c = (j[None, :] + j[:, None]) % S                                                    # c[s][j]
    G, n = T[j[None, :], c], ok[j[None, :], c].sum(1)
    total = np.add.accumulate(G, axis=1)[:, -1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 0, total / n.astype(np.float64), np.inf)


def best_of(profile):
    """(shift, dist): the smallest dist, the smaller shift winning a tie."""
    s = int(np.argmin(profile))                                                         # (the first of equal minima)
    return s, float(profile[s])


def search(query, db, m, k):
    """-> dict(entry (n,k), shift (n,k), dist (n,k), best_shift (n,m), best_dist (n,m), profile (n,m,sectors))."""
    query, db = np.asarray(query), np.asarray(db)
    n, S = query.shape[0], query.shape[1]
    profile = np.full((n, m, S), np.inf)
    best_shift, best_dist = np.zeros((n, m), np.int32), np.full((n, m), np.inf)
    for q in range(n):
        for e in range(m):
            profile[q, e] = shift_profile(query[q], db[e])
            best_shift[q, e], best_dist[q, e] = best_of(profile[q, e])
    entry, shift, dist = np.full((n, k), -1, np.int32), np.full((n, k), -1, np.int32), np.full((n, k), np.inf)
    for q in range(n):
        order = sorted(range(m), key=lambda e: (best_dist[q, e], e))[:k]
        for r, e in enumerate(order):
            entry[q, r], shift[q, r], dist[q, r] = e, best_shift[q, e], best_dist[q, e]
    return dict(entry=entry, shift=shift, dist=dist, best_shift=best_shift, best_dist=best_dist, profile=profile)


def yaw_of(shift, sectors):
    """The query's heading relative to the entry's, in [-pi, pi): minus the shift's share of a turn (columns run against the
    azimuth)."""
    shift = shift % sectors
    if 2 * shift > sectors:
        shift -= sectors
    return -shift * (2.0 * math.pi / sectors) if shift else 0.0
