"""numpy restatement of what particles on several ranks add to tests/particles_ref.py: the ownership rule, the class of a
particle along one cut direction, and the device order a migration leaves (stayers in their order, then the arrivals from
pprev, then those from pnext, each in the sender's order), y before z.  Nothing here is shared with the code under test.

A layout is nproc_dir = (1, Py, Pz); rank = ry + Py rz, as in x3d2_amd/mesh.py."""
import numpy as np


def rank_of(layout, ry, rz):
    return int(ry) + int(layout[1]) * int(rz)


def position_of(layout, rank):
    """(0, ry, rz) of a rank"""
    return 0, int(rank) % int(layout[1]), int(rank) // int(layout[1])


def owns(ax, nproc, r, x):
    """does rank r of `nproc` along the direction `ax` (a particles_ref.Axis) own x?  c[r nl] <= x < c[(r + 1) nl]; the last
    rank up to L (periodic) or up to and including the last vertex"""
    x = np.asarray(x, dtype=np.float64)
    nl = ax.n // nproc
    lower = x >= ax.c[r * nl]
    if r == nproc - 1:
        return lower & ((x < ax.L) if ax.periodic else (x <= ax.hi))
    return lower & (x < ax.c[(r + 1) * nl])


def owner_1d(ax, nproc, x):
    """the owner along one direction, -1 where nobody owns x, and how many ranks claim each x"""
    x = np.asarray(x, dtype=np.float64)
    out, count = np.full(x.shape, -1, dtype=np.int64), np.zeros(x.shape, dtype=np.int64)
    for r in range(nproc):
        m = owns(ax, nproc, r, x)
        out[m] = r
        count += m
    return out, count


def owner(axes, layout, x):
    """the rank that owns each row of x [n, 3] (wrapped, inside the domain)"""
    ry, _ = owner_1d(axes[1], int(layout[1]), x[:, 1])
    rz, _ = owner_1d(axes[2], int(layout[2]), x[:, 2])
    return ry + int(layout[1]) * rz


def classify(ax, nproc, r, x, status):
    """0 stays, 1 to pprev, 2 to pnext, 3 owned by neither; status 2 always stays.  Two ranks around a period: the other rank
    is pnext."""
    x = np.asarray(x, dtype=np.float64)
    nxt = r + 1 if r + 1 < nproc else (0 if ax.periodic else None)
    prv = r - 1 if r > 0 else (nproc - 1 if ax.periodic else None)
    cls = np.full(x.shape, 3, dtype=np.int64)
    if prv is not None:
        cls[owns(ax, nproc, prv, x)] = 1
    if nxt is not None:
        cls[owns(ax, nproc, nxt, x)] = 2
    cls[owns(ax, nproc, r, x)] = 0
    cls[np.asarray(status) == 2] = 0
    return cls


def migrate(axes, layout, order, x, status):
    """order: per rank the ids in device order BEFORE the migration; x [n, 3], status [n]: the state by id after the move.
    Returns the per-rank ids in device order after the y and the z exchange.  A particle owned by neither neighbour stays."""
    order = [np.asarray(o, dtype=np.int64) for o in order]
    for d in (1, 2):
        P = int(layout[d])
        if P == 1:
            continue
        stay, to_prev, to_next = {}, {}, {}
        for rank, ids in enumerate(order):
            r = position_of(layout, rank)[d]
            cls = classify(axes[d], P, r, x[ids, d], status[ids])
            stay[rank], to_prev[rank], to_next[rank] = ids[(cls == 0) | (cls == 3)], ids[cls == 1], ids[cls == 2]
        new = []
        for rank in range(len(order)):
            pos = list(position_of(layout, rank))
            prv, nxt = list(pos), list(pos)
            prv[d], nxt[d] = (pos[d] - 1) % P, (pos[d] + 1) % P
            prv, nxt = rank_of(layout, prv[1], prv[2]), rank_of(layout, nxt[1], nxt[2])
            new.append(np.concatenate([stay[rank], to_next[prv], to_prev[nxt]]))
        order = new
    return order


def initial_order(axes, layout, x0):
    """per rank the ids it is seeded with: the rows it owns, ascending"""
    own = owner(axes, layout, x0)
    return [np.nonzero(own == r)[0] for r in range(int(np.prod(layout)))]


def assemble(pieces):
    """rank pieces (dicts with `id` and per-particle arrays) -> one dict in id order"""
    ids = np.concatenate([p["id"] for p in pieces])
    o = np.argsort(ids, kind="stable")
    return {k: np.concatenate([p[k] for p in pieces])[o] for k in pieces[0]}
