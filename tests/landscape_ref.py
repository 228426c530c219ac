"""The distance landscape in plain NumPy: what kgma_dist_bins, kgma_dist_sweep and api.best_loci must return, over a distance vector
`d` (the order of kgma_get_dists) and its layout `offset` (record c = d[offset[c]:offset[c + 1]]; value i of a record is window
start i + 2).  Nothing here calls the library under test."""
import numpy as np


def layout(record_lens, W):
    """offset of the single engine's distance vector: a record of L >= W residues has L - W + 1 windows and L - W values."""
    n = [max(int(L) - int(W), 0) for L in record_lens]
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def bins(d, offset, width):
    """(bin_min, bin_argmin, bin_offset): per record, bins of `width` values (the last may be shorter, a record without values has
    none); the minimum, and the window start (1-based) of the first value attaining it."""
    d = np.asarray(d, dtype=np.float64)
    mins, args, boff = [], [], [0]
    for c in range(len(offset) - 1):
        x = d[offset[c]:offset[c + 1]]
        starts = np.arange(0, x.size, width)
        if x.size:
            mins.append(np.minimum.reduceat(x, starts))
            args.append(np.array([s + int(np.argmin(x[s:s + width])) + 2 for s in starts], dtype=np.int64))
        boff.append(boff[-1] + starts.size)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return cat(mins, np.float64), cat(args, np.int64), np.asarray(boff, dtype=np.int64)


def rank(thr, d):
    """r(d): the number of thresholds <= d."""
    return np.searchsorted(np.asarray(thr, dtype=np.float64), np.asarray(d, dtype=np.float64), side="right")


def run_starts(below, offset):
    """Number of maximal runs of True inside the records of a boolean vector."""
    n = 0
    for c in range(len(offset) - 1):
        b = below[offset[c]:offset[c + 1]]
        if b.size:
            n += int(b[0]) + int(np.count_nonzero(b[1:] & ~b[:-1]))
    return n


def sweep_brute(d, offset, thr):
    """(windows_below, dips_below) threshold by threshold: values d < t, and maximal runs of such values inside a record."""
    d = np.asarray(d, dtype=np.float64)
    below = np.array([int(np.count_nonzero(d < t)) for t in thr], dtype=np.int64)
    dips = np.array([run_starts(d < t, offset) for t in thr], dtype=np.int64)
    return below, dips


def sweep(d, offset, thr):
    """The same through r(d), as the device computes it: a histogram of r, and a difference array of the runs each value starts
    (+1 at r(d_i), -1 at r(predecessor) where r(d_i) < r(predecessor); a record's first value has predecessor +inf)."""
    thr = np.asarray(thr, dtype=np.float64)
    n = thr.size
    r = rank(thr, d)
    rp = np.empty_like(r)
    rp[1:] = r[:-1]
    first = np.unique(offset[:-1][np.diff(offset) > 0])
    rp[first] = n
    hist = np.bincount(r, minlength=n + 1)[:n]
    starts = r < rp
    diff = (np.bincount(r[starts], minlength=n + 1) - np.bincount(rp[starts], minlength=n + 1))[:n]
    return np.cumsum(hist).astype(np.int64), np.cumsum(diff).astype(np.int64)


def best_loci(track, n, sep):
    """api.best_loci restated naively: all (minimum, record, argmin) triples sorted, then taken one by one; a triple is dropped when
    an accepted one of the same record lies fewer than `sep` windows away."""
    triples = sorted((float(m), r, int(a)) for r, t in enumerate(track) for m, a in zip(t[1], t[2]))
    out = []
    for m, r, a in triples:
        if len(out) == n:
            break
        if all(not (r2 == r and abs(a - a2) < sep) for r2, a2, _ in out):
            out.append((r, a, m))
    return out
