"""Plain-Python reference for the strobemer calibration entry points (kgma_strobe_window_dists, kgma_strobe_mutation_dists), built
on tests/strobe_oracle.py alone (a helper module, not a conftest).  Everything is in Python integers.

A window with start q of a record is the reference's count vector after step q - 1 (strobe_oracle.window_counts_direct, which runs
the reference's update literally): W - k + 1 items -- for q = 1 the randstrobes at 0-based positions 0 .. W - k of the record, for
q >= 2 those at q - 1 .. q + W - k - 2 plus one permanent copy of the one at position W - k.  Valid starts are 1 .. max(1, L - W) on a
record of L >= W residues.  `params` is (s, w_min, w_max, q)."""
import numpy as np

from tests import strobe_oracle as so


def k_of(params):
    return params[2] + params[0] - 1


def D_of_counts(S, N, cnt):
    """sum_x (S[x] - N c[x])^2."""
    return sum((int(a) - N * int(c)) ** 2 for a, c in zip(S, cnt))


def window_D(seq, S, N, params, W, start):
    return D_of_counts(S, N, so.window_counts_direct(seq, *params, W, start - 1))


def valid_starts(L, W):
    return range(1, max(1, L - W) + 1) if L >= W else range(0)


def item_positions(L, params, W, start):
    """0-based positions in the record of the window's W - k + 1 items (the permanent one last)."""
    k = k_of(params)
    assert start in valid_starts(L, W)
    if start == 1:
        return list(range(0, W - k + 1))
    return list(range(start - 1, start - 1 + W - k)) + [W - k]


def residues_read(L, params, W, start):
    """0-based residues the window's items read."""
    k = k_of(params)
    return sorted({p + t for p in item_positions(L, params, W, start) for t in range(k)})


def position_D(bins, S, N):
    """The kernel's identity over an item's bins: sumS2 - 2 N sum_j S[x_j] + N^2 sum_j c[x_j]."""
    bins = [int(b) for b in bins]
    cnt = {}
    for b in bins:
        cnt[b] = cnt.get(b, 0) + 1
    sumS2 = sum(int(a) ** 2 for a in S)
    return sumS2 - 2 * N * sum(int(S[b]) for b in bins) + N * N * sum(cnt[b] for b in bins)


def window_position_D(seq, S, N, params, W, start):
    bins = so.strobe_bins(seq, *params)
    return position_D([bins[p] for p in item_positions(len(seq), params, W, start)], S, N)


def all_window_D(seq, S, N, params, W):
    """[D of start 1, 2, ..., max(1, L - W)] by ONE run of the reference's update (what window_counts_direct repeats per start),
    D carried along exactly.  tests/test_strobe_calib_host.py holds it to window_D."""
    k = k_of(params)
    L = len(seq)
    assert L >= W
    bins = so.strobe_bins(seq, *params).tolist()
    c = np.bincount(np.asarray(bins[:W - k + 1], dtype=np.int64), minlength=4 ** (2 * params[0])).tolist()
    Sl = [int(x) for x in S]
    D = sum((a - N * b) ** 2 for a, b in zip(Sl, c))
    out = [D]
    for j in range(1, max(1, L - W)):
        l, r = bins[j - 1], bins[j - 1 + W - k]
        if l != r:
            D += (Sl[l] - N * (c[l] - 1)) ** 2 - (Sl[l] - N * c[l]) ** 2 + (Sl[r] - N * (c[r] + 1)) ** 2 - (Sl[r] - N * c[r]) ** 2
            c[l] -= 1
            c[r] += 1
        out.append(D)
    return out


def mutation_D(seq, S, N, params, rate, seed, stream):
    """D of the whole mutated copy: all len - k + 1 randstrobes, no permanent item (shorter than k: sum S^2)."""
    from kmergma_amd import api
    return D_of_counts(S, N, so.strobe_count(api.mutate_seq(seq, rate, seed=seed, stream=stream), *params))
