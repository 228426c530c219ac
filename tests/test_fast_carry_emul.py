"""The order-independent step total of stream8_kernel's fast path, emulated in numpy.

One steady step of the stream kernel applies its 64 lanes' transitions as two atomic instructions: every entering k-mer's
count is incremented (in some order inside the instruction), then every leaving k-mer's count is decremented.  The fast path
forms each lane's increment from the counts those atomics returned,

    e'_i = S[l] - S[r] - N (olds_i - 1 - oldp_i),

instead of the exact counts in lane order.  The emulation checks, for random and adversarial orders inside each atomic
instruction, that the step total is exact and that every prefix stays within N floor((P + 2)^2 / 4) of the exact prefix,
P = pending entering + pending leaving lanes (0 when P = 0).
"""
import numpy as np
import pytest

LANES = 64


def _kmers(codes, k):
    n = len(codes) - k + 1
    v = np.zeros(n, dtype=np.int64)
    for j in range(k):
        v = (v << 2) | codes[j:j + n]
    return v


def _orders(rng, lanes):
    """Orders inside one atomic instruction: random, lane order, reverse lane order."""
    lanes = list(lanes)
    yield list(rng.permutation(lanes))
    yield lanes
    yield lanes[::-1]


def _check_step(counts, S, N, kp, ks, order_e, order_l):
    """One step from the start counts `counts`: returns (total exact, total fast, max |E' - E|, P)."""
    act = kp != ks
    cp, cs = counts[kp], counts[ks]                            # start-of-step counts (the kernel's byte loads)
    # exact: lane order
    c = counts.copy()
    e = np.zeros(LANES, dtype=np.int64)
    for i in range(LANES):
        if not act[i]:
            continue
        cP, cS = c[kp[i]], c[ks[i]]
        e[i] = S[ks[i]] - S[kp[i]] - N * (cS - cP - 1)
        c[kp[i]] += 1
        c[ks[i]] -= 1
    # atomics: every entering add, then every leaving subtract, each in its own order
    a = counts.copy()
    oldp = np.zeros(LANES, dtype=np.int64)
    olds = np.zeros(LANES, dtype=np.int64)
    for i in order_e:
        oldp[i] = a[kp[i]]
        a[kp[i]] += 1
    for i in order_l:
        olds[i] = a[ks[i]]
        a[ks[i]] -= 1
        assert a[ks[i]] >= 0, "a leaving k-mer's count went below zero"
    assert np.array_equal(a, c), "the atomics end on other counts than the lane order"
    ef = np.where(act, S[ks] - S[kp] - N * (olds - 1 - oldp), 0)
    P = int(np.count_nonzero(act & (oldp != cp)) + np.count_nonzero(act & (olds != cs)))
    dev = int(np.max(np.abs(np.cumsum(ef) - np.cumsum(e))))
    return int(e.sum()), int(ef.sum()), dev, P, c


def _margin(P):
    return 0 if P == 0 else (P + 2) ** 2 // 4


def _run(seq_codes, k, nk, S, N, rng, orders=3):
    """Slides a window of nk k-mers over the sequence in steps of 64 windows; checks every step under several orders."""
    km = _kmers(seq_codes, k)
    counts = np.zeros(1 << (2 * k), dtype=np.int64)
    np.add.at(counts, km[:nk], 1)
    worst = {}
    for s in range(0, len(km) - nk - LANES + 1, LANES):
        # lane i: k-mer nk + s + i enters, k-mer s + i leaves
        kp = km[nk + s:nk + s + LANES]
        ks = km[s:s + LANES]
        act = np.nonzero(kp != ks)[0]
        nxt = None
        for oe, ol in zip(_orders(rng, act), _orders(rng, act)):
            tot, totf, dev, P, nxt = _check_step(counts, S, N, kp, ks, oe, ol)
            assert tot == totf, f"step {s}: fast total {totf} != exact total {tot}"
            assert dev <= N * _margin(P), f"step {s}: prefix deviation {dev} > N * {_margin(P)} (P = {P})"
            worst[P] = max(worst.get(P, 0), dev // N)
        if nxt is None:
            continue
        counts = nxt
    return worst


def _S(rng, k, N=7):
    return rng.integers(0, N + 1, size=1 << (2 * k)).astype(np.int64), N


# (nk < 64: a lane's leaving k-mer entered by lane p - nk of the same step -- it is not in the start-of-step counts, so nearly every
#  lane is pending; the step total and the prefix margin hold all the same)
@pytest.mark.parametrize("k,nk", [(6, 284), (5, 120), (2, 200), (6, 2), (6, 17), (6, 63), (5, 33), (2, 3)])
def test_random_sequence(k, nk):
    rng = np.random.default_rng(1000 + k)
    S, N = _S(rng, k)
    worst = _run(rng.integers(0, 4, size=nk + k - 1 + 64 * 40), k, nk, S, N, rng)
    assert worst, "no step was checked"


def test_homopolymer_next_to_random():
    rng = np.random.default_rng(7)
    k, nk = 6, 284
    S, N = _S(rng, k)
    seq = np.concatenate([rng.integers(0, 4, size=400), np.full(500, 2), rng.integers(0, 4, size=600)])
    _run(seq, k, nk, S, N, rng)


@pytest.mark.parametrize("period", range(1, 9))
def test_tandem_repeats(period):
    rng = np.random.default_rng(100 + period)
    k, nk = 6, 284
    S, N = _S(rng, k)
    unit = rng.integers(0, 4, size=period)
    rep = np.tile(unit, 700 // period + 1)[:700]
    seq = np.concatenate([rng.integers(0, 4, size=350), rep, rng.integers(0, 4, size=500)])
    worst = _run(seq, k, nk, S, N, rng)
    assert max(worst) > 0 or period == 1, "a repeat without pending lanes"


@pytest.mark.parametrize("nk", [17, 63])
def test_short_windows_tandem_and_homopolymer(nk):
    """Windows of fewer k-mers than a step has lanes, over a tandem repeat (period 3 and 7) and a homopolymer next to random sequence."""
    k = 6
    for period in (3, 7):
        rng = np.random.default_rng(200 + 10 * nk + period)
        S, N = _S(rng, k)
        unit = rng.integers(0, 4, size=period)
        rep = np.tile(unit, 700 // period + 1)[:700]
        worst = _run(np.concatenate([rng.integers(0, 4, size=350), rep, rng.integers(0, 4, size=500)]), k, nk, S, N, rng)
        assert max(worst) > 0, "a repeat without pending lanes"
    rng = np.random.default_rng(300 + nk)
    S, N = _S(rng, k)
    worst = _run(np.concatenate([rng.integers(0, 4, size=400), np.full(500, 2), rng.integers(0, 4, size=600)]), k, nk, S, N, rng)
    assert max(worst) > 0


def test_many_collisions():
    """k = 1 and 2: every step is full of collisions (P up to 128); the bound still holds, far from tight."""
    rng = np.random.default_rng(3)
    for k, nk in ((1, 150), (2, 90)):
        S, N = _S(rng, k, N=5)
        worst = _run(rng.integers(0, 4, size=nk + k - 1 + 64 * 30), k, nk, S, N, rng)
        assert max(worst) >= 20


def test_bound_is_needed():
    """The prefix does deviate (the margin is not vacuous): a two-letter stretch at k = 1 under reverse order."""
    rng = np.random.default_rng(11)
    k, nk = 1, 100
    S, N = _S(rng, k, N=3)
    seq = np.concatenate([np.zeros(nk), np.tile([0, 1], 40)]).astype(np.int64)
    worst = _run(seq, k, nk, S, N, rng)
    assert any(v > 0 for v in worst.values())


def test_margin_superadditive():
    """Keys' bounds add up under the step's bound: floor((a+2)^2/4) + floor((b+2)^2/4) <= floor((a+b+2)^2/4) for a, b >= 1."""
    for a in range(1, 130):
        for b in range(1, 130 - a):
            assert _margin(a) + _margin(b) <= _margin(a + b)
