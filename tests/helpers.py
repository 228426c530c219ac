"""Shared helpers for the parity tests: seeded synthetic genomes with planted, mutated genes."""
import numpy as np

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def random_dna(rng, n):
    return BASES[rng.integers(0, 4, size=n)].tobytes()


def mutate(rng, seq: bytes, rate: float) -> bytes:
    a = np.frombuffer(seq.upper(), dtype=np.uint8).copy()
    hit = rng.random(a.size) < rate
    a[hit] = BASES[rng.integers(0, 4, size=int(hit.sum()))]
    return a.tobytes()


def make_genome(rng, lengths, genes, n_plants_per_mb=40.0, max_rate=0.15, n_runs=True, lowercase=True):
    """Random contigs of the given lengths with mutated copies of `genes` planted at random
    positions, a few runs of N and some lower-case stretches.  Returns (contigs, plants)."""
    contigs, plants = [], []
    for ci, L in enumerate(lengths):
        a = bytearray(random_dna(rng, L))
        n_pl = int(rng.poisson(n_plants_per_mb * L / 1e6)) if L > 400 else 0
        for _ in range(n_pl):
            g = genes[int(rng.integers(0, len(genes)))]
            g = mutate(rng, g, float(rng.random()) * max_rate)
            if len(g) >= L:
                continue
            pos = int(rng.integers(0, L - len(g)))
            a[pos:pos + len(g)] = g
            plants.append((ci, pos + 1, len(g)))
        if n_runs and L > 2000:
            for _ in range(int(rng.integers(0, 3))):
                pos = int(rng.integers(0, L - 600))
                ln = int(rng.integers(1, 600))
                a[pos:pos + ln] = b"N" * ln
        if lowercase and L > 100:
            pos = int(rng.integers(0, L - 50))
            a[pos:pos + 50] = bytes(a[pos:pos + 50]).lower()
        contigs.append(bytes(a))
    return contigs, plants


def hit_key(h):
    return (h["contig"], h["kfv"], h["cmi"], h["lo"], h["hi"], h["genome_pos"])


_CODE = np.full(256, 3, dtype=np.int64)                       # N (and anything else the scans accept) reads as T
for _c, _v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    _CODE[_c] = _v


def kmer_values(seq: bytes, k: int) -> np.ndarray:
    """Natural k-mer value of every window of seq (first base most significant; lower case as upper, N as T)."""
    c = _CODE[np.frombuffer(seq, dtype=np.uint8)]
    n = len(c) - k + 1
    v = np.zeros(max(n, 0), dtype=np.int64)
    for j in range(k):
        v = (v << 2) | c[j:j + n]
    return v


def sparse_family(rng, L, k, n_refs=7, rate=0.03):
    """A reference family as gen_ref_ws_cons sees it, without a 4^k table: (base, dict(keys, S, N, vals, ws, k)), keys the k-mers
    of the references in increasing order, S their counts, vals = S * (1 / N) (gen_ref_ws_cons's form)."""
    base = random_dna(rng, L)
    refs = [mutate(rng, base, rate) for _ in range(n_refs)]
    keys, S = np.unique(np.concatenate([kmer_values(r, k) for r in refs]), return_counts=True)
    S = S.astype(np.int64)
    return base, dict(keys=keys.astype(np.uint32), S=S, N=n_refs, vals=S * (1.0 / n_refs), ws=L, k=k)


def thr_for_sparse(rng, ref, frac=0.5):
    """_thr_for (tests/test_gpu_wide.py) of a sparse ref: a fraction of a random window's distance, rounded to 0.1."""
    from oracle import oracle as orc
    return float(np.round(frac * orc.kmer_dist_kfv_sparse(random_dna(rng, ref["ws"]), (ref["keys"], ref["vals"]), ref["k"]), 1))


def sparse_int_D(seq: bytes, skeys, sS, N: int, k: int, W: int) -> np.ndarray:
    """D = sum_x (S[x] - N c[x])^2 of every window of seq, from the window's distinct k-mers and the KFV's non-zero keys: a numpy
    restatement independent of the oracle (one np.unique per window: short sequences only)."""
    km = kmer_values(seq, k)
    nk = W - k + 1
    Smap = dict(zip(np.asarray(skeys).tolist(), np.asarray(sS).tolist()))
    base = int(np.sum(np.asarray(sS).astype(object) ** 2))
    out = []
    for s in range(len(seq) - W + 1):
        u, c = np.unique(km[s:s + nk], return_counts=True)
        D = base
        for x, cx in zip(u.tolist(), c.tolist()):
            Sx = Smap.get(x, 0)
            D += (Sx - N * cx) ** 2 - Sx * Sx
        out.append(D)
    return np.asarray(out, dtype=np.int64)
