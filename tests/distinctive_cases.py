"""MapPoint::ComputeDistinctiveDescriptors: a plain reference and descriptor sets at the edges of csrc/distinctive.hip.

Uniformly random descriptors put every row median near 128 and make ties rare.  The sets here have distances of 0 and of 256
(the top bit of the 9-step radix select, bin 256 of the big kernel's histogram), tied medians (the strict `<` of
MapPoint.cc:418: the FIRST row with the smallest median wins) and list lengths on both sides of every width class."""
import numpy as np

INT_MAX = 2 ** 31 - 1
SIZES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129, 320, 1000)
# distinct_small_kernel<W>: one W-lane segment per point with N <= W, 256 / W points per block; distinct_big_kernel above 64
WIDTHS = (8, 16, 32, 64)
BLOCK = 256


def reference_distinctive(desc, obs_begin):
    """MapPoint.cc:391-423 per point: the N x N Hamming matrix from the unpacked bits, every row sorted, entry int(0.5 * (N - 1))
    of each, the first row with the strictly smallest one.  -> (best_idx, best_median) as int32; (-1, INT_MAX) for N == 0."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n = len(obs_begin) - 1
    best_idx, best_median = np.full(n, -1, np.int32), np.full(n, INT_MAX, np.int32)
    for p in range(n):
        b, e = int(obs_begin[p]), int(obs_begin[p + 1])
        N = e - b
        if N == 0:
            continue
        bits = np.unpackbits(desc[b:e], axis=1).astype(np.float64)       # N x 256 of 0 / 1: the products below are exact integers
        dist = bits @ (1 - bits).T
        dist = (dist + dist.T).astype(np.int64)                          # bits set in exactly one of the two
        medians = np.sort(dist, axis=1)[:, int(0.5 * (N - 1))]
        best, idx = INT_MAX, 0
        for i in range(N):                                               # :412-423
            if medians[i] < best:
                best, idx = int(medians[i]), i
        best_idx[p], best_median[p] = idx, best
    return best_idx, best_median


def row_medians(desc):
    """The medians of one point's rows (for the assertions about what a set contains)."""
    bits = np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1).astype(np.int64)
    dist = bits @ (1 - bits).T
    return np.sort(dist + dist.T, axis=1)[:, int(0.5 * (len(bits) - 1))]


def _flip(rng, d, n_bits, lo, hi):
    """d with n_bits distinct bits of [lo, hi) flipped"""
    bits = np.unpackbits(d)
    bits[lo + rng.choice(hi - lo, n_bits, replace=False)] ^= 1
    return np.packbits(bits)


def identical(rng, N):
    """every distance 0: every median 0, row 0 wins"""
    return np.tile(rng.integers(0, 256, 32, dtype=np.uint8), (N, 1))


def pool3(rng, N):
    """Rows drawn from three patterns A, B, C with d(A,B) = 40, d(A,C) = 90, d(B,C) = 130: rows of one pattern tie, the medians take
    a handful of values.  Row 0 is C, the pattern farthest from the others, so from N = 3 on the minimum is rarely at row 0."""
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    pats = np.stack([a, _flip(rng, a, 40, 0, 128), _flip(rng, a, 90, 128, 256)])
    which = rng.integers(0, 3, N)
    which[0] = 2
    return pats[which]


def complement(rng, N):
    """The first (N - 1) // 2 rows are the bitwise complement of the others: distances are 0 or 256.  The majority's rows have median
    0; the minority's rows come first and have (N - 1) // 2 zeros in front of entry (N - 1) // 2, so median 256, for odd and even N
    from 3 on; the winner is the first row of the majority, not row 0."""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    d = np.tile(base, (N, 1))
    d[:(N - 1) // 2] = ~base
    return d


def outlier(rng, N):
    """identical rows and one at distance 77: at row 0 when N is odd (the winner is row 1 from N = 3 on), at the last row else"""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    d = np.tile(base, (N, 1))
    d[0 if N % 2 else N - 1] = _flip(rng, base, 77, 0, 256)
    return d


FAMILIES = dict(identical=identical, pool3=pool3, complement=complement, outlier=outlier)


def _pack(lists, lead=0):
    """lists of N x 32 arrays -> (desc, obs_begin); `lead` unused descriptors in front (obs_begin[0] > 0)"""
    sizes = [len(x) for x in lists]
    desc = np.concatenate([np.full((lead, 32), 0xA5, np.uint8)] + [np.asarray(x, np.uint8).reshape(-1, 32) for x in lists])
    return np.ascontiguousarray(desc), (lead + np.cumsum([0] + sizes)).astype(np.int32)


def _mixed(rng, W, with_empties=False):
    """2 * (256 / W) + 1 points of width class W: the third block has ONE live segment, the threads of the others leave at
    `if (g >= n_list) return` while it goes on to __ballot.  The list lengths cycle through the class, so the segments of a
    wavefront differ in N: 1..8 for W = 8 (N = 1 included), else W/2 + 1 .. W (both ends of the class)."""
    lo = 1 if W == 8 else W // 2 + 1
    n = 2 * (BLOCK // W) + 1
    sizes = [lo + (i * 5) % (W - lo + 1) for i in range(n)]
    sizes[-1] = W
    fams = list(FAMILIES.values())
    lists = [fams[i % 4](rng, N) for i, N in enumerate(sizes)]
    if with_empties:
        lists = [x for l in lists for x in (l, np.zeros((0, 32), np.uint8))]
    return lists


def edge_sets():
    """name -> (desc, obs_begin)"""
    out = {}
    for f, (name, fam) in enumerate(FAMILIES.items()):
        rng = np.random.Generator(np.random.PCG64(100 + f))
        out["sweep_" + name] = _pack([fam(rng, N) for N in SIZES])
    for W in WIDTHS:
        out["mixed_%d" % W] = _pack(_mixed(np.random.Generator(np.random.PCG64(200 + W)), W))
    rng = np.random.Generator(np.random.PCG64(300))
    out["offset_begin"] = _pack([pool3(rng, N) for N in (5, 1, 12, 70, 33)], lead=5)
    # every class at once, an empty point after every point, one in front, and obs_begin[0] > 0
    everything = [np.zeros((0, 32), np.uint8)] + [x for W in WIDTHS for x in _mixed(rng, W, with_empties=True)] + [complement(rng, 131)]
    out["empties_interleaved"] = _pack(everything, lead=3)
    return out
