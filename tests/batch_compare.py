"""Image-by-image comparison of a whole extracted batch with the CPU oracle, and the reader of bench.py --dump-outputs.
Shared by test_bench_batch_gpu.py (every image of the bench batch) and test_bench_batch_cpu.py (the reader's own check)."""
import hashlib
import os

import numpy as np

FIELDS = ("octave", "x", "y", "response", "size", "angle", "class_id")


def workers():
    """Oracle threads: the oracle is a ctypes CDLL (the GIL is released), at most 16 CPUs per job."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def pairwise_distinct(items):
    """True if no two of the digests are equal."""
    items = list(items)
    return len(set(items)) == len(items)


class OracleBatch:
    """The oracle's outputs for every image of a batch: mono[j], kps[j] (KP_DTYPE records), desc[j] (n x 32 u8)."""

    def __init__(self, mono, kps, desc):
        self.mono = np.asarray(mono, np.int64)
        self.kps = list(kps)
        self.desc = list(desc)

    def __len__(self):
        return len(self.kps)

    def distinct(self):
        return pairwise_distinct(digest(k, d) for k, d in zip(self.kps, self.desc))

    def same_as_oracle(self, i, counts, mono, kps, desc, src=None):
        """Image i of a batch (counts / mono per image; kps[i] KP_DTYPE records, desc[i] rows of 32 bytes, each at least
        counts[i] long) against oracle image src[i] (default i): count, monoIndex, every keypoint field by its uint32 bit
        pattern, the descriptor bytes.  Raises AssertionError naming the image and the first field that differs."""
        j = i if src is None else int(src[i])
        where = f"image {i}" + ("" if j == i else f" (oracle image {j})")
        rk, rd = self.kps[j], self.desc[j]
        c = int(counts[i])
        if c != len(rk):
            raise AssertionError(f"{where}: {c} keypoints, the oracle has {len(rk)}")
        if int(mono[i]) != self.mono[j]:
            raise AssertionError(f"{where}: monoIndex {int(mono[i])}, the oracle has {self.mono[j]}")
        k = np.asarray(kps[i])[:c]
        for f in FIELDS:
            a, b = k[f].view(np.uint32), rk[f].view(np.uint32)
            if not np.array_equal(a, b):
                r = int(np.flatnonzero(a != b)[0])
                raise AssertionError(f"{where}: keypoint {r} field {f} is {k[f][r]}, the oracle has {rk[f][r]}")
        d = np.asarray(desc[i])[:c]
        if not np.array_equal(d, rd):
            r = int(np.flatnonzero((d != rd).any(axis=1))[0])
            raise AssertionError(f"{where}: descriptor {r} differs from the oracle's")

    def assert_batch(self, counts, mono, kps, desc, src=None, what="batch"):
        """same_as_oracle for every image of the batch; the message counts the images that differ and names the first few."""
        assert len(counts) == len(mono) == len(kps) == len(desc) == (len(self) if src is None else len(src))
        bad = []
        for i in range(len(counts)):
            try:
                self.same_as_oracle(i, counts, mono, kps, desc, src)
            except AssertionError as e:
                bad.append(str(e))
        assert not bad, f"{what}: {len(bad)} of {len(counts)} images differ from the oracle; " + "; ".join(bad[:4])


def read_dump(path, kp_dtype):
    """bench.py --dump-outputs DIR -> (counts, mono, kps, desc): per image, the keypoints as kp_dtype records and the
    descriptors as n x 32 bytes.  The dump must hold every row: a sampled one (keypoint_index.npy) cannot be split by image."""
    assert not os.path.exists(os.path.join(path, "keypoint_index.npy")), "the dump holds a sample of the rows, not all of them"
    ld = lambda name: np.load(os.path.join(path, name + ".npy"))
    counts_f, mono_f, cols, words = ld("counts"), ld("mono"), ld("keypoints"), ld("descriptors")
    for a in (counts_f, mono_f):
        assert a.dtype == np.float64 and a.ndim == 1 and np.array_equal(a, np.rint(a))
    counts, mono = counts_f.astype(np.int64), mono_f.astype(np.int64)
    total = int(counts.sum())
    assert len(mono) == len(counts) and counts.min() >= 0
    assert cols.dtype == np.float32 and cols.shape == (total, len(kp_dtype.names)), cols.shape
    assert words.dtype == np.float64 and words.shape == (total, 8), words.shape
    rec = np.zeros(total, kp_dtype)
    for k, f in enumerate(kp_dtype.names):
        col = cols[:, k]
        if kp_dtype[f].kind != "f":
            assert np.array_equal(col, np.rint(col)), f"column {f} is not integral"
        rec[f] = col.astype(kp_dtype[f])
    assert np.all((words >= 0) & (words < 2.0 ** 32)) and np.array_equal(words, np.rint(words)), "descriptor words are not uint32"
    raw = words.astype(np.uint64).astype("<u4").view(np.uint8).reshape(total, 32)
    ends = np.cumsum(counts)
    starts = ends - counts
    return counts, mono, [rec[a:b] for a, b in zip(starts, ends)], [raw[a:b] for a, b in zip(starts, ends)]
