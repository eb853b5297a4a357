"""ms-slam_amd/host/KeyFrameDatabase_device.h compiled against stand-in KeyFrame / Frame / Map types (tests/dropin_kfdb_main.cc),
linked to libmsorb.so through the C ABI and run on the GPU: after every query the returned KeyFrames and the six members the
reference leaves on every KeyFrame equal the Python restatement of KeyFrameDatabase.cc (tests/kfdb_cases.py)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.dirname(os.path.abspath(__file__))]
import kfdb_cases as kc  # noqa: E402

pytestmark = pytest.mark.gpu

ADD, ERASE, CLEAR, CLEAR_MAP, RELOC, NBEST = range(6)
MEMBERS = np.dtype([("rq", "<i4"), ("rw", "<i4"), ("rs", "<f4"), ("pq", "<i4"), ("pw", "<i4"), ("ps", "<f4")])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("kfdb") / "dropin_kfdb"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include",
                           f"{ROOT}/tests/dropin_kfdb_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd",
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", str(out)])
    return out


def _bow(words, values):
    return struct.pack("<i", len(words)) + np.asarray(words, np.int32).tobytes() + np.asarray(values, np.float64).tobytes()


def _write(path, n_words, kfs, maps, ops):
    """kfs: every KeyFrame object of the scenario (index = position); ops: tuples as the main reads them."""
    index = {kf: i for i, kf in enumerate(kfs)}
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", n_words, len(kfs), len(ops)))
        for kf in kfs:
            f.write(struct.pack("<iiii", kf.mnId, maps.index(kf.GetMap()), int(kf.mbSparsified), int(kf.mbBad)))
            f.write(_bow(kf.words, kf.values))
            for group in (kf.neighbours, sorted(kf.connected, key=index.__getitem__)):
                f.write(struct.pack("<i", len(group)) + np.array([index[x] for x in group], np.int32).tobytes())
        for op in ops:
            if op[0] in (ADD, ERASE):
                f.write(struct.pack("<ii", op[0], index[op[1]]))
            elif op[0] == CLEAR:
                f.write(struct.pack("<i", CLEAR))
            elif op[0] == CLEAR_MAP:
                f.write(struct.pack("<ii", CLEAR_MAP, maps.index(op[1])))
            elif op[0] == RELOC:
                f.write(struct.pack("<iii", RELOC, op[1].mnId, maps.index(op[2])) + _bow(op[1].words, op[1].values))
            else:
                f.write(struct.pack("<iii", NBEST, index[op[1]], op[2]))


def _replay(db, ops):
    """The same operations on the restatement -> per query (lists of returned ids, members of every KeyFrame)."""
    for op in ops:
        if op[0] == ADD:
            db.add(op[1])
        elif op[0] == ERASE:
            db.erase(op[1])
        elif op[0] == CLEAR:
            db.clear()
        elif op[0] == CLEAR_MAP:
            db.clearMap(op[1])
        elif op[0] == RELOC:
            yield [[kf.mnId for kf in db.DetectRelocalizationCandidates(op[1], op[2])]]
        else:
            loop, merge = db.DetectNBestCandidates(op[1], op[2])
            yield [[kf.mnId for kf in loop], [kf.mnId for kf in merge]]


def _compare(blob, kfs, db, ops):
    pos, n_queries, n_found = 0, 0, 0
    for want in _replay(db, ops):
        for ids in want:
            n, = struct.unpack_from("<i", blob, pos)
            got = np.frombuffer(blob, np.int32, n, pos + 4).tolist()
            pos += 4 + 4 * n
            assert got == ids, (n_queries, got, ids)
            n_found += len(ids)
        m = np.frombuffer(blob, MEMBERS, len(kfs), pos)
        pos += MEMBERS.itemsize * len(kfs)
        exp = np.array([kf.members() for kf in kfs], MEMBERS)
        for name in MEMBERS.names:
            bad = np.nonzero(m[name] != exp[name])[0]
            assert len(bad) == 0, (n_queries, name, bad[:5], m[name][bad[:5]], exp[name][bad[:5]])
        n_queries += 1
    size, = struct.unpack_from("<i", blob, pos)
    assert pos + 4 == len(blob)
    return n_queries, n_found, size


def test_relocalisation_sequence(exe, tmp_path, msorb_mod):
    """The 40 consecutive held-out frames on the 600-KeyFrame three-lap database, two maps, with erases, re-adds and a clearMap on the
    way: the stale mRelocScore of earlier queries takes part (tests/test_kf_database_cpu.py shows that it changes results)."""
    _, kfs, frames, m0 = kc.reloc_sequence(0)
    m1 = kc.Map(1)
    for kf in kfs[400:440]:
        kf.mpMap = m1
    db = kc.KeyFrameDatabase(100000)
    ops = [(ADD, kf) for kf in kfs]
    for t, F in enumerate(frames):
        ops.append((RELOC, F, m0 if t % 9 else m1))
        if t == 15:
            ops += [(ERASE, kfs[i]) for i in (5, 210, 211, 590)] + [(ADD, kfs[211]), (ADD, kfs[5])]
        if t == 28:
            ops.append((CLEAR_MAP, m1))
    ops.append((ADD, kfs[7]))      # already in: ignored
    _write(tmp_path / "in.bin", 100000, kfs, [m0, m1], ops)
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    n_queries, n_found, size = _compare((tmp_path / "out.bin").read_bytes(), kfs, db, ops)
    assert n_queries == 40 and n_found >= 40 and size == 600 - 2 - 40


def test_nbest_sequence(exe, tmp_path, msorb_mod):
    """DetectNBestCandidates on the database with exact duplicates (ties of the accumulated score), unsparsified and bad KeyFrames,
    two maps and connected sets; every 8th query is asked twice (the KeyFrames then carry the query's id already), and the
    twelve-BowVector case of the 0.6f arm follows after a clear."""
    ref, kfs, queries = kc.nbest_sequence(0)
    m0, m1 = queries[0].GetMap(), next(kf.GetMap() for kf in kfs if kf.GetMap() is not queries[0].GetMap())
    _, small, q_small = kc.small_case()
    for k, kf in enumerate(small + [q_small]):     # ids and words of their own, the maps of this scenario
        kf.mnId, kf.mpMap = 7000 + k, m0
    everyone = kfs + queries + small + [q_small]
    db = kc.KeyFrameDatabase(100000)
    ops = [(ADD, kfs[i]) for i in ref.add_order]
    for t, q in enumerate(queries):
        ops.append((NBEST, q, 3))
        if t % 8 == 0:
            ops.append((NBEST, q, 3))
        if t == 20:
            ops += [(ERASE, kfs[i]) for i in (3, 300, 650)] + [(ADD, kfs[300])]
    ops.append((CLEAR,))
    ops += [(ADD, kf) for kf in small] + [(NBEST, q_small, 3)]
    _write(tmp_path / "in.bin", 100000, everyone, [m0, m1], ops)
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    n_queries, n_found, size = _compare((tmp_path / "out.bin").read_bytes(), everyone, db, ops)
    assert n_queries == 46 and n_found >= 40 and size == 12


def test_three_threads_query_while_a_fourth_adds_and_erases(exe, tmp_path, msorb_mod):
    """Through the C ABI: every concurrent result equals the serial result of the snapshot it ran on (with or without the entry that
    the fourth thread erases and adds again)."""
    tr = kc.Trajectory(8, 300, n_words=20000, laps=2)
    kfs = tr.keyframes(kc.Map(0))
    kfs.append(kc.KeyFrame(300, kfs[140].words, kfs[140].values, kfs[0].GetMap()))   # the toggled entry: shares words with many
    _write(tmp_path / "in.bin", 20000, kfs, [kfs[0].GetMap(), kc.Map(1)], [])
    out = subprocess.check_output([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "threads"], timeout=600).decode()
    n_q, differ, n_with, n_without, n_wrong, n_failed, toggles, toggle_failed = struct.unpack("<8i", (tmp_path / "out.bin").read_bytes())
    print(out)
    assert n_wrong == 0 and n_failed == 0 and toggle_failed == 0, out
    assert differ > 0 and toggles > 0, out
    assert n_with + n_without == 6 * sum(n_q - t for t in range(3)), out
