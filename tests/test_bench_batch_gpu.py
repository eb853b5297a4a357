"""Every image of bench.py's batch against the oracle: 128 distinct KITTI-size stereo pairs (256 images, 2000 features), the
images bench.py builds for `--pairs 128 --unique-pairs 128` on one GPU.  The other tests at this size tile at most 16 distinct
images, so an error that sends image i to image i + 8k (a sub-batch reading another's slices, a wait returning another
handle's block) would leave them passing.  Here the inputs and the oracle's outputs are pairwise distinct, and every image is
compared: the synchronous batch under every sub-batch split, the bench's two-handle pipelined loop with content that changes
from step to step, what bench.py itself returns, the stereo association of all 128 pairs and the dense top-2 of all 128 frames."""
import json
import os
import queue
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from msorb import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matcher_cases as mc  # noqa: E402
from batch_compare import OracleBatch, digest, pairwise_distinct, read_dump, workers  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CFG = synth.KITTI
PAIRS = 128
N = 2 * PAIRS
MB, MBF = mc.KITTI_BF / mc.KITTI_FX, mc.KITTI_BF
SENTINEL = 0xFF          # output blocks are filled with it before a run: bytes the library did not write cannot pass


def _extractor(msorb_mod):
    return msorb_mod.ORBextractor(CFG["nfeatures"], CFG["scale"], CFG["nlevels"], CFG["ini_th"], CFG["min_th"])


def _resident(torch, host):
    """bench.py's resident(): the batch on the device with a 64-byte row pitch"""
    n, rows, cols = host.shape
    st = torch.zeros((n, rows, (cols + 63) // 64 * 64), dtype=torch.uint8, device="cuda")
    v = st[:, :, :cols]
    v.copy_(torch.from_numpy(np.ascontiguousarray(host)).cuda())
    torch.cuda.synchronize()            # the library's streams are not ordered after torch's
    return v


def _blocks(torch, cap):
    out = (torch.full((N, cap, 28), SENTINEL, dtype=torch.uint8, device="cuda"),
           torch.full((N, cap, 32), SENTINEL, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(workers()) as p:
        yield p


@pytest.fixture(scope="module")
def images():
    A = synth.stereo_batch(PAIRS, CFG["rows"], CFG["cols"], seed0=0)
    assert A.shape == (N, CFG["rows"], CFG["cols"])
    assert pairwise_distinct(digest(a) for a in A)
    return A


@pytest.fixture(scope="module")
def ref(oracle, images, pool):
    """The oracle on every image (one pair of OracleExtractors per worker), with each pair's stereo association while both
    pyramids are still held (the oracle keeps only its last image's pyramid)."""
    make = lambda: oracle.OracleExtractor(CFG["nfeatures"], CFG["scale"], CFG["nlevels"], CFG["ini_th"], CFG["min_th"])
    spare = queue.Queue()
    for _ in range(workers()):
        spare.put((make(), make()))
    tab = make().tables()

    def pair(p):
        exl, exr = spare.get()
        try:
            left, right = exl(images[2 * p]), exr(images[2 * p + 1])
            st = oracle.compute_stereo_matches(left[1], left[2], right[1], right[2], [exl.level(l) for l in range(CFG["nlevels"])],
                                               [exr.level(l) for l in range(CFG["nlevels"])], tab["scale"], tab["inv_scale"], MB, MBF)
        finally:
            spare.put((exl, exr))
        return left, right, st

    res = list(pool.map(pair, range(PAIRS)))
    r = OracleBatch(*zip(*[out for left, right, _ in res for out in (left, right)]))
    r.stereo = [st for _, _, st in res]
    r.tables = tab
    assert len(r) == N and r.distinct()
    assert min(len(k) for k in r.kps) > 1800
    return r


@pytest.fixture(scope="module")
def d_images(images):
    import torch
    return _resident(torch, images)


@pytest.fixture(scope="module")
def extracted(msorb_mod, d_images):
    """One synchronous extraction of the batch with the default sub-batch split, kept on its handle (the stereo association
    reads the handle's pyramids of its last batch)."""
    import torch
    ex = _extractor(msorb_mod)
    counts, mono, d_kps, d_desc = ex.extract_batch(d_images, (0, 0), out=_blocks(torch, ex.capacity))
    yield ex, counts, mono, d_kps, d_desc
    ex.close()


def _host(msorb_mod, counts, d_kps, d_desc):
    return msorb_mod.keypoints_from_device(d_kps, counts), d_desc.cpu().numpy()


def test_sync_batch_every_image_under_every_sub_batch_split(msorb_mod, ref, d_images):
    """extract_batch on 256 distinct images: 2 groups (default, cut at image 128), 1 (the bench's pipelined setting), 3 (85 / 85
    / 86) and 4 without the blur stream, one handle reconfigured between the runs; every image equals the oracle each time."""
    import torch
    assert d_images.stride(1) == 1280
    ex = _extractor(msorb_mod)
    try:
        for groups, blur2 in ((2, True), (1, True), (3, True), (4, False)):
            ex.set_overlap(groups, blur2)
            counts, mono, d_kps, d_desc = ex.extract_batch(d_images, (0, 0), out=_blocks(torch, ex.capacity))
            ref.assert_batch(counts, mono, *_host(msorb_mod, counts, d_kps, d_desc), what=f"set_overlap({groups}, {blur2})")
    finally:
        ex.close()


def test_pipelined_two_handles_with_content_that_changes_between_batches(msorb_mod, ref, images, d_images):
    """bench.py's loop (two handles, one sub-batch each, own output blocks; step k + 1 submitted before step k is waited for) on
    batches A and B = A rolled by one pair.  Each waited block is copied at once and compared, all 256 images, with the oracle of
    what was submitted: a wait that returns before its block is complete, or returns the other handle's block, cannot pass."""
    import torch
    roll = (np.arange(N) + 2) % N                     # B[i] = A[i + 2]: left stays left, every position changes content
    content = [(d_images, None), (_resident(torch, images[roll]), roll)]
    # A, B, A, B ... as the bench's loop would run with changing input (handle k % 2 sees the same content every time), then
    # B, A, B, A: each handle now gets the other content, so a handle that returned its own previous block would be seen
    seq = [0, 1] * 4 + [1, 0] * 2
    exs = [_extractor(msorb_mod) for _ in range(2)]
    side = torch.cuda.Stream()
    try:
        for e in exs:
            e.set_overlap(1, True)
        outs = [_blocks(torch, exs[0].capacity) for _ in range(2)]
        inflight, waited = [], []

        def wait():
            k, h = inflight.pop(0)
            counts, mono, d_kps, d_desc = exs[h].extract_batch_wait()
            assert d_kps is outs[h][0] and d_desc is outs[h][1]
            waited.append((k, counts, mono, d_kps.clone(), d_desc.clone()))

        for k, c in enumerate(seq):
            h = k % 2
            side.wait_stream(torch.cuda.current_stream())   # after the copy of the block's previous batch
            with torch.cuda.stream(side):             # that batch was waited for: no writer is left
                outs[h][0].fill_(SENTINEL)
                outs[h][1].fill_(SENTINEL)
            side.synchronize()
            exs[h].extract_batch_submit(content[c][0], (0, 0), out=outs[h])
            inflight.append((k, h))
            if len(inflight) == 2:
                wait()
        while inflight:
            wait()
        torch.cuda.synchronize()
        assert [w[0] for w in waited] == list(range(len(seq)))
        for k, counts, mono, d_kps, d_desc in waited:
            ref.assert_batch(counts, mono, *_host(msorb_mod, counts, d_kps, d_desc), src=content[seq[k]][1],
                             what=f"step {k} ({'AB'[seq[k]]}, handle {k % 2})")
    finally:
        for e in exs:
            e.close()


def _env():
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MSORB_BENCH_SYNC", "MSORB_BENCH_DEPTH",
              "MSORB_BENCH_STAGGER_US"):
        e.pop(k, None)
    return e


def _last_json(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert lines, stdout[-2000:]
    return json.loads(lines[-1])


def test_what_bench_returns_is_the_oracle_for_every_image(msorb_mod, ref, tmp_path):
    """The headline run itself (pipelined, two batches in flight, staggered: >= 8 steps) with 128 distinct pairs: the dumped
    last step, every row of it, decoded back into per-image keypoints and descriptors, equals the oracle image by image."""
    d = tmp_path / "dump"
    q = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--pairs", str(PAIRS), "--unique-pairs", str(PAIRS),
                        "--steps", "10", "--warmup", "2", "--dump-outputs", str(d)], cwd=ROOT, env=_env(), capture_output=True, text=True,
                       timeout=900)
    assert q.returncode == 0, q.stderr[-3000:]
    out = _last_json(q.stdout)
    assert out["steps"] == 10 and out["config"]["images_per_step_per_gpu"] == N
    assert out["config"]["batches_in_flight"] == 2 and out["config"]["stagger_us"] > 0, out["config"]
    counts, mono, kps, desc = read_dump(str(d), msorb_mod.KP_DTYPE)
    assert len(counts) == N and int(counts.sum()) == out["keypoints_per_step"]
    ref.assert_batch(counts, mono, kps, desc, what="bench.py --dump-outputs")


def test_stereo_association_of_all_128_pairs(msorb_mod, oracle, ref, extracted):
    """msorb_stereo_matches_batch over the extracted batch: uRight and depth of every pair bit for bit, the per-pair count of
    out-of-range windows, -1 past each left count."""
    ex, counts, mono, d_kps, d_desc = extracted
    assert np.array_equal(ex.GetScaleFactors(), ref.tables["scale"])
    assert np.array_equal(ex.GetInverseScaleFactors(), ref.tables["inv_scale"])
    assert np.array_equal(counts, [len(k) for k in ref.kps])
    d_ur, d_dp, oob, _ = msorb_mod.stereo_matches_batch(ex, counts, d_kps, d_desc, MB, MBF)
    ur, dp = d_ur.cpu().numpy(), d_dp.cpu().numpy()
    assert ur.shape[0] == PAIRS and len(oob) == PAIRS
    bad = []
    for p, (rur, rdp, roob) in enumerate(ref.stereo):
        nl = int(counts[2 * p])
        if not np.array_equal(ur[p, :nl].view(np.uint32), rur.view(np.uint32)):
            bad.append(f"pair {p}: uRight")
        if not np.array_equal(dp[p, :nl].view(np.uint32), rdp.view(np.uint32)):
            bad.append(f"pair {p}: depth")
        if oob[p] != roob:
            bad.append(f"pair {p}: n_oob {oob[p]}, the oracle has {roob}")
        if not (np.all(ur[p, nl:] == -1) and np.all(dp[p, nl:] == -1)):
            bad.append(f"pair {p}: entries past the left count")
    assert not bad, f"{len(bad)} differences: " + "; ".join(bad[:6])
    assert min(int((r[0] > 0).sum()) for r in ref.stereo) > 500          # every pair has stereo work


def test_dense_top2_of_all_128_frames(msorb_mod, oracle, ref, extracted, pool):
    """Left against right descriptors of every frame, both formulations, every live row against oracle.dense_top2."""
    import torch
    _, counts, _, _, d_desc = extracted
    dq, dt = d_desc[0::2].contiguous(), d_desc[1::2].contiguous()
    nq = torch.from_numpy(np.ascontiguousarray(counts[0::2])).cuda()
    nt = torch.from_numpy(np.ascontiguousarray(counts[1::2])).cuda()
    want = list(pool.map(lambda f: oracle.dense_top2(ref.desc[2 * f], ref.desc[2 * f + 1]), range(PAIRS)))
    assert pairwise_distinct(digest(*w) for w in want)
    for name, form in (("popcount", msorb_mod.DENSE_POPCOUNT), ("matrix cores", msorb_mod.DENSE_MATRIX_CORES)):
        got = [g.cpu().numpy() for g in msorb_mod.hamming_dense_top2_batch(dq, dt, nq, nt, formulation=form)[:3]]
        bad = [f for f in range(PAIRS)
               if not all(np.array_equal(w, g[f, :int(counts[2 * f])]) for w, g in zip(want[f], got))]
        assert not bad, f"{name}: {len(bad)} of {PAIRS} frames differ from the oracle, first {bad[:8]}"
