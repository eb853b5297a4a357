"""msorb_create_new_map_points_kf on the device against R32 of tests/new_map_points_cases.py, bit for bit: match12, status, the bits of
x3D, nmatches and n_created of every neighbour.  Small shapes at the edges of new_points_kernel (one thread per feature of the
current KeyFrame, workgroups of 256, wavefronts of 64) and of the chain (one to ten neighbours, a neighbour without features, one
without a common node, nothing created, everything created at the first neighbour)."""
import numpy as np
import pytest

import new_map_points_cases as nmp

pytestmark = pytest.mark.gpu


def _all_created_at_first(seed, n1):
    """a scene whose valid queries all get their point at neighbour 0: the queries are cut down to those that do, until that holds"""
    sc = nmp.make_scene(seed, n1=n1, K=3, far_frac=0.0, octave_jitter=0.0, mask_frac=0.0)
    while True:
        r = nmp.R32(sc)
        made = (r[0]["status"] >= nmp.TRIANGULATED) & (r[0]["status"] <= nmp.STEREO2)
        if np.array_equal(made, sc["valid1"].astype(bool)):
            return sc
        sc["valid1"] = made.astype(np.uint8)


SHAPES = {
    "n1=0": lambda: nmp.make_scene(21, n1=0, K=2, n2=40),
    "n1=1": lambda: nmp.make_scene(22, n1=1, K=2, n2=40, mask_frac=0.0, n_nodes=1),
    "n1=63": lambda: nmp.make_scene(23, n1=63, K=2),
    "n1=64": lambda: nmp.make_scene(24, n1=64, K=2),
    "n1=65": lambda: nmp.make_scene(25, n1=65, K=1),
    "n1=257": lambda: nmp.make_scene(26, n1=257, K=2),
    "K=3": lambda: nmp.make_scene(27, n1=90, K=3),
    "K=10": lambda: nmp.make_scene(28, n1=120, K=10, n2=100, step=(0.5, 0.02, 0.3)),
    "n2=0": lambda: nmp.make_scene(29, n1=90, K=3, n2=[80, 0, 90]),
    "no_common_node": lambda: nmp.make_scene(30, n1=90, K=3, disjoint_nodes=(2,)),
    "all_rejected": lambda: nmp.make_scene(31, n1=90, K=2, th_far=0.5, stereo_frac=0.0, far_frac=0.0),
    "all_created_first": lambda: _all_created_at_first(32, 120),
}
SHAPES.update(nmp.SCENES)   # plain, reclaimed, inertial_far (inertial, th_far on), coarse_noorient (coarse on, orientation off), degenerate


@pytest.fixture(scope="module")
def store(msorb_mod):
    st = msorb_mod.KeyFrameStore()
    yield st
    st.close()


@pytest.fixture(scope="module")
def cases(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            sc = SHAPES[name]()
            cache[name] = (sc, nmp.R32(sc))
        return cache[name]
    return get


def _run(store, sc, **kw):
    ids = nmp.store_scene(store, sc)
    try:
        call, nbs = nmp.device_call(sc, ids, **kw)
        return store.create_new_map_points(call, nbs)
    finally:
        for i in ids:
            store.remove(i)


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_r32_bit_for_bit(store, cases, name):
    sc, ref = cases(name)
    if name == "all_rejected":
        assert sum(r["nmatches"] for r in ref) > 10 and sum(r["n_created"] for r in ref) == 0
    if name == "all_created_first":
        assert ref[0]["n_created"] == int(sc["valid1"].sum()) > 20 and all(r["nmatches"] == 0 for r in ref[1:])
    if name == "no_common_node":
        assert ref[1]["nmatches"] == 0 and ref[0]["nmatches"] > 0 and ref[2]["nmatches"] > 0
    if name == "reclaimed":
        assert any(not np.array_equal(a["match12"], b["match12"]) for a, b in zip(ref, nmp.stale(sc)))
    dev = _run(store, sc)
    assert nmp.same_bits(dev, ref) is None, nmp.same_bits(dev, ref)
    again = _run(store, sc)
    assert nmp.same_bits(again, dev) is None


def test_one_call_equals_one_call_per_neighbour(store, cases):
    sc, ref = cases("reclaimed")
    ids = nmp.store_scene(store, sc)
    valid = sc["valid1"].copy()
    single = []
    for k in range(len(ref)):
        call, nbs = nmp.device_call(sc, ids, valid1=valid, neighbours=[k])
        r = store.create_new_map_points(call, nbs)[0]
        single.append(r)
        valid[(r["status"] >= nmp.TRIANGULATED) & (r["status"] <= nmp.STEREO2)] = 0
    for i in ids:
        store.remove(i)
    assert nmp.same_bits(single, ref) is None


def test_interleaved_with_the_resident_search(store, cases):
    sc, ref = cases("plain")
    ids = nmp.store_scene(store, sc)
    st = [(kf["geometry"]["u_right"] >= 0).astype(np.uint8) for kf in sc["kfs"]]
    pairs = [dict(kf1=ids[0], kf2=ids[k + 1], valid1=sc["valid1"], avail2=sc["avail2"][k], stereo1=st[0], stereo2=st[k + 1],
                  F12=sc["F12"][k], ep=sc["ep"][k]) for k in range(len(ref))]
    call, nbs = nmp.device_call(sc, ids)
    s0 = store.search_for_triangulation(pairs, sc["coarse"], sc["check_orientation"])[0]
    a = store.create_new_map_points(call, nbs)
    s1 = store.search_for_triangulation(pairs, sc["coarse"], sc["check_orientation"])[0]
    b, ms = store.create_new_map_points(call, nbs, timing=True)
    for i in ids:
        store.remove(i)
    assert nmp.same_bits(a, ref) is None and nmp.same_bits(b, ref) is None and ms > 0
    assert all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(s0, s1))
    assert np.array_equal(s0[0][1], ref[0]["match12"])      # the first neighbour sees the masks the batched search sees


def test_bad_arguments_are_refused(msorb_mod, store, cases):
    sc, ref = cases("n1=63")
    ids = nmp.store_scene(store, sc)
    call, nbs = nmp.device_call(sc, ids)

    def refused(c, n):
        with pytest.raises(msorb_mod.MsorbError) as e:
            store.create_new_map_points(c, n)
        return e.value.code == msorb_mod.E_INVALID

    assert store.create_new_map_points(call, []) == []
    store.n[10 ** 6] = 63
    assert refused(dict(call, kf1=10 ** 6), nbs)                                  # unknown ids
    assert refused(call, [dict(nbs[0], kf2=10 ** 6), nbs[1]])
    assert refused(call, [dict(nbs[0], kf2=ids[0]), nbs[1]])                      # kf2 == kf1
    assert refused(call, [nbs[0], dict(nbs[1], kf2=nbs[0]["kf2"])])               # the same kf2 twice
    assert refused(dict(call, valid1=None), nbs)                                  # null arrays
    assert refused(call, [dict(nbs[0], avail2=None), nbs[1]])
    for key in ("u_right", "depth"):
        assert refused(dict(call, geometry=dict(call["geometry"], **{key: None})), nbs)
        assert refused(call, [nbs[0], dict(nbs[1], geometry=dict(nbs[1]["geometry"], **{key: None}))])
    del store.n[10 ** 6]
    assert nmp.same_bits(store.create_new_map_points(call, nbs), ref) is None     # and the store still answers
    for i in ids:
        store.remove(i)
