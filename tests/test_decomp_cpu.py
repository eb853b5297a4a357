"""The small dense decompositions of the solvers and optimisers, one routine at a time, on the host: ms-slam_amd/csrc/
decomp_probe_device.h (the text msorb_debug_decomp compiles, which calls two_view_device.h, new_points_device.h, sim3_device.h,
mlpnp_device.h and inertial_device.h) built as tests/decomp_probe_main.cc with g++ -O2, and once under the address / undefined-
behaviour sanitizers (a stand-alone program, nothing loaded into Python), and run over every record of tests/decomp_cases.py:

 - the families reach what they name (the restatements' traces: zero rotations, every reordering swap, a negated U column, both
   degenerate arms of the 2x2 step, both signs of tau and tau == 0, the floor test refusing a pair, every early exit of the rank);
 - the host program within 16 D(op, family, measure) of the exact value, D from tests/golden/decomp_sensitivity.json, and exact
   where something is exact (the order and sign of S, ranks, ok flags, a refusal leaving x untouched, the documented outcome of a
   non-finite or out-of-domain input);
 - the host program equal, bit for bit, to the restatements of decomp_cases.py and to the ones the solvers' own tests use
   (new_map_points_cases, sim3_cases, mlpnp_cases), on every record (a NaN matching a NaN);
 - the sweeps each family needs, below the cap on every family inside the routine's domain;
 - the golden file reproduced from scratch.
No GPU."""
import os
import subprocess

import numpy as np
import pytest

import decomp_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
BUILDS = (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


@pytest.fixture(scope="module")
def host_outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("decomp_cpu")
    blocks = [(op, dc.records(op)[0]) for op in dc.OPS] + [("tv_svd3", np.zeros((0, 9)))]   # (an empty block is valid)
    dc.write_blocks(str(d / "in.bin"), blocks)
    out = {}
    for tag, extra in BUILDS:
        exe = str(d / f"decomp_probe_main_{tag}")
        b = subprocess.run(["g++", *FLAGS, *extra, os.path.join(ROOT, "tests", "decomp_probe_main.cc"), "-o", exe], capture_output=True,
                           text=True, timeout=600)
        assert b.returncode == 0, b.stderr
        p = subprocess.run([exe, str(d / "in.bin"), str(d / f"out_{tag}.bin")], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (tag, p.stdout[-400:], p.stderr[-3000:])
        out[tag] = dict(zip(dc.OPS, dc.read_blocks(str(d / f"out_{tag}.bin"), blocks)))
    return out


@pytest.mark.parametrize("op", dc.OPS)
def test_the_records(op):
    rec, fams = dc.records(op)
    assert len(rec) >= 40 and rec.shape[1] == dc.in_width(op) and len(fams) == len(rec)
    if op in dc.FLOAT_OPS:                                           # float ops take exactly representable floats
        with np.errstate(all="ignore"):
            assert dc.same_bits(rec, rec.astype(np.float32).astype(np.float64))
    if op in ("tv_null_vector_8", "tv_null_vector_16"):              # the scale families sit where their names say
        for r, fam in zip(rec, fams):
            N = float(np.sqrt((r.reshape(-1, 9) ** 2).sum(0).max()))
            if fam == "scale: below the domain":
                assert 1e-18 < N < dc.TV_DOMAIN[0], (fam, N)
            elif fam == "scale: nothing rotates":
                assert N < 1e-19 or N > 2.0 ** 32, (fam, N)
            elif not fam.startswith("non-finite") and fam != "zero":
                assert dc.TV_DOMAIN[0] <= N <= dc.TV_DOMAIN[1], (fam, N)
    if op == "mlpnp_rank3":                                          # "near the rule" is within a factor of 4 of 3 eps, "clear gap" far above
        for r, fam in zip(rec, fams):
            if fam in ("near the rule", "clear gap: rank 3"):
                s = np.linalg.svd(r.reshape(3, 3), compute_uv=False)
                ratio = s[2] / s[0]
                assert (0.25 <= ratio / (3 * dc.EPS64) <= 4.0) if fam == "near the rule" else ratio >= 1e-8, (fam, ratio)


def test_the_families_reach_what_they_name():
    def seen(op, key, fams=None):
        return sum(tr.get(key, 0) for tr, fam in zip(dc.restated_all(op)[1], dc.records(op)[1]) if fams is None or fam in fams)

    for op in ("tv_svd3", "np_null_vector"):
        for key in ("|d|<tiny", "deno<tiny", "tau>0", "tau<0", "tau==0", "swap0", "swap1"):
            assert seen(op, key) > 0, (op, key)
        assert seen(op, "rotations", ("identity", "diagonal", "zero")) == 0   # an already diagonal input: zero rotations
    assert seen("tv_svd3", "negated") > 0
    assert seen("np_null_vector", "swap2") > 0 and seen("np_null_vector", "zero maximum") > 0
    fams, traces = dc.records("tv_svd3")[1], dc.restated_all("tv_svd3")[1]
    orders = {(tr.get("swap0", 0), tr.get("swap1", 0)) for tr, fam in zip(traces, fams) if fam == "permutation"}
    assert orders == {(0, 0), (0, 1), (1, 0), (1, 1)}                          # every combination of the two selection swaps
    for op in ("tv_null_vector_8", "tv_null_vector_16"):
        for key in ("tau>0", "tau<0", "tau==0", "floor refused", "minimum tie"):
            assert seen(op, key) > 0, (op, key)
        assert seen(op, "rotations", ("identity", "permutation", "orthogonal columns", "zero", "scale: nothing rotates")) == 0
        assert seen(op, "floor refused", ("nullity 1", "nullity 2", "nullity 4", "zero column")) > 0
    for op in ("sim3_largest_eigenvector", "mlpnp_eig3", "mlpnp_null_vector_12", "mlpnp_null_vector_9"):
        for key in ("tau>0", "tau<0", "tau==0"):
            assert seen(op, key) > 0, (op, key)
        assert seen(op, "rotations", ("identity", "diagonal", "zero")) == 0
        assert seen(op, "rotations", ("zero diagonal",)) > 0                   # max_diag == 0 at entry still rotates
    assert seen("sim3_largest_eigenvector", "maximum tie") > 0
    assert seen("mlpnp_null_vector_12", "minimum tie") > 0 and seen("mlpnp_null_vector_9", "minimum tie") > 0
    for key in ("nonzero=0", "nonzero=1", "nonzero=2", "tailsq<=tiny", "big==bound"):
        assert seen("mlpnp_rank3", key) > 0, key
    for col in (0, 1, 2, 4, 8):
        assert seen("inertial_ldlt", f"refused at {col}") > 0, col


@pytest.mark.parametrize("op", dc.OPS)
def test_the_golden_record_is_current(op):
    """D comes from LAPACK, whose last bits are the installed library's: a regenerated D may differ from the committed one, which is
    the bound the tests use, by a factor of 4 at the most (most entries are the n eps floor and do not move); the sweep counts are the
    restatements' and are exact"""
    g, m = dc.golden()["D"].get(op, {}), dc.measure(op)
    assert sorted(g) == sorted(m) == sorted({f for f in dc.records(op)[1] if dc.judged_by_measure(op, f)})
    for fam in m:
        assert sorted(g[fam]) == sorted(m[fam])
        for k in m[fam]:
            assert 0.25 <= g[fam][k] / m[fam][k] <= 4.0, (op, fam, k, g[fam][k], m[fam][k])
    assert dc.golden()["sweeps"].get(op, {}) == dc.sweeps(op)


@pytest.mark.parametrize("op", [op for op in dc.OPS if op in dc.SWEEP_CAP])
def test_the_sweeps_stay_below_the_cap(op):
    s = dc.sweeps(op)
    print(f"{op}: the most rotating sweeps of a family {max(s.values())} of {dc.SWEEP_CAP[op]}: {s}")
    over = {fam: n for fam, n in s.items() if n >= dc.SWEEP_CAP[op] and not dc.sweep_cap_exempt(op, fam)}
    assert not over, over


@pytest.mark.parametrize("op", dc.OPS)
def test_the_host_program_against_the_exact_value(op, host_outputs):
    out = host_outputs["plain"][op]
    worst, failures = dc.judge(op, out)
    print(f"{op}: {len(out)} records, host program: largest measure / D {worst:.3f}")
    assert not failures, (len(failures), failures[:5])


@pytest.mark.parametrize("op", dc.OPS)
def test_the_host_program_against_the_restatement_in_bits(op, host_outputs):
    out, fams = host_outputs["plain"][op], dc.records(op)[1]
    bad = dc.differing_records(out, dc.restated_all(op)[0])
    assert not bad, (len(bad), [(i, fams[i]) for i in bad[:5]])


def test_the_solvers_own_restatements_give_the_same_bits(host_outputs):
    """the restatements the solvers' tests replay whole pipelines with, held to the host program on the new families"""
    import mlpnp_cases
    import new_map_points_cases
    import sim3_cases
    out = host_outputs["plain"]
    with np.errstate(all="ignore"):
        rec = dc.records("np_null_vector")[0]
        x = new_map_points_cases.jacobi_null_vector32(rec.reshape(-1, 4, 4).astype(np.float32))
        assert not dc.differing_records(out["np_null_vector"][:, :4], x.astype(np.float64))
        rec = dc.records("sim3_largest_eigenvector")[0]
        for i, r in enumerate(rec):                                   # (one at a time: the batched form rotates every lane together)
            q = sim3_cases.jacobi_largest_eigenvector(r.reshape(1, 4, 4).astype(np.float32))[0]
            assert dc.same_bits(out["sim3_largest_eigenvector"][i, :4], q.astype(np.float64)), (i, dc.records("sim3_largest_eigenvector")[1][i])
        rec = dc.records("sim3_rotation_of_quaternion")[0]
        R = sim3_cases.rotation_of_quaternion(rec.astype(np.float32)).reshape(-1, 9)
        assert not dc.differing_records(out["sim3_rotation_of_quaternion"][:, :9], R.astype(np.float64))
        pose = mlpnp_cases._Pose(mlpnp_cases.Variant())
        for i, r in enumerate(dc.records("mlpnp_rank3")[0]):
            assert out["mlpnp_rank3"][i, 0] == pose.rank3(r.reshape(3, 3).copy()), (i, dc.records("mlpnp_rank3")[1][i])
        for i, r in enumerate(dc.records("mlpnp_eig3")[0]):
            assert dc.same_bits(out["mlpnp_eig3"][i, :9], pose.eig3(r.reshape(3, 3).copy()).reshape(-1)), (i, dc.records("mlpnp_eig3")[1][i])
        for i, r in enumerate(dc.records("mlpnp_solve6")[0]):
            assert dc.same_bits(out["mlpnp_solve6"][i, :6], pose.solve6(r[:36].reshape(6, 6), r[36:42])), (i, dc.records("mlpnp_solve6")[1][i])
        for op, nc in (("mlpnp_null_vector_12", 12), ("mlpnp_null_vector_9", 9)):
            for i, r in enumerate(dc.records(op)[0]):
                assert dc.same_bits(out[op][i, :nc], pose.smallest_vector(r.reshape(nc, nc).copy())), (op, i, dc.records(op)[1][i])


def test_the_sanitized_build_returns_the_same_bits(host_outputs):
    """the index arithmetic of the reorderings, the pivoting of the rank and the strided triangles of the factorisation on the edge
    records, under ASan / UBSan"""
    for op in dc.OPS:
        assert dc.same_bits(host_outputs["plain"][op], host_outputs["sanitized"][op]), op
