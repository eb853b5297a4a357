"""The scenes of tests/test_fast_emission_gpu.py do to the FAST kernel what they are meant to: checked here on the CPU, from the
host's cell table and the oracle's candidate lists alone (tests/fast_emission_scenes.py has the scenes and the arithmetic)."""
import pytest

import fast_emission_scenes as fes


@pytest.mark.parametrize("name", fes.NAMES)
def test_scene_produces_its_situation(msorb_mod, oracle, name):
    s = fes.scenes(msorb_mod, oracle)[name]
    assert len(s["cand"][0]) > 0
    fes.check(name, s)


def test_geometries_route_to_both_workgroup_shapes(msorb_mod):
    small, large = fes.cell_table(msorb_mod, fes.SMALL, 128), fes.cell_table(msorb_mod, fes.LARGE, 256)
    assert fes.threads_of(small) == 128 and fes.threads_of(large) == 256
    assert len({c["y0"] for c in large if c["level"] == 0}) == 1 and max(c["rh"] for c in large) > 57, "one row of tall cells"
    assert fes.SMALL[1] % 4 and fes.LARGE[1] % 4, "tightly packed rows are not 4-byte aligned: the byte-granular variant"
    wide = fes.cell_table(msorb_mod, fes.WIDE, 256)
    assert fes.threads_of(wide) == 256 and fes.WIDE[1] % 4 and max(c["x_hi"] - c["gx0"] for c in wide) > 64, "a third bitmap word"
    # both ways of dealing rows, each with a level-0 cell that has rows to spare
    assert {fes.by_wave(c, 128) for c in small if c["level"] == 0 and fes.spare_row_threads(c, 128)} == {0, 1}
