"""build.py's table of units: a unit is a row (name, source, flags, defines), and a march source's second build is a
second row over the same source, not a file.  Compiles nothing."""
from pathlib import Path

import pytest

from black_hole_ray_marching_amd import build

# the units of the library, by object stem: what --extra takes and what tools/kernel_text_cmp.py reports
UNIT_NAMES = {
    "bh_march_exact", "bh_march_exact_lat", "bh_march_fast", "bh_march_refine_lat",
    "bh_march_rays", "bh_march_rays_lat", "bh_march_rays_pose", "bh_march_rays_pose_lat",
    "bh_march_rays_org", "bh_march_rays_org_lat", "bh_march_hits", "bh_march_hits_lat",
    "bh_tiles", "bh_lens", "bh_disc", "bh_bloom", "bh_selftest",
    "bh_host", "bh_camera", "bh_bloom_host", "bh_bloom_plan", "bh_tiles_host", "bh_mirror", "bh_present",
}
# the second builds: unit -> the source it builds again
SECOND_BUILDS = {
    "bh_march_exact_lat": "bh_march_exact.hip", "bh_march_refine_lat": "bh_march_exact.hip",
    "bh_march_rays_lat": "bh_march_rays.hip", "bh_march_rays_pose_lat": "bh_march_rays_pose.hip",
    "bh_march_rays_org_lat": "bh_march_rays_org.hip", "bh_march_hits_lat": "bh_march_hits.hip",
}


def test_unit_names_are_unique_and_the_known_ones():
    names = [u.name for u in build.UNITS]
    assert len(names) == len(set(names))
    assert set(names) == UNIT_NAMES


def test_every_row_has_a_source_and_every_source_a_row():
    for u in build.UNITS:
        assert (build.CSRC / u.src).is_file(), u
    sources = {p.name for p in build.CSRC.iterdir() if p.suffix in (".hip", ".cpp")}
    assert sources == {u.src for u in build.UNITS}  # no orphan: a file that no row builds


def test_second_builds_share_a_source_and_carry_bh_lat():
    second = {u.name: u for u in build.UNITS if u.defines}
    assert {n: u.src for n, u in second.items()} == SECOND_BUILDS
    for u in second.values():
        assert "-DBH_LAT=1" in u.defines, u
        assert all(d.startswith("-D") for d in u.defines), u
    # every other unit is its source's own build: named after it, no defines, and a source has one such row at most
    first = [u for u in build.UNITS if not u.defines]
    assert all(u.name == Path(u.src).stem for u in first)
    assert len({u.src for u in first}) == len(first)
    assert {u.src for u in second.values()} <= {u.src for u in first}


def test_compile_commands(tmp_path):
    cmds = build.unit_commands(tmp_path)
    assert list(cmds) == [u.name for u in build.UNITS]
    for u in build.UNITS:
        assert cmds[u.name] == [build.HIPCC, *build.COMMON, *u.flags, *u.defines, "-c", str(build.CSRC / u.src), "-o",
                                str(tmp_path / (u.name + ".o"))]
    # --extra: after the row's own flags and defines, by name with or without the source's suffix
    for key in ("bh_march_exact_lat", "bh_march_exact_lat.hip"):
        more = build.unit_commands(tmp_path, {key: ["-DX=1"]})
        assert more["bh_march_exact_lat"] == cmds["bh_march_exact_lat"][:-4] + ["-DX=1"] + cmds["bh_march_exact_lat"][-4:]
        assert {n: c for n, c in more.items() if n != "bh_march_exact_lat"} == \
               {n: c for n, c in cmds.items() if n != "bh_march_exact_lat"}
    assert build.unit_commands(tmp_path, {"bh_host.cpp": ["-g"]})["bh_host"][-5] == "-g"


@pytest.mark.parametrize("unit", ["bh_march_nope.hip", "bh_march_nope", "bh_march_exact.cu", ""])
def test_extra_for_an_unknown_unit_raises(tmp_path, unit):
    with pytest.raises(ValueError, match="no such unit"):
        build.build_product(out_dir=tmp_path / "variant", extra={unit: ["-DX=1"]})
    assert not list((tmp_path / "variant").glob("*.o"))  # refused before anything is compiled
