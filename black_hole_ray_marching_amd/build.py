"""In-tree build of the native libraries (no cmake, no JIT cache — the .so files travel with the repo).

  black_hole_ray_marching_amd/libbh_render.so   product: HIP kernels for gfx950 + C ABI (hipcc)
  oracle/libbh_oracle.so                        test infrastructure: CPU oracle (gcc, OpenMP)

Run `python -m black_hole_ray_marching_amd.build` or call build_all().

A variant of the product for an A/B (other flags for some units, or another revision's sources) goes to a
directory of its own, from the same list of units and flags:
    python -m black_hole_ray_marching_amd.build --out DIR [--extra bh_march_exact.hip="-mllvm -amdgpu-..."]... [--csrc DIR]
writes DIR/libbh_render.so and its objects (DIR/*.o, what tools/kernel_text_cmp.py compares).

The units are the rows of UNITS: a name, a source, flags and defines.  A unit's name is its object's stem
(bh_march_exact_lat); --extra takes it with or without the source's suffix (bh_march_exact_lat.hip too).  Two rows may
build one source: a march source's second build is a row with -DBH_LAT=1, not a file.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import NamedTuple

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
OBJ = PKG / "_build"
LIB = PKG / "libbh_render.so"
ORACLE_SRCS = [ROOT / "oracle" / "bh_oracle.c", ROOT / "oracle" / "bh_bloom_oracle.c"]
EXAMPLE_SRC = ROOT / "examples" / "render_frame.c"
EXAMPLE_BIN = ROOT / "examples" / "render_frame"
ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
ORACLE_LIB = ROOT / "oracle" / "libbh_oracle.so"

ARCH = os.environ.get("BH_OFFLOAD_ARCH", "gfx950")
HIPCC = os.environ.get("HIPCC", shutil.which("hipcc") or "/opt/rocm/bin/hipcc")

COMMON = ["-O3", "-fPIC", "-std=c++17", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function"]
# The exact kernels' arithmetic: one rounding per op, IEEE division and square root.  No SLP packing: packed FP32 has
# no throughput advantage on gfx950 (tools/ubench/valu_rates.hip).  Alone, these are the flags of the scheduled builds
# (LLVM's machine schedulers: shorter per-step latency for tail-bound frames).
EXACT = ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize"]
# The issue-order builds.  No machine scheduling (pre- or post-RA): the step's source order issues faster than the
# scheduler's interleavings (0.687 -> 0.644 ms headline, A/B r01).  No machine LICM: it hoists
# loop-invariant materialisations (e.g. the shading's f64 constants) out of the frame-independent loops and lengthens
# live ranges; off, 0.6226 -> 0.6168 ms per frame headline, 1920x1080 0.162 -> 0.159 ms (A/B r02,
# profiles/r02b/ab_nolicm.log; the scheduled builds got slower with it, 0.736 -> 0.768 ms at cap 1000, so they keep
# LICM).
EXACT_ISSUE_ORDER = EXACT + ["-mllvm", "-enable-misched=0", "-mllvm", "-enable-post-misched=0",
                             "-mllvm", "-disable-machine-licm"]
# The second build of a march source: the machine schedulers' build (EXACT alone), its namespace and its packed tail
# step chosen in the source by BH_LAT (csrc/bh_march.hpp).
LAT = ["-DBH_LAT=1"]


class Unit(NamedTuple):
    """One translation unit of the product: a compile command.  name: the object's stem, what --extra takes and what
    tools/kernel_text_cmp.py and tools/kernel_resources.py report; src: its source in csrc/ (several rows may build
    one source); flags: its floating-point contract and scheduling options (DESIGN.md "Math modes"); defines: the
    -D options that pick a second build of the source."""
    name: str
    src: str
    flags: list[str]
    defines: list[str] = []


UNITS = [
    # the march (bh_render and its forms): the issue-order build, and the scheduled one over the same source
    Unit("bh_march_exact", "bh_march_exact.hip", EXACT_ISSUE_ORDER),
    Unit("bh_march_exact_lat", "bh_march_exact.hip", EXACT, LAT),
    # the fast (tolerance) kernels: no machine scheduling either (0.468 -> 0.440 ms headline, A/B r01)
    Unit("bh_march_fast", "bh_march_fast.hip", ["-ffp-contract=fast", "-fno-hip-fp32-correctly-rounded-divide-sqrt",
                                 "-mllvm", "-enable-misched=0", "-mllvm", "-enable-post-misched=0"]),
    # the scheduled build of the adaptive render's work-list march alone, without machine LICM (see the source)
    Unit("bh_march_refine_lat", "bh_march_exact.hip", EXACT + ["-mllvm", "-disable-machine-licm"],
         LAT + ["-DBH_REFINE_ONLY=1"]),
    # the ray-map march (bh_render_rays), the posed one (bh_render_frames_rays, its shutter and lens forms) and the
    # one with an origin map (bh_render_frames_rays_origins, its lens form): the two exact builds of a source each
    Unit("bh_march_rays", "bh_march_rays.hip", EXACT_ISSUE_ORDER),
    Unit("bh_march_rays_lat", "bh_march_rays.hip", EXACT, LAT),
    Unit("bh_march_rays_pose", "bh_march_rays_pose.hip", EXACT_ISSUE_ORDER),
    Unit("bh_march_rays_pose_lat", "bh_march_rays_pose.hip", EXACT, LAT),
    Unit("bh_march_rays_org", "bh_march_rays_org.hip", EXACT_ISSUE_ORDER),
    Unit("bh_march_rays_org_lat", "bh_march_rays_org.hip", EXACT, LAT),
    # the lens march with a hit map (bh_render_lens_hits, bh_render_lens_rays_posed_hits): the same two builds
    Unit("bh_march_hits", "bh_march_hits.hip", EXACT_ISSUE_ORDER),
    Unit("bh_march_hits_lat", "bh_march_hits.hip", EXACT, LAT),
    Unit("bh_tiles", "bh_tiles.hip", []),
    # the lens shades and the sky chain: the march kernels' shading arithmetic, one rounding per op (bh_lens.hpp)
    Unit("bh_lens", "bh_lens.hip", EXACT),
    # the disc shade (bh_shade_lens_disc): the same contract, in a unit of its own beside the shades it extends
    Unit("bh_disc", "bh_disc.hip", EXACT),
    # post-RA scheduling off: fused bloom chain 0.556 -> 0.548 ms (A/B r01; pre-RA off too: 0.561)
    # no SLP vectorisation: packed-FP32 forms of the filter's adjacent channel ops cost more than the
    # scalar ops on gfx950 (a v_pk op issues slower than two scalar ones, plus the shuffles and hazard
    # nops around it) and hold more VGPRs
    Unit("bh_bloom", "bh_bloom.hip", ["-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-enable-post-misched=0",
                            "-mllvm", "-pragma-unroll-threshold=200000"]),  # the quad pass's 8 taps x 9 read forms
    Unit("bh_selftest", "bh_selftest.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),
    # the host side of the ABI: arithmetic whose bits are tested (camera, frame constants, bloom plans, mirrors)
    Unit("bh_host", "bh_host.cpp", ["-ffp-contract=off", "-x", "hip"]),
    Unit("bh_camera", "bh_camera.cpp", ["-ffp-contract=off", "-x", "hip"]),
    Unit("bh_bloom_host", "bh_bloom_host.cpp", ["-ffp-contract=off", "-x", "hip"]),
    # plain C++ (no HIP): the bloom's plan builders replay the kernels' f32 arithmetic, IEEE and uncontracted
    Unit("bh_bloom_plan", "bh_bloom_plan.cpp", ["-ffp-contract=off"]),
    Unit("bh_tiles_host", "bh_tiles_host.cpp", ["-ffp-contract=off", "-x", "hip"]),
    Unit("bh_mirror", "bh_mirror.cpp", ["-ffp-contract=off", "-x", "hip"]),
    Unit("bh_present", "bh_present.cpp", ["-x", "hip"]),
]


def unit_commands(obj_dir: Path, extra: dict[str, list[str]] | None = None, csrc: Path = CSRC) -> dict[str, list[str]]:
    """Every unit's compile command, by name.  extra: per unit, flags after the row's own; a key is a unit's name,
    with or without its source's suffix (bh_march_exact_lat, bh_march_exact_lat.hip).  ValueError for any other."""
    names = {u.name for u in UNITS}
    more: dict[str, list[str]] = {}
    for key, flags in (extra or {}).items():
        name = key.removesuffix(".hip").removesuffix(".cpp")
        if name not in names:
            raise ValueError(f"no such unit: {key!r} (units: {sorted(names)})")
        more[name] = more.get(name, []) + flags
    return {u.name: [HIPCC, *COMMON, *u.flags, *u.defines, *more.get(u.name, []), "-c", str(csrc / u.src), "-o",
                     str(obj_dir / (u.name + ".o"))] for u in UNITS}


def _run(cmd: list[str]) -> None:
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"build step failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout}")


def _stale(target: Path, deps: list[Path]) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(d.stat().st_mtime > t for d in deps)


def build_product(force: bool = False, out_dir: Path | None = None, extra: dict[str, list[str]] | None = None,
                  csrc: Path = CSRC) -> Path:
    """The product library.  out_dir: objects and library into that directory instead of the package (a variant
    build); extra: per unit, flags after its row's own (unit_commands); csrc: another tree's sources (with
    ../../include beside it)."""
    obj_dir = Path(out_dir) if out_dir else OBJ
    lib = obj_dir / LIB.name if out_dir else LIB
    commands = unit_commands(obj_dir, extra, csrc)
    obj_dir.mkdir(parents=True, exist_ok=True)
    headers = list(csrc.glob("*.hpp")) + [csrc.parent.parent / "include" / "bh_render.h"]
    objs, jobs = [], []
    for u in UNITS:
        o = obj_dir / (u.name + ".o")
        if force or _stale(o, [csrc / u.src, *headers, Path(__file__)]):
            jobs.append(commands[u.name])
        objs.append(o)
    # the translation units compile independently: in parallel (BH_BUILD_JOBS, default min(cpus, 8))
    n = int(os.environ.get("BH_BUILD_JOBS", "0")) or min(os.cpu_count() or 1, 8)
    with ThreadPoolExecutor(max_workers=max(1, n)) as ex:
        list(ex.map(_run, jobs))
    if force or _stale(lib, objs):
        tmp = lib.with_suffix(".so.tmp")
        _run([HIPCC, "-shared", f"--offload-arch={ARCH}", "-o", str(tmp), *map(str, objs)])
        os.replace(tmp, lib)
    return lib


def build_oracle(force: bool = False) -> Path:
    if force or _stale(ORACLE_LIB, [*ORACLE_SRCS, ROOT / "include" / "bh_render.h", Path(__file__)]):
        tmp = ORACLE_LIB.with_suffix(".so.tmp")
        # -O3 -ffp-contract=off (no fast-math: the golden tests prove the bits unchanged)
        _run(["gcc", "-O3", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC",
              "-shared", "-o", str(tmp), *map(str, ORACLE_SRCS), "-lm"])
        os.replace(tmp, ORACLE_LIB)
    return ORACLE_LIB


def build_example(force: bool = False) -> Path:
    """examples/render_frame: a plain C11 host of the C ABI (gcc + the HIP runtime's C API, no torch)."""
    if force or _stale(EXAMPLE_BIN, [EXAMPLE_SRC, ROOT / "include" / "bh_render.h", LIB, Path(__file__)]):
        tmp = EXAMPLE_BIN.with_suffix(".tmp")
        _run(["gcc", "-std=c11", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", f"-I{ROOT / 'include'}",
              f"-I{ROCM / 'include'}", str(EXAMPLE_SRC), "-o", str(tmp), f"-L{PKG}", "-lbh_render",
              f"-L{ROCM / 'lib'}", "-lamdhip64", "-Wl,-rpath,$ORIGIN/../black_hole_ray_marching_amd",
              f"-Wl,-rpath,{ROCM / 'lib'}", "-lm"])
        os.replace(tmp, EXAMPLE_BIN)
    return EXAMPLE_BIN


def build_all(force: bool = False) -> None:
    build_product(force)
    build_oracle(force)
    build_example(force)


if __name__ == "__main__":
    import argparse
    import shlex

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--force", action="store_true", help="rebuild everything")
    ap.add_argument("--out", type=Path, help="build only the product library, into this directory (a variant)")
    ap.add_argument("--extra", action="append", default=[], metavar='UNIT="FLAGS"',
                    help="with --out: more flags for one unit, after its own (may repeat)")
    ap.add_argument("--csrc", type=Path, default=CSRC, help="with --out: the csrc directory of another tree")
    args = ap.parse_args()
    if args.out:
        extra = {u: shlex.split(f) for u, _, f in (e.partition("=") for e in args.extra)}
        print(build_product(args.force, args.out, extra, args.csrc.resolve()))
    else:
        if args.extra or args.csrc != CSRC:
            ap.error("--extra and --csrc build a variant: give --out")
        build_all(force=args.force)
        print(LIB)
        print(ORACLE_LIB)
