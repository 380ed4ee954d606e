"""Per-kernel machine-code comparison of two builds (black_hole_ray_marching_amd/_build directories): for every
object file, the gfx950 code object is taken out of the fat binary and every function symbol's bytes in
.text are hashed, so that a change which only ADDS kernels can be shown to leave each existing kernel's
machine code byte for byte as it was (tools/text_hash.sh hashes the whole .text, which any added kernel
changes).
    python tools/kernel_text_cmp.py OLD_BUILD_DIR NEW_BUILD_DIR [--match march_]
Prints one line per kernel of the old build: same / DIFFERENT / MISSING, then the kernels only the new build
has; a function of a unit that the new build no longer has is matched by name in its other units ("moved to");
exit status 1 if any kernel differs or is missing."""
import argparse
import hashlib
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")


def kernels(obj: Path, tmp: Path) -> dict:
    """function symbol -> sha256 of its bytes, for the gfx950 code object bundled in `obj`"""
    fb, co, text = tmp / (obj.stem + ".fb"), tmp / (obj.stem + ".co"), tmp / (obj.stem + ".text")
    subprocess.run([LLVM / "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb], check=True)
    if not fb.exists() or fb.stat().st_size == 0:
        return {}
    subprocess.run([LLVM / "clang-offload-bundler", "--unbundle", "--type=bc",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}", f"--output={co}"], check=True)
    subprocess.run([LLVM / "llvm-objcopy", "-O", "binary", "--only-section=.text", co, text], check=True)
    data = text.read_bytes()
    base = None
    for line in subprocess.run([LLVM / "llvm-readelf", "-S", "--wide", co], check=True, capture_output=True,
                               text=True).stdout.splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 3 and f[1] == ".text":
            base = int(f[3], 16)
    out = {}
    for line in subprocess.run([LLVM / "llvm-readelf", "--symbols", "--wide", co], check=True, capture_output=True,
                               text=True).stdout.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[6] != "UND":
            addr, size = int(f[1], 16), int(f[2], 0)
            out[f[7]] = hashlib.sha256(data[addr - base:addr - base + size]).hexdigest()[:16] + f" {size}"
    return out


p = argparse.ArgumentParser()
p.add_argument("old")
p.add_argument("new")
p.add_argument("--match", default="", help="only kernels whose (mangled) name contains this")
args = p.parse_args()
bad = 0
with tempfile.TemporaryDirectory() as t:
    to, tn = Path(t) / "old", Path(t) / "new"
    to.mkdir()
    tn.mkdir()
    units = sorted({f.name for d in (args.old, args.new) for f in Path(d).glob("*.o")})  # a new unit has new kernels only
    old = {u: kernels(Path(args.old) / u, to) if (Path(args.old) / u).exists() else {} for u in units}
    new = {u: kernels(Path(args.new) / u, tn) if (Path(args.new) / u).exists() else {} for u in units}
    # a unit the new build no longer has: its functions are looked up by name in the new build's other units
    gone = [u for u in units if not (Path(args.new) / u).exists()]
    moved = {name: u for u in units for name in new[u] if any(name in old[g] for g in gone) and name not in old[u]}
    for unit in units:
        stem = Path(unit).stem
        for name, h in sorted(old[unit].items()):
            if args.match not in name:
                continue
            at = moved[name] if unit in gone and name in moved else unit
            state = "MISSING" if name not in new[at] else "same" if new[at][name] == h else "DIFFERENT"
            bad += state != "same"
            print(f"{state:9} {stem:20} {h} {name}" + (f"  (moved to {Path(at).stem})" if at != unit else ""))
        for name in sorted(set(new[unit]) - set(old[unit]) - set(moved)):
            if args.match in name:
                print(f"{'new':9} {stem:20} {new[unit][name]} {name}")
sys.exit(1 if bad else 0)
