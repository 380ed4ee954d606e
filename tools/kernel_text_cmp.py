"""Per-kernel machine-code comparison of two builds (black_hole_ray_marching_amd/_build directories): for every
object file, the gfx950 code object is taken out of the fat binary and every function symbol's bytes in
.text are hashed, so that a change which only ADDS kernels can be shown to leave each existing kernel's
machine code byte for byte as it was (tools/text_hash.sh hashes the whole .text, which any added kernel
changes).
    python tools/kernel_text_cmp.py OLD_BUILD_DIR NEW_BUILD_DIR [--match march_]
Prints one line per kernel of the old build: same / DIFFERENT / MISSING, then the kernels only the new build
has; exit status 1 if any kernel differs or is missing."""
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
    for unit in sorted({f.name for d in (args.old, args.new) for f in Path(d).glob("*.o")}):  # a new unit has new kernels only
        o, n = Path(args.old) / unit, Path(args.new) / unit
        ko, kn = kernels(o, to) if o.exists() else {}, kernels(n, tn) if n.exists() else {}
        for name, h in sorted(ko.items()):
            if args.match not in name:
                continue
            state = "MISSING" if name not in kn else "same" if kn[name] == h else "DIFFERENT"
            bad += state != "same"
            print(f"{state:9} {o.stem:20} {h} {name}")
        for name in sorted(set(kn) - set(ko)):
            if args.match in name:
                print(f"{'new':9} {o.stem:20} {kn[name]} {name}")
sys.exit(1 if bad else 0)
