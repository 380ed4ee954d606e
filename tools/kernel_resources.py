"""Registers, LDS and scratch of a build's kernels, from the gfx950 code objects' metadata (no GPU):
    python tools/kernel_resources.py BUILD_DIR UNIT[:MATCH] [UNIT[:MATCH] ...]
For every named object file (bh_march_rays_pose.o, ...) one line per kernel whose mangled name contains MATCH: VGPRs,
SGPRs, static LDS bytes, scratch bytes, spilled registers and the waves per SIMD its VGPRs allow (512 VGPRs, granule 8,
at most 8)."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")
FIELDS = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"),
          ("scratch", ".private_segment_fixed_size"), ("spilled", ".vgpr_spill_count"), ("sgpr_spilled", ".sgpr_spill_count"))


def kernels(obj: Path, tmp: Path) -> list[dict]:
    fb, co = tmp / (obj.stem + ".fb"), tmp / (obj.stem + ".co")
    subprocess.run([LLVM / "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb], check=True)
    subprocess.run([LLVM / "clang-offload-bundler", "--unbundle", "--type=bc",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}", f"--output={co}"], check=True)
    notes = subprocess.run([LLVM / "llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out = []
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        k = {"name": re.search(r"\.name:\s+(\S+)", block).group(1)}
        for key, field in FIELDS:
            k[key] = int(re.search(rf"{re.escape(field)}:\s+(\d+)", block).group(1))
        out.append(k)
    return sorted(out, key=lambda k: k["name"])


def main() -> None:
    build = Path(sys.argv[1])
    with tempfile.TemporaryDirectory() as t:
        for spec in sys.argv[2:]:
            unit, _, match = spec.partition(":")
            ks = [k for k in kernels(build / unit, Path(t)) if match in k["name"]]
            print(f"{unit}: {len(ks)} kernels" + (f" matching {match}" if match else ""))
            for k in ks:
                waves = min(8, 512 // (-(-k["vgpr"] // 8) * 8))
                print(k["name"] + "  " + " ".join(f"{key} {k[key]}" for key, _ in FIELDS) + f" waves/SIMD {waves}")


if __name__ == "__main__":
    main()
