"""The refusal census: every render entry point of include/bh_render.h against one table of faults, alone and in pairs.

Each of the eighteen entry points starts from an accepted call of a 16x8 frame and gets every fault of FAULTS it has a
parameter for, then every unordered pair of PAIRED; a cell is the call's status and, when that is not BH_OK, the text
of bh_last_error() without the "(file:line)" of an invalid-argument message.  tests/golden/refusals.json holds the
distinct outcomes, and per entry point the number of cells, a digest of their labels and the outcome of each: the test
asserts that its own enumeration has exactly that many cells under those labels, and compares exactly.  What a call with
two faults answers is the order of the host's checks (csrc/bh_host.cpp, render_request): nothing else pins it.

The refused calls launch nothing; the accepted ones (the bases, and the faults an entry point does not mind: fast math
for a pinhole render, say) render the 16x8 frame into buffers that hold the ss = 8 virtual frame's maps.  The device is
needed only because bh_create needs one.  The per-family refusal tests stay what they are: this one adds the coinciding
faults and the one table for all entry points.

Recording (after a deliberate change of the table or of the library's answers):
    python -m tests.test_gpu_refusals OUT.json      writes OUT.json (the golden's format) and OUT.json.txt (a line per cell)
"""
import ctypes as C
import hashlib
import itertools
import json
import re
import sys
from pathlib import Path

import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from tests._cases import camera_uniform, uniforms

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "refusals.json"
W, H, CAP = 16, 8, 16
SLOT = 256 * 1024  # bytes of each device buffer: a map of the ss = 8 virtual frame (64 x 128 x 3 floats) is 96 KiB
SLOTS = ["col0", "col1", "bo0", "bo1", "dirs", "orgs", "lens", "hits", "dbg_n_rk0", "dbg_n_rk1", "dbg_fate0",
         "dbg_fate1", "dbg_steps0", "dbg_steps1"]
N_DESCS, N_CAMS = _abi.BH_MAX_FRAMES + 4, 2 * _abi.BH_MAX_FRAMES + 8  # zeroed beyond the base call's own: never valid

# entry point -> (the rays' source, its parameters in order); `descs` is one desc where the entry takes one
ENTRIES = {
    "bh_render": ("cams", "ctx src U descs stream"),
    "bh_render_frames": ("cams", "ctx n_frames src U descs stream"),
    "bh_render_ss": ("cams", "ctx src U descs ss stream"),
    "bh_render_frames_ss": ("cams", "ctx n_frames src U descs ss stream"),
    "bh_render_shutter": ("cams", "ctx n_sub src U descs ss stream"),
    "bh_render_frames_shutter": ("cams", "ctx n_frames n_sub src U descs ss stream"),
    "bh_render_adaptive": ("cams", "ctx src U descs ad stream"),
    "bh_render_frames_adaptive": ("cams", "ctx n_frames src U descs ad stream"),
    "bh_render_lens": ("cams", "ctx src U descs lens stream"),
    "bh_render_lens_hits": ("cams", "ctx src U descs lens hits stream"),
    "bh_render_rays": ("pos", "ctx src U descs dirs ss stream"),
    "bh_render_lens_rays": ("pos", "ctx src U descs dirs lens stream"),
    "bh_render_frames_rays": ("poses", "ctx n_frames src U descs dirs ss stream"),
    "bh_render_frames_shutter_rays": ("poses", "ctx n_frames n_sub src U descs dirs ss stream"),
    "bh_render_lens_rays_posed": ("poses", "ctx src U descs dirs lens stream"),
    "bh_render_lens_rays_posed_hits": ("poses", "ctx src U descs dirs lens hits stream"),
    "bh_render_frames_rays_origins": ("poses", "ctx n_frames src U descs dirs orgs ss stream"),
    "bh_render_lens_rays_origins": ("poses", "ctx src U descs dirs orgs lens stream"),
}


def params(entry):
    p = set(ENTRIES[entry][1].split())
    return p | {"ss"} if "ad" in p else p  # an adaptive render's ss travels in its bh_adaptive_desc


def bases(entry):
    """The ss of the entry's accepted base calls."""
    p = params(entry)
    return (2,) if "ad" in p else (1, 2) if "ss" in p else (1,)


def base_state(entry, ss):
    """What the accepted base call passes; a device pointer is (slot, byte offset) or None."""
    p = params(entry)
    lens = "lens" in p
    descs = [dict(width=W, height=H, max_iters=CAP, scene_flags=bh.BH_SCENE_DEFAULT, format=bh.BH_OUT_RGBA32F,
                  math=bh.BH_MATH_EXACT, layout=bh.BH_LAYOUT_ROWMAJOR, shard_index=0, shard_count=1,
                  schedule=bh.BH_SCHED_TILE, out_col=None if lens else (f"col{i}", 0),
                  out_blackout=None if lens else (f"bo{i}", 0), dbg_n_rk=None, dbg_fate=None, dbg_steps=None)
             for i in range(2)]
    return dict(ctx=True, src=True, U=True, descs=descs, n_frames=2 if "n_frames" in p else 1,
                n_sub=2 if "n_sub" in p else 1, ss=ss, threshold=0.1, tri=False,
                dirs=("dirs", 0), orgs=("orgs", 0), lens=("lens", 0), hits=("hits", 0))


# ---- the faults: (label, the parameter or source the entry must have, what it does to the state) ---------------------
def put(key, value):
    return lambda s: s.__setitem__(key, value)


def every(**kw):
    """the fields in every desc: one fault, not also "the descs differ\""""
    return lambda s: [d.update(kw) for d in s["descs"]]


def dbg(name):
    return lambda s: [d.__setitem__(name, (f"{name}{i}", 0)) for i, d in enumerate(s["descs"])]


def misalign(key, by):
    return lambda s: s.__setitem__(key, (key, by))


def too_wide(s):
    for d in s["descs"]:
        d["width"] = 65536 // s["ss"] + 1


def second_desc(s):
    s["descs"][1]["max_iters"] = CAP + 1


MAPS = [("dirs", 1), ("orgs", 1), ("hits", 1), ("lens", 4)]  # the maps and outputs beside the desc: misaligned by
FAULTS = (
    [("ctx=NULL", None, put("ctx", None)), ("source=NULL", None, put("src", None)), ("U=NULL", None, put("U", None)),
     ("descs=NULL", None, put("descs", None))] +
    [(f"{m}=NULL", m, put(m, None)) for m, _ in MAPS] +
    [(f"{m} misaligned", m, misalign(m, by)) for m, by in MAPS] +
    [(f"ss={v}", "ss", put("ss", v)) for v in (0, 3, 16)] +
    [(f"n_sub={v}", "n_sub", put("n_sub", v)) for v in (0, 3, 32)] +
    [(f"n_frames={v}", "n_frames", put("n_frames", v)) for v in (0, _abi.BH_MAX_FRAMES + 1, 0xFFFFFFFF)] +
    [("n_frames*n_sub=258", "n_frames n_sub", put("n_frames", _abi.BH_MAX_FRAMES // 2 + 1)),
     ("width=0", None, every(width=0)), ("width*ss>65536", None, too_wide),
     ("max_iters=0", None, every(max_iters=0)), ("max_iters=65536", None, every(max_iters=65536)),
     ("format=9", None, every(format=9)), ("math=FAST", None, every(math=bh.BH_MATH_FAST)), ("math=7", None, every(math=7)),
     ("layout=TILES", None, every(layout=bh.BH_LAYOUT_TILES)), ("layout=9", None, every(layout=9)),
     ("shard_count=2", None, every(shard_count=2)), ("shard_index=shard_count", None, every(shard_index=1)),
     ("schedule=PAIR", None, every(schedule=bh.BH_SCHED_PAIR)),
     ("schedule=PERSISTENT", None, every(schedule=bh.BH_SCHED_PERSISTENT)),
     ("schedule flag 0x800", None, every(schedule=bh.BH_SCHED_TILE | 0x800)),
     ("scene_flags bit 4", None, every(scene_flags=bh.BH_SCENE_DEFAULT | 4)),
     ("out_col=NULL", "no lens", every(out_col=None)),
     ("out_col set", "lens", every(out_col=("col0", 0))), ("out_blackout set", "lens", every(out_blackout=("bo0", 0)))] +
    [(f"{n} set", None, dbg(n)) for n in ("dbg_n_rk", "dbg_fate", "dbg_steps")] +
    [("screen triangle of the last camera", "cams", put("tri", True)),
     ("second desc: max_iters", "n_frames", second_desc)])
# one fault per step of the host's checks, in every unordered pair
PAIRED = ["U=NULL", "dirs misaligned", "source=NULL", "ss=3", "n_sub=3", "n_frames=0", "width=0", "math=FAST",
          "layout=TILES", "dbg_fate set", "max_iters=0", "format=9", "schedule=PERSISTENT"]


def applies(entry, needs):
    p = params(entry) | {ENTRIES[entry][0]}
    if needs == "no lens":
        return "lens" not in p
    return all(n in p for n in (needs or "").split())


def cells(entry):
    """[(label, [what to do to the base state])]: the base, every fault alone, every pair of PAIRED."""
    have = [f for f in FAULTS if applies(entry, f[1])]
    by_label = {f[0]: f for f in have}
    # the pair list's second line: a misaligned map where the entry takes one, null cameras where it is a pinhole's
    paired = [by_label[n] for n in PAIRED if n in by_label and not (n == "source=NULL" and "dirs" in params(entry))]
    out = [("base", [])] + [(f[0], [f[2]]) for f in have]
    out += [(f"{a[0]} + {b[0]}", [a[2], b[2]]) for a, b in itertools.combinations(paired, 2)]
    return out


def labels(entry):
    return [f"ss={ss}: {label}" for ss in bases(entry) for label, _ in cells(entry)]


# ---- the calls --------------------------------------------------------------------------------------------------------
class Rig:
    """One context, the device buffers and the host arguments of every call."""

    def __init__(self, torch):
        self.torch = torch
        self.scene = bh.Scene(W, H, sky=bh.synthetic_sky(64, 32), max_iters=CAP, math=bh.BH_MATH_EXACT)
        self.lib = self.scene.lib
        self.pool = torch.zeros(len(SLOTS) * SLOT, dtype=torch.uint8, device="cuda")
        self.at = {n: self.pool.data_ptr() + i * SLOT for i, n in enumerate(SLOTS)}
        i = SLOTS.index("dirs")
        self.pool[i * SLOT:(i + 1) * SLOT].view(torch.float32).fill_(1.0)  # every direction (1, 1, 1); origins 0
        self.U = uniforms().to_c()
        self.cam = camera_uniform("B", W, H).c
        self.stream = torch.cuda.current_stream().cuda_stream

    def close(self):
        self.torch.cuda.synchronize()
        self.scene.close()

    def ptr(self, p):
        return None if p is None else self.at[p[0]] + p[1]

    def source(self, kind, s, last):
        n = 4  # the cameras of the largest base call (2 frames of 2); `last`: the last one this entry's base call reads
        if kind == "pos":
            return (C.c_float * 3)(0.0, 3.0, -20.0)
        if kind == "poses":
            ps = (_abi.bh_ray_pose * N_CAMS)()
            for i in range(n):
                ps[i] = _abi.bh_ray_pose((0.25 * i, 3.0, -20.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
            return ps
        cams = (_abi.bh_camera_uniform * N_CAMS)()
        for i in range(n):
            C.memmove(C.byref(cams[i]), C.byref(self.cam), C.sizeof(self.cam))
            cams[i].pos[0] += 0.25 * i
        if s["tri"]:
            cams[last].screen_tri[0][0] = 2.0
        return cams

    def call(self, entry, s):
        """(status, message or None) of the entry point called with what the state says"""
        kind, order = ENTRIES[entry]
        descs = None
        if s["descs"] is not None:
            descs = (_abi.bh_render_desc * N_DESCS)()
            for i, d in enumerate(s["descs"]):
                for k, v in d.items():
                    setattr(descs[i], k, self.ptr(v) if k.startswith(("out_", "dbg_")) else v)
        ad = _abi.bh_adaptive_desc(s["ss"], s["threshold"], None, None)
        b = base_state(entry, 1)
        src = self.source(kind, s, b["n_frames"] * b["n_sub"] - 1) if s["src"] else None
        value = dict(ctx=self.scene._ctx if s["ctx"] else None, src=src, U=C.byref(self.U) if s["U"] else None,
                     descs=descs, ad=C.byref(ad), stream=self.stream, n_frames=s["n_frames"], n_sub=s["n_sub"],
                     ss=s["ss"], **{m: self.ptr(s[m]) for m, _ in MAPS})
        st = getattr(self.lib, entry)(*[value[a] for a in order.split()])
        if st == _abi.BH_OK:
            return st, None
        return st, re.sub(r"\s*\([\w.]+:\d+\)$", "", self.lib.bh_last_error().decode())

    def census(self, entry):
        """the outcome of every cell of the entry, in labels(entry)'s order; one synchronisation, at the end"""
        out = []
        for ss in bases(entry):
            for _, faults in cells(entry):
                s = base_state(entry, ss)
                for f in faults:
                    f(s)
                out.append(self.call(entry, s))
        self.torch.cuda.synchronize()
        return out


def digest(entry):
    return hashlib.sha1("\n".join(labels(entry)).encode()).hexdigest()


@pytest.fixture(scope="module")
def rig():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = Rig(torch)
    yield r
    r.close()


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_table_covers_the_header():
    """the eighteen render entry points, each declared in the ABI's signature table"""
    assert len(ENTRIES) == 18 and all(e in _abi.SIGNATURES for e in ENTRIES)
    declared = {n for n in _abi.SIGNATURES if n.startswith("bh_render")}
    assert declared == set(ENTRIES)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_census(entry, rig, golden):
    g = golden["entries"][entry]
    names = labels(entry)
    assert len(names) == g["cells"] == len(g["outcome"]) and digest(entry) == g["labels_sha1"], \
        "the enumeration is not the one the golden was recorded from"
    got = rig.census(entry)
    assert got[0][0] == _abi.BH_OK, f"the base call is refused: {got[0]}"
    want = [tuple(golden["outcomes"][i]) for i in g["outcome"]]
    bad = [f"{n}: {a} != {b}" for n, a, b in zip(names, got, want) if a != b]
    assert not bad, f"{len(bad)} of {len(names)} cells differ:\n" + "\n".join(bad[:20])


def record(path):
    import torch
    r = Rig(torch)
    outcomes, entries, lines = [], {}, []
    for entry in ENTRIES:
        got = r.census(entry)
        for o in got:
            if o not in outcomes:
                outcomes.append(o)
        entries[entry] = dict(cells=len(got), labels_sha1=digest(entry), outcome=[outcomes.index(o) for o in got])
        lines += [f"{entry} | {n} -> {st}" + (f" {msg}" if msg is not None else "") for n, (st, msg) in zip(labels(entry), got)]
    r.close()
    body = ",\n".join(f' "{e}": ' + json.dumps(v, separators=(",", ":")) for e, v in entries.items())
    Path(path).write_text('{"outcomes": ' + json.dumps(outcomes, indent=1) + ',\n"entries": {\n' + body + "\n}}\n")
    Path(str(path) + ".txt").write_text("\n".join(lines) + "\n")
    print(f"{sum(v['cells'] for v in entries.values())} cells, {len(outcomes)} distinct outcomes -> {path}")


if __name__ == "__main__":
    record(sys.argv[1])
