"""The register budget of every bvh_pixels instantiation (rt_bvh.hip), read from the metadata the compiler writes for gfx950.
The 8- and 12-wave forms live on six waves per SIMD, which 80 VGPRs buy ("Occupancy"); the tile's primary directions
(`tile_dir`, three registers that live across walks) were paid for out of the path state, not with more registers or scratch.
The bounds are the figures of the build before `tile_dir`:

    8- / 12-wave, LDS nodes, flat sky      80 VGPRs,  8 bytes of scratch
    8-wave, global nodes, flat sky         80 VGPRs, 12 bytes
    8- / 12-wave, textured sky             80 VGPRs,  0 bytes
    16-wave                                89 VGPRs,  0 bytes"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-fast-math -Wall -Wno-unused-function -ffp-contract=off -fno-slp-vectorize".split()

# _ZN3rtk10bvh_pixelsILi8ELb1ELb1ELi12ELb1EEEv...: WAVES, SGN, NLDS, CAP, FLAT
NAME = re.compile(r"bvh_pixelsILi(\d+)ELb([01])ELb([01])ELi(\d+)ELb([01])EEE")


def bound(waves, nlds, flat):
    if waves == 16:
        return 89, 0
    if not flat:
        return 80, 0
    return (80, 8) if nlds else (80, 12)


def kernels_of(asm):
    """{(WAVES, SGN, NLDS, CAP, FLAT): (vgprs, scratch bytes)} from the amdhsa.kernels metadata of an assembly file."""
    meta = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry)
        m = name and NAME.search(name.group(1))
        if not m:
            continue
        key = (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)))
        out[key] = (int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)),
                    int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1)))
    return out


@pytest.fixture(scope="module")
def product_kernels(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bvh_regs") / "rt_bvh.s")
    r = subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", out,
                        os.path.join(ROOT, "compute_raytracer_amd", "csrc", "rt_bvh.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return kernels_of(open(out).read())


def test_every_form_is_there(product_kernels):
    # launch_bvh's ladder: 8 / 12 / 12 with short lists / 16 / 16 with short lists / global nodes, each under either node test and sky
    forms = {(w, nlds, cap) for (w, sgn, nlds, cap, flat) in product_kernels}
    assert forms == {(8, 1, 12), (12, 1, 12), (12, 1, 6), (16, 1, 12), (16, 1, 6), (8, 0, 8)}, forms
    assert len(product_kernels) == 24, sorted(product_kernels)


def test_no_form_exceeds_its_registers_or_scratch(product_kernels):
    over = {}
    for key, (vgprs, scratch) in sorted(product_kernels.items()):
        waves, sgn, nlds, cap, flat = key
        v, s = bound(waves, nlds, flat)
        print("bvh_pixels<%d, %d, %d, %d, %d>: %d VGPRs, %d bytes of scratch (bounds %d, %d)" % (key + (vgprs, scratch, v, s)))
        if vgprs > v or scratch > s:
            over[key] = (vgprs, scratch, v, s)
    assert not over, over


def test_the_parser_reads_the_metadata():
    text = "\n".join(["amdhsa.kernels:", "  - .args: []", "    .name:           _ZN3rtk10bvh_pixelsILi8ELb1ELb0ELi8ELb1EEEvK11RtFrameArgs",
                      "    .private_segment_fixed_size: 12", "    .vgpr_count:     80",
                      "  - .args: []", "    .name:           _ZN3rtk11sky_resolveE11RtFrameArgs", "    .private_segment_fixed_size: 0", "    .vgpr_count:     40"])
    assert kernels_of(text) == {(8, 1, 0, 8, 1): (80, 12)}
    assert bound(8, 0, 1) == (80, 12) and bound(12, 1, 1) == (80, 8) and bound(12, 1, 0) == (80, 0) and bound(16, 1, 1) == (89, 0)
