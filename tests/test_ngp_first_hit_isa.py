"""CPU check of the first-hit kernels' ISA, the twin of tests/test_abi.py::test_ray_generator_spills_no_sgprs: the ray
generator's wrong rays beside another stream's kernels appeared in every build that spilled SGPRs into
VGPR lanes.  The first-hit kernels rebuild rays from the same camera loads, so they are held to the same rule: no
v_writelane_b32 / v_readlane_b32, no scratch (hipcc -S for gfx950, no GPU needed)."""
import re
import shutil
import subprocess

import pytest


def test_first_hit_kernels_spill_no_sgprs(tmp_path):
    from pixtrack_amd import _build

    if shutil.which(_build.HIPCC) is None:
        pytest.skip("no hipcc")
    src = _build.CSRC / "pxt_ngp.hip"
    out = tmp_path / "ngp.s"
    subprocess.check_call([_build.HIPCC, *_build.FLAGS, *_build.EXTRA.get("pxt_ngp", []), "--cuda-device-only", "-S", str(src),
                           "-o", str(out)], stderr=subprocess.DEVNULL)
    asm = out.read_text()
    name, lane_moves, seen = None, {}, set()
    for line in asm.splitlines():
        if line.startswith("_ZN3pxt") and ":" in line.split()[0]:
            name = line.split(":")[0]
            if "ngp_first_hit_kernel" in name:
                seen.add(name)
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name and "ngp_first_hit_kernel" in name and ("v_writelane_b32" in line or "v_readlane_b32" in line):
            lane_moves[name] = lane_moves.get(name, 0) + 1
    assert len(seen) == 2, "the first-hit kernels (_v and _m) were not found in the ISA: %s" % sorted(seen)
    assert not lane_moves, lane_moves
    meta = re.findall(r"\.name:\s+(\S*ngp_first_hit_kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                      r"(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", asm)
    assert len(meta) == 2, meta
    for kernel, scratch, sgpr_spills, vgpr_spills in meta:
        assert (int(scratch), int(sgpr_spills), int(vgpr_spills)) == (0, 0, 0), (kernel, scratch, sgpr_spills, vgpr_spills)
