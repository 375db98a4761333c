"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every
symbol include/pixtrack_hip.h declares (no compute without a GPU)."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def declared_symbols():
    text = (ROOT / "include" / "pixtrack_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pxt_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_expected_entry_points():
    syms = declared_symbols()
    for s in ["pxt_lm_refine", "pxt_sample_sparse", "pxt_unet_forward", "pxt_ngp_render", "pxt_depth_mask"]:
        assert s in syms


def test_library_exports_every_declared_symbol():
    from pixtrack_amd import _build, _lib

    _build.build(verbose=False)
    L = ctypes.CDLL(str(_lib.LIB_PATH))
    missing = [s for s in declared_symbols() if not hasattr(L, s)]
    assert not missing, missing


def test_binding_covers_every_declared_symbol():
    from pixtrack_amd import _lib

    assert sorted(_lib.PROTOTYPES) == declared_symbols()
    L = _lib.lib()
    assert L.pxt_version() == _lib.ABI_VERSION
    assert int(L.pxt_lm_workspace_bytes()) > 0


def test_struct_layouts_match_header_sizes():
    """ctypes mirrors must have the sizes the C compiler gives the header structs."""
    import subprocess, tempfile, textwrap
    from pixtrack_amd import _lib

    src = textwrap.dedent(
        """
        #include <stdio.h>
        #include "pixtrack_hip.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pxt_lm_level), sizeof(pxt_lm_conf),
                 sizeof(pxt_sample_level), sizeof(pxt_ngp_model), sizeof(pxt_ngp_view), sizeof(pxt_unet_layer_view));
          return 0;
        }
        """
    )
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), str(Path(d) / "s.c"), "-o", str(Path(d) / "s")])
        out = subprocess.check_output([str(Path(d) / "s")]).decode().split()
    sizes = [int(x) for x in out]
    got = [ctypes.sizeof(c) for c in (_lib.LmLevel, _lib.LmConf, _lib.SampleLevel, _lib.NgpModel, _lib.NgpView,
                                      _lib.UnetLayerView)]
    assert got == sizes


def test_product_path_refuses_cpu_tensors():
    import torch
    from pixtrack_amd import _lib
    from pixtrack_amd.optimizer import PixTrackOptimizer
    from pixtrack_amd.geometry import Camera, Pose

    opt = PixTrackOptimizer(dict(num_iters=3))
    with pytest.raises(_lib.PxtError):
        opt.run(torch.zeros(20, 3), torch.zeros(20, 32), torch.zeros(32, 8, 8),
                Pose(torch.zeros(12)), Camera(torch.zeros(8)))


def test_the_timing_instrument_build_still_compiles(tmp_path):
    """-DPXT_EXP_STAMPS=1 (in-kernel s_memtime stamps read by scripts/{conv,lm}_stamps.py) is the one
    compile-time switch left in csrc/; it is compiled here so that it cannot rot unnoticed.  (The other round-2
    experiment forks - level-major encoder, dense levels in LDS, x-pair gathers - were deleted in round 3.)"""
    import shutil
    import subprocess

    from pixtrack_amd import _build

    if shutil.which(_build.HIPCC) is None:
        import pytest

        pytest.skip("no hipcc")
    for src in _build.sources():
        if "PXT_EXP_STAMPS" not in src.read_text():
            continue
        cmd = [_build.HIPCC, *_build.FLAGS, *_build.EXTRA.get(src.stem, []), "-DPXT_EXP_STAMPS=1", "-c", str(src), "-o",
               str(tmp_path / (src.stem + ".o"))]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
    left = set()
    import re

    for f in list(_build.CSRC.glob("*.hip")) + list(_build.CSRC.glob("*.h")):
        left |= set(re.findall(r"#\s*if(?:n?def)?\s+(PXT_[A-Z_0-9]+)", f.read_text()))
    assert left <= {"PXT_EXP_STAMPS"}, left


def test_no_convolution_kernel_uses_scratch(tmp_path):
    """A conv3x3 instantiation that spills to scratch costs milliseconds per launch (scratch set-up) - it has happened
    twice (round 2: an un-unrolled step loop; round 3: hoisted blend weights).  The assembly's kernel descriptors
    are checked here so that a spill fails the CPU suite, not the frame rate."""
    import re
    import shutil
    import subprocess

    from pixtrack_amd import _build

    if shutil.which(_build.HIPCC) is None:
        import pytest

        pytest.skip("no hipcc")
    src = _build.CSRC / "pxt_unet.hip"
    cmd = [_build.HIPCC, *_build.FLAGS, "-save-temps", "-c", str(src), "-o", str(tmp_path / "u.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    asm = next(tmp_path.glob("*gfx950*.s")).read_text()
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", asm)
    conv = {n: int(sz) for n, sz in kernels if "conv3x3" in n or "conv_first" in n or "head_mfma" in n}
    assert len(conv) >= 10, sorted(conv)
    assert all(sz == 0 for sz in conv.values()), {n: sz for n, sz in conv.items() if sz}


def test_ray_generator_spills_no_sgprs(tmp_path):
    """Round 6 (profiles/r06_experiments.md section 8): beside another stream's convolution kernels single waves of the ray
    generator computed their rays slightly wrong - in every build whose ray generator spilled SGPRs into VGPR lanes
    (v_writelane_b32 / v_readlane_b32), in none that did not.  The mechanism is not established; until it is, a change that
    brings the spills back must not go unnoticed: the kernel's ISA is checked here (hipcc -S, no GPU needed)."""
    import subprocess

    from pixtrack_amd import _build

    src = _build.CSRC / "pxt_ngp.hip"
    out = tmp_path / "ngp.s"
    subprocess.check_call([_build.HIPCC, *_build.FLAGS, *_build.EXTRA.get("pxt_ngp", []), "--cuda-device-only", "-S", str(src), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    name, spills, seen = None, {}, 0
    for line in out.read_text().splitlines():
        if line.startswith("_ZN3pxt") and line.rstrip().endswith(":") or (line.startswith("_ZN3pxt") and ":" in line.split()[0]):
            name = line.split(":")[0]
            seen += "ngp_raygen_kernel" in name
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name and "ngp_raygen_kernel" in name and "v_writelane_b32" in line:
            spills[name] = spills.get(name, 0) + 1
    assert seen >= 2, "the ray generator kernels were not found in the ISA"
    assert not spills, spills
