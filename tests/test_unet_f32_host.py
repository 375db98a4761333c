"""CPU checks of the UNet's fp32 option: the fp32 weight pack, the C ABI's new entry points (header, exports, ctypes
table) and the --unet_precision flags of the r9 and multi-object command lines."""
import re
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

from pixtrack_amd import _lib
from pixtrack_amd.unet import (HEAD_INPUTS, OUTPUT_DIMS, conv_layer_dims, conv_layer_names, make_synthetic_unet_weights,
                               pack_unet_weights)

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["pxt_unet_create_f32", "pxt_unet_precision", "pxt_conv3x3_nhwc_f32"]


def _arrays(blob):
    n_conv, n_heads = struct.unpack_from("<ii", blob, 8)
    dims = struct.unpack_from(f"<{2 * (n_conv + n_heads)}i", blob, 16)
    off = 16 + 8 * (n_conv + n_heads)
    table = struct.unpack_from(f"<{4 * (n_conv + n_heads)}q", blob, off)
    return n_conv, n_heads, dims, [(table[2 * i], table[2 * i + 1]) for i in range(2 * (n_conv + n_heads))]


def test_fp32_pack_size_and_layout():
    w = make_synthetic_unet_weights(7, bn_trivial=False)
    b16, b32 = pack_unet_weights(w), pack_unet_weights(w, precision="fp32")
    assert b16[:8] == b"PXTUNET1" and b32[:8] == b"PXTUNF32"
    n_conv, n_heads, dims, arrays = _arrays(b32)
    assert (n_conv, n_heads) == (17, 3)
    assert list(zip(dims[0:34:2], dims[1:34:2])) == conv_layer_dims()
    assert list(zip(dims[34::2], dims[35::2])) == list(zip(HEAD_INPUTS, OUTPUT_DIMS))
    n_params = 0
    for li, (cin, cout) in enumerate(conv_layer_dims()):
        (ow, nw), (ob, nb) = arrays[2 * li], arrays[2 * li + 1]
        assert nw == cout * 9 * cin * 4 and nb == cout * 4 and ow % 16 == 0 and ob % 16 == 0
        n_params += cout * 9 * cin
    assert len(b32) >= 4 * n_params
    # every 3x3 filter [cout][ky][kx][cin] in float32; decoders carry the folded BatchNorm, in fp32
    name = conv_layer_names()[14]
    cin, cout = conv_layer_dims()[14]
    s = w[f"{name}.bn_weight"] / torch.sqrt(w[f"{name}.bn_var"] + 1e-5)
    want = (w[f"{name}.weight"] * s[:, None, None, None]).permute(0, 2, 3, 1).contiguous().numpy()
    ow, nw = arrays[28]
    got = np.frombuffer(b32, np.float32, nw // 4, ow).reshape(cout, 3, 3, cin)
    np.testing.assert_array_equal(got, want.astype(np.float32))
    # the fp16 pack keeps its layout: same header and table shape, half the bytes per 3x3 weight after layer 0
    _, _, dims16, arrays16 = _arrays(b16)
    assert dims16 == dims and arrays16[2][1] * 2 == arrays[2][1]
    with pytest.raises(ValueError):
        pack_unet_weights(w, precision="bf16")


def test_new_entry_points_in_header_library_and_binding():
    from pixtrack_amd import _build

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pixtrack_hip.h").read_text(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", text), s
        assert s in _lib.PROTOTYPES, s
    _build.build(verbose=False)
    L = _lib.lib()
    assert L.pxt_version() == _lib.ABI_VERSION == 13
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s
    assert L.pxt_unet_precision(None) < 0


def test_create_f32_refuses_an_fp16_pack():
    import ctypes as C

    L = _lib.lib()
    w = make_synthetic_unet_weights(7)
    ctx = C.c_void_p()
    b16 = pack_unet_weights(w)
    assert L.pxt_unet_create_f32(b16, len(b16), C.byref(ctx)) == -1  # PXT_E_ARG before any device call
    b32 = bytearray(pack_unet_weights(w, precision="fp32"))
    assert L.pxt_unet_create_f32(bytes(b32[:4096]), 4096, C.byref(ctx)) == -1  # truncated


class _Stop(Exception):
    pass


def _capture(monkeypatch, module):
    seen = {}

    def fake(*a, **k):
        seen.update(k)
        raise _Stop

    monkeypatch.setattr(module, "PixLocPoseTrackerR9", fake)
    return seen


@pytest.mark.parametrize("flag,want", [([], "fp16"), (["--unet_precision", "fp32"], "fp32"),
                                       (["--unet_precision", "fp16"], "fp16")])
def test_r9_cli_unet_precision(monkeypatch, tmp_path, flag, want):
    from pixtrack_amd.pose_trackers import pixloc_tracker_r9 as r9

    monkeypatch.setattr(r9.torch.cuda, "is_available", lambda: False)
    seen = _capture(monkeypatch, r9)
    with pytest.raises(_Stop):
        r9.main(["--object_path", str(tmp_path), "--query", str(tmp_path), "--out_dir", str(tmp_path / "o")] + flag)
    assert seen["unet_precision"] == want


@pytest.mark.parametrize("flag,want", [([], "fp16"), (["--unet_precision", "fp32"], "fp32")])
def test_multi_object_cli_unet_precision(monkeypatch, tmp_path, flag, want):
    from pixtrack_amd.pose_trackers import multi_object_tracker as mo

    monkeypatch.setattr(mo.torch.cuda, "is_available", lambda: False)
    seen = _capture(monkeypatch, mo)
    with pytest.raises(_Stop):
        mo.main(["--object_path", str(tmp_path), "--query", str(tmp_path), "--out_dir", str(tmp_path / "o"),
                 "--obj_aabb", "[[0,0,0],[1,1,1]]", "--upright_ref_img", "a.png"] + flag)
    assert seen["unet_precision"] == want


def test_cli_refuses_an_unknown_precision(tmp_path):
    from pixtrack_amd.pose_trackers import pixloc_tracker_r9 as r9

    with pytest.raises(SystemExit):
        r9.main(["--object_path", str(tmp_path), "--query", str(tmp_path), "--out_dir", str(tmp_path / "o"),
                 "--unet_precision", "fp8"])
