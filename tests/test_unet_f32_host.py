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
NEW_SYMBOLS = ["pxt_unet_create_f32", "pxt_unet_precision", "pxt_conv3x3_nhwc_f32", "pxt_conv3x3_f32_cfg",
               "pxt_conv3x3_nhwc_f32_cfg", "pxt_unet_layer_views_f32"]


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


def _tiles(H, W):
    return ((H + 15) // 16) * ((W + 15) // 16)


def test_conv3x3_f32_cfg_at_the_thresholds_and_production_sizes():
    """pxt_conv3x3_f32_cfg (the function launch_conv itself asks): 1 = <2,2,2,2>, 2 = <2,1,2,2>, 3 = <2,2,1,4>,
    4 = <2,1,1,4>, 5 = <1,2,1,4>.  The large-map configurations start at tiles * 2 * (Cout / 128) >= 1024 and
    tiles * (Cout / 64) >= 1024, tiles counted as 16 x 16 with partial ones."""
    cfg = _lib.lib().pxt_conv3x3_f32_cfg
    # Cout = 512: 128 tiles and up
    for H, W, tiles, want in [(16, 127 * 16, 127, 2), (16, 127 * 16 + 1, 128, 1), (16, 128 * 16, 128, 1), (125, 240, 120, 2),
                              (125, 250, 128, 1), (113, 241, 128, 1), (112, 241, 112, 2)]:
        assert _tiles(H, W) == tiles and cfg(H, W, 512) == want, (H, W)
    # Cout = 64: 1024 tiles and up
    assert _tiles(33 * 16, 31 * 16) == 1023 and _tiles(512, 512) == 1024 and _tiles(497, 497) == 1024
    assert cfg(33 * 16, 31 * 16, 64) == 4 and cfg(512, 512, 64) == 3 and cfg(497, 497, 64) == 3
    assert cfg(33 * 16, 31 * 16 + 1, 64) == 3  # one column more: 33 x 32 tiles
    # the channel groups count: Cout = 192 is three groups of 64, Cout = 256 two of 128
    assert _tiles(273, 290) == 342 and cfg(273, 290, 192) == 3 and cfg(272, 288, 192) == 4  # 342 x 3 / 306 x 3
    assert cfg(16, 255 * 16, 256) == 2 and cfg(16, 256 * 16, 256) == 1
    # no multiple of 64: one configuration at any size
    for cout in (96, 160, 32):
        for H, W in [(1, 1), (75, 100), (480, 640), (4096, 4096)]:
            assert cfg(H, W, cout) == 5, (H, W, cout)
    # production: 640 x 480 block 0, 1024 x 576 block 1, 320 x 240 at 128 channels
    assert cfg(480, 640, 64) == 3 and cfg(288, 512, 128) == 1 and cfg(240, 320, 128) == 2
    assert cfg(576, 1024, 64) == 3 and cfg(240, 320, 64) == 4
    # what launch_conv refuses
    for H, W, cout in [(0, 16, 64), (16, 0, 64), (-1, 16, 64), (16, 16, 0), (16, 16, 16), (16, 16, 48), (16, 16, -64),
                       (16, 16, 100)]:
        assert cfg(H, W, cout) == -1, (H, W, cout)


def test_forced_configuration_entry_refuses_before_any_device_call():
    """pxt_conv3x3_nhwc_f32_cfg: a configuration out of range or one whose channel span (128 / 128 / 64 / 64 / 32) does not
    divide Cout is PXT_E_ARG, like a null pointer or a bad shape - all before the first device call."""
    L = _lib.lib()
    p = 256  # (never dereferenced: every call below is refused)

    def call(H=16, W=16, cin=16, cout=128, cfg=0, x=p, w=p, b=p, o=p):
        return L.pxt_conv3x3_nhwc_f32_cfg(x, H, W, cin, w, b, cout, 1, o, cfg, None)

    assert call(cfg=-1) == -1 and call(cfg=6) == -1
    for cfg, cout in [(1, 64), (2, 64), (1, 192), (2, 96), (3, 96), (4, 32), (3, 160), (4, 160)]:
        assert call(cfg=cfg, cout=cout) == -1, (cfg, cout)
    for cfg in range(6):
        assert call(cfg=cfg, cin=8) == -1 and call(cfg=cfg, cin=24) == -1 and call(cfg=cfg, cout=48) == -1
        assert call(cfg=cfg, H=0) == -1 and call(cfg=cfg, W=0) == -1
        assert call(cfg=cfg, x=None) == -1 and call(cfg=cfg, w=None) == -1 and call(cfg=cfg, b=None) == -1
        assert call(cfg=cfg, o=None) == -1
    assert L.pxt_conv3x3_nhwc_f32(p, 16, 16, 8, p, p, 128, 1, p, None) == -1  # the old entry: the same checks
    out = (_lib.UnetLayerView * 22)()
    assert L.pxt_unet_layer_views_f32(None, 1, 64, 64, out) == -1


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
