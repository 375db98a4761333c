"""Every layer of the fp16 UNet pass against a float64 replay of that layer on the operands the kernel itself read.

After a pass the workspace still holds every layer's fp16 output (all but the fused first layer and the last decoder
layer, which only ever exists in the fused fine head's registers); ``UNet.layer_views`` (pxt_unet_layer_views) says where,
and which tile configuration, split-K factor and pool path the pass planned for it.  A layer is replayed in float64 on the
CPU from the stored fp16 input (the previous layer, the pooled plane, or the previous decoder output and the skip) with the
weights as the library holds them (pack_unet_weights' arrays), so what is left between the replay and the stored output is
fp32 summation order and ONE fp16 rounding: the stand-alone layer test's bar, max|got - ref| < 2e-3 * max(1, max|ref|),
holds for every layer of every case - and a wrong bilinear tap, a tile seam or an uneven split-K share does not.

The cases are chosen so that together they run every kernel variant a 640x480 or 1024x576 frame runs
(test_cases_cover_every_production_plan: a condition on the plans pxt_unet_layer_views reports, not a hope).

Knobs read from the environment are not varied here, so of the coarse-head kernels only head_pair_kernel (one image) and
head_batch_kernel (a batch) are held to the head bars; head_mfma_kernel runs only with PXT_UNET_MERGE_HEADS=0, which
tests/test_variants_gpu.py proves bit-identical."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pixtrack_amd import _lib
from pixtrack_amd.unet import OUTPUT_DIMS, UNet, conv_layer_dims, make_synthetic_unet_weights, pack_unet_weights

pytestmark = pytest.mark.gpu

LAYER_BAR = 2e-3        # x max(1, max|ref|): fp32 summation order + one fp16 rounding (test_conv3x3_layer_matches_conv2d)
# Heads 1 and 2 (head_pair_kernel / head_batch_kernel, both head_mfma_body): fp32 output of a 1x1 layer on identical operands, so the
# error is fp32 accumulation over at most 512 terms plus the fp32 epilogue.  Each bar is 4 x the largest value measured
# over all the cases below (DESIGN.md "Per-layer replay of the fp16 pass" lists them): the margin for other inputs.
HEAD_FEATURE_BAR = 4 * 4.3e-7   # max|err| / max|ref| of the descriptor channels (measured: 4.292e-7, 333x421 u8, coarse head)
HEAD_CONF_BAR = 4 * 2.4e-7      # max|err| of the confidence channel (measured: 2.393e-7, 486x650 masked float, coarse head)
BLOCK_LAST = [1, 3, 6, 9, 12]   # each encoder block's last convolution: the skips, the pool sources, the coarse head's input
BLOCK_FIRST = [0, 2, 4, 7, 10]
N_VIEWS = 21


# ---- the network as the library holds it --------------------------------------------------------------------------------
_NET = {}


def _weights():
    """Synthetic weights with non-trivial BatchNorm, and pack_unet_weights' arrays parsed back out of the blob: layer 0 in
    fp32, the other 3x3 taps fp16-rounded (the decoders' BatchNorm folded in fp32 before the rounding), fp32 biases; the
    head taps rounded to fp16 as pxt_unet_create rounds them.  All as float64 tensors, made once."""
    if _NET:
        return _NET
    w = make_synthetic_unet_weights(seed=3, bn_trivial=False)
    blob = pack_unet_weights(w, "fp16")
    dims = conv_layer_dims()
    n_arrays = 2 * (17 + 3)
    table = np.frombuffer(blob, np.int64, 2 * n_arrays, 16 + 8 * 20).reshape(n_arrays, 2)

    def arr(i, dtype):
        off, n = int(table[i, 0]), int(table[i, 1])
        return np.frombuffer(blob, dtype, n // np.dtype(dtype).itemsize, off)

    conv = []
    for li, (cin, cout) in enumerate(dims):
        taps = arr(2 * li, np.float32 if li == 0 else np.float16).reshape(cout, 3, 3, cin).astype(np.float64)
        conv.append((torch.from_numpy(taps).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(arr(2 * li + 1, np.float32).astype(np.float64))))
    heads = []
    for k, (cin, dim) in enumerate(zip([32, 64, 512], OUTPUT_DIMS)):
        taps = arr(2 * (17 + k), np.float32).reshape(cin, dim + 1).astype(np.float16).astype(np.float64)  # [cin][dim + 1]
        heads.append((taps, arr(2 * (17 + k) + 1, np.float32).astype(np.float64)))
    _NET.update(w=w, conv=conv, heads=heads)
    return _NET


# ---- float64 pieces -----------------------------------------------------------------------------------------------------
def _f16(x):
    """float64 -> fp16 (one correct rounding: numpy converts double to half directly) -> float64."""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def _conv3x3_f64(x_hwc, taps, bias, relu=True, rows=96):
    """3x3 convolution, pad 1, of an [h][w][cin] float64 array -> [h][w][cout] float64, in strips of rows (the im2col
    buffer of a whole 480x640 layer would take gigabytes)."""
    x = F.pad(torch.from_numpy(np.ascontiguousarray(x_hwc)).permute(2, 0, 1), (1, 1, 1, 1))
    h = x.shape[1] - 2
    out = [F.conv2d(x[None, :, y:min(y + rows, h) + 2], taps, bias)[0] for y in range(0, h, rows)]
    y = torch.cat(out, 1)
    return (F.relu(y) if relu else y).permute(1, 2, 0).numpy()


def _upsample_as_the_kernels(prev):
    """x2 bilinear upsampling (align_corners = False) of an fp16 [hp][wp][c] map as patch_interp (pxt_conv_v2.h) and
    patch_interp_piece (pxt_conv_v3.h) form it, bit for bit: source coordinate max((g + 0.5) / 2 - 0.5, 0), taps clamped
    to the last row / column, weights (1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay, ax ay (exact in fp16), and the blend in
    packed fp16: p00 * wa, then three fused multiply-adds in the order p01, p10, p11, each rounded to fp16.  The products
    and sums are exact in float64, so rounding each step to fp16 reproduces the kernels' operand."""
    hp, wp, _ = prev.shape

    def taps(n_low):
        g = np.arange(2 * n_low)
        s = np.maximum((g + 0.5) * 0.5 - 0.5, 0.0)
        i0 = np.minimum(s.astype(np.int64), n_low - 1)
        return i0, np.minimum(i0 + 1, n_low - 1), s - i0

    y0, y1, ay = taps(hp)
    x0, x1, ax = taps(wp)
    ay, ax = ay[:, None, None], ax[None, :, None]
    r0, r1 = prev[y0], prev[y1]

    def tap(rows, cols):
        return rows[:, cols].astype(np.float64)

    v = _f16(tap(r0, x0) * ((1 - ax) * (1 - ay)))
    v = _f16(tap(r0, x1) * (ax * (1 - ay)) + v)
    v = _f16(tap(r1, x0) * ((1 - ax) * ay) + v)
    return _f16(tap(r1, x1) * (ax * ay) + v)


def _decoder_input(prev, skip):
    """cat([upsampled prev, skip cropped to it]) as the decoder kernels stage it: [2hp][2wp][cp + cs] float64."""
    up = _upsample_as_the_kernels(prev)
    return np.concatenate([up, skip[: up.shape[0], : up.shape[1]].astype(np.float64)], -1)


def _first_layer_f64(image, mask, taps, bias):
    """The first layer from the image as conv_first sees it: u8 or float, times the mask, / 255, ImageNet mean and std."""
    x = image.astype(np.float64)
    if mask is not None:
        x = x * mask.astype(np.float64)[..., None]
    x = (x / 255.0 - np.array([0.485, 0.456, 0.406])) / np.array([0.229, 0.224, 0.225])
    return _conv3x3_f64(x, taps, bias)


def _head_f64(x, taps, bias, normalize):
    """1x1 head on an [h][w][cin] map: descriptor (L2-normalised per pixel if asked) and confidence sigmoid(-x)."""
    y = x @ taps + bias
    f, u = y[..., :-1], y[..., -1]
    if normalize:
        f = f / np.maximum(np.sqrt((f * f).sum(-1, keepdims=True)), 1e-12)
    return f, 1.0 / (1.0 + np.exp(u))


# ---- cases --------------------------------------------------------------------------------------------------------------
def _smooth_image(H, W, seed, u8):
    rng = np.random.default_rng(seed)
    img = rng.uniform(0, 255, size=(H, W, 3)).astype(np.float32)
    img = (img + np.roll(img, 1, 0) + np.roll(img, 1, 1) + np.roll(img, 2, 0)) / 4  # an image rather than white noise
    return np.floor(img).astype(np.uint8) if u8 else img


def _blob_mask(H, W):
    """A dilated-silhouette mask: 1 inside an ellipse, 0 over most of the frame (turns constant-tile skipping on)."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return ((((yy - 0.52 * H) / (0.3 * H)) ** 2 + ((xx - 0.47 * W) / (0.33 * W)) ** 2) < 1.0).astype(np.uint8)


def _render_like(H, W, seed):
    """A tracker-like reference render: uint8, exactly 0 outside the object."""
    return _smooth_image(H, W, seed, True) * _blob_mask(H, W)[..., None]


def _item(H, W, seed, kind, normalize):
    if kind == "float":
        return (_smooth_image(H, W, seed, False), None, normalize)
    if kind == "u8":
        return (_smooth_image(H, W, seed, True), None, normalize)
    if kind == "masked":
        return (_smooth_image(H, W, seed, False), _blob_mask(H, W), normalize)
    assert kind == "render"
    return (_render_like(H, W, seed), None, normalize)


# name -> (items of (H, W, kind, normalize), peers)
CASES = {
    "16x16 float": ([(16, 16, "float", False)], 1),           # 1x1 bottleneck: every bilinear tap clamps, every tile partial
    "17x31 float": ([(17, 31, "float", True)], 1),
    "75x100 float": ([(75, 100, "float", True)], 1),          # odd at every level, split-K everywhere, cropped skips
    "batch of 3 at 75x100": ([(75, 100, "u8", False), (75, 100, "masked", True), (75, 100, "float", True)], 1),
    "333x421 u8": ([(333, 421, "u8", False)], 1),
    "486x650 masked float": ([(486, 650, "masked", True)], 1),
    "pair 486x650 render, 333x421 masked": ([(486, 650, "render", False), (333, 421, "masked", True)], 2),
}
PRODUCTION = [(480, 640), (576, 1024)]


def _plan_key(views, li):
    """What distinguishes the kernel a 3x3 layer runs: configuration, split-K class (1, odd, even), who pools, decoder
    variant, deep tap ring, fused first layer, fused fine head."""
    v = views[li]
    split_class = "1" if v["splits"] == 1 else ("odd" if v["splits"] % 2 else "even")
    return (v["cfg"], split_class, bool(v["pool_fused"]), bool(v["decoder"]), bool(v["deep_ring"]),
            li == 1 and not views[0]["in_memory"], li == 16 and not views[16]["in_memory"])


def _pool_key(views, b):
    return ("pool", bool(views[17 + b - 1]["pool_fused"]))


def _keys(views):
    return {_plan_key(views, li) for li in range(1, 17)} | {_pool_key(views, b) for b in range(1, 5)}


def _case_views(net, case):
    items, peers = CASES[case]
    if peers == 2:
        return [net.layer_views(1, H, W, 2) for H, W, _k, _n in items]
    return [net.layer_views(len(items), items[0][0], items[0][1], 1)]


@pytest.fixture(scope="module")
def net(device):
    return UNet(_weights()["w"], device)


def test_layer_views_describe_the_pass(net):
    """Shapes, the two layers that are never written, the decoder flags and the argument checks of pxt_unet_layer_views."""
    views = net.layer_views(1, 75, 100)
    assert len(views) == N_VIEWS
    assert [(v["h"], v["w"]) for v in views[:13:3]] == [(75, 100), (37, 50), (18, 25), (9, 12), (4, 6)]
    assert [(v["h"], v["w"], v["c"]) for v in views[13:17]] == [(8, 12, 64), (16, 24, 64), (32, 48, 64), (64, 96, 32)]
    assert [(v["h"], v["w"], v["c"]) for v in views[17:]] == [(37, 50, 64), (18, 25, 128), (9, 12, 256), (4, 6, 512)]
    assert [v["c"] for v in views[:17]] == [c for _cin, c in conv_layer_dims()]
    assert [li for li, v in enumerate(views) if not v["in_memory"]] == [0, 16]  # as UNet.activation_stats reports them
    assert [bool(v["decoder"]) for v in views[:17]] == [False] * 13 + [True] * 4
    assert all(v["cfg"] > 0 and v["splits"] >= 1 for v in views[1:17]) and views[0]["cfg"] == 0
    assert all(v["offset"] % 256 == 0 for v in views)
    spans = sorted((v["offset"], v["offset"] + 2 * v["h"] * v["w"] * v["c"]) for li, v in enumerate(views) if li not in (0, 16))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "two layers of one pass share workspace bytes"
    L = _lib.lib()
    out = (_lib.UnetLayerView * N_VIEWS)()
    assert L.pxt_unet_layer_views(None, 1, 64, 64, 1, out) == -1
    assert L.pxt_unet_layer_views(net._ctx, 1, 64, 64, 1, None) == -1
    assert L.pxt_unet_layer_views(net._ctx, 1, 15, 64, 1, out) == -1      # no 1/16 level
    assert L.pxt_unet_layer_views(net._ctx, 2, 64, 64, 2, out) == -1      # a peer is ONE image of a pair
    assert L.pxt_unet_layer_views(net._ctx, 1, 64, 64, 3, out) == -1
    net32 = UNet(_weights()["w"], net.device, precision="fp32")
    assert L.pxt_unet_layer_views(net32._ctx, 1, 64, 64, 1, out) == -1    # the fp32 pass has its own layout


def test_cases_cover_every_production_plan(net):
    """Every kernel variant a 640x480 or 1024x576 frame runs - lone pass or one half of the pair pass - is run, and held
    to the layer bar, by one of the replay cases.  A change to plan_conv that moves production onto a variant no case
    reaches fails here."""
    covered = set()
    for case in CASES:
        for views in _case_views(net, case):
            covered |= _keys(views)
    for H, W in PRODUCTION:
        for peers in (1, 2):
            views = net.layer_views(1, H, W, peers)
            missing = _keys(views) - covered
            print(f"{W}x{H} peers {peers}: " + " ".join(
                f"{li}:{v['cfg']}" + (f"/{v['splits']}" if v["splits"] > 1 else "") + ("+pool" if v["pool_fused"] else "") +
                ("+deep" if v["deep_ring"] else "") for li, v in enumerate(views[:17]) if li))
            assert not missing, (H, W, peers, sorted(missing, key=str))


def _replay(net, case):
    """One pass, one copy of the workspace, every stored layer against its float64 replay.  Returns the per-layer figures
    and the two coarse heads' errors."""
    net_w = _weights()
    conv, heads = net_w["conv"], net_w["heads"]
    items, peers = CASES[case]
    device = net.device
    host = [_item(H, W, 11 + 7 * i, kind, normalize) for i, (H, W, kind, normalize) in enumerate(items)]
    dev = [(torch.from_numpy(im).to(device), None if m is None else torch.from_numpy(m).to(device), nz) for im, m, nz in host]
    # the workspace is the module's UNet's, reused from case to case: every byte is set to 0xFF (fp16 NaN) before the pass,
    # so that a layer the pass failed to write fails the finite check instead of being compared with an earlier case's bytes
    L = _lib.lib()
    if peers == 2:
        need = int(L.pxt_unet_workspace_bytes_pair(net._ctx, (C.c_int32 * 2)(items[0][0], items[1][0]),
                                                   (C.c_int32 * 2)(items[0][1], items[1][1])))
    else:
        need = int(L.pxt_unet_workspace_bytes_batch(net._ctx, len(items), items[0][0], items[0][1]))
    assert need > 0
    if net._ws is None or net._ws.numel() < need:
        net._ws = torch.empty(need, dtype=torch.uint8, device=device)
    net._ws.fill_(0xFF)
    held = net._ws.data_ptr()
    outs = net.forward_packed_batch(dev)
    torch.cuda.synchronize()
    assert net._ws.data_ptr() == held, "the pass ran in another workspace than the one that was filled"
    ws = net._ws.cpu().numpy()
    outs = [[o.cpu().numpy() for o in per] for per in outs]
    if peers == 2:  # two single-image passes in the two halves of the workspace
        passes = [(net.layer_views(1, H, W, 2), base, 1, [i]) for i, ((H, W, _k, _n), base) in enumerate(
            zip(items, (0, int(L.pxt_unet_workspace_bytes(net._ctx, items[0][0], items[0][1])))))]
    else:
        passes = [(net.layer_views(len(items), items[0][0], items[0][1], 1), 0, len(items), list(range(len(items))))]
    figures, head_feat, head_conf = [], 0.0, 0.0
    for views, base, n, members in passes:
        def stored(vi, im):
            v = views[vi]
            assert v["in_memory"]
            a = np.frombuffer(ws, np.float16, n * v["h"] * v["w"] * v["c"], base + v["offset"])
            return a.reshape(n, v["h"], v["w"], v["c"])[im]

        for im, item in enumerate(members):
            image, mask, normalize = host[item]
            tag = f"{case} image {item}"

            def check(li, ref, got, what=""):
                assert np.isfinite(got).all(), (tag, li, what)
                scale = max(1.0, float(np.abs(ref).max()))
                err = float(np.abs(got.astype(np.float64) - ref).max()) / scale
                v = views[li]
                figures.append((tag, li, v["cfg"], v["splits"], err))
                print(f"{tag}: layer {li:2d}{what} {v['w']}x{v['h']} cfg {v['cfg']:2d} splits {v['splits']} "
                      f"{'pool ' if v['pool_fused'] else ''}max|err|/max(1,max|ref|) = {err:.3e}")
                assert err < LAYER_BAR, (tag, li, what, err)

            # layer 0: in memory only with PXT_UNET_FUSE_FIRST=0.  Fused, it is replayed in float64 and rounded to fp16
            # for layer 1; the kernel forms it in fp32 (hi / lo split MFMAs), so a few of layer 1's operands may sit one
            # fp16 ulp from the replay's - a relative 5e-4 on a few of 576 terms, far inside the layer bar.
            x0 = _first_layer_f64(image, mask, *conv[0])
            if views[0]["in_memory"]:
                check(0, x0, stored(0, im))
                x0 = stored(0, im).astype(np.float64)
            else:
                x0 = _f16(x0)
            for li in range(1, 13):
                b = max(k for k in range(5) if BLOCK_FIRST[k] <= li)
                if li == 1:
                    x = x0
                elif li == BLOCK_FIRST[b]:
                    x = stored(17 + b - 1, im).astype(np.float64)  # the pooled plane the kernel read
                else:
                    x = stored(li - 1, im).astype(np.float64)
                check(li, _conv3x3_f64(x, *conv[li]), stored(li, im))
            # pools: bit for bit the 2x2 max of the stored fp16 layer (floor: an odd last row / column is dropped), whether
            # the layer's epilogue or maxpool2_kernel wrote them
            for b in range(1, 5):
                src, got = stored(BLOCK_LAST[b - 1], im), stored(17 + b - 1, im)
                h2, w2 = got.shape[:2]
                want = src[: 2 * h2, : 2 * w2].reshape(h2, 2, w2, 2, -1).max((1, 3))
                assert np.array_equal(got, want), (tag, "pool", b, bool(views[17 + b - 1]["pool_fused"]))
            # decoder
            for d in range(4):
                li = 13 + d
                x = _decoder_input(stored(li - 1, im), stored(BLOCK_LAST[3 - d], im))
                ref = _conv3x3_f64(x, *conv[li])
                if views[li]["in_memory"]:
                    check(li, ref, stored(li, im))
                else:
                    # the fused fine head (FusedHead, pxt_conv_v2.h / pxt_conv_v3.h epilogue): bias + ReLU, ONE rounding to
                    # fp16 - the B operand of the head's MFMA - then the 1x1 head with fp16-rounded taps
                    f, c = _head_f64(_f16(ref), *heads[0], normalize)
                    o = outs[item][0]
                    check(16, f, o[..., :32], " + fine head, features")
                    check(16, c[..., None], o[..., 32:33], " + fine head, confidence")
                    assert (o[..., 33:] == 0).all()
            # the coarse heads on the stored fp16 layers they read
            for k, src in ((1, 14), (2, 12)):
                f, c = _head_f64(stored(src, im).astype(np.float64), *heads[k], normalize)
                o, dim = outs[item][k], OUTPUT_DIMS[k]
                assert np.isfinite(o).all() and (o[..., dim + 1:] == 0).all()
                ef = float(np.abs(o[..., :dim] - f).max() / np.abs(f).max())
                ec = float(np.abs(o[..., dim] - c).max())
                print(f"{tag}: head {k} features max|err|/max|ref| = {ef:.3e}  confidence max|err| = {ec:.3e}")
                head_feat, head_conf = max(head_feat, ef), max(head_conf, ec)
                assert ef < HEAD_FEATURE_BAR and ec < HEAD_CONF_BAR, (tag, k, ef, ec)
    return figures, head_feat, head_conf


@pytest.mark.parametrize("case", list(CASES))
def test_every_layer_matches_its_float64_replay(net, case):
    figures, head_feat, head_conf = _replay(net, case)
    worst = max(figures, key=lambda f: f[4])
    print(f"{case}: worst layer {worst[1]} (cfg {worst[2]}, splits {worst[3]}) {worst[4]:.3e}; coarse heads: features "
          f"{head_feat:.3e}, confidence {head_conf:.3e}")


# ---- stand-alone decoder layers -----------------------------------------------------------------------------------------
def _upcat_conv(device, prev, skip, w, b, cfg, splits):
    """prev [hp][wp][cp], skip [hs][ws][cs] fp16 numpy, w [cout][cp + cs][3][3] fp16 -> out [2hp][2wp][cout] fp16 numpy
    through pxt_conv3x3_pack_weights + pxt_conv3x3_upcat_packed."""
    L = _lib.lib()
    (hp, wp, cp), (hs, ws_, cs) = prev.shape, skip.shape
    cout = w.shape[0]
    pd, sd = torch.from_numpy(prev).to(device), torch.from_numpy(skip).to(device)
    wd = w.permute(0, 2, 3, 1).contiguous().to(device)
    bd = b.to(device)
    packed = torch.empty(int(L.pxt_conv3x3_packed_bytes(cp + cs, cout)), dtype=torch.uint8, device=device)
    _lib.check(L.pxt_conv3x3_pack_weights(wd.data_ptr(), cp + cs, cout, packed.data_ptr(), _lib.stream_ptr(device)), "pack")
    out = torch.full((2 * hp, 2 * wp, cout), float("nan"), dtype=torch.float16, device=device)
    part = torch.empty(splits * 4 * hp * wp * cout * 4, dtype=torch.uint8, device=device) if splits > 1 else None
    _lib.check(L.pxt_conv3x3_upcat_packed(pd.data_ptr(), hp, wp, cp, sd.data_ptr(), hs, ws_, cs, packed.data_ptr(), bd.data_ptr(),
                                          cout, 1, out.data_ptr(), cfg, splits, _lib.dptr(part),
                                          part.numel() if part is not None else 0, _lib.stream_ptr(device)), "upcat conv")
    torch.cuda.synchronize()
    return out.cpu().numpy()


# (prev h, w) -> (skip h, w): a 1x1 map under a 3x3 skip (every tap clamps); 5x9 -> 10x18 under 11x19; 19x13 -> 38x26 under
# 38x27: partial tiles both ways, more than one tile row for the 24- and 32-row tiles
UPCAT_SHAPES = [((1, 1), (3, 3)), ((5, 9), (11, 19)), ((19, 13), (38, 27))]
# (cp, cs, split-K factors): the uneven factors leave no split empty (ceil(chunks / splits) chunks each, the last the rest:
# 3 chunks -> 1 + 1 + 1, 32 -> 6 x 5 + 2, 10 -> 4 + 4 + 2)
UPCAT_CHANNELS = [(64, 32, (1, 2, 3)), (512, 512, (1, 2, 7)), (64, 256, (1, 2, 3))]
_UPCAT_REFS = {}


def _upcat_reference(shape, channels, cout):
    """Operands and the float64 reference of one stand-alone decoder layer, made once per (shape, channels, cout)."""
    key = (shape, channels[:2], cout)
    if key not in _UPCAT_REFS:
        (hp, wp), (hs, ws_) = shape
        cp, cs = channels[:2]
        g = torch.Generator().manual_seed(hp * 1000 + wp * 10 + cp + cout)
        prev = torch.randn(hp, wp, cp, generator=g).half().numpy()
        skip = torch.randn(hs, ws_, cs, generator=g).half().numpy()
        w = (torch.randn(cout, cp + cs, 3, 3, generator=g) * (2.0 / (9 * (cp + cs))) ** 0.5).half()
        b = torch.randn(cout, generator=g)
        ref = _conv3x3_f64(_decoder_input(prev, skip), w.double(), b.double())
        _UPCAT_REFS[key] = (prev, skip, w, b, ref)
    return _UPCAT_REFS[key]


@pytest.mark.parametrize("cfg,cout", [(2, 64), (6, 32), (16, 32), (17, 64), (20, 32), (21, 64)])
@pytest.mark.parametrize("channels", UPCAT_CHANNELS, ids=lambda c: f"{c[0]}+{c[1]}")
@pytest.mark.parametrize("shape", UPCAT_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}")
def test_decoder_layer_every_configuration(device, cfg, cout, channels, shape):
    """Every tile configuration that has a decoder (upsample + concat) variant, through pxt_conv3x3_upcat_packed, against
    the float64 layer on the emulated blend: clamped taps, cropped skips, partial tiles, the upsampled / skip boundary
    inside the K walk, split-K with even and uneven shares.  (The pyramid picks 2, 20 and 21; the others are reachable
    through PXT_CONV_PLAN.)"""
    prev, skip, w, b, ref = _upcat_reference(shape, channels, cout)
    tol = LAYER_BAR * max(1.0, float(np.abs(ref).max()))
    for splits in channels[2]:
        got = _upcat_conv(device, prev, skip, w, b, cfg, splits)
        assert np.isfinite(got).all(), splits
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print(f"cfg {cfg} splits {splits}: max|err| = {err:.3e} (bar {tol:.3e})")
        assert err < tol, (cfg, splits, err)


def test_decoder_layer_entry_checks_its_arguments(device):
    """pxt_conv3x3_upcat_packed under launch_conv's checks: channel multiples, a skip smaller than the output, a
    configuration without a decoder variant for this Cout, a split-K region that is too small."""
    L = _lib.lib()
    t = torch.zeros(1 << 18, dtype=torch.float16, device=device)  # (larger than any operand of the calls that launch)
    o = torch.zeros(4 * 4 * 64, dtype=torch.float16, device=device)
    p, s = t.data_ptr(), _lib.stream_ptr(device)

    def call(hp=2, wp=2, cp=32, hs=4, ws_=4, cs=32, cout=32, cfg=0, splits=1, part=None, part_bytes=0):
        return L.pxt_conv3x3_upcat_packed(p, hp, wp, cp, p, hs, ws_, cs, p, p, cout, 1, o.data_ptr(), cfg, splits, part,
                                          part_bytes, s)

    assert call(cp=16) == -1 and call(cs=48) == -1 and call(cout=48) == -1
    assert call(hs=3) == -1 and call(ws_=3) == -1
    assert call(cfg=1) == -1 and call(cfg=15) == -1           # no decoder variant
    assert call(cfg=2) == -1 and call(cfg=20, cout=64) == -1  # the variant serves the other channel count
    assert call(splits=2) == -1 and call(splits=2, part=p, part_bytes=2 * 16 * 32 * 4 - 1) == -1
    assert L.pxt_conv3x3_upcat_packed(None, 2, 2, 32, p, 4, 4, 32, p, p, 32, 1, o.data_ptr(), 0, 1, None, 0, s) == -1
    assert call(cfg=20) == 0 and call(cfg=2, cout=64) == 0
    torch.cuda.synchronize()
