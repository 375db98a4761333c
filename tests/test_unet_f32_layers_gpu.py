"""Every layer of the fp32 UNet pass (pxt_unet_f32.hip) against a float64 replay of that layer on the operands the kernel
itself read, and every conv3x3_f32_kernel configuration against every other, bit for bit.

The fp32 pass keeps every buffer in its workspace: ``UNet.layer_views_f32`` (pxt_unet_layer_views_f32) says where, from the
pass's own make_plan, and which of the five tile configurations launch_conv takes for each 3x3 layer, from the one
function launch_conv asks (pxt_conv3x3_f32_cfg).  A layer is replayed in float64 on the CPU from the stored fp32 input with
the taps as the library holds them (pack_unet_weights' fp32 arrays), so what is left between replay and stored output is
fp32 accumulation: the stand-alone layer test's bar, max|got - ref| < 1e-5 * max(1, max|ref|), holds for every layer -
two orders of magnitude under the end-to-end bar of tests/test_unet_f32_gpu.py.

The two large-map configurations (1 = <2,2,2,2>, 3 = <2,2,1,4>) are the ones 640x480 and 1024x576 frames run on their most
expensive layers; no pass small enough for a test reaches their thresholds, so they are forced on small maps
(pxt_conv3x3_nhwc_f32_cfg) and planned once each at the smallest shape that crosses the threshold.  The file's header
promises that which workgroup or wave computes a value changes nothing: all configurations must give the same bits.
test_production_plans_run_only_tested_configurations makes the coverage a condition on the lists below."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pixtrack_amd import _lib
from pixtrack_amd.unet import HEAD_INPUTS, OUTPUT_DIMS, UNet, conv_layer_dims, make_synthetic_unet_weights, pack_unet_weights
from test_unet_layers_gpu import BLOCK_FIRST, BLOCK_LAST, _conv3x3_f64, _first_layer_f64, _head_f64, _item

pytestmark = pytest.mark.gpu

LAYER_BAR = 1e-5   # x max(1, max|ref|): fp32 accumulation alone (test_conv3x3_f32_layer_matches_conv2d's bar)
# upcat_f32_kernel against the float64 bilinear: the lambdas (0, 0.25, 0.75, 1) and 1 - lambda are exact in fp32, and every
# intermediate of ly0 (lx0 a + lx1 b) + ly1 (lx0 d + lx1 e) is a weighted mean of taps, no larger than max|prev|.  Of
# the six products at most three round (in each pair lambda, 1 - lambda only a 0.75 does: 0, 0.25 and 1 multiply exactly),
# the three sums round, a fused multiply-add saves one: at most seven roundings counted generously, each within half an
# ulp = 2^-24 of its magnitude: 7 * 2^-24, taken as 8
UPSAMPLE_BAR = 8 * 2.0 ** -24   # x max|prev|
# The 1x1 heads (head_f32_kernel) on identical fp32 operands against the float64 head: fp32 accumulation over at most 512
# terms plus the fp32 epilogue.  Each bar is 4 x the largest value measured on the MI355X over all the cases below
# (DESIGN.md "Per-layer replay of the fp32 pass" lists them), the margin the fp16 replay uses for its heads.
HEAD_FEATURE_BAR = 4 * 5.9e-7   # max|err| / max|ref| of the descriptor channels (measured: 5.881e-7, batch of 3, image 2, stride 16)
HEAD_CONF_BAR = 4 * 3.1e-7      # max|err| of the confidence channel (measured: 3.059e-7, batch of 3, image 1, stride 16)
N_VIEWS = 22
GUARD = 4096
HEAD_SOURCE = [16, 14, 12]      # the layers the heads at strides 1, 4, 16 read

# conv3x3_f32_kernel<CB, PB, WC, WP> as pxt_conv3x3_f32_cfg numbers them, and the output channels a workgroup spans
CFG_SPAN = {1: 128, 2: 128, 3: 64, 4: 64, 5: 32}


def _admitted(cout):
    return [cfg for cfg, span in CFG_SPAN.items() if cout % span == 0]


# ---- every configuration, same bits -------------------------------------------------------------------------------------
# one pixel; one partial tile; partial tiles both ways with two tile rows of the 16-row tiles; 3 x 4 tiles of 16 x 16
FORCED_SHAPES = [(1, 1), (7, 5), (17, 31), (37, 50)]
# (Cin, Cout): one chunk; an odd number of chunks (the double buffer ends on the other half); more than one channel group
# per grid row for every configuration
FORCED_CHANNELS = [(16, 128), (48, 128), (64, 256)]
FORCED_CFGS = sorted({cfg for _cin, cout in FORCED_CHANNELS for cfg in _admitted(cout)})
_OPERANDS = {}


def _operands(H, W, Cin, Cout):
    """Random asymmetric operands (as test_conv3x3_f32_layer_matches_conv2d draws them) and the float64 convolution before
    the ReLU, [Cout][H][W]; made once per shape."""
    key = (H, W, Cin, Cout)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(H * 1000 + W + Cin)
        x = torch.randn(Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
        b = torch.randn(Cout, generator=g)
        _OPERANDS[key] = (x, w, b, F.conv2d(x.double()[None], w.double(), b.double(), padding=1)[0])
    return _OPERANDS[key]


def _to_device(device, x, w, b):
    return x.permute(1, 2, 0).contiguous().to(device), w.permute(0, 2, 3, 1).contiguous().to(device), b.to(device)


def _conv(device, xd, wd, bd, relu, cfg):
    """One stand-alone layer in configuration cfg (0: the pass's choice) into a NaN-filled output, [H][W][Cout] on the
    device; the caller synchronises."""
    (H, W, Cin), Cout = xd.shape, wd.shape[0]
    out = torch.full((H, W, Cout), float("nan"), dtype=torch.float32, device=device)
    _lib.check(_lib.lib().pxt_conv3x3_nhwc_f32_cfg(xd.data_ptr(), H, W, Cin, wd.data_ptr(), bd.data_ptr(), Cout, relu,
                                                   out.data_ptr(), cfg, _lib.stream_ptr(device)), f"cfg {cfg}")
    return out


def _within_the_bar(out, ref, what):
    got = out.double().cpu().permute(2, 0, 1)
    assert torch.isfinite(got).all(), what
    err, scale = (got - ref).abs().max().item(), max(1.0, ref.abs().max().item())
    print(f"{what}: max|err| / max(1, max|ref|) = {err / scale:.3e}")
    assert err < LAYER_BAR * scale, (what, err)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("Cin,Cout", FORCED_CHANNELS)
@pytest.mark.parametrize("H,W", FORCED_SHAPES)
def test_every_configuration_gives_the_same_bits(device, H, W, Cin, Cout, relu):
    """All five instantiations on the same operands: each within the float64 bar, and all the same bits - one K-ordered
    chain per value, whichever workgroup or wave forms it."""
    x, w, b, ref = _operands(H, W, Cin, Cout)
    ref = F.relu(ref) if relu else ref
    xd, wd, bd = _to_device(device, x, w, b)
    cfgs = _admitted(Cout)
    assert cfgs == [1, 2, 3, 4, 5]
    outs = [_conv(device, xd, wd, bd, relu, cfg) for cfg in cfgs]
    torch.cuda.synchronize()
    for cfg, out in zip(cfgs, outs):
        _within_the_bar(out, ref, f"{H}x{W} {Cin}->{Cout} relu {relu} cfg {cfg}")
    for cfg, out in zip(cfgs[1:], outs[1:]):
        differ = int((out != outs[0]).sum())
        assert torch.equal(out, outs[0]), f"cfg {cfg} and cfg {cfgs[0]} differ in {differ} of {out.numel()} values"


# ---- the planned path at the thresholds ---------------------------------------------------------------------------------
# (H, W, Cin, Cout, the configuration pxt_conv3x3_f32_cfg must name): the smallest shapes that cross each threshold with
# partial tiles on both sides - 18 x 19 = 342 tiles x 3 channel groups >= 1024; 8 x 16 = 128 tiles x 2 x 4 >= 1024 - and
# one tile column under the second
THRESHOLDS = [(273, 290, 48, 192, 3), (125, 250, 48, 512, 1), (125, 240, 48, 512, 2)]


@pytest.mark.parametrize("H,W,Cin,Cout,want", THRESHOLDS)
def test_planned_configuration_at_the_thresholds(device, H, W, Cin, Cout, want):
    """cfg = 0 where launch_conv's own choice is a large-map configuration (and one tile under): the float64 bar, the same
    bits as the forced call and as the narrowest configuration."""
    assert _lib.lib().pxt_conv3x3_f32_cfg(H, W, Cout) == want
    x, w, b, ref = _operands(H, W, Cin, Cout)
    ref = F.relu(ref)
    xd, wd, bd = _to_device(device, x, w, b)
    planned, forced, narrow = (_conv(device, xd, wd, bd, 1, cfg) for cfg in (0, want, 5))
    torch.cuda.synchronize()
    _within_the_bar(planned, ref, f"{H}x{W} {Cin}->{Cout} planned (cfg {want})")
    assert torch.equal(planned, forced), int((planned != forced).sum())
    assert torch.equal(planned, narrow), int((planned != narrow).sum())


# ---- a NaN stays where it is --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y,x", [(0, 0), (15, 16), (36, 49)], ids=["corner", "tile seam", "last pixel"])
@pytest.mark.parametrize("cfg", [1, 5])
def test_a_nan_reaches_its_neighbourhood_and_nothing_else(device, cfg, y, x):
    """relu_nan: "NaN passes, like torch.relu".  One NaN input element: exactly the 3x3 neighbourhood of its pixel, clipped
    to the image, is NaN in every output channel (every tap is non-zero; NaN x 0 would be NaN anyway), and the rest is
    the clean run's bits - no other pixel's chain reads it, no staging slot is shared."""
    H, W, Cin, Cout = 37, 50, 48, 128
    xs, w, b, _ref = _operands(H, W, Cin, Cout)
    assert (w != 0).all()
    xd, wd, bd = _to_device(device, xs, w, b)
    bad = xd.clone()
    bad[y, x, 21] = float("nan")
    clean, got = _conv(device, xd, wd, bd, 1, cfg), _conv(device, bad, wd, bd, 1, cfg)
    torch.cuda.synchronize()
    clean, got = clean.cpu(), got.cpu()
    assert torch.isfinite(clean).all()
    want = torch.zeros(H, W, dtype=torch.bool)
    want[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    assert torch.equal(torch.isnan(got), want[..., None].expand(H, W, Cout))
    assert torch.equal(got[~want], clean[~want])


# ---- the per-layer replay of the pass -----------------------------------------------------------------------------------
_NET = {}


def _weights():
    """Synthetic weights with non-trivial BatchNorm, and pack_unet_weights' fp32 arrays parsed back out of the blob (the
    decoders' BatchNorm folded as the library folds it), as float64 tensors; made once."""
    if _NET:
        return _NET
    w = make_synthetic_unet_weights(seed=3, bn_trivial=False)
    blob = pack_unet_weights(w, "fp32")
    dims = conv_layer_dims()
    n_arrays = 2 * (17 + 3)
    table = np.frombuffer(blob, np.int64, 2 * n_arrays, 16 + 8 * 20).reshape(n_arrays, 2)

    def arr(i):
        off, n = int(table[i, 0]), int(table[i, 1])
        return np.frombuffer(blob, np.float32, n // 4, off).astype(np.float64)

    conv = [(torch.from_numpy(arr(2 * li).reshape(cout, 3, 3, cin)).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(arr(2 * li + 1)))
            for li, (cin, cout) in enumerate(dims)]
    heads = [(arr(2 * (17 + k)).reshape(cin, dim + 1), arr(2 * (17 + k) + 1)) for k, (cin, dim) in enumerate(zip(HEAD_INPUTS, OUTPUT_DIMS))]
    _NET.update(w=w, conv=conv, heads=heads)
    return _NET


def _bilinear_x2_f64(prev):
    """torch's x2 bilinear upsampling (align_corners = False) of an [h][w][c] float64 array, in float64."""
    t = torch.from_numpy(np.ascontiguousarray(prev)).permute(2, 0, 1)[None]
    up = F.interpolate(t, size=(2 * prev.shape[0], 2 * prev.shape[1]), mode="bilinear", align_corners=False)
    return up[0].permute(1, 2, 0).numpy()


# name -> (items of (H, W, kind, normalize), pair pass)
CASES = {
    "16x16 float": ([(16, 16, "float", False)], False),          # 1x1 bottleneck: every bilinear tap clamps
    "17x31 u8, normalize": ([(17, 31, "u8", True)], False),      # odd rows and columns dropped by the first pool
    "75x100 masked float, normalize": ([(75, 100, "masked", True)], False),  # odd at every level, cropped skips
    "batch of 3 at 75x100": ([(75, 100, "u8", False), (75, 100, "masked", True), (75, 100, "float", True)], False),
    "pair 75x100 u8, 37x50 masked": ([(75, 100, "u8", False), (37, 50, "masked", True)], True),
}
PRODUCTION = [(480, 640), (576, 1024)]


@pytest.fixture(scope="module")
def net(device):
    return UNet(_weights()["w"], device, precision="fp32")


def test_layer_views_f32_describe_the_pass(net):
    """Shapes, flags, the configurations (the shared choice function's) and the argument checks of pxt_unet_layer_views_f32."""
    L = _lib.lib()
    views = net.layer_views_f32(2, 75, 100)
    dims = conv_layer_dims()
    assert len(views) == N_VIEWS
    assert [(v["h"], v["w"]) for v in views[:13:3]] == [(75, 100), (37, 50), (18, 25), (9, 12), (4, 6)]
    assert [(v["h"], v["w"], v["c"]) for v in views[13:17]] == [(8, 12, 64), (16, 24, 64), (32, 48, 64), (64, 96, 32)]
    assert [(v["h"], v["w"], v["c"]) for v in views[17:21]] == [(37, 50, 64), (18, 25, 128), (9, 12, 256), (4, 6, 512)]
    assert (views[21]["h"], views[21]["w"], views[21]["c"]) == (64, 96, dims[16][0])
    assert [v["c"] for v in views[:17]] == [cout for _cin, cout in dims]
    assert all(v["in_memory"] == 1 and v["splits"] == 1 and v["pool_fused"] == 0 and v["deep_ring"] == 0 and v["reserved"] == 0
               for v in views)
    assert [v["decoder"] for v in views] == [0] * 13 + [1] * 4 + [0] * 5
    assert views[0]["cfg"] == 0 and all(v["cfg"] == 0 for v in views[17:])
    assert [v["cfg"] for v in views[1:17]] == [L.pxt_conv3x3_f32_cfg(v["h"], v["w"], v["c"]) for v in views[1:17]]
    assert all(v["offset"] % 256 == 0 for v in views)
    # the layout does not depend on the configuration and scales with the batch: the same shapes for one image
    assert [(v["h"], v["w"], v["c"], v["cfg"]) for v in net.layer_views_f32(1, 75, 100)] == [(v["h"], v["w"], v["c"], v["cfg"]) for v in views]
    out = (_lib.UnetLayerView * N_VIEWS)()
    assert L.pxt_unet_layer_views_f32(None, 1, 64, 64, out) == -1
    assert L.pxt_unet_layer_views_f32(net._ctx, 1, 64, 64, None) == -1
    assert L.pxt_unet_layer_views_f32(net._ctx, 1, 15, 64, out) == -1     # no 1/16 level
    assert L.pxt_unet_layer_views_f32(net._ctx, 0, 64, 64, out) == -1
    assert L.pxt_unet_layer_views_f32(net._ctx, _lib.PXT_UNET_MAX_BATCH + 1, 64, 64, out) == -1
    assert L.pxt_unet_layer_views_f32(net._ctx, 1, 64, 64, out) == 0
    net16 = UNet(_weights()["w"], net.device)
    assert L.pxt_unet_layer_views_f32(net16._ctx, 1, 64, 64, out) == -1   # the fp16 pass has pxt_unet_layer_views


def test_production_plans_run_only_tested_configurations(net):
    """Every configuration a 640x480 or a 1024x576 fp32 frame runs is one test_every_configuration_gives_the_same_bits
    forces, and the large-map ones are planned by test_planned_configuration_at_the_thresholds.  A sixth configuration or a
    moved threshold that puts production on an untested kernel fails here."""
    planned = {want for *_shape, want in THRESHOLDS}
    for H, W in PRODUCTION:
        views = net.layer_views_f32(1, H, W)
        print(f"{W}x{H}: " + " ".join(f"{li}:{v['cfg']}" for li, v in enumerate(views[:17]) if li))
        cfgs = {v["cfg"] for v in views[1:17]}
        assert cfgs <= set(FORCED_CFGS), (H, W, sorted(cfgs - set(FORCED_CFGS)))
        assert cfgs & {1, 3} <= planned, (H, W, cfgs)
    assert views[3]["cfg"] == 1 and views[1]["cfg"] == 3  # 1024x576 does run both large-map configurations


def _replay(net, case):
    """One pass into a 0xFF-filled workspace with a guard behind it, one copy of the workspace, every buffer against its
    float64 replay.  Returns the per-layer figures and the heads' errors."""
    net_w = _weights()
    conv, heads, dims = net_w["conv"], net_w["heads"], conv_layer_dims()
    items, pair = CASES[case]
    device = net.device
    host = [_item(H, W, 11 + 7 * i, kind, normalize) for i, (H, W, kind, normalize) in enumerate(items)]
    dev = [(torch.from_numpy(im).to(device), None if m is None else torch.from_numpy(m).to(device), nz) for im, m, nz in host]
    L = _lib.lib()
    if pair:
        need = int(L.pxt_unet_workspace_bytes_pair(net._ctx, (C.c_int32 * 2)(items[0][0], items[1][0]),
                                                   (C.c_int32 * 2)(items[0][1], items[1][1])))
    else:
        need = int(L.pxt_unet_workspace_bytes_batch(net._ctx, len(items), items[0][0], items[0][1]))
    assert need > 0
    # every byte 0xFF (fp32 NaN): a value the pass failed to write fails the finite check, and a write past the workspace
    # shows in the guard
    held = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=device)
    net._ws = held
    outs = net.forward_packed_batch(dev)
    torch.cuda.synchronize()
    assert net._ws is held, "the pass ran in another workspace than the one that was filled"
    ws = held.cpu().numpy()
    assert (ws[need:] == 0xFF).all(), "the pass wrote behind its workspace"
    outs = [[o.cpu().numpy() for o in per] for per in outs]
    if pair:  # two single-image passes, the second one's workspace behind the first one's
        bases = (0, int(L.pxt_unet_workspace_bytes(net._ctx, items[0][0], items[0][1])))
        passes = [(net.layer_views_f32(1, H, W), base, 1, [i], int(L.pxt_unet_workspace_bytes(net._ctx, H, W)))
                  for i, ((H, W, _k, _n), base) in enumerate(zip(items, bases))]
    else:
        passes = [(net.layer_views_f32(len(items), items[0][0], items[0][1]), 0, len(items), list(range(len(items))), need)]
    # no two buffers share a byte, every one lies inside its pass's workspace - the decoder-input buffer, which the record
    # describes as its last user leaves it, for each of its four users
    spans = []
    for views, base, n, _members, size in passes:
        for vi, v in enumerate(views):
            end = v["offset"] + 4 * n * v["h"] * v["w"] * v["c"]
            assert 0 <= v["offset"] and end <= size, (case, vi)
            spans.append((base + v["offset"], base + end))
        for li in range(13, 17):
            assert views[21]["offset"] + 4 * n * views[li]["h"] * views[li]["w"] * dims[li][0] <= size, (case, li)
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "two buffers of one pass share workspace bytes"
    assert spans[-1][1] <= need
    figures, head_feat, head_conf = [], 0.0, 0.0
    for views, base, n, members, _size in passes:
        def stored(vi, im):
            v = views[vi]
            a = np.frombuffer(ws, np.float32, n * v["h"] * v["w"] * v["c"], base + v["offset"])
            return a.reshape(n, v["h"], v["w"], v["c"])[im]

        for im, item in enumerate(members):
            image, mask, normalize = host[item]
            tag = f"{case} image {item}"

            def check(li, ref, got):
                assert np.isfinite(got).all(), (tag, li)
                err = float(np.abs(got.astype(np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))
                v = views[li]
                figures.append((tag, li, v["cfg"], err))
                print(f"{tag}: layer {li:2d} {v['w']}x{v['h']} cfg {v['cfg']} max|err|/max(1,max|ref|) = {err:.3e}")
                assert err < LAYER_BAR, (tag, li, err)

            # encoder: the first layer from the image, the others from the stored fp32 input the kernel read
            check(0, _first_layer_f64(image, mask, *conv[0]), stored(0, im))
            for li in range(1, 13):
                b = max(k for k in range(5) if BLOCK_FIRST[k] <= li)
                src = 17 + b - 1 if li == BLOCK_FIRST[b] else li - 1   # the pooled plane, or the previous layer
                check(li, _conv3x3_f64(stored(src, im).astype(np.float64), *conv[li]), stored(li, im))
            # pools: bit for bit the 2x2 max of the stored layer (floor: an odd last row / column is dropped)
            for b in range(1, 5):
                src, got = stored(BLOCK_LAST[b - 1], im), stored(17 + b - 1, im)
                h2, w2 = got.shape[:2]
                assert (h2, w2) == (src.shape[0] // 2, src.shape[1] // 2)
                want = src[: 2 * h2, : 2 * w2].reshape(h2, 2, w2, 2, -1).max((1, 3))
                assert np.array_equal(got, want), (tag, "pool", b)
            # decoder: torch's bilinear x2 of the stored previous layer in float64, then the stored skip cropped to it
            for d in range(4):
                li = 13 + d
                up = _bilinear_x2_f64(stored(li - 1, im).astype(np.float64))
                skip = stored(BLOCK_LAST[3 - d], im)[: up.shape[0], : up.shape[1]]
                assert skip.shape[:2] == up.shape[:2] and up.shape[2] + skip.shape[2] == dims[li][0]
                check(li, _conv3x3_f64(np.concatenate([up, skip.astype(np.float64)], -1), *conv[li]), stored(li, im))
            # the decoder-input buffer as layer 16 read it: [upsampled layer 15 | layer 1 cropped]
            prev, cat = stored(15, im), stored(21, im)
            cp = prev.shape[2]
            assert np.isfinite(cat).all()
            assert np.array_equal(cat[..., cp:], stored(1, im)[: cat.shape[0], : cat.shape[1]]), (tag, "skip crop")
            eu = float(np.abs(cat[..., :cp] - _bilinear_x2_f64(prev.astype(np.float64))).max()) / float(np.abs(prev).max())
            print(f"{tag}: decoder input, upsampled channels max|err|/max|prev| = {eu:.3e} (bar {UPSAMPLE_BAR:.3e})")
            assert eu <= UPSAMPLE_BAR, (tag, eu)
            # the heads on the stored fp32 layers they read
            for k, src in enumerate(HEAD_SOURCE):
                f, c = _head_f64(stored(src, im).astype(np.float64), *heads[k], normalize)
                o, dim = outs[item][k], OUTPUT_DIMS[k]
                assert o.shape[:2] == f.shape[:2] and np.isfinite(o).all() and (o[..., dim + 1:] == 0).all(), (tag, k)
                ef = float(np.abs(o[..., :dim] - f).max() / np.abs(f).max())
                ec = float(np.abs(o[..., dim] - c).max())
                print(f"{tag}: head {k} features max|err|/max|ref| = {ef:.3e}  confidence max|err| = {ec:.3e}")
                head_feat, head_conf = max(head_feat, ef), max(head_conf, ec)
                assert ef < HEAD_FEATURE_BAR and ec < HEAD_CONF_BAR, (tag, k, ef, ec)
    return figures, head_feat, head_conf


@pytest.mark.parametrize("case", list(CASES))
def test_every_layer_matches_its_float64_replay(net, case):
    figures, head_feat, head_conf = _replay(net, case)
    worst = max(figures, key=lambda f: f[3])
    print(f"{case}: worst layer {worst[1]} (cfg {worst[2]}) {worst[3]:.3e}; heads: features {head_feat:.3e}, "
          f"confidence {head_conf:.3e}")
