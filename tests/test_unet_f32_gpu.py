"""The UNet's fp32 pass (UNet(..., precision="fp32"), pxt_unet_create_f32): fp32 activations, 3x3 convolutions on the
exact f32-input MFMA.  Against the fp32 PyTorch-CPU oracle the bars are 1e-4 x max|ref| per level and 2e-5 on the
confidences (the fp16 pass's are 2e-2 and 5e-3); each image's maps are the same bits whatever batch or pair it rides in;
checkpoints whose activations overflow fp16 run as they are."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_oracle as UO
from pixtrack_amd import _lib
from pixtrack_amd.unet import OUTPUT_DIMS, UNet, make_synthetic_unet_weights

pytestmark = pytest.mark.gpu

FEAT_BAR, CONF_BAR = 1e-4, 2e-5


@pytest.mark.parametrize("H,W,Cin,Cout,relu", [(16, 16, 16, 32, 1), (37, 50, 64, 64, 1), (20, 33, 128, 96, 0),
                                               (30, 40, 512, 128, 1), (7, 5, 32, 160, 1), (48, 64, 1024, 64, 1)])
def test_conv3x3_f32_layer_matches_conv2d(device, H, W, Cin, Cout, relu):
    """pxt_conv3x3_nhwc_f32 against F.conv2d in float64: asymmetric random operands catch transposed fragments."""
    g = torch.Generator().manual_seed(H * 1000 + W + Cin)
    x = torch.randn(Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(x.double()[None], w.double(), b.double(), padding=1)[0]
    if relu:
        ref = F.relu(ref)
    xd = x.permute(1, 2, 0).contiguous().to(device)
    wd = w.permute(0, 2, 3, 1).contiguous().to(device)
    bd = b.to(device)
    out = torch.full((H, W, Cout), float("nan"), dtype=torch.float32, device=device)
    _lib.check(_lib.lib().pxt_conv3x3_nhwc_f32(xd.data_ptr(), H, W, Cin, wd.data_ptr(), bd.data_ptr(), Cout, relu,
                                               out.data_ptr(), _lib.stream_ptr(device)), "pxt_conv3x3_nhwc_f32")
    torch.cuda.synchronize()
    got = out.double().cpu().permute(2, 0, 1)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    assert err < 1e-5 * max(1.0, ref.abs().max().item()), err


def _image(H, W, seed, u8):
    rng = np.random.default_rng(seed)
    img = rng.uniform(0, 255, size=(H, W, 3)).astype(np.float32)
    img = (img + np.roll(img, 1, 0) + np.roll(img, 1, 1) + np.roll(img, 2, 0)) / 4
    return np.floor(img).astype(np.uint8) if u8 else img


def _errors(outs, feats, confs, normalize):
    """per level: (max |feature error| / max |ref|, max |confidence error|)"""
    errs = []
    for k, (o, c) in enumerate(zip(outs, OUTPUT_DIMS)):
        o = o.cpu()
        f_ref = feats[k].permute(1, 2, 0)
        assert o.shape[:2] == f_ref.shape[:2], (o.shape, f_ref.shape)
        if normalize:
            f_ref = f_ref / f_ref.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        assert torch.isfinite(o).all(), k
        assert (o[..., c + 1:] == 0).all(), k
        errs.append(((o[..., :c] - f_ref).abs().max().item() / f_ref.abs().max().item(),
                     (o[..., c] - confs[k][0]).abs().max().item()))
    return errs


@pytest.mark.parametrize("H,W", [(64, 48), (96, 128), (75, 100)])
@pytest.mark.parametrize("variant", ["float", "mask_u8_normalize", "mask_float_normalize"])
def test_fp32_pyramid_matches_the_oracle(device, H, W, variant, capsys):
    w = make_synthetic_unet_weights(seed=3, bn_trivial=False)
    u8 = variant == "mask_u8_normalize"
    normalize = variant != "float"
    img = _image(H, W, H + W, u8)
    mask = None
    if variant != "float":
        mask = (np.random.default_rng(H * W).uniform(size=(H, W)) > 0.3).astype(np.uint8)
    img_ref = img.astype(np.float32) * (mask[..., None] if mask is not None else 1.0)
    feats, confs = UO.unet_forward(w, torch.from_numpy(img_ref).permute(2, 0, 1) / 255.0)
    src = torch.from_numpy(img).to(device)
    md = torch.from_numpy(mask).to(device) if mask is not None else None
    net32, net16 = UNet(w, device, precision="fp32"), UNet(w, device)
    assert net32.precision == "fp32" and net16.precision == "fp16"
    assert _lib.lib().pxt_unet_precision(net32._ctx) == 32 and _lib.lib().pxt_unet_precision(net16._ctx) == 16
    e32 = _errors(net32.forward_packed(src, md, normalize=normalize), feats, confs, normalize)
    e16 = _errors(net16.forward_packed(src, md, normalize=normalize), feats, confs, normalize)
    with capsys.disabled():
        print(f"\n{H}x{W} {variant}: level | fp32 feature / conf error | fp16 feature / conf error")
        for k in range(3):
            print("   %d | %.2e %.2e | %.2e %.2e" % (k, *e32[k], *e16[k]))
    for k, (fe, ce) in enumerate(e32):
        assert fe <= FEAT_BAR and ce <= CONF_BAR, (k, fe, ce)


def _items(device, specs):
    out = []
    for H, W, seed, u8, masked, normalize in specs:
        img = torch.from_numpy(_image(H, W, seed, u8)).to(device)
        m = None
        if masked:
            m = torch.from_numpy((np.random.default_rng(seed).uniform(size=(H, W)) > 0.3).astype(np.uint8)).to(device)
        out.append((img, m, normalize))
    return out


@pytest.mark.parametrize("n", [3, 16])
def test_fp32_batch_equals_single_passes_bit_for_bit(device, n):
    """No split-K, no atomics, one fixed K order per value: an image's maps do not depend on the batch it rides in (the fp16
    pass needs set_batch_plan(1) for this); set_batch_plan and set_tile_skip change nothing."""
    net = UNet(make_synthetic_unet_weights(seed=5), device, precision="fp32")
    items = _items(device, [(72, 88, 100 + i, i % 2 == 0, i % 3 == 0, i % 2 == 1) for i in range(n)])
    single = [[o.clone() for o in net.forward_packed(*it)] for it in items]
    batch = net.forward_packed_batch(items)
    net.set_batch_plan(True)
    net.set_tile_skip(False)
    planned = net.forward_packed_batch(items)
    torch.cuda.synchronize()
    for i in range(n):
        for k in range(3):
            assert torch.equal(batch[i][k], single[i][k]), (i, k)
            assert torch.equal(planned[i][k], single[i][k]), (i, k)


def test_fp32_pair_of_two_sizes_and_repeat_are_bit_identical(device):
    net = UNet(make_synthetic_unet_weights(seed=5), device, precision="fp32")
    a, b = _items(device, [(144, 191, 11, True, False, False), (240, 320, 12, False, True, True)])
    single_a = [o.clone() for o in net.forward_packed(*a)]
    single_b = [o.clone() for o in net.forward_packed(*b)]
    both = net.forward_packed_batch([a, b])
    swapped = net.forward_packed_batch([b, a])
    again = net.forward_packed_batch([a, b])
    net.set_defer_join(True)  # the first image's maps are complete on return; join() makes the second safe
    deferred = net.forward_packed_batch([a, b])
    net.join()
    torch.cuda.synchronize()
    for k in range(3):
        for got_a, got_b in ((both[0][k], both[1][k]), (swapped[1][k], swapped[0][k]), (again[0][k], again[1][k]),
                             (deferred[0][k], deferred[1][k])):
            assert torch.equal(got_a, single_a[k]) and torch.equal(got_b, single_b[k]), k


@pytest.mark.parametrize("factor", [3.5, 12.0])
def test_checkpoints_fp16_cannot_hold_run_in_fp32(device, factor, capsys):
    """Every 3x3 filter of the synthetic weights x 3.5 / x 12: the fp16 pass overflows (tests/test_unet_gpu.py); the fp32
    pass gives finite maps that match the oracle of those same weights, with no rescaling."""
    w = make_synthetic_unet_weights(7)
    big = {k: (v * factor if (v.dim() == 4 and v.shape[-1] == 3) else v) for k, v in w.items()}
    img = _image(96, 128, 5, False)
    src = torch.from_numpy(img).to(device)
    raw16 = UNet(big, device).forward_packed(src, None, normalize=True)
    assert not all(bool(torch.isfinite(o).all()) for o in raw16)
    feats, confs = UO.unet_forward(big, torch.from_numpy(img).permute(2, 0, 1) / 255.0)
    e32 = _errors(UNet(big, device, precision="fp32").forward_packed(src, None, normalize=True), feats, confs, True)
    with capsys.disabled():
        print(f"\nfilters x {factor}: level | fp32 feature / conf error (fp16: non-finite)")
        for k in range(3):
            print("   %d | %.2e %.2e" % (k, *e32[k]))
    for k, (fe, ce) in enumerate(e32):
        assert fe <= FEAT_BAR and ce <= CONF_BAR, (k, fe, ce)


def test_fp32_activation_stats_report_what_fp16_cannot_store(device):
    w = make_synthetic_unet_weights(7)
    img = (torch.rand(120, 160, 3, generator=torch.Generator().manual_seed(3)) * 255).to(device)
    st = UNet(w, device, precision="fp32").activation_stats(img)
    assert len(st) == 17 and all(s is not None for s in st), st  # every layer is in memory in the fp32 pass
    assert all(n == 0 for _, n in st) and all(1e-3 < m < 6.0e4 for m, _ in st), st
    big = {k: (v * 12.0 if (v.dim() == 4 and v.shape[-1] == 3) else v) for k, v in w.items()}
    st2 = UNet(big, device, precision="fp32").activation_stats(img)
    assert all(n == 0 for _, n in st2), st2
    assert max(m for m, _ in st2) > 65504.0, st2
