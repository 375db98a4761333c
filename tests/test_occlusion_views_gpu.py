"""pxt_occlusion_mask_views (csrc/pxt_occlusion.hip; torch.ops.pixtrack.occlusion_mask_views): up to 16 image pairs of
different sizes in one chain of two launches.

Every view's two planes and its record are compared BIT FOR BIT, no tolerance and no pixel left out, with
 * occlusion.occlusion_mask_reference (the numpy float32 restatement, tests/test_occlusion_host.py), and
 * a pxt_occlusion_mask call on the same pair alone (all 16 record words).
The inputs are those of tests/test_occlusion_gpu.py (quarter-integer depths and counts: many q - d_s == delta_q ties, one
+inf depth and one NaN alpha per image), the sensor images sit between guard arrays, canaries sit behind every output
plane and behind the records.  Sizes on both sides of the 64 x 16 tile's edges; 1, 2, 3 and 16 (a full table) views."""
import numpy as np
import pytest
import torch

import test_occlusion_gpu as single
from pixtrack_amd import _lib, ops
from pixtrack_amd import occlusion as OC

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (3, 2), (63, 17), (64, 16), (65, 33), (161, 119), (1025, 2))
RADII = ((0, 0), (1, 3), (8, 8), (16, 0))
SHIFTS = ((0, 0), (1, 0), (-3, 2), (0, -1), (2, 5), (-1, -1))
QUANTA = ((0.25, 0.25), (0.5, 0.25), (0.25, 0.5), (0.125, 0.75))  # dyadic: products and differences stay exact, ties stay
MIN_ALPHA = single.MIN_ALPHA
CANARY, TAIL, SENTINEL = single.CANARY, single.TAIL, single.SENTINEL


class View:
    """One image pair: seeded inputs of a size, a shift and a pair of quanta; the oracle's answer per radii pair."""

    def __init__(self, size, seed, shift, quanta, device, sensor_of=None):
        self.W, self.H = size
        self.shift, self.quanta = shift, quanta
        self.img, sensor, self.mask = single._inputs(self.W, self.H, seed)
        if sensor_of is None:
            self.sensor = sensor
            self.whole, self.d_sensor = single._guarded(sensor, device)
        else:  # ONE sensor image for several views
            self.sensor, self.whole, self.d_sensor = sensor_of.sensor, sensor_of.whole, sensor_of.d_sensor
        self.d_img = torch.from_numpy(self.img).to(device)
        self.d_mask = torch.from_numpy(self.mask).to(device)
        self._ref = {}

    def ref(self, radii):
        if radii not in self._ref:
            self._ref[radii] = OC.occlusion_mask_reference(self.img, self.sensor, self.mask, self.shift, MIN_ALPHA,
                                                           self.quanta[0], self.quanta[1], *radii)
        return self._ref[radii]


@pytest.fixture(scope="module")
def tables(device):
    """The view tables of the module: name -> list of View."""
    mk = lambda i, size, **kw: View(size, 7000 + i, SHIFTS[i % len(SHIFTS)], QUANTA[i % len(QUANTA)], device, **kw)
    full = [mk(i, SIZES[i % len(SIZES)]) for i in range(16)]  # every size at least twice, each with inputs of its own
    first = mk(40, (161, 119))
    shared = [first, mk(41, (161, 119), sensor_of=first), mk(42, (161, 119), sensor_of=first)]
    t = {"one": [full[5]], "one_pixel": [full[0]], "two": [full[3], full[4]], "three": [full[6], full[0], full[2]],
         "sixteen": full, "one_sensor": shared}
    big = full[5].ref((1, 3))["record"]
    assert big[3] > 0 and big[2] > big[3] and 0 < big[6] < big[5]  # the opening leaves something and removes something
    assert shared[1].d_sensor.data_ptr() == shared[0].d_sensor.data_ptr()
    return t


class Outs:
    """Per view mask and occluder with canaries behind them; records [K, 16] with a sentinel row behind; a workspace."""

    def __init__(self, views, device, pinned_records=False):
        self.views = views
        K = len(views)
        self.flat = [[torch.full((v.W * v.H + TAIL,), CANARY, dtype=torch.uint8, device=device) for v in views] for _ in range(2)]
        self.masks = [f[:v.W * v.H].view(v.H, v.W) for f, v in zip(self.flat[0], views)]
        self.occluders = [f[:v.W * v.H].view(v.H, v.W) for f, v in zip(self.flat[1], views)]
        rec = torch.full((K + 1, OC.RECORD), SENTINEL, dtype=torch.int32)
        self.rec_all = rec.pin_memory() if pinned_records else rec.to(device)
        self.records = self.rec_all[:K]
        sizes = [x for v in views for x in (v.W, v.H)]
        need = int(_lib.lib().pxt_occlusion_mask_views_workspace_bytes(K, (_lib.C.c_int32 * (2 * K))(*sizes)))
        assert need == sum(((v.W + 63) // 64) * ((v.H + 15) // 16) for v in views) * 32
        self.ws = torch.empty(need, dtype=torch.uint8, device=device)

    def run(self, radii):
        vs = self.views
        OC.occlusion_mask_views([v.d_img for v in vs], [v.d_sensor for v in vs], [v.d_mask for v in vs],
                                [v.shift for v in vs], MIN_ALPHA, [v.quanta for v in vs], radii[0], radii[1],
                                masks=self.masks, occluders=self.occluders, records=self.records, workspace=self.ws)

    def get(self):
        torch.cuda.synchronize()
        for flats in self.flat:
            for f, v in zip(flats, self.views):
                assert (f[v.W * v.H:] == CANARY).all()
        assert (self.rec_all[len(self.views):] == SENTINEL).all()
        rec = self.records.cpu().numpy().copy()
        return [(m.cpu().numpy().copy(), o.cpu().numpy().copy(), rec[k]) for k, (m, o) in enumerate(zip(self.masks, self.occluders))]


def _single_call(v, radii, device):
    """pxt_occlusion_mask on the pair alone -> (mask, occluder, record)."""
    out = OC.occlusion_mask(v.d_img, v.d_sensor, v.d_mask, v.shift, MIN_ALPHA, v.quanta[0], v.quanta[1], radii[0], radii[1])
    torch.cuda.synchronize()
    return out["mask"].cpu().numpy(), out["occluder"].cpu().numpy(), out["record"].cpu().numpy()


@pytest.mark.parametrize("name", ("one", "one_pixel", "two", "three", "sixteen", "one_sensor"))
def test_every_view_matches_the_restatement_and_the_single_call(tables, device, name):
    views = tables[name]
    outs = Outs(views, device)
    for radii in RADII:
        outs.run(radii)
        for k, (v, (mask, occ, rec)) in enumerate(zip(views, outs.get())):
            what = f"{name} view {k} {v.W}x{v.H} radii {radii} shift {v.shift} quanta {v.quanta}"
            ref = v.ref(radii)
            assert np.array_equal(occ, ref["occluder"]), what
            assert np.array_equal(mask, ref["mask"]), what
            assert np.array_equal(rec, ref["record"]), (what, rec.tolist(), ref["record"].tolist())
            s_mask, s_occ, s_rec = _single_call(v, radii, device)
            assert np.array_equal(mask, s_mask) and np.array_equal(occ, s_occ) and np.array_equal(rec, s_rec), what
    for v in views:
        assert single._guards_untouched(v.whole)


def test_a_view_does_not_depend_on_its_place_or_its_neighbours(tables, device):
    """The full table reversed, rotated, and a view among other neighbours: the same bits per view; pinned records."""
    full = tables["sixteen"]
    base = Outs(full, device)
    base.run((1, 3))
    want = {id(v): got for v, got in zip(full, base.get())}
    for order in (full[::-1], full[5:] + full[:5], [full[9], full[5], full[0]], [full[5]]):
        outs = Outs(order, device, pinned_records=True)
        outs.run((1, 3))
        for v, got in zip(order, outs.get()):
            for x, y in zip(got, want[id(v)]):
                assert np.array_equal(x, y), (v.W, v.H)


def test_a_call_repeats_and_runs_beside_another_stream(tables, device):
    """The same call twice on one stream, and beside a different call on a second stream (own outputs and workspace):
    the same bits."""
    views, other = tables["sixteen"], tables["one_sensor"]
    a, b = Outs(views, device), Outs(other, device)
    a.run((8, 8))
    first = a.get()
    a.run((8, 8))
    second = a.get()
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    for _ in range(3):
        with torch.cuda.stream(side):
            b.run((1, 3))
        a.run((8, 8))
    side.synchronize()
    third, beside = a.get(), b.get()
    for x, y, z in zip(first, second, third):
        for p, q, r in zip(x, y, z):
            assert np.array_equal(p, q) and np.array_equal(p, r)
    for v, (mask, occ, rec) in zip(views, third):
        assert np.array_equal(rec, v.ref((8, 8))["record"]) and np.array_equal(mask, v.ref((8, 8))["mask"])
    for v, (mask, occ, rec) in zip(other, beside):
        assert np.array_equal(rec, v.ref((1, 3))["record"]) and np.array_equal(occ, v.ref((1, 3))["occluder"])


def test_bad_arguments_launch_nothing(tables, device):
    views = tables["three"]
    outs = Outs(views, device)
    L = _lib.lib()
    stream = _lib.stream_ptr(device)
    K = len(views)

    def table(edit=None, n=K):
        arr = (_lib.OcclusionView * max(n, 1))()
        for k in range(min(n, K)):
            v, a = views[k], arr[k]
            a.depth, a.sensor, a.mask_in = v.d_img.data_ptr(), v.d_sensor.data_ptr(), v.d_mask.data_ptr()
            a.mask_out, a.occluder = outs.masks[k].data_ptr(), outs.occluders[k].data_ptr()
            a.width, a.height, a.shift_x, a.shift_y = v.W, v.H, v.shift[0], v.shift[1]
            a.sensor_q, a.delta_q = v.quanta
        if edit:
            edit(arr)
        return arr

    def call(edit=None, n=K, ro=1, rg=3, rec=outs.records.data_ptr(), ws=outs.ws.data_ptr(), views_ptr=True):
        return L.pxt_occlusion_mask_views(table(edit, n) if views_ptr else None, n, MIN_ALPHA, ro, rg, rec, ws, stream)

    def setter(k, **kw):
        def edit(arr):
            for name, value in kw.items():
                setattr(arr[k], name, value)
        return edit

    m0, o0, m1 = outs.masks[0].data_ptr(), outs.occluders[0].data_ptr(), outs.masks[1].data_ptr()
    bad = [dict(n=0), dict(n=17), dict(n=-1), dict(views_ptr=False), dict(rec=None), dict(ws=None),
           dict(ro=9, rg=8), dict(ro=17, rg=0), dict(ro=-1), dict(rg=-1), dict(rec=outs.records.data_ptr() + 2),
           dict(ws=outs.ws.data_ptr() + 4)]
    bad += [dict(edit=setter(1, **{name: None})) for name in ("depth", "sensor", "mask_in", "mask_out", "occluder")]
    bad += [dict(edit=setter(2, width=0)), dict(edit=setter(2, height=0)), dict(edit=setter(0, width=-4)),
            dict(edit=setter(0, width=1 << 20, height=1 << 9)),              # 2^29 pixels
            dict(edit=setter(1, depth=views[1].d_img.data_ptr() + 4)),       # a misaligned depth plane
            dict(edit=setter(1, sensor=views[1].d_sensor.data_ptr() + 1)),
            dict(edit=setter(0, shift_x=32768)), dict(edit=setter(2, shift_y=-32768)),
            dict(edit=setter(0, occluder=m0)),                               # a view's two outputs are one plane
            dict(edit=setter(1, mask_out=o0)),                               # view 1 writes over view 0's occluder
            dict(edit=setter(1, occluder=m0 + 1)),                           # ... into the middle of view 0's mask
            dict(edit=setter(0, mask_out=views[1].d_mask.data_ptr())),       # an output over ANOTHER view's mask_in
            dict(edit=setter(1, occluder=views[1].d_mask.data_ptr())),       # the occluder over the view's own mask_in
            dict(edit=setter(2, mask_out=outs.records.data_ptr())),          # an output over the records
            dict(edit=setter(2, occluder=m1))]
    for kw in bad:
        assert call(**kw) == -1, kw  # PXT_E_ARG
    C = _lib.C
    assert int(L.pxt_occlusion_mask_views_workspace_bytes(0, (C.c_int32 * 2)(4, 4))) < 0
    assert int(L.pxt_occlusion_mask_views_workspace_bytes(17, (C.c_int32 * 34)(*([4] * 34)))) < 0
    assert int(L.pxt_occlusion_mask_views_workspace_bytes(1, (C.c_int32 * 2)(0, 4))) < 0
    assert int(L.pxt_occlusion_mask_views_workspace_bytes(1, None)) < 0
    torch.cuda.synchronize()
    for flats in outs.flat:
        for f in flats:
            assert (f == CANARY).all()
    assert (outs.rec_all == SENTINEL).all()
    with pytest.raises(_lib.PxtError):  # the op refuses what the library would
        ops.ops.occlusion_mask_views([v.d_img for v in views], [v.d_sensor for v in views], [v.d_mask for v in views],
                                     [0] * 6, MIN_ALPHA, [0.25] * 6, [9, 8], outs.masks, outs.occluders, outs.records, outs.ws)
    with pytest.raises(_lib.PxtError):
        ops.ops.occlusion_mask_views([v.d_img for v in views], [v.d_sensor for v in views], [v.d_mask for v in views],
                                     [0] * 6, MIN_ALPHA, [0.25] * 6, [1, 3], [outs.masks[0], outs.masks[1], outs.masks[2]],
                                     [outs.occluders[0], outs.occluders[1], outs.masks[2]], outs.records, outs.ws)
    torch.cuda.synchronize()
    assert (outs.rec_all == SENTINEL).all()
    # a view's mask_out may BE its own mask_in, as in the single call
    own = views[2].d_mask.clone()
    assert call(edit=setter(2, mask_in=own.data_ptr(), mask_out=own.data_ptr())) == 0
    torch.cuda.synchronize()
    assert np.array_equal(own.cpu().numpy(), views[2].ref((1, 3))["mask"])
    assert call() == 0
    for v, (mask, occ, rec) in zip(views, outs.get()):
        assert np.array_equal(rec, v.ref((1, 3))["record"]) and np.array_equal(mask, v.ref((1, 3))["mask"])
