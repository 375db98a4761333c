"""Share of the last two decoder layers' tiles a sampled reference pass computes on the benchmark's view.

    python scripts/reference_tile_share.py [frames]

Tracks the first frames of bench.py's default sequence (seed 1002, 640 x 480), takes the sample-point record the refiner
hands each warm frame's reference pass (PoseTrackerRefiner.reference_sample_points) and evaluates the flag rule on the
host (pxt_unet_reference_tiles_host: the device kernel's own functions) for 16-row tiles, the decoder's configurations."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from pixtrack_amd import _lib  # noqa: E402
from pixtrack_amd.pose_trackers.pixloc_tracker_r9 import PixLocPoseTrackerR9  # noqa: E402
from pixtrack_amd.synthetic import make_tracking_assets, render_query_frames  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    dev = torch.device("cuda:0")
    assets = make_tracking_assets(seed=1002, width=640, height=480, n_frames=n)
    tr = PixLocPoseTrackerR9("", "", "", "/tmp", debug=0, device=dev, assets=assets)
    frames = render_query_frames(assets, tr.testbed)
    refiner = tr.localizer.refiner
    records = []
    inner = refiner.reference_sample_points

    def spy(image_id, pose, p3d, image, image_scale, window):
        rec = inner(image_id, pose, p3d, image, image_scale, window)
        if rec is not None:
            records.append((rec, tuple(int(x) for x in image.shape[:2])))
        return rec

    refiner.reference_sample_points = spy
    for i, f in enumerate(frames):
        tr.run_single_frame((f"{i:06d}.png", f))
    L = _lib.lib()
    for k, (rec, hw) in enumerate(records):
        fh, fw = tr.localizer.extractor.model.level_shapes(*hw)[0]
        xyz = np.ascontiguousarray(rec["p3d"].detach().cpu().numpy(), np.float32)
        pts = _lib.UnetSamplePoints()
        pts.p3d, pts.n_points = xyz.ctypes.data, len(xyz)
        pts.T[:] = rec["pose_camera"][:12]
        pts.cam[:] = rec["pose_camera"][12:]
        pts.ndist, pts.pad, pts.x0, pts.y0, pts.full_w, pts.full_h = rec["ints"]
        fine = np.zeros((-(-fh // 16), -(-fw // 16)), np.uint8)
        low = np.zeros((-(-(fh // 2) // 16), -(-(fw // 2) // 16)), np.uint8)
        _lib.check(L.pxt_unet_reference_tiles_host(C.byref(pts), fh, fw, 16, 16, fine.ctypes.data, low.ctypes.data),
                   "pxt_unet_reference_tiles_host")
        print(f"reference pass {k}: fine map {fw} x {fh}, {len(xyz)} points; last layer {int(fine.sum())} of {fine.size} "
              f"tiles ({100.0 * fine.mean():.1f} %), layer before {int(low.sum())} of {low.size} ({100.0 * low.mean():.1f} %)")


if __name__ == "__main__":
    main()
