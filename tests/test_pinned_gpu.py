"""pinned.PinnedRing and pinned.SensorStage: the two host mechanisms every frame hand-off goes through (no kernel of the
package is launched here: pinned allocations and one copy)."""
import numpy as np
import pytest
import torch

from pixtrack_amd.pinned import PinnedRing, SensorStage

pytestmark = pytest.mark.gpu


def test_a_ring_of_three_hands_out_three_pinned_blocks_and_wraps(device):
    ring = PinnedRing((4, 6), torch.float32, n=3)
    blocks = [ring.next() for _ in range(3)]
    assert len({b.data_ptr() for b in blocks}) == 3
    assert all(b.is_pinned() and tuple(b.shape) == (4, 6) and b.dtype == torch.float32 and not b.any() for b in blocks)
    fourth = ring.next()
    assert fourth.data_ptr() == blocks[0].data_ptr() and tuple(fourth.shape) == (4, 6)
    # next(rows): a view of the next block's first rows
    blocks[1][:] = torch.arange(24, dtype=torch.float32).reshape(4, 6)
    head = ring.next(2)
    assert tuple(head.shape) == (2, 6) and head.data_ptr() == blocks[1].data_ptr() and head.is_pinned()
    assert torch.equal(head, blocks[1][:2])
    head[1, 5] = -7.0
    assert float(blocks[1][1, 5]) == -7.0


def test_a_ring_asked_for_more_rows_allocates_all_its_blocks_anew(device):
    ring = PinnedRing((4, 6), torch.int32, n=3)
    old = [ring.next() for _ in range(3)]
    assert ring.next(4).data_ptr() == old[0].data_ptr()  # (as many rows as there are: no new blocks)
    big = [ring.next(9) for _ in range(3)]
    assert all(tuple(b.shape) == (9, 6) and b.is_pinned() and b.dtype == torch.int32 for b in big)
    assert len({b.data_ptr() for b in big}) == 3 and not {b.data_ptr() for b in big} & {b.data_ptr() for b in old}
    assert ring.next(9).data_ptr() == big[0].data_ptr()  # keeps wrapping
    assert ring.shape[0] >= 9 and tuple(ring.next().shape) == (ring.shape[0], 6)
    small = ring.next(2)  # fewer rows again: a view, no new blocks
    assert tuple(small.shape) == (2, 6) and small.data_ptr() == big[2].data_ptr()


def test_a_record_ring_has_one_dimension(device):
    ring = PinnedRing((16,), torch.float32)
    blocks = [ring.next() for _ in range(9)]
    assert len({b.data_ptr() for b in blocks[:8]}) == 8 and blocks[8].data_ptr() == blocks[0].data_ptr()
    assert all(tuple(b.shape) == (16,) and b.is_pinned() for b in blocks)


def test_a_sensor_image_arrives_with_its_sixteen_bit_patterns(device):
    stage = SensorStage(device)
    image = np.arange(35, dtype=np.uint16).reshape(5, 7) * 1871
    image[0, :5] = (0, 1, 32767, 32768, 65535)
    dev = stage.upload(image, "000001.png")
    torch.cuda.synchronize(device)
    assert dev.device.type == "cuda" and dev.dtype == torch.int16 and tuple(dev.shape) == (5, 7)
    assert np.array_equal(dev.cpu().numpy().view(np.uint16), image)
    assert stage.host.is_pinned()
    # a second image of the same shape: the same two buffers
    ptrs = (stage.host.data_ptr(), dev.data_ptr())
    second = np.ascontiguousarray(image[::-1])
    dev2 = stage.upload(second, "000002.png")
    torch.cuda.synchronize(device)
    assert (stage.host.data_ptr(), dev2.data_ptr()) == ptrs
    assert np.array_equal(dev2.cpu().numpy().view(np.uint16), second)
    # a non-contiguous image is taken as its contiguous copy
    dev3 = stage.upload(image.T[:5, :5].T[:, ::-1], "000003.png")
    torch.cuda.synchronize(device)
    assert np.array_equal(dev3.cpu().numpy().view(np.uint16), image[:5, :5][:, ::-1])
    # another shape: new buffers (the old device buffer stays alive here, so a new one cannot take its address)
    tall = np.full((6, 7), 40000, np.uint16)
    dev4 = stage.upload(tall, "000004.png")
    torch.cuda.synchronize(device)
    assert tuple(dev4.shape) == (6, 7) and dev4.data_ptr() not in (dev.data_ptr(), dev3.data_ptr())
    assert tuple(stage.host.shape) == (6, 7) and np.array_equal(dev4.cpu().numpy().view(np.uint16), tall)


@pytest.mark.parametrize("image,said", [(np.zeros((5, 7), np.float32), "float32 (5, 7)"),
                                        (np.zeros((5, 7), np.int16), "int16 (5, 7)"),
                                        (np.zeros((5, 7, 1), np.uint16), "uint16 (5, 7, 1)")],
                         ids=("float32", "int16", "three_dimensions"))
def test_anything_but_uint16_h_w_is_refused_in_the_trackers_words(device, image, said):
    stage = SensorStage(device)
    with pytest.raises(ValueError) as e:
        stage.upload(image, "dir/000007.png")
    assert str(e.value) == f"the sensor depth image of dir/000007.png is {said}, not uint16 [H, W]"
    assert stage.host is None and stage.dev is None  # (refused before anything is allocated)
