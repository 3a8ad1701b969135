"""`MultiImageMultiBBoxDataset(..., decode="device")` on the host side: baseline JPEG files travel as `EncodedImage` (bytes + header
+ plan) through `Util.transform`, `collate_fn` and a `DataLoader(num_workers=2)`, everything else as a PIL-decoded `RawImage`;
the plans, boxes and sizes are those `decode="host"` draws under the same seed.  Nothing here touches the GPU."""
import inspect
import random

import numpy as np
import torch
from PIL import Image

import jpeg_ref as J


def _files(tmp_path):
    rng = np.random.default_rng(5)
    paths = []
    for i, (h, w) in enumerate([(40, 56), (33, 31), (64, 48), (50, 50)]):
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = str(tmp_path / f"i{i}.jpg")
        if i == 2:
            Image.fromarray(px).save(p, "JPEG", quality=85, progressive=True)
        else:
            Image.fromarray(px).save(p, "JPEG", quality=85, subsampling=("4:2:0", "4:4:4", None, "4:2:2")[i])
        paths.append(p)
    n = len(paths)
    return paths, [[[1., 2., 20., 25.], [3., 3., 15., 28.]]] * n, [["dog", "cat"]] * n, [[0, 1]] * n, list(range(n))


def test_decode_keyword_is_last_and_defaults_to_host():
    from objectdetection_ssd_amd import Dataset
    params = list(inspect.signature(Dataset.MultiImageMultiBBoxDataset.__init__).parameters.values())
    assert params[-1].name == "decode" and params[-1].default == "host"
    assert [p.name for p in params[1:8]] == ["all_images", "all_multi_bboxes", "all_multi_labels", "all_difficulties", "all_indices",
                                             "isTest", "keep_difficult"]
    try:
        Dataset.MultiImageMultiBBoxDataset([], [], [], [], [], decode="gpu")
    except ValueError:
        pass
    else:
        raise AssertionError("an unknown decode mode must be refused")


def test_items_are_the_host_modes_items_without_pixels(tmp_path):
    from objectdetection_ssd_amd import Dataset
    args = _files(tmp_path)
    host = Dataset.MultiImageMultiBBoxDataset(*args)
    dev = Dataset.MultiImageMultiBBoxDataset(*args, decode="device")
    for test_mode in (True, False):
        host.isTest = dev.isTest = test_mode
        for i in range(len(host)):
            random.seed(100 + i)
            a = host[i]
            random.seed(100 + i)
            b = dev[i]
            assert type(a[0]) is Dataset.RawImage                                 # decode="host": unchanged in type
            assert type(b[0]) is (Dataset.RawImage if i == 2 else Dataset.EncodedImage)
            assert a[0].plan == b[0].plan and a[0].size == b[0].size
            assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]
            if i == 2:
                assert np.array_equal(a[0].pixels, b[0].pixels)
            else:
                with open(args[0][i], "rb") as f:
                    assert b[0].data == f.read()
                assert (b[0].header.width, b[0].header.height) == Image.open(args[0][i]).size


def test_device_mode_through_dataloader_workers(tmp_path):
    from objectdetection_ssd_amd import Dataset
    args = _files(tmp_path)
    ds = Dataset.MultiImageMultiBBoxDataset(*args, isTest=True, decode="device")
    dl = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=2, collate_fn=Dataset.collate_fn)
    batches = list(dl)
    assert len(batches) == 1
    inputs, classes, boxes, indices = batches[0]
    assert isinstance(inputs, Dataset.RawBatch) and not inputs.arena.is_cuda and inputs.arena.dtype == torch.uint8
    assert inputs.shape == (4, 3, 300, 300) and indices == [0, 1, 2, 3]
    assert [h is not None for h in inputs.headers] == [True, True, False, True]
    assert inputs.decode_status is None                                           # set by .to(device)
    # pixel slots by today's rule, one per image; on the host only the progressive image's pixels and the three streams exist
    sizes = [(40, 56), (33, 31), (64, 48), (50, 50)]
    offs, total = [], 0
    for h, w in sizes:
        offs.append(total)
        total += (h * w * 3 + 255) & ~255
    assert inputs.offsets == offs
    streams = [h.data_end - h.data_begin for h in inputs.headers if h is not None]
    assert inputs.arena.numel() == ((64 * 48 * 3 + 255) & ~255) + sum((s + 15) & ~15 for s in streams)
    assert inputs.device_bytes == total + sum((s + 15) & ~15 for s in streams)
    assert inputs.arena.numel() < total                                           # pixel slots of encoded images are not materialised
    hv = inputs.arena.numpy()
    assert np.array_equal(hv[inputs.host_offsets[2]:inputs.host_offsets[2] + 64 * 48 * 3].reshape(64, 48, 3),
                          np.asarray(Image.open(args[0][2]).convert("RGB")))
    for i in (0, 1, 3):
        data = open(args[0][i], "rb").read()
        h = inputs.headers[i]
        assert bytes(hv[inputs.host_offsets[i]:inputs.host_offsets[i] + h.data_end - h.data_begin]) == data[h.data_begin:h.data_end]
        assert J.parse(data)["seg_offsets"] == h.seg_offsets.tolist()
    for p, (h, w) in zip(inputs.plans, sizes):
        assert p == Dataset.identity_plan(h, w)
    pinned_like = Dataset.RawBatch(inputs.arena, inputs.offsets, inputs.plans, inputs.out_hw, inputs.headers, inputs.host_offsets,
                                   inputs.device_bytes)
    assert pinned_like.device_bytes == inputs.device_bytes
    try:
        inputs.to("cpu")
    except RuntimeError as e:
        assert "no CPU fallback" in str(e)
    else:
        raise AssertionError("no CPU rendering")


def test_pack_batch_takes_bytes_and_keeps_host_batches_as_they_were(tmp_path):
    from objectdetection_ssd_amd import Dataset
    args = _files(tmp_path)
    blobs = [open(p, "rb").read() for p in args[0]]
    rb = Dataset.pack_batch(blobs)
    assert [h is not None for h in rb.headers] == [True, True, False, True]
    px = [np.asarray(Image.open(p).convert("RGB")) for p in args[0]]
    host = Dataset.pack_batch(px)
    assert host.headers is None and host.decode_status is None and host.offsets == rb.offsets
    assert host.arena.numel() == sum((a.size + 255) & ~255 for a in px)
    only_pil = Dataset.pack_batch([blobs[2]])                                     # no stream in the batch: a plain host batch
    assert only_pil.headers is None and only_pil.arena.numel() == (64 * 48 * 3 + 255) & ~255
    try:
        Dataset.pack_batch(blobs, [Dataset.identity_plan(1, 1)] * 4)
    except ValueError as e:
        assert "plan does not belong" in str(e)
    else:
        raise AssertionError("a plan of another size must be refused")
