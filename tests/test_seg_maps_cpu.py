"""The layout rules of segmentation._Maps, a list of uint8 maps in one flat buffer, on CPU tensors.  Every expected offset and
size is written out by hand from the rules: contiguous views of one storage are used where they lie; anything else is copied
into a zeroed buffer at offsets that are multiples of 4; ground truths lie gapless one after the other."""
import torch

from segclip_amd.segmentation import _Maps

SEPARATE_SIZES = [(3, 3), (1, 1), (2, 5)]


def _separate():
    g = torch.Generator().manual_seed(1)
    return [torch.randint(1, 256, hw, generator=g, dtype=torch.uint8) for hw in SEPARATE_SIZES]


def _views_of_one_buffer():
    buf = torch.arange(1, 61, dtype=torch.uint8)
    return buf, [buf[0:12].view(3, 4), buf[12:37].view(5, 5), buf[40:47].view(1, 7)]


def test_views_of_one_buffer_are_used_in_place():
    buf, views = _views_of_one_buffer()
    m = _Maps.of(views)
    assert m.flat.data_ptr() == buf.data_ptr() and m.flat.numel() == 47 and m.flat.dtype == torch.uint8
    assert m.offs == [0, 12, 40] and m.sizes == [(3, 4), (5, 5), (1, 7)]
    assert all(v.data_ptr() == w.data_ptr() for v, w in zip(m.views(), views))
    # the buffer starts at the first map, wherever that lies in the storage
    m = _Maps.of(views[1:])
    assert m.flat.data_ptr() == buf.data_ptr() + 12 and m.flat.numel() == 35 and m.offs == [0, 28]


def test_separate_tensors_are_copied_to_multiples_of_4():
    maps = _separate()
    m = _Maps.of(maps)
    assert m.offs == [0, 12, 16] and m.flat.numel() == 28 and m.sizes == SEPARATE_SIZES
    assert all(m.flat.data_ptr() != t.data_ptr() for t in maps)
    assert all(torch.equal(v, t) for v, t in zip(m.views(), maps))
    used = torch.zeros(28, dtype=torch.bool)
    for o, n in zip([0, 12, 16], [9, 1, 10]):
        used[o:o + n] = True
    assert int(used.sum()) == 20 and bool((m.flat[~used] == 0).all()) and bool((m.flat[used] != 0).all())


def test_a_view_that_is_not_contiguous_forces_the_copy():
    buf = torch.arange(1, 61, dtype=torch.uint8)
    t = buf[0:24].view(4, 6)
    views = [t[:, ::2], buf[24:30].view(2, 3)]
    m = _Maps.of(views)
    assert m.flat.untyped_storage().data_ptr() != buf.untyped_storage().data_ptr()
    assert m.offs == [0, 12] and m.flat.numel() == 20 and m.sizes == [(4, 3), (2, 3)]
    assert all(torch.equal(v, w) for v, w in zip(m.views(), views))


def test_gapless():
    buf = torch.arange(1, 61, dtype=torch.uint8)
    packed = _Maps.of([buf[5:17].view(3, 4), buf[17:42].view(5, 5)])
    assert packed.offs == [0, 12] and packed.gapless() is packed.flat
    for m in (_Maps.of(_views_of_one_buffer()[1]), _Maps.of(_separate())):
        flat = m.gapless()
        assert flat.dim() == 1 and flat.numel() == sum(h * w for h, w in m.sizes)
        assert torch.equal(flat, torch.cat([v.reshape(-1) for v in m.views()]))
    # maps that fill their buffer in another order than the list's are not gapless as they lie
    swapped = _Maps.of([buf[12:37].view(5, 5), buf[0:12].view(3, 4)])
    assert swapped.offs == [12, 0] and torch.equal(swapped.gapless(), torch.cat([buf[12:37], buf[0:12]]))


def test_gapless_of_ground_truths():
    gts = _separate()
    flat, offs = _Maps.gapless_of(gts)
    assert offs == [0, 9, 10] and flat.numel() == 20 and torch.equal(flat, torch.cat([g.reshape(-1) for g in gts]))
    one, offs = _Maps.gapless_of(gts[2:])
    assert offs == [0] and one.data_ptr() == gts[2].data_ptr()       # a single ground truth is not copied
    assert _Maps.gapless_of(None) == (None, None)


def test_empty_like():
    m = _Maps.of(_separate())
    out = m.empty_like()
    assert out.offs == [0, 12, 16] and out.sizes == SEPARATE_SIZES and out.flat.numel() == 28 and out.flat.dtype == torch.uint8
    assert out.flat.data_ptr() != m.flat.data_ptr()
    for v in out.views():
        v.fill_(7)
    assert int((out.flat == 0).sum()) == 8 and int((out.flat == 7).sum()) == 20      # the bytes between the maps are zero
    # without gaps only the layout is required, not the contents
    buf = torch.arange(1, 61, dtype=torch.uint8)
    packed = _Maps.of([buf[0:12].view(3, 4), buf[12:37].view(5, 5)]).empty_like()
    assert packed.offs == [0, 12] and packed.flat.numel() == 37 and packed.flat.data_ptr() != buf.data_ptr()


def test_views_round_trip():
    maps = _separate()
    m = _Maps(torch.zeros(40, dtype=torch.int32), [4, 20, 28], SEPARATE_SIZES)     # a kernel's output buffer, any dtype
    for v, t in zip(m.views(), maps):
        v.copy_(t)
    again = _Maps(m.flat, m.offs, m.sizes).views()
    assert [tuple(v.shape) for v in again] == SEPARATE_SIZES and all(v.dtype == torch.int32 for v in again)
    assert all(torch.equal(v, t.int()) for v, t in zip(again, maps))
    assert int(m.flat.sum()) == sum(int(t.sum()) for t in maps)
