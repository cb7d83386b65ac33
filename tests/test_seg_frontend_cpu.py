"""CPU: the yardstick of the segmentation front end (tests/seg_frontend_reference.py) against F.interpolate in fp64, and the
host-side parts of the product (ImageTransform.net_size, the no-CPU-fallback error of predict_raw)."""
import pytest
import torch
import torch.nn.functional as F

from tests import seg_frontend_reference as sfr

MEAN, STD = (122.7709383, 116.7460125, 104.09373615), (68.5005327, 66.6321579, 70.32316305)
# source (h, w) -> network (H, W): two downscales, a strong one, an upscale, and one where the edge clamps dominate
SIZE_PAIRS = [((500, 375), (299, 224)), ((281, 500), (224, 399)), ((1200, 1600), (224, 299)), ((37, 53), (128, 183)),
              ((5, 7), (128, 179))]


@pytest.mark.parametrize("src,net", SIZE_PAIRS)
def test_reference_against_interpolate(src, net):
    g = torch.Generator().manual_seed(src[0] + net[1])
    raw = torch.randint(0, 256, (*src, 3), generator=g, dtype=torch.uint8)
    inv_std = tuple(1.0 / s for s in STD)
    got = sfr.resize_normalise(raw, net, MEAN, inv_std)
    x = F.interpolate(raw.double().permute(2, 0, 1)[None], size=net, mode="bilinear", align_corners=False)[0]
    want = (x - torch.tensor(MEAN, dtype=torch.float64)[:, None, None]) * torch.tensor(inv_std, dtype=torch.float64)[:, None, None]
    err = float((got - want).abs().max())
    print(f"{src} -> {net}: largest difference to F.interpolate in fp64 {err:.3e}")
    assert got.shape == (3, *net) and err <= 1e-9
    flipped = sfr.resize_normalise(raw.flip(2), net, MEAN, inv_std, reverse_channels=True)
    assert torch.equal(flipped, got)


@pytest.mark.parametrize("hw,expect", [((300, 300), (224, 224)), ((500, 375), (299, 224)), ((375, 500), (224, 299)),
                                       ((281, 500), (224, 399))])
def test_net_size(hw, expect):
    from segclip_amd.segmentation import ImageTransform
    tf = ImageTransform()
    assert tf.net_size(*hw) == expect
    assert tf.mean == MEAN and tf.std == STD
    assert tf.inv_std == tuple(float(torch.tensor(1.0 / s, dtype=torch.float64).float()) for s in STD)
    assert ImageTransform(img_scale=(512, 128)).net_size(300, 300) == (128, 128)
    with pytest.raises(ValueError, match="channel_order"):
        ImageTransform(channel_order="gbr")


def test_predict_raw_has_no_cpu_fallback():
    """A CPU image is refused before anything is planned or launched (no model or library is needed to see it)."""
    from segclip_amd.segmentation import ImageTransform, SegInference, preprocess
    seg = SegInference.__new__(SegInference)
    seg.model = torch.nn.Identity().eval()
    raw = torch.zeros(300, 300, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg.predict_raw([raw], ImageTransform())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        preprocess([raw], ImageTransform())
