"""fp64 yardstick of the segmentation front end (segclip_seg_windows_from_u8, include/segclip_hip.h): the bilinear resize of
a decoded uint8 image to its network size with cv2 INTER_LINEAR's geometry, the normalisation, and the windows cut out of it.
Restated from the definition: the source coordinate of destination d along an axis of n source and m destination pixels is
the rational ((2 d + 1) n - m) / (2 m), split in integers; nothing here calls an interpolation routine."""
import torch


def axis_taps(n, m):
    """-> (s0, s1 int64 (m), f fp64 (m)): the two taps of every destination pixel and the weight of the second."""
    d = torch.arange(m, dtype=torch.int64)
    num, den = (2 * d + 1) * n - m, 2 * m
    s0 = torch.div(num, den, rounding_mode="floor")
    f = (num - s0 * den).double() / float(den)
    low, high = s0 < 0, s0 >= n - 1
    s0 = s0.clamp(0, n - 1)
    f = torch.where(low | high, torch.zeros_like(f), f)
    return s0, (s0 + 1).clamp(max=n - 1), f


def resize_normalise(raw, net, mean, inv_std, reverse_channels=False):
    """raw (h, w, 3) uint8, net = (H, W) -> (3, H, W) fp64: (r - mean[c]) * inv_std[c], channel c read from source channel
    2 - c with reverse_channels."""
    h, w, _ = raw.shape
    H, W = net
    v = raw.double().permute(2, 0, 1)
    if reverse_channels:
        v = v.flip(0)
    ya, yb, fy = axis_taps(h, H)
    xa, xb, fx = axis_taps(w, W)
    fy, fx = fy[None, :, None], fx[None, None, :]
    top = v[:, ya][:, :, xa] * (1 - fx) + v[:, ya][:, :, xb] * fx
    bot = v[:, yb][:, :, xa] * (1 - fx) + v[:, yb][:, :, xb] * fx
    r = top * (1 - fy) + bot * fy
    mean = torch.tensor(mean, dtype=torch.float64)[:, None, None]
    inv_std = torch.tensor(inv_std, dtype=torch.float64)[:, None, None]
    return (r - mean) * inv_std


def windows(images, wins, win):
    """images [(3, H_i, W_i)], wins [(image, y0, x0)] -> (n, 3, win_h, win_w)."""
    wh, ww = win
    return torch.stack([images[i][:, y:y + wh, x:x + ww] for (i, y, x) in wins])
