"""The image side of the reference's data loader on the device (dataloaders/rawimage_util.py): RawImageExtractor's train and
test transforms and get_felzenszwalb_from_cache, for a batch of decoded uint8 images of mixed sizes.

  RawImageTransform(is_train=True)    RandomResizedCropCoord(size, scale=(0.5, 1.0), BICUBIC) -> ToTensor -> Normalize  (:45-50)
  RawImageTransform(is_train=False)   Resize(size, BICUBIC) -> CenterCrop(size) -> ToTensor -> Normalize               (:47-50)
  RawImageTransform.patch_labels      get_felzenszwalb_from_cache                                                      (:100-144)

The host draws the crops (a few Python floats per image) and computes the integer geometry; the pixels are produced by
segclip_train_images_from_u8 and segclip_train_patch_labels, one launch each, bit for bit what Pillow, torchvision and numpy
give on the CPU.  Not covered: image decoding, the paired_aug branch (ColorJitter, RandomGrayscale, GaussianBlur), and crops
more than 8 times the output side, which raise."""
import math
import random

import torch

from . import ops

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


class RawImageTransform:
    """rng: the random.Random that __call__ draws the crops from when it is given none (default: the `random` module, as in
    the reference)."""

    def __init__(self, size=224, is_train=False, mean=CLIP_MEAN, std=CLIP_STD, scale=(0.5, 1.0), ratio=(3. / 4., 4. / 3.),
                 patch_size=16, rng=None):
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("mean and std have one entry per channel")
        self.size, self.is_train, self.patch_size = int(size), bool(is_train), int(patch_size)
        if self.size < 1 or self.patch_size < 1 or self.size % self.patch_size != 0:
            raise ValueError(f"size is a positive multiple of patch_size, got {size} / {patch_size}")
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(v) for v in std)
        self.scale, self.ratio = tuple(scale), tuple(ratio)
        self.rng = rng
        self._lut = {}

    def value_table(self, device=None):
        """ToTensor then Normalize of every byte, (256, 3) fp32: the operations of torchvision in their order, by torch on the
        CPU, so the table is exact by construction.  With a device: its copy there, made once."""
        if "cpu" not in self._lut:
            m = torch.tensor(self.mean, dtype=torch.float32).view(1, 3)
            s = torch.tensor(self.std, dtype=torch.float32).view(1, 3)
            self._lut["cpu"] = ((torch.arange(256, dtype=torch.float32) / 255).view(-1, 1) - m) / s
        key = "cpu" if device is None else str(torch.device(device))
        if key not in self._lut:
            self._lut[key] = self._lut["cpu"].to(device).contiguous()
        return self._lut[key]

    def sample(self, h, w, rng):
        """RandomResizedCropCoord.get_params draw for draw (rawimage_util.py:303-345) and the coord of __call__ (:355-360):
        -> ((i, j, ch, cw), [x_ul, y_ul, x_lr, y_lr]); the coord is zeros for an image one pixel wide or high."""
        area = h * w
        box = None
        for _ in range(10):
            target_area = rng.uniform(*self.scale) * area
            log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
            aspect_ratio = math.exp(rng.uniform(*log_ratio))
            cw = int(round(math.sqrt(target_area * aspect_ratio)))
            ch = int(round(math.sqrt(target_area / aspect_ratio)))
            if 0 < cw <= w and 0 < ch <= h:
                i = rng.randint(0, h - ch)
                j = rng.randint(0, w - cw)
                box = (i, j, ch, cw)
                break
        if box is None:  # central crop
            in_ratio = float(w) / float(h)
            if in_ratio < min(self.ratio):
                cw = w
                ch = int(round(cw / min(self.ratio)))
            elif in_ratio > max(self.ratio):
                ch = h
                cw = int(round(ch * max(self.ratio)))
            else:
                cw, ch = w, h
            box = ((h - ch) // 2, (w - cw) // 2, ch, cw)
        return box, self.coord(box, h, w)

    @staticmethod
    def coord(box, h, w):
        i, j, ch, cw = box
        if w - 1 == 0 or h - 1 == 0:
            return [0., 0., 0., 0.]
        return [float(j) / (w - 1), float(i) / (h - 1), float(j + cw - 1) / (w - 1), float(i + ch - 1) / (h - 1)]

    def eval_geometry(self, h, w):
        """torchvision's Resize(size) then CenterCrop(size) -> (RW, RH, ox, oy): the whole image resized to RH x RW (the short
        side to size, the other to int(size * long / short); unchanged when the short side is size already) and the
        size x size window at (ox, oy) = int(round((R - size) / 2.0))."""
        s = self.size
        if w <= h:
            RW, RH = s, int(s * h / w)
        else:
            RW, RH = int(s * w / h), s
        return RW, RH, int(round((RW - s) / 2.0)), int(round((RH - s) / 2.0))

    def __call__(self, raws, rng=None, boxes=None):
        """raws: [(h, w, 3) uint8 device tensors] -> (image (B, 3, size, size) fp32 on the device, coord (B, 1, 4) float64 on
        the host).  With is_train the crops (i, j, ch, cw) are `boxes` when given, else drawn by sample() from rng; without,
        the centre window of the resized image and a coord of zeros (ComposeCoord, :204-205).  One launch."""
        if len(raws) == 0:
            raise ValueError("empty image list")
        s = self.size
        geometry, coords = [], []
        if self.is_train:
            if boxes is None:
                rng = rng or self.rng or random
                boxes = []
                for t in raws:
                    box, _ = self.sample(int(t.shape[0]), int(t.shape[1]), rng)
                    boxes.append(box)
            elif len(boxes) != len(raws):
                raise ValueError(f"{len(raws)} images but {len(boxes)} boxes")
            for t, (i, j, ch, cw) in zip(raws, boxes):
                geometry.append((j, i, cw, ch, s, s, 0, 0, 0))
                coords.append(self.coord((i, j, ch, cw), int(t.shape[0]), int(t.shape[1])))
        else:
            if boxes is not None:
                raise ValueError("boxes belong to the train transform")
            for t in raws:
                h, w = int(t.shape[0]), int(t.shape[1])
                if min(h, w) < 1:
                    raise ValueError(f"an empty image: {tuple(t.shape)}")
                RW, RH, ox, oy = self.eval_geometry(h, w)
                geometry.append((0, 0, w, h, RW, RH, ox, oy, 0))
                coords.append([0., 0., 0., 0.])
        table = ops.train_source_table(raws, geometry, (s, s))
        image = ops.train_images_from_u8(raws, geometry, (s, s), self.value_table(raws[0].device), table=table)
        return image, torch.tensor(coords, dtype=torch.float64).view(-1, 1, 4)

    def label_box(self, coord, h, w):
        """The crop of get_felzenszwalb_from_cache (:108-120) for one coord row, which the reference holds as a float32
        tensor: swapped corners mean a flip -> (x0, y0, x1, y1, flags)."""
        xu, yu, xl, yl = torch.as_tensor(coord, dtype=torch.float64).reshape(4).float().tolist()
        flags = 0
        if xu > xl:
            xu, xl, flags = xl, xu, flags | 1
        if yu > yl:
            yu, yl, flags = yl, yu, flags | 2
        return int(xu * w), int(yu * h), math.ceil(xl * w), math.ceil(yl * h), flags

    def patch_labels(self, seg_maps, coord):
        """seg_maps: [(h, w) int32 device tensors], coord: (B, 1, 4) or (B, 4) as __call__ returns it -> the (B, 1, P, P)
        int64 label grid of the model's image_seg.  One launch."""
        coord = torch.as_tensor(coord).reshape(-1, 4).cpu()
        if coord.shape[0] != len(seg_maps):
            raise ValueError(f"{len(seg_maps)} segment maps but {coord.shape[0]} coord rows")
        boxes = [self.label_box(c, int(m.shape[0]), int(m.shape[1])) for m, c in zip(seg_maps, coord)]
        return ops.train_patch_labels(seg_maps, boxes, self.size, self.patch_size)
