"""References for the Pascal VOC reader (N22).  The oracle is Pillow itself - what the reference's torchvision transforms call - and a NumPy
restatement of the two ragged kernels that walks the descriptor table and the pool the front end builds (no bands: two passes over the
whole box, uint8 rounding after each), so that the table / pool layout is checked on the host without a GPU."""
import io

import numpy as np
from PIL import Image

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
(SRC, H, W, X0, Y0, BW, BH, FLIP, HK, HB, HKS, VK, VB, VKS, YT, XT) = range(16)

# the grid of the issue: (H, W) sources and target sizes
SOURCES = [(1, 1), (5, 7), (7, 5), (3, 4), (37, 53), (64, 48), (23, 23), (200, 3), (3, 200), (375, 500)]
TARGETS = [1, 4, 7, 16, 23, 33]
MASK_TARGETS = [1, 7, 9, 100]
BOX_CASE = ((37, 53), (3, 2, 20, 11), 16)    # (H, W), (x0, y0, w, h), S


def image(h: int, w: int, seed: int) -> np.ndarray:
    """A uint8 [h, w, 3] test image: noise over a gradient, so that both flat and busy neighbourhoods occur."""
    rng = np.random.default_rng(1000 * seed + 7 * h + w)
    ramp = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5) % 256)[..., None]
    return ((rng.integers(0, 256, (h, w, 3)) + ramp) // 2).astype(np.uint8)


def mask(h: int, w: int, seed: int) -> np.ndarray:
    """A uint8 [h, w] label map with labels 0 .. 21 and a row of 255 (VOC's void label)."""
    rng = np.random.default_rng(2000 * seed + 7 * h + w)
    m = rng.integers(0, 22, (h, w)).astype(np.uint8)
    m[h // 2] = 255
    return m


def pillow_resize(img: np.ndarray, size, box=None, flip=False) -> np.ndarray:
    """``Image.crop(box).resize((OW, OH), BILINEAR)`` (then a horizontal flip): uint8 [OH, OW, 3]."""
    OH, OW = (size, size) if isinstance(size, int) else size
    im = Image.fromarray(img, "RGB")
    if box is not None:
        x0, y0, w, h = box
        im = im.crop((x0, y0, x0 + w, y0 + h))
    out = np.array(im.resize((OW, OH), Image.BILINEAR))      # (a writable copy)
    return np.ascontiguousarray(out[:, ::-1]) if flip else out


def to_tensor_normalize(u8: np.ndarray) -> np.ndarray:
    """ToTensor + Normalize in fp32: float32 [3, OH, OW] of a uint8 [OH, OW, 3]."""
    v = u8.astype(np.float32) / np.float32(255)
    v = (v - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    return np.ascontiguousarray(v.transpose(2, 0, 1)).astype(np.float32)


def pillow_mask_resize(m: np.ndarray, size, box=None, flip=False) -> np.ndarray:
    """``Image.resize((R, R), NEAREST)`` of the mode-P image: uint8 [R, R]."""
    OH, OW = (size, size) if isinstance(size, int) else size
    im = Image.fromarray(m, "P")
    if box is not None:
        x0, y0, w, h = box
        im = im.crop((x0, y0, x0 + w, y0 + h))
    out = np.array(im.resize((OW, OH), Image.NEAREST))
    return np.ascontiguousarray(out[:, ::-1]) if flip else out


def _clip8(a):
    return np.clip(a >> 22, 0, 255).astype(np.uint8)


def numpy_resize_ragged(buf: np.ndarray, table: np.ndarray, pool: np.ndarray, OH: int, OW: int) -> np.ndarray:
    """The resize kernel restated: uint8 [n, OH, OW, 3] from the byte buffer, the table and the pool."""
    out = np.zeros((len(table), OH, OW, 3), np.uint8)
    for i, row in enumerate(table):
        h_img, w_img = int(row[H]), int(row[W])
        img = buf[row[SRC]:row[SRC] + h_img * w_img * 3].reshape(h_img, w_img, 3)
        box = img[row[Y0]:row[Y0] + row[BH], row[X0]:row[X0] + row[BW]].astype(np.int64)
        if row[BW] != OW:
            ks = int(row[HKS])
            kk = pool[row[HK]:row[HK] + OW * ks].reshape(OW, ks)
            bounds = pool[row[HB]:row[HB] + 2 * OW].reshape(OW, 2)
            tmp = np.zeros((box.shape[0], OW, 3), np.int64)
            for xx in range(OW):
                xmin, cnt = bounds[xx]
                tmp[:, xx] = (1 << 21) + np.tensordot(box[:, xmin:xmin + cnt], kk[xx, :cnt].astype(np.int64), axes=([1], [0]))
            box = _clip8(tmp).astype(np.int64)
        if row[BH] != OH:
            ks = int(row[VKS])
            kk = pool[row[VK]:row[VK] + OH * ks].reshape(OH, ks)
            bounds = pool[row[VB]:row[VB] + 2 * OH].reshape(OH, 2)
            res = np.zeros((OH, OW, 3), np.int64)
            for yy in range(OH):
                ymin, cnt = bounds[yy]
                res[yy] = (1 << 21) + np.tensordot(kk[yy, :cnt].astype(np.int64), box[ymin:ymin + cnt], axes=([0], [0]))
            o = _clip8(res)
        else:
            o = box.astype(np.uint8)
        out[i] = o[:, ::-1] if row[FLIP] else o
    return out


def numpy_gather_ragged(buf: np.ndarray, table: np.ndarray, pool: np.ndarray, OH: int, OW: int) -> np.ndarray:
    out = np.zeros((len(table), OH, OW), np.uint8)
    for i, row in enumerate(table):
        img = buf[row[SRC]:row[SRC] + row[H] * row[W]].reshape(int(row[H]), int(row[W]))
        out[i] = img[pool[row[YT]:row[YT] + OH]][:, pool[row[XT]:row[XT] + OW]]
    return out


def pack(arrays):
    """Arrays packed back to back with no padding: (uint8 buffer, byte offsets)."""
    offs, at = [], 0
    for a in arrays:
        offs.append(at)
        at += a.size
    return np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in arrays]), offs


def jpeg_bytes(img: np.ndarray, subsampling, progressive=False) -> bytes:
    f = io.BytesIO()
    Image.fromarray(img, "RGB").save(f, "JPEG", quality=90, subsampling=subsampling, progressive=progressive)
    return f.getvalue()


def voc_palette():
    pal = []
    for i in range(256):
        pal += [(i * 37) % 256, (i * 91) % 256, (i * 53) % 256]
    return pal


def make_voc_tree(root: str, sizes=((20, 30), (30, 20), (17, 25), (24, 24), (33, 19))):
    """A small VOC tree: ``images/``, ``SegmentationClass/``, ``SegmentationClassAug/``, ``sets/{val,trainaug}.txt``.  Five images of
    different sizes, 4:2:0 and 4:4:4, the third progressive (the device decoder does not take it); palette PNGs with a 255 border band.
    Returns the file names in split order."""
    import os

    for d in ("images", "SegmentationClass", "SegmentationClassAug", "sets"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    names = [f"2007_{k:06d}" for k in range(len(sizes))]
    for k, (name, (h, w)) in enumerate(zip(names, sizes)):
        with open(os.path.join(root, "images", name + ".jpg"), "wb") as f:
            f.write(jpeg_bytes(image(h, w, 50 + k), "4:2:0" if k % 2 == 0 else "4:4:4", progressive=(k == 2)))
        m = mask(h, w, 60 + k) % 5      # few classes, as a small head sees them
        m[:2] = m[-2:] = 255
        m[:, :2] = m[:, -2:] = 255
        im = Image.fromarray(m, "P")
        im.putpalette(voc_palette())
        for d in ("SegmentationClass", "SegmentationClassAug"):
            im.save(os.path.join(root, d, name + ".png"))
    for split in ("val", "trainaug"):
        with open(os.path.join(root, "sets", split + ".txt"), "w") as f:
            f.write("\n".join(names) + "\n")
    return names


def voc_reference(root: str, name: str, folder: str, S: int, R: int):
    """The reference's chain on one file: (float32 [3, S, S], float32 [1, R, R] = index / 255, uint8 [R, R] indices)."""
    import os

    im = Image.open(os.path.join(root, "images", name + ".jpg")).convert("RGB")
    x = to_tensor_normalize(np.asarray(im.resize((S, S), Image.BILINEAR)))
    m = Image.open(os.path.join(root, folder, name + ".png"))
    idx = np.asarray(m.resize((R, R), Image.NEAREST))
    return x, (idx.astype(np.float32) / np.float32(255))[None], idx
