"""torch-CPU restatement of ``tt_overlay_grid`` (N17), shared by tests/test_overlay_host.py (as a stand-in for the kernel under the
Python layers) and tests/test_hip_overlay.py (as what the kernel is compared against with ``torch.equal``).  Written from the rules
the header states: ``make_grid``'s layout, ``denormalize`` + ``(img * 255).type(torch.uint8)`` with the clamp, ``palette[idx mod P]``,
``draw_segmentation_masks``' blend in three rounded fp32 operations."""
import torch

PHOTO, LABELS = 0, 1


def colour(v, palette, lut=None):
    """v int64 [F, H, W] -> uint8 [F, 3, H, W].  ``lut`` [L] or [F, L]: a value outside [0, L) gives index 0."""
    Fr = v.shape[0]
    idx = v
    if lut is not None:
        lut = lut.long()
        L = lut.shape[-1]
        inside = (v >= 0) & (v < L)
        vv = v.clamp(0, L - 1)
        idx = lut[vv] if lut.dim() == 1 else torch.gather(lut, 1, vv.reshape(Fr, -1)).view_as(v)
        idx = torch.where(inside, idx, torch.zeros_like(idx))
    idx = torch.remainder(idx, palette.shape[0])          # the sign of the divisor: a true modulo
    return palette[idx].permute(0, 3, 1, 2).contiguous()


def base(frames, mean=None, std=None):
    """float32 [F, 3, H, W] -> uint8: three rounded fp32 operations, NaN -> 0, clamp to [0, 255] after truncation."""
    m = torch.tensor([0.0, 0.0, 0.0] if mean is None else list(mean), dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor([1.0, 1.0, 1.0] if std is None else list(std), dtype=torch.float32).view(1, 3, 1, 1)
    x = (frames * s + m) * 255
    x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    return x.trunc().clamp(0, 255).to(torch.uint8)


def blend(a, b, alpha):
    """uint8, uint8 -> uint8: ``a * (1 - alpha) + b * alpha`` as torch evaluates it on float32 tensors with a Python scalar (the scalar
    rounded to fp32 once, each operation rounded), then ``.to(torch.uint8)``."""
    w_a, w_b = torch.tensor(1.0 - alpha, dtype=torch.float32), torch.tensor(alpha, dtype=torch.float32)
    return (a.float() * w_a + b.float() * w_b).to(torch.uint8)


def overlay_grid(mode, labels_a, palette, frames=None, labels_b=None, size=None, ytab=None, xtab=None, lut=None, alpha=0.5, pad=2, mean=None,
                 std=None):
    """The signature of ``hip_ops.overlay_grid`` on CPU tensors."""
    palette = torch.as_tensor(palette).cpu()
    a = labels_a.cpu().long()
    b = None if labels_b is None else labels_b.cpu().long()
    if ytab is not None:
        iy, ix = torch.as_tensor(ytab).long(), torch.as_tensor(xtab).long()
        a = a[:, iy][:, :, ix]
        b = None if b is None else b[:, iy][:, :, ix]
    lut = None if lut is None else torch.as_tensor(lut).cpu()
    ca = colour(a, palette, lut)
    if mode == PHOTO:
        ph = base(frames.cpu(), mean, std)
        tiles = [ph, blend(ph, ca, alpha)]
    else:
        cb = colour(b, palette)                           # the ground truth is never mapped
        tiles = [cb, ca, blend(cb, ca, alpha)]
    Fr, _, H, W = tiles[0].shape
    if size is not None:
        assert (H, W) == tuple(size)
    n = len(tiles)
    out = torch.zeros((Fr, 3, H + 2 * pad, n * W + (n + 1) * pad), dtype=torch.uint8)
    for k, t in enumerate(tiles):
        out[:, :, pad:pad + H, k * (W + pad) + pad: k * (W + pad) + pad + W] = t
    return out
