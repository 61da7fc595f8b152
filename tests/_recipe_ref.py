"""Host restatements for the training-recipe tests (include/rcn_hipx.h, rcn_hipx_augment): the draw with Python integers masked to
64 bits, and the augmented batch as np.pad + slice + reverse on the STORED values.  Nothing here calls the library."""
import numpy as np

M64 = (1 << 64) - 1


def draw_ref(seed, epoch, pad, hflip, q):
    z = (seed ^ ((epoch * 0xD1342543DE82EF95) & M64)) & M64
    z = (z + (q + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    dy = (((z & 0xffff) * (2 * pad + 1)) >> 16) - pad
    dx = ((((z >> 16) & 0xffff) * (2 * pad + 1)) >> 16) - pad
    return dy, dx, ((z >> 32) & 1) if hflip else 0


def augment_ref(rows, pad, hflip, seed, epoch, q0):
    """rows: [B, H, W, C] stored values (uint8 or float32), already gathered.  Row r is padded with `pad` zeros on every side, cropped at
    offset (pad + dy, pad + dx) and mirrored if it draws a flip (torchvision: RandomCrop(padding=pad), then RandomHorizontalFlip) --
    out[h][w] = S(h + dy, (flip ? W-1-w : w) + dx), the stored value 0 outside the image.  Still in the stored dtype."""
    B, H, W, _ = rows.shape
    out = np.empty_like(rows)
    for r in range(B):
        dy, dx, flip = draw_ref(seed, epoch, pad, hflip, q0 + r)
        padded = np.pad(rows[r], ((pad, pad), (pad, pad), (0, 0)))
        crop = padded[pad + dy:pad + dy + H, pad + dx:pad + dx + W]
        out[r] = crop[:, ::-1] if flip else crop
    return out
