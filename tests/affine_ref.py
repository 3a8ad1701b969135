"""The random affine warp restated (tests only): `warp` is the kernel specification of include/ssd_gfx950.h `ssd_affine_warp_f32` in
numpy float32, every operation a separate float32 numpy operation (so nothing is fused and nothing is kept wider), under
np.errstate(all="ignore"); `map_boxes` is the host's box mapping in float64, written box by box; `matrix` is the closed form of
`Dataset.plan_affine` from six given draws."""
import math

import numpy as np

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
FILLER_U8 = (123, 116, 103)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
f32 = np.float32


def fill():
    """the normalised filler: ((float)u8 / 255.0f - mean) / std in float32, the vertical pass's expression"""
    return np.array([(f32(u) / f32(255.0) - f32(m)) / f32(s) for u, m, s in zip(FILLER_U8, MEAN, STD)], f32)


def warp_one(x, m, fl):
    """x: (3, H, W) float32; m: six float32 coefficients, output pixel centre -> input coordinates; fl: three float32"""
    x = np.asarray(x, f32)
    _, H, W = x.shape
    m = [f32(v) for v in m]
    half, one = f32(0.5), f32(1.0)
    with np.errstate(all="ignore"):
        fx = (np.arange(W, dtype=np.int32).astype(f32) + half)[None, :]
        fy = (np.arange(H, dtype=np.int32).astype(f32) + half)[:, None]
        a = m[0] * fx
        b = m[1] * fy
        sx = ((a + b) + m[2]) - half
        a = m[3] * fx
        b = m[4] * fy
        sy = ((a + b) + m[5]) - half
        assert sx.dtype == f32 and sy.dtype == f32 and sx.shape == (H, W) == sy.shape
        live = (sx > -one) & (sx < f32(W)) & (sy > -one) & (sy < f32(H))               # a NaN compares false
        sxl, syl = np.where(live, sx, f32(0)), np.where(live, sy, f32(0))              # nothing that is not live becomes an integer
        flx, fly = np.floor(sxl), np.floor(syl)
        ax, ay = sxl - flx, syl - fly
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        out = np.empty_like(x)
        for c in range(3):
            def tap(yy, xx):
                ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                return np.where(ok, x[c][np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], f32(fl[c])).astype(f32)
            v00, v01, v10, v11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
            d = v01 - v00
            top = v00 + d * ax
            d = v11 - v10
            bot = v10 + d * ax
            d = bot - top
            r = top + d * ay
            assert r.dtype == f32
            out[c] = np.where(live, r, f32(fl[c]))
    return out


def warp(x, mats, fl=None):
    """x: (B, 3, H, W) float32, mats: (B, 6) -> (B, 3, H, W) float32"""
    fl = fill() if fl is None else fl
    return np.stack([warp_one(xi, mi, fl) for xi, mi in zip(np.asarray(x, f32), np.asarray(mats, f32))])


def warp_f64(x, mats, fl=None):
    """An independent evaluation in float64: torch.nn.functional.grid_sample (bilinear, align_corners=False, zero padding) of x - fill
    at the coordinates the float32 coefficients give in float64, plus fill.  x: (B, 3, H, W) float32 -> float64."""
    import torch
    fl = fill() if fl is None else fl
    x = torch.from_numpy(np.asarray(x, f32)).double()
    B, _, H, W = x.shape
    m = torch.from_numpy(np.asarray(mats, f32)).double().view(B, 6, 1, 1)
    fx = (torch.arange(W, dtype=torch.float64) + 0.5).view(1, 1, W)
    fy = (torch.arange(H, dtype=torch.float64) + 0.5).view(1, H, 1)
    cx = m[:, 0] * fx + m[:, 1] * fy + m[:, 2]                                     # pixel-centre coordinates: index + 0.5
    cy = m[:, 3] * fx + m[:, 4] * fy + m[:, 5]
    grid = torch.stack([2.0 * cx / W - 1.0, 2.0 * cy / H - 1.0], dim=-1)           # align_corners=False: index i sits at (2i + 1) / n - 1
    f = torch.from_numpy(np.asarray(fl, f32)).double().view(1, 3, 1, 1)
    return (torch.nn.functional.grid_sample(x - f, grid, mode="bilinear", padding_mode="zeros", align_corners=False) + f).numpy()


def noise(B, H, W, seed):
    """normalised 8-bit noise, (B, 3, H, W) float32: what the resize's last pass makes of random bytes"""
    u8 = np.random.default_rng(seed).integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    mean, std = np.array(MEAN, f32).reshape(1, 3, 1, 1), np.array(STD, f32).reshape(1, 3, 1, 1)
    return ((u8.astype(f32) / f32(255.0) - mean) / std).astype(f32)


def drawn_mats(n, W, H, seed):
    """n coefficient sets drawn in the dataset's default ranges, (n, 6) float32"""
    import random
    rng = random.Random(seed)
    return np.asarray([matrix(W, H, *draw(W, H, rng))[1] for _ in range(n)], f32)


DISTANCE_SHAPES = ((13, 17), (64, 48), (300, 300))                                 # (H, W)
DISTANCE_FILE = "affine_ref_distance.json"


def distance(H, W, seed=0, n=4):
    """max |restatement - float64 evaluation| over n drawn matrices on noise of one shape"""
    x, mats = noise(n, H, W, 100 + seed), drawn_mats(n, W, H, 200 + seed)
    return float(np.abs(warp(x, mats).astype(np.float64) - warp_f64(x, mats)).max())


def matrix(W, H, angle, s, shx, shy, tx, ty):
    """six draws -> (forward M, top two rows as six float64; the six float32 coefficients of its inverse): the closed form"""
    c, sn = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    kx, ky = math.tan(math.radians(shx)), math.tan(math.radians(shy))
    a00, a01 = s * (c + kx * sn), s * (kx * c - sn)
    a10, a11 = s * (ky * c + sn), s * (c - ky * sn)
    m02 = tx - (a00 * (W / 2) + a01 * (H / 2))
    m12 = ty - (a10 * (W / 2) + a11 * (H / 2))
    det = a00 * a11 - a01 * a10
    i00, i01, i10, i11 = a11 / det, -a01 / det, -a10 / det, a00 / det
    inv = (i00, i01, -(i00 * m02 + i01 * m12), i10, i11, -(i10 * m02 + i11 * m12))
    return (a00, a01, m02, a10, a11, m12), tuple(float(f32(v)) for v in inv)


def matrix_by_products(W, H, angle, s, shx, shy, tx, ty):
    """the same map as 3 x 3 products, M = T(tx,ty) . Shear . sR . T(-W/2,-H/2), and numpy's inverse: (M, M^-1) float64"""
    c, sn = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    T = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)
    Sh = np.array([[1, math.tan(math.radians(shx)), 0], [math.tan(math.radians(shy)), 1, 0], [0, 0, 1]], np.float64)
    R = np.array([[s * c, -s * sn, 0], [s * sn, s * c, 0], [0, 0, 1]], np.float64)
    C = np.array([[1, 0, -W / 2], [0, 1, -H / 2], [0, 0, 1]], np.float64)
    M = T @ Sh @ R @ C
    return M, np.linalg.inv(M)


def draw(W, H, rng, degrees=10.0, scale=(0.8, 1.25), shear=2.0, translate=0.1):
    """the six draws in the dataset's order"""
    angle = rng.uniform(-degrees, degrees)
    s = rng.uniform(scale[0], scale[1])
    shx = rng.uniform(-shear, shear)
    shy = rng.uniform(-shear, shear)
    tx = rng.uniform(0.5 - translate, 0.5 + translate) * W
    ty = rng.uniform(0.5 - translate, 0.5 + translate) * H
    return angle, s, shx, shy, tx, ty


def map_boxes(M, boxes, W, H, min_box=2.0, min_visible=0.3):
    """standardised xyxy float32 boxes through the forward map M (six float64) -> (new boxes float32 (n, 4), keep list): pixels, four
    corners, hull, clip to the frame, the two rules; min_box None: the ignore regions' rule (whatever has area)"""
    m00, m01, m02, m10, m11, m12 = (float(v) for v in M)
    out, keep = [], []
    for bx in np.asarray(boxes, np.float32).reshape(-1, 4):
        x0, y0, x1, y1 = float(bx[0]) * W, float(bx[1]) * H, float(bx[2]) * W, float(bx[3]) * H
        px = [(m00 * x + m01 * y) + m02 for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))]
        py = [(m10 * x + m11 * y) + m12 for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))]
        hx0, hy0, hx1, hy1 = min(px), min(py), max(px), max(py)
        cx0, cx1 = min(max(hx0, 0.0), float(W)), min(max(hx1, 0.0), float(W))
        cy0, cy1 = min(max(hy0, 0.0), float(H)), min(max(hy1, 0.0), float(H))
        cw, ch = cx1 - cx0, cy1 - cy0
        k = cw > 0 and ch > 0
        if min_box is not None:
            k = k and cw >= min_box and ch >= min_box and cw * ch >= min_visible * ((hx1 - hx0) * (hy1 - hy0))
        out.append([cx0 / W, cy0 / H, cx1 / W, cy1 / H])
        keep.append(bool(k))
    return np.asarray(out, np.float64).reshape(-1, 4).astype(np.float32), keep


if __name__ == "__main__":                                                         # records the golden distances: python tests/affine_ref.py
    import json
    import os
    rec = {f"{H}x{W}": distance(H, W) for H, W in DISTANCE_SHAPES}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", DISTANCE_FILE), "w") as f:
        json.dump({"what": "max |float32 restatement - float64 grid_sample| of tests/affine_ref.py distance(H, W), seed 0", "distance": rec}, f,
                  indent=1)
        f.write("\n")
    print(rec)
