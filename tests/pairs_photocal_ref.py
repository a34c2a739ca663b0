"""numpy restatement of the photometric calibration of include/mbavo.h (mbavo_photometric_table, mbavo_pairs_set_photometric,
mbavo_photometric_u8_batch): the table, the inverse vignette, the tap, the pinhole intake and the raw intake (helper, no test in
it).  float64 arithmetic in the order written there; numpy contracts nothing, its float32 and float64 divisions are IEEE, and a
product of two float32 values formed in float64 is exact.  The remap is tests/pairs_undistort_ref.py's with every tap replaced.
Also the synthetic sensor of the tests: a radial vignette and a gamma response."""
import numpy as np

import pairs_undistort_ref as uref

V_MIN = np.float32(0.0625)


def table(G=None, scale=1.0):
    """lut[i] = (float)(scale * (255.0 * (G[i] - G[0]) / (G[255] - G[0]))), 256 float32; None where the call rejects."""
    G = np.arange(256, dtype=np.float64) if G is None else np.asarray(G, np.float64)
    scale = np.float64(scale)
    if G.shape != (256,) or not np.isfinite(G).all() or not (scale > 0.0 and scale <= 1.0):
        return None
    if not G[255] > G[0] or (np.diff(G) < 0).any():
        return None
    return (scale * (np.float64(255.0) * (G - G[0]) / (G[255] - G[0]))).astype(np.float32)


def inverse_vignette(V, v_min=0.0):
    """inv = (V is finite && V >= v_min) ? 1.0f / V : 0.0f in float32 (v_min = 0: 0.0625)."""
    V = np.asarray(V, np.float32)
    v_min = V_MIN if v_min == 0 else np.float32(v_min)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):  # (a subnormal that passes a tiny v_min has the inverse inf)
        ok = np.isfinite(V) & (V >= v_min)
        return np.where(ok, np.float32(1.0) / np.where(ok, V, np.float32(1.0)), np.float32(0.0)).astype(np.float32)


def tap(lut, inv, raw):
    """t = (double)lut[raw] * (double)inv; inv None: 1."""
    t = lut[raw].astype(np.float64)
    return t if inv is None else t * inv.astype(np.float64)


def to_u8(v):
    """(unsigned char)(int)(fmin(v, 255.0) + 0.5)"""
    return (np.fmin(v, 255.0) + 0.5).astype(np.int64).astype(np.uint8)


def pinhole_values(raw, lut, inv=None):
    """The doubles the pinhole intake rounds to bytes: (usable, v), both H x W."""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint8 and lut.dtype == np.float32 and lut.shape == (256,) and (inv is None or (inv.dtype == np.float32 and inv.shape == raw.shape))
    with np.errstate(invalid="ignore"):
        return np.ones(raw.shape, bool), tap(lut, inv, raw)


def pinhole(raw, lut, inv=None):
    """The pinhole intake of an H x W uint8 image under (lut, inv H x W or None)."""
    return to_u8(pinhole_values(raw, lut, inv)[1])


def remap_values(raw, map_xy, lut, inv=None):
    """The doubles the raw intake rounds to bytes: (usable, v), both H x W; an entry that is not usable gives the byte 0."""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint8 and raw.ndim == 2 and map_xy.dtype == np.float32 and (inv is None or (inv.dtype == np.float32 and inv.shape == raw.shape))
    Hs, Ws = raw.shape
    ok, x0, y0, ax, ay = uref._taps(map_xy)

    def p(y, x):
        inside = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
        yc, xc = np.clip(y, 0, Hs - 1), np.clip(x, 0, Ws - 1)
        return np.where(inside, tap(lut, None if inv is None else inv[yc, xc], raw[yc, xc]), 0.0)

    with np.errstate(invalid="ignore"):
        return ok, (1.0 - ay) * ((1.0 - ax) * p(y0, x0) + ax * p(y0, x0 + 1)) + ay * ((1.0 - ax) * p(y0 + 1, x0) + ax * p(y0 + 1, x0 + 1))


def remap(raw, map_xy, lut, inv=None):
    """The raw intake: the Hs x Ws uint8 image through an H x W x 2 map, every dereferenced tap replaced by t at that raw pixel."""
    ok, v = remap_values(raw, map_xy, lut, inv)
    with np.errstate(invalid="ignore"):
        return np.where(ok, to_u8(v), 0).astype(np.uint8)


# ---- the synthetic sensor: raw = clip(rint(U(I * V)))

def radial_vignette(H, W, corner=0.5):
    """V = 1 - (1 - corner) r^2 / r_corner^2 about the image centre, float32: 1 at the centre, `corner` at the corners."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64) - (H - 1) / 2.0, np.arange(W, dtype=np.float64) - (W - 1) / 2.0, indexing="ij")
    r2 = (x * x + y * y) / (((H - 1) / 2.0) ** 2 + ((W - 1) / 2.0) ** 2)
    return (1.0 - (1.0 - corner) * r2).astype(np.float32)


def gamma_response(x, gamma=2.2):
    """U: irradiance 0 .. 255 to the encoded value 0 .. 255, 255 (x / 255)^(1 / gamma)."""
    return 255.0 * np.power(np.clip(x, 0.0, 255.0) / 255.0, 1.0 / gamma)


def gamma_G(gamma=2.2):
    """The matching inverse response as a pcalib.txt holds it: G[i] = 255 (i / 255)^gamma."""
    return 255.0 * np.power(np.arange(256, dtype=np.float64) / 255.0, gamma)


def sensor(I, V, gamma=2.2):
    """What the synthetic camera records of the irradiance image I (uint8 or float) under vignette V."""
    return np.clip(np.rint(gamma_response(np.asarray(I, np.float64) * V.astype(np.float64), gamma)), 0, 255).astype(np.uint8)
