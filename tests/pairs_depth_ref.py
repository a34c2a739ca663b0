"""numpy restatement of the depth formats of mbavo_pairs_opts.depth_format / mbavo_depth_to_z, as include/mbavo.h defines them:
float64 arithmetic in the order written there, then np.float32.  numpy's float64 division and square root are IEEE (correctly
rounded), and nothing here can be contracted into a fused multiply-add.  tests/test_pairs_depth_api.py pins the edge cases on the
CPU; tests/test_gpu_pairs_depth.py holds the device to these functions bit for bit."""
import numpy as np

UNREAL = dict(depth_format=1, depth_unit=0.0, depth_max=100.0)   # Utils::load_depthMap + Utils::convert_ray_d_to_z
ETH3D = dict(depth_format=2, depth_unit=5000.0, depth_max=0.0)   # a 16-bit image / 5000


def ray_to_z(d, intr, depth_max=0.0):
    """Format 1: H x W float32 distances along the viewing ray -> float32 z.  intr: level-0 (fx, fy, cx, cy)."""
    d = np.asarray(d)
    assert d.dtype == np.float32 and d.ndim == 2
    H, W = d.shape
    fx, fy, cx, cy = (np.float64(v) for v in intr)
    if np.float32(depth_max) > 0:
        d = np.where(d > np.float32(depth_max), np.float32(0), d)
    xn = (np.arange(W, dtype=np.float64) - cx) / fx
    yn = (np.arange(H, dtype=np.float64) - cy) / fy
    n = np.sqrt(((xn * xn)[None, :] + (yn * yn)[:, None]) + 1.0)  # summed left to right
    return (d.astype(np.float64) * (1.0 / n)).astype(np.float32)


def u16_to_z(v, depth_unit):
    """Format 2: H x W uint16 -> float32 z = value / depth_unit (the unit is a C float)."""
    v = np.asarray(v)
    assert v.dtype == np.uint16 and np.float32(depth_unit) > 0
    return (v.astype(np.float64) / np.float64(np.float32(depth_unit))).astype(np.float32)


def to_z(depth_format, depth, intr, depth_unit=0.0, depth_max=0.0):
    """One map, or a stack of them, in any format -> float32 z."""
    depth = np.asarray(depth)
    if depth.ndim == 3:
        return np.stack([to_z(depth_format, m, intr, depth_unit, depth_max) for m in depth])
    if depth_format == 0:
        assert depth.dtype == np.float32
        return depth.copy()
    return ray_to_z(depth, intr, depth_max) if depth_format == 1 else u16_to_z(depth, depth_unit)


def has_depth(z):
    """The detector's test on a float32 z (blur_aware_direct_tracker.cpp:401): not ((double)z < 1e-2)."""
    z = np.asarray(z)
    assert z.dtype == np.float32
    return ~(z.astype(np.float64) < 1e-2)
