"""The option-laden objects A - D of tests/pairs_oracle.py under a photometric calibration (helper, no test in it): each object's
calibration, the intake hook that makes pairs_oracle.host_levels the restatement of the calibrated object
(tests/pairs_photocal_ref.py: remap, pinhole) and the calibrated device object.  tests/test_pairs_photocal_options_inputs.py
asserts on the CPU what tests/test_gpu_pairs_photocal_options.py rests on.

The calibration of an object: one gamma table per camera (GAMMAS, a different gamma for each), ONE scale per object -- the ABI
takes one scale per call -- and one vignette per camera in the geometry the images arrive in (the raw geometry where the object
undistorts).  A vignette is a radial fall-off, 1 at the centre and CORNER + 0.05 g at the corners, and holds a DEAD_BLOCK below
v_min (0.03), a NaN, a 0 and a BRIGHT_BLOCK above 1 (1.25).  The blocks lie where every object's maps read them, off the margin.
Scale 0.8 saturates bytes of A and B (51 and 27 of their level-0 bytes are 255); under it the largest value of C is 245.6 and of
D 224.3, so their scale is raised until the restatement holds bytes at 255: 0.9 for C (15 bytes), 1.0 for D (17 bytes)."""
import numpy as np

import pairs_cameras_ref as cref
import pairs_oracle as po
import pairs_photocal_ref as pc

GAMMAS = (2.2, 1.8, 2.0)
SCALE = dict(A=0.8, B=0.8, C=0.9, D=1.0)
CORNER = 0.55
DEAD_BLOCK, BRIGHT_BLOCK = (5, 6), (4, 7)  # rows x columns
_CAL = {}


def cameras(name):
    """Number of calibrations the object takes: max(1, num_cameras)."""
    o = po.OBJECTS[name]
    return len(o["cams"]) if o["cam_of"] is not None else 1


def arriving_size(name):
    o = po.OBJECTS[name]
    return (o["cams"][0]["Hs"], o["cams"][0]["Ws"]) if o["undistort"] else (o["H"], o["W"])


def vignette(Hr, Wr, g):
    """Camera g's vignette, Hr x Wr float32."""
    V = pc.radial_vignette(Hr, Wr, CORNER + 0.05 * g)
    y, x = Hr // 4 + g, Wr // 4 + 2 * g
    V[y:y + DEAD_BLOCK[0], x:x + DEAD_BLOCK[1]] = 0.03
    V[y + 1, x + 2], V[y + 2, x + 3] = np.nan, 0.0
    y, x = Hr // 2 + 3 - g, Wr // 2 + 5 + g
    V[y:y + BRIGHT_BLOCK[0], x:x + BRIGHT_BLOCK[1]] = 1.25
    return V


def build(gammas, scale, V):
    """dict(n, G n x 256 float64, scale, V n x Hr x Wr float32, luts n x 256 float32, inv n x Hr x Wr float32) of one gamma and one
    vignette per camera."""
    G = np.stack([pc.gamma_G(gamma) for gamma in gammas])
    V = np.ascontiguousarray(V, dtype=np.float32)
    assert len(G) == len(V)
    return dict(n=len(G), G=G, scale=scale, V=V, luts=np.stack([pc.table(g, scale) for g in G]), inv=pc.inverse_vignette(V))


def calibration(name):
    """The object's calibration (a dict as `build` makes them), made once and left unchanged."""
    if name not in _CAL:
        n = cameras(name)
        Hr, Wr = arriving_size(name)
        _CAL[name] = build(GAMMAS[:n], SCALE[name], np.stack([vignette(Hr, Wr, g) for g in range(n)]))
    return _CAL[name]


def another(name):
    """A second calibration of the object, far from its own: other gammas, scale 0.6, the vignettes turned by half a turn."""
    cal = calibration(name)
    return build([1.5 + 0.2 * g for g in range(cal["n"])], 0.6, cal["V"][:, ::-1, ::-1])


def swapped(cal):
    """The calibration with the cameras' entries in reverse order (the wrong-camera control)."""
    return dict(cal, G=np.ascontiguousarray(cal["G"][::-1]), V=np.ascontiguousarray(cal["V"][::-1]), luts=np.ascontiguousarray(cal["luts"][::-1]),
                inv=np.ascontiguousarray(cal["inv"][::-1]))


def intake(cal, values=None):
    """The hook of pairs_oracle.host_levels under a calibration.  values: a list that receives (usable, v) of every image taken in,
    the doubles before the rounding to a byte."""
    def hook(pair, g, image, map_xy):
        lut, inv = cal["luts"][g], cal["inv"][g]
        if values is not None:
            values.append(pc.pinhole_values(image, lut, inv) if map_xy is None else pc.remap_values(image, map_xy, lut, inv))
        return pc.pinhole(image, lut, inv) if map_xy is None else pc.remap(image, map_xy, lut, inv)
    return hook


def host_levels(name, c=None, cal=None):
    """pairs_oracle.host_levels of the calibrated object."""
    return po.host_levels(name, c, intake=intake(calibration(name) if cal is None else cal))


def level0_images(name, c=None, hook=None):
    """Level 0 of every image of the object as an intake takes it: B keyframes, then B current frames."""
    o = po.OBJECTS[name]
    c = po.inputs(name) if c is None else c
    hook = po.plain_intake if hook is None else hook
    out = []
    for which in ("sharp", "blur"):
        for b in range(o["B"]):
            cam = po.camera_of(o, b)
            g = o["cam_of"][b] if o["cam_of"] is not None else 0
            out.append(hook(b, g, c[which][b], None if cam is None else cref.camera_map(cam, o["H"], o["W"])))
    return out


def set_photometric(pb, cal):
    """mbavo_pairs_set_photometric with a calibration of this file; the vignette's tensor is returned for the caller to hold."""
    import torch
    V = torch.from_numpy(cal["V"]).to("cuda:0")
    assert pb.set_photometric(cal["G"], V, scale=cal["scale"]) == 0
    return V


def make_calibrated(ctx, name, cal=None):
    """pairs_oracle.make_object with set_photometric after the camera and mask calls and before the prepare: (PairBatch, counts)."""
    cal = calibration(name) if cal is None else cal
    return po.make_object(ctx, name, before_prepare=lambda pb: set_photometric(pb, cal))
