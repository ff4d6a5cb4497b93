"""The fixture scene of the chained guide pass: a "mirror room" that exercises every class of the chain -- planar mirrors that
face each other (link counts up to the limit), a solid glass box (entry, exit, total internal reflection), a thin-walled pane, a rough metal sphere that
is never followed, checker-textured diffuse surfaces to be seen in the mirrors, and sky above the walls.  tests/test_chain_host.py asserts the census.
A plain module: no test lives here."""
import numpy as np

from vk_raytrace_amd import capi, host_device as hd, synth
from vk_raytrace_amd.scene import Camera, Scene, rotate_y, translate

MIRROR_X = 2.0                       # the two mirrors lie in the planes x = -MIRROR_X (facing +x) and x = +MIRROR_X (facing -x)
MIRROR_TINT = (0.9, 0.8, 0.7)
STRAFE = 0.2                         # camera B of the reprojection measurement: camera A moved this far along its right vector


def checker(size=16, hi=(0.9, 0.9, 0.85), lo=(0.15, 0.2, 0.3)):
    """an RGBA8 image whose texels alternate between two colours: one checker cell per texel"""
    yy, xx = np.mgrid[0:size, 0:size]
    rgb = np.where(((xx + yy) % 2 == 0)[..., None], np.asarray(hi), np.asarray(lo))
    return (np.concatenate([rgb, np.ones((size, size, 1))], -1) * 255.0 + 0.5).astype(np.uint8)


def mirror_room(eye=(1.2, 1.1, 2.2), center=(-2.0, 1.0, 1.2)):
    sc = Scene("mirror_room")
    t_floor = sc.add_texture(checker(16), magFilter=hd.FILTER_NEAREST)
    t_wall = sc.add_texture(checker(16, (0.85, 0.5, 0.3), (0.2, 0.25, 0.6)), magFilter=hd.FILTER_NEAREST)
    m_floor = sc.add_material(pbrBaseColorTexture=t_floor, pbrMetallicFactor=0.0, pbrRoughnessFactor=0.9)
    m_wall = sc.add_material(pbrBaseColorTexture=t_wall, pbrMetallicFactor=0.0, pbrRoughnessFactor=0.9)
    m_mirror = sc.add_material(pbrBaseColorFactor=MIRROR_TINT + (1.0,), pbrMetallicFactor=1.0, pbrRoughnessFactor=0.0)
    m_glass = sc.add_material(pbrBaseColorFactor=(0.95, 1.0, 0.95, 1.0), pbrMetallicFactor=0.0, pbrRoughnessFactor=0.0, transmissionFactor=1.0, ior=1.5,
                              thicknessFactor=1.0, doubleSided=1)
    m_pane = sc.add_material(pbrBaseColorFactor=(0.8, 0.9, 1.0, 1.0), pbrMetallicFactor=0.0, pbrRoughnessFactor=0.0, transmissionFactor=1.0, thicknessFactor=0.0,
                             doubleSided=1)
    m_rough = sc.add_material(pbrBaseColorFactor=(0.95, 0.8, 0.4, 1.0), pbrMetallicFactor=1.0, pbrRoughnessFactor=0.6)
    x = MIRROR_X
    synth._add(sc, synth.grid(4, 6, (-x, 0, 3), (2 * x, 0, 0), (0, 0, -6)), m_floor)                       # floor, y = 0, normal +y
    synth._add(sc, synth.grid(4, 2, (-x, 0, -3), (2 * x, 0, 0), (0, 2.0, 0)), m_wall)                      # back wall, z = -3, normal +z; sky above it
    synth._add(sc, synth.grid(1, 1, (-x, 0.05, 3), (0, 0, -6), (0, 2.2, 0)), m_mirror)                     # mirror in x = -2, normal +x
    synth._add(sc, synth.grid(1, 1, (x, 0.05, -3), (0, 0, 6), (0, 2.2, 0)), m_mirror)                      # the mirror facing it, normal -x
    synth._add(sc, synth.box((0.6, 0.6, 0.6)), m_glass, translate(-0.7, 0.31, 0.9) @ rotate_y(0.4))        # solid glass
    synth._add(sc, synth.grid(1, 1, (-1.4, 0.0, -1.8), (1.6, 0, 0), (0, 1.5, 0)), m_pane)                  # thin-walled pane in front of the back wall
    synth._add(sc, synth.uv_sphere(0.35, 24, 12), m_rough, translate(0.9, 0.35, -0.6))                     # rough metal: never followed
    sc.camera = Camera(eye=eye, center=center, up=(0, 1, 0), fov=60.0)
    sc.finalize(capi.pack_vertices)
    return sc


def strafed(scene_camera, by=STRAFE):
    """(eye, center) of the camera moved `by` along its right vector"""
    eye, center, up = (np.asarray(v, np.float64) for v in (scene_camera.eye, scene_camera.center, scene_camera.up))
    fwd = center - eye
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    return tuple(eye + by * right), tuple(center + by * right)


def matte_room():
    """a diffuse floor, a back wall and two boxes under the sky: nothing the chain follows, hits and misses"""
    sc = Scene("chain_matte")
    mats = [sc.add_material(pbrBaseColorFactor=c + (1,), pbrMetallicFactor=0.0, pbrRoughnessFactor=1.0) for c in ((0.7, 0.7, 0.7), (0.8, 0.25, 0.2), (0.2, 0.6, 0.3))]
    synth._add(sc, synth.grid(4, 4, (-3, 0, 3), (6, 0, 0), (0, 0, -6)), mats[0])
    synth._add(sc, synth.grid(4, 3, (-3, 0, -2), (6, 0, 0), (0, 1.5, 0)), mats[0])
    synth._add(sc, synth.box((0.8, 1.2, 0.8)), mats[1], translate(-1.0, 0.6, -0.6) @ rotate_y(0.5))
    synth._add(sc, synth.box((0.9, 0.7, 0.9)), mats[2], translate(0.4, 0.35, 0.2) @ rotate_y(-0.3))
    sc.camera = Camera(eye=(0.0, 1.6, 3.4), center=(0.0, 0.9, -0.5), up=(0, 1, 0), fov=50.0)
    sc.finalize(capi.pack_vertices)
    return sc


def followable_by_factors(scene, p):
    """True when some material of the scene can be followed under the chain parameters p, judged from the material factors alone (a texture can only
    lower roughness, metallic and transmission: a material with a metallic-roughness texture counts as followable when its factors allow it at all)"""
    for m in scene.materials:
        rough = float(m["pbrRoughnessFactor"])
        if int(m["pbrMetallicRoughnessTexture"]) > -1:
            rough = 0.0
        if int(m["unlit"]) == 1 or max(rough, 0.001) > p.maxRoughness:
            continue
        if float(m["pbrMetallicFactor"]) >= p.minMetallic or float(m["transmissionFactor"]) >= p.minTransmission:
            return True
    return False
