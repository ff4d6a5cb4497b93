"""The fixture of the hand-over tests (tests/test_handover_host.py, tests/test_handover_gpu.py): a few hundred triangles built so that the
packet stage's pass A often cannot stand -- alpha cards stacked a few millimetres apart in front of an opaque wall (and two behind it), all
sharing one 8 x 8 NEAREST texture whose alpha channel holds exactly 0, exactly 255 and 128.  Under ALPHA_BLEND the opacity of a texel is then
exactly 0, exactly 1 or fractional.  The cards overlap in every box of the hierarchy, so a walk meets them in no particular order along the
ray: zero-opacity candidates are evaluated BEHIND the hit that is finally kept (the case pass B exists for).  One card lies twice in the same
plane with the texture flipped -- identical triangles, so the two candidates tie in t and the world index decides.  The card mesh is
instantiated many times (one instance rotated about the axis of view, one mirrored), the flipped card once: in the two-level form the former
is a bottom-level structure of its own, the latter part of the merged one."""
import numpy as np

from vk_raytrace_amd import host_device as hd, synth
from vk_raytrace_amd.scene import Scene, Camera, translate, scale, rotate_x, rotate_y, rotate_z

EYE = (0.0, 0.0, 6.0)


def alpha_texture(seed=7):
    rng = np.random.default_rng(seed)
    img = np.zeros((8, 8, 4), np.uint8)
    img[..., :3] = rng.integers(40, 255, (8, 8, 3))
    pick = rng.random((8, 8))
    img[..., 3] = np.where(pick < 0.72, 0, np.where(pick < 0.95, 255, 128))
    return img


def handover_scene():
    sc = Scene("handover")
    m_wall = sc.add_material(pbrBaseColorFactor=(0.7, 0.6, 0.5, 1.0), pbrMetallicFactor=0.0, pbrRoughnessFactor=0.8)
    tex = sc.add_texture(alpha_texture(), magFilter=hd.FILTER_NEAREST)
    m_card = sc.add_material(pbrBaseColorTexture=tex, alphaMode=hd.ALPHA_BLEND, doubleSided=1, pbrMetallicFactor=0.0, pbrRoughnessFactor=0.6)
    wall = synth.grid(4, 4, (-2.5, -2.5, 0.0), (5.0, 0.0, 0.0), (0.0, 5.0, 0.0))
    sc.add_node(sc.add_prim_mesh(wall[0], wall[1], wall[2], wall[3], m_wall, tangents=wall[4]))
    pos, nrm, uv, idx, tan = synth.grid(3, 3, (-1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0))
    card = sc.add_prim_mesh(pos, nrm, uv, idx, m_card, tangents=tan)
    flipped = sc.add_prim_mesh(pos, nrm, (1.0 - uv).astype(np.float32), idx, m_card, tangents=tan)
    # in front of the wall: a tight stack (the candidates behind a hit), the coincident pair, a rotated and a mirrored instance, loose ones nearer the eye
    for k, z in enumerate((0.500, 0.504, 0.508, 0.512, 0.516, 0.520, 0.524)):
        sc.add_node(card, translate(0.11 * (k % 3) - 0.1, 0.07 * (k % 4) - 0.1, z))
    # ... and a fan of cards tilted through one another: the boxes of their triangles start at about the same distance, the hits do not
    for k, a in enumerate((-0.24, -0.15, -0.07, 0.06, 0.13, 0.22)):
        sc.add_node(card, translate(0.05 * k - 0.1, 0.04 * k - 0.1, 0.36) @ (rotate_x(a) if k % 2 else rotate_y(a)))
    sc.add_node(card, translate(0.0, 0.0, 0.75))
    sc.add_node(flipped, translate(0.0, 0.0, 0.75))
    sc.add_node(card, translate(0.1, -0.05, 1.0) @ rotate_z(0.3))
    sc.add_node(card, translate(-0.05, 0.1, 1.25) @ scale(-1.0, 1.0, 1.0))
    sc.add_node(card, translate(0.3, 0.2, 2.0))
    # behind the wall: never the hit of a camera ray, but inside the boxes the walks visit
    sc.add_node(card, translate(0.0, 0.0, -0.25))
    sc.add_node(card, translate(0.2, 0.1, -0.5) @ rotate_z(-0.4))
    # the optical axis meets the image inside an 8 x 8 block, not on a block boundary: that block's rays disagree on the signs of their direction
    sc.camera = Camera(eye=EYE, center=(0.2, 0.13, 0.0), up=(0, 1, 0), fov=40.0)
    return sc
