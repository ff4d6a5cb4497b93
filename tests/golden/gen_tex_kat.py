"""Mints tests/golden/tex_kat.npz: the software texture path held to an INDEPENDENT model.

The HIP code (vk_raytrace_amd/csrc/pt_surface.h), the CPU oracle (oracle/orc_scene.h) and the compiled reference (its texel filtering
is the oracle's, through hooks) share one implementation of SURVEY.md Appendix F4 / F6.  This file is the leg that shares nothing with them: numpy only,
written from Appendix F4 / F6 and the Vulkan texel-coordinate rules ("Texel Coordinate Systems", "Texel Filtering", "Wrapping Operation"), in
float64 and exact integers.

The model, per axis (W texels, float32 coordinate u, LOD 0):
  unnormalised coordinate   x = u W - 0.5   (NEAREST: x = u W)                                    F4; Vulkan "(u,v,w) = (s,t,r) x size", "shifted by 0.5"
  base texel and fraction   i = floor(x), a = x - i                                              F4 floor / frac
  REPEAT                    i mod W                                                              Vulkan wrapping operation
  MIRRORED_REPEAT           (W - 1) - mirror((i mod 2W) - W),  mirror(m) = m >= 0 ? m : -(1 + m)
  CLAMP_TO_EDGE             clamp(i, 0, W - 1)
  LINEAR                    texels (i, j) (i+1, j) (i, j+1) (i+1, j+1) with weights (1-a)(1-b), a(1-b), (1-a)b, ab on the 0..255 values, scaled by 1/255
  NEAREST                   texel (i, j), byte / 255
  environment (F6)          RGBA32F texels, LINEAR, U repeat, V clamp to edge
float32 x integer (W < 2^16) is exact in float64, and so are the subtraction of 0.5, the floor and the fraction: the model has NO rounding of its own
in the footprint and the weights for |x| < 2^29; the weighted sum is rounded at 2^-53.

The bound the float32 implementations are held to (tests/test_texture_model.py), derived, not measured:
  LINEAR    |got - model| <= (|u W| + |v H| + 4) 2^-23 on the 0..1 scale (environment: times the largest |texel| of the footprint).
            The float32 product u W is off by at most |u W| 2^-24, the subtraction of 0.5 by at most as much again: the coordinate moves by at most
            |x| 2^-23.  A weight moves by the same amount, and it blends values at most 1 apart (0..1 scale), so the result moves by at most
            |u W| 2^-23 per axis.  Bilinear filtering is CONTINUOUS across texel edges (at a = 0 the footprint (i-1, i) with a = 1 gives the same
            value), so this holds even where float32 floors to the neighbouring texel.  The filter itself -- 1 - a, three lerps of two products
            and a sum each, the scale by 1/255 -- adds fewer than four more ulps of a value <= 1.
  NEAREST   on KEPT rows the byte is named exactly: |got - byte / 255| <= 2^-23 (division against multiplication by the rounded 1/255).  A row is
            kept when, on both axes, the distance of u W to the nearest integer exceeds |u W| 2^-23 or u W is exactly representable in float32
            (then float32 computes it exactly).  The model alone decides.  On rows not kept the answer must be one of the model's two adjacent
            texels per axis (stored as the alternative footprint) -- as long as float32 resolves single texels, |u W| 2^-23 < 1/2.  Beyond that
            (the rows up to 1e5 on the 1024-wide image, the rows near 2^30) no float32 evaluation of u W can name a texel or its neighbour, and
            the row allows every texel within ceil(|u W| 2^-23) of the model's on that axis (`far`, see axis()).

What the fixture stores: inputs (texture bytes, environment texels, per row texture / wrap pair / filter / u / v) and the model's exact outputs per
row -- the wrapped footprint (two columns, two rows), the weights a and b, the kept mask, the alternative texel of a NEAREST row.  The weighted sums
are random bytes blended with arbitrary weights: 58 k rows of four float64 do not fit the 1 MiB a committed file may have.  `want_rgba` / `want_env`
below finish the model's value from the stored footprint and weights (the test imports this file for it); every WANT_STRIDE-th row is stored in full
and the test checks the two against each other bit for bit.

Run:  python tests/golden/gen_tex_kat.py   (rewrites tex_kat.npz; deterministic, byte-identical on every run)
"""
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_kat import tea  # noqa: E402

REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE = 0, 1, 2   # include/pt_types.h
NEAREST, LINEAR = 0, 1
SIZES = [(1, 1), (2, 2), (1, 9), (9, 1), (3, 5), (7, 5), (8, 4), (12, 20), (16, 16), (24, 12), (7, 64), (64, 7), (40, 4), (255, 3), (1024, 8)]   # (W, H)
ENV_SIZES = [(8, 4), (5, 3), (1, 2), (16, 1)]
CONFIGS = 18   # config = (wrapS * 3 + wrapT) * 2 + filter
WANT_STRIDE = 16
EPS = 2.0 ** -23


def words(n, salt):
    """n deterministic 32-bit words (shaders/random.glsl tea, from gen_kat: no dependence on numpy's generators)"""
    return tea(np.arange(n, dtype=np.uint64), np.full(n, salt, np.uint64))


def uniform(n, salt, lo, hi):
    return lo + (hi - lo) * (words(n, salt).astype(np.float64) / 2.0 ** 32)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------------
def mirror(m):
    return np.where(m >= 0, m, -(1 + m))


def wrap(i, n, mode):
    """integer texel coordinate -> [0, n): exact integers (int64 arrays or Python ints)"""
    i = np.asarray(i, np.int64)
    if mode == CLAMP_TO_EDGE:
        return np.clip(i, 0, n - 1)
    if mode == MIRRORED_REPEAT:
        return (n - 1) - mirror(np.mod(i, 2 * n) - n)
    return np.mod(i, n)   # (numpy's mod is the floored one: the result has the sign of n)


def wrap_modes(i, n, modes):
    out = np.zeros(len(i), np.int64)
    for mode in (REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE):
        m = modes == mode
        out[m] = wrap(i[m], n, mode)
    return out


def axis(u, n, modes, linear):
    """one axis of the tap: u float32, n texels, per-row wrap mode, per-row filter -> wrapped (i0, i1), weight a, and for NEAREST: kept, the alternative
    texel, and (unwrapped base texel, lo, hi): the float32 coordinate floors to base + d for some lo <= d <= hi"""
    x = u.astype(np.float64) * float(n)
    exact = x.astype(np.float32).astype(np.float64) == x
    near = np.rint(x)
    kept = (np.abs(x - near) > np.abs(x) * EPS) | exact | linear
    xs = np.where(linear, x - 0.5, x)
    i = np.floor(xs)
    a = np.where(linear, xs - i, 0.0)
    i = i.astype(np.int64)
    # NEAREST, not kept: float32 rounds u n by at most |u n| 2^-24.  Below |u n| 2^-23 < 1/2 the row is within that of ONE texel edge and the answer is
    # the texel on either side of it.  Beyond, float32 no longer resolves single texels (from 2^23 on it holds integers only, 64 apart near 2^30): the
    # adjacency rule cannot hold for any float32 implementation of F4, and the row allows every texel within ceil(|u n| 2^-23) of the model's instead.
    fine = np.abs(x) * EPS < 0.5
    side = np.where(x - np.floor(x) < 0.5, -1, 1)
    reach = np.ceil(np.abs(x) * EPS).astype(np.int64)
    lo = np.where(kept, 0, np.where(fine, np.minimum(side, 0), -reach))
    hi = np.where(kept, 0, np.where(fine, np.maximum(side, 0), reach))
    i0 = wrap_modes(i, n, modes)
    i1 = np.where(linear, wrap_modes(i + 1, n, modes), i0)
    alt = np.where(kept | ~fine, i0, wrap_modes(i + side, n, modes))
    return i0, i1, a, kept, alt, (i, lo, hi, fine | kept)


def blend(t00, t10, t01, t11, a, b):
    """(1-a)(1-b), a(1-b), (1-a)b, ab"""
    a, b = a[:, None], b[:, None]
    return t00 * ((1 - a) * (1 - b)) + t10 * (a * (1 - b)) + t01 * ((1 - a) * b) + t11 * (a * b)


def want_rgba(kat, rows=None):
    """the model's RGBA on the 0..1 scale for the fixture's texture rows, float64"""
    rows = np.arange(len(kat["row_tex"])) if rows is None else np.asarray(rows)
    out = np.zeros((len(rows), 4))
    tex = kat["row_tex"][rows]
    for t, (w, h) in enumerate(kat["sizes"]):
        m = tex == t
        if not m.any():
            continue
        r = rows[m]
        img = kat[f"tex{t}"].astype(np.float64)   # (H, W, 4)
        x0, x1, y0, y1 = (kat[k][r].astype(np.int64) for k in ("row_x0", "row_x1", "row_y0", "row_y1"))
        out[m] = blend(img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1], kat["row_a"][r], kat["row_b"][r]) / 255.0
    return out


def want_env(kat, rows=None):
    """the model's RGB for the environment rows, and the largest |texel| of each footprint (the scale of the bound)"""
    rows = np.arange(len(kat["env_img"])) if rows is None else np.asarray(rows)
    out, scale = np.zeros((len(rows), 3)), np.zeros(len(rows))
    which = kat["env_img"][rows]
    for e in range(len(kat["env_sizes"])):
        m = which == e
        r = rows[m]
        img = kat[f"env{e}"].astype(np.float64)[:, :, :3]
        x0, x1, y0, y1 = (kat[k][r].astype(np.int64) for k in ("env_x0", "env_x1", "env_y0", "env_y1"))
        taps = [img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]]
        out[m] = blend(*taps, kat["env_a"][r], kat["env_b"][r])
        scale[m] = np.max([np.abs(t).max(1) for t in taps], 0)
    return out, scale


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------
def family(n, salt):
    """the coordinates of one axis of n texels, float32"""
    k = np.arange(-3 * n - 2, 3 * n + 3, dtype=np.float64)
    edges = np.stack([k / n, (k + 0.5) / n], 1).reshape(-1).astype(np.float32)   # every texel edge and every texel centre, three periods each way
    inf = np.float32(np.inf)
    edges = np.stack([np.nextafter(edges, -inf), edges, np.nextafter(edges, inf)], 1).reshape(-1)   # ... and the float32 neighbours on both sides
    special = np.array([0.0, -0.0, 1.0, -1.0, 1.0 - 2.0 ** -24, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126], np.float32)
    top = (2.0 ** 30 - 64.0 * np.arange(1, 5)) / n * (1 - 2.0 ** -22)   # a few just inside the domain |u n| < 2^30
    far = np.concatenate([uniform(16, salt + 1, -1e3, 1e3), uniform(16, salt + 2, -1e5, 1e5), top, -top]).astype(np.float32)
    u = np.concatenate([edges, special, uniform(64 + 4 * n, salt, -4.0, 4.0).astype(np.float32), far])
    assert (np.abs(u.astype(np.float64) * n) < 2.0 ** 30).all()
    return u


def rows_for(w, h, salt):
    """u from the family of W, v from the family of H, row by row: the two start in phase, so texel corners meet texel corners and centres meet centres;
    the shorter family goes on with random coordinates in [-4, 4] (a NEAREST row is kept only if both axes are)"""
    U, V = family(w, salt), family(h, salt + 7)
    n = max(len(U), len(V))
    u = np.concatenate([U, uniform(n - len(U), salt + 3, -4.0, 4.0).astype(np.float32)])
    v = np.concatenate([V, uniform(n - len(V), salt + 4, -4.0, 4.0).astype(np.float32)])
    j = np.arange(n)
    cfg = (j // 6 + j) % CONFIGS   # the families repeat with period 6 (edge / centre x three neighbours): step the wrap pair and filter against it
    return u, v, cfg


def main(path=None):
    out = {"sizes": np.array(SIZES, np.int32), "env_sizes": np.array(ENV_SIZES, np.int32), "WANT_STRIDE": np.int64(WANT_STRIDE)}
    cols = {k: [] for k in ("tex", "cfg", "u", "v", "x0", "x1", "y0", "y1", "a", "b", "kept", "ax", "ay")}
    far = []
    for t, (w, h) in enumerate(SIZES):
        out[f"tex{t}"] = words(w * h, 100 + t).view(np.uint8).reshape(h, w, 4)   # random RGBA bytes
        u, v, cfg = rows_for(w, h, 1000 + 20 * t)
        linear = (cfg % 2) == LINEAR
        x0, x1, a, kx, ax, fx = axis(u, w, cfg // 6, linear)
        y0, y1, b, ky, ay, fy = axis(v, h, (cfg // 2) % 3, linear)
        coarse = np.nonzero(~(fx[3] & fy[3]))[0]   # NEAREST rows on which float32 does not resolve single texels
        rows_before = sum(len(p) for p in cols["tex"])
        far.append(np.stack([coarse + rows_before, fx[0][coarse], fx[1][coarse], fx[2][coarse], fy[0][coarse], fy[1][coarse], fy[2][coarse]], 1))
        for k, val in zip(cols, (np.full(len(u), t), cfg, u, v, x0, x1, y0, y1, a, b, kx & ky, ax, ay)):
            cols[k].append(val)
    dtypes = dict(tex=np.uint8, cfg=np.uint8, u=np.float32, v=np.float32, a=np.float64, b=np.float64, kept=bool)
    for k, parts in cols.items():
        out["row_" + k] = np.concatenate(parts).astype(dtypes.get(k, np.int16))
    for t, (w, h) in enumerate(SIZES):   # every wrap pair and both filters on every texture; NEAREST keeps at least half of its rows
        m = out["row_tex"] == t
        assert len(set(out["row_cfg"][m])) == CONFIGS
        near = m & (out["row_cfg"] % 2 == NEAREST)
        assert out["row_kept"][near].mean() >= 0.5, (w, h, out["row_kept"][near].mean())
    out["far"] = np.concatenate(far).astype(np.int32)   # row, then per axis: unwrapped base texel, lowest and highest offset the float32 coordinate may floor to
    out["row_want"] = want_rgba(out, np.arange(0, len(out["row_tex"]), WANT_STRIDE))

    cols = {k: [] for k in ("img", "u", "v", "x0", "x1", "y0", "y1", "a", "b")}
    for e, (w, h) in enumerate(ENV_SIZES):
        img = uniform(w * h * 4, 300 + e, 0.0, 16.0).astype(np.float32).reshape(h, w, 4)
        img[0, 0, :3] = (1.0e4, 0.0, 3.0e3)   # a sun-like texel: the bound scales with the footprint
        out[f"env{e}"] = img
        u, v, _ = rows_for(w, h, 2000 + 20 * e)
        on = np.ones(len(u), bool)
        x0, x1, a = axis(u, w, np.full(len(u), REPEAT), on)[:3]          # F6: U repeat
        y0, y1, b = axis(v, h, np.full(len(u), CLAMP_TO_EDGE), on)[:3]   #     V clamp to edge
        for k, val in zip(cols, (np.full(len(u), e), u, v, x0, x1, y0, y1, a, b)):
            cols[k].append(val)
    dtypes = dict(img=np.uint8, u=np.float32, v=np.float32, a=np.float64, b=np.float64)
    for k, parts in cols.items():
        out["env_" + k] = np.concatenate(parts).astype(dtypes.get(k, np.int16))
    out["env_want"] = want_env(out, np.arange(0, len(out["env_img"]), WANT_STRIDE))[0]

    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tex_kat.npz")
    with zipfile.ZipFile(path, "w") as z:  # like np.savez_compressed, with a fixed timestamp: the same bytes on every run
        for k, v in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote", path, os.path.getsize(path), "bytes,", len(out["row_tex"]), "texture rows,", len(out["env_img"]), "environment rows")


if __name__ == "__main__":
    main()
