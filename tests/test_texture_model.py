"""The software texture path held to an INDEPENDENT model: address modes, texel footprint, bilinear weights, the environment lookup, the storage
orders of the texel pool and the device's own index arithmetic.

Every other check reaches the sampler through whole frames, and the three legs of "HIP == oracle == reference" share ONE implementation of SURVEY.md
Appendix F4 / F6: the compiled reference takes its texel filtering from the oracle's hooks (oracle/ref_glue/ref_driver.h), so for textures the
reference leg is the oracle and adds nothing -- it is not run here.  tests/golden/gen_tex_kat.py is the leg that shares nothing with them (numpy, float64
and exact integers, written from Appendix F and the Vulkan texel-coordinate rules; the derivation of the bounds is in its docstring).  Here the sampler
is called ON ITS OWN through

    orc_sample_texture / orc_hook_sample_env / orc_wrap_coord (oracle)      th_texture_probe (the product's headers, host build, the product's own
    pt_debug_texture_probe (the same function on the device, one row per lane)                 records / material lines / pool of a loaded scene)

Probe kinds (vk_raytrace_amd/csrc/pt_probe.h texture_probe): TAP (tex_tap: indices and weights, no loads), SAMPLE_REC (sample_rgba8_rec),
SAMPLE_DESC (tex_desc_unpack of a material-line descriptor, tex_tap, four loads, tex_filter -- the lines of resolve_material), ENV (sample_env), WRAP
(wrap_index), INDEX (tex_index), DESC (tex_desc_unpack(tex_desc_pack(r))), OPACITY (opacity_eval<false> and <true> side by side).

Held to the model, on every in-domain row (|u W|, |v H| < 2^30) of the fixture -- 15 image sizes x 9 wrap pairs x 2 filters, every texel edge and
centre three periods each way with its float32 neighbours, signed zeros, denormals, magnitudes up to 2^30 / W:
  LINEAR   within (|u W| + |v H| + 4) 2^-23 (environment: x the largest |texel| of the footprint)
  NEAREST  the model's texel on kept rows (within 2^-23 of byte / 255), one of the model's two adjacent texels per axis on the others; >= 50 % of
           every texture's NEAREST rows are kept
and oracle == host build == device, bit for bit, on every row.  Outside the domain (NaN, Inf, 3e38, 2^31, 2^33) float -> int conversion is undefined
in C++: only TAP runs there and only "every index is inside the pool" is asserted (numerical contract).

Measured worst error / bound on the LINEAR rows: oracle 0.444, host build (SAMPLE_REC and SAMPLE_DESC) 0.444 -- the same bits -- over 32 025 rows;
environment 0.447 over 1808 rows (a float32 numpy emulation on 1.13 M rows reached 0.61).  NEAREST: 29 032 of 32 025 rows kept, worst 7.4e-8.

One rule had to be completed.  "Rows not kept: one of the model's two adjacent texels" can hold only while float32 resolves single texels: from
|u W| 2^-23 >= 1/2 on (the coordinates up to 1e5 on the 1024-wide image, the ones near 2^30; 54 rows) u W in float32 is off by a texel or more -- 64
near 2^30 -- for ANY implementation of F4, so those rows allow every texel within ceil(|u W| 2^-23) of the model's on that axis instead.  The model
decides which rows these are (`far` in the fixture).  Every other row is held to the rule as stated.

"ZERO, ONE and UNKNOWN in every material's map" cannot hold on the whole grid of factors and cutoffs either (see test_opacity_maps_never_change_a_result).

That the checks can fail (done once in a scratch copy: the MODEL broken one rule at a time and re-minted, the unchanged oracle and host build run
against it; x = worst error / bound):
  -0.5 dropped                      oracle 8.9e5 x, tap footprint, environment 1.4e8 x, opacity (MASK decision, material 1)
  mirror without the -(1 + m)       wrap_index / wrap_coord, oracle 1.2e6 x, tap footprint, storage orders (texel read through a descriptor)
  clamp to n                        minting refuses (the model indexes its own image at n); wrap_index / wrap_coord
  weights a(1-b), (1-a)b swapped    oracle 7.6e5 x, environment 6.0e5 x, opacity (MASK decision)
  REPEAT on V of the environment    environment 2.1e8 x (nothing else: only that rule reads it)
and on the product's side, host build only:
  tex_index, tile row and tile column swapped (pt_device.h)        SAMPLE_REC, SAMPLE_DESC, tap footprint, storage orders, extreme sizes (65528 x 4 is no
                                                                    bijection), opacity (the map changed the class of an opacity)
  opacity apron removed (pt_scene_records.cpp build_opacity_maps, k = 0..3) opacity: the five blocks with one texel of 0 in their apron are classified ONE
"""
import ctypes as C

import numpy as np
import pytest

from tests import orc, tex_kat_io as io

EPS = 2.0 ** -23
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def kat():
    return io.load()


@pytest.fixture(scope="module")
def gen():
    return io.generator()


@pytest.fixture(scope="module")
def scene(kat):
    return io.fixture_scene(kat)


@pytest.fixture(scope="module")
def host(scene):
    h = io.HostScene(scene)
    yield h
    h.close()


@pytest.fixture(scope="module")
def oracle(scene):
    o = orc.Oracle()
    o.set_scene(scene)
    yield o
    o.close()


def oracle_rgba(oracle, kat):
    tid = kat["row_tex"].astype(np.int64) * io.CONFIGS + kat["row_cfg"]
    out = np.zeros((len(tid), 4), np.float32)
    fn, ctx, base = oracle.L.orc_sample_texture, oracle.ctx, out.ctypes.data
    for i, (t, u, v) in enumerate(zip(tid.tolist(), kat["row_u"].tolist(), kat["row_v"].tolist())):
        fn(ctx, t, u, v, base + 16 * i)
    return out


def oracle_env(oracle, u, v):
    out = np.zeros((len(u), 4), np.float32)
    fn, ctx, base = oracle.L.orc_hook_sample_env, oracle.ctx, out.ctypes.data
    for i, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
        fn(ctx, a, b, base + 16 * i)
    return out[:, :3]


# ---- the fixture itself -------------------------------------------------------------------------------------------------------------------------------
def test_generator_is_independent_and_deterministic(tmp_path, gen):
    import os
    import re
    src = open(os.path.join(io.GOLDEN, "gen_tex_kat.py")).read()
    imports = re.findall(r"^\s*(?:from|import)\s+([\w.]+)", src, re.M)
    assert set(imports) <= {"io", "os", "sys", "zipfile", "numpy", "gen_kat"}, imports   # nothing of oracle/, tests/orc.py, tests/ref.py, vk_raytrace_amd/
    out = str(tmp_path / "again.npz")
    gen.main(out)
    assert open(out, "rb").read() == open(os.path.join(io.GOLDEN, "tex_kat.npz"), "rb").read()
    assert os.path.getsize(out) < (1 << 20)


def test_fixture_meets_the_caps(kat, gen):
    want = {(1, 1), (2, 2), (1, 9), (9, 1), (3, 5), (7, 5), (8, 4), (12, 20), (16, 16), (24, 12), (7, 64), (64, 7), (40, 4), (255, 3), (1024, 8)}
    assert want <= {tuple(s) for s in kat["sizes"].tolist()}
    u, v = kat["row_u"].astype(np.float64), kat["row_v"].astype(np.float64)
    for t, (w, h) in enumerate(kat["sizes"]):
        m = kat["row_tex"] == t
        assert kat[f"tex{t}"].shape == (h, w, 4) and set(kat["row_cfg"][m]) == set(range(io.CONFIGS))   # 9 wrap pairs x 2 filters
        assert (np.abs(u[m] * w) < 2.0 ** 30).all() and (np.abs(v[m] * h) < 2.0 ** 30).all()              # the fixture is in-domain
        near = m & (kat["row_cfg"] % 2 == 0)
        assert kat["row_kept"][near].mean() >= 0.5, (w, h)
        # every k / W and (k + 0.5) / W over three periods each way, with both float32 neighbours
        k = np.arange(-3 * w - 2, 3 * w + 3, dtype=np.float64)
        for e in (np.float32(k / w), np.float32((k + 0.5) / w)):
            have = set(kat["row_u"][m].view(np.uint32).tolist())
            for x in (e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))):
                assert set(x.view(np.uint32).tolist()) <= have
        for s in (0.0, -0.0, 1.0, -1.0, 1.0 - 2.0 ** -24, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126):
            assert np.float32(s).view(np.uint32) in kat["row_u"][m].view(np.uint32) and np.float32(s).view(np.uint32) in kat["row_v"][m].view(np.uint32)
        assert np.abs(u[m] * w).max() > 2.0 ** 29 and np.abs(u[m]).max() > 1e4
    # the rows stored in full are the model's value as want_rgba / want_env rebuild it from the stored footprint and weights
    stride = int(kat["WANT_STRIDE"])
    assert np.array_equal(gen.want_rgba(kat)[::stride], kat["row_want"]) and np.array_equal(gen.want_env(kat)[0][::stride], kat["env_want"])


# ---- address modes, exhaustively --------------------------------------------------------------------------------------------------------------------------
def wrap_cases():
    i, n = [], []
    for size in list(range(1, 131)) + [255, 256, 1024, 65535]:
        ii = np.concatenate([np.arange(-3 * size - 2, 3 * size + 3), [2 ** 30, -2 ** 30, INT_MIN, INT_MAX]])
        i.append(ii)
        n.append(np.full(len(ii), size))
    return np.concatenate(i).astype(np.int64), np.concatenate(n).astype(np.int64)


def test_wrap_index_and_wrap_coord_equal_the_model_everywhere(gen, host):
    """wrap_index (pt_surface.h; with and without the power-of-two mask) and the oracle's wrap_coord against exact integer arithmetic: every size 1..130
    and 255, 256, 1024, 65535, every i three periods each way and +-2^30, INT_MIN, INT_MAX, the three address modes"""
    i, n = wrap_cases()
    pot = (n & (n - 1)) == 0
    L = orc.lib()
    for mode in (gen.REPEAT, gen.MIRRORED_REPEAT, gen.CLAMP_TO_EDGE):
        want = np.zeros(len(i), np.int64)
        for size in np.unique(n):
            m = n == size
            want[m] = gen.wrap(i[m], int(size), mode)
        assert ((want >= 0) & (want < n)).all()
        for use_pot in (False, True):
            m = pot if use_pot else np.ones(len(i), bool)
            got = host.probe(io.WRAP, io.rows(*io.ints(i[m], n[m], np.full(m.sum(), mode), np.full(m.sum(), int(use_pot)))))[:, 0].view(np.int32)
            assert np.array_equal(got, want[m]), (mode, use_pot, np.nonzero(got != want[m])[0][:5])
        fn = L.orc_wrap_coord
        got = np.fromiter((fn(a, b, mode) for a, b in zip(i.tolist(), n.tolist())), np.int64, len(i))
        assert np.array_equal(got, want), (mode, np.nonzero(got != want)[0][:5])


# ---- oracle and host build against the model ----------------------------------------------------------------------------------------------------------------
def check_against_model(kat, gen, got, leg):
    """LINEAR rows within the derived bound; NEAREST rows: the model's texel where kept, one of its two adjacent texels per axis elsewhere"""
    want = gen.want_rgba(kat)
    g = got.astype(np.float64)
    assert np.isfinite(g).all(), leg
    w, h = kat["sizes"][kat["row_tex"]].T
    bound = (np.abs(kat["row_u"].astype(np.float64) * w) + np.abs(kat["row_v"].astype(np.float64) * h) + 4.0) * EPS
    err = np.abs(g - want).max(1)
    lin = kat["row_cfg"] % 2 == 1
    ratio = err[lin] / bound[lin]
    print(f"{leg:12s} LINEAR  worst error / bound {ratio.max():.3f} over {int(lin.sum())} rows")
    assert ratio.max() <= 1.0, f"{leg}: LINEAR row {np.nonzero(lin)[0][ratio.argmax()]} is {ratio.max():.2f} x the bound away from the model"
    kept = kat["row_kept"] & ~lin
    print(f"{leg:12s} NEAREST worst error on {int(kept.sum())} kept rows {err[kept].max():.3e}")
    assert err[kept].max() <= EPS, f"{leg}: NEAREST row {np.nonzero(kept)[0][err[kept].argmax()]} is not the model's texel"
    far = kat["far"]
    rest = np.setdiff1d(np.nonzero(~kept & ~lin)[0], far[:, 0])
    ok = np.zeros(len(rest), bool)
    for xs in ("row_x0", "row_ax"):
        for ys in ("row_y0", "row_ay"):
            cand = np.zeros((len(rest), 4))
            for t in np.unique(kat["row_tex"][rest]):
                m = kat["row_tex"][rest] == t
                cand[m] = kat[f"tex{t}"][kat[ys][rest[m]], kat[xs][rest[m]]] / 255.0
            ok |= np.abs(g[rest] - cand).max(1) <= EPS
    assert ok.all(), f"{leg}: NEAREST row {rest[~ok][:5]} (not kept) is neither of the model's adjacent texels"
    # ... and where float32 no longer resolves single texels (|u W| 2^-23 >= 1/2): a texel within the coordinate's rounding of the model's
    for r, ix, xlo, xhi, iy, ylo, yhi in far.tolist():
        t, cfg = int(kat["row_tex"][r]), int(kat["row_cfg"][r])
        img = kat[f"tex{t}"]
        xs = gen.wrap(np.arange(ix + xlo, ix + xhi + 1), img.shape[1], cfg // 6)
        ys = gen.wrap(np.arange(iy + ylo, iy + yhi + 1), img.shape[0], (cfg // 2) % 3)
        cand = img[np.unique(ys)][:, np.unique(xs)].reshape(-1, 4) / 255.0
        assert (np.abs(cand - g[r]).max(1) <= EPS).any(), f"{leg}: NEAREST row {r} is no texel within the coordinate's rounding of the model's"
    return float(ratio.max())


def test_oracle_against_the_model(kat, gen, oracle):
    check_against_model(kat, gen, oracle_rgba(oracle, kat), "oracle")


@pytest.mark.parametrize("kind", ["SAMPLE_REC", "SAMPLE_DESC"])
def test_host_build_against_the_model_and_the_oracle(kat, gen, host, oracle, kind):
    """sample_rgba8_rec on the plain record, and the descriptor path of resolve_material (tex_desc_unpack, tex_tap, four loads, tex_filter) on the
    material line: within the bound of the model, and bit-identical to the oracle on every row, kept or not"""
    got = host.probe(getattr(io, kind), io.fixture_rows(kat, io.BASE_SLOT if kind == "SAMPLE_DESC" else -1))[:, :4]
    check_against_model(kat, gen, got, "host " + kind)
    bad = io.same_bits(got, oracle_rgba(oracle, kat))
    assert bad == 0, f"{kind}: host build and oracle differ in {bad} values"


def test_tap_is_the_models_footprint(kat, gen, host):
    """tex_tap on its own: on kept NEAREST rows and on LINEAR rows whose coordinate is exact in float32 the four indices are the model's footprint in
    the storage order of the record (tex_index through the INDEX probe) and the weights are the model's exactly; everywhere the weights are within
    the coordinate's rounding of the model's (modulo the texel edge, where the footprint shifts by one and the weight wraps round)"""
    tap = host.probe(io.TAP, io.fixture_rows(kat))
    idx, a, b = tap[:, :4].view(np.uint32).astype(np.int64), tap[:, 4].astype(np.float64), tap[:, 5].astype(np.float64)
    tid = kat["row_tex"].astype(np.int64) * io.CONFIGS + kat["row_cfg"]
    rec = host.tex_recs[tid]
    w, h = kat["sizes"][kat["row_tex"]].T
    assert (idx >= rec[:, 0:1]).all() and (idx < (rec[:, 0] + w * h)[:, None]).all()
    lin = kat["row_cfg"] % 2 == 1
    x, y = kat["row_u"].astype(np.float64) * w, kat["row_v"].astype(np.float64) * h
    f32 = lambda c: c.astype(np.float32) == c
    exact = f32(x) & f32(y) & f32(x - 0.5) & f32(y - 0.5)   # (x - 0.5 can leave float32 where it crosses a power of two: -7.5000005 - 0.5 rounds to -8)
    sure = np.where(lin, exact, kat["row_kept"])
    assert sure[lin].mean() > 0.2 and sure[~lin].mean() > 0.5
    for k, (xs, ys) in enumerate((("row_x0", "row_y0"), ("row_x1", "row_y0"), ("row_x0", "row_y1"), ("row_x1", "row_y1"))):
        at = host.probe(io.INDEX, io.rows(*io.ints(w, kat[xs], kat[ys], rec[:, 7] & 1)))[:, 0].view(np.uint32).astype(np.int64)
        assert np.array_equal(idx[sure, k], (rec[:, 0] + at)[sure]), k
    fits = sure & f32(kat["row_a"]) & f32(kat["row_b"])   # (the fraction of a small negative coordinate, 1 - 1e-7, needs more than 24 bits)
    assert fits[lin].mean() > 0.2 and np.array_equal(a[fits], kat["row_a"][fits]) and np.array_equal(b[fits], kat["row_b"][fits])
    for got, want, c in ((a, kat["row_a"], x), (b, kat["row_b"], y)):
        d = np.abs(got - want)
        d = np.minimum(d, 1.0 - d)
        assert (d[lin] <= np.abs(c[lin]) * EPS + 2.0 ** -24).all()
        assert (got >= 0).all() and (got <= 1).all()


def test_environment_against_the_model(kat, gen, host, oracle):
    """sample_env (RGBA32F, U repeat, V clamp to edge): oracle and host build within the bound x the largest |texel| of the footprint, and equal bit for bit"""
    want, scale = gen.want_env(kat)
    worst = 0.0
    for e, (w, h) in enumerate(kat["env_sizes"]):
        m = kat["env_img"] == e
        u, v = kat["env_u"][m], kat["env_v"][m]
        host.set_env(kat[f"env{e}"])
        oracle.set_env(kat[f"env{e}"])
        a, b = oracle_env(oracle, u, v), host.probe(io.ENV, io.rows(u, v))[:, :3]
        assert io.same_bits(a, b) == 0, f"environment {w} x {h}: host build and oracle differ"
        bound = (np.abs(u.astype(np.float64) * w) + np.abs(v.astype(np.float64) * h) + 4.0) * EPS * scale[m]
        ratio = np.abs(a.astype(np.float64) - want[m]).max(1) / bound
        assert np.isfinite(ratio).all() and ratio.max() <= 1.0, (w, h, ratio.max(), int(ratio.argmax()))
        worst = max(worst, float(ratio.max()))
    print(f"environment  LINEAR  worst error / bound {worst:.3f} over {len(want)} rows")


# ---- storage orders ---------------------------------------------------------------------------------------------------------------------------------------------
ROLES = ("normalTexture", "emissiveTexture", "pbrMetallicRoughnessTexture", "pbrBaseColorTexture")   # the order of a material line's descriptors


def storage_scene(gen):
    """materials with one to four textures of equal size and sampler, one with equal size and different samplers, one texture in two roles, one
    texture shared by materials that group differently; tile-eligible (16 x 8, 8 x 4, 24 x 12) and not (12 x 20) sizes, both filters, all address modes"""
    from vk_raytrace_amd.scene import Scene
    sc = Scene("storage orders")
    img = lambda w, h, salt: gen.words(w * h, salt).view(np.uint8).reshape(h, w, 4)
    A = [sc.add_texture(img(16, 8, 500 + k), magFilter=1, wrapS=gen.REPEAT, wrapT=gen.MIRRORED_REPEAT) for k in range(4)]
    B = [sc.add_texture(img(12, 20, 510 + k), magFilter=0, wrapS=gen.CLAMP_TO_EDGE, wrapT=gen.REPEAT) for k in range(2)]
    Cs = [sc.add_texture(img(8, 4, 520), magFilter=1, wrapS=gen.REPEAT, wrapT=gen.REPEAT), sc.add_texture(img(8, 4, 521), magFilter=0, wrapS=gen.MIRRORED_REPEAT, wrapT=gen.CLAMP_TO_EDGE)]
    D = sc.add_texture(img(24, 12, 530), magFilter=1, wrapS=gen.MIRRORED_REPEAT, wrapT=gen.MIRRORED_REPEAT)
    mats = [dict(pbrBaseColorTexture=A[0]),
            dict(normalTexture=A[0], pbrBaseColorTexture=A[1]),
            dict(normalTexture=A[0], emissiveTexture=A[1], pbrMetallicRoughnessTexture=A[2]),
            dict(normalTexture=A[0], emissiveTexture=A[1], pbrMetallicRoughnessTexture=A[2], pbrBaseColorTexture=A[3]),
            dict(normalTexture=Cs[0], pbrBaseColorTexture=Cs[1]),                                       # equal size, different samplers
            dict(normalTexture=B[0], emissiveTexture=B[1], pbrBaseColorTexture=B[0]),                  # one texture in two roles
            dict(emissiveTexture=A[0], pbrMetallicRoughnessTexture=A[2], pbrBaseColorTexture=D),       # A[0] and A[2] again, grouped differently
            dict(normalTexture=D, emissiveTexture=A[3], pbrMetallicRoughnessTexture=D, pbrBaseColorTexture=A[0])]
    for m in mats:
        sc.add_material(**m)
    io.add_quad(sc, 0)
    return sc.finalize(io.capi.pack_vertices), mats


def test_storage_orders_hold_the_same_texels(gen):
    """row-major, block-linear and interleaved group storage under PT_TUNE unset, texTile=0, texGroups=0 and both: every texel of every texture read
    through every material-line descriptor (tex_tap, both filters) is the source image's texel; tex_index is a bijection onto [0, w h);
    tex_desc_unpack(tex_desc_pack(r)) == r; SAMPLE_DESC == SAMPLE_REC bit for bit, and the same bits under all four settings"""
    sc, mats = storage_scene(gen)
    uvs = np.concatenate([gen.uniform(400, 77, -3.0, 3.0).reshape(-1, 2), [(0, 0), (1, 1), (-1, 0.5), (0.5, -0.0), (0.999999, 1e-7)]]).astype(np.float32)
    reference, layered = None, {}
    for tune in io.TUNES:
        hs = io.HostScene(sc, tune)
        recs = hs.tex_recs
        assert np.array_equal(hs.probe(io.DESC, io.rows(*io.ints(np.arange(len(recs)), np.full(len(recs), -1)))).view(np.int32), recs)
        for r in recs:
            o, w, h, tiled = int(r[0]), int(r[1]), int(r[2]), int(r[7])
            assert tiled == (0 if tune and "texTile=0" in tune else int(w % 8 == 0 and h % 4 == 0))
            ix, iy = np.meshgrid(np.arange(w), np.arange(h))
            at = hs.probe(io.INDEX, io.rows(*io.ints(np.full(w * h, w), ix.ravel(), iy.ravel(), np.full(w * h, tiled))))[:, 0].view(np.uint32)
            assert np.array_equal(np.sort(at), np.arange(w * h))
        sampled = []
        layered[tune] = 0
        for m, roles in enumerate(mats):
            for slot, role in enumerate(ROLES):
                if role not in roles:
                    continue
                t = roles[role]
                tex = sc.textures[t]
                src = tex.rgba8.reshape(-1, 4).view(np.uint32).reshape(tex.rgba8.shape[:2])
                d = hs.probe(io.DESC, io.rows(*io.ints(m, slot)))[0].view(np.int32)
                assert np.array_equal(d[1:7], recs[t][1:7]) and (d[7] & 1) == (recs[t][7] & 1), (tune, m, role)
                layered[tune] += int((d[7] >> 8) & 3 > 0)
                h, w = src.shape
                ix, iy = (a.ravel() for a in np.meshgrid(np.arange(w), np.arange(h)))
                off = 0.75 if tex.magFilter == 1 else 0.5   # LINEAR: x - 0.5 = ix + 0.25, the footprint is (ix, iy) .. (ix + 1, iy + 1)
                tap = hs.probe(io.TAP, io.rows(*io.ints(np.full(w * h, m), np.full(w * h, slot)), ((ix + off) / w).astype(np.float32), ((iy + off) / h).astype(np.float32)))
                idx = tap[:, :4].view(np.uint32)
                assert idx.max() < len(hs.texels)
                step = int(tex.magFilter == 1)
                for k, (dx, dy) in enumerate(((0, 0), (step, 0), (0, step), (step, step))):
                    want = src[gen.wrap(iy + dy, h, tex.wrapT), gen.wrap(ix + dx, w, tex.wrapS)]
                    assert np.array_equal(hs.texels[idx[:, k]], want), (tune, m, role, k)
                a = hs.probe(io.SAMPLE_DESC, io.rows(*io.ints(np.full(len(uvs), m), np.full(len(uvs), slot)), uvs[:, 0], uvs[:, 1]))[:, :4]
                b = hs.probe(io.SAMPLE_REC, io.rows(*io.ints(np.full(len(uvs), t), np.full(len(uvs), -1)), uvs[:, 0], uvs[:, 1]))[:, :4]
                assert np.isfinite(a).all() and io.same_bits(a, b) == 0, (tune, m, role)
                sampled.append(a)
        sampled = np.concatenate(sampled)
        reference = sampled if reference is None else reference
        assert io.same_bits(sampled, reference) == 0, tune
        hs.close()
    # the settings do what they say: groups exist by default and with texTile=0 only
    assert layered[None] > 0 and layered["texTile=0"] > 0 and layered["texGroups=0"] == 0 and layered["texTile=0,texGroups=0"] == 0


EXTREMES = ((65535, 1), (1, 65535), (65528, 4), (8, 65532))


def extreme_scene(sizes=EXTREMES):
    from vk_raytrace_amd.scene import Scene
    sc = Scene("extreme sizes")
    for k, (w, h) in enumerate(sizes):
        t = sc.add_texture(np.zeros((h, w, 4), np.uint8), magFilter=k % 2, wrapS=k % 3, wrapT=(k + 1) % 3)
        sc.add_material(pbrBaseColorTexture=t)
    io.add_quad(sc, 0)
    return sc.finalize(io.capi.pack_vertices)


def extreme_index_rows(hs):
    """tex_index rows over the whole of every extreme image in the storage order of its record"""
    out = []
    for r in hs.tex_recs:
        w, h, tiled = int(r[1]), int(r[2]), int(r[7]) & 1
        ix, iy = (a.ravel() for a in np.meshgrid(np.arange(w), np.arange(h)))
        out.append((w, h, io.rows(*io.ints(np.full(w * h, w), ix, iy, np.full(w * h, tiled)))))
    return out


def extreme_tap_rows(hs, gen):
    n = 2000
    u, v = gen.uniform(n, 91, -3.0, 3.0).astype(np.float32), gen.uniform(n, 92, -3.0, 3.0).astype(np.float32)
    edge = np.array([0.0, 1.0, -1.0, 1.0 - 2.0 ** -24, -2.0 ** -149, 0.5, 65534.5 / 65535, 65527.75 / 65528], np.float32)
    u, v = np.concatenate([u, edge, edge[::-1]]), np.concatenate([v, edge, edge])
    return [io.rows(*io.ints(np.full(len(u), t), np.full(len(u), slot)), u, v) for t in range(len(hs.tex_recs)) for slot in (-1, io.BASE_SLOT)]


def test_extreme_sizes_index_inside_the_image(gen):
    """65535 x 1, 1 x 65535, 65528 x 4 and 8 x 65532 (the last two block-linear): tex_index is a bijection onto [0, w h), every tap index stays
    inside the image's part of the pool; 65536 texels on either side are rejected"""
    hs = io.HostScene(extreme_scene())
    assert [int(r[7]) & 1 for r in hs.tex_recs] == [0, 0, 1, 1]
    for w, h, r in extreme_index_rows(hs):
        at = hs.probe(io.INDEX, r)[:, 0].view(np.uint32)
        assert np.array_equal(np.sort(at), np.arange(w * h)), (w, h)
    for k, r in enumerate(extreme_tap_rows(hs, gen)):
        rec = hs.tex_recs[k // 2]
        idx = hs.probe(io.TAP, r)[:, :4].view(np.uint32).astype(np.int64)
        assert (idx >= rec[0]).all() and (idx < rec[0] + int(rec[1]) * int(rec[2])).all(), k
    hs.close()
    for sizes in (((65536, 1),), ((1, 65536),)):
        bad = io.HostScene(extreme_scene(sizes), expect_error=True)
        assert not bad.h and "65535" in bad.error, bad.error


# ---- outside the domain ---------------------------------------------------------------------------------------------------------------------------------------
def outside_rows(kat):
    c = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 2.0 ** 31, -2.0 ** 31, 2.0 ** 33, -2.0 ** 33, 0.25], np.float32)
    u, v = (a.ravel() for a in np.meshgrid(c, c))
    u, v = u[:-1], v[:-1]   # (0.25, 0.25) is inside
    ids = np.arange(len(kat["sizes"]) * io.CONFIGS)
    return [io.rows(*io.ints(np.repeat(ids, len(u)), np.full(len(ids) * len(u), slot)), np.tile(u, len(ids)), np.tile(v, len(ids))) for slot in (-1, io.BASE_SLOT)]


def test_outside_the_domain_every_index_stays_inside_the_pool(kat, scene):
    """NaN, +-Inf, +-3e38, +-2^31, +-2^33 on either axis, every size, wrap pair and filter, plain record and material-line descriptor, all four storage
    settings: tex_tap (no loads) returns indices below the pool size.  Nothing else is claimed there (the conversion is undefined in C++)"""
    for tune in io.TUNES:
        hs = io.HostScene(scene, tune)
        for r in outside_rows(kat):
            idx = hs.probe(io.TAP, r, fill=0.0)[:, :4].view(np.uint32)
            assert idx.max() < len(hs.texels), tune
        hs.close()


def test_probe_refuses_what_it_cannot_hold(host):
    """unknown kinds, short rows, ids beyond the scene's arrays; a loading kind leaves an out-of-domain row untouched instead of loading"""
    p, h = host.L.th_texture_probe, host.h
    r, o = np.zeros((4, io.IN), np.float32), np.zeros((4, io.OUT), np.float32)
    assert p(h, 99, 4, r.ctypes.data, io.IN, o.ctypes.data, io.OUT) == -1 and p(h, io.TAP, 4, r.ctypes.data, io.IN - 1, o.ctypes.data, io.OUT) == -1
    big = len(host.tex_recs)
    for kind, row in ((io.TAP, io.rows(*io.ints(big, -1), 0.5, 0.5)), (io.SAMPLE_REC, io.rows(*io.ints(-1, -1), 0.5, 0.5)), (io.SAMPLE_DESC, io.rows(*io.ints(big, 3), 0.5, 0.5)),
                      (io.SAMPLE_DESC, io.rows(*io.ints(0, 4), 0.5, 0.5)), (io.SAMPLE_REC, io.rows(*io.ints(0, -1), np.float32(np.nan), 0.5)),
                      (io.SAMPLE_DESC, io.rows(*io.ints(0, 3), 0.5, np.float32(2.0 ** 31)))):
        assert np.isnan(host.probe(kind, row)).all(), kind
    assert np.isfinite(host.probe(io.SAMPLE_DESC, io.rows(*io.ints(0, 3), 0.5, 0.5))[:, :4]).all()



# ---- opacity maps -----------------------------------------------------------------------------------------------------------------------------------------------
MASK, BLEND = 1, 2
ALPHA_FAST_TAP, ALPHA_NO_MAP = 1 << 24, 0xFFFFFFFF
ST_UNKNOWN, ST_ZERO, ST_ONE = 0, 1, 2
ASIZE = 64                       # 16 x 16 blocks of 4 x 4 texels
# blocks whose surroundings are looked at tap by tap: the uniform regions' interiors, a background block, the corner of the alpha-0 region, and the
# blocks that are uniform except for ONE texel in their apron (column, row, corner, and the wrapped neighbours across the left and the top image edge)
POKES = {(8, 8): (31, 33), (12, 8): (49, 36), (0, 12): (63, 49), (13, 0): (54, 63), (8, 12): (31, 47)}   # block -> the texel in its apron
WINDOWS = [(2, 2), (6, 2), (10, 2), (2, 6), (6, 6), (1, 1)] + list(POKES)


def alpha_image(gen):
    """RGB random; alpha 255 except: a 12 x 12 region of 0, of 170 (1.5 x 170 / 255 = 1 and 1 x 170 / 255 = 2 / 3), of 200 and of random bytes, and single
    texels of 0 in the apron of otherwise uniform blocks"""
    img = gen.words(ASIZE * ASIZE, 700).view(np.uint8).reshape(ASIZE, ASIZE, 4).copy()
    a = img[:, :, 3]
    rnd = a.copy()
    a[:] = 255
    a[4:16, 4:16] = 0
    a[4:16, 20:32] = 170
    a[4:16, 36:48] = 200
    a[20:32, 4:16] = rnd[20:32, 4:16]
    for x, y in POKES.values():
        a[y, x] = 0
    return img


def alpha_materials():
    """(mode, cutoff, factor, texture): the issue's grid, then factors tuned so that factor x 200 / 255 falls 2e-5 and 5e-6 below, on, and as much above
    the cutoff 0.5 (MASK) and 1 (BLEND: where the map may say ONE) -- below, inside and above the 1e-5 window -- and the NEAREST copy of the image"""
    out = [(MASK, c, f, 0) for c in (0.0, 0.5, 1.0, -0.25) for f in (0.0, 0.7, 1.0, 1.5)] + [(BLEND, 0.5, f, 0) for f in (0.0, 0.7, 1.0, 1.5)]
    for k in (-2.0, -0.5, 0.0, 0.5, 2.0):
        out.append((MASK, 0.5, 0.5 * 255 / 200 * (1 + k * 1e-5), 0))
        out.append((BLEND, 0.5, 255 / 200 * (1 + k * 1e-5), 0))
    out += [(MASK, 0.5, 1.0, 1), (MASK, 1.0, 1.5, 1), (BLEND, 0.5, 1.5, 1)]
    return out


def alpha_scene(gen):
    from vk_raytrace_amd.scene import Scene
    sc = Scene("adversarial alpha")
    img = alpha_image(gen)
    for mag in (1, 0):
        sc.add_texture(img, magFilter=mag, minFilter=mag, wrapS=gen.REPEAT, wrapT=gen.REPEAT)
    for mode, cutoff, factor, tex in alpha_materials():
        sc.add_material(alphaMode=mode, alphaCutoff=cutoff, pbrBaseColorFactor=(1.0, 1.0, 1.0, factor), pbrBaseColorTexture=tex)
    io.add_quad(sc, 0)
    return sc.finalize(io.capi.pack_vertices), img


def alpha_taps():
    """barycentrics (bu, bv) = (u, v) of the triangle (0, 0) (1, 0) (0, 1): 16 x 16 taps per texel, texel edges and centres included, over an 8 x 8-texel
    window round every block of WINDOWS (negative coordinates left of / above the image: the wrapped neighbours), and 4 x 4 taps per texel over the image"""
    parts = []
    for bx, by in WINDOWS:
        u = (np.arange(129) / 16.0 + (4 * bx - 2)) / ASIZE
        v = (np.arange(129) / 16.0 + (4 * by - 2)) / ASIZE
        parts.append(np.stack(np.meshgrid(u, v), -1).reshape(-1, 2))
    c = np.arange(4 * ASIZE + 1) / (4.0 * ASIZE)
    parts.append(np.stack(np.meshgrid(c, c), -1).reshape(-1, 2))
    return np.concatenate(parts).astype(np.float32)   # (every value is a multiple of 2^-10: exact)


def opacity_rows(material, taps):
    n = len(taps)
    one, zero = np.ones(n, np.float32), np.zeros(n, np.float32)
    return io.rows(zero, zero, one, zero, zero, one, io.ints(np.full(n, material))[0], taps[:, 0], taps[:, 1])


def map_states(hs, m):
    am = hs.alpha_mats[m]
    off, bw, bh = int(am[17]), int(am[13]) >> 2, int(am[14]) >> 2
    if off == ALPHA_NO_MAP:
        return None
    b = np.arange(bw * bh)
    return ((hs.alpha_maps[off + (b >> 4)] >> ((b & 15) * 2)) & 3).reshape(bh, bw)


def check_opacity(gen, img, mats, taps, m, got):
    """the four assertions on every tap of material m; returns how many taps the map answered"""
    mode, cutoff, factor, tex = mats[m]
    exact, mapped = got[:, 0].astype(np.float64), got[:, 1].astype(np.float64)
    assert np.isfinite(got[:, :2]).all()
    inside = (exact > 0) & (exact < 1)
    assert np.array_equal(got[inside, 1].view(np.uint32), got[inside, 0].view(np.uint32)), f"material {m} {mats[m]}: the map changed an opacity in (0, 1)"
    assert (((exact <= 0) & (mapped <= 0)) | ((exact >= 1) & (mapped >= 1)))[~inside].all(), f"material {m} {mats[m]}: the map changed the class of an opacity"
    # the model: factor x filtered alpha (float32 factor and cutoff as the records hold them)
    lin = np.full(len(taps), tex == 0)
    rep = np.zeros(len(taps), np.int64)
    x0, x1, a = gen.axis(taps[:, 0], ASIZE, rep, lin)[:3]
    y0, y1, b = gen.axis(taps[:, 1], ASIZE, rep, lin)[:3]
    al = img[:, :, 3:4].astype(np.float64)
    f32 = float(np.float32(factor))
    value = f32 * gen.blend(al[y0, x0], al[y0, x1], al[y1, x0], al[y1, x1], a, b)[:, 0] / 255.0
    bound = (np.abs(taps[:, 0].astype(np.float64) * ASIZE) + np.abs(taps[:, 1].astype(np.float64) * ASIZE) + 4.0) * EPS
    if tex == 1:   # NEAREST: the taps are multiples of 1 / 16 texel, exact in float32 -- the texel is the model's, the value byte x factor / 255
        bound = np.full(len(taps), 4.0 * EPS)
    if mode == BLEND:
        ratio = np.abs(exact - value) / bound
        assert ratio.max() <= 1.0, f"material {m} {mats[m]}: opacity {ratio.max():.2f} x the bound away from the model at tap {int(ratio.argmax())}"
    else:
        clear = np.abs(value - float(np.float32(cutoff))) > bound
        assert np.array_equal(exact[clear], (value > float(np.float32(cutoff)))[clear].astype(np.float64)), f"material {m} {mats[m]}: MASK decision differs from the model"
    return int(np.count_nonzero(got[:, 1].view(np.uint32) != got[:, 0].view(np.uint32))), (float(clear.mean()) if mode == MASK else None)


def test_opacity_maps_never_change_a_result(gen):
    """opacity_eval<true> (the map answers where it can) against opacity_eval<false> (the exact value) and against the model, on adversarial alpha: MASK
    and BLEND, cutoffs 0, 0.5, 1, -0.25, factors 0, 0.7, 1, 1.5 and factors tuned to put factor x alpha below, inside and above the 1e-5 window round
    the cutoff; blocks that are uniform but for one texel in their apron column, row or corner, and in the wrapped neighbour across the image edge.
    On every tap: equal where the exact value is in (0, 1); <= 0 or >= 1 together elsewhere; BLEND within the LINEAR bound of the model's
    factor x alpha; the MASK decision the model's wherever its value is farther than the bound from the cutoff.
    The maps must be exercised: "ZERO, ONE and UNKNOWN in every material" cannot hold for all of the grid above (factor 0 decides every block the same
    way, a negative cutoff makes every block ONE, cutoff 1 with factor <= 1 leaves nothing above it), so it is asserted for every material where the
    three are reachable -- MASK with cutoff 0.5 and factor >= 0.7, BLEND with factor >= 1.5; every block with a poked apron
    must be UNKNOWN wherever its unpoked twin (6, 6) is ONE and the alpha-0 block (2, 2) is ZERO.
    Fast tap == general path: the same taps with ALPHA_FAST_TAP cleared in the records (wrap_index with the power-of-two masks), bit for bit."""
    sc, img = alpha_scene(gen)
    mats, taps = alpha_materials(), alpha_taps()
    assert len(taps) >= 16 * 16 * 64 * len(WINDOWS)
    hs = io.HostScene(sc)
    answered, poked, clears, results = 0, 0, [], []
    for m, (mode, cutoff, factor, tex) in enumerate(mats):
        am = hs.alpha_mats[m]
        assert int(am[16]) & ALPHA_FAST_TAP and int(am[2]) == mode and am[0:2].view(np.float32).tolist() == [np.float32(factor), np.float32(cutoff)]
        st = map_states(hs, m)
        assert st is not None
        have = set(np.unique(st).tolist())
        if (mode == MASK and cutoff == 0.5 and factor >= 0.7) or (mode == BLEND and factor >= 1.5):
            assert have == {ST_UNKNOWN, ST_ZERO, ST_ONE}, (mats[m], have)
        if st[6, 6] == ST_ONE and st[2, 2] == ST_ZERO:   # alpha 255 and alpha 0 decide differently: one texel of 0 in the apron must undo the block
            poked += 1
            assert all(st[by, bx] == ST_UNKNOWN for bx, by in POKES), (mats[m], [int(st[by, bx]) for bx, by in POKES])
        got = hs.probe(io.OPACITY, opacity_rows(m, taps))
        n, clear = check_opacity(gen, img, mats, taps, m, got)
        answered += n
        clears += [] if clear is None else [clear]
        results.append(got[:, :2].copy())
    assert np.mean(clears) > 0.7   # the MASK decision is checked on most taps (not where factor x alpha IS the cutoff: alpha 0 against cutoff 0, 200 against the tuned factors)
    assert poked >= 8
    assert answered > 100000   # (the map answers with exactly 0 or 1: it differs from the exact value wherever that is a BLEND opacity > 1 or < 0, and says so here)
    hs.L.th_clear_fast_tap(hs.h)
    for m in range(len(mats)):
        got = hs.probe(io.OPACITY, opacity_rows(m, taps))
        assert np.array_equal(got[:, 0].view(np.uint32), results[m][:, 0].view(np.uint32)), f"material {m} {mats[m]}: fast tap and general path differ"
        assert np.array_equal(got[:, 1].view(np.uint32), got[:, 0].view(np.uint32))   # (no map without the fast tap)
    hs.close()


# ---- the device -----------------------------------------------------------------------------------------------------------------------------------------------
class DeviceScene:
    def __init__(self, scene, tune=None, env=None):
        from vk_raytrace_amd import capi
        self.L = capi.lib()
        self.ctx = C.c_void_p()
        with io.tuned(tune):
            assert self.L.pt_create(0, C.byref(self.ctx)) == 0
        d, self.keep = scene.desc()
        assert self.L.pt_set_scene(self.ctx, C.byref(d)) == 0, self.L.pt_last_error(self.ctx)
        if env is not None:
            self.set_env(env)

    def set_env(self, img):
        img = np.ascontiguousarray(img, np.float32)
        assert self.L.pt_set_env(self.ctx, img.ctypes.data, img.shape[1], img.shape[0], None, None) == 0

    def probe(self, kind, r, fill=np.nan):
        return io.probe(self.L.pt_debug_texture_probe, self.ctx, kind, r, fill)

    def close(self):
        self.L.pt_destroy(self.ctx)


@pytest.mark.gpu
def test_device_tap_and_samples_are_the_host_builds(kat, gen, scene, host):
    """one context on the fixture's scene: tex_tap, sample_rgba8_rec, the descriptor path, sample_env, wrap_index and tex_index on the device, bit for
    bit the host build of the same headers on every in-domain row (this is where tex_index's 24-bit multiply is seen), and within the model's bound;
    out-of-domain rows: TAP only, every index inside the pool, under all four storage settings"""
    dev = DeviceScene(scene)
    try:
        plain, line = io.fixture_rows(kat), io.fixture_rows(kat, io.BASE_SLOT)
        for kind, r in ((io.TAP, plain), (io.TAP, line), (io.SAMPLE_REC, plain), (io.SAMPLE_DESC, line)):
            a, b = dev.probe(kind, r), host.probe(kind, r)
            assert np.array_equal(a.view(np.uint32)[:, :6], b.view(np.uint32)[:, :6]), f"kind {kind}: device and host build differ on {np.count_nonzero((a.view(np.uint32) != b.view(np.uint32))[:, :6].any(1))} rows"
            if kind != io.TAP:
                check_against_model(kat, gen, a[:, :4], f"device {kind}")
        i, n = wrap_cases()
        for mode in (0, 1, 2):
            for use_pot in (0, 1):
                m = ((n & (n - 1)) == 0) if use_pot else np.ones(len(i), bool)
                r = io.rows(*io.ints(i[m], n[m], np.full(m.sum(), mode), np.full(m.sum(), use_pot)))
                assert np.array_equal(dev.probe(io.WRAP, r)[:, 0].view(np.uint32), host.probe(io.WRAP, r)[:, 0].view(np.uint32)), (mode, use_pot)
        for e in range(len(kat["env_sizes"])):
            m = kat["env_img"] == e
            r = io.rows(kat["env_u"][m], kat["env_v"][m])
            dev.set_env(kat[f"env{e}"])
            host.set_env(kat[f"env{e}"])
            a, b = dev.probe(io.ENV, r)[:, :3], host.probe(io.ENV, r)[:, :3]
            assert np.isfinite(a).all() and io.same_bits(a, b) == 0, f"environment {e}: device and host build differ"
        # refused before anything is launched / left alone by the kernel
        z, o = np.zeros((4, io.IN), np.float32), np.zeros((4, io.OUT), np.float32)
        fn = dev.L.pt_debug_texture_probe
        assert fn(dev.ctx, 99, 4, z.ctypes.data, io.IN, o.ctypes.data, io.OUT) == io.capi.PT_ERR_INVALID and fn(dev.ctx, io.TAP, 4, z.ctypes.data, io.IN - 1, o.ctypes.data, io.OUT) == io.capi.PT_ERR_INVALID
        assert np.isnan(dev.probe(io.SAMPLE_REC, io.rows(*io.ints(len(host.tex_recs) + 100000, -1), 0.5, 0.5))).all()
        assert np.isnan(dev.probe(io.SAMPLE_DESC, io.rows(*io.ints(0, 3), np.float32(np.nan), 0.5))).all()
    finally:
        dev.close()
    for tune in io.TUNES:
        hs, dev = io.HostScene(scene, tune), DeviceScene(scene, tune)
        try:
            for r in outside_rows(kat):
                idx = dev.probe(io.TAP, r, fill=0.0)[:, :4].view(np.uint32)
                bad = np.nonzero((idx >= len(hs.texels)).any(1))[0]
                assert len(bad) == 0, f"PT_TUNE={tune}: {len(bad)} taps index outside the pool, first (texture id, slot, u, v) = {[(int(a), int(b), float(c), float(d)) for a, b, c, d in zip(r[bad[:6], 0].view(np.int32), r[bad[:6], 1].view(np.int32), r[bad[:6], 2], r[bad[:6], 3])]}, wrap modes of all: {sorted(set(((r[bad, 0].view(np.int32) % io.CONFIGS) // 2).tolist()))}"
            r = io.fixture_rows(kat, io.BASE_SLOT)[::7]
            assert np.array_equal(dev.probe(io.SAMPLE_DESC, r).view(np.uint32)[:, :4], hs.probe(io.SAMPLE_DESC, r).view(np.uint32)[:, :4]), tune
        finally:
            dev.close()
            hs.close()


@pytest.mark.gpu
def test_device_index_arithmetic_at_the_extreme_sizes(gen):
    """65535 x 1, 1 x 65535, 65528 x 4, 8 x 65532: tex_index over the whole image and tex_tap, device == host build (row x stride reaches 2^18 x 2^18
    / 4: what the device multiplies in 24 bits)"""
    sc = extreme_scene()
    hs, dev = io.HostScene(sc), DeviceScene(sc)
    try:
        for w, h, r in extreme_index_rows(hs):
            assert np.array_equal(dev.probe(io.INDEX, r)[:, 0].view(np.uint32), hs.probe(io.INDEX, r)[:, 0].view(np.uint32)), (w, h)
        for r in extreme_tap_rows(hs, gen):
            assert np.array_equal(dev.probe(io.TAP, r).view(np.uint32)[:, :6], hs.probe(io.TAP, r).view(np.uint32)[:, :6])
    finally:
        dev.close()
        hs.close()


@pytest.mark.gpu
def test_device_opacity_is_the_host_builds(gen):
    """opacity_eval<false> and <true> on the device, bit for bit the host build on every tap of the adversarial alpha scene, with the image stored
    block-linear (the default) and row-major"""
    sc, _ = alpha_scene(gen)
    mats, taps = alpha_materials(), alpha_taps()
    for tune in (None, "texTile=0"):
        hs, dev = io.HostScene(sc, tune), DeviceScene(sc, tune)
        try:
            for m in range(len(mats)):
                r = opacity_rows(m, taps)
                a, b = dev.probe(io.OPACITY, r)[:, :2], hs.probe(io.OPACITY, r)[:, :2]
                assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{tune}: material {m} {mats[m]}: device and host build differ"
        finally:
            dev.close()
            hs.close()


def uv_transform(rotation=0.0, offset=(0.0, 0.0), scale=(1.0, 1.0)):
    """the 16 floats of pt_GltfShadeMaterial::uvTransform: u' = u m0 + v m1 + m2 + m3, v' = u m4 + v m5 + m6 + m7 (pt_surface.h resolve_material)"""
    c, s = np.cos(rotation), np.sin(rotation)
    m = np.eye(4, dtype=np.float32)
    m[0, :3] = (scale[0] * c, -scale[1] * s, offset[0])
    m[1, :3] = (scale[0] * s, scale[1] * c, offset[1])
    return m.reshape(16)


def texture_chart(kat, gen):
    """a wall of quads, one per fixture texture and sampler (the 9 wrap pairs and both filters go round), texture coordinates from -1.5 to 2.5 so that
    every address mode shows; every third material turns, shifts or flips its coordinates (rotation, offset, negative scale: the full-record path of
    resolve_material, the others take the material-line path); in front of the wall MASK and BLEND cards with the adversarial alpha image"""
    from vk_raytrace_amd.scene import Scene, Camera
    sc = Scene("texture chart")
    cols = 6
    xforms = [None, None, dict(rotation=0.6, offset=(0.25, -0.4)), None, None, dict(scale=(-1.5, 0.75), offset=(0.1, 0.3)), None, None, dict(rotation=-2.2, scale=(0.5, -2.0))]
    quad = lambda x, y, z, s: [(x - s, y - s, z), (x + s, y - s, z), (x + s, y + s, z), (x - s, y + s, z)]
    uv = [(-1.5, -1.5), (2.5, -1.5), (2.5, 2.5), (-1.5, 2.5)]
    n = 0
    for t in range(len(kat["sizes"])):
        for rep in range(2):
            cfg = (7 * n + 3) % io.CONFIGS
            tid = sc.add_texture(kat[f"tex{t}"], magFilter=cfg % 2, minFilter=cfg % 2, wrapS=cfg // 6, wrapT=(cfg // 2) % 3)
            kw = dict(pbrBaseColorTexture=tid, pbrMetallicFactor=0.0, pbrRoughnessFactor=0.9, doubleSided=1)
            if rep:   # a second image of the same size and sampler in the emissive role: the pair is stored as an interleaved group
                kw["emissiveTexture"] = sc.add_texture(np.roll(kat[f"tex{t}"], 1, axis=2), magFilter=cfg % 2, minFilter=cfg % 2, wrapS=cfg // 6, wrapT=(cfg // 2) % 3)
                kw["emissiveFactor"] = (0.5, 0.5, 0.5)
            if xforms[n % len(xforms)]:
                kw["uvTransform"] = uv_transform(**xforms[n % len(xforms)])
            m = sc.add_material(**kw)
            pm = sc.add_prim_mesh(quad(1.1 * (n % cols) - 2.75, 1.1 * (n // cols) - 2.2, 0.0, 0.5), [(0, 0, 1)] * 4, uv, [0, 1, 2, 0, 2, 3], m)
            sc.add_node(pm)
            n += 1
    img = alpha_image(gen)
    for k, (mode, cutoff, factor, xf) in enumerate(((MASK, 0.5, 1.0, None), (BLEND, 0.5, 1.5, None), (MASK, 0.5, 0.5 * 255 / 200, dict(rotation=0.3, offset=(0.5, 0.5))),
                                                    (BLEND, 0.5, 0.7, dict(scale=(-1.0, 1.0))), (MASK, 0.0, 0.7, None), (BLEND, 0.5, 255 / 200, dict(rotation=1.0)))):
        tid = sc.add_texture(img, magFilter=1 - k % 2 * (k > 3), wrapS=gen.REPEAT, wrapT=gen.REPEAT)
        kw = dict(alphaMode=mode, alphaCutoff=cutoff, pbrBaseColorFactor=(1.0, 1.0, 1.0, factor), pbrBaseColorTexture=tid, pbrMetallicFactor=0.0, doubleSided=1)
        if xf:
            kw["uvTransform"] = uv_transform(**xf)
        m = sc.add_material(**kw)
        pm = sc.add_prim_mesh(quad(2.0 * (k % 3) - 2.0, 2.2 * (k // 3) - 1.1, 0.6, 0.9), [(0, 0, 1)] * 4, [(0, 0), (1, 0), (1, 1), (0, 1)], [0, 1, 2, 0, 2, 3], m)
        sc.add_node(pm)
    sc.camera = Camera(eye=(0.3, 0.2, 7.5), center=(0.0, 0.0, 0.0), fov=50.0)
    return sc


@pytest.mark.gpu
def test_texture_chart_frames_equal_the_oracle(kat, gen):
    """one whole-frame check: every fixture texture on a quad, turned / shifted / flipped texture coordinates, MASK and BLEND cards with the adversarial
    alpha image: GPU == oracle bit for bit, flat and two-level, under the four storage settings"""
    from tests.common import Config, render_hip, render_oracle
    from vk_raytrace_amd import capi, synth
    cfg = Config(texture_chart(kat, gen), synth.procedural_sky(64, 32), 192, 160, depth=4)
    ref = render_oracle(cfg, 2)
    assert np.isfinite(ref).all() and ref[..., :3].std() > 0.01
    o = render_oracle(cfg, 1, return_obj=True)[1]
    assert o.stats()["texTaps"] > 20000 and o.stats()["alphaTests"] > 5000   # the chart is in view
    o.close()
    for tune in io.TUNES:
        for accel in (capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL):
            with io.tuned(tune):
                got = render_hip(cfg, 2, accel=accel)
            bad = np.count_nonzero((got.view(np.uint32) != ref.view(np.uint32)).any(-1))
            assert bad == 0, f"PT_TUNE={tune} accel={accel}: {bad} pixels differ from the oracle"
