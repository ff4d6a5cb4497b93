"""Shared by tests/test_trace_model.py and tests/test_trace_gpu.py: the fixture of tests/golden/gen_trace_kat.py, the rows of the trace probe
(vk_raytrace_amd/csrc/pt_probe.h trace_probe) and the assertions, written once so that the host build, the oracle and the device are held to the same ones.
Every probe -- th_trace_probe, orc_trace_probe, pt_debug_trace_probe -- takes (kind, n, in, in_stride, out, out_stride); integers travel as bit patterns.
The derivations behind the numbers used here (the T2 bound, the margins of the box tests, the order rule) are in the generator's docstring."""
import importlib.util
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_trace_kat", os.path.join(GOLDEN, "gen_trace_kat.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

TRP_TRI, TRP_WORLD_TRI, TRP_RAYBOX, TRP_NODE, TRP_CNODE, TRP_CN_PLANE, TRP_ENTER = range(7)
WORDS = {TRP_TRI: (16, 4), TRP_WORLD_TRI: (21, 9), TRP_RAYBOX: (6, 12), TRP_NODE: (36, 5), TRP_CNODE: (36, 6), TRP_CN_PLANE: (1, 2), TRP_ENTER: (20, 12)}
FILL = 0x4B3C614E  # what the caller puts into every output word: a probe that leaves a word alone leaves this
NONE, ALPHA = gen.BVH_NONE, gen.BVH_ALPHA
U = 2.0 ** -24


def load():
    with np.load(os.path.join(GOLDEN, "trace_kat.npz")) as z:
        return {k: z[k] for k in z.files}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def probe(fn, kind, rows, ctx=None):
    """rows (n, >= words of the kind) float32 through one call; returns (n, out words) float32, every word FILL beforehand, or None where that side answers -1"""
    rows = np.ascontiguousarray(rows, np.float32)
    assert rows.shape[1] >= WORDS[kind][0]
    out = np.full((len(rows), WORDS[kind][1]), FILL, np.uint32).view(np.float32)
    args = (kind, len(rows), rows.ctypes.data, rows.shape[1], out.ctypes.data, out.shape[1])
    if ctx is None:
        return None if fn(*args) == -1 else out
    rc = fn(ctx, *args)
    assert rc == 0, f"probe {kind} failed with {rc}"
    return out


def host_fn():
    from tests import host_harness
    return host_harness.lib().th_trace_probe


def orc_fn():
    from tests import orc
    return orc.lib().orc_trace_probe


def cn_plane_rows():
    """all 2048 grid integers, each in the low half of one word and in the high half of another (numpy's float16 makes the halves)"""
    i = np.arange(2048)
    h = i.astype(np.float16).view(np.uint16).astype(np.uint32)
    return (h | (h[::-1] << 16)).astype(np.uint32).view(np.float32).reshape(-1, 1)


def raybox_rows(kat):
    return np.concatenate([kat["node_in"][:, 28:34], kat["enter_ray"]])


def run_all(fn, kat, ctx=None, kinds=tuple(range(7))):
    """every row of every kind through one leg: name -> output"""
    sets = {"tri": (TRP_TRI, kat["tri_in"]), "tri_degenerate": (TRP_TRI, kat["tri_degenerate"]), "world_tri": (TRP_WORLD_TRI, kat["world_tri_in"]),
            "raybox": (TRP_RAYBOX, raybox_rows(kat)), "node": (TRP_NODE, kat["node_in"]), "node_degenerate": (TRP_NODE, kat["node_degenerate"]),
            "cnode": (TRP_CNODE, kat["node_in"]), "cnode_degenerate": (TRP_CNODE, kat["node_degenerate"]), "cn_plane": (TRP_CN_PLANE, cn_plane_rows()),
            "enter": (TRP_ENTER, kat["enter_in"])}
    return {name: probe(fn, kind, rows, ctx) for name, (kind, rows) in sets.items() if kind in kinds}


def same_bits(a, b):
    """the rule of tests/test_fpmath.py: NaN in the same places (payload free), every other value equal as bits; returns the number of differing values"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    an, bn = np.isnan(a), np.isnan(b)
    return int(np.count_nonzero(an != bn) + np.count_nonzero((a.view(np.uint32) != b.view(np.uint32)) & ~an & ~bn))


# ---- the fixture itself ----------------------------------------------------------------------------------------------------------------------------------
def check_fixture(kat):
    s, dec = kat["tri_set"], kat["tri_decided"]
    share = {name: 1.0 - dec[s == k].mean() for k, name in enumerate(gen.SETS)}
    print("undecided share per set:", {k: round(float(v), 4) for k, v in share.items()})
    assert share["interior"] <= 0.05 and share["sliver"] <= 0.50 and share["lattice"] == 0.0  # the caps that keep the test honest
    assert (s == 0).sum() >= 1000 and (s == 1).sum() >= 300 and (s == 2).sum() >= 300
    fl = u32(kat["tri_in"][:, 9])
    for f in (0, 2, 4, 6):  # every flag combination meets both windings: triangles of either facing, decided, on the flags set
        m = (s == 3) & (fl == f) & dec
        assert (kat["tri_detsign"][m] > 0).sum() >= 10 and (kat["tri_detsign"][m] < 0).sum() >= 10, f
    cats = np.bincount(kat["lattice_cat"], minlength=len(gen.LATTICE_CATEGORIES))
    assert (cats >= 20).all(), cats
    lat = kat["tri_in"][s == 4]
    assert np.abs(lat[:, :9]).max() <= 8 and (lat[:, :9] == np.round(lat[:, :9])).all()  # small-integer vertices
    dl = np.abs(lat[kat["lattice_cat"] <= 8][:, 13:16])
    assert np.isin(dl, (0.0, 0.25, 0.5, 1.0, 2.0, 4.0)).all()  # power-of-two direction components
    nd = kat["node_in"]
    words, d, lim = u32(nd[:, 24:28]), nd[:, 31:34], nd[:, 34]
    assert np.abs(nd[:, 28:31]).max() < 2 ** 20 and np.abs(nd[:, :24][np.abs(nd[:, :24]) < 1e38]).max() < 2 ** 20 and (np.abs(d).max(1) >= 0.5).all()
    assert ((words == NONE).sum(0) >= 100).all() and ((words != NONE) & (words & ALPHA != 0)).sum() >= 500 and ((words != NONE) & (words & ALPHA == 0)).sum() >= 500
    with np.errstate(over="ignore"):  # the empty slots
        ext = (nd[:, 12:24] - nd[:, 0:12]).reshape(-1, 3, 4)
    flat = ((ext == 0).sum(1))[words != NONE]
    assert (flat == 1).sum() >= 200 and (flat == 2).sum() >= 100 and (flat == 0).sum() >= 1000
    for v in (1e-30, -1e-20, 1e-10):
        assert (d == np.float32(v)).sum() >= 50, v
    assert ((d == 0) & ~np.signbit(d)).sum() >= 50 and ((d == 0) & np.signbit(d)).sum() >= 50
    assert (lim == 0).sum() >= 100 and (lim == np.float32(3e38)).sum() >= 500 and ((lim > 0) & (lim < 1e38)).sum() >= 100
    assert (u32(nd[:, 35]) == 1).sum() >= 200 and kat["node_must"].sum() >= 1000
    o = nd[:, 28:31, None]
    on_plane = ((o == nd[:, 0:12].reshape(-1, 3, 4)) | (o == nd[:, 12:24].reshape(-1, 3, 4))).any(2) & (np.abs(d) < 1e-9)
    assert on_plane.any(1).sum() >= 100  # rays that run exactly along a face plane


# ---- T1 --------------------------------------------------------------------------------------------------------------------------------------------------
def check_t1(out, kat, leg):
    bad = np.flatnonzero((u32(out) != u32(kat["world_tri_want"])).any(1))
    assert len(bad) == 0, f"{leg}: world_tri differs from the bit model on {len(bad)} rows, first {bad[0]}: {out[bad[0]]} want {kat['world_tri_want'][bad[0]]}"


# ---- T2 / T3 ---------------------------------------------------------------------------------------------------------------------------------------------
def check_t2(out, kat, leg):
    acc, tuv = u32(out[:, 0]), out[:, 1:4]
    assert np.isin(acc, (0, 1)).all()
    assert (u32(tuv)[acc == 0] == FILL).all(), f"{leg}: a rejected row's t, u, v were written"
    s, dec, ver, want, bound = kat["tri_set"], kat["tri_decided"], kat["tri_verdict"], kat["tri_want"], kat["tri_bound"].astype(np.float64)
    rnd = dec & (s != 4)
    bad = np.flatnonzero(rnd & ((acc == 1) != ver))
    assert len(bad) == 0, f"{leg}: verdict differs from the exact one on {len(bad)} decided rows, first {bad[0]} (set {gen.SETS[s[bad[0]]]})"
    # culling follows the sign of the exact det under every flag combination
    fl, sign = u32(kat["tri_in"][:, 9]), kat["tri_detsign"]
    front = np.where(fl & gen.TRI_FLIP != 0, sign < 0, sign > 0)
    culled = dec & (fl & gen.TRI_NOCULL == 0) & ~front
    assert culled.sum() >= 100 and (acc[culled] == 0).all(), f"{leg}: a back face was accepted"
    for f in (0, 2, 4, 6):
        m = dec & (s == 3) & (fl == f) & (front | (f & gen.TRI_NOCULL != 0))
        assert (acc[m] == ver[m]).all() and acc[m].sum() >= 20, f"{leg}: flags {f}"
    hit = rnd & (acc == 1)
    err = np.abs(tuv[hit].astype(np.float64) - want[hit])
    ratio = err / bound[hit]
    for k, name in enumerate("tuv"):
        print(f"{leg}: {name}: {hit.sum()} accepted decided rows, largest error / bound {ratio[:, k].max():.3f}")
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert (err <= bound[hit]).all(), f"{leg}: {'tuv'[worst[1]]} of row {np.flatnonzero(hit)[worst[0]]} is {ratio[worst]:.3g} x its derived bound"
    return float(ratio.max())


def check_lattice(out, kat, leg):
    m = kat["tri_set"] == 4
    acc, tuv, ver, want = u32(out[m, 0]), out[m, 1:4], kat["tri_verdict"][m], kat["tri_want"][m].astype(np.float32)
    names = np.array(gen.LATTICE_CATEGORIES)[kat["lattice_cat"]]
    bad = np.flatnonzero((acc == 1) != ver)
    assert len(bad) == 0, f"{leg}: exact lattice rows with the wrong verdict: {sorted(set(names[bad]))}"
    assert want.astype(np.float64).tolist() == kat["tri_want"][m].tolist()  # the exact values are fp32 numbers
    bad = np.flatnonzero(ver & (tuv != want).any(1))  # == : a zero of either sign is the exact zero
    assert len(bad) == 0, f"{leg}: exact lattice rows whose t, u, v are not the exact values: {sorted(set(names[bad]))}, first {tuv[bad[0]]} want {want[bad[0]]}"
    for cat in range(6):  # the vertices and the three edges are inside
        assert ver[(kat["lattice_cat"] == cat) & ((u32(kat["tri_in"][m, 9]) & gen.TRI_NOCULL) != 0)].all()
    assert not ver[kat["lattice_cat"] >= 9].any()  # det == 0 is a miss


# ---- node visits -----------------------------------------------------------------------------------------------------------------------------------------
def visit(out, rows, compact):
    """-> ok (n), seq: per row the children in the order reported (pushed ones, then the one returned), as child positions 0..3, or an error string"""
    w = u32(out)
    ok = w[:, 0] == 1 if compact else np.ones(len(w), bool)
    w = w[:, 1:] if compact else w
    words = u32(rows[:, 24:28])
    seqs, errors = [], []
    for i in range(len(w)):
        seq = []
        if ok[i]:
            nearest, npush = w[i, 0], w[i, 1]
            listed = ([] if npush == FILL else list(w[i, 2:2 + min(int(npush), 3)])) + ([] if nearest == NONE else [nearest])
            if nearest == FILL or npush > 3 or (nearest == NONE and npush != 0) or (w[i, 2 + min(int(npush), 3):] != FILL).any():
                errors.append(f"row {i}: malformed answer {w[i]}")
            for c in listed:
                k = np.flatnonzero(words[i] == c)
                if c == NONE or len(k) != 1:
                    errors.append(f"row {i}: reported {c:#x}, which is none of its children {words[i]}")
                else:
                    seq.append(int(k[0]))
            if len(set(seq)) != len(seq):
                errors.append(f"row {i}: a child reported twice")
        elif (w[i] != FILL).any():
            errors.append(f"row {i}: not encodable, yet written")
        seqs.append(seq)
    return ok, seqs, errors


def check_nodes(out, kat, compact, leg):
    """one-sided, tightness and order; returns (lost exact hits, reports outside the derived margin, order violations) as lists of strings"""
    rows = kat["node_in"]
    ok, seqs, errors = visit(out, rows, compact)
    assert not errors, f"{leg}: {errors[:3]}"
    assert ok.all(), f"{leg}: {np.count_nonzero(~ok)} nodes of the domain were not encodable"
    must, may = kat["node_must"], kat["node_may_c" if compact else "node_may"]
    e_hi, e_lo = kat["node_entry_hi"], kat["node_entry_lo_c" if compact else "node_entry_lo"]
    rep = np.zeros_like(must)
    for i, seq in enumerate(seqs):
        rep[i, seq] = True
    lost = [f"row {i} child {k}" for i, k in zip(*np.nonzero(must & ~rep))]
    loose = [f"row {i} child {k}" for i, k in zip(*np.nonzero(rep & ~may))]
    order = []
    for i, seq in enumerate(seqs):
        for a in range(len(seq)):
            for b in range(a + 1, len(seq)):
                if e_hi[i, seq[a]] < e_lo[i, seq[b]]:  # reported earlier = farther; here it is certainly nearer
                    order.append(f"row {i}: child {seq[a]} (entry <= {e_hi[i, seq[a]]}) before child {seq[b]} (entry >= {e_lo[i, seq[b]]})")
    print(f"{leg}: {int(must.sum())} exact hits, {int(rep.sum())} children reported, {int((rep & ~must).sum())} of them inside the margin only; "
          f"{sum(len(s) > 1 for s in seqs)} visits with an order to check")
    return lost, loose, order


def check_degenerate_nodes(out, kat, compact, leg):
    _, _, errors = visit(out, kat["node_degenerate"], compact)
    assert not errors, f"{leg}: {errors[:3]}"


# ---- cn_plane, make_raybox, enter_instance ---------------------------------------------------------------------------------------------------------------
def check_cn_plane(out, leg):
    i = np.arange(2048, dtype=np.float32)
    assert u32(out[:, 0]).tolist() == u32(i).tolist() and u32(out[:, 1]).tolist() == u32(i[::-1]).tolist(), f"{leg}: a grid integer does not decode to itself"


def check_raybox(out, rows, leg):
    """the promise of make_raybox's comment, exactly (a product of two fp32 numbers is exact in float64): nlo <= -(o idir) <= nhi, idir = fl(1 / d) with |d|
    raised to 1e-18, near planes picked by the sign of d (of -0.0 too)"""
    o, d = rows[:, 0:3].astype(np.float64), rows[:, 3:6]
    idir, nlo, nhi, off = out[:, 0:3].astype(np.float64), out[:, 3:6].astype(np.float64), out[:, 6:9].astype(np.float64), u32(out[:, 9:12])
    dc = np.copysign(np.maximum(np.abs(d), np.float32(1e-18)), d).astype(np.float64)
    assert (np.abs(idir * dc - 1.0) <= U).all(), f"{leg}: idir is not the rounded reciprocal"
    assert (off == np.where(np.signbit(d), 48, 0)).all(), f"{leg}: near-plane offsets"
    x = -(o * idir)
    assert (nlo <= x).all() and (x <= nhi).all(), f"{leg}: n is biased the wrong way"
    beta = np.abs(x) * 2.0 ** -21 * 1.26 + 1e-43
    assert (np.abs(nlo - x) <= beta).all() and (np.abs(nhi - x) <= beta).all(), f"{leg}: the bias is larger than BETA |o idir|"


def check_enter(out, raybox_of_ray, kat, leg):
    """enter_instance == make_raybox of the transformed ray (the bit model's, through the same leg's TRP_RAYBOX), widened by eps |idir|: within the fp32
    rounding of fl(fl(padC1 max|o|) + padC0), of its product with |idir| (3 u in all) and of the final sum (u |result|)"""
    rb = raybox_of_ray.astype(np.float64)
    got = out.astype(np.float64)
    assert same_bits(out[:, 0:3], raybox_of_ray[:, 0:3]) == 0 and (u32(out[:, 9:12]) == u32(raybox_of_ray[:, 9:12])).all(), f"{leg}: idir / near planes of the transformed ray"
    g = kat["enter_eps"][:, None] * np.abs(rb[:, 0:3])
    for name, lo, sign in (("nlo", 3, -1.0), ("nhi", 6, 1.0)):
        want = rb[:, lo:lo + 3] + sign * g
        tol = U * (3.0 * g + np.abs(want)) * (1.0 + 1e-6) + 1e-45
        err = np.abs(got[:, lo:lo + 3] - want)
        assert (err <= tol).all(), f"{leg}: {name} of row {np.argmax((err / tol).max(1))} is {(err / tol).max():.3g} x the rounding of its expression"
    assert (g > 0).all()
