"""Node-by-node audit of a built acceleration structure, in numpy on the host.  A plain module: no test lives here.

audit(dump, scene_inputs) judges the arrays a build left behind -- the device's through pt_debug_accel_read, the host harness's through
th_accel_read (ids and info record: vk_raytrace_amd/csrc/pt_accel_dump.h) -- against the formats of csrc/pt_device.h and the contracts of DESIGN.md
("What the build guarantees").  It never runs a builder: what a box, a record or a table must hold is restated here from the scene's vertices,
indices and instance records.  Comparisons are exact (bit patterns, or float64 values of float32 numbers where an order is needed); the one stated
tolerance is the leaf padding, which may be rounded separately or fused.

report: check name -> int64 array of offenders, one row (hierarchy, node or slot or instance, child slot or -1) each; "_facts" holds what the audit
observed without judging it (padding form, arrays that were absent and therefore not checked).  Hierarchy numbers: 0 flat, 1 merged, 2 TLAS,
3 + k the k-th range of BLAS_RANGES; -1 for tables."""
import ctypes as C

import numpy as np

U, F = np.uint32, np.float32
IDS = ["WIDE", "CNODES", "TRIS", "ALPHA_RECS", "BVH2", "TLAS", "CTLAS", "TLAS_LEAVES", "INST_TRI_BASE", "INST_BLOCK", "INST_NODE_BASE", "INST_PAD", "ACTIVE",
       "BLAS_RANGES", "MERGED_LIST", "SHADE_TRIS"]
WORDS = {"WIDE": 32, "CNODES": 20, "TRIS": 12, "ALPHA_RECS": 8, "BVH2": 16, "TLAS": 32, "CTLAS": 20, "TLAS_LEAVES": 8, "INST_PAD": 2, "BLAS_RANGES": 2, "SHADE_TRIS": 32}
INFO = ["accelMode", "numTris", "numInstances", "numWideNodes", "nodeCapacity", "numBvhNodes", "numTlasNodes", "numActive", "numBlas", "mergedTris", "mergedWide",
        "mergedOnly", "haveCNodes", "haveShadeTris", "mbox0", "mbox1", "mbox2", "mbox3", "mbox4", "mbox5", "builder"]
BVH_LEAF, BVH_ALPHA, BVH_SLOT_MASK, BVH_NONE = 0x80000000, 0x40000000, 0x3FFFFFFF, 0xFFFFFFFF
TRI_OPAQUE, TRI_INDEX_MASK = 1, 0x1FFFFFFF
PT_INST_MERGED, PT_INST_BLOCK_SHIFT = 0xFFFFFFFE, 8
CN_GRID_MAX = 2047
FLT_MAX_BITS, NEG_FLT_MAX_BITS = 0x7F7FFFFF, 0xFF7FFFFF
H_FLAT, H_MERGED, H_TLAS, H_BLAS0 = 0, 1, 2, 3

INSTANCE_DTYPE = np.dtype([("objectToWorld", F, (3, 4)), ("worldToObject", F, (3, 4)), ("vertexOffset", U), ("firstIndex", U), ("materialIndex", np.int32), ("primMesh", np.int32),
                           ("triBase", U), ("triCount", U), ("flags", U), ("_pad", U)])
assert INSTANCE_DTYPE.itemsize == 128

# every check audit() can report; tests/test_accel_audit.py refuses a name without a planted defect that lights it
CHECKS = ["ref_range", "node_reach", "node_count", "node_arity", "empty_slot", "slot_order", "leaf_permutation", "tri_record", "tri_world_index", "alpha_rec", "leaf_alpha_tag",
          "inner_alpha_tag", "leaf_box", "inner_box", "cnode_child", "cnode_origin", "cnode_exponent", "cnode_plane", "cnode_enclose", "cnode_tight", "cnode_empty",
          "tlas_leaf_set", "tlas_leaf_node_base", "tlas_leaf_fields", "tlas_leaf_pad", "merged_box", "merged_list", "inst_tri_base", "inst_block", "blas_ranges",
          "active_list", "inst_pad", "bvh2_root", "shade_tris_ids"]


# ---- reading a dump ------------------------------------------------------------------------------------------------------------------------------
def read_dump(info_fn, read_fn):
    """info_fn(out_ptr, words) -> words; read_fn(which, dst_ptr, bytes) -> bytes held (negative: error).  -> {"info": {...}, id: (n, words) uint32 | None}"""
    raw = np.zeros(len(INFO), U)
    got = info_fn(raw.ctypes.data, len(raw))
    assert got == len(INFO), f"info record: {got} words, expected {len(INFO)}"
    dump = {"info": {k: int(v) for k, v in zip(INFO, raw)}}
    dump["info"]["mergedBox"] = raw[14:20].copy().view(F)
    for which, name in enumerate(IDS):
        have = read_fn(which, None, 0)
        assert have >= 0 or have == -1, (name, have)
        if have == 0:
            dump[name] = None
            continue
        # a null / short buffer must copy nothing and report PT_ERR_INVALID (-1); the size comes from a buffer that is certainly large enough
        buf = np.zeros(1 << 16, U)
        have = read_fn(which, buf.ctypes.data, buf.nbytes)
        while have == -1:
            buf = np.zeros(len(buf) * 8, U)
            have = read_fn(which, buf.ctypes.data, buf.nbytes)
        assert have > 0 and have % 4 == 0, (name, have)
        a = buf[:have // 4].copy()
        w = WORDS.get(name, 1)
        assert len(a) % w == 0, (name, have)
        dump[name] = a.reshape(-1, w) if w > 1 else a
    return dump


def device_dump(renderer):
    L, ctx = renderer._lib, renderer._ctx
    return read_dump(lambda out, n: L.pt_debug_accel_info(ctx, out, n), lambda which, dst, nbytes: L.pt_debug_accel_read(ctx, which, dst, nbytes))


def harness_dump(traced, two):
    L, h = traced.L, traced.h
    return read_dump(lambda out, n: L.th_accel_info(h, int(two), out, n), lambda which, dst, nbytes: L.th_accel_read(h, int(two), which, dst, nbytes))


def scene_inputs(scene, any_hit=True, merge_singles=True):
    """vertices, indices, the instance records as the kernels see them (pt_debug_scene_records + the useAnyHit override of effective_instances) and the
    per-instance object-space padding (pt_debug_two_level_pad's rule through the same entry)"""
    from vk_raytrace_amd import capi
    L = capi.lib()
    L.pt_debug_scene_records.restype = C.c_int
    L.pt_debug_scene_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    if scene.vertices is None:
        scene.finalize(capi.pack_vertices)
    d, keep = scene.desc()
    counts = (C.c_ulonglong * 5)()
    err = C.create_string_buffer(256)
    assert L.pt_debug_scene_records(C.byref(d), counts, None, None, None, None, None, None, err, 256) == 0, err.value
    inst = np.zeros(max(1, counts[0]), INSTANCE_DTYPE)
    pad = np.zeros(2 * counts[0] + 2, F)
    assert L.pt_debug_scene_records(C.byref(d), counts, inst.ctypes.data, pad.ctypes.data, None, None, None, None, err, 256) == 0, err.value
    inst = inst[:counts[0]]
    if not any_hit:
        inst["flags"] |= TRI_OPAQUE
    v = np.ascontiguousarray(scene.vertices)
    return {"vertices": v.view(F).reshape(len(v), 8).copy(), "indices": np.ascontiguousarray(scene.indices, U).copy(), "inst": inst, "pad": pad[:2 * counts[0]].reshape(-1, 2).copy(),
            "merge_singles": bool(merge_singles)}


# ---- float helpers -------------------------------------------------------------------------------------------------------------------------------
def _f(a):
    return np.ascontiguousarray(a, U).view(F)


def _u(a):
    return np.ascontiguousarray(a, F).view(U)


def _ordered(a):
    """float32 -> int64 whose order is the floats' and whose differences count ulps"""
    i = _u(a).astype(np.int64)
    return np.where(i & 0x80000000, -(i & 0x7FFFFFFF), i)


def padded_box(p0, e1, e2):
    """the padded box of a record (p0, p0 + e1, p0 + e2), float32 (n, 3) each: bounds of the three fp32 points grown by m * 4e-6f + 1e-30f, m the largest
    coordinate magnitude of the axis.  -> lo, hi (the unpadded fp32 bounds) and the padded bounds with the padding rounded separately / fused"""
    p0, e1, e2 = (np.asarray(x, F) for x in (p0, e1, e2))
    p1, p2 = p0 + e1, p0 + e2
    lo, hi = np.minimum(p0, np.minimum(p1, p2)), np.maximum(p0, np.maximum(p1, p2))
    m = np.maximum(np.abs(lo), np.abs(hi))
    pad_sep = (m * F(4e-6)) + F(1e-30)
    pad_fus = (m.astype(np.float64) * np.float64(F(4e-6)) + np.float64(F(1e-30))).astype(F)  # the product of two float32 is exact in float64
    return lo, hi, m, (lo - pad_sep, hi + pad_sep), (lo - pad_fus, hi + pad_fus)


def xform_point(rows, p):
    """pt_math.h xform_point in float32, one rounding per operation: ((r.x * x + r.y * y) + r.z * z) + r.w.  rows (n, 3, 4), p (n, 3)"""
    rows, p = np.asarray(rows, F), np.asarray(p, F)
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    return ((rows[:, :, 0] * x + rows[:, :, 1] * y) + rows[:, :, 2] * z) + rows[:, :, 3]


def _positions(S, ii, kk):
    """object-space positions (n, 3, 3) of primitive kk of instance ii, and the vertex ids (n, 3)"""
    I = S["inst"]
    vid = np.stack([S["indices"][I["firstIndex"][ii].astype(np.int64) + 3 * kk.astype(np.int64) + j].astype(np.int64) + I["vertexOffset"][ii] for j in range(3)], 1)
    return S["vertices"][vid][:, :, 0:3], vid


def world_records(S, ii, kk):
    """trace contract T1: the world record (p0, e1, e2) of primitive kk of instance ii, float32"""
    pos, _ = _positions(S, ii, kk)
    rows = S["inst"]["objectToWorld"][ii]
    p = [xform_point(rows, pos[:, j]) for j in range(3)]
    return p[0], p[1] - p[0], p[2] - p[0]


# ---- one hierarchy -------------------------------------------------------------------------------------------------------------------------------
class _Hier:
    """what the audit needs to know about one hierarchy: wide nodes, root, the nodes and leaf slots it must occupy, the compact form"""

    def __init__(self, hid, W, root, nodes, slot0, nslots, count, C=None):
        self.hid, self.W, self.root, self.nodes, self.slot0, self.nslots, self.count, self.C = hid, W, root, nodes, slot0, nslots, count, C


def _rows(hid, a, b=None):
    a = np.asarray(a, np.int64).reshape(-1)
    b = np.full(len(a), -1, np.int64) if b is None else np.asarray(b, np.int64).reshape(-1)
    return np.stack([np.full(len(a), hid, np.int64), a, b], 1)


class _Report(dict):
    def add(self, name, rows):
        assert name in CHECKS, name
        if len(rows):
            self[name] = np.concatenate([self[name], rows]) if name in self else rows


def _walk(h, rep):
    """level by level from the root: every node expanded once.  -> levels (list of node arrays), leaf references (node, k, ref)"""
    W, N = h.W, len(h.W)
    child = W[:, 24:28]
    reached = np.zeros(N, np.int64)
    levels, leaves = [], []
    if h.root >= N:
        rep.add("ref_range", _rows(h.hid, [h.root]))
        return levels, np.zeros((0, 3), np.int64), reached
    frontier = np.array([h.root], np.int64)
    while len(frontier):
        uniq, cnt = np.unique(frontier, return_counts=True)
        fresh = uniq[reached[uniq] == 0]
        reached[uniq] += cnt
        if len(fresh) == 0:
            break
        levels.append(fresh)
        ref = child[fresh]
        used = ref != BVH_NONE
        leaf = used & ((ref & BVH_LEAF) != 0)
        inner = used & ~leaf
        idx = (ref & BVH_SLOT_MASK).astype(np.int64)
        bad = inner & (idx >= N)
        nn, kk = np.nonzero(bad)
        rep.add("ref_range", _rows(h.hid, fresh[nn], kk))
        nn, kk = np.nonzero(leaf)
        leaves.append(np.stack([fresh[nn], kk, ref[nn, kk].astype(np.int64)], 1))
        frontier = idx[inner & ~bad]
    return levels, (np.concatenate(leaves) if leaves else np.zeros((0, 3), np.int64)), reached


def _boxes(W):
    """(n, 4, 3) lower and upper corners of the child boxes"""
    f = _f(W[:, 0:24]).reshape(-1, 6, 4)
    return np.transpose(f[:, 0:3], (0, 2, 1)), np.transpose(f[:, 3:6], (0, 2, 1))


def _audit_shape(h, rep, facts):
    """reachability, shape, inner boxes and tags.  -> (slot -> (node, k) of its one leaf reference, or -1), reached node ids"""
    levels, leaves, reached = _walk(h, rep)
    W = h.W
    nodes = np.concatenate(levels) if levels else np.zeros(0, np.int64)
    # reached exactly once, and exactly the nodes the hierarchy owns
    rep.add("node_reach", _rows(h.hid, np.nonzero(reached > 1)[0]))
    if h.nodes is not None:
        own = np.zeros(len(W), bool)
        own[h.nodes[(h.nodes >= 0) & (h.nodes < len(W))]] = True
        rep.add("node_reach", _rows(h.hid, np.nonzero(own != (reached > 0))[0]))
    if len(nodes) != h.count:
        rep.add("node_count", _rows(h.hid, [h.root], [len(nodes)]))
    child = W[nodes, 24:28]
    used = child != BVH_NONE
    lo, hi = _boxes(W[nodes])
    # empty slots: BVH_NONE with the inverted box, after the used ones
    inv = (_u(lo) == FLT_MAX_BITS).all(2) & (_u(hi) == NEG_FLT_MAX_BITS).all(2)
    nn, kk = np.nonzero(~used & ~inv)
    rep.add("empty_slot", _rows(h.hid, nodes[nn], kk))
    nn, kk = np.nonzero(used[:, 1:] & ~used[:, :-1])
    rep.add("slot_order", _rows(h.hid, nodes[nn], kk + 1))
    nused = used.sum(1)
    single = h.nslots == 1
    rep.add("node_arity", _rows(h.hid, nodes[(nused != 1) if single else (nused < 2)]))
    # leaf slots: a permutation of the hierarchy's slot range
    slot = (leaves[:, 2] & BVH_SLOT_MASK) - h.slot0
    inr = (slot >= 0) & (slot < h.nslots)
    rep.add("ref_range", _rows(h.hid, leaves[~inr, 0], leaves[~inr, 1]))
    times = np.bincount(slot[inr], minlength=h.nslots)
    rep.add("leaf_permutation", _rows(h.hid, np.nonzero(times != 1)[0] + h.slot0))
    where = np.full((h.nslots, 2), -1, np.int64)
    where[slot[inr]] = leaves[inr, 0:2]
    # inner references bottom-up: box = union of the leaf reference boxes below, tag = some leaf below carries it
    N = len(W)
    ulo, uhi, ual = np.full((N, 3), np.inf), np.full((N, 3), -np.inf), np.zeros(N, bool)
    allc, (alo, ahi) = W[:, 24:28], _boxes(W)
    for lv in reversed(levels):
        c = allc[lv]
        u = c != BVH_NONE
        isleaf = u & ((c & BVH_LEAF) != 0)
        idx = np.where(u & ~isleaf, c & BVH_SLOT_MASK, 0).astype(np.int64)
        idx = np.where(idx < N, idx, 0)
        inn = u & ~isleaf & ((c & BVH_SLOT_MASK) < N)
        blo = np.where(isleaf[:, :, None], alo[lv].astype(np.float64), np.where(inn[:, :, None], ulo[idx], np.inf))
        bhi = np.where(isleaf[:, :, None], ahi[lv].astype(np.float64), np.where(inn[:, :, None], uhi[idx], -np.inf))
        bal = np.where(isleaf, (c & BVH_ALPHA) != 0, inn & ual[idx])
        ulo[lv], uhi[lv], ual[lv] = blo.min(1), bhi.max(1), bal.any(1)
        bad = inn & ~((alo[lv] == ulo[idx]).all(2) & (ahi[lv] == uhi[idx]).all(2))
        nn, kk = np.nonzero(bad)
        rep.add("inner_box", _rows(h.hid, lv[nn], kk))
        nn, kk = np.nonzero(inn & (((c & BVH_ALPHA) != 0) != ual[idx]))
        rep.add("inner_alpha_tag", _rows(h.hid, lv[nn], kk))
    root_box = (ulo[h.root], uhi[h.root]) if h.root < N else None
    if h.C is not None:
        _audit_compact(h, nodes, rep)
    return where, nodes, root_box


def _audit_leaves(h, rep, facts, where, valid, p0, e1, e2, opaque, extra=None):
    """leaf reference boxes and tags of the slots whose triangle is known (valid): p0, e1, e2 the record the box is built from; extra: points the box must
    enclose besides (n, k, 3)"""
    ok = valid & (where[:, 0] >= 0)
    s = np.nonzero(ok)[0]
    if len(s) == 0:
        return
    node, k = where[s, 0], where[s, 1]
    f = _f(h.W[node, 0:24]).reshape(-1, 6, 4)
    blo, bhi = f[np.arange(len(s)), 0:3, k], f[np.arange(len(s)), 3:6, k]
    lo, hi, m, (slo, shi), (flo, fhi) = padded_box(p0[s], e1[s], e2[s])
    if extra is not None:
        lo, hi = np.minimum(lo, extra[s].min(1)), np.maximum(hi, extra[s].max(1))
    lo64, hi64, blo64, bhi64 = (x.astype(np.float64) for x in (lo, hi, blo, bhi))
    encl = np.where(m > 0, (blo64 < lo64) & (bhi64 > hi64), (blo64 <= lo64) & (bhi64 >= hi64))
    near = lambda a, b: np.abs(_ordered(a) - _ordered(b)) <= 1
    sep, fus = near(blo, slo) & near(bhi, shi), near(blo, flo) & near(bhi, fhi)
    bad = ~(encl & (sep | fus)).all(1)
    rep.add("leaf_box", _rows(h.hid, node[bad], k[bad]))
    differ = (_u(slo) != _u(flo)) | (_u(shi) != _u(fhi))
    facts["pad_separate"] += int((differ & (_u(blo) == _u(slo)) & (_u(bhi) == _u(shi))).sum())
    facts["pad_fused"] += int((differ & (_u(blo) == _u(flo)) & (_u(bhi) == _u(fhi))).sum())
    facts["pad_exact"] += int(((_u(blo) == _u(slo)) & (_u(bhi) == _u(shi))).sum())
    facts["pad_planes"] += int(differ.size)
    tag = (h.W[node, 24 + k] & BVH_ALPHA) != 0
    bad = tag != ~opaque[s]
    rep.add("leaf_alpha_tag", _rows(h.hid, node[bad], k[bad]))


def _audit_compact(h, nodes, rep):
    W, Cn = h.W, h.C
    inr = nodes < len(Cn)
    rep.add("cnode_child", _rows(h.hid, nodes[~inr]))
    nodes = nodes[inr]
    if len(nodes) == 0:
        return
    w, c = W[nodes], Cn[nodes]
    child = w[:, 24:28]
    used = child != BVH_NONE
    rep.add("cnode_child", _rows(h.hid, nodes[(c[:, 16:20] != child).any(1)]))
    lo, hi = _boxes(w)                                       # (n, 4, 3)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    mn = np.where(used[:, :, None], lo64, np.inf).min(1)     # (n, 3)
    mx = np.where(used[:, :, None], hi64, -np.inf).max(1)
    p = _f(c[:, 0:3]).astype(np.float64)
    some = used.any(1)
    rep.add("cnode_origin", _rows(h.hid, nodes[some & (p != mn).any(1)]))
    e = np.stack([(c[:, 3] >> (8 * a)) & 0xFF for a in range(3)], 1).astype(np.int64)
    ext = np.where(some[:, None], mx - mn, 0.0)
    with np.errstate(invalid="ignore"):
        mant, ex = np.frexp(ext)                             # ext = mant * 2^ex, mant in [0.5, 1): 2047 * 2^k >= ext iff k >= ex - 11 (mant <= 2047/2048) or ex - 10
    k = np.where(mant <= 2047.0 / 2048.0, ex - 11, ex - 10)
    want = np.where(ext > 0, np.maximum(27, k + 127), 27)
    rep.add("cnode_exponent", _rows(h.hid, nodes[(e != want).any(1)]))
    step = np.ldexp(1.0, (e - 127).astype(np.int64))         # (n, 3)
    planes = c[:, 4:16].reshape(-1, 3, 4)                    # per axis: lo0|lo1, lo2|lo3, hi0|hi1, hi2|hi3
    half = np.stack([planes & 0xFFFF, planes >> 16], 3).reshape(-1, 3, 8).astype(np.uint16)   # per axis lo0..lo3, hi0..hi3
    q = half.view(np.float16).astype(np.float64)
    isint = np.isfinite(q) & (q == np.floor(np.where(np.isfinite(q), q, 0))) & (q >= 0) & (q <= CN_GRID_MAX)
    rep.add("cnode_plane", _rows(h.hid, nodes[~isint.all((1, 2))]))
    q = np.where(isint, q, 0.0)
    ql, qh = np.transpose(q[:, :, 0:4], (0, 2, 1)), np.transpose(q[:, :, 4:8], (0, 2, 1))   # (n, 4, 3)
    # float64 holds p + q * step exactly unless p is tiny against the step (its last bit then lies more than 53 bits below the step's first): those
    # nodes, and every node float64 finds at fault, are judged again in rational arithmetic
    P, St = p[:, None, :], step[:, None, :]
    u3 = used[:, :, None]
    out = u3 & ((P + ql * St > lo64) | (P + qh * St < hi64))
    with np.errstate(invalid="ignore"):
        loose = u3 & ((lo64 >= P + (ql + 1) * St) | (P + (qh - 1) * St >= hi64))
    inexact = ((p != 0) & (np.abs(p) < step * 2.0 ** -18)).any(1)
    bad_out, bad_loose = out.any((1, 2)), loose.any((1, 2))
    from fractions import Fraction as Q
    for n in np.nonzero(inexact | bad_out | bad_loose)[0]:
        bad_out[n] = bad_loose[n] = False
        for a in range(3):
            pa, sa = Q(float(p[n, a])), Q(float(step[n, a]))
            for k in np.nonzero(used[n])[0]:
                l, hgh, a0, a1 = Q(float(lo64[n, k, a])), Q(float(hi64[n, k, a])), int(ql[n, k, a]), int(qh[n, k, a])
                bad_out[n] |= pa + a0 * sa > l or pa + a1 * sa < hgh
                bad_loose[n] |= l >= pa + (a0 + 1) * sa or pa + (a1 - 1) * sa >= hgh
    rep.add("cnode_enclose", _rows(h.hid, nodes[bad_out]))
    rep.add("cnode_tight", _rows(h.hid, nodes[bad_loose]))
    rep.add("cnode_empty", _rows(h.hid, nodes[(~u3 & ((ql != 0) | (qh != 0))).any((1, 2))]))


# ---- the records of the leaves -------------------------------------------------------------------------------------------------------------------
def _audit_world_leaves(h, rep, facts, where, dump, S, insts):
    """flat / merged structure: every TriRec is the T1 world record of its (instance, primitive); insts: the instances the hierarchy holds"""
    I = S["inst"]
    T = dump["TRIS"][h.slot0:h.slot0 + h.nslots]
    slots = np.arange(len(T)) + h.slot0
    ii, kk = T[:, 7].astype(np.int64), T[:, 11].astype(np.int64)
    member = np.zeros(len(I) + 1, bool)
    member[insts] = True
    valid = (ii < len(I)) & member[np.minimum(ii, len(I))]
    valid &= kk < np.where(valid, I["triCount"][np.minimum(ii, len(I) - 1)], 0)
    rep.add("tri_record", _rows(h.hid, slots[~valid]))
    iv, kv = np.where(valid, ii, insts[0]), np.where(valid, kk, 0)
    p0, e1, e2 = world_records(S, iv, kv)
    want = np.zeros((len(T), 12), U)
    want[:, 0:3], want[:, 4:7], want[:, 8:11] = _u(p0), _u(e1), _u(e2)
    want[:, 3] = (I["triBase"][iv] + kv).astype(U) | (I["flags"][iv] << 29)
    want[:, 7], want[:, 11] = iv, kv
    rest = [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11]
    rep.add("tri_record", _rows(h.hid, slots[valid & (T[:, rest] != want[:, rest]).any(1)]))
    # world indices: p0w.w of every record, and as a set the world triangles of the hierarchy's instances, each once
    rep.add("tri_world_index", _rows(h.hid, slots[valid & (T[:, 3] != want[:, 3])]))
    expect = np.concatenate([I["triBase"][i] + np.arange(I["triCount"][i], dtype=np.int64) for i in insts]) if len(insts) else np.zeros(0, np.int64)
    got = (T[:, 3] & TRI_INDEX_MASK).astype(np.int64)
    uniq, cnt = np.unique(got, return_counts=True)
    dup = np.isin(got, uniq[cnt > 1]) | ~np.isin(got, expect)
    rep.add("tri_world_index", _rows(h.hid, slots[dup]))
    opaque = (I["flags"][iv] & TRI_OPAQUE) != 0
    _audit_alpha_recs(h, rep, dump, S, slots, valid, iv, kv)
    _audit_leaves(h, rep, facts, where, valid, p0, e1, e2, opaque)
    if dump.get("SHADE_TRIS") is not None and len(dump["SHADE_TRIS"]) >= h.slot0 + len(T):
        last = dump["SHADE_TRIS"][h.slot0:h.slot0 + len(T), 24:28]   # the quad after the six attribute quads: (instance, primitive, ...)
        rep.add("shade_tris_ids", _rows(h.hid, slots[(last[:, 0] != T[:, 7]) | (last[:, 1] != T[:, 11])]))


def _audit_alpha_recs(h, rep, dump, S, slots, valid, iv, kv):
    A = dump.get("ALPHA_RECS")
    if A is None or len(A) < h.slot0 + h.nslots:
        rep.add("alpha_rec", _rows(h.hid, slots))
        return
    A = A[h.slot0:h.slot0 + h.nslots]
    _, vid = _positions(S, iv, kv)
    want = np.zeros((len(A), 8), U)
    want[:, 0:6] = _u(S["vertices"][vid][:, :, 4:6].reshape(-1, 6))
    want[:, 6] = np.maximum(S["inst"]["materialIndex"][iv], 0).astype(U)
    rep.add("alpha_rec", _rows(h.hid, slots[valid & (A != want).any(1)]))


def _audit_blas_leaves(h, rep, facts, where, dump, S, inst):
    """object-space BLAS of instance inst's prim-mesh: the three vertex positions as the vertex buffer holds them, p0w.w = primitive, the other w lanes 0.
    -> number of slots that do not hold the mesh's triangle"""
    I = S["inst"]
    T = dump["TRIS"][h.slot0:h.slot0 + h.nslots]
    slots = np.arange(len(T)) + h.slot0
    kk = T[:, 3].astype(np.int64)
    valid = kk < I["triCount"][inst]
    kv = np.where(valid, kk, 0)
    iv = np.full(len(T), inst, np.int64)
    pos, _ = _positions(S, iv, kv)
    want = np.zeros((len(T), 12), U)
    want[:, 0:3], want[:, 4:7], want[:, 8:11] = _u(pos[:, 0]), _u(pos[:, 1]), _u(pos[:, 2])
    want[:, 3] = kv
    bad = ~valid | (T != want).any(1)
    rep.add("tri_record", _rows(h.hid, slots[bad]))
    _audit_alpha_recs(h, rep, dump, S, slots, valid, iv, kv)
    opaque = np.full(len(T), (I["flags"][inst] & TRI_OPAQUE) != 0)
    # the box is built from the edge form of the record under the identity transform: p0 = v0, e = fl(v - v0)
    _audit_leaves(h, rep, facts, where, valid, pos[:, 0], pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0], opaque)
    return int(bad.sum())


# ---- the audit -----------------------------------------------------------------------------------------------------------------------------------
def _hierarchies(dump):
    """the hierarchies of a dump by name: what cost() and audit() walk"""
    info, out = dump["info"], {}
    W = dump["WIDE"]
    cn = dump.get("CNODES") if info["haveCNodes"] else None
    if info["accelMode"] == 0:
        if W is not None and info["numTris"]:
            out["flat"] = _Hier(H_FLAT, W, 0, np.arange(info["numWideNodes"]), 0, info["numTris"], info["numWideNodes"], cn)
        return out
    if info["mergedTris"] and W is not None:
        out["merged"] = _Hier(H_MERGED, W, 0, np.arange(info["mergedWide"]), 0, info["mergedTris"], info["mergedWide"], cn)
    R = dump.get("BLAS_RANGES")
    if R is not None and W is not None:
        for k, (base, num) in enumerate(R.astype(np.int64)):
            out[f"blas{k}"] = _Hier(H_BLAS0 + k, W, int(base), np.arange(base, base + num), None, None, int(num), None if info["mergedOnly"] else cn)
    if dump.get("TLAS") is not None and dump.get("TLAS_LEAVES") is not None:
        out["tlas"] = _Hier(H_TLAS, dump["TLAS"], 0, np.arange(info["numTlasNodes"]), 0, len(dump["TLAS_LEAVES"]), info["numTlasNodes"], dump.get("CTLAS") if info["haveCNodes"] else None)
    return out


def _blas_slots(h):
    """a BLAS's slot range is what its leaves reference: [smallest, smallest + number of leaf references)"""
    levels, leaves, _ = _walk(h, _Report())
    if len(leaves) == 0:
        return 0, 0
    s = leaves[:, 2] & BVH_SLOT_MASK
    return int(s.min()), len(s)


def cost(dump):
    """per hierarchy: the float64 sum of dx dy + dy dz + dz dx over the used child boxes of its reached nodes"""
    out = {}
    for name, h in _hierarchies(dump).items():
        levels, _, _ = _walk(h, _Report())
        nodes = np.concatenate(levels) if levels else np.zeros(0, np.int64)
        lo, hi = _boxes(h.W[nodes])
        d = hi.astype(np.float64) - lo.astype(np.float64)
        used = h.W[nodes, 24:28] != BVH_NONE
        out[name] = float(np.where(used, d[:, :, 0] * d[:, :, 1] + d[:, :, 1] * d[:, :, 2] + d[:, :, 2] * d[:, :, 0], 0.0).sum())
    return out


def audit(dump, S):
    rep = _Report()
    facts = {"pad_separate": 0, "pad_fused": 0, "pad_exact": 0, "pad_planes": 0, "not_checked": [n for n in IDS if dump.get(n) is None]}
    rep["_facts"] = facts
    info, I = dump["info"], S["inst"]
    hier = _hierarchies(dump)
    if info["accelMode"] == 0:
        if "flat" in hier:
            h = hier["flat"]
            where, nodes, root_box = _audit_shape(h, rep, facts)
            _audit_world_leaves(h, rep, facts, where, dump, S, np.nonzero(I["triCount"] > 0)[0])
            B = dump.get("BVH2")
            if B is not None and info["numTris"] > 1:
                lo, hi = _boxes(h.W[0:1])
                used = h.W[0, 24:28] != BVH_NONE
                root_box = lo[0][used].astype(np.float64).min(0), hi[0][used].astype(np.float64).max(0)
                b = _f(B[0, 0:12]).astype(np.float64)   # lmin.xyz lmax.xyz rmin.xyz rmax.xyz
                two = B[0, 13] != BVH_NONE
                lo = np.minimum(b[0:3], b[6:9]) if two else b[0:3]
                hi = np.maximum(b[3:6], b[9:12]) if two else b[3:6]
                if not ((lo == root_box[0]).all() and (hi == root_box[1]).all()):
                    rep.add("bvh2_root", _rows(H_FLAT, [0]))
        return rep
    _audit_two_level(dump, S, hier, rep, facts)
    return rep


def _audit_two_level(dump, S, hier, rep, facts):
    info, I = dump["info"], S["inst"]
    ninst = len(I)
    has = I["triCount"] > 0
    # which instances are merged: the prim-meshes instantiated once, when the build merges them
    uses = np.bincount(I["primMesh"][has], minlength=int(I["primMesh"].max(initial=0)) + 1)
    want_merged = np.nonzero(has & (uses[np.maximum(I["primMesh"], 0)] == 1))[0] if S["merge_singles"] else np.zeros(0, np.int64)
    ML = dump.get("MERGED_LIST")
    got_merged = np.zeros(0, np.int64) if ML is None else ML.astype(np.int64)
    if not np.array_equal(np.sort(got_merged), want_merged):
        rep.add("merged_list", _rows(-1, np.setxor1d(got_merged, want_merged)))
    is_merged = np.zeros(ninst, bool)
    is_merged[want_merged] = True
    active = np.nonzero(has & ~is_merged)[0]
    # instance tables
    tb = dump.get("INST_TRI_BASE")
    if tb is None or len(tb) != ninst:
        rep.add("inst_tri_base", _rows(-1, [ninst]))
    else:
        rep.add("inst_tri_base", _rows(-1, np.nonzero(tb != I["triBase"])[0]))
    blk = dump.get("INST_BLOCK")
    entries = (info["numTris"] >> PT_INST_BLOCK_SHIFT) + 2
    first = np.arange(entries, dtype=np.int64) << PT_INST_BLOCK_SHIFT
    want_blk = np.maximum(np.searchsorted(I["triBase"].astype(np.int64), first, side="right") - 1, 0)   # the last instance whose triBase <= first
    if blk is None or len(blk) != entries:
        rep.add("inst_block", _rows(-1, [entries]))
    else:
        rep.add("inst_block", _rows(-1, np.nonzero(blk != want_blk)[0]))
    if info["numActive"] != len(active) or info["numBlas"] != (0 if dump.get("BLAS_RANGES") is None else len(dump["BLAS_RANGES"])) + (1 if info["mergedTris"] else 0):
        rep.add("active_list", _rows(-1, [ninst]))   # the counts the context reports
    # the build's inputs where the dump has them: the active instances in ascending order, their padding constants
    if dump.get("ACTIVE") is not None and not np.array_equal(dump["ACTIVE"].astype(np.int64), active):
        rep.add("active_list", _rows(-1, np.setxor1d(dump["ACTIVE"].astype(np.int64), active) if len(dump["ACTIVE"]) != len(active) else active[dump["ACTIVE"] != active]))
    if dump.get("INST_PAD") is not None:
        P = dump["INST_PAD"]
        rep.add("inst_pad", _rows(-1, [ninst]) if len(P) != ninst else _rows(-1, active[(P[active] != _u(S["pad"][active])).any(1)]))
    # the ranges of the object-space BLASes: pairwise disjoint, inside the node capacity, clear of the merged structure
    R = dump.get("BLAS_RANGES")
    R = np.zeros((0, 2), np.int64) if R is None else R.astype(np.int64)
    owner = np.zeros(max(info["nodeCapacity"], 1) + 1, np.int64)
    owner[0:min(info["mergedWide"], info["nodeCapacity"])] += 1
    for base, num in R:
        owner[min(base, len(owner) - 1):min(base + num, len(owner) - 1)] += 1
    for k, (base, num) in enumerate(R):
        if num < 1 or base + num > info["nodeCapacity"] or (owner[base:base + num] > 1).any():
            rep.add("blas_ranges", _rows(-1, [k]))
    # merged structure
    merged_root = None
    if "merged" in hier:
        h = hier["merged"]
        where, nodes, merged_root = _audit_shape(h, rep, facts)
        _audit_world_leaves(h, rep, facts, where, dump, S, want_merged if len(want_merged) else got_merged)
        mb = info["mergedBox"].astype(np.float64)
        if merged_root is None or not ((mb[0:3] == merged_root[0]).all() and (mb[3:6] == merged_root[1]).all()):
            rep.add("merged_box", _rows(H_MERGED, [0]))
    if (len(want_merged) > 0) != (info["mergedTris"] > 0) or info["mergedTris"] != int(I["triCount"][want_merged].sum()):
        rep.add("merged_list", _rows(-1, [ninst]))
    # every BLAS by itself: shape; its records are judged against the mesh of the instances whose TLAS leaf names it
    shapes = {}
    for k, (base, num) in enumerate(R):
        h = hier[f"blas{k}"]
        h.slot0, h.nslots = _blas_slots(h)
        shapes[int(base)] = (h, _audit_shape(h, rep, facts)[0])
    # TLAS
    if "tlas" not in hier:
        if len(active) or len(want_merged):
            rep.add("tlas_leaf_set", _rows(H_TLAS, active))
        return
    h = hier["tlas"]
    where, nodes, _ = _audit_shape(h, rep, facts)
    Lf = dump["TLAS_LEAVES"]
    slots = np.arange(len(Lf))
    li = Lf[:, 0].astype(np.int64)
    ism = li == PT_INST_MERGED
    isi = ~ism & (li < ninst)
    uniq, cnt = np.unique(li[isi], return_counts=True)
    wrong = np.concatenate([np.setxor1d(uniq, active), uniq[cnt > 1], li[~ism & ~isi]])
    rep.add("tlas_leaf_set", _rows(H_TLAS, wrong))
    if int(ism.sum()) != (1 if info["mergedTris"] else 0):
        rep.add("tlas_leaf_set", _rows(H_TLAS, [PT_INST_MERGED]))
    iv = np.where(isi, li, 0)
    # fields
    bad = isi & ((Lf[:, 2] != (I["triBase"][iv] | (I["flags"][iv] << 29))) | (Lf[:, 3] != 0) | (Lf[:, 6] != 0) | (Lf[:, 7] != 0))
    bad |= ism & ((Lf[:, 1] != 0) | (Lf[:, 3:8] != 0).any(1))
    rep.add("tlas_leaf_fields", _rows(H_TLAS, slots[bad]))
    rep.add("tlas_leaf_pad", _rows(H_TLAS, slots[isi & (Lf[:, 4:6] != _u(S["pad"][iv])).any(1)]))
    # nodeBase: the root of the BLAS that holds the instance's own mesh; one BLAS per prim-mesh (two meshes never share one, a mesh never has two)
    nb = Lf[:, 1].astype(np.int64)
    bad = np.zeros(len(Lf), bool)
    judged = {}
    for s in slots[isi]:
        key = (int(nb[s]), int(I["primMesh"][li[s]]))
        if key not in judged:
            if key[0] not in shapes:
                judged[key] = False
            else:
                hb, wb = shapes[key[0]]
                judged[key] = hb.nslots == I["triCount"][li[s]] and _audit_blas_leaves(hb, _Report(), dict(facts), wb, dump, S, int(li[s])) == 0
        bad[s] = not judged[key]
    pm = I["primMesh"][iv]
    for s in slots[isi]:
        same_mesh, same_base = isi & (pm == pm[s]), isi & (nb == nb[s])
        bad[s] |= (nb[same_mesh] != nb[s]).any() or (pm[same_base] != pm[s]).any()
    inb = dump.get("INST_NODE_BASE")
    if inb is not None:
        bad |= isi & (inb[np.minimum(iv, len(inb) - 1)] != nb)
    rep.add("tlas_leaf_node_base", _rows(H_TLAS, slots[bad]))
    # the records, boxes and tags of every BLAS, against the mesh of the first instance that names it (an unnamed BLAS holds no known mesh)
    named = {}
    for s in slots[isi]:
        named.setdefault(int(nb[s]), int(li[s]))
    for base, (hb, wb) in shapes.items():
        if base in named and hb.nslots == I["triCount"][named[base]]:
            _audit_blas_leaves(hb, rep, facts, wb, dump, S, named[base])
        else:
            rep.add("tlas_leaf_node_base", _rows(hb.hid, [base]))
    # leaf boxes: the padded box of the exact fp32 bounds of the instance's T1 world vertices; the merged leaf: the padded mergedBox
    lo, hi = np.zeros((len(Lf), 3), F), np.zeros((len(Lf), 3), F)
    for s in slots[isi]:
        i = li[s]
        if I["triCount"][i] == 0:
            isi[s] = False
            continue
        kk = np.arange(I["triCount"][i], dtype=np.int64)
        pos, _ = _positions(S, np.full(len(kk), i, np.int64), kk)
        w = xform_point(np.broadcast_to(I["objectToWorld"][i], (len(kk) * 3, 3, 4)), pos.reshape(-1, 3))
        lo[s], hi[s] = w.min(0), w.max(0)
    lo[ism], hi[ism] = info["mergedBox"][0:3], info["mergedBox"][3:6]
    opaque = np.where(isi, (I["flags"][iv] & TRI_OPAQUE) != 0, False)
    if ism.any():   # the merged leaf carries the tag iff the merged structure holds a non-opaque triangle
        opaque[ism] = bool(((I["flags"][want_merged] & TRI_OPAQUE) != 0).all()) if len(want_merged) else True
    _audit_leaves(h, rep, facts, where, isi | ism, lo, hi - lo, np.zeros_like(lo), opaque, extra=np.stack([lo, hi], 1))


def padding_form(report):
    f = report["_facts"]
    if f["pad_separate"] and not f["pad_fused"]:
        return "separate"
    if f["pad_fused"] and not f["pad_separate"]:
        return "fused"
    return "undecided" if not (f["pad_separate"] or f["pad_fused"]) else "mixed"


def failing(report):
    return sorted(k for k in report if not k.startswith("_") and len(report[k]))


def assert_clean(report, what=""):
    bad = failing(report)
    for k in bad:
        print(f"{what} {k}: {len(report[k])} offenders (hierarchy, id, slot), first: {report[k][:6].tolist()}")
    assert not bad, f"{what}: failing checks {bad}"


# ---- the scenes both test files audit ------------------------------------------------------------------------------------------------------------
LADDER = [1, 2, 3, 4, 5, 12, 13, 14, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 5000]


def _soup_mesh(rng, n, spread=4.0, size=0.3):
    c = rng.uniform(-spread, spread, (n, 1, 3))
    pos = (c + rng.normal(0, size, (n, 3, 3))).reshape(-1, 3).astype(F)
    return pos, np.tile([(0, 0, 1)], (3 * n, 1)), rng.uniform(0, 1, (3 * n, 2)).astype(F), np.arange(3 * n, dtype=U)


def _one_mesh_scene(name, pos, uv=None, matrix=None):
    from vk_raytrace_amd.scene import Scene
    sc = Scene(name)
    m = sc.add_material()
    n = len(pos)
    uv = np.linspace(0, 1, 2 * n).reshape(n, 2) if uv is None else uv
    sc.add_node(sc.add_prim_mesh(pos, np.tile([(0, 0, 1)], (n, 1)), uv, np.arange(n, dtype=U), m), matrix)
    return sc


def soup(n, seed=0):
    """one instance (rotated, non-uniformly scaled: the world records are not the vertex buffer) of n random triangles"""
    from vk_raytrace_amd.scene import translate, rotate_y, rotate_x, scale
    rng = np.random.default_rng(1000 * seed + n)
    pos, _, uv, _ = _soup_mesh(rng, n)
    return _one_mesh_scene(f"soup{n}", pos, uv, translate(0.5, -1.0, 2.0) @ rotate_y(0.7) @ rotate_x(0.3) @ scale(1.5, 0.75, 1.25))


def coincident(n=300):
    return _one_mesh_scene("coincident", np.tile(np.array([(0.25, 0.5, 1), (1.5, 0.5, 1.25), (0.75, 1.75, 0.5)], F), (n, 1)))


def zero_area(n=300, seed=3):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-3, 3, (n, 1, 3))
    d = rng.normal(0, 0.5, (n, 1, 3)) * (np.arange(n) % 2)[:, None, None]   # every other one a point, the rest collinear
    pos = (p + d * np.array([0.0, 1.0, 2.0])[None, :, None]).astype(F)
    # some along x from 0 to a tiny t: the lower plane is then -pad itself, and pad = m * 4e-6 + 1e-30 is small enough for its two roundings to show
    tiny = np.arange(0, n, 5)
    pos[tiny, :, 0] = (rng.uniform(1, 9, (len(tiny), 1)) * 1e-25 * np.array([0.0, 1.0, 2.0])).astype(F)
    pos[tiny, :, 1:3] = pos[tiny, 0:1, 1:3]
    return _one_mesh_scene("zero_area", pos.reshape(-1, 3))


def half_coincident(n=300, seed=4):
    rng = np.random.default_rng(seed)
    pos, _, _, _ = _soup_mesh(rng, n // 2)
    return _one_mesh_scene("half_coincident", np.concatenate([pos, np.tile(pos[0:3], (n - n // 2, 1))]))


def forest(seed=7):
    """two-level scene: 12 prim-meshes of 1, 2, 3, 13, 64 and 257 triangles (two of each; the two of 13 geometrically identical), instantiated once or 2-5
    times, rotated / non-uniformly scaled / mirrored; a MASK material on one mesh; two instances without triangles in the middle of the node list"""
    from vk_raytrace_amd import host_device as hd
    from vk_raytrace_amd.scene import Scene, translate, rotate_y, rotate_x, rotate_z, scale
    rng = np.random.default_rng(seed)
    sc = Scene("forest")
    m = sc.add_material()
    mask = sc.add_material(alphaMode=hd.ALPHA_MASK, alphaCutoff=0.5, doubleSided=1, pbrBaseColorFactor=(0.5, 0.6, 0.7, 0.4))
    meshes = []
    for j, n in enumerate([1, 2, 3, 13, 64, 257] * 2):
        if n == 13 and j >= 6:
            pos, nrm, uv, idx = keep13    # the same geometry under another prim-mesh: a wrong nodeBase between the two changes no pixel
        else:
            pos, nrm, uv, idx = _soup_mesh(rng, n, spread=1.0, size=0.25)
            if n == 13:
                keep13 = (pos, nrm, uv, idx)
        meshes.append(sc.add_prim_mesh(pos, nrm, uv, idx, mask if (n == 64 and j < 6) else m))
    hole = sc.add_prim_mesh(np.zeros((3, 3)), [(0, 0, 1)] * 3, np.zeros((3, 2)), np.zeros(0, U), m)
    uses = [1, 3, 1, 2, 2, 1, 2, 1, 5, 2, 2, 4]   # instances per prim-mesh
    node = 0
    for pm, k in zip(meshes, uses):
        for _ in range(k):
            s = 10.0 ** rng.uniform(-0.5, 0.5, 3)
            if node % 4 == 1:
                s[node % 3] *= -1.0   # mirrored
            sc.add_node(pm, translate(*rng.uniform(-8, 8, 3)) @ rotate_y(rng.uniform(0, 6.3)) @ rotate_x(rng.uniform(0, 6.3)) @ rotate_z(rng.uniform(0, 6.3)) @ scale(*s))
            node += 1
            if node in (5, 11):
                sc.add_node(hole, translate(*rng.uniform(-8, 8, 3)))
    return sc
