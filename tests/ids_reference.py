"""Test-side reference for the object identity queries (zr_read_ids / zr_pick / zr_instance_coverage): primitive id -> add-order
(object, instance, triangle) and instance slot, from nothing but the scene description.

Primitive ids use one global draw-order numbering (the oracle's zo_visibility and the renderer's winner plane): non-instanced draws
first, then instanced ones (ZE:3445-3476), each draw's ids running instance * triangles + triangle from its prim_base.  Objects and
instance slots are numbered in add order, one slot per instance, one per non-instanced object.  tests/test_ids_cpu.py holds this mapping
to the oracle's shaded output, so it is not a restatement of the library.
"""
import numpy as np

NO_ID = 0xFFFFFFFF


def items_of_scene(scene):
    """(triangles, instances or None) per object of an independent_scenes.Scene, in add order"""
    return [(len(it["idx"]) // 3, it["instances"]) for it in scene.items]


def items_of_config(cfg):
    """the same for a zeldaengine_amd.scenes.config*() dict"""
    return [(len(o["mesh"][1]) // 3, o.get("instances")) for o in cfg["objects"]]


def tables(items):
    """-> (prim_base, n_tris, object, slot_base) per draw in draw order, slot_base per object, slot count"""
    counts = [1 if inst is None else len(inst) for _, inst in items]
    slot_base = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if items else np.zeros(0, np.int64)
    draws, prim = [], 0
    for instanced in (False, True):
        for i, (nt, inst) in enumerate(items):
            if (inst is not None) != instanced:
                continue
            draws.append((prim, nt, i, int(slot_base[i])))
            prim += nt * counts[i]
    return np.array(draws, dtype=np.int64).reshape(-1, 4), slot_base, int(sum(counts))


def mapping(vis, items):
    """vis: primitive ids (any shape, NO_ID = none) -> dict of object, instance, triangle, slot arrays (NO_ID / -1 where none)"""
    draws, _, _ = tables(items)
    v = np.asarray(vis).astype(np.int64)
    hit = v != NO_ID
    d = np.clip(np.searchsorted(draws[:, 0], v, side="right") - 1, 0, len(draws) - 1)
    local = v - draws[d, 0]
    nt = np.maximum(draws[d, 1], 1)
    inst, tri = local // nt, local % nt
    none = np.uint32(NO_ID)
    return {"object": np.where(hit, draws[d, 2], none).astype(np.uint32), "instance": np.where(hit, inst, none).astype(np.uint32),
            "triangle": np.where(hit, tri, none).astype(np.uint32), "slot": np.where(hit, draws[d, 3] + inst, -1)}


def object_plane(vis, items):
    """what zr_read_ids(ZR_IDS_OBJECT) returns for this primitive plane: (H, W, 2) uint32"""
    m = mapping(vis, items)
    return np.stack([m["object"], m["instance"]], axis=-1)


def coverage(vis, items):
    """pixels won per instance slot"""
    m = mapping(vis, items)
    s = m["slot"][m["slot"] >= 0]
    return np.bincount(s, minlength=tables(items)[2]).astype(np.uint32)


def pick(vis, depth, items, x, y, w, h, cap=None):
    """zr_pick's answer from the primitive plane and GBuffer target 0: (list of hit tuples in order, total)"""
    H, W = vis.shape
    if x >= W or y >= H:
        return [], 0
    x1, y1 = min(W, x + w), min(H, y + h)
    sub = vis[y:y1, x:x1]
    m = mapping(sub, items)
    dep = np.ascontiguousarray(depth[y:y1, x:x1], dtype=np.float32)
    ys, xs = np.nonzero(sub != NO_ID)
    if len(ys) == 0:
        return [], 0
    slot = m["slot"][ys, xs]
    k64 = (dep[ys, xs].view(np.uint32).astype(np.uint64) << np.uint64(32)) | ((y + ys) * W + (x + xs)).astype(np.uint64)
    order = np.lexsort((k64, slot))                  # by slot, then nearest first
    slot_s = slot[order]
    first = np.concatenate([[True], slot_s[1:] != slot_s[:-1]])
    starts = np.nonzero(first)[0]
    counts = np.diff(np.concatenate([starts, [len(order)]]))
    hits = []
    for st, n in zip(starts, counts):
        q = order[st]
        yy, xx = ys[q], xs[q]
        hits.append((int(m["object"][yy, xx]), int(m["instance"][yy, xx]), int(n), int(m["triangle"][yy, xx]), int(x + xx), int(y + yy),
                     float(dep[yy, xx])))
    hits.sort(key=lambda t: (t[6], t[0], t[1]))
    total = len(hits)
    return (hits if cap is None else hits[:cap]), total
