"""Checker of oxc_draw_physical_pages: rmvsm_build_draw_commands and rmvsm_draw_physical_pages (Shadowmaps.cpp:466-754) restated in numpy
under the rules include/oxcull.h states.  The vertex fetch is the oracle's orc_draw_visbuffer vertex part in binary32 without contraction
(micro_index, dequantize_half, the world transform, mul_mp); then the clipper, the 1/256-pixel snap, integer edge functions with the
top-left rule after orientation (cull mode None), binary64 depth from the exact edge values, the [0, 1] depth test, the fs_main page
lookup and a u32 minimum per texel.  Vectorised over triangles; only triangles that cross a clip plane and pixel boxes larger than
8 x 8 are walked one at a time (those per drawable page)."""
from __future__ import annotations

import numpy as np

import vsm_pages_model as VM
from pixel_rules import _u32, mul_mp

F = np.float32
VISIBLE, DIRTY, BACKED = VM.VISIBLE, VM.DIRTY, VM.BACKED
WMIN, GUARD = F(0.0009765625), F(64.0)
SMALL = 8


def dequantize_half(h) -> np.ndarray:
    """com::dequantize_half: denormals flush to signed zero, everything else is the IEEE value."""
    h = np.asarray(h).astype(np.uint16)
    f = h.view(np.float16).astype(np.float32)
    return np.where((h & 0x7FFF) < 0x400, np.where((h & 0x8000) != 0, F(-0.0), F(0.0)), f).astype(np.float32)


def decode_indices(indices, wide=0):
    """(meshlet instance, corner) of every index: (id << 8) | corner, (id << 9) | corner (wide = 1) or {id, corner} pairs (wide = 2)."""
    idx = _u32(indices).reshape(-1)
    if int(wide) == 2:
        p = idx.reshape(-1, 2)
        return p[:, 0].astype(np.int64), p[:, 1].astype(np.int64)
    bits = 9 if wide else 8
    return (idx >> bits).astype(np.int64), (idx & ((1 << bits) - 1)).astype(np.int64)


def fetch_world(scene, meshlet_instances, indices, wide=0, triangles=None) -> np.ndarray:
    """vs_main's vertex part for every corner of the list: world positions float32 [T, 3, 3].  `scene` is a CPU Scene: its Mesh and
    MeshLOD records hold the addresses of its own arrays, which locate every LOD array inside them."""
    mli, corner = decode_indices(indices, wide)
    T = len(mli) // 3 if triangles is None else min(int(triangles), len(mli) // 3)
    mli, corner = mli[:3 * T], corner[:3 * T]
    recs = np.asarray(meshlet_instances).reshape(-1, 2).astype(np.int64)[mli]
    mi = np.asarray(scene.mesh_instances).reshape(-1, 5).astype(np.int64)[recs[:, 0]]
    mesh = np.asarray(scene.meshes).reshape(-1, 8)[mi[:, 0]]
    lod = np.asarray(scene.lods).reshape(-1, 8)[(mesh[:, 4] - scene.lods.data_ptr()) // 64 + mi[:, 1]]
    ml = np.asarray(scene.meshlets).reshape(-1, 4).astype(np.int64)[(lod[:, 1] - scene.meshlets.data_ptr()) // 16 + recs[:, 1]]
    micro = np.asarray(scene.micro).reshape(-1).view(np.uint8)
    li = micro[lod[:, 3] - scene.micro.data_ptr() + ml[:, 1] + corner].astype(np.int64)  # scene.slang:336-342
    vi = _u32(scene.vidx).reshape(-1)[(lod[:, 4] - scene.vidx.data_ptr()) // 4 + ml[:, 0] + li].astype(np.int64)
    q = _u32(scene.positions).view(np.uint16).reshape(-1, 4)[(mesh[:, 0] - scene.positions.data_ptr()) // 8 + vi]
    p = dequantize_half(q[:, :3])
    xf = np.asarray(scene.transforms, dtype=np.float32).reshape(-1, 16)[mi[:, 3]]
    with np.errstate(invalid="ignore", over="ignore"):  # (a non-finite position is the caller's to drop)
        return mul_mp(xf, p)[:, :3].reshape(T, 3, 3)


def build_draw_commands(dirty_flags, count: int, source_command, commands=None, clipmaps=None):
    """rmvsm_build_draw_commands: active clipmaps in descending index; returns (commands int64 [count, 5], draw_count, clipmaps int64
    [count]) as u32 values, rows past draw_count keeping `commands` / `clipmaps`."""
    cmds = np.zeros((count, 5), np.int64) if commands is None else (np.array(commands, dtype=np.int64).reshape(count, 5) & 0xFFFFFFFF)
    cl = np.zeros(count, np.int64) if clipmaps is None else (np.array(clipmaps, dtype=np.int64).reshape(count) & 0xFFFFFFFF)
    src = np.asarray(source_command, dtype=np.int64).reshape(-1)[:5] & 0xFFFFFFFF
    active = active_clipmaps(dirty_flags, count)
    for i, c in enumerate(active):
        cmds[i] = src
        cl[i] = c
    return cmds, len(active), cl


def active_clipmaps(dirty_flags, count: int):
    f = np.asarray(dirty_flags).reshape(-1)
    return [c for c in range(count - 1, -1, -1) if int(f[c]) != 0]


def page_map(table, clipmaps, count: int, n: int, page_size: int, physical_page_table_size: int) -> np.ndarray:
    """Per clipmap and VIRTUAL page: the physical page coords (addr % P, addr / P) of its entry after wrapping when that entry is Backed &&
    Dirty with addr < P^2, else -1: int64 [count, n, n, 2]."""
    P = physical_page_table_size // page_size
    _, offs, _ = VM.unpack_clipmaps(clipmaps)
    t = _u32(table).reshape(count, n, n)
    vy, vx = np.mgrid[0:n, 0:n]
    out = np.full((count, n, n, 2), -1, dtype=np.int64)
    for c in range(count):
        e = t[c, VM.wrap(vy, offs[c, 1], n), VM.wrap(vx, offs[c, 0], n)].astype(np.int64)
        addr = e >> 16
        ok = ((e & (BACKED | DIRTY)) == (BACKED | DIRTY)) & (addr < P * P)
        out[c, ..., 0] = np.where(ok, addr % P, -1)
        out[c, ..., 1] = np.where(ok, addr // P, -1)
    return out


def _dists(v):
    x, y, w = v[..., 0], v[..., 1], v[..., 3]
    return [w - WMIN, GUARD * w - x, GUARD * w + x, GUARD * w - y, GUARD * w + y]


def clip_class(clip) -> np.ndarray:
    """0: every corner inside every plane, 1: crosses a plane (clipped), 2: all corners outside one plane (dropped); clip [T, 3, 4]."""
    with np.errstate(invalid="ignore"):
        ins = np.stack([d >= 0 for d in _dists(clip)])  # [5, T, 3]
    out = (~ins).all(axis=2).any(axis=0)
    cross = (~ins.all(axis=2)).any(axis=0)
    return np.where(out, 2, np.where(cross, 1, 0))


def clip_polygon(tri) -> list:
    """Sutherland-Hodgman of one [3, 4] triangle against the five planes in order (new vertex from the inside end I to the outside end O,
    binary32), fanned: list of [3, 4] triangles."""
    poly = [np.asarray(v, dtype=np.float32) for v in tri]
    for pl in range(5):
        if len(poly) < 3:
            break
        out, n = [], len(poly)
        for k in range(n):
            p, q = poly[k], poly[(k + 1) % n]
            dp, dq = _dists(p)[pl], _dists(q)[pl]
            ip, iq = bool(dp >= 0), bool(dq >= 0)
            if ip:
                out.append(p)
            if ip != iq:
                I, O = (p, q) if ip else (q, p)
                dI, dO = (dp, dq) if ip else (dq, dp)
                t = F(dI / (dI - dO))
                out.append((I + t * (O - I)).astype(np.float32))
        poly = out
    return [np.stack([poly[0], poly[k], poly[k + 1]]) for k in range(1, len(poly) - 1)]


def setup(clip, V: int):
    """The screen mapping, snap and orientation (cull mode None) of [K, 3, 4] clip-space triangles on a V x V viewport.  Returns (ok, X, Y,
    z): X, Y int64 [K, 3] in 24.8 fixed point, oriented with positive area; z float32 [K, 3]; ok False for zero area (and the guards)."""
    clip = np.asarray(clip, dtype=np.float32).reshape(-1, 3, 4)
    with np.errstate(all="ignore"):
        w = clip[..., 3]
        sx = ((clip[..., 0] / w) * F(0.5) + F(0.5)) * F(V)
        sy = ((clip[..., 1] / w) * F(0.5) + F(0.5)) * F(V)
        z = clip[..., 2] / w
        ok = (w > 0).all(1) & (np.abs(sx) <= F(1048576.0)).all(1) & (np.abs(sy) <= F(1048576.0)).all(1)
        X = np.where(ok[:, None], np.floor(sx * F(256.0) + F(0.5)), F(0)).astype(np.int64)
        Y = np.where(ok[:, None], np.floor(sy * F(256.0) + F(0.5)), F(0)).astype(np.int64)
    area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    ok &= area != 0
    order = np.where((area < 0)[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
    return ok, np.take_along_axis(X, order, 1), np.take_along_axis(Y, order, 1), np.take_along_axis(z, order, 1)


def _incl(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return (dy > 0) | ((dy == 0) & (dx < 0))


def _fragments(X, Y, z, px, py):
    """Coverage (top-left rule) and binary32 depth of pixels px, py [K, Q] of oriented triangles [K]: (covered & 0 <= z <= 1, z)."""
    cx, cy = px * 256 + 128, py * 256 + 128

    def edge(a, b):
        return (X[:, b, None] - X[:, a, None]) * (cy - Y[:, a, None]) - (Y[:, b, None] - Y[:, a, None]) * (cx - X[:, a, None])

    e = [edge(1, 2), edge(2, 0), edge(0, 1)]
    bias = [np.where(_incl(X[:, a], Y[:, a], X[:, b], Y[:, b]), 0, -1)[:, None] for a, b in ((1, 2), (2, 0), (0, 1))]
    inside = (e[0] + bias[0] >= 0) & (e[1] + bias[1] >= 0) & (e[2] + bias[2] >= 0)
    area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    inv = 1.0 / area.astype(np.float64)
    zd = ((e[0].astype(np.float64) * z[:, 0, None].astype(np.float64) + e[1].astype(np.float64) * z[:, 1, None].astype(np.float64)) +
          e[2].astype(np.float64) * z[:, 2, None].astype(np.float64)) * inv[:, None]
    zf = zd.astype(np.float32)
    with np.errstate(invalid="ignore"):
        keep = inside & (zf >= 0) & (zf <= 1)
    return keep, zf


def _write(u, pm, ps: int, phys: int, px, py, keep, zf):
    vx, vy = px // ps, py // ps
    m = pm[vy, vx]
    keep = keep & (m[..., 0] >= 0)
    tx = m[..., 0] * ps + (px - vx * ps)
    ty = m[..., 1] * ps + (py - vy * ps)
    np.minimum.at(u, (ty * phys + tx)[keep], zf.view(np.uint32)[keep])
    return int(keep.sum())


DROPPED, SMALL_PATH, DIRECT, TILED = "dropped", "small", "direct", "tiled"
SMALL_SPREAD, DIRECT_PAGES, BATCH = 4096, 4, 64


def classify(X, Y, V: int, pm, ps: int, from_clipper=None) -> dict:
    """What the kernels have to do with oriented set-up triangles [K] of one clipmap (page map `pm` [n, n, 2]), as arrays [K]:
    px0, py0, px1, py1  the pixel box clamped to the viewport;  spread  the larger of the corners' x and y extents (1/256 px);
    pages    drawable pages in the page box cut to the clipmap's rectangle of drawable pages (0: the pair is dropped);
    box_pages  pages of that cut box;
    small    pixel box at most 8 x 8 and -- unless the triangle comes out of the clipper (`from_clipper` bool [K]) -- spread < 4096: drawn
             where it was set up; every other kept pair goes to the big list;
    tiled    a big pair that hands out tiles: its cut box has more than 64 pages (every batch of 64 with a drawable page queues them) or more
             than 4 of its pages are drawable; `tiles` is then `pages`.  Other big pairs are drawn by their own wave (direct).
    All in int64: |X|, |Y| <= 2^28 (the 2^20-pixel guard of the setup), so extents stay below 2^29 and page counts below 2^16."""
    K = len(X)
    fc = np.zeros(K, bool) if from_clipper is None else np.asarray(from_clipper, bool)
    minx, maxx, miny, maxy = X.min(1), X.max(1), Y.min(1), Y.max(1)
    px0, py0 = np.maximum((minx - 128 + 255) >> 8, 0), np.maximum((miny - 128 + 255) >> 8, 0)
    px1, py1 = np.minimum((maxx - 128) >> 8, V - 1), np.minimum((maxy - 128) >> 8, V - 1)
    spread = np.maximum(maxx - minx, maxy - miny)
    boxed = (px1 >= px0) & (py1 >= py0)
    ok_page = pm[..., 0] >= 0
    n = ok_page.shape[0]
    sat = np.zeros((n + 1, n + 1), np.int64)
    sat[1:, 1:] = ok_page.astype(np.int64).cumsum(0).cumsum(1)
    pages, box_pages = np.zeros(K, np.int64), np.zeros(K, np.int64)
    if ok_page.any():
        ys, xs = np.nonzero(ok_page)
        rx0, rx1, ry0, ry1 = xs.min(), xs.max(), ys.min(), ys.max()
        sx0, sy0, sx1, sy1 = (np.where(boxed, v, 0) for v in (px0, py0, px1, py1))
        qx0, qx1 = np.maximum(sx0 // ps, rx0), np.minimum(sx1 // ps, rx1)
        qy0, qy1 = np.maximum(sy0 // ps, ry0), np.minimum(sy1 // ps, ry1)
        cut = boxed & (qx1 >= qx0) & (qy1 >= qy0)
        qx0, qx1, qy0, qy1 = (np.where(cut, v, 0) for v in (qx0, qx1, qy0, qy1))
        pages = np.where(cut, sat[qy1 + 1, qx1 + 1] - sat[qy0, qx1 + 1] - sat[qy1 + 1, qx0] + sat[qy0, qx0], 0)
        box_pages = np.where(cut, (qx1 - qx0 + 1) * (qy1 - qy0 + 1), 0)
    kept = pages > 0
    bw, bh = px1 - px0 + 1, py1 - py0 + 1
    small = kept & (bw <= SMALL) & (bh <= SMALL) & (fc | (spread < SMALL_SPREAD))
    big = kept & ~small
    tiled = big & ((box_pages > BATCH) | (pages > DIRECT_PAGES))
    return dict(px0=px0, py0=py0, px1=px1, py1=py1, spread=spread, pages=pages, box_pages=box_pages, kept=kept, small=small, big=big, tiled=tiled,
                tiles=np.where(tiled, pages, 0))


def raster(u, X, Y, z, V: int, pm, ps: int, phys: int, chunk: int = 8192, from_clipper=None):
    """Draw oriented triangles [K] into the u32 view `u` of the physical image through page map `pm` [n, n, 2] of one clipmap.
    Returns (pairs whose page box holds a drawable page, fragments written, big pairs, tiles) -- the last two as `classify` counts them.
    (Which pixel walk a pair gets here follows its box alone: every walk writes the same texels.)"""
    if len(X) == 0:
        return 0, 0, 0, 0
    k = classify(X, Y, V, pm, ps, from_clipper)
    px0, py0, px1, py1 = k["px0"], k["py0"], k["px1"], k["py1"]
    draw = np.flatnonzero(k["kept"])
    pairs, frags = len(draw), 0
    bw, bh = px1[draw] - px0[draw] + 1, py1[draw] - py0[draw] + 1
    small = draw[(bw <= SMALL) & (bh <= SMALL)]
    kk = np.arange(SMALL * SMALL)
    for s in range(0, len(small), chunk):
        ids = small[s:s + chunk]
        px = px0[ids, None] + kk % SMALL
        py = py0[ids, None] + kk // SMALL
        inbox = (px <= px1[ids, None]) & (py <= py1[ids, None])
        px, py = np.minimum(px, V - 1), np.minimum(py, V - 1)
        keep, zf = _fragments(X[ids], Y[ids], z[ids], px, py)
        frags += _write(u, pm, ps, phys, px, py, keep & inbox, zf)
    for i in draw[(bw > SMALL) | (bh > SMALL)]:
        vys, vxs = np.nonzero(pm[py0[i] // ps:py1[i] // ps + 1, px0[i] // ps:px1[i] // ps + 1, 0] >= 0)
        for vy, vx in zip((vys + py0[i] // ps).tolist(), (vxs + px0[i] // ps).tolist()):
            x0, x1 = max(px0[i], vx * ps), min(px1[i], vx * ps + ps - 1)
            y0, y1 = max(py0[i], vy * ps), min(py1[i], vy * ps + ps - 1)
            gy, gx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
            px, py = gx.reshape(1, -1), gy.reshape(1, -1)
            keep, zf = _fragments(X[i:i + 1], Y[i:i + 1], z[i:i + 1], px, py)
            frags += _write(u, pm, ps, phys, px, py, keep, zf)
    return pairs, frags, int(k["big"].sum()), int(k["tiles"].sum())


def _setups(scene, meshlet_instances, indices, draw_cmd, table, clipmaps, dirty_flags, n, ps, phys, count, wide):
    """Per active clipmap (descending): (clipmap, page map, triangle of the list [K], fan index [K] (-1: not clipped), ok, X, Y, z, crossing
    pairs) for every triangle the setup is run on."""
    cmd = np.asarray(draw_cmd, dtype=np.int64).reshape(-1) & 0xFFFFFFFF
    active = active_clipmaps(dirty_flags, count)
    T = 0 if cmd[1] == 0 else int(cmd[0]) // 3
    if not active or not T:
        return
    world = fetch_world(scene, meshlet_instances, indices, wide, T)
    pm = page_map(table, clipmaps, count, n, ps, phys)
    mats = VM.unpack_clipmaps(clipmaps)[0]
    for c in active:
        with np.errstate(invalid="ignore", over="ignore"):
            clip = mul_mp(mats[c], world)  # [T, 3, 4]
        cls = clip_class(clip)
        tris, tri, fan = [clip[cls == 0]], [np.flatnonzero(cls == 0)], [np.full(int((cls == 0).sum()), -1, np.int64)]
        for t in np.flatnonzero(cls == 1):
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                pieces = clip_polygon(clip[t])
            tris += [p[None] for p in pieces]
            tri.append(np.full(len(pieces), t, np.int64))
            fan.append(np.arange(len(pieces), dtype=np.int64))
        ok, X, Y, z = setup(np.concatenate(tris).reshape(-1, 3, 4), V=n * ps)
        yield c, pm[c], np.concatenate(tri), np.concatenate(fan), ok, X, Y, z, int((cls == 1).sum())


def predict(scene, meshlet_instances, indices, draw_cmd, table, clipmaps, dirty_flags, *, page_size: int, page_table_size: int,
            physical_page_table_size: int, clipmap_count: int, wide=0) -> list:
    """What the kernels have to do with every (triangle, clipmap) pair that reaches the setup, in the order clipmaps descending, unclipped
    triangles in list order, then the clipper's fan triangles: dicts {clipmap, triangle, fan (-1: not clipped), path, pages, box_pages,
    tiles, bw, bh, spread}.  path: `dropped` (zero area, empty pixel box, or no drawable page in its page box), `small` (drawn where it was
    set up), `direct` / `tiled` (big list; see `classify`)."""
    n, ps = page_table_size, page_size
    out = []
    for c, pm, tri, fan, ok, X, Y, z, _ in _setups(scene, meshlet_instances, indices, draw_cmd, table, clipmaps, dirty_flags, n, ps,
                                                    physical_page_table_size, clipmap_count, wide):
        k = classify(X, Y, n * ps, pm, ps, fan >= 0)
        for i in range(len(tri)):
            live = bool(ok[i]) and bool(k["kept"][i])
            path = DROPPED if not live else SMALL_PATH if k["small"][i] else TILED if k["tiled"][i] else DIRECT
            out.append(dict(clipmap=int(c), triangle=int(tri[i]), fan=int(fan[i]), path=path, pages=int(k["pages"][i]) if live else 0,
                            box_pages=int(k["box_pages"][i]) if live else 0, tiles=int(k["tiles"][i]) if live else 0,
                            bw=int(k["px1"][i] - k["px0"][i] + 1), bh=int(k["py1"][i] - k["py0"][i] + 1), spread=int(k["spread"][i]),
                            X=X[i].tolist(), Y=Y[i].tolist()))
    return out


def draw(image, scene, meshlet_instances, indices, draw_cmd, table, clipmaps, dirty_flags, *, page_size: int, page_table_size: int,
         physical_page_table_size: int, clipmap_count: int, wide=0, stats: dict = None) -> np.ndarray:
    """One oxc_draw_physical_pages call on a copy of `image` (float32 [phys, phys]): the physical image after it.  `stats` receives what
    oxc_debug_vsm_draw_stats counts when no queue overflows: pairs, fragments, big_pairs, tiles, clipped_pairs."""
    n, ps, phys, count = page_table_size, page_size, physical_page_table_size, clipmap_count
    img = np.array(image, dtype=np.float32).reshape(phys, phys).copy()
    u = img.view(np.uint32).reshape(-1)
    pairs = frags = big = tiles = crossing = 0
    for c, pm, tri, fan, ok, X, Y, z, cross in _setups(scene, meshlet_instances, indices, draw_cmd, table, clipmaps, dirty_flags, n, ps, phys, count, wide):
        p, fr, b, t = raster(u, X[ok], Y[ok], z[ok], n * ps, pm, ps, phys, from_clipper=(fan >= 0)[ok])
        pairs, frags, big, tiles, crossing = pairs + p, frags + fr, big + b, tiles + t, crossing + cross
    if stats is not None:
        stats.update(pairs=pairs, fragments=frags, big_pairs=big, tiles=tiles, clipped_pairs=crossing)
    return img


# ---- hand-made scenes -------------------------------------------------------------------------------------------------------------------
def flat_scene(tris_xyz):
    """One mesh instance with an identity world matrix whose vertices are the given (x, y, z) (half-exact values), and the index list of
    all its triangles as cull_triangles writes it: (scene, indices int32)."""
    import torch

    import oracle
    from oxylus_amd.synth import build_meshlets_simple, make_scene_from_mesh

    verts = sorted({tuple(v) for t in tris_xyz for v in t})
    index = {v: i for i, v in enumerate(verts)}
    pos = torch.tensor(verts, dtype=torch.float32)
    tris = torch.tensor([[index[tuple(v)] for v in t] for t in tris_xyz], dtype=torch.int64)
    meshlets, vidx, micro = build_meshlets_simple(tris)
    b, m6, q = oracle.build_meshlet_bounds(pos, meshlets, vidx, micro)
    s = make_scene_from_mesh(1, b, meshlets, micro, vidx, q, m6, device="cpu")
    s.transforms[0] = torch.eye(4).flatten()
    ml = s.meshlet_instances[:, 1].long()
    idx = [(i << 8) | c for i, m in enumerate(ml.tolist()) for c in range(3 * int(s.meshlets[m, 3]))]
    return s, torch.tensor(idx, dtype=torch.int64).to(torch.int32)


def pixel_clipmaps(count: int, V: int, offsets=None, scales=None) -> np.ndarray:
    """uint8 [count * 76] clipmap records whose matrix maps world (x, y) in pixels of a V x V viewport to clip space with w = 1
    (screen = (ndc * 0.5 + 0.5) * V = (x, y) / scale) and passes z through."""
    rec = np.zeros((count, 19), dtype=np.float32)
    for c in range(count):
        s = 1.0 if scales is None else float(scales[c])
        m = np.zeros(16, np.float32)
        m[0], m[12] = 2.0 / (V * s), -1.0
        m[5], m[13] = 2.0 / (V * s), -1.0
        m[10], m[15] = 1.0, 1.0
        rec[c, :16] = m
        if offsets is not None:
            rec.view(np.int32)[c, 16:18] = offsets[c]
    return rec.view(np.uint8).reshape(-1).copy()


def entry(addr: int, flags: int = VISIBLE | DIRTY | BACKED) -> int:
    return (int(addr) << 16) | int(flags)
