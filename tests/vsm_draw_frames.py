"""Hand-written frames for oxc_draw_physical_pages and the table of cases its path tests share (CPU only; nothing here touches the device).

A `VFrame` is a raster_frames.Frame -- unit-triangle mesh instances under half-exact `affine` world matrices, so a corner lands on the
intended 1/256-pixel integer when the viewport is a power of two -- together with what the shadow draw needs besides: the shape
(page_table_size n, page_size, physical image side, clipmap count), the page table, the clipmap records (vsm_draw_model.pixel_clipmaps: world
units are viewport pixels, w = 1, z passes through), the dirty flags, the image before the draw and the draw command.  `expect` names, per
triangle of the index list, the path vsm_draw_model.predict must give it in the frame's first active clipmap (None: no claim), either as a
path or as (path, drawable pages of the cut page box, tiles); `intent` the snapped corners a threshold case was written for."""
import functools

import numpy as np

import raster_frames as RF
import vsm_draw_model as DM
from raster_frames import affine, px, right_triangle, translation

F = np.float32
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
ALL = DM.VISIBLE | DM.DIRTY | DM.BACKED


class VFrame:
    def __init__(self, frame, shape, table, clipmaps=None, flags=None, image=None, cmd=None, form=0, draw=None, expect=None, intent=None):
        n, ps, phys, count = shape
        self.frame, self.shape, self.form, self.draw = frame, shape, form, draw
        self.table = np.ascontiguousarray(table, dtype=np.uint32).reshape(count, n, n)
        self.clipmaps = DM.pixel_clipmaps(count, n * ps) if clipmaps is None else np.asarray(clipmaps, dtype=np.uint8)
        self.flags = [1] * count if flags is None else list(flags)
        self.image = np.ones((phys, phys), np.float32) if image is None else np.asarray(image, dtype=np.float32)
        self._cmd, self.expect, self.intent = cmd, expect, intent

    @property
    def V(self):
        return self.shape[0] * self.shape[1]

    def indices(self):
        return self.frame.indices(self.form, self.draw)

    @property
    def cmd(self):
        return [self.indices().numel() // (2 if self.form == 2 else 1), 1, 0, 0, 0] if self._cmd is None else list(self._cmd)

    def _args(self):
        n, ps, phys, count = self.shape
        s = self.frame.scene
        return (s, s.meshlet_instances, self.indices(), self.cmd, self.table, self.clipmaps, self.flags), dict(
            page_size=ps, page_table_size=n, physical_page_table_size=phys, clipmap_count=count, wide=self.form)

    def model(self):
        """(image after the draw, the model's stats)."""
        if not hasattr(self, "_model"):
            a, kw = self._args()
            st = {}
            self._model = (DM.draw(self.image, *a, stats=st, **kw), st)
        return self._model

    def predict(self):
        a, kw = self._args()
        return DM.predict(*a, **kw)

    def first_clipmap(self):
        """predict's rows of the unclipped pairs of the first active clipmap by triangle of the list (clipped pairs: the list of their fan rows)."""
        rows = self.predict()
        if not rows:
            return {}
        c, out = rows[0]["clipmap"], {}
        for r in rows:
            if r["clipmap"] == c:
                if r["fan"] < 0:
                    out[r["triangle"]] = r
                else:
                    out.setdefault(r["triangle"], []).append(r)
        return out


def table_of(shape, pages, clipmap=0, flags=ALL):
    """A table of `shape` that is empty but for {(vx, vy): address} (wrapped coordinates) in `clipmap`."""
    n, _, _, count = shape
    t = np.zeros((count, n, n), np.uint32)
    for (x, y), addr in pages.items():
        t[clipmap, y, x] = DM.entry(addr, flags)
    return t


def full_table(shape, seed=5, hole=None):
    """Every entry Backed && Dirty with an address of its own (a fixed shuffle of 0 .. n^2 - 1 per clipmap; needs P^2 >= n^2) except the
    pages `hole(vx, vy)` names."""
    n, ps, phys, count = shape
    assert (phys // ps) ** 2 >= n * n
    t = np.zeros((count, n, n), np.uint32)
    for c in range(count):
        perm = np.random.default_rng(seed + c).permutation(n * n).reshape(n, n)
        for y in range(n):
            for x in range(n):
                t[c, y, x] = DM.entry(int(perm[y, x]), ALL if hole is None or not hole(x, y) else DM.VISIBLE | DM.BACKED)
    return t


def units(tris, V, z=0.5):
    """raster_frames.units_case with the winding kept (cull mode None draws both): (Frame, intent or None)."""
    case = RF.units_case(tris, V, V, z=z, exact=V & (V - 1) == 0, keep_winding=True)
    return case.frame, case.intent


def page_box_triangle(ps, qx0, qy0, qx1, qy1):
    """A right triangle whose pixel box is exactly pages [qx0, qx1] x [qy0, qy1] (inclusive), in 1/256-px units."""
    return right_triangle(qx0 * ps, qy0 * ps, (qx1 - qx0 + 1) * ps, (qy1 - qy0 + 1) * ps)


# ---- 1. stride loops -------------------------------------------------------------------------------------------------------------------------------
STRIDE_SHAPE = (16, 16, 256, 1)


@functools.lru_cache(maxsize=None)
def stride_frame(count, form=0):
    """The first `count` triangles of raster_frames' shuffled stride frame (320 mesh instances, boxes of at most 3 x 3 px on 256 x 128 px) over
    a table whose 256 pages are all drawable, each with an address of its own."""
    return VFrame(RF.stride_frame(), STRIDE_SHAPE, full_table(STRIDE_SHAPE), form=form, draw=RF.stride_draw(count))


def perspective_clipmaps(count):
    """Clipmap records with raster_frames.clipped_stride_frame's matrix: clip = (x, y, 0.25, z)."""
    rec = np.zeros((count, 19), np.float32)
    rec[:, :16] = np.asarray(RF.clipped_stride_frame().pv, dtype=np.float32)
    return rec.view(np.uint8).reshape(-1).copy()


@functools.lru_cache(maxsize=None)
def clip_stride_frame():
    """136 thin triangles that each cross w = 2^-10 on a 128-px viewport: 136 queued pairs."""
    shape = (8, 16, 128, 1)
    return VFrame(RF.clipped_stride_frame(), shape, full_table(shape), clipmaps=perspective_clipmaps(1))


@functools.lru_cache(maxsize=None)
def big_stride_frame():
    """12 triangles with 40 x 40-px boxes (9 or 16 drawable pages each: tiled) and 3 with 20 x 20-px boxes (at most 4 pages: direct)."""
    tris = [right_triangle(3 + 17 * i, 5 + 13 * i, 40, 40) for i in range(12)] + [right_triangle(200, 8 + 60 * i, 20, 20) for i in range(3)]
    f, intent = units(tris, 256, z=[0.25 + 0.03125 * i for i in range(15)])
    return VFrame(f, STRIDE_SHAPE, full_table(STRIDE_SHAPE), expect=[DM.TILED] * 12 + [DM.DIRECT] * 3, intent=intent)


@functools.lru_cache(maxsize=None)
def wide_table_frame():
    """n = 96: 288 bitmap words per clipmap, two clipmaps; drawable pages in the words beyond 256 (rows 86 ..) and before."""
    shape = (96, 16, 256, 2)
    pages0 = {(0, 0): 0, (95, 95): 1, (50, 90): 2, (3, 86): 3, (40, 40): 4}
    pages1 = {(95, 0): 5, (0, 95): 6, (60, 88): 7}
    t = table_of(shape, pages0, 0) + table_of(shape, pages1, 1)
    tris = [page_box_triangle(16, 0, 0, 95, 95), page_box_triangle(16, 49, 89, 51, 91), right_triangle(16 * 60 + 2, 16 * 88 + 3, 7, 7), right_triangle(16 * 3 + 1, 16 * 86 + 1, 12, 12)]
    f, _ = units(tris, 96 * 16, z=[0.75, 0.5, 0.25, 0.375])
    return VFrame(f, shape, t)


# ---- 2. bitmap and rectangle ---------------------------------------------------------------------------------------------------------------------
BITMAP_NS, BITMAP_BITS = (24, 40, 64), ("bit0", "bit31", "mid")
BITMAP_ADDRESSES = (0, 15, 6)  # P = 4: the first and the last physical page and one between; 16 = P * P names no page


def bitmap_page(n, which):
    """The first page (vx, vy) with 3 <= vx, vy <= n - 4 on a bitmap row that straddles a 32-bit word whose bit is 0, 31 or strictly between."""
    for vy in range(3, n - 3):
        if (vy * n) >> 5 == (vy * n + n - 1) >> 5:
            continue
        for vx in range(3, n - 3):
            b = (vy * n + vx) & 31
            if (which == "bit0" and b == 0) or (which == "bit31" and b == 31) or (which == "mid" and 8 <= b <= 23):
                return vx, vy
    raise AssertionError((n, which))


@functools.lru_cache(maxsize=None)
def bitmap_frame(n, which, addr):
    """One drawable page (at physical address `addr`) and five triangles: page boxes that contain it, end one page short of it on its left
    and above it, and start one page past it on its right and below it -- the last four as wide as the table allows."""
    shape = (n, 16, 64, 1)
    dx, dy = bitmap_page(n, which)
    boxes = [(dx - 1, dy - 1, dx + 1, dy + 1), (0, dy - 1, dx - 1, dy + 1), (dx + 1, dy - 1, n - 1, dy + 1), (0, 0, n - 1, dy - 1), (0, dy + 1, n - 1, n - 1)]
    f, _ = units([page_box_triangle(16, *b) for b in boxes], n * 16)
    drawn = addr < 16
    return VFrame(f, shape, table_of(shape, {(dx, dy): addr}), expect=[(DM.DIRECT, 1, 0) if drawn else DM.DROPPED] + [DM.DROPPED] * 4)


@functools.lru_cache(maxsize=None)
def corners_frame(n):
    """Only (0, 0) and (n - 1, n - 1) are drawable: the rectangle is the whole table.  A triangle over the whole viewport (tiled: n^2 > 64
    pages), one whose page box leaves out column 0 and row n - 1 (no drawable page: every bitmap row of it is searched in vain), the same
    mirrored, and 2 x 2-page boxes on both corners."""
    shape = (n, 16, 64, 1)
    boxes = [(0, 0, n - 1, n - 1), (1, 0, n - 1, n - 2), (0, 1, n - 2, n - 1), (0, 0, 1, 1), (n - 2, n - 2, n - 1, n - 1)]
    tris = [page_box_triangle(16, *b) for b in boxes]
    tris[4] = [(v[0], v[1]) for v in px((n * 16, n * 16), (n * 16, n * 16 - 32), (n * 16 - 32, n * 16))]  # right angle on the far corner
    f, _ = units(tris, n * 16, z=[0.75, 0.5, 0.5, 0.25, 0.25])
    return VFrame(f, shape, table_of(shape, {(0, 0): 15, (n - 1, n - 1): 0}),
                  expect=[(DM.TILED, 2, 2), DM.DROPPED, DM.DROPPED, (DM.DIRECT, 1, 0), (DM.DIRECT, 1, 0)])


# ---- 3. small or big ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def box_shapes_frame():
    """Every box shape 1..8 x 1..8 (small path), in list order with triangles over an undrawable page (dropped: empty boxes in the wave's
    distribution) in front of them, after every fourth and behind them; the first wave's boxes total far more than 64 pixels."""
    shape = (16, 16, 256, 1)
    gone = right_triangle(200, 200, 6, 6)
    tris, expect = [gone] * 3, [DM.DROPPED] * 3
    for h in range(1, 9):
        for w in range(1, 9):
            tris.append(right_triangle(16 * (w - 1) + (4 + 3 * h) % 16, 16 * (h - 1) + (7 + 5 * w) % 16, w, h))
            expect.append(DM.SMALL_PATH)
            if w % 4 == 0:
                tris.append(gone)
                expect.append(DM.DROPPED)
    tris += [gone] * 3
    expect += [DM.DROPPED] * 3
    f, intent = units(tris, 256, z=[0.125 + 0.005 * (i % 100) for i in range(len(tris))])
    return VFrame(f, shape, full_table(shape, hole=lambda x, y: x >= 12 and y >= 12), expect=expect, intent=intent)


@functools.lru_cache(maxsize=None)
def threshold_frames():
    """name -> VFrame, one boundary each."""
    c = {}
    shape = (8, 16, 64, 1)  # V = 128
    some = {(x, y): (x + 3 * y) % 16 for y in range(8) for x in range(8)}
    f, intent = units([right_triangle(2, 2, 8, 8), right_triangle(20, 2, 9, 8), right_triangle(40, 2, 8, 9)], 128, z=[0.25, 0.5, 0.75])
    c["box-8x8-9x8-8x9"] = VFrame(f, shape, table_of(shape, {(x, y): x + 4 * y for y in range(2) for x in range(4)}),
                                  expect=[DM.SMALL_PATH, DM.DIRECT, DM.DIRECT], intent=intent)
    # a triangle hanging off each viewport edge: the on-screen box is 8 x 8 either way, the spread 4095 (small) or 4096 (big)
    E = 128 * 256
    tris, expect = [], []
    for far, path in ((2047, DM.SMALL_PATH), (2048, DM.DIRECT)):
        tris += [[(2048, 4096), (-far, 4096), (2048, 4096 + 2048)],                 # left
                 [(E - 2048, 12288), (E + far, 12288), (E - 2048, 12288 + 2048)],   # right
                 [(8192, 2048), (8192, -far), (8192 + 2048, 2048)],                 # top
                 [(20480, E - 2048), (20480, E + far), (20480 + 2048, E - 2048)]]   # bottom
        expect += [path] * 4
    f, intent = units(tris, 128, z=[0.25 + 0.0625 * i for i in range(8)])
    c["spread-4095-4096"] = VFrame(f, shape, table_of(shape, some), expect=expect, intent=intent)
    # 32- against 64-bit area at setup: both halves of the square, each in both windings
    shape = (16, 16, 128, 1)  # V = 256: 32768 units are half the viewport
    some = {(x, y): (x * 5 + y) % 64 for y in range(16) for x in range(16) if (3 * x + y) % 7 == 0}
    for s in (32767, 32768):
        a, b = [(0, 0), (s, 0), (0, s)], [(s, s), (0, s), (s, 0)]
        f, intent = units([a, b, [a[0], a[2], a[1]], [b[0], b[2], b[1]]], 256, z=[0.5, 0.25, 0.625, 0.375])
        c[f"spread-{s}"] = VFrame(f, shape, table_of(shape, some), expect=[DM.TILED] * 4, intent=intent)
    return c


# ---- 4. direct or tiled --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def direct_tiled_frames():
    """name -> VFrame with one big pair each.  The drawable pages reach the corners of the triangle's page box (or lie outside it), so the
    clipmap's rectangle does not cut the box."""
    shape = (16, 16, 256, 1)
    c = {}

    def one(name, box, pages, expect, z=0.5):
        # the right angle at the box's bottom-left corner or top-left corner
        f, _ = units([page_box_triangle(16, *box)], 256, z=z)
        c[name] = VFrame(f, shape, table_of(shape, {p: i + 1 for i, p in enumerate(pages)}), expect=[expect])

    four = [(2, 2), (5, 2), (3, 4), (2, 5)]
    one("4-pages", (2, 2, 5, 5), four, (DM.DIRECT, 4, 0))
    one("5-pages", (2, 2, 5, 5), four + [(4, 3)], (DM.TILED, 5, 5))
    one("64-page-box", (0, 0, 7, 7), [(0, 0), (7, 0), (0, 7), (3, 3)], (DM.DIRECT, 4, 0))
    one("72-page-box", (0, 0, 8, 7), [(0, 0), (8, 0), (0, 7), (3, 3)], (DM.TILED, 4, 4))
    one("65-page-box", (0, 0, 12, 4), [(0, 0), (12, 0), (0, 4)], (DM.TILED, 3, 3))
    # 81 pages, the drawable ones of the box at k = 64 .. 80 (rows 8 and 9 of pages 1 .. 9); (0, 12) and (12, 0) only widen the rectangle
    one("second-batch", (1, 1, 9, 9), [(0, 12), (12, 0), (2, 8), (1, 9), (2, 9)], (DM.TILED, 3, 3))
    return c


# ---- 5. deterministic overflows ------------------------------------------------------------------------------------------------------------------
OVERFLOW_SHAPE = (16, 16, 256, 1)
CAPACITY = 64


def _edge_table():
    return table_of(OVERFLOW_SHAPE, {(x, y): (y * 2 + (x != 0)) for y in range(16) for x in (0, 15)})


def _big_unclipped(k):
    """k triangles with 12 x 11-px boxes inside page column 0 (one or two drawable pages: direct)."""
    return [right_triangle(2, 1 + 3 * i, 12, 11) for i in range(k)]


def _crossing_big(k):
    """k thin triangles from x = 1 across the whole viewport and the guard band (x > 32.5 V): clipped, their pieces big (direct: columns 0 and 15)."""
    return [px((1, 3 + 30 * i), (1, 15 + 30 * i), (40 * 256, 9 + 30 * i)) for i in range(k)]


def _needles(k):
    """k thin triangles from the last four pixel columns across the guard band: clipped, their pieces at most 4 x 3 px (the clipper's own walk)."""
    return [px((252, 3 * i + 0.25), (252, 3 * i + 2.75), (40 * 256, 3 * i + 1.5)) for i in range(k)]


@functools.lru_cache(maxsize=None)
def overflow_frames():
    c = {}
    # three big pairs of 50 drawable pages in a 64-page box: 150 tiles for a list of 128, the third pair's ballot crosses it
    pages = {(x, y): x + 8 * y for y in range(8) for x in range(8) if x + 8 * y < 50}
    f, _ = units([page_box_triangle(16, 0, 0, 7, 7), [(v[0] + 64, v[1] + 32) for v in page_box_triangle(16, 0, 0, 7, 7)],
                  [(v[0] + 16, v[1] + 80) for v in page_box_triangle(16, 0, 0, 7, 7)]], 256, z=[0.5, 0.375, 0.25])
    c["tiles"] = VFrame(f, OVERFLOW_SHAPE, table_of(OVERFLOW_SHAPE, pages), expect=[(DM.TILED, 50, 50)] * 3)
    z = lambda k: [0.125 + 0.01 * (i % 64) for i in range(k)]  # noqa: E731
    f, _ = units(_big_unclipped(70) + _crossing_big(6), 256, z=z(76))
    c["big"] = VFrame(f, OVERFLOW_SHAPE, _edge_table())
    f, _ = units(_needles(70), 256, z=z(70))
    c["clip"] = VFrame(f, OVERFLOW_SHAPE, _edge_table())
    f, _ = units(_big_unclipped(70) + _needles(70), 256, z=z(140))
    c["big-and-clip"] = VFrame(f, OVERFLOW_SHAPE, _edge_table())
    return c


# ---- 6. the draw command -------------------------------------------------------------------------------------------------------------------------
COMMAND_SHAPE = (8, 16, 64, 2)


@functools.lru_cache(maxsize=None)
def command_frame(form=0, cmd=None, flags=(1, 1)):
    """Five triangles in a row (boxes 5 x 5 px, pages (0..1, 0)), every page of both clipmaps drawable; the second clipmap is scaled by 2."""
    f, _ = units([right_triangle(1 + 6 * i, 1, 5, 5) for i in range(5)], 128, z=[0.25 + 0.125 * i for i in range(5)])
    t = table_of(COMMAND_SHAPE, {(x, y): (x + 5 * y) % 16 for y in range(8) for x in range(8)}, 0) + \
        table_of(COMMAND_SHAPE, {(x, y): (3 * x + y) % 16 for y in range(8) for x in range(8)}, 1)
    return VFrame(f, COMMAND_SHAPE, t, clipmaps=DM.pixel_clipmaps(2, 128, scales=[1.0, 2.0]), flags=flags, form=form, cmd=cmd)


# ---- 7. page offsets -----------------------------------------------------------------------------------------------------------------------------
OFFSET_NS = (16, 24)


def offset_values(n):
    return [0, -1, n - 1, n, -n, 2 * n + 3, INT32_MIN, INT32_MAX]


@functools.lru_cache(maxsize=None)
def offset_frame(n, i):
    """page_offset = (values[i], values[(i + 3) % 8]) over a table in which every entry has an address of its own; one triangle over most of
    the viewport and three small ones."""
    shape = (n, 16, n * 16, 1)
    v = offset_values(n)
    V = n * 16
    tris = [px((1, 1), (1, V - 2), (V - 2, 1)), px((V - 1, V - 1), (V - 1, V // 2), (V // 2, V - 1)), right_triangle(V - 9, 3, 6, 6), right_triangle(V // 2 + 1, V // 2 + 2, 5, 7)]
    f, _ = units(tris, V, z=[0.75, 0.625, 0.25, 0.125])
    return VFrame(f, shape, full_table(shape, seed=n + i), clipmaps=DM.pixel_clipmaps(1, V, offsets=[(v[i], v[(i + 3) % 8])]))


# ---- 8. depth and non-finite input ---------------------------------------------------------------------------------------------------------------
DEPTH_SHAPE = (8, 16, 128, 1)
NEG_ZERO_BITS = 0x80000000


def _neg_zero_clipmaps(V):
    """pixel_clipmaps whose z row is (-0, -0, 1, -0): a world z of -0.0 stays -0.0 through the matrix product for positive x and y."""
    rec = DM.pixel_clipmaps(1, V).view(np.float32).copy()
    rec[2] = rec[6] = rec[14] = F(-0.0)
    return rec.view(np.uint8)


@functools.lru_cache(maxsize=None)
def neg_zero_frame():
    """Two triangles whose corners all have z = -0.0 (mesh z -0.0, a world matrix and a clipmap matrix whose z rows add -0.0 only), one with
    a box of 6 x 6 px and one of 20 x 20 px, over an image that holds 1.0, +0.0, 0.5 and -1.0 in bands: only the -1.0 texels change."""
    mesh = [[[(0.0, 0.0, -0.0), (1.0, 0.0, -0.0), (0.0, 1.0, -0.0)]]]
    worlds = []
    for x, y, s in ((2.0, 2.0, 6.0), (10.0, 10.0, 20.0)):
        m = affine((x, y, 0.0), (x + s, y, 0.0), (x, y + s, 0.0))
        m[2, :] = (-0.0, -0.0, 1.0, -0.0)
        worlds.append(m)
    f = RF.Frame(mesh, worlds, 128, 128)
    img = np.ones((128, 128), np.float32)
    table = full_table(DEPTH_SHAPE)
    vf = VFrame(f, DEPTH_SHAPE, table, clipmaps=_neg_zero_clipmaps(128), image=img)
    # bands by physical row, so that every triangle meets every stored value
    img[1::4], img[2::4], img[3::4] = F(0.0), F(0.5), F(-1.0)
    return vf


@functools.lru_cache(maxsize=None)
def half_depth_frame():
    """Depth from the mesh's binary16 z under translations: flat at 1.0 (kept), flat at the next binary16 above 1 (dropped), from 1.0 up to it
    (kept only on the diagonal edge, which runs through pixel centres and owns them: z is exactly 1.0 there), and from the binary16 below 1 up to the one above
    (partly kept) -- boxes 6 x 6 and 24 x 24 px."""
    up, dn = RF.Z_ABOVE_ONE_HALF, float(np.uint16(0x3BFF).view(np.float16))
    meshlets = []
    for z0, z1, z2 in ((1.0, 1.0, 1.0), (up, up, up), (1.0, 1.0, up), (dn, dn, up)):
        meshlets.append([[(0.0, 0.0, z2), (0.0, 6.0, z0), (6.0, 0.0, z1)], [(8.0, 0.0, z2), (8.0, 24.0, z0), (32.0, 0.0, z1)]])
    f = RF.Frame(meshlets, [translation(1.0, 1.0 + 30.0 * k) for k in range(4)], 128, 128)
    f.draw = [(k, k, j) for k in range(4) for j in range(2)]  # meshlet k under mesh instance k: each in a band of its own
    return VFrame(f, DEPTH_SHAPE, full_table(DEPTH_SHAPE), image=np.full((128, 128), 2.0, np.float32))


@functools.lru_cache(maxsize=None)
def nonfinite_frame(bits):
    """Three meshlets of one triangle each side by side; the middle one has one vertex whose x is `bits` (binary16: NaN 0x7E00, +Inf 0x7C00),
    patched into the scene's positions after the frame is built."""
    meshlets = [[[(2.0, 2.0, 0.5), (2.0, 9.0, 0.5), (9.0, 2.0, 0.5)]], [[(12.0, 2.0, 0.5), (12.0, 9.0, 0.5), (19.0, 2.0, 0.5)]],
                [[(22.0, 2.0, 0.25), (22.0, 9.0, 0.25), (29.0, 2.0, 0.25)]]]
    f = RF.Frame(meshlets, [translation(0.0, 0.0)], 128, 128)
    q = f.scene.positions.view(-1, 4)
    row = [i for i in range(q.shape[0]) if float(np.uint16(int(q[i, 0]) & 0xFFFF).view(np.float16)) == 19.0]
    assert len(row) == 1
    q[row[0], 0] = int(np.uint16(bits).view(np.int16))
    return VFrame(f, DEPTH_SHAPE, full_table(DEPTH_SHAPE), expect=[DM.SMALL_PATH, None, DM.SMALL_PATH])


@functools.lru_cache(maxsize=None)
def shared_edge_frame(s):
    """The quad (2, 2) .. (2 + s, 2 + s) split along a diagonal through pixel centres, the halves wound oppositely: s^2 fragments."""
    a, b = RF.diagonal_quad(s)
    f, intent = units([a, [b[0], b[2], b[1]]], 256, z=[0.25, 0.75])  # diagonal_quad winds both halves alike
    shape = (16, 16, 256, 1)
    return VFrame(f, shape, full_table(shape), intent=intent)


# ---- 9. V = 16384 --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def limit_frame():
    """n = 256, page_size 64 (V = 16384), a 256-texel image of 16 pages, 8 drawable pages in each of two clipmaps.  Clipmap 0 maps pixels:
    one triangle well inside, one that leaves the guard band (32.5 V px) on two sides.  Clipmap 1 has the perspective matrix clip = (x, y,
    0.25, z): one triangle around the viewport's centre with a corner behind w = 2^-10.  (Each triangle is set up under both matrices; the
    pixel ones lie outside the other's guard band, the perspective one is a speck at pixel (0, 0) of clipmap 0.)"""
    shape = (256, 64, 256, 2)
    V = 16384
    pages0 = {(1, 1): 0, (2, 2): 1, (3, 1): 2, (255, 255): 3, (128, 128): 4, (0, 255): 5, (255, 0): 6, (8, 8): 7}
    pages1 = {(128, 128): 8, (127, 127): 9, (128, 150): 10, (127, 200): 11, (128, 255): 12, (120, 128): 13, (136, 127): 14, (128, 100): 15}
    t = table_of(shape, pages0, 0) + table_of(shape, pages1, 1)
    rec = np.concatenate([DM.pixel_clipmaps(1, V), perspective_clipmaps(1)])
    worlds = [affine((70.0, 70.0, 0.25), (70.0, 250.0, 0.5), (250.0, 70.0, 0.75)),
              affine((100.0, 100.0, 0.5), (40.0 * V, 200.0, 0.5), (200.0, 40.0 * V, 0.5)),
              affine((-0.03125, -0.5, 1.0), (0.0, 1.0, -0.5), (0.03125, -0.5, 1.0))]
    f = RF.Frame(RF.UNIT, worlds, V, V)
    return VFrame(f, shape, t, clipmaps=rec)


# ---- 10. the two draws on one frame ----------------------------------------------------------------------------------------------------------
AGREEMENT_SHAPE = (8, 16, 128, 1)
AGREEMENT_CLASSES = ("small box", "big box in one page", "box over 9 pages", "box over 64 px", "crossing w = 2^-10")


@functools.lru_cache(maxsize=None)
def agreement_frame():
    """One frame for oxc_draw_visbuffer at 128 x 128 and oxc_draw_physical_pages with one clipmap of 8 x 8 pages of 16 px, every page backed,
    dirty and mapped to itself (V = 128), both under raster_frames.clipped_stride_frame's matrix clip = (x, y, 0.25, z): depth is 0.25 / w.
    Five front-facing triangles that share no pixel, one per AGREEMENT_CLASSES: boxes of 6 x 6, 12 x 12 (inside page (1, 0)), 40 x 40 (pages
    5..7 x 0..2) and 50 x 70 px at w = 1, 0.5, 0.3125, 0.4, and a sliver down the middle columns from w = 1 to w = -0.5, whose pixels with
    w > 0.25 have a depth below 1.  The image starts at 2.0, so every texel the shadow draw writes shows."""
    def flat(t, w):  # a triangle given in 1/256 px on the plane of clip w
        return [((X / 256.0 / 64.0 - 1.0) * w, (Y / 256.0 / 64.0 - 1.0) * w, w) for X, Y in t]

    tris = [flat(right_triangle(4, 4, 6, 6), 1.0), flat(right_triangle(17, 1, 12, 12), 0.5), flat(right_triangle(80, 4, 40, 40), 0.3125),
            flat(right_triangle(2, 50, 50, 70), 0.4), [(-0.0625, -0.5, 1.0), (0.0, 1.0, -0.5), (0.0625, -0.5, 1.0)]]
    f = RF.Frame(RF.UNIT, [affine(*t) for t in tris], 128, 128, pv=RF.clipped_stride_frame().pv)
    table = table_of(AGREEMENT_SHAPE, {(x, y): x + 8 * y for y in range(8) for x in range(8)})
    return VFrame(f, AGREEMENT_SHAPE, table, clipmaps=perspective_clipmaps(1), image=np.full((128, 128), 2.0, np.float32),
                  expect=[DM.SMALL_PATH, (DM.DIRECT, 1, 0), (DM.TILED, 9, 9), DM.TILED, None])


# ---- every frame by name (the CPU tests walk this; the GPU tests take the frames from the functions above) --------------------------------------
@functools.lru_cache(maxsize=None)
def all_frames():
    c = {f"stride-{n}-form{form}": stride_frame(n, form) for n in RF.STRIDE_COUNTS for form in (0, 1, 2)}
    c.update({"stride-clip": clip_stride_frame(), "stride-big": big_stride_frame(), "stride-wide-table": wide_table_frame()})
    for n in BITMAP_NS:
        for k, which in enumerate(BITMAP_BITS):
            c[f"bitmap-n{n}-{which}"] = bitmap_frame(n, which, BITMAP_ADDRESSES[k])
        c[f"bitmap-n{n}-outside-the-image"] = bitmap_frame(n, "mid", 16)
        c[f"corners-n{n}"] = corners_frame(n)
    c["box-shapes"] = box_shapes_frame()
    c.update({f"threshold-{k}": v for k, v in threshold_frames().items()})
    c.update({f"pages-{k}": v for k, v in direct_tiled_frames().items()})
    c.update({f"overflow-{k}": v for k, v in overflow_frames().items()})
    c.update({f"command-form{form}": command_frame(form) for form in (0, 2)})
    c.update({f"offset-n{n}-{i}": offset_frame(n, i) for n in OFFSET_NS for i in range(8)})
    c.update({"neg-zero": neg_zero_frame(), "half-depth": half_depth_frame(), "nan": nonfinite_frame(0x7E00), "inf": nonfinite_frame(0x7C00),
              "shared-edge-8": shared_edge_frame(8), "shared-edge-40": shared_edge_frame(40), "limit": limit_frame(), "agreement": agreement_frame()})
    return c
