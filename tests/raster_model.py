"""A third statement of oxc_draw_visbuffer's rules for triangles that no clip plane touches (include/oxcull.h: vertex, setup, cover, depth),
beside the device code and the C checker.  It has no paths: no small / big / tile split and no 32- versus 64-bit edge functions -- one
triangle, one pixel box, one formula.  `predict` is the other half: for one snapped triangle, which of the device's pixel walkers has to
take it and how many tile-list items it makes, written from the header and the switch-over conditions, not from the library.

Arithmetic.  Up to the snap every step is a numpy.float32 operation in the stated order (no contraction: numpy has none).  After the snap
everything is an integer: the setup (area sign, orientation, pixel box, top-left bias) and `pixel` use Python integers.  `draw` evaluates
the edge functions of a whole pixel box at once in int64, after `setup` has proved in Python integers that no edge value of the box reaches
2^62 (the functions are affine: their extremes lie at the box's corners), so the int64 values are the exact integers; `pixel` is the same
rule for one pixel in Python integers alone, and the tests hold the two against each other.  z/w is interpolated in binary64,
((e0 z0 + e1 z1) + e2 z2) * (1 / area), and rounded to binary32.  CPU only."""
import numpy as np

F = np.float32
SMALL_SPAN = 8      # pixel boxes up to 8 x 8 are walked by the wave that set them up ...
SMALL_SPREAD = 4096  # ... when the corners' spread is below 2^12 units (1/256 px)
TILE = 64           # a box beyond 64 x 64 px is cut into tiles of that size, one tile-list item each
NARROW = 32768      # 32-bit edge functions while every difference that enters them stays below 2^15 units
CLIP_W_MIN = F(2.0 ** -10)
GUARD = F(64.0)
RANGE = F(1048576.0)  # |screen| <= 2^20 px


def mul_point(m16, p):
    """mul(M, (p, 1)) with M column-major: ((m_r0 p0 + m_r1 p1) + m_r2 p2) + m_r3 per row, binary32."""
    m = np.asarray(m16, dtype=F)
    p = [F(v) for v in p]
    return [F(F(F(m[0 * 4 + r] * p[0]) + F(m[1 * 4 + r] * p[1])) + F(m[2 * 4 + r] * p[2])) + m[3 * 4 + r] for r in range(4)]


def clip_coords(p, world16, pv16):
    """vs_main: world = mul(world, (p, 1)).xyz, clip = mul(projection_view, (world, 1))."""
    return mul_point(pv16, mul_point(world16, p)[:3])


def touches_a_clip_plane(clips) -> bool:
    """True when a corner lies outside one of the five planes: the clipper's business, which this model leaves out."""
    for c in clips:
        x, y, w = F(c[0]), F(c[1]), F(c[3])
        d = (F(w - CLIP_W_MIN), F(F(GUARD * w) - x), F(F(GUARD * w) + x), F(F(GUARD * w) - y), F(F(GUARD * w) + y))
        if any(not (v >= 0) for v in d):
            return True
    return False


def snap(clips, W, H):
    """setup, first half: three clip-space corners -> ([X0, X1, X2], [Y0, Y1, Y2], [z0, z1, z2]) with X, Y Python integers in 1/256 px and z
    binary32, or None when a corner has w <= 0 or leaves the fixed-point range."""
    X, Y, z = [], [], []
    with np.errstate(all="ignore"):
        for c in clips:
            cx, cy, cz, cw = (F(v) for v in c)
            if not (cw > 0):
                return None
            sx = F(F(F(F(cx / cw) * F(0.5)) + F(0.5)) * F(W))
            sy = F(F(F(F(cy / cw) * F(0.5)) + F(0.5)) * F(H))
            if not (abs(sx) <= RANGE) or not (abs(sy) <= RANGE):
                return None
            X.append(int(np.floor(F(F(sx * F(256.0)) + F(0.5)))))
            Y.append(int(np.floor(F(F(sy * F(256.0)) + F(0.5)))))
            z.append(F(cz / cw))
    return X, Y, z


def edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _owns(ax, ay, bx, by) -> bool:
    """top-left rule of a positively oriented triangle: an edge owns the pixel centres on it when it goes down, or is horizontal going left."""
    dx, dy = bx - ax, by - ay
    return dy > 0 or (dy == 0 and dx < 0)


def setup(snapped, W, H):
    """setup, second half, in Python integers.  None for a back face or zero area (fixed-point area >= 0); else a dict with the oriented
    corners (corners 1 and 2 exchanged), the area, the clamped pixel box (px0 > px1 or py0 > py1: empty), the three biases, and the spread."""
    X, Y, z = snapped
    area = edge(X[0], Y[0], X[1], Y[1], X[2], Y[2])
    if area >= 0:
        return None
    X, Y, z = [X[0], X[2], X[1]], [Y[0], Y[2], Y[1]], [z[0], z[2], z[1]]
    t = dict(X=X, Y=Y, z=z, area=-area, spread=max(max(X) - min(X), max(Y) - min(Y)))
    # pixel (px, py) has its centre at (256 px + 128, 256 py + 128): the first centre at or after the minimum, the last at or before the maximum
    t["px0"], t["py0"] = max(-((128 - min(X)) // 256), 0), max(-((128 - min(Y)) // 256), 0)
    t["px1"], t["py1"] = min((max(X) - 128) // 256, W - 1), min((max(Y) - 128) // 256, H - 1)
    t["bias"] = [0 if _owns(X[(k + 1) % 3], Y[(k + 1) % 3], X[(k + 2) % 3], Y[(k + 2) % 3]) else -1 for k in range(3)]
    if t["px0"] <= t["px1"] and t["py0"] <= t["py1"]:  # the int64 evaluation of `draw` is exact: extremes of an affine function lie at corners
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            for px in (t["px0"], t["px1"]):
                for py in (t["py0"], t["py1"]):
                    assert abs(edge(X[a], Y[a], X[b], Y[b], 256 * px + 128, 256 * py + 128)) < 2 ** 62
    return t


def _depth_bits(e, z, area):
    e = [np.asarray(v, dtype=np.float64) for v in e]  # integer -> binary64 rounds to nearest even, as the C conversion does
    zd = ((e[0] * np.float64(z[0]) + e[1] * np.float64(z[1])) + e[2] * np.float64(z[2])) * (np.float64(1.0) / np.float64(area))
    return np.asarray(zd).astype(F)


def pixel(t, vis, px, py):
    """cover + depth for ONE pixel of a set-up triangle, Python integers: the packed (depth bits << 32 | vis) value, or 0 when the pixel
    is outside the box, not covered, or its depth is outside (0, 1]."""
    if not (t["px0"] <= px <= t["px1"] and t["py0"] <= py <= t["py1"]):
        return 0
    X, Y = t["X"], t["Y"]
    e = [edge(X[(k + 1) % 3], Y[(k + 1) % 3], X[(k + 2) % 3], Y[(k + 2) % 3], 256 * px + 128, 256 * py + 128) for k in range(3)]
    if any(e[k] + t["bias"][k] < 0 for k in range(3)):
        return 0
    zf = _depth_bits(e, t["z"], t["area"])
    if not (zf > 0) or zf > 1:
        return 0
    return (int(zf.view(np.uint32)) << 32) | vis


def draw_triangle(t, vis, image):
    """All pixels of a set-up triangle into `image` (uint64 [H, W]): per pixel the maximum of depth bits << 32 | vis."""
    if t is None or t["px0"] > t["px1"] or t["py0"] > t["py1"]:
        return
    X, Y = t["X"], t["Y"]
    cx = (np.arange(t["px0"], t["px1"] + 1, dtype=np.int64) * 256 + 128)[None, :]
    cy = (np.arange(t["py0"], t["py1"] + 1, dtype=np.int64) * 256 + 128)[:, None]
    e, inside = [], True
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        ek = (X[b] - X[a]) * (cy - Y[a]) - (Y[b] - Y[a]) * (cx - X[a])
        e.append(ek)
        inside = inside & (ek + t["bias"][k] >= 0)
    zf = _depth_bits(e, t["z"], t["area"])
    keep = inside & (zf > 0) & ~(zf > 1)
    packed = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(vis)
    win = image[t["py0"]:t["py1"] + 1, t["px0"]:t["px1"] + 1]
    np.maximum(win, np.where(keep, packed, np.uint64(0)), out=win)


def draw(frame, W, H, image=None):
    """frame: [(vis, [p0, p1, p2], world16, pv16)] -- triangles as positions (binary16-exact values), a column-major world matrix and
    projection_view.  Returns (image uint64 [H, W], [set-up triangle or None per entry]).  A triangle that touches a clip plane is an error:
    the model does not clip."""
    image = np.zeros((H, W), dtype=np.uint64) if image is None else image
    setups = []
    for vis, corners, world16, pv16 in frame:
        clips = [clip_coords(p, world16, pv16) for p in corners]
        assert not touches_a_clip_plane(clips), ("the model does not clip", vis, clips)
        s = snap(clips, W, H)
        t = setup(s, W, H) if s is not None else None
        setups.append(t)
        draw_triangle(t, vis, image)
    return image, setups


# ---- which walker, how many tiles ------------------------------------------------------------------------------------------------------------------
DROPPED, SMALL, RECT32, RECT64, TILES32, TILES64 = "dropped", "small", "rect32", "rect64", "tiles32", "tiles64"


def _narrow(t, x0, y0, x1, y1) -> bool:
    """The 32-bit form is exact for the pixel rectangle: corner - corner and pixel centre - corner all below 2^15 units on both axes."""
    lox, hix = min(min(t["X"]), 256 * x0 + 128), max(max(t["X"]), 256 * x1 + 128)
    loy, hiy = min(min(t["Y"]), 256 * y0 + 128), max(max(t["Y"]), 256 * y1 + 128)
    return hix - lox < NARROW and hiy - loy < NARROW


def predict(t):
    """For a set-up triangle (`setup`'s result; None = dropped at setup): (walker, tile-list items, goes to the big list).
    dropped  back face, zero area, or an empty clamped pixel box;
    small    box at most 8 x 8 px and spread below 4096: the setup wave's own pass (32-bit);
    rect32 / rect64      box at most 64 x 64 px: one rectangle, no tile item;
    tiles32 / tiles64    ceil(bw / 64) * ceil(bh / 64) >= 2 items, each 32-bit where its own rectangle allows."""
    if t is None or t["px0"] > t["px1"] or t["py0"] > t["py1"]:
        return DROPPED, 0, False
    bw, bh = t["px1"] - t["px0"] + 1, t["py1"] - t["py0"] + 1
    if bw <= SMALL_SPAN and bh <= SMALL_SPAN and t["spread"] < SMALL_SPREAD:
        return SMALL, 0, False
    ntx, nty = -(-bw // TILE), -(-bh // TILE)
    if ntx * nty == 1:
        return (RECT32 if _narrow(t, t["px0"], t["py0"], t["px1"], t["py1"]) else RECT64), 0, True
    # every tile's rectangle lies inside the corners' own box, so the test comes out the same for all of them
    kinds = {_narrow(t, t["px0"] + TILE * tx, t["py0"] + TILE * ty, min(t["px0"] + TILE * tx + TILE - 1, t["px1"]), min(t["py0"] + TILE * ty + TILE - 1, t["py1"]))
             for ty in range(nty) for tx in range(ntx)}
    assert len(kinds) == 1
    return (TILES32 if kinds == {True} else TILES64), ntx * nty, True


def setup_uses_wide_area(t) -> bool:
    """The area's sign is taken in 64 bits at setup when the spread reaches 2^15 units."""
    return t["spread"] >= NARROW
