"""Hand-assembled inputs of the meshlet bounds producer (oxc_build_meshlet_bounds) for the places random meshes do not reach: the
triangle-count switch-overs, the cone's decision thresholds, signed zeros that only the (value, index) reductions get right, values
finite assets can produce that leave the comfortable range, and meshlet counts that cross the producer's chunk seam and stride loops.

Every builder is deterministic and returns a Frame (or a dict of named Frames): positions f32 [V, 3], meshlets i32 [M, 4] =
{vertex_offset, tri_offset (bytes, a multiple of 4), vertex_count, tri_count}, vidx i32, micro u8 -- the arguments of
oracle.build_meshlet_bounds and RendererInstance.build_meshlet_bounds -- plus `info`, what the CPU tests assert about it.  Every frame is
checked by validate(): no index of it leaves its arrays, so a kernel that follows the meshlet records reads in bounds."""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

F32 = np.float32
PZ, NZ = F32(0.0), F32(-0.0)
NAN, INF = F32(np.nan), F32(np.inf)

LADDER_COUNTS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)


@dataclass
class Frame:
    name: str
    positions: torch.Tensor
    meshlets: torch.Tensor
    vidx: torch.Tensor
    micro: torch.Tensor
    info: dict = field(default_factory=dict)

    def args(self):
        return self.positions, self.meshlets, self.vidx, self.micro

    def cuda_args(self):
        return tuple(t.cuda() for t in self.args())


def validate(f: Frame) -> Frame:
    """Every read the producer derives from the records stays inside the arrays."""
    ml = f.meshlets.numpy().astype(np.int64)
    micro, vidx, V = f.micro.numpy(), f.vidx.numpy(), f.positions.shape[0]
    assert f.positions.dtype == torch.float32 and f.meshlets.dtype == torch.int32 and f.vidx.dtype == torch.int32 and f.micro.dtype == torch.uint8
    assert (ml >= 0).all() and (ml[:, 1] % 4 == 0).all(), "tri_offset is a multiple of 4"
    assert len(vidx) == 0 or (0 <= vidx.min() and vidx.max() < V)
    assert (ml[:, 1] + 3 * ml[:, 3] <= len(micro)).all()
    if len(ml) <= 8192:
        for vo, to, _, tc in ml.tolist():
            if tc:
                assert vo + int(micro[to:to + 3 * tc].max()) < len(vidx)
    else:  # the shared-pool frames: the coarse form of the same statement
        assert int(ml[:, 0].max()) + int(micro.max()) < len(vidx)
    return f


class _Mesh:
    """Appends meshlets; each brings its own vertices, stored in reverse so that vidx is not the identity."""

    def __init__(self, name):
        self.name, self.pos, self.vidx, self.micro, self.meshlets, self.nv = name, [], [], [], [], 0

    def add(self, verts, tris):
        verts = np.asarray(verts, dtype=F32).reshape(-1, 3)
        tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
        assert 1 <= len(verts) <= 256 and (len(tris) == 0 or (0 <= tris.min() and tris.max() < len(verts)))
        vo, to, n = len(self.vidx), len(self.micro), len(verts)
        self.pos.append(verts[::-1])
        self.vidx.extend(self.nv + n - 1 - i for i in range(n))
        self.nv += n
        self.micro.extend(int(v) for v in tris.ravel())
        self.micro.extend([0] * (-len(self.micro) % 4))
        self.meshlets.append((vo, to, n, len(tris)))
        return len(self.meshlets) - 1

    def add_empty(self):
        self.meshlets.append((0, len(self.micro), 0, 0))
        return len(self.meshlets) - 1

    def finish(self, **info):
        pos = np.concatenate(self.pos) if self.pos else np.zeros((1, 3), F32)
        return validate(Frame(self.name, torch.from_numpy(np.ascontiguousarray(pos, dtype=F32)), torch.tensor(self.meshlets, dtype=torch.int32).reshape(-1, 4),
                              torch.tensor(self.vidx, dtype=torch.int32), torch.tensor(self.micro + [0] * 4, dtype=torch.uint8), info))


def _random_tris(rng, nv, count):
    """`count` triangles of three distinct local vertices: non-degenerate for vertices in general position."""
    return np.stack([rng.choice(nv, 3, replace=False) for _ in range(count)]) if count else np.zeros((0, 3), np.int64)


def _degenerate(tris, at):
    tris = tris.copy()
    for k, t in enumerate(at):
        a, b = tris[t, 0], tris[t, 1]
        tris[t] = [(a, a, b), (a, b, a), (b, a, a), (a, a, a)][k % 4]
    return tris


# ---- count_ladder ----------------------------------------------------------------------------------------------------------------------------------
def count_ladder() -> Frame:
    """One meshlet per triangle count on both sides of each switch-over (8-blocks of the one-lane cone code, the 64-triangle passes, the
    LDS strip above 64, the 256-triangle cone limit), all-degenerate meshlets of 5 and 70 triangles, and meshlets whose degenerate
    triangles sit at 0, 7, 8, 63, 64 and last, so that the compaction rank crosses block and pass boundaries.  Random seeded triangles:
    the bounding-sphere sweep depends on their order."""
    rng = np.random.default_rng(20240607)
    m = _Mesh("count_ladder")
    info = {"counts": {}, "empty": [], "all_degenerate": [], "sprinkled": []}

    def verts(nv, k):
        return rng.uniform(-4.0, 4.0, (nv, 3)) + np.array([3.0 * (k % 5), -2.0 * (k % 3), 1.5 * k])

    for k, T in enumerate(LADDER_COUNTS):
        nv = 256 if T > 64 else min(64, T + 3)
        i = m.add(verts(nv, k), _random_tris(rng, nv, T))
        info["counts"][T] = i
        if T == 0:
            info["empty"].append(i)
    for T in (5, 70):
        nv = 256 if T > 64 else 16
        t = _random_tris(rng, nv, T)
        info["all_degenerate"].append(m.add(verts(nv, T), _degenerate(t, range(T))))
    for T, at in ((64, (0, 7, 8, 63)), (61, (0, 7, 8, 60)), (200, (0, 7, 8, 63, 64, 199)), (257, (0, 7, 8, 63, 64, 255, 256)), (129, (63, 64, 128))):
        nv = 256 if T > 64 else 64
        info["sprinkled"].append(m.add(verts(nv, T), _degenerate(_random_tris(rng, nv, T), at)))
    m.add_empty()
    info["empty"].append(len(m.meshlets) - 1)
    m.add(verts(12, 99), _random_tris(rng, 12, 9))  # an ordinary meshlet behind the empty one
    return m.finish(**info)


# ---- cone_thresholds -------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _frame_of(axis):
    a = _unit(axis)
    k = np.array([1.0, 0.0, 0.0]) if abs(a[0]) < 0.6 else np.array([0.0, 1.0, 0.0])
    b = _unit(np.cross(a, k))
    return a, b, np.cross(a, b)


def _tri_with_normal(n, origin=(0.0, 0.0, 0.0)):
    """Three corners whose (p1 - p0) x (p2 - p0) points along n."""
    n, u, v = _frame_of(n)
    o = np.asarray(origin, dtype=np.float64)
    return np.stack([o, o + u, o + v])


def _normal32(p0, p1, p2):
    """meshopt_computeClusterBounds' triangle normal in binary32, operation by operation (numpy rounds each one, fuses none)."""
    p0, p1, p2 = (np.asarray(p, dtype=F32) for p in (p0, p1, p2))
    a, b = p1 - p0, p2 - p0
    nx = a[1] * b[2] - a[2] * b[1]
    ny = a[2] * b[0] - a[0] * b[2]
    nz = a[0] * b[1] - a[1] * b[0]
    area = np.sqrt((nx * nx + ny * ny) + nz * nz)
    return np.array([nx / area, ny / area, nz / area], dtype=F32)


def _mirror_pair_mindp(X, Y):
    """The two triangles (0, ez, (X, Y, 0)) and (0, ez, (-X, Y, 0)) have the normals (a, b, 0) and (a, -b, 0) with bit-equal a and b.  For
    them every step of the cone code is exact but three: the extremal pair on axis y is the two normals, the centre is p1 + (p2 - p1) * 0.5
    = (a, 0, 0) exactly, the sweep finds d = sqrt(b * b) = b = radius and moves nothing, the axis is (a * (1 / a), 0, 0), and both dots
    are a * axis.x.  Returns that dot: the meshlet's mindp."""
    n = _normal32((0, 0, 0), (0, 0, 1), (X, Y, 0))
    n2 = _normal32((0, 0, 0), (0, 0, 1), (-X, Y, 0))
    assert n[0] == n2[0] and n[1] == -n2[1] and n[2] == 0 and n2[2] == 0
    a = n[0]
    return a * (a * (F32(1.0) / a))


def _mirror_pairs_around_a_tenth():
    """(X, Y) whose mirror pair has mindp == the float below 0.1f, 0.1f itself, and the float above it: Y is walked ulp by ulp."""
    tenth = F32(0.1)
    want = [np.nextafter(tenth, F32(0)), tenth, np.nextafter(tenth, F32(1))]
    X = F32(math.sqrt(0.99))
    found = {}
    y = F32(-0.1).view(np.uint32)
    for step in range(-4000, 4000):
        Y = np.uint32(int(y) + step).view(F32)
        dp = _mirror_pair_mindp(X, Y)
        for w in want:
            if dp == w and float(w) not in found:
                found[float(w)] = (X, Y)
    assert len(found) == 3, "the ulp walk must meet all three values"
    return [found[float(w)] for w in want]


def cone_thresholds() -> Frame:
    """Cones at the decisions of the cone code: mirror pairs whose mindp is exactly the float below 0.1f, 0.1f and the float above; two-
    and three-normal fans sweeping mindp across 0.1 around random axes; fans a hair narrower than the limit around random axes, where
    127 * (cutoff + the three s8 errors) + 1 passes 128 and only the clamp keeps the byte positive; two exactly opposite normals (centre 0,
    axis length 0); 1, 2 and 64 identical normals (paxisd = 0 and d = 0 guards)."""
    rng = np.random.default_rng(977)
    m = _Mesh("cone_thresholds")
    info = {"below": [], "exact": [], "above": [], "sweep2": [], "sweep3": [], "near_limit": [], "opposite": [], "identical": []}
    for key, (X, Y) in zip(("below", "exact", "above"), _mirror_pairs_around_a_tenth()):
        info[key].append(m.add([(0, 0, 0), (0, 0, 1), (X, Y, 0), (-X, Y, 0)], [(0, 1, 2), (0, 1, 3)]))

    def fan(axis, cos_half, count, extra=0):
        a, b, c = _frame_of(axis)
        s = math.sqrt(1.0 - cos_half * cos_half)
        verts, tris = [], []
        for j in range(count):
            phi = 2.0 * math.pi * j / count + 0.3
            n = cos_half * a + s * (math.cos(phi) * b + math.sin(phi) * c)
            for _ in range(1 + extra):
                verts.extend(_tri_with_normal(n, origin=rng.uniform(-1, 1, 3)))
                tris.append((len(verts) - 3, len(verts) - 2, len(verts) - 1))
        return m.add(verts, tris)

    for cos_half in np.linspace(0.09, 0.11, 41):
        info["sweep2"].append(fan(rng.normal(size=3), float(cos_half), 2))
    for cos_half in np.linspace(0.05, 0.6, 41):  # the sphere of three points is not centred on the fan's axis: mindp is below cos_half
        info["sweep3"].append(fan(rng.normal(size=3), float(cos_half), 3, extra=1))
    for j in range(96):
        info["near_limit"].append(fan(rng.normal(size=3), 0.1004 + 0.00008 * j, 2))
    for axis in ((0, 0, 1), (1, 0, 0), (0.3, -0.5, 0.8), (-1, 2, 3)):
        t = _tri_with_normal(axis)
        info["opposite"].append(m.add(t, [(0, 1, 2), (0, 2, 1)]))
    for axis, count in (((0, 0, 1), 1), ((0.2, 0.9, -0.4), 1), ((0, 1, 0), 2), ((-0.6, 0.1, 0.7), 2), ((0.5, 0.5, 0.7), 64)):
        t = _tri_with_normal(axis, origin=(1, 2, 3))
        info["identical"].append(m.add(t, [(0, 1, 2)] * count))
    return m.finish(**info)


# ---- signed_zeros ----------------------------------------------------------------------------------------------------------------------------------
def _flat_x_meshlet(m, rng, corner_x):
    """A meshlet of len(corner_x) / 3 triangles whose corner i has x = corner_x[i] (+0.0, -0.0 or NaN) and random y, z."""
    kinds = {"p": PZ, "n": NZ, "x": NAN}
    pools, verts = {}, []
    for k, x in kinds.items():
        pools[k] = list(range(len(verts), len(verts) + 8))
        for _ in range(8):
            verts.append((x, rng.uniform(-3, 3), rng.uniform(-3, 3)))
    tris = [[pools[corner_x[3 * t + c]][(3 * t + c) % 8] for c in range(3)] for t in range(len(corner_x) // 3)]
    return m.add(verts, tris)


def _pattern(T, first_tri, first, nan_tris=()):
    """Corner kinds: triangles in nan_tris have NaN x, corner 0 of first_tri is `first`, every other corner the other zero."""
    other = "n" if first == "p" else "p"
    c = [other] * (3 * T)
    for t in nan_tris:
        c[3 * t:3 * t + 3] = "xxx"
    c[3 * first_tri] = first
    return c


# what a flat axis shows when the first corner the fold keeps is +0.0 / -0.0: centre (hi + lo) * 0.5 and extent hi - lo, as
# half bits in the record and as float bits in the mesh box
ZERO_BITS = {"p": {"centre_half": 0x0000, "extent_half": 0x0000, "centre_f32": 0x00000000, "extent_f32": 0x00000000},
             "n": {"centre_half": 0x8000, "extent_half": 0x0000, "centre_f32": 0x80000000, "extent_f32": 0x00000000}}


def signed_zeros() -> dict:
    """Frames whose x axis is flat at zero with zeros of both signs.  The fold keeps the FIRST zero it meets (`b < a ? b : a` never
    replaces one zero by the other), hi and lo are then the same zero, and its sign is visible: centre = (hi + lo) * 0.5 is -0.0 for a
    first -0.0, extent = hi - lo is +0.0.  A reduction that breaks the tie any other way shows up as a flipped centre, or -- where it
    makes hi and lo zeros of opposite sign -- as a centre of +0.0 for a first -0.0 or an extent of -0.0.  info["first"][i] is the kind of
    the first zero of meshlet i, info["mesh_first"] that of the mesh.

    "meshlets": 130- and 40-triangle meshlets.  The first zero is corner 0, or comes behind triangles with NaN x (which both compares
    skip) -- behind the whole first pass of 64, behind all three triangles of lane 0, or late in the first pass while lane 0's next-pass
    triangle holds the other zero -- so the lane that starts the wave reduction does not hold the answer itself.
    "mesh_*": 1700 one-triangle meshlets.  With OXC_TUNE_BOUNDS_GRID 1, 2, 3 the partial fold's threads are 256, 512, 768 meshlets apart:
    the first zero and the other zeros then meet inside one thread's stride steps, in different threads and in different blocks."""
    rng = np.random.default_rng(4711)
    out = {}
    m = _Mesh("signed_zeros/meshlets")
    first = []
    for T in (130, 40):
        late = [t for t in range(T) if t % 64 == 0]
        for f in "pn":
            for c in (_pattern(T, 0, f), _pattern(T, 1, f, nan_tris=late), _pattern(T, 37, f, nan_tris=range(37))):
                _flat_x_meshlet(m, rng, c)
                first.append(f)
            if T > 64:
                _flat_x_meshlet(m, rng, _pattern(T, 64, f, nan_tris=range(64)))
                first.append(f)
                _flat_x_meshlet(m, rng, _pattern(T, 70, f, nan_tris=range(70)))
                first.append(f)
    out["meshlets"] = m.finish(first=first, mesh_first=first[0])

    def mesh(name, kinds):
        mm = _Mesh("signed_zeros/" + name)
        for k in kinds:
            if k == "e":
                mm.add_empty()
            else:
                mm.add([(PZ if k == "p" else NZ, rng.uniform(-3, 3), rng.uniform(-3, 3)) for _ in range(3)], [(0, 1, 2)])
        firsts = [k for k in kinds if k != "e"]
        return mm.finish(first=[None if k == "e" else k for k in kinds], mesh_first=firsts[0])

    n = 1700
    out["mesh_first_plus"] = mesh("mesh_first_plus", ["p"] + ["n"] * (n - 1))
    out["mesh_first_minus"] = mesh("mesh_first_minus", ["n"] + ["p"] * (n - 1))
    out["mesh_late_plus"] = mesh("mesh_late_plus", ["e"] * 300 + ["p"] + ["n"] * (n - 301))
    out["mesh_late_minus"] = mesh("mesh_late_minus", ["e"] * 300 + ["n"] + ["p"] * (n - 301))
    out["mesh_alternating"] = mesh("mesh_alternating", ["e"] * 5 + ["n" if i % 2 == 0 else "p" for i in range(n - 5)])
    return out


# ---- edge_values -----------------------------------------------------------------------------------------------------------------------------------
def edge_values() -> dict:
    """Coordinates at the ends of binary32 and at the half quantiser's boundaries, in a few vertices of otherwise ordinary meshlets and as
    whole meshlets, one frame per kind so that each keeps its own mesh box.
    huge: 1e20, where the cross product overflows to inf - inf and the normals become NaN.  tiny: 1e-20 and 1e-40 (the cross product is
    denormal or zero) and whole meshlets at 1e-10 .. 3e-12, where the squares under the square root are denormal: flushing any of them
    changes which triangles are degenerate.  fltmax: +-3e38, where hi - lo and hi + lo overflow.  nan, posinf, neginf, bothinf.
    half_bounds: boxes whose centre or extent is 2^-14, 65504, 65520, 65536 or the float next to one of them."""
    rng = np.random.default_rng(31337)
    out = {}

    def ordinary(m, specials, count=3):
        for j in range(count):
            v = rng.uniform(-2.0, 2.0, (24, 3)).astype(F32)
            for k, s in enumerate(specials):
                v[(5 * k + j) % 24, (k + j) % 3] = s
            m.add(v, _random_tris(rng, 24, 20))
        m.add(rng.uniform(-2.0, 2.0, (24, 3)), _random_tris(rng, 24, 20))  # an untouched one

    def whole(m, verts, T=20):
        m.add(verts, _random_tris(rng, len(verts), T))

    m = _Mesh("edge_values/huge")
    ordinary(m, [1e20, -1e20])
    whole(m, rng.uniform(-1, 1, (24, 3)) * 1e20)
    whole(m, rng.uniform(-1, 1, (200, 3)) * 3e19, T=100)
    out["huge"] = m.finish()

    m = _Mesh("edge_values/tiny")
    ordinary(m, [1e-20, -1e-20, 1e-40, -1e-40])
    for scale in (1e-20, 1e-40, 1e-9, 1e-10, 3e-11, 1e-11, 3e-12, 1e-12):
        whole(m, rng.uniform(-1, 1, (24, 3)) * scale)
    whole(m, rng.uniform(-1, 1, (200, 3)) * 2e-11, T=100)
    out["tiny"] = m.finish()

    m = _Mesh("edge_values/fltmax")
    ordinary(m, [3e38, -3e38])
    whole(m, rng.choice([3e38, -3e38, 1.0], (24, 3)))
    whole(m, np.full((8, 3), 3e38), T=4)
    whole(m, np.full((8, 3), -3e38), T=4)
    out["fltmax"] = m.finish()

    m = _Mesh("edge_values/nan")
    ordinary(m, [NAN, NAN, NAN])
    whole(m, np.full((8, 3), NAN), T=6)
    v = rng.uniform(-2, 2, (24, 3))
    v[:, 0] = NAN
    whole(m, v)
    whole(m, np.where(rng.uniform(size=(200, 3)) < 0.1, NAN, rng.uniform(-2, 2, (200, 3))), T=100)
    out["nan"] = m.finish()

    for name, vals in (("posinf", [INF]), ("neginf", [-INF]), ("bothinf", [INF, -INF])):
        m = _Mesh("edge_values/" + name)
        ordinary(m, vals * 2)
        whole(m, rng.choice(vals + [1.0], (24, 3)))
        whole(m, np.full((8, 3), vals[0]), T=4)
        out[name] = m.finish()

    m = _Mesh("edge_values/half_bounds")
    marks = [2.0 ** -14, 65504.0, 65520.0, 65536.0]
    vals = []
    for b in marks:
        for v in (b, 2.0 * b):  # as extent / centre of a flat box, and as centre of the box [0, 2b]
            vals += [F32(v), np.nextafter(F32(v), F32(0)), np.nextafter(F32(v), INF)]
    for v in vals:
        for lo in (F32(0.0), v):
            verts = rng.uniform(-2, 2, (8, 3)).astype(F32)
            verts[:, 0] = np.where(np.arange(8) % 2 == 0, lo, v)
            verts[:, 1] = np.where(np.arange(8) % 3 == 0, -v, verts[:, 1])
            whole(m, verts, T=6)
    out["half_bounds"] = m.finish(values=[float(v) for v in vals])
    return out


# ---- many_small ------------------------------------------------------------------------------------------------------------------------------------
def many_small(n: int) -> Frame:
    """n meshlets of 1 to 3 triangles over a shared pool of 64 vertices: windows into one vidx array and one micro array, so that the
    real constants (2^18 meshlets per chunk, the gather stride above 16 384, the fold stride above 65 536) are crossed with a few
    megabytes.  Neighbouring meshlets get different windows, hence different records."""
    rng = np.random.default_rng(5150)
    pos = rng.uniform(-8.0, 8.0, (64, 3)).astype(F32)
    vidx = rng.integers(0, 64, 4096 + 16).astype(np.int32)
    micro = rng.integers(0, 9, 4096 + 16).astype(np.uint8)  # local indices 0 .. 8
    i = np.arange(n, dtype=np.int64)
    ml = np.stack([(i * 7 + i // 4096) % 4096, 4 * ((i * 5 + i // 1024) % 1021), np.full(n, 9), 1 + i % 3], axis=1).astype(np.int32)
    return validate(Frame(f"many_small({n})", torch.from_numpy(pos), torch.from_numpy(ml), torch.from_numpy(vidx), torch.from_numpy(micro)))
