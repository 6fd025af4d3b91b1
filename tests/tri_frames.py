"""Hand-written frames for the triangle stage (cull_triangles: tris_test_body, tris_fused_body, tris_emit_body, expand_slots_wide) and the
tables of cases its tests share (CPU only; nothing here touches the device).

A `Frame` is a visible list written out slot by slot: every slot names a `Shape` -- vertex count, one meant-to-pass flag per stored triangle,
the micro-index byte offset mod 4, dangling offsets or not -- and the builder lays the shapes out as ONE mesh (make_scene_from_mesh) whose
Meshlet records follow the list (record i = slot i, geometry shared between equal shapes; `instances` > 1: the list is the first n entries of
the usual instance-major expansion, so slot i names record i mod K of instance i div K).  Either way the visibility-mask bit of slot i is
bit i, and the meshlet bounds are huge boxes with a degenerate cone, so the meshlet cull keeps every slot whatever the flags: V = n.

Pass and fail are decisive by construction.  Vertices sit on the parabola (x, x * x) with integer x in [-32, 31] (exact in binary16), z = 0.5;
projection_view is the identity and a world matrix is a translation by small integers with a power-of-two x scale.  Three vertices with
ascending x make a determinant (xj - xi)(xk - xi)(xk - xj) >= 2 (dropped), the same three with two corners exchanged <= -2 (kept); every
product is an integer below 2^24, so every evaluation order gives the same bits.  A meshlet of four or more vertices keeps vertex 0 at
z = -1: every other meant-to-fail triangle is a kept orientation through that vertex (dropped by clip.z alone).  `check_intent` asserts
|det| >= 1 with the meant sign, z >= 0.5 or z <= -0.5, and the oracle's own backface test, for every distinct (shape, instance).

Late lists: `early` = E puts E slots in front whose mask bits are set; with an all-zero pyramid (nothing is ever occluded: reversed Z, zero
is the far plane) the early call emits exactly those, the late call the other n - E, from first = E (odd)."""
import functools
import itertools

import numpy as np
import torch

F = np.float32
CHUNK, FUSED_SPAN, SPAN, EMIT_RUN, TICKET_COUNTERS, CHUNKS_PER_SUPER = 64, 128, 256, 1024, 16, 64  # oxcull_types.hpp, oxcull_kernels.hip
EARLY = 7          # early slots in front of a late list: odd, no multiple of 4
SENTINEL = -1      # what the tests pre-fill the output lists with
LARGEST_CUS = 256  # the CPU tests size family D for 256 CUs: 256 * 256 + 1 = 65 537 one-triangle meshlets is the largest frame of the module
DANGLING = (0x3FFFFFFF, 0x3FFFFFFC)  # vertex / micro offsets of an empty meshlet nothing may be read through


def cap(form):
    return 128 if form else 64


def words(form):
    return 2 if form == 2 else 1


def kdw(form):
    return 6 if form == 2 else 3


class Shape:
    """vcount vertices; passes[t]: triangle t is meant to pass (len = the STORED triangle count, cut to 64 / 128 by the stage); boff: micro byte offset mod 4."""

    def __init__(self, vcount, passes, boff=0, dangling=False):
        self.vcount, self.passes, self.boff, self.dangling = int(vcount), tuple(bool(p) for p in passes), int(boff) & 3, bool(dangling)
        assert 1 <= self.vcount <= 64 and self.vcount != 2 and (self.vcount >= 3 or not any(self.passes)), "one vertex makes no triangle that passes"
        assert not (dangling and self.passes), "dangling offsets only where nothing is read"
        self.key = (self.vcount, self.passes, self.boff, self.dangling)

    @property
    def T(self):
        return len(self.passes)

    def count(self, form):
        return sum(self.passes[:cap(form)])

    def mask(self, form):
        return sum(1 << t for t, p in enumerate(self.passes[:cap(form)]) if p)

    def positions(self):
        if self.vcount == 1:
            return [(0.0, 0.0, -1.0)]
        xs = [v - self.vcount // 2 for v in range(self.vcount)]
        return [(float(x), float(x * x), -1.0 if (v == 0 and self.vcount >= 4) else 0.5) for v, x in enumerate(xs)]

    def corners(self):
        """Three local vertex indices per stored triangle.  The last triangle always ends on the last vertex (the lane clamp of stage_idx / stage_pos)."""
        out = []
        lo = 1 if self.vcount >= 4 else 0
        for t, p in enumerate(self.passes):
            if self.vcount < 3:
                out.append((self.vcount - 1,) * 3)
                continue
            k = self.vcount - 1 - ((self.T - 1 - t) % (self.vcount - lo - 2))
            i, j = k - 2, k - 1
            if p:
                out.append((i, k, j))
            elif lo and t % 2:
                out.append((0, k, j))  # a kept orientation through the z = -1 vertex
            else:
                out.append((i, j, k))
        return out


def translation(tx, ty, sx=1.0):
    m = np.eye(4, dtype=F)
    m[0, 0], m[0, 3], m[1, 3] = sx, tx, ty
    return m


def default_worlds(M):
    return [translation(float(i % 5), float(i % 3), 2.0 if i % 2 else 1.0) for i in range(M)]


IDENTITY_PV = np.eye(4, dtype=F).reshape(-1).tolist()
BOUNDS_ROW = [0, 0, 0, 0, 0x6C00, 0x6C00, 0x6C00, 0x7F7F]  # centre 0, cone axis (0, 0), extent 4096 (binary16), axis z = 1, cutoff 127 / 127 = 1: never cone-culled


class Frame:
    """slots: one Shape per record (instances == 1: per slot).  n: length of the list (default: instances * records).  pairs: an explicit list of
    (mesh instance, record) instead of the expansion (no mask bits then: plain calls only).  early: the first `early` slots are last frame's."""

    def __init__(self, slots, instances=1, n=None, worlds=None, pv=None, resolution=None, pairs=None, early=0, name=""):
        from oxylus_amd.synth import make_scene_from_mesh

        self.name, self.records, self.M, self.early = name, list(slots), int(instances), int(early)
        K = len(self.records)
        self.worlds = default_worlds(self.M) if worlds is None else [np.asarray(w, dtype=F) for w in worlds]
        assert len(self.worlds) == self.M
        self.pv = IDENTITY_PV if pv is None else [float(v) for v in pv]
        if pairs is None:
            self.n = self.M * K if n is None else int(n)
            assert (self.M - 1) * K < self.n <= self.M * K
            self.pairs = None
        else:
            assert early == 0
            self.pairs, self.n = [(int(i), int(k)) for i, k in pairs], len(pairs)
        geometry, positions, vidx, micro, rows = {}, [], [], [], []
        for s in self.records:
            if s.dangling:
                rows.append((DANGLING[0], DANGLING[1] + s.boff - 4 * (s.boff != 0), s.vcount, 0))
                continue
            if s.key not in geometry:
                micro += [0] * ((s.boff - len(micro)) % 4)  # no other padding between meshlets
                geometry[s.key] = (len(vidx), len(micro))
                vidx += [len(positions) + v for v in range(s.vcount)]
                positions += s.positions()
                micro += [c for tri in s.corners() for c in tri]
            voff, boff = geometry[s.key]
            assert boff % 4 == s.boff
            rows.append((voff, boff, s.vcount, s.T))
        micro += [0] * (-len(micro) % 4)
        positions, vidx, micro = positions or [(0.0, 0.0, 0.0)], vidx or [0], micro or [0, 0, 0, 0]
        q = torch.zeros((len(positions), 4), dtype=torch.int16)
        p16 = torch.tensor(positions, dtype=torch.float32).to(torch.float16)
        assert torch.equal(p16.to(torch.float32), torch.tensor(positions, dtype=torch.float32)), "mesh positions must be exact in binary16"
        q[:, :3] = p16.view(torch.int16)
        bounds = torch.tensor([BOUNDS_ROW], dtype=torch.int32).to(torch.int16).repeat(K, 1)
        s = make_scene_from_mesh(self.M, bounds, torch.tensor(rows, dtype=torch.int32).reshape(-1, 4), torch.tensor(micro, dtype=torch.uint8),
                                 torch.tensor(vidx, dtype=torch.int32), q, torch.zeros(6))
        for i, w in enumerate(self.worlds):
            s.transforms[i] = torch.from_numpy(np.ascontiguousarray(w.T).reshape(-1).copy())  # column-major
        s.meshlet_instances = (s.meshlet_instances[:self.n] if self.pairs is None else torch.tensor(self.pairs, dtype=torch.int32).reshape(-1, 2)).contiguous().clone()
        s.camera = dict(s.camera, projection_view=list(self.pv))
        if resolution is not None:
            s.camera["resolution"] = [float(resolution[0]), float(resolution[1])]
        self.scene = s
        self.mask = torch.zeros(max((self.n + 31) // 32, 1), dtype=torch.int32)
        for i in range(self.early):
            self.mask[i // 32] |= 1 << (i % 32)

    def slot(self, i):
        """(mesh instance, Shape) of slot i of the whole list."""
        inst, k = (i // len(self.records), i % len(self.records)) if self.pairs is None else self.pairs[i]
        return inst, self.records[k]

    @property
    def V(self):
        """Length of the list the frame was written for: the late list where there is an early one."""
        return self.n - self.early

    def counts(self, form):
        """Meant pass count per slot of that list."""
        return [self.slot(i)[1].count(form) for i in range(self.early, self.n)]

    def meant(self, form, first=None, count=None):
        """The index list the intent spells out (ordered form), without asking the oracle."""
        first = self.early if first is None else first
        out = []
        for i in range(first, self.n if count is None else first + count):
            for t, p in enumerate(self.slot(i)[1].passes[:cap(form)]):
                if p:
                    for c in range(3 * t, 3 * t + 3):
                        out += [i, c] if form == 2 else [(i << (9 if form == 1 else 8)) | c]
        return np.array(out, dtype=np.int64).astype(np.int32)

    def clip(self, inst, p):
        """Clip coordinates of mesh-local p under instance `inst`, the way the oracle forms them: mvp = pv * world, then ((m0 x + m1 y) + m2 z) + m3."""
        import oracle

        mvp = oracle.mul_mat4(self.pv, np.ascontiguousarray(self.worlds[inst].T).reshape(-1)).reshape(4, 4)  # [col][row]
        x, y, z = (F(v) for v in p)
        return ((mvp[0] * x + mvp[1] * y) + mvp[2] * z) + mvp[3]

    def check_intent(self):
        """Every triangle of every distinct (shape, instance) is decisive and the oracle's rule agrees with what the shape means."""
        import oracle

        seen = set()
        for i in range(self.n):
            inst, s = self.slot(i)
            if (inst, s.key) in seen or s.dangling:
                continue
            seen.add((inst, s.key))
            pos = s.positions()
            for t, (tri, p) in enumerate(zip(s.corners(), s.passes)):
                cp = np.stack([self.clip(inst, pos[v]) for v in tri]).astype(F)
                a, b, c = (cp[r, [0, 1, 3]].astype(np.float64) for r in range(3))
                det = float(np.linalg.det(np.stack([a, b, c])))
                zmin = float(cp[:, 2].min())
                if p:
                    assert det <= -1.0 and zmin >= 0.5, (self.name, i, t, det, zmin)
                else:
                    assert det >= 1.0 or zmin <= -0.5, (self.name, i, t, det, zmin)
                assert (not oracle.triangle_backface(cp.reshape(-1)) and zmin >= 0.0) == p, (self.name, i, t)


def zero_pyramid(device="cpu"):
    """The pyramid of the late frames: 64 x 64, all zero -- what generate_hiz makes of an all-zero (all far, reversed Z) depth image."""
    from oxylus_amd.renderer import ImageAttachment

    return ImageAttachment.hiz(64, 64, device)


def want(fr, form=0, small=False):
    """The oracle's lists for frame `fr`, in the layout of util.gpu_frame: plain call, or early + late call where the frame has early slots."""
    import oracle
    from oxylus_amd import lib as L

    cpu, cam = fr.scene, fr.scene.cull_camera()
    mli = cpu.meshlet_instances

    def tris(vis, first, count):
        return oracle.cull_triangles(cpu, cam, mli, vis, first, count, wide=form, small_triangle_cull=small).numpy().copy()

    if not fr.early:
        vis = oracle.cull_meshlets(cpu, cam, mli)
        return {"visible": vis.numpy().copy(), "indices": tris(vis, 0, vis.numel())}
    att = zero_pyramid()
    hz = oracle.make_hiz(att.data, att.width, att.height, att.levels, att.level_offset)
    v, out, mask, res = oracle.Visibility(fr.n, 0, 0), torch.zeros(max(fr.n, 1), dtype=torch.int32), fr.mask.clone(), {}
    for tag, flags in (("early", L.CULL_TEST_ALL), ("late", L.CULL_TEST_ALL | L.CULL_LATE_PASS)):
        first = v.early if tag == "late" else 0
        emitted = oracle.cull_meshlets_hiz(cpu, cam, mli, flags, hz, v, mask, out)
        res[f"{tag}_emitted"], res[f"{tag}_visible"], res[f"{tag}_indices"] = emitted, out[first:first + emitted].numpy().copy(), tris(out, first, emitted)
    res["early"], res["late"], res["mask"] = v.early, v.late, mask.numpy().copy()
    return res


_WANT = {}


def want_cached(fr, form=0, small=False):
    """want(), computed once per (frame name, form, small) and shared: nobody writes into the result.  (Keyed by the name, which spells out every
    parameter of a frame: the cache pins no Frame.)"""
    key = (fr.name, int(form), bool(small))
    if key not in _WANT:
        _WANT[key] = want(fr, form, small)
    return _WANT[key]


# ---- a Python copy of expand_slots_wide's bookkeeping ----------------------------------------------------------------------------------------------
def expansion(counts, form, fused, base_dwords=0):
    """counts: pass count per slot of a list.  Ordered: spans of 256 slots, 64 per wave.  Fused: ONE item of up to 128 slots, 32 per wave (a list
    of at most 128 slots has one item whose base is 0, so the run positions are known).  Returns one record per wave that has slots:
    {pad0, events}, events = ('skip', k) for a zero-count slot k of the share, ('add', filled before, n3) and ('flush', pad, filled, head, nch, tail,
    why) with why = 'full' (filled + n3 > 1024) or 'end'.  The index list is taken to start on a 16-byte boundary."""
    d, share = kdw(form), 32 if fused else 64
    assert not fused or len(counts) <= FUSED_SPAN
    waves, g0 = [], base_dwords
    for w0 in range(0, len(counts), share):
        pad, filled, ev = g0 & 3, 0, []
        rec = {"pad0": pad, "events": ev, "first_slot": w0}

        def flush(why):
            nonlocal pad, filled
            head = min((4 - pad) & 3, filled)
            nch = (filled - head) >> 2
            ev.append(("flush", pad, filled, head, nch, filled - head - 4 * nch, why))
            pad, filled = (pad + filled) & 3, 0

        for k, c in enumerate(counts[w0:w0 + share]):
            n3 = c * d
            if n3 == 0:
                ev.append(("skip", k))
                continue
            if filled + n3 > EMIT_RUN:
                flush("full")
            ev.append(("add", filled, n3))
            filled += n3
            assert pad + filled <= EMIT_RUN + 8, "the LDS run of a wave holds kEmitRun + 8 dwords"
        if filled:
            flush("end")
        g0 += d * sum(counts[w0:w0 + share])
        waves.append(rec)
    return waves


def expansion_seams(counts, form, fused):
    """Names of the seams of expand_slots_wide that a list with these pass counts reaches."""
    share, d, seams = 32 if fused else 64, kdw(form), set()
    waves = expansion(counts, form, fused)
    for w in waves:
        ev = w["events"]
        kinds = [e[0] for e in ev]
        span0 = w["first_slot"] - w["first_slot"] % SPAN
        base = d * sum(counts[:span0])  # dwords in front of the wave's span: `base` of tris_emit_body (in triangles) times dwords per triangle
        if not fused and base and kinds.count("flush") == 1:
            seams.add(f"base-{base & 3}-run-{ev[kinds.index('flush')][2] // d}")
        for n, e in enumerate(ev):
            if e[0] == "flush":
                _, pad, filled, head, nch, tail, why = e
                if why == "full":
                    seams.add(f"flush-full-at-{filled}")
                    nxt = ev[n + 1]
                    seams.add(f"slot-{nxt[2]}-arrives-at-{filled}-flushes")
                total = filled // d
                if why == "end" and kinds.count("flush") == 1:
                    seams.add(f"pad-{pad}-run-{total}")
                seams |= {name for name, hit in (("head-only", head and not nch and not tail), ("head+tail", head and tail), ("nch-0", nch == 0), ("nch-1", nch == 1),
                                                 ("nch-many", nch > 1)) if hit}
            if e[0] == "add":
                if e[1] + e[2] in (1020, 1023):
                    seams.add(f"fits-to-{e[1] + e[2]}")
                if e[2] >= 128 * 3 and e[1]:  # (filled is 0 right after a flush)
                    seams.add(f"slot-{e[2]}-arrives-at-{e[1]}-fits")
        skips = [e[1] for e in ev if e[0] == "skip"]
        if skips and "add" in kinds:
            if 0 in skips:
                seams.add("zero-first")
            if share - 1 in skips:
                seams.add("zero-last")
            if any(all(k + r in skips for r in range(16)) for k in skips):
                seams.add("zeros-16-in-a-row")
            first_add = min(n for n, k in enumerate(kinds) if k == "add")
            last_add = max(n for n, k in enumerate(kinds) if k == "add")
            if any(k == "skip" for k in kinds[first_add:last_add]):
                seams.add("zero-inside-a-run")
        if "add" not in kinds and any("add" in [e[0] for e in o["events"]] for o in waves):
            seams.add("idle-wave")
    return seams


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_pass(c, boff=0):
    """c triangles, all passing, on as many vertices as fit."""
    return Shape(min(64, max(3, c + 2)), [True] * c, boff) if c else Shape(33, [], boff)


ALL_FAIL = Shape(5, [False] * 3, 1)
SMALL_SHAPES = (Shape(3, [True], 0), Shape(4, [False, True], 3), Shape(5, [False, True, True], 2), Shape(4, [True, True], 1), Shape(5, [True, False, True], 0),
                Shape(6, [False, False, True], 3), Shape(3, [True, True, True], 2))  # family A's mesh: 1 - 3 triangles, pass masks 1 2 6 3 5 4 7: neighbours differ


# ---- A: V seams ------------------------------------------------------------------------------------------------------------------------------------
A_COUNTS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def a_frame(V, late=False):
    """The first V (+ EARLY) entries of the expansion of a 7-meshlet mesh: the last visible meshlet has a pass count > 0 and its predecessor another mask."""
    K, n = len(SMALL_SHAPES), V + (EARLY if late else 0)
    return Frame(SMALL_SHAPES, instances=-(-n // K), n=n, early=EARLY if late else 0, name=f"A-{V}{'-late' if late else ''}")


# ---- B: meshlet shapes -----------------------------------------------------------------------------------------------------------------------------
B_VCOUNTS = (1, 3, 33, 64)


def b_tcounts(form):
    return (0, 1, 63, 64, 200) if form == 0 else (0, 1, 63, 64, 65, 124, 127, 128, 200)


@functools.lru_cache(maxsize=None)
def b_shapes(form):
    """Every (vertex count, T) with each boff & 3: index 4 n + b holds combination c = n + 7 b at boff (b + c) & 3.  One vertex: all fail.  Three vertices: one
    triangle, T times over.  More: pass / fail by a fixed pattern with the last triangle passing.  T = 0 with 33 or 64 vertices: dangling offsets."""
    out, combos = [], list(itertools.product(B_VCOUNTS, b_tcounts(form)))
    for n in range(len(combos)):
        for b in range(4):
            c = (n + 7 * b) % len(combos)  # (neighbours in the list differ in T: an empty meshlet sits between populated ones)
            vc, T = combos[c]
            if vc == 1:
                passes = [False] * T
            elif vc == 3:
                passes = [c % 2 == 0] * T
            else:
                passes = [(t * 7 + c) % 3 != 0 or t == T - 1 for t in range(T)]
            out.append(Shape(vc, passes, (b + c) & 3, dangling=(T == 0 and vc >= 33 and b % 2 == 0)))
    return tuple(out)


def b_rotations(form):
    return range(0, len(b_shapes(form)), 4)


B_CUTS = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def b_frame(form, r, late=False, cut=0):
    """The shapes rotated by r, less the last `cut`.  Over all rotations (steps of 4) every shape reaches pipeline slot 0 (list position 0..3 of a
    chunk) and slot 15 (60..63); with the four cuts every shape, at its own boff & 3, also ends a list that stops inside a chunk -- the slot that
    every clamped slot beyond V does again."""
    L = b_shapes(form)
    rot = list(L[r:] + L[:r])
    rot = rot[:len(rot) - cut]
    assert len(rot) % CHUNK
    early = [all_pass(2, 1)] * EARLY if late else []
    return Frame(early + rot, early=len(early), name=f"B-{form}-{r}{f'-cut{cut}' if cut else ''}{'-late' if late else ''}")


# ---- C: expansion runs -----------------------------------------------------------------------------------------------------------------------------
SPLIT = {0: [], 1: [1], 2: [1, 0, 1], 3: [3], 4: [0, 3, 1], 5: [2, 0, 0, 3]}


def c_shares(form):
    """name -> four wave shares, each a list of per-slot pass counts (the builder fills a share up with zero-count slots)."""
    f = {}
    if form == 0:
        f["run-1023"] = [[1], [64] * 5 + [21, 1, 1], [], [64] * 5 + [20, 1, 1, 1]]      # filled 1023, then a 1-triangle slot: flush at 1023 + 3
        f["run-1020"] = [[2], [64] * 5 + [20, 2], [3], [64] * 5 + [20, 1, 2]]            # filled 1020, 1020 + 6 flushes; 1020 + 3 fits, then 1023 + 6
    elif form == 1:
        f["run-1023"] = [[1], [128, 128, 85, 1, 1], [], [64] * 5 + [21, 1]]
        f["run-1020"] = [[2], [128, 128, 84, 2], [3], [128, 128, 84, 1, 2]]
        # (filled is a multiple of 3: 640 is not reached; 639 + 384 = 1023 fits, 642 + 384 flushes)
        f["slot-384"] = [[128, 85, 128, 1], [128, 86, 128], [86, 128], [3, 128, 128, 128]]
    else:
        f["run-1020"] = [[1], [128, 42, 1], [], [128, 42, 2]]                              # pairs: 170 triangles = 1020 dwords
        # (filled is a multiple of 6: 640 is not reached; 252 + 768 = 1020 fits, 258 + 768 and 636 + 768 flush)
        f["slot-768"] = [[42, 128, 1], [43, 128], [106, 128], [1, 128, 128]]
    for p in range(4):  # run lengths 1, 2, 4, 5 triangles at each start inside a 16-byte granule: 3 (p + ...) mod 4 runs through 0..3 with p
        f[f"pads-a{p}"] = [SPLIT[p], SPLIT[1], SPLIT[4], SPLIT[2]]
        f[f"pads-b{p}"] = [SPLIT[p], SPLIT[5], SPLIT[2], SPLIT[4]]
    f["masks"] = [["bit0", "bit63", "ones", "alt"] + (["bit127"] if form else []), [0] * 16 + ["ones"], ["alt", 0, "bit63"], [0, "bit0"]]
    return f


MASK_SHAPES = {"bit0": Shape(64, [True] + [False] * 63, 1), "bit63": Shape(64, [False] * 63 + [True], 2), "ones": Shape(64, [True] * 64, 3),
               "alt": Shape(33, [True, False] * 32, 0), "bit127": Shape(64, [False] * 127 + [True], 1)}


BASE_NAMES = tuple(f"base-{p}" for p in range(4))


def c_names(form):
    return list(c_shares(form)) + list(BASE_NAMES)


@functools.lru_cache(maxsize=None)
def c_frame(form, name, fused, late=False):
    """Four wave shares of 32 (fused: one item) or 64 slots (ordered: one span); zero-count filler alternates between an all-fail meshlet, an
    empty one and an empty one with dangling offsets."""
    share, slots = 32 if fused else 64, []
    filler = (ALL_FAIL, Shape(33, [], 2), Shape(64, [], 3, dangling=True))
    shares = c_shares(form).get(name)
    if name in BASE_NAMES:
        # two spans of the emit kernel (64-slot shares whatever `fused` says): the first emits 4 + p triangles, so the second span's base is not
        # zero and base * 3 mod 4 takes each value with p; its waves are runs of 1, 4, 2 and 5 triangles.  (In the fused form a second item's base
        # is the counter's value on arrival: not determined, so not pinned.)
        p, share = int(name[-1]), 64
        shares = [[2, 0, 2], SPLIT[p], [], []] + [SPLIT[1], SPLIT[4], SPLIT[2], SPLIT[5]]
    for w, sh in enumerate(shares):
        row = [MASK_SHAPES[c] if isinstance(c, str) else (filler[(w + k) % 3] if c == 0 else all_pass(c, (w + k) & 3)) for k, c in enumerate(sh)]
        assert len(row) <= share
        slots += row + [filler[(w + k) % 3] for k in range(share - len(row))]
    early = [all_pass(2, 1)] * EARLY if late else []
    return Frame(early + slots, early=len(early), name=f"C-{form}-{name}-{'fused' if fused else 'ordered'}{'-late' if late else ''}")


def c_required(form, fused=False):
    """The seams family C must reach, per index form and share size (asserted by test_tri_frames)."""
    d = kdw(form)
    pads = (0, 2) if form == 2 else (0, 1, 2, 3)  # a pair is six dwords: a run of pairs starts on an even dword
    need = {f"pad-{p}-run-{n}" for p in pads for n in (1, 2, 4, 5)}
    need |= {"head+tail", "nch-1", "nch-many"} | (set() if form == 2 else {"head-only", "nch-0"})  # (six dwords never fit into a head of at most three)
    need |= {"zero-first", "zero-last", "zeros-16-in-a-row", "zero-inside-a-run", "idle-wave"}
    if form == 0:
        need |= {"flush-full-at-1023", "flush-full-at-1020", "fits-to-1023", "fits-to-1020"}
    elif form == 1:
        need |= {"flush-full-at-1023", "flush-full-at-1020", "fits-to-1023", "fits-to-1020", "slot-384-arrives-at-639-fits", "slot-384-arrives-at-642-flushes",
                 "slot-384-arrives-at-258-fits"}
    else:
        need |= {"flush-full-at-1020", "fits-to-1020", "slot-768-arrives-at-252-fits", "slot-768-arrives-at-258-flushes", "slot-768-arrives-at-636-flushes"}
    if not fused:  # a second span: a base that is not zero, at every residue of base * dwords-per-triangle mod 4
        need |= {f"base-{b}-run-{n}" for b in pads for n in (1, 2, 4, 5)} if form != 2 else {f"base-{b}-run-1" for b in pads}
    assert d in (3, 6)
    return need


# ---- D: work distribution --------------------------------------------------------------------------------------------------------------------------
def d_fused_counts(C):
    return (128 * C, 128 * C + 1, 128 * C + 65, 128 * C + 64 * 17, 256 * C - 64, 256 * C - 63, 256 * C + 1)


def d_ordered_counts(C):
    return (64 * C + 1, 256 * C + 1)  # the second iteration of tris_test_body's (64-slot chunks) and of tris_emit_body's (256-slot spans) grid-stride loop


D_ONE, D_TWO = Shape(3, [True], 0), Shape(4, [True, True], 3)


def d_marked(i):
    return i % 251 == 7  # the few slots with two triangles: one in every span of 256


@functools.lru_cache(maxsize=None)
def d_frame(V):
    """V meshlets of one passing triangle, a marked few of two: an item lost or run twice changes the list."""
    return Frame([D_TWO if d_marked(i) else D_ONE for i in range(V)], name=f"D-{V}")


def ticket_count(V):
    """TriTestArgs::ticket_count as the host sets it: one accumulator per 64 chunks of the list."""
    chunks = -(-V // CHUNK)
    return max(-(-chunks // CHUNKS_PER_SUPER), 1)


def fused_items(V, grid, tickets, pick=None):
    """tris_fused_body's item sequence.  Returns (static_chunks, Kc, handed): handed = every chunk index < nchunks that some block was given, in the
    order the blocks took them.  pick(ready) chooses which of the running blocks takes its next step (default: the lowest): the arrival order.
    This is a transcription of the kernel's loop, not an independent reference: it proves that the ALGORITHM hands every chunk out once under any
    arrival order; that the kernel still implements it is what the set comparison of the family-D frames on the GPU shows."""
    nchunks = -(-V // CHUNK)
    nspans = -(-nchunks // 2)
    static_chunks = min(max(1, nspans // grid) * grid * 2, nchunks)
    Kc = max(1, min(TICKET_COUNTERS, grid, tickets))
    counters, handed = [0] * Kc, []
    state = {b: (b * 2, 2) for b in range(grid) if b * 2 < nchunks}
    while state:
        b = min(state) if pick is None else pick(sorted(state))
        item, item_n = state[b]
        handed += [c for c in range(item, item + item_n) if c < nchunks]
        next_static = item + grid * 2
        if static_chunks < nchunks and (item_n < 2 or next_static >= static_chunks):
            kx = b % Kc
            tk, counters[kx] = counters[kx], counters[kx] + 1
            item, item_n = static_chunks + tk * Kc + kx, 1
        else:
            item = nchunks if next_static >= static_chunks else next_static
        if item < nchunks:
            state[b] = (item, item_n)
        else:
            del state[b]
    return static_chunks, Kc, handed


# ---- E: rule thresholds ----------------------------------------------------------------------------------------------------------------------------
T0001 = F(0.0001)
MIN_NORMAL = float(np.finfo(F).tiny)
NEG0_PV = np.eye(4, dtype=F)  # [col][row]: row 2 of the matrix is (-0, -0, 1, -0), so that a sum of nothing but negative zeros stays -0
NEG0_PV[0, 2] = NEG0_PV[1, 2] = NEG0_PV[3, 2] = -0.0


def _diag(kx=1.0, kz=1.0, neg0_row2=False):
    m = np.eye(4, dtype=F)
    m[0, 0], m[2, 2] = kx, kz
    if neg0_row2:
        m[2, 0] = m[2, 1] = m[2, 3] = -0.0
    return m


class _Raw(Shape):
    """A meshlet given by its positions and corner triples."""

    def __init__(self, pos, tris, passes):
        self._pos, self._tris = [tuple(float(c) for c in p) for p in pos], [tuple(t) for t in tris]
        self.vcount, self.passes, self.boff, self.dangling = len(pos), tuple(passes), 0, False
        self.key = ("raw", tuple(self._pos), tuple(self._tris))

    def positions(self):
        return self._pos

    def corners(self):
        return self._tris


def e_plain_cases():
    """(name, mesh instance, record, kept?, inside the oracle's boundary band?, the decision in words).  Triangle (0, 0), (1, 0), (0, 1) under
    diag(k, 1, 1): a = (0, 0, 1), b = (k, 0, 1), c = (0, 1, 1), so the determinant is 1 * (k * 1 - 0 * 0) = k in every evaluation order."""
    below, above = float(np.nextafter(T0001, F(0))), float(np.nextafter(T0001, F(1)))
    return [
        ("det-threshold", 0, 0, False, True, "det == 0.0001f: `det >= 0.0001f` holds, dropped"),
        ("det-below", 1, 0, True, True, "det one ulp below 0.0001f: kept"),
        ("det-above", 2, 0, False, True, "det one ulp above 0.0001f: dropped"),
        ("det-zero", 3, 0, True, False, "det == 0 (degenerate): kept"),
        ("det-negative", 4, 0, True, False, "det == -0.0001f: kept"),
        ("z-plus-zero", 5, 1, True, True, "clip.z of one corner +0.0: `z >= 0` holds, kept"),
        ("z-minus-zero", 6, 2, True, True, "clip.z of one corner -0.0 (matrix row 2 all negative zeros): -0 >= 0 holds, kept"),
        ("z-largest-negative-normal", 7, 3, False, False, "clip.z of one corner -FLT_MIN, the others +FLT_MIN: dropped"),
        ("z-min-normal", 7, 4, True, False, "clip.z of every corner +FLT_MIN: kept"),
    ], [_diag(float(T0001)), _diag(below), _diag(above), _diag(0.0), _diag(-float(T0001)), _diag(), _diag(neg0_row2=True), _diag(kz=MIN_NORMAL)]


@functools.lru_cache(maxsize=None)
def e_plain_frame():
    cases, worlds = e_plain_cases()
    cw = [(0, 2, 1)]  # the kept orientation: det = -1
    records = [_Raw([(0, 0, .5), (1, 0, .5), (0, 1, .5)], [(0, 1, 2)], [False]),
               _Raw([(0, 0, 0.0), (1, 0, .5), (0, 1, .5)], cw, [True]),
               _Raw([(0, 0, -0.0), (1, 0, .5), (0, 1, .5)], cw, [True]),
               _Raw([(0, 0, -1.0), (1, 0, 1.0), (0, 1, 1.0)], cw, [False]),
               _Raw([(0, 0, 1.0), (1, 0, 1.0), (0, 1, 1.0)], cw, [True])]
    # (under small_triangle_cull the same frame runs at 4096 x 4096: the det cases are 0.2-px triangles and go, the z cases span 2048 px and stay)
    return Frame(records, instances=len(worlds), worlds=worlds, pv=NEG0_PV.reshape(-1).tolist(), pairs=[(c[1], c[2]) for c in cases], name="E-plain")


def e_small_pv(W, H):
    """clip.xy as raster_frames.pixel_pv (screen = the world's x, y in pixels, exactly, for coordinates of few bits), clip.z = 0.5, clip.w = the position's z."""
    pv = np.zeros((4, 4), dtype=F)  # [col][row]
    pv[0, 0], pv[1, 1] = F(2.0) / F(W), F(2.0) / F(H)
    pv[2, 0] = pv[2, 1] = -1.0  # the -1 rides on w: x' = 2 X / W * 1 - 1 * pz
    pv[3, 2] = 0.5
    pv[2, 3] = 1.0
    return pv.reshape(-1).tolist()


def e_small_cases():
    """(name, three (X, Y, w) corners in pixels of a 64 x 64 image, kept under small_triangle_cull?, words).  All are kept orientations two pixel
    rows tall or more, so only the x extent (or w) decides; without the small-triangle cull every one is kept."""
    d = 1.0 / 256
    return [
        ("lo-on-centre", [(2.5, 1, 1), (2.5, 9, 1), (3.5 - d, 1, 1)], False, "lo on the centre 2.5, hi just below 3.5: floor(lo + .5) == floor(hi + .5), covers no further centre -- dropped"),
        ("hi-on-centre", [(2.5 - d, 1, 1), (2.5 - d, 9, 1), (2.5, 1, 1)], True, "lo just below 2.5, hi on it: floors 2 and 3 differ -- kept"),
        ("lo-eq-hi", [(2.5, 1, 1), (2.5, 9, 1), (2.5, 5, 1)], False, "lo == hi on a centre (det == 0 passes the backface test): floors equal -- dropped"),
        ("w-zero", [(2.75, 1, 1), (2.75, 9, 1), (3.0, 1, 0)], True, "one corner with w == 0: `!(w > 0)`, the small-triangle test does not apply -- kept"),
        ("w-negative", [(2.75, 9, 1), (2.75, 1, 1), (3.0, 1, -1)], True, "one corner with w < 0 and z >= 0: the small-triangle test does not apply -- kept"),
    ]


@functools.lru_cache(maxsize=None)
def e_small_frame():
    records = [_Raw([(x * (w if w else 1), y * (w if w else 1), w) for x, y, w in tri], [(0, 1, 2)], [True]) for _, tri, _, _ in e_small_cases()]
    return Frame(records, pv=e_small_pv(64, 64), worlds=[np.eye(4, dtype=F)], resolution=(64, 64), name="E-small")
