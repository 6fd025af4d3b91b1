"""The fixtures of bounds_frames, held against the C checker on the CPU: each one reaches what it was built for (floors asserted through
the checker's output), every signed-zero case gives the hand-stated bits, and the checker's boxes agree with an independent numpy
restatement of the fold."""
import functools

import numpy as np
import pytest

import bounds_frames as BF

FMAX = np.float32(3.402823466e+38)


@functools.lru_cache(maxsize=None)
def _frames():
    f = {"count_ladder": BF.count_ladder(), "cone_thresholds": BF.cone_thresholds(), "many_small(3001)": BF.many_small(3001)}
    f.update({"signed_zeros/" + k: v for k, v in BF.signed_zeros().items()})
    f.update({"edge_values/" + k: v for k, v in BF.edge_values().items()})
    return f


FRAME_NAMES = ["count_ladder", "cone_thresholds", "many_small(3001)"] + ["signed_zeros/" + k for k in ("meshlets", "mesh_first_plus", "mesh_first_minus", "mesh_late_plus", "mesh_late_minus", "mesh_alternating")] + [
    "edge_values/" + k for k in ("huge", "tiny", "fltmax", "nan", "posinf", "neginf", "bothinf", "half_bounds")]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    import oracle

    oracle.build()
    b, m6, q = oracle.build_meshlet_bounds(*_frames()[name].args())
    return b.numpy().view(np.uint16), m6.numpy().view(np.uint32), q.numpy().view(np.uint16)


def _cone(rec):
    """(axis x, y, z, cutoff) as int8 of records u16 [M, 8]."""
    return np.stack([rec[:, 3] & 0xFF, rec[:, 3] >> 8, rec[:, 7] & 0xFF, rec[:, 7] >> 8], axis=1).astype(np.uint8).view(np.int8)


def test_the_frame_list_is_complete():
    assert sorted(FRAME_NAMES) == sorted(_frames())


# ---- the fixtures reach what they were built for ---------------------------------------------------------------------------------------------------
def test_cone_thresholds_has_both_sides_of_every_decision():
    f = _frames()["cone_thresholds"]
    cone = _cone(_oracle("cone_thresholds")[0])
    axis0 = (cone[:, :3] == 0).all(axis=1)
    cut = cone[:, 3]
    # mindp exactly 0.1f and the float below it: `<=` gives cutoff 127 and no axis; the float above it: a real cone (which the clamp caps)
    for i in f.info["below"] + f.info["exact"]:
        assert cut[i] == 127 and axis0[i], (i, cone[i])
    for i in f.info["above"]:
        assert cut[i] == 127 and not axis0[i], (i, cone[i])
    for key in ("sweep2", "sweep3"):
        ids = f.info[key]
        wide = sum(1 for i in ids if cut[i] == 127 and axis0[i])
        assert wide >= 5 and len(ids) - wide >= 5, (key, wide)
        assert all(cut[i] > 0 for i in ids)
    # the clamp: cutoff 127 WITH an axis.  Generic axes carry s8 errors of about 0.002 each, and at mindp just above 0.1 the sum passes 1.
    near = f.info["near_limit"]
    assert all(not axis0[i] for i in near)
    assert sum(1 for i in near if cut[i] == 127) >= 48
    for i in f.info["opposite"]:  # centre 0: axis length 0, mindp 0
        assert cut[i] == 127 and axis0[i], (i, cone[i])
    for i in f.info["identical"]:  # a cone of no opening: only the s8 errors remain
        assert 0 < cut[i] <= 3 and not axis0[i], (i, cone[i])


def test_count_ladder_zero_cones_are_the_empty_and_degenerate_meshlets():
    f = _frames()["count_ladder"]
    cone = _cone(_oracle("count_ladder")[0])
    assert sorted(f.info["counts"]) == sorted(BF.LADDER_COUNTS)
    none = set(f.info["empty"] + f.info["all_degenerate"])
    assert len(f.info["empty"]) == 2 and len(f.info["all_degenerate"]) == 2
    for i in range(len(cone)):
        if i in none:
            assert (cone[i] == 0).all(), (i, cone[i])
        else:
            assert cone[i, 3] > 0, (i, cone[i])
    tc = f.meshlets[:, 3].tolist()
    assert [tc[i] for i in f.info["all_degenerate"]] == [5, 70] and max(tc) == 300
    assert all(o % 4 == 0 for o in f.meshlets[:, 1].tolist())


@pytest.mark.parametrize("name", [n for n in FRAME_NAMES if n.startswith("signed_zeros/")])
def test_signed_zero_cases_give_the_stated_bits(name):
    f = _frames()[name]
    rec, mesh6, _ = _oracle(name)
    seen = set()
    for i, kind in enumerate(f.info["first"]):
        if kind is None:  # an empty meshlet: the FLT_MAX fold
            assert rec[i, 0] == 0x0000 and rec[i, 4] == 0xFC00
            continue
        want = BF.ZERO_BITS[kind]
        assert rec[i, 0] == want["centre_half"] and rec[i, 4] == want["extent_half"], (i, kind, hex(rec[i, 0]), hex(rec[i, 4]))
        seen.add(kind)
    assert seen == {"p", "n"}
    want = BF.ZERO_BITS[f.info["mesh_first"]]
    assert mesh6[0] == want["centre_f32"] and mesh6[3] == want["extent_f32"], (hex(mesh6[0]), hex(mesh6[3]))


def test_nan_normals_give_the_stated_cone_bytes():
    """include/oxcull.h: a NaN axis component is stored as -127 and the cutoff is then 0."""
    hits = 0
    for name in ("edge_values/huge", "edge_values/nan"):
        cone = _cone(_oracle(name)[0])
        nan_axis = (cone[:, :3] == -127).any(axis=1) & (cone[:, 3] == 0)
        hits += int(nan_axis.sum())
        assert nan_axis.any(), name
    assert hits >= 4


def test_many_small_records_differ_across_the_chunk_seam():
    """What makes an `out[k]` for `out[first + k]` visible: the records behind the seam are not those at the front."""
    import oracle

    f = BF.many_small((1 << 18) + 5)
    b = oracle.build_meshlet_bounds(*f.args())[0].numpy()
    tail, head = b[1 << 18:], b[:5]
    assert len(tail) == 5 and all((tail[k] != head[k]).any() for k in range(5))
    assert len(np.unique(b[:4096], axis=0)) > 2000


# ---- the checker's boxes against an independent restatement ----------------------------------------------------------------------------------------
def _first_extreme(vals, init, smallest):
    """The value `b < a ? b : a` (or `a < b ? b : a`) leaves after folding vals into init, stated without the loop: NaNs never win a
    compare; among the rest the extreme value; and where several elements compare equal to it -- +0.0 and -0.0, or repeats -- the FIRST
    one, init included, because an equal element never replaces the kept one."""
    v = np.concatenate([[init], vals]).astype(np.float32)
    ok = ~np.isnan(v)
    e = v[ok].min() if smallest else v[ok].max()
    return v[np.flatnonzero(ok & (v == e))[0]]


def _half(x):
    """meshopt_quantizeHalf on float32 arrays, by its published integer steps."""
    ui = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    s, em = (ui >> 16) & 0x8000, ui & 0x7FFFFFFF
    h = (em - (112 << 23) + (1 << 12)) >> 13
    h = np.where(em < (113 << 23), 0, h)
    h = np.where(em >= (143 << 23), 0x7C00, h)
    h = np.where(em > (255 << 23), 0x7E00, h)
    return (s | h).astype(np.uint16)


@pytest.mark.parametrize("name", FRAME_NAMES)
def test_boxes_match_the_numpy_restatement(name):
    f = _frames()[name]
    rec, mesh6, qpos = _oracle(name)
    P, ml, vidx, micro = f.positions.numpy(), f.meshlets.numpy(), f.vidx.numpy(), f.micro.numpy()
    lo = np.empty((len(ml), 3), np.float32)
    hi = np.empty((len(ml), 3), np.float32)
    for i, (vo, to, _, tc) in enumerate(ml.tolist()):
        corners = P[vidx[vo + micro[to:to + 3 * tc].astype(np.int64)]]  # every triangle, also beyond the cone's 256
        for c in range(3):
            lo[i, c] = _first_extreme(corners[:, c], FMAX, True)
            hi[i, c] = _first_extreme(corners[:, c], -FMAX, False)
    with np.errstate(all="ignore"):
        centre, extent = (hi + lo) * np.float32(0.5), hi - lo
        assert np.array_equal(_half(centre), rec[:, 0:3]) and np.array_equal(_half(extent), rec[:, 4:7])
        mlo = np.array([_first_extreme(lo[:, c], FMAX, True) for c in range(3)], np.float32)
        mhi = np.array([_first_extreme(hi[:, c], -FMAX, False) for c in range(3)], np.float32)
        want6 = np.concatenate([(mhi + mlo) * np.float32(0.5), mhi - mlo]).astype(np.float32).view(np.uint32)
    assert np.array_equal(want6, mesh6), ([hex(v) for v in want6], [hex(v) for v in mesh6])
    assert np.array_equal(qpos[:, :3], _half(P)) and (qpos[:, 3] == 0).all()
