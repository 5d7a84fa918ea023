"""CPU tests of the two 4-wide device formats and of the exact model the GPU tests hold the 4-wide kernels to.

The product's host half (collapseWide, quantiseWide: racc_host_scene_wide_nodes, the code racc_hip_scene_upload runs) against
oracle/racc_oracle_wide.c byte for byte; the records' structure and the conservative, tight quantisation from numpy and exact rational
arithmetic alone; the model's traversal against the binary oracle; and a scene in which the visiting rule itself shows."""
from fractions import Fraction

import numpy as np
import pytest

import rayaccel_amd as ra
from oracle import oracle as orc
from rayaccel_amd import engine, synth
from helpers import MISS, assert_same_closest_hit, comb_scene, frame_scene, leaf_scene, make_rays, tie_scene, wide_model

INNER = 0x80000000


def area_scene():
    """Two inner candidates whose surface areas differ in double (27 - 5.7e-14 against 27) and are EQUAL in binary32: after the root's inner
    child has been opened there is room for one more, and the collapse (double areas, first among equals) must open the second one."""
    e = np.float32(3.0) + np.spacing(np.float32(3.0)), np.float32(3.0) - np.spacing(np.float32(3.0))
    nodes = np.zeros(4, orc.GPU_NODE_DTYPE)
    nodes["kind"] = 1
    nodes[0]["first"], nodes[0]["last"] = INNER | 1, (1 << 24) | 4
    nodes[0]["leftMin"], nodes[0]["leftMax"], nodes[0]["rightMin"], nodes[0]["rightMax"] = (0, 0, 0), (8, 8, 8), (9, 0, 0), (10, 1, 1)
    nodes[1]["first"], nodes[1]["last"] = INNER | 2, INNER | 3
    nodes[1]["leftMin"], nodes[1]["leftMax"] = (0, 0, 0), (e[0], 3, e[1])              # 27 - e^2 in double, 27 in binary32
    nodes[1]["rightMin"], nodes[1]["rightMax"] = (4, 4, 4), (7, 7, 7)                  # 27
    for n, k in ((2, 0), (3, 2)):
        nodes[n]["first"], nodes[n]["last"] = (1 << 24) | k, (1 << 24) | (k + 1)
        lo = np.array(nodes[1]["leftMin" if n == 2 else "rightMin"])
        nodes[n]["leftMin"], nodes[n]["leftMax"], nodes[n]["rightMin"], nodes[n]["rightMax"] = lo, lo + 1, lo + 1, lo + 2
    pairs = np.zeros(32, orc.PAIR_DTYPE)
    pairs[:] = leaf_scene(1)[0]["pairs"][0]
    return dict(nodes=nodes, pairs=pairs, remap=np.arange(10, dtype=np.uint32), pair_count=5)


def tiny_meshes():
    """The tiny meshes of tests/test_host_build.py::test_device_node_order_on_degenerate_trees."""
    rng = np.random.default_rng(1)
    for tris in (6, 9, 17, 40, 131):
        centres = np.repeat(rng.uniform(-10, 10, (tris, 3)), 3, axis=0)
        v = np.concatenate([(centres + rng.uniform(-0.3, 0.3, (tris * 3, 3))).astype(np.float32), np.ones((tris * 3, 1), np.float32)], 1)
        yield "mesh of %d triangles" % tris, ra.HostScene(v, np.arange(tris * 3, dtype=np.uint32).reshape(tris, 3)).blobs()


@pytest.fixture(scope="module")
def shapes(small_host, small_default_host):
    out = {"small": small_host.blobs(), "small, library default tree": small_default_host.blobs(), "comb": comb_scene(40),
           "single inner node": leaf_scene(3)[0], "tie scene": tie_scene()[0], "areas equal in binary32": area_scene()}
    out.update(tiny_meshes())
    for kind in ("flat_z", "point", "one_ulp", "huge"):
        out["frame " + kind] = frame_scene(kind)[0]
    return out


def _product(blobs, fmt):
    return engine.wide_nodes(blobs["nodes"], len(blobs["pairs"]), len(blobs["remap"]), fmt)


def test_model_records_equal_the_products(shapes):
    """orc_collapse_wide / orc_quantise_wide against the records racc_host_scene_wide_nodes returns — the very collapseWide and quantiseWide
    that upload runs: every byte of the 128 B and of the 64 B records, their number and the stack bound."""
    for name, blobs in shapes.items():
        wide, bound = _product(blobs, 45)
        packed, bound_q = _product(blobs, 50)
        m_wide, m_bound = orc.collapse_wide(blobs["nodes"])
        rc, m_packed = orc.quantise_wide(m_wide)
        assert rc == 0 and bound == bound_q == m_bound, "%s: stack bound %d / %d, model %d" % (name, bound, bound_q, m_bound)
        assert wide.shape == m_wide.shape and packed.shape == m_packed.shape == (len(wide), 16), name
        bad = np.nonzero((wide != m_wide).any(1))[0]
        assert len(bad) == 0, "%s: 128 B records %s differ, e.g.\n%s\n%s" % (name, bad[:4], wide[bad[0]], m_wide[bad[0]])
        bad = np.nonzero((packed != m_packed).any(1))[0]
        assert len(bad) == 0, "%s: 64 B records %s differ, e.g.\n%s\n%s" % (name, bad[:4], packed[bad[0]], m_packed[bad[0]])
    wide = _product(shapes["areas equal in binary32"], 45)[0]
    assert wide[0, 0] == INNER | 1 and list(wide[0, 1:4]) == [(1 << 24) | 2, (1 << 24) | 3, (1 << 24) | 4]      # the SECOND candidate (27 > 27 - e^2) was opened


def test_refusals(shapes):
    """A frame whose extent overflows binary32 and a child box that is not finite: refused for the compressed format with the codes the header
    names, by the product and by the model alike; the 128 B format holds both."""
    for kind, code in (("overflow", -4), ("nonfinite", -1)):      # RACC_HIP_ERR_LIMIT, RACC_HIP_ERR_INVALID
        blobs = frame_scene(kind)[0]
        wide, _ = _product(blobs, 45)
        assert np.array_equal(wide, orc.collapse_wide(blobs["nodes"])[0])
        with pytest.raises(ra.RaccError) as e:
            _product(blobs, 50)
        assert e.value.code == code, (kind, e.value.code)
        assert orc.quantise_wide(wide)[0] == code
    with pytest.raises(ra.RaccError):
        _product(shapes["small"], 47)                                    # not a format
    bad = shapes["small"]["nodes"].copy()
    bad[5]["first"] = INNER | 3                                           # a node referenced twice: validateScene's refusal, as for upload
    with pytest.raises(ra.RaccError):
        engine.wide_nodes(bad, len(shapes["small"]["pairs"]), len(shapes["small"]["remap"]), 45)


def test_record_structure(shapes):
    """From numpy alone, on the product's records: every BVH2 leaf ref sits in exactly one used slot and every wide node but the root is referenced
    once; the numbering is breadth first; every used box of the 128 B format is bit-equal to a box of the blob; unused slots are what the
    header says (+inf planes / lower 255, upper 0; the ref of a real leaf); both formats carry the same refs."""
    for name, blobs in shapes.items():
        wide, bound = _product(blobs, 45)
        packed, _ = _product(blobs, 50)
        n = len(wide)
        used = wide[:, 28]
        assert ((used >= 2) & (used <= 4)).all() and not wide[:, 29:].any(), name
        slot_used = np.arange(4)[None, :] < used[:, None]
        refs = wide[:, :4]
        assert np.array_equal(refs, packed[:, :4]), name
        kids = np.concatenate([blobs["nodes"]["first"], blobs["nodes"]["last"]])
        leaves = np.sort(kids[(kids & INNER) == 0])
        got_leaves = refs[slot_used & ((refs & INNER) == 0)]
        assert np.array_equal(np.sort(got_leaves), leaves), "%s: the used slots do not hold every leaf ref exactly once" % name
        inner = refs[slot_used & ((refs & INNER) != 0)] & 0x7FFFFFFF
        assert np.array_equal(inner, np.arange(1, n)), "%s: inner refs are not 1 .. N-1 in record and slot order (breadth first, each once)" % name
        first_leaf = blobs["nodes"]["first"][0] if not (blobs["nodes"]["first"][0] & INNER) else 0x01000000
        assert (refs[~slot_used] == first_leaf).all(), name
        planes = wide[:, 4:28].reshape(n, 6, 4)
        assert (planes.transpose(0, 2, 1)[~slot_used] == np.float32(np.inf).view(np.uint32)).all(), name
        # every used box, as (lo.x lo.y lo.z hi.x hi.y hi.z) words, is a child box of the blob (an inverted one as its mirror image)
        bn = blobs["nodes"]
        def boxes(mn, mx):
            return np.concatenate([np.minimum(bn[mn], bn[mx]), np.maximum(bn[mn], bn[mx])], 1).astype(np.float32).view(np.uint32)
        blob_boxes = {(int(r),) + tuple(int(w) for w in b) for r, b in zip(kids, np.concatenate([boxes("leftMin", "leftMax"), boxes("rightMin", "rightMax")]))}
        fl = planes.transpose(0, 2, 1)[slot_used]                       # [used slots, 6]: lo.x hi.x lo.y hi.y lo.z hi.z
        leaf_slot = (refs[slot_used] & INNER) == 0
        for r, b in zip(refs[slot_used][leaf_slot], fl[leaf_slot]):     # (leaf refs keep their value: ref and box must belong together)
            assert (int(r),) + tuple(int(w) for w in b[[0, 2, 4, 1, 3, 5]]) in blob_boxes, "%s: a leaf slot's box is not the blob's" % name
        only_boxes = {b[1:] for b in blob_boxes}
        for b in fl[~leaf_slot]:
            assert tuple(int(w) for w in b[[0, 2, 4, 1, 3, 5]]) in only_boxes, "%s: an inner slot's box is not a box of the blob" % name
        q = packed[:, 10:16].view(np.uint8).reshape(n, 6, 4).transpose(0, 2, 1)      # [node, slot, plane]
        assert (q[~slot_used][:, 0::2] == 255).all() and (q[~slot_used][:, 1::2] == 0).all(), name
        # the stack bound: three entries per level of the longest path + 1
        depth = np.zeros(n, np.int64)
        depth[0] = 1
        for i in range(n):
            for r in refs[i][slot_used[i]]:
                if r & INNER:
                    depth[r & 0x7FFFFFFF] = depth[i] + 1
        assert bound == 3 * depth.max() + 1, name


def _round_to_binary32(x):
    """The binary32 value nearest to the rational x (ties to even) — ONE rounding, found exactly."""
    c = np.float32(float(x))
    cands = {float(c), float(np.nextafter(c, np.float32(-np.inf))), float(np.nextafter(c, np.float32(np.inf)))}
    cands = [v for v in cands if np.isfinite(v)]
    def key(v):
        return (abs(Fraction(v) - x), int(np.float32(v).view(np.uint32)) & 1)
    return np.float32(min(cands, key=key))


@pytest.mark.parametrize("shape", ["small", "tie scene", "frame flat_z", "frame point", "frame one_ulp", "frame huge"])
def test_quantisation_is_conservative_and_tight(shapes, shape):
    """Independent of C's fmaf: for every used plane of the compressed format the exact rational byte * scale + origin, rounded ONCE to
    binary32, is what the model decodes; it lies on the outer side of the blob's plane (lower <=, upper >=); the next byte inwards would
    not (except at 255 / 0); and the frame reaches the children's upper corner."""
    blobs = shapes[shape]
    wide, _ = _product(blobs, 45)
    packed, _ = _product(blobs, 50)
    decoded = orc.decode_wide(packed, 50)
    assert np.array_equal(orc.decode_wide(wide, 45).view(np.uint32), wide[:, 4:28].reshape(-1, 6, 4))
    ref = wide[:, 4:28].view(np.float32).reshape(-1, 6, 4)
    org, scl = packed[:, 4:7].view(np.float32), packed[:, 7:10].view(np.float32)
    q = packed[:, 10:16].view(np.uint8).reshape(-1, 6, 4)
    assert np.isfinite(org).all() and np.isfinite(scl).all() and (scl > 0).all()
    checked = 0
    for n in range(len(packed)):
        used = int(wide[n, 28])
        for p in range(6):
            a, upper = p >> 1, p & 1
            s, o = Fraction(float(scl[n, a])), Fraction(float(org[n, a]))
            dec = lambda byte: _round_to_binary32(byte * s + o)
            if upper:
                assert dec(255) >= ref[n, p, :used].max(), "node %d axis %d: the frame does not reach the upper corner" % (n, a)
            for i in range(4):
                b = int(q[n, p, i])
                d = dec(b)
                assert d.view(np.uint32) == decoded[n, p, i].view(np.uint32) or d == decoded[n, p, i] == 0, \
                    "node %d plane %d slot %d: byte %d decodes to %r in one rounding, the model says %r" % (n, p, i, b, d, decoded[n, p, i])
                if i >= used:
                    continue
                checked += 1
                if upper:
                    assert d >= ref[n, p, i], "node %d plane %d slot %d: decoded %r is inside the box (%r)" % (n, p, i, d, ref[n, p, i])
                    assert b == 0 or dec(b - 1) < ref[n, p, i], "node %d plane %d slot %d: byte %d is not the smallest that holds %r" % (n, p, i, b, ref[n, p, i])
                else:
                    assert d <= ref[n, p, i], "node %d plane %d slot %d: decoded %r is inside the box (%r)" % (n, p, i, d, ref[n, p, i])
                    assert b == 255 or dec(b + 1) > ref[n, p, i], "node %d plane %d slot %d: byte %d is not the largest that holds %r" % (n, p, i, b, ref[n, p, i])
    assert checked >= 12


def test_a_point_frame_enters_its_unused_slots(shapes):
    """A frame without extent on any axis: in the compressed format the unused slots (lower 255, upper 0) decode to the same point as the used
    ones, so a ray through that point ENTERS them — four leaf visits, not two — and lands on real geometry: they hold the ref of a real leaf.
    The 128 B format keeps them out (+inf planes).  A model that skipped unused slots by their ref would count two."""
    blobs, rays = frame_scene("point")
    through = rays[:1]
    ref = orc.traverse(blobs, through)
    for fmt, tests in ((45, 2), (50, 4)):
        records, _ = _product(blobs, fmt)
        res, depth, c = orc.traverse_wide(records, fmt, blobs, through)
        assert c["node_visits"] == 1 and c["pair_tests"] == tests and depth[0] == tests - 1, (fmt, c)
        assert res["triangle"][0] == 0 and res["t"][0] == 5.0 and res.tobytes() == ref.tobytes()
    records, _ = _product(blobs, 50)
    assert (records[0, 2:4] == records[0, 0]).all() and (np.abs(orc.decode_wide(records, 50)) <= 255 * np.finfo(np.float32).tiny).all()      # (scale = the smallest normal: a distance absorbs it)
    res, _, c = orc.traverse_wide(records, 50, blobs, rays)
    assert c["pair_tests"] == 4 * int((res["triangle"] != MISS).sum()) > 0      # every ray through the point enters all four slots, every other ray none


def _arbiter_of_lone_pairs(blobs):
    """Vertices and indices of a blob whose pairs are all unpaired triangles with remap[2k] = k (comb_scene, tie_scene)."""
    p = blobs["pairs"][:blobs["pair_count"]]
    v = np.stack([p["p0"], p["p0"] - p["e1"], p["p0"] + p["e2"]], 1).reshape(-1, 3).astype(np.float32)
    return dict(vertices=np.concatenate([v, np.ones((len(v), 1), np.float32)], 1), indices=np.arange(len(v), dtype=np.uint32).reshape(-1, 3))


@pytest.fixture(scope="module")
def batch(small_scene):
    return np.concatenate([synth.primary_rays(small_scene["camera"], 128, 128)[0], synth.random_rays(6000, seed=3, ymax=30.0)])


@pytest.mark.parametrize("fmt", [45, 50])
@pytest.mark.parametrize("tree", ["small", "small, library default tree", "comb"])
def test_model_traversal_against_the_binary_oracle(shapes, small_scene, batch, tree, fmt):
    """The model on the product's records against the binary oracle, one 128 x 128 tile of primaries (synth.primary_rays hands out whole
    tiles only: 96 x 96 would be no ray at all) + 6000 random rays (the comb: 64 rays down its axis as well): the oracle's closest hit under
    tests/helpers.py::assert_same_closest_hit with the brute-force arbiter; no ray's stack deeper than the stack bound; the comb deeper than
    15 levels (40: the kernels' LDS levels do spill on it).  Counted — records that differ from the binary oracle, of 22,384 (comb: 22,448),
    as ties / closer hits / aliases:
        small (reference builder's tree)   format 45: 0 / 0 / 0     format 50: 0 / 0 / 0
        small (library default tree)       format 45: 0 / 0 / 2     format 50: 0 / 0 / 2
        comb                               format 45: 0 / 0 / 0     format 50: 0 / 0 / 0
    (an alias: a triangle that spatial splits put into two leaves, met through its other reference).  The compressed format visits 0.7 %
    more nodes and tests 0.4 - 0.5 % more pairs than the 128 B one on the two small trees."""
    blobs = shapes[tree]
    if tree == "comb":
        o = np.stack([np.linspace(-20, 20, 64), np.linspace(-15, 15, 64), np.full(64, -10.0)], 1)
        rays, env, arbiter = np.concatenate([make_rays(o, [[0, 0, 1]] * 64), batch]), None, _arbiter_of_lone_pairs(blobs)
    else:
        rays, env, arbiter = batch, small_scene["env"], dict(vertices=small_scene["vertices"], indices=small_scene["indices"])
    ref = orc.traverse(blobs, rays, env=env)
    res, depth, c, bound = wide_model(blobs, fmt, rays, env=env)
    print("%s, format %d: %d rays, %s, stack bound %d" % (tree, fmt, len(rays), c, bound))
    differ = assert_same_closest_hit(res, ref, "%s, format %d" % (tree, fmt), arbiter=dict(arbiter, rays=rays))
    assert c["others"] == 0 and c["ties"] + c["closer"] == differ and c["differ"] == differ + c["aliases"]
    assert depth.max() == c["max_depth"] <= bound
    assert c["node_visits"] > len(rays) // 2 and c["pair_tests"] > 0
    if tree == "comb":
        assert depth.max() > 15
    single, depth1, _ = orc.traverse_wide(_product(blobs, fmt)[0], fmt, blobs, rays, env=env, threads=1, compare=False)
    assert single.tobytes() == res.tobytes() and np.array_equal(depth, depth1)      # the threads only split the batch


@pytest.mark.parametrize("fmt", [45, 50])
def test_the_order_rule_shows_on_the_tie_scene(fmt):
    """tie_scene(): per ray, the id the 4-wide rule reports differs from the binary oracle's, from "highest slot among equals" and from the
    reversed push order — and those three differ from each other: a kernel (or a model) that changed the rule would be seen on every ray."""
    blobs, rays = tie_scene()
    ref = orc.traverse(blobs, rays)
    model, highest, reverse = (wide_model(blobs, fmt, rays, order=k)[0] for k in (orc.WIDE_ORDER_PRODUCT, orc.WIDE_ORDER_HIGHEST_AMONG_EQUALS, orc.WIDE_ORDER_REVERSED_PUSH))
    answers = np.stack([r["triangle"] for r in (model, ref, highest, reverse)])
    assert (answers != MISS).all() and (answers // 4 == answers[0] // 4).all()      # every ray hits its group's four duplicates
    for r in (ref, highest, reverse):
        assert np.array_equal(r["t"].view(np.uint32), model["t"].view(np.uint32))     # ... at the same distance bit for bit
    for a in range(4):
        for b in range(a + 1, 4):
            same = np.nonzero(answers[a] == answers[b])[0]
            assert len(same) == 0, "rays %s do not tell %s from %s" % (same[:8], ("the rule", "the binary oracle", "highest slot among equals", "reversed push")[a],
                                                                       ("the rule", "the binary oracle", "highest slot among equals", "reversed push")[b])
    assert (answers[0] % 4 == 1).all()                                              # nearest first, lowest slot among equals, the others in slot order: 0 3 2 1
    assert_same_closest_hit(model, ref, "tie scene", max_ties=len(rays), arbiter=dict(_arbiter_of_lone_pairs(blobs), rays=rays))
