"""Shared by the wide-refit tests (tests/test_wide_refit_host.py, tests/test_gpu_wide_refit.py): target meshes and the checks of the
rule of racc_host_scene_wide_nodes_refit (include/racc_hip.h) that need no second implementation of it."""
import numpy as np

from oracle import oracle as orc


def flattened(vertices):
    """Every vertex in the plane y = 0 (as -0.0 / +0.0 by turns): no frame has an extent on y."""
    v = np.array(vertices, np.float32, copy=True)
    v[:, 1] = 0.0
    v[::2, 1] = np.float32("-0.0")
    return v


def collapsed(vertices):
    """Every vertex at one point: no frame has an extent on any axis."""
    v = np.array(vertices, np.float32, copy=True)
    v[:, :3] = np.array([1.5, -0.0, 7.0], np.float32)
    return v


def overflowing(vertices):
    """The mesh with its lowest-x vertex at -3e38 and its highest-x vertex at +3e38: finite coordinates whose difference is not."""
    v = np.array(vertices, np.float32, copy=True)
    v[int(np.argmin(v[:, 0])), 0] = -3e38
    v[int(np.argmax(v[:, 0])), 0] = 3e38
    return v


def child_boxes(nodes):
    """-> (uint32 [2N, 6] the child boxes of a node blob as lo.x hi.x lo.y hi.y lo.z hi.z bit patterns, uint32 [2N] their references)."""
    lo = np.stack([nodes["leftMin"], nodes["rightMin"]], 1).reshape(-1, 3)
    hi = np.stack([nodes["leftMax"], nodes["rightMax"]], 1).reshape(-1, 3)
    below = lo < hi      # the collapse's per-axis ordering: (min, max) where min < max, else (max, min) — which only shows in the signs of two zeros
    box = np.stack([np.where(below, lo, hi), np.where(below, hi, lo)], 2).reshape(-1, 6)
    refs = np.stack([nodes["first"], nodes["last"]], 1).reshape(-1)
    return np.ascontiguousarray(box, np.float32).view(np.uint32), refs


def assert_wide_refit_rule(built45, now45, now50, now_nodes, disabled, what):
    """What the rule says of refitted records without restating it: references, `used` and the count are the built records'; a used
    format-45 box is bit-equal to a child box of the refitted blob — for a leaf slot, the box of THAT leaf —; a decoded format-50 box
    contains its format-45 box; and (no frame disabled) the format-50 records are the exact model's quantisation of the format-45 ones."""
    assert now45.shape == built45.shape and len(now50) == len(built45), what
    assert np.array_equal(now45[:, :4], built45[:, :4]) and np.array_equal(now50[:, :4], built45[:, :4]), what + ": references changed"
    assert np.array_equal(now45[:, 28:], built45[:, 28:]), what + ": `used` changed"
    boxes, refs = child_boxes(now_nodes)
    known = {b.tobytes() for b in boxes}
    leaf_box = {int(r): b.tobytes() for b, r in zip(boxes, refs) if not r & 0x80000000}
    planes = now45[:, 4:28].reshape(-1, 6, 4)
    for n in range(len(now45)):
        for i in range(4):
            key = planes[n, :, i].tobytes()
            if i >= now45[n, 28]:
                assert np.isposinf(planes[n, :, i].view(np.float32)).all(), "%s: unused slot %d of record %d" % (what, i, n)
            elif now45[n, i] & 0x80000000:
                assert key in known, "%s: slot %d of record %d holds a box that no child of the refitted blob has" % (what, i, n)
            else:
                assert key == leaf_box[int(now45[n, i])], "%s: slot %d of record %d does not hold its leaf's refitted box" % (what, i, n)
    d45, d50 = orc.decode_wide(now45, 45), orc.decode_wide(now50, 50)
    used = np.arange(4)[None, :] < now45[:, 28][:, None]
    off = np.isposinf(d50).all((1, 2))      # a disabled frame: every plane decodes to +inf
    assert int(off.sum()) == disabled, "%s: %d frames decode to +inf, %d are counted" % (what, off.sum(), disabled)
    for p in range(6):
        inside = d50[:, p, :] <= d45[:, p, :] if p % 2 == 0 else d50[:, p, :] >= d45[:, p, :]
        assert (inside | ~used | off[:, None]).all(), "%s: a decoded plane %d lies inside its box" % (what, p)
    if disabled == 0:
        rc, model = orc.quantise_wide(now45)
        # the model folds the origin with fminf, which leaves open WHICH zero a frame of +0.0 and -0.0 planes gets (no plane decodes differently
        # for it); the product's choice is pinned against quantiseWide itself (tests/test_wide_refit_host.py), so a zero origin's sign is set aside here
        same = model == now50
        same[:, 4:7] |= (model[:, 4:7].view(np.float32) == 0) & (now50[:, 4:7].view(np.float32) == 0)
        assert rc == 0 and same.all(), "%s: the format-50 records are not the model's quantisation of the format-45 records" % what
    else:
        q = now50[off]
        assert np.isposinf(q[:, 4:7].view(np.float32)).all() and (q[:, 7:10].view(np.float32) == np.finfo(np.float32).tiny).all(), what
        assert (q[:, 10::2] == 0xFFFFFFFF).all() and (q[:, 11::2] == 0).all(), what + ": a disabled frame's slots are not all unused"
