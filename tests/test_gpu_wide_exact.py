"""The 4-wide kernels against the EXACT model of their device format (oracle/racc_oracle_wide.c), bit for bit.

tests/helpers.py::assert_same_closest_hit says what a 4-wide kernel MAY differ from the binary oracle in (exact-distance ties, arbiter-confirmed
closer hits, aliases).  Here nothing may differ: each lane owns its node and its stack, so the sequence of box and pair tests of a ray is fixed
by the device records and the visiting rule — nearest hit child next, lowest slot among equals, the others pushed in slot order — and the model
walks the product's own records (racc_host_scene_wide_nodes; held to the model's byte for byte by tests/test_wide_format.py) by that rule.
kernel_variant 45, 46, 48, 49 are held to the format-45 model, 50, 51, 53 to the format-50 model, and with that every variant to the others of
its format — the plain C++ instantiations (46, 48, 51) arbitrate should the assembly and the model ever disagree; a default context with
wide_below routes its small launches to variant 45.  Host path and three back-to-back device-path batches each."""
import numpy as np
import pytest

import rayaccel_amd as ra
from oracle import oracle as orc
from rayaccel_amd import synth
from helpers import MISS, WIDE_FORMAT, assert_wide_exact, comb_scene, frame_scene, make_rays, tie_scene, wide_model

pytestmark = pytest.mark.gpu

CONFIGS = {
    "v9 4-wide (45)": (45, dict(kernel_variant=45)),
    "v9 4-wide C++ 6-entry (46)": (46, dict(kernel_variant=46)),
    "v9 4-wide C++ (48)": (48, dict(kernel_variant=48)),
    "v9 4-wide 7-entry (49)": (49, dict(kernel_variant=49)),
    "default kernel, wide_below routes small launches to 45": (45, dict(wide_below=1 << 20)),
    "v10 compressed 4-wide (50)": (50, dict(kernel_variant=50)),
    "v10 compressed 4-wide (50), every batch chained": (50, dict(kernel_variant=50, chain_min_rays=1)),
    "v10 compressed 4-wide C++ (51)": (51, dict(kernel_variant=51, chain_min_rays=1)),
    "v10 compressed 4-wide 7-entry (53)": (53, dict(kernel_variant=53, chain_min_rays=1)),
}


@pytest.fixture(scope="module")
def contexts():
    ctxs = {name: ra.Context(device=0, **opt) for name, (_, opt) in CONFIGS.items()}      # raises (never falls back) when the extension or the GPU is missing
    yield ctxs
    for c in ctxs.values():
        c.destroy()


def _device_path(ctx, scene, env, rays, batches=3):
    """Three back-to-back batches on the engine's own streams, then one wait (tests/test_gpu_edge_cases.py::_device_path)."""
    n = len(rays)
    d_r = ctx.alloc(n * 32)
    d_r.upload(rays)
    outs = [ctx.alloc(n * 16) for _ in range(batches)]
    for o in outs:
        ctx.intersect_device(scene, env, d_r.ptr, o.ptr, n, lane=ra.LANE_AUTO)
    ctx.wait(ra.LANE_AUTO)
    res = [o.download(orc.RESULT_DTYPE, n) for o in outs]
    for o in outs:
        o.free()
    d_r.free()
    return res


def run_exact(contexts, blobs, rays, what, env=None, spills=None):
    """Every wide configuration, host path and device path, against the model of its format.  Returns the two models' records."""
    model = {fmt: wide_model(blobs, fmt, rays, env=env) for fmt in (45, 50)}
    for name, ctx in contexts.items():
        variant = CONFIGS[name][0]
        fmt = WIDE_FORMAT[variant]
        want, depth, _, bound = model[fmt]
        scene = ctx.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
        if spills is not None and "kernel_variant" in CONFIGS[name][1]:
            assert (scene.info["spill_levels"] > 0) == (variant in spills), "%s | %s: spill_levels %d" % (what, name, scene.info["spill_levels"])
        e = ctx.create_environment(env) if env is not None else None
        results = [("host path", ctx.intersect(scene, e, rays))] + [("device path, batch %d" % k, r) for k, r in enumerate(_device_path(ctx, scene, e, rays))]
        for path, got in results:
            assert_wide_exact(got, want, "%s | %s | %s" % (what, name, path))
        scene.destroy()
        if e is not None:
            e.destroy()
    return model[45][0], model[50][0]


@pytest.mark.parametrize("tree", ["reference builder's tree", "library default tree"])
def test_small_scene_bit_exact(contexts, small_scene, small_host, small_default_host, tree):
    """Both small trees, the 256 x 256 primaries + 6000 random rays, with the probe image: every record of every wide kernel is the model's."""
    host = small_host if tree.startswith("reference") else small_default_host
    rays = np.concatenate([synth.primary_rays(small_scene["camera"], 256, 256)[0], synth.random_rays(6000, seed=3, ymax=30.0)])
    assert len(rays) == 256 * 256 + 6000
    a, b = run_exact(contexts, host.blobs(), rays, "small scene, " + tree, env=small_scene["env"])
    assert 0.3 < (a["triangle"] != MISS).mean() < 1.0 and np.array_equal(a["triangle"] != MISS, b["triangle"] != MISS)


def test_comb_spills_the_stack(contexts):
    """comb_scene(40): the model's deepest stack is 40 levels — beyond every variant's LDS levels (18 / 14 at most, 6 / 7 for 46, 49, 53):
    the spill levels in global memory carry the rule as well."""
    blobs = comb_scene(40)
    o = np.stack([np.linspace(-20, 20, 64), np.linspace(-15, 15, 64), np.full(64, -10.0)], 1)
    rays = np.concatenate([make_rays(o, [[0, 0, 1]] * 64), synth.random_rays(3000, seed=3, ymax=30.0)])
    depth = wide_model(blobs, 50, rays)[1]
    assert depth.max() == 40
    a, b = run_exact(contexts, blobs, rays, "comb", spills=(45, 46, 48, 49, 50, 51, 53))
    down = a["triangle"][:64]
    assert (down != MISS).sum() >= 32 and (down[down != MISS] == 40).all() and a.tobytes() == b.tobytes()      # the nearest of the 41 sheets, found last


def test_tie_scene_reports_what_the_rule_says(contexts):
    """tie_scene(): every ray hits four exact duplicates and the reported id tells the visiting order — the binary order, "highest slot among
    equals" and a reversed push order would each report another id on EVERY ray (tests/test_wide_format.py asserts that of the scene)."""
    blobs, rays = tie_scene()
    a, b = run_exact(contexts, blobs, rays, "tie scene")
    assert (a["triangle"] % 4 == 1).all() and a.tobytes() == b.tobytes()
    assert (orc.traverse(blobs, rays)["triangle"] != a["triangle"]).all()


@pytest.mark.parametrize("kind", ["flat_z", "point", "one_ulp", "huge"])
def test_degenerate_frames(contexts, kind):
    """Hand-made nodes whose quantisation frame has no extent on one axis or on all three (the compressed kernels ENTER the unused slots there:
    they hold the ref of a real leaf), extents of one ulp, coordinates of +-1e30."""
    blobs, rays = frame_scene(kind)
    a, b = run_exact(contexts, blobs, rays, "frame " + kind, env=synth.environment_synth(64, 32))
    assert (a["triangle"] != MISS).any() and (a["triangle"] == MISS).any()


@pytest.mark.parametrize("kind,code", [("overflow", -4), ("nonfinite", -1)])
def test_frames_the_compressed_format_refuses(contexts, kind, code):
    """Upload refuses what racc_host_scene_wide_nodes refuses, with the same code; the 128 B format holds both scenes and traces them exactly."""
    blobs, rays = frame_scene(kind)
    with pytest.raises(ra.RaccError) as e:
        contexts["v10 compressed 4-wide (50)"].upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
    assert e.value.code == code
    want = wide_model(blobs, 45, rays)[0]
    for name in ("v9 4-wide (45)", "v9 4-wide C++ (48)"):
        scene = contexts[name].upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
        assert_wide_exact(contexts[name].intersect(scene, None, rays), want, "frame %s | %s" % (kind, name))
        scene.destroy()
