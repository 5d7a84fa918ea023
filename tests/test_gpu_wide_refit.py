"""Refit of scenes uploaded for the 4-wide and compressed kernels — racc_hip_refit_create_wide, refitWideKernel
(rayaccel_amd/csrc/racc_refit_wide.inc).  The bar: after every refit the binary records equal racc_host_blobs_refit and the wide records
equal racc_host_scene_wide_nodes_refit BYTE FOR BYTE, and the wide kernels on the refitted scene are held, record for record, to the exact
model (oracle/racc_oracle_wide.c) walking those very records."""
import numpy as np
import pytest

import rayaccel_amd as ra
from oracle import oracle as orc
from rayaccel_amd import engine, synth
from helpers import MISS, assert_wide_exact
from refit_helpers import displaced, scene_size
from test_gpu_refit import _free_device_memory, assert_same_records
from wide_refit_helpers import collapsed, flattened, overflowing

pytestmark = pytest.mark.gpu

CONFIGS = {      # name -> (the format its scenes carry and its kernels walk, context options)
    "v9 4-wide (45)": (45, dict(kernel_variant=45)),
    "v9 4-wide C++ (48)": (45, dict(kernel_variant=48)),
    "v10 compressed (50)": (50, dict(kernel_variant=50)),
    "v10 compressed C++ (51)": (50, dict(kernel_variant=51)),
    "v10 compressed (50), every batch chained": (50, dict(kernel_variant=50, chain_min_rays=1)),
    "default kernel, wide_below routes small launches to 45": (45, dict(wide_below=1 << 20)),
}
TREES = ("quality 0", "default tree")


@pytest.fixture(scope="module")
def hosts(small_host, small_default_host):
    return {"quality 0": small_host, "default tree": small_default_host}


@pytest.fixture(scope="module")
def rays(small_scene):
    return np.concatenate([synth.random_rays(16384, 7), synth.primary_rays(small_scene["camera"], 128, 128)[0]])


@pytest.fixture(scope="module")
def wr(small_scene, hosts):
    """Every configuration's context with both trees uploaded, each with its wide refit handle."""
    sc, out = small_scene, {}
    for name, (fmt, opt) in CONFIGS.items():
        ctx = ra.Context(device=0, **opt)
        trees = {}
        for tree, host in hosts.items():
            scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
            trees[tree] = dict(scene=scene, refit=ctx.create_refit(scene, sc["indices"], len(sc["vertices"]), wide=True))
        out[name] = dict(ctx=ctx, fmt=fmt, trees=trees)
    yield out
    for c in out.values():
        for t in c["trees"].values():
            t["refit"].destroy()
            t["scene"].destroy()
        c["ctx"].destroy()


_expected = {}


def expected(hosts, sc, tree, key, vertices, rays=None):
    """The host side of one refit, computed once per (tree, target) and shared: the refitted blobs, both formats' records with their
    disabled counts and — given rays — the binary oracle's and both wide models' results."""
    e = _expected.get((tree, key))
    if e is None:
        host = hosts[tree]
        blobs = ra.host_refit(host.blobs(), vertices, sc["indices"])
        e = dict(blobs=blobs, wide={fmt: ra.host_wide_refit(host.nodes, blobs["nodes"], len(host.pairs), len(host.remap), fmt) for fmt in (45, 50)})
        _expected[(tree, key)] = e
    if rays is not None and "binary" not in e:
        e["binary"] = orc.traverse(e["blobs"], rays, threads=16)
        e["model"] = {fmt: orc.traverse_wide(e["wide"][fmt][0], fmt, e["blobs"], rays, threads=16)[0] for fmt in (45, 50)}
    return e


def assert_same_wide(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(1))[0]
    assert len(bad) == 0, "%s: %d of %d wide records differ, e.g. record %d: device %s, host %s" % (what, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]])


def check_records(c, t, e, what, disabled=0):
    assert_same_records(t["refit"].download(), e["blobs"], what)
    want, want_disabled = e["wide"][c["fmt"]]
    assert_same_wide(t["refit"].download_wide(c["fmt"]), want, what)
    assert want_disabled == disabled and t["refit"].check() == disabled, "%s: %d frames disabled on the device, %d on the host" % (what, t["refit"].check(), want_disabled)


def check_trace(c, t, e, rays, what):
    ctx, want = c["ctx"], e["model"][c["fmt"]]
    assert_wide_exact(ctx.intersect(t["scene"], None, rays), want, what + ", host path")
    n = len(rays)
    d_rays, outs = ctx.alloc(n * 32), [ctx.alloc(n * 16) for _ in range(3)]
    d_rays.upload(rays)
    for o in outs:
        ctx.intersect_device(t["scene"], None, d_rays.ptr, o.ptr, n, lane=ra.LANE_AUTO)
    ctx.wait(ra.LANE_AUTO)
    for k, o in enumerate(outs):
        assert_wide_exact(o.download(orc.RESULT_DTYPE, n), want, "%s, device batch %d" % (what, k))
    for b in [d_rays] + outs:
        b.free()
    occ = ctx.occluded(t["scene"], rays)
    assert np.array_equal(occ, (e["binary"]["triangle"] != MISS).astype(np.uint8)), what + ": occluded differs from 'the binary oracle reports a hit'"


# ------------------------------------------------------------------------------------------------------------ 1. download before any refit
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_download_before_any_refit_is_the_upload(small_scene, hosts, config):
    fmt, opt = CONFIGS[config]
    with ra.Context(device=0, **opt) as ctx:
        for tree, host in hosts.items():
            scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
            refit = ctx.create_refit(scene, small_scene["indices"], len(small_scene["vertices"]), wide=True)
            assert_same_wide(refit.download_wide(fmt), engine.wide_nodes(host.nodes, len(host.pairs), len(host.remap), fmt)[0], "%s | %s, download right after create" % (config, tree))
            assert_same_records(refit.download(), host.blobs(), "%s | %s, download right after create" % (config, tree))
            assert refit.check() == 0
            with pytest.raises(ra.RaccError) as e:      # the scene carries one format (wide_below on a default context: format 45)
                refit.download_wide(50 if fmt == 45 else 45)
            assert e.value.code == -1
            refit.destroy()
            scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 2. A -> B -> A
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_there_and_back(wr, small_scene, hosts, config):
    c, sc = wr[config], small_scene
    for tree in TREES:
        t, host = c["trees"][tree], hosts[tree]
        for key, v in (("B", displaced(sc["vertices"], 3.0)), ("A", sc["vertices"])):
            t["refit"].refit(v)
            check_records(c, t, expected(hosts, sc, tree, key, v), "%s | %s, refit to %s" % (config, tree, key))
        if tree == "quality 0":
            assert_same_records(t["refit"].download(), host.blobs(), config + " | quality 0, back at A: the original upload")
            assert_same_wide(t["refit"].download_wide(c["fmt"]), engine.wide_nodes(host.nodes, len(host.pairs), len(host.remap), c["fmt"])[0], config + " | quality 0, back at A: the original upload")


# ------------------------------------------------------------------------------------------------------------ 3. trace after refit
@pytest.mark.parametrize("displacement", ["a few units", "as large as the scene"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_trace_after_refit(wr, small_scene, hosts, rays, config, displacement):
    c, sc = wr[config], small_scene
    v = displaced(sc["vertices"], 3.0 if displacement == "a few units" else scene_size(sc["vertices"]), phase=0.5)
    for tree in TREES:
        t = c["trees"][tree]
        e = expected(hosts, sc, tree, "trace " + displacement, v, rays)
        for what, part in (("random rays", slice(0, 16384)), ("primary rays", slice(16384, None))):
            frac = (e["model"][c["fmt"]]["triangle"][part] != MISS).mean()
            print("%s | %s, %s, %s: the model's hit fraction is %.3f" % (config, tree, displacement, what, frac))
            assert 0.1 <= frac <= 0.9, "%s | %s, %s: the model's hit fraction on the %s is %.3f" % (config, tree, displacement, what, frac)
        t["refit"].refit(v)
        what = "%s | %s refitted, displacement %s" % (config, tree, displacement)
        check_records(c, t, e, what)
        check_trace(c, t, e, rays, what)
        t["refit"].refit(sc["vertices"])


# ------------------------------------------------------------------------------------------------------------ 4. refit_device
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_refit_device_on_a_callers_stream(wr, small_scene, hosts, config):
    c, sc = wr[config], small_scene
    ctx = c["ctx"]
    st, d_v = ctx.create_stream(), ctx.alloc(len(sc["vertices"]) * 16)
    for tree in TREES:
        t = c["trees"][tree]
        for key, v in (("B", displaced(sc["vertices"], 3.0)), ("A", sc["vertices"])):
            v = np.ascontiguousarray(v, np.float32)
            assert v.shape[1] == 4
            d_v.upload(v)
            t["refit"].refit_device(d_v.ptr, len(v), stream=st)
            ctx.stream_synchronize(st)
            check_records(c, t, expected(hosts, sc, tree, key, v), "%s | %s, refit_device to %s" % (config, tree, key))
    d_v.free()
    ctx.destroy_stream(st)


# ------------------------------------------------------------------------------------------------------------ 5. degenerate targets
@pytest.mark.parametrize("target", ["plane", "point"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_degenerate_targets(wr, small_scene, hosts, rays, config, target):
    c, sc = wr[config], small_scene
    v = flattened(sc["vertices"]) if target == "plane" else collapsed(sc["vertices"])
    for tree in TREES:
        t = c["trees"][tree]
        e = expected(hosts, sc, tree, target, v, rays)
        t["refit"].refit(v)
        what = "%s | %s, mesh flattened to a %s" % (config, tree, target)
        check_records(c, t, e, what)
        check_trace(c, t, e, rays, what)
        t["refit"].refit(sc["vertices"])


# ------------------------------------------------------------------------------------------------------------ 6. overflow
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_overflowing_extent(wr, small_scene, hosts, rays, config):
    """+-3e38: the blocking entry refuses it up front where the scene has a compressed copy (-4, every record as it was); refit_device does
    not validate, the refit disables the frames that cannot hold their boxes and counts them.  No trace on that state; then back to A."""
    c, sc = wr[config], small_scene
    ctx = c["ctx"]
    v = np.ascontiguousarray(overflowing(sc["vertices"]), np.float32)
    st, d_v = ctx.create_stream(), ctx.alloc(len(v) * 16)
    d_v.upload(v)
    for tree in TREES:
        t = c["trees"][tree]
        e = expected(hosts, sc, tree, "overflow", v)
        disabled = e["wide"][c["fmt"]][1]
        assert (disabled > 0) == (c["fmt"] == 50)
        if c["fmt"] == 50:
            before = (t["refit"].download(), t["refit"].download_wide(50))
            with pytest.raises(ra.RaccError) as err:
                t["refit"].refit(v)
            assert err.value.code == -4
            after = (t["refit"].download(), t["refit"].download_wide(50))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(before[0] + (before[1],), after[0] + (after[1],))), "the refused refit changed a record"
        t["refit"].refit_device(d_v.ptr, len(v), stream=st)
        ctx.stream_synchronize(st)
        check_records(c, t, e, "%s | %s, +-3e38 through refit_device" % (config, tree), disabled=disabled)
        t["refit"].refit(sc["vertices"])
        ea = expected(hosts, sc, tree, "A", sc["vertices"], rays)
        check_records(c, t, ea, "%s | %s, back at A after the overflow" % (config, tree))
        check_trace(c, t, ea, rays, "%s | %s, back at A after the overflow" % (config, tree))
    d_v.free()
    ctx.destroy_stream(st)


# ------------------------------------------------------------------------------------------------------------ 7. handles and memory
@pytest.mark.parametrize("config", ["v10 compressed (50)", "default kernel, wide_below routes small launches to 45"])
def test_one_wide_handle_per_scene(wr, small_scene, small_host, config):
    c, sc = wr[config], small_scene
    t = c["trees"]["default tree"]
    for wide in (True, False):      # a second wide handle; the plain create on a scene with a wide copy
        with pytest.raises(ra.RaccError) as e:
            c["ctx"].create_refit(t["scene"], sc["indices"], len(sc["vertices"]), wide=wide)
        assert e.value.code == -1 and "refit_create" in str(e.value)
    # ... and once the handle is gone the scene may have another
    host = small_host
    s2 = c["ctx"].upload_scene(host.nodes, host.pairs, host.remap)
    r1 = c["ctx"].create_refit(s2, sc["indices"], len(sc["vertices"]), wide=True)
    r1.destroy()
    r2 = c["ctx"].create_refit(s2, sc["indices"], len(sc["vertices"]), wide=True)
    r2.destroy()
    s2.destroy()


def test_a_scene_without_wide_copies_is_refused(small_scene, small_host):
    with ra.Context(device=0) as ctx:
        scene = ctx.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)
        with pytest.raises(ra.RaccError) as e:
            ctx.create_refit(scene, small_scene["indices"], len(small_scene["vertices"]), wide=True)
        assert e.value.code == -1 and "refit_create_wide" in str(e.value)
        plain = ctx.create_refit(scene, small_scene["indices"], len(small_scene["vertices"]))
        assert plain.check() == 0
        plain.destroy()
        scene.destroy()


def test_destroy_gives_the_memory_back():
    """As tests/test_gpu_refit.py::test_destroy_gives_the_memory_back, with the wide handle's 16 B per wide record on top: what create + one
    refit took must come back but for an eighth (allocation granularity)."""
    sc = synth.battlefield_synth(grid=300, boxes=32, quads=100)
    host = ra.HostScene(sc["vertices"], sc["indices"], quality=0)
    with ra.Context(device=0, kernel_variant=50) as ctx:
        scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
        before = _free_device_memory()
        refit = ctx.create_refit(scene, sc["indices"], len(sc["vertices"]), wide=True)
        refit.refit(sc["vertices"])
        assert refit.check() == 0
        held = before - _free_device_memory()
        refit.destroy()
        after = _free_device_memory()
        print("wide refit handle: %d bytes of device memory held, %d not returned by destroy" % (held, before - after))
        assert held >= 2 << 20, "the handle holds %d bytes: too little for this test to see" % held
        assert abs(before - after) <= held // 8
        scene.destroy()
