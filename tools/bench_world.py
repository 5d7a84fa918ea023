"""Instancing (racc_hip_world_*) against the flattened scene on the existing closest-hit path, in the same session.  1M diffuse rays each.

   (a) battlefield-synth, the library's default tree: a world of ONE identity instance against racc_hip_intersect_device on the same scene
       — the price of the two-level plain-HIP kernel against the assembly kernel.
   (b) N = 64 and N = 4,096 instances of a small mesh (battlefield-synth at grid=40, boxes=32, quads=100: 3,784 triangles) on a square
       grid, against the same triangles flattened into one scene (vertices carried into world space in double) and traced by
       racc_hip_intersect_device; device bytes and setup time (host build + upload, + create_world) of both.
   (c) World.update with unchanged transforms (wall time, median of 5).
   Timed: K launches between two synchronisations after a warm-up round, both paths in turn, ROUNDS times over; Mrays/s as median with
   min and max of the rounds.  The diffuse rays come from the flattened path's own primary hits, so both paths trace the same batch; the
   fraction of records on which they agree (instance * T + triangle, t to 1e-4 relative) is reported.  Prints one JSON line.

   python tools/bench_world.py [--rounds 5] [--k 10] [--sizes 64,4096]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import rayaccel_amd as ra
from rayaccel_amd import synth

COUNT = 1 << 20
IDENTITY = np.eye(3, 4, dtype=np.float32)


def diffuse(ctx, scene, sc):
    prim, _ = synth.primary_rays(sc["camera"], 1024, 1024)
    hits = ctx.intersect(scene, None, prim)
    return synth.diffuse_bounce_rays(sc, prim, hits, COUNT)


def measure(ctx, runs, rounds, k):
    rates = {name: [] for name in runs}
    for rnd in range(rounds + 1):      # round 0 is the warm-up
        for name, go in runs.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            go()
            dt = time.perf_counter() - t0
            if rnd:
                rates[name].append(k * COUNT / dt / 1e6)
    return {name: dict(median=round(float(np.median(v)), 1), min=round(float(min(v)), 1), max=round(float(max(v)), 1)) for name, v in rates.items()}


def compare(ctx, world, scene, rays, d_rays, tri_per_instance, k, rounds):
    """Both paths over the same device-resident batch; returns (rates, agreement)."""
    st = ctx.create_stream()
    d_w, d_i, d_f = ctx.alloc(COUNT * 16), ctx.alloc(COUNT * 4), [ctx.alloc(COUNT * 16) for _ in range(3)]

    def run_world():
        for _ in range(k):
            world.intersect_device(d_rays.ptr, d_w.ptr, d_i.ptr, COUNT, stream=st)
        ctx.stream_synchronize(st)

    def run_flat():
        for i in range(k):
            ctx.intersect_device(scene, None, d_rays.ptr, d_f[i % 3].ptr, COUNT, lane=ra.LANE_AUTO)
        ctx.wait(ra.LANE_AUTO)

    stat = measure(ctx, {"world": run_world, "flattened": run_flat}, rounds, k)
    w, inst, f = d_w.download(synth.RESULT_DTYPE, COUNT), d_i.download(np.uint32, COUNT), d_f[0].download(synth.RESULT_DTYPE, COUNT)
    hit = w["triangle"] != synth.INVALID_TRIANGLE
    ids = np.where(hit, inst.astype(np.uint64) * tri_per_instance + w["triangle"], synth.INVALID_TRIANGLE).astype(np.uint32)
    same = (ids == f["triangle"]) & (~hit | np.isclose(w["t"], f["t"], rtol=1e-4, atol=0))
    for b in [d_w, d_i] + d_f:
        b.free()
    ctx.destroy_stream(st)
    return stat, round(float(same.mean()), 5), round(float(hit.mean()), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--sizes", default="64,4096")
    args = ap.parse_args()
    ctx = ra.Context(device=0, chain_launches=2)      # every closest-hit launch stands alone, as every world launch does
    out = dict(tool="bench_world", rays=COUNT, k=args.k, rounds=args.rounds)

    # (a) one identity instance of battlefield-synth against the scene itself
    sc = synth.battlefield_synth()
    host = ra.HostScene(sc["vertices"], sc["indices"], quality=None)
    scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
    rays = diffuse(ctx, scene, sc)
    d_rays = ctx.alloc(rays.nbytes); d_rays.upload(rays)
    world = ctx.create_world([(IDENTITY, scene)])
    stat, agree, frac = compare(ctx, world, scene, rays, d_rays, len(sc["indices"]), args.k, args.rounds)
    out["one_identity_instance"] = dict(scene=sc["name"], mrays_per_s=stat, ratio=round(stat["world"]["median"] / stat["flattened"]["median"], 3), agreement=agree, hit_fraction=frac)
    world.destroy(); scene.destroy(); d_rays.free()

    # (b) N instances of a small mesh against the flattened triangles, (c) World.update
    mesh = synth.battlefield_synth(grid=40, boxes=32, quads=100)
    v64, idx = mesh["vertices"][:, :3].astype(np.float64), mesh["indices"]
    pitch = 200.0
    out["instances"] = {}
    for n in [int(s) for s in args.sizes.split(",")]:
        side = int(round(np.sqrt(n)))
        assert side * side == n
        transforms = np.tile(IDENTITY, (n, 1, 1))
        transforms[:, 0, 3] = pitch * (np.arange(n) % side); transforms[:, 2, 3] = pitch * (np.arange(n) // side)
        t0 = time.perf_counter()
        mesh_host = ra.HostScene(mesh["vertices"], mesh["indices"], quality=None)
        mesh_scene = ctx.upload_scene(mesh_host.nodes, mesh_host.pairs, mesh_host.remap)
        world = ctx.create_world([(m, mesh_scene) for m in transforms])
        setup_world = time.perf_counter() - t0
        flat_v = np.concatenate([v64 + m[:, 3].astype(np.float64) for m in transforms]).astype(np.float32)
        flat = dict(vertices=np.concatenate([flat_v, np.ones((len(flat_v), 1), np.float32)], 1),
                    indices=np.concatenate([idx + k * len(v64) for k in range(n)]).astype(np.uint32))
        t0 = time.perf_counter()
        flat_host = ra.HostScene(flat["vertices"], flat["indices"], quality=None)
        flat_scene = ctx.upload_scene(flat_host.nodes, flat_host.pairs, flat_host.remap)
        setup_flat = time.perf_counter() - t0
        w = pitch * side
        flat["camera"] = dict(mesh["camera"], origin=np.array([0.5 * w - 100.0, 0.35 * w + 60.0, -0.25 * w - 100.0], np.float32),
                              target=np.array([0.5 * w - 100.0, 0.0, 0.4 * w - 100.0], np.float32))
        rays = diffuse(ctx, flat_scene, flat)
        d_rays = ctx.alloc(rays.nbytes); d_rays.upload(rays)
        stat, agree, frac = compare(ctx, world, flat_scene, rays, d_rays, len(idx), args.k, args.rounds)
        updates = []
        for _ in range(5):
            t0 = time.perf_counter()
            world.update(transforms)
            updates.append((time.perf_counter() - t0) * 1e3)
        out["instances"][str(n)] = dict(triangles=int(n * len(idx)), mrays_per_s=stat, ratio=round(stat["world"]["median"] / stat["flattened"]["median"], 3),
                                        agreement=agree, hit_fraction=frac,
                                        device_bytes=dict(world=int(world.info["device_bytes"] + mesh_scene.info["device_bytes"]), flattened=int(flat_scene.info["device_bytes"])),
                                        setup_s=dict(world=round(setup_world, 3), flattened=round(setup_flat, 3)),
                                        update_ms=dict(median=round(float(np.median(updates)), 3), min=round(min(updates), 3), max=round(max(updates), 3)),
                                        world_info=world.info)
        print(json.dumps({str(n): out["instances"][str(n)]}), file=sys.stderr, flush=True)
        world.destroy(); mesh_scene.destroy(); flat_scene.destroy(); d_rays.free()
        del flat_host, flat, flat_v
    print(json.dumps(out), flush=True)
    ctx.destroy()


if __name__ == "__main__":
    main()
